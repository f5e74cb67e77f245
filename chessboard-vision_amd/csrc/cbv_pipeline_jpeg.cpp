// The pipeline's Motion-JPEG ingest (cbv_pipeline_set_input_format(p, CBV_FMT_MJPEG)).  The host ring holds one stream per
// slot, `lengths` says how many bytes of each slot are used.  cbv_pipeline_submit parses the slots' headers out of the
// pinned ring (a few hundred bytes each; the entropy data is never read on the host), copies the used bytes and enqueues the
// decode on the copy stream behind the copy, `depth` frames at a time through one set of scratch buffers
// (cbv_pipeline_set_jpeg_depth).  Which buffers there are is the plan's (frame_plan.h, cbv_pipeline_frames.cpp).
#include "cbv_pipeline.h"

// the samplings in the order in which the planes modes admit them: CBV_JPEG_PLANES_<X> admits those up to X
static int jpeg_sampling(const JpegDesc& D) { return D.ncomp == 1 ? CBV_JPEG_PLANES_GRAY : D.hs == 1 ? CBV_JPEG_PLANES_444 : D.vs == 1 ? CBV_JPEG_PLANES_422 : CBV_JPEG_PLANES_420; }
static const char* jpeg_sampling_name(int s)
{
    return s == CBV_JPEG_PLANES_GRAY ? "gray" : s == CBV_JPEG_PLANES_420 ? "4:2:0" : s == CBV_JPEG_PLANES_422 ? "4:2:2" : s == CBV_JPEG_PLANES_444 ? "4:4:4" : "off";
}

WarpSrc pipeline_jpeg_warp_src(const Pipe& P, int slot0, const ProfileTabs* ptabs, int np, size_t dst_profile_stride)
{
    return warp_src_jpeg(P.plane_ring + P.plan.plane_slot * slot0, P.plan.plane_slot, P.jpeg->d_wdesc + slot0, P.g, ptabs, np, dst_profile_stride);
}

int pipeline_jpeg_slot_bgr(Pipe& P, int slot, u8* bgr)
{
    JpegBatch B;
    memset(&B, 0, sizeof(B));
    B.descs = P.jpeg->d_wdesc + slot;
    B.planes = P.plane_ring + P.plan.plane_slot * slot;
    B.plane_stride = P.plan.plane_slot;
    B.bgr = bgr;
    B.bgr_stride = P.g.stride;
    B.bgr_frame_stride = P.g.frame_stride;
    B.nframes = 1;
    return launch_jpeg_color(P.ctx, B, P.w, P.h);
}

// a stream's header against the pipeline: it parses, the frame has the pipeline's size, and the plane ring's slots hold its
// sampling; name_slot: the first two messages name the slot too
static int jpeg_checked_header(Pipe& P, const char* who, int slot, bool name_slot, const u8* data, size_t n, JpegDesc* D, JpegTables* T)
{
    cbv_ctx* ctx = P.ctx;
    char msg[200], at[24] = "";
    if (name_slot) snprintf(at, sizeof(at), "slot %d: ", slot);
    const int rc = jpeg_parse_header(data, n, D, T, msg, sizeof(msg));
    if (rc) return cbv_fail(ctx, rc, "%s: %s%s", who, at, msg);
    if (D->w != P.w || D->h != P.h) return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "%s: %sa %d x %d frame, the pipeline's are %d x %d", who, at, D->w, D->h, P.w, P.h);
    if (P.plan.plane_mode != CBV_JPEG_PLANES_OFF && jpeg_sampling(*D) > P.plan.plane_mode)
        return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "%s: slot %d: a %s frame, the plane ring's slots hold up to %s (cbv_pipeline_set_jpeg_planes)", who, slot,
                        jpeg_sampling_name(jpeg_sampling(*D)), jpeg_sampling_name(P.plan.plane_mode));
    return CBV_OK;
}

// cbv_pipeline_submit with the Motion-JPEG format: called under the context's lock with the copy stream made; read_ev = what the
// writes into the frame ring wait for (may be null)
int pipeline_jpeg_submit(Pipe& P, int slot0, int count, hipEvent_t read_ev)
{
    cbv_ctx* ctx = P.ctx;
    JpegState* J = P.jpeg;
    const FramePlan& pl = P.plan;
    const char* who = "cbv_pipeline_submit";
    const size_t sb = pl.slot_bytes;
    const bool to_ring = pl.source == FRAMES_PLANES; // the decode stops at the slots' planes
    if (J->nsets == JpegState::NSETS) { // the cache is full: start again once nothing reads it
        CBV_HIP(ctx, hipStreamSynchronize(P.copy_stream));
        J->nsets = 0;
    }
    const int sets_before = J->nsets;
    // 1. every header, and a table set for it (one of the cache, or a new one), before anything is enqueued
    for (int s = slot0; s < slot0 + count; s++) {
        const u32 len = J->h_lengths[s];
        JpegTables T;
        int rc = CBV_OK;
        if (len == 0 || len > sb) rc = cbv_fail(ctx, CBV_ERR_ARG, "%s: slot %d: length %u, a slot holds %zu bytes", who, s, len, sb);
        else rc = jpeg_checked_header(P, who, s, true, P.host_ring + sb * s, len, &J->h_desc[s], &T);
        int k = 0;
        while (!rc && k < J->nsets && memcmp(&J->h_tabs[k], &T, sizeof(T))) k++;
        if (!rc && k == JpegState::NSETS) rc = cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "%s: slot %d: more than %d different table sets in flight", who, s, k);
        if (rc) {
            J->nsets = sets_before;
            return rc;
        }
        if (k == J->nsets) memcpy(&J->h_tabs[J->nsets++], &T, sizeof(T));
        J->h_desc[s].table_set = k;
    }
    for (int c0 = 0; c0 < count; c0 += pl.depth) {
        const int s = slot0 + c0, cf = std::min<int>(pl.depth, count - c0);
        u32 acc = 0;
        for (int i = 0; i < cf; i++) {
            J->h_ioff[2 * s + i] = acc;
            acc += (u32)J->h_desc[s + i].nint;
        }
        J->h_ioff[2 * s + cf] = acc;
    }
    // 2. the used bytes of every slot, the descriptors, the new table sets
    for (int s = slot0; s < slot0 + count; s++) {
        const size_t bytes = std::min(sb, ((size_t)J->h_lengths[s] + 255) & ~(size_t)255);
        CBV_HIP(ctx, hipMemcpyAsync(P.raw_ring + sb * s, P.host_ring + sb * s, bytes, hipMemcpyHostToDevice, P.copy_stream));
    }
    CBV_HIP(ctx, hipMemcpyAsync(J->d_desc + slot0, J->h_desc + slot0, (size_t)count * sizeof(JpegDesc), hipMemcpyHostToDevice, P.copy_stream));
    CBV_HIP(ctx, hipMemcpyAsync(J->d_ioff + 2 * slot0, J->h_ioff + 2 * slot0, (size_t)2 * count * sizeof(u32), hipMemcpyHostToDevice, P.copy_stream));
    if (J->nsets > sets_before)
        CBV_HIP(ctx, hipMemcpyAsync(J->d_tabs + sets_before, J->h_tabs + sets_before, (size_t)(J->nsets - sets_before) * sizeof(JpegTables),
                                    hipMemcpyHostToDevice, P.copy_stream));
    if (read_ev) CBV_HIP(ctx, hipStreamWaitEvent(P.copy_stream, read_ev, 0));
    // The runs in flight read the plane ring and the warp's descriptors of their slots: both change only from here on, behind
    // the wait.  (d_desc above is read by the decode alone, whose launches of these slots are in stream order.)
    if (to_ring)
        CBV_HIP(ctx, hipMemcpyAsync(J->d_wdesc + slot0, J->d_desc + slot0, (size_t)count * sizeof(JpegDesc), hipMemcpyDeviceToDevice, P.copy_stream));
    // 3. the decode, a chunk of frames at a time through the one set of scratch buffers (stream order keeps them apart)
    hipStream_t caller = ctx->stream;
    ctx->stream = P.copy_stream;
    int rc = CBV_OK;
    for (int c0 = 0; c0 < count && !rc; c0 += pl.depth) {
        const int s = slot0 + c0, cf = std::min<int>(pl.depth, count - c0);
        JpegBatch B;
        B.data = P.raw_ring + sb * s;
        B.data_stride = sb;
        B.descs = J->d_desc + s;
        B.tables = J->d_tabs;
        B.ioff = J->d_ioff + 2 * s;
        B.mpos = P.jsc.mpos;
        B.nfound = J->d_nfound + s;
        B.status = J->d_status + s;
        B.coef = P.jsc.coef;
        B.coef_stride = pl.frame_elems;
        B.planes = to_ring ? P.plane_ring + pl.plane_slot * s : P.jsc.planes;
        B.plane_stride = to_ring ? pl.plane_slot : pl.frame_elems;
        B.bgr = to_ring ? nullptr : P.frames + P.g.frame_stride * s;
        B.bgr_stride = P.g.stride;
        B.bgr_frame_stride = P.g.frame_stride;
        B.nframes = cf;
        B.piece_bytes = pl.piece_bytes;
        B.pieces = P.jsc.pieces;
        B.piece_stride = pl.piece_words;
        B.piece_cap = pl.piece_cap;
        B.segments = pl.segments;
        B.segs = P.jsc.segs;
        B.seg_stride = pl.seg_words;
        B.stats = J->d_stats + 3 * (size_t)s;
        int any_dri = 0, any_pieces = 0;
        u32 max_blocks = 0;
        for (int i = 0; i < cf; i++) {
            any_dri |= J->h_desc[s + i].dri != 0;
            any_pieces |= pl.piece_bytes && (pl.segments || !J->h_desc[s + i].dri);
            max_blocks = std::max(max_blocks, J->h_desc[s + i].plane_total / 64u);
        }
        rc = launch_jpeg_decode(ctx, B, J->h_ioff[2 * s + cf], any_dri, any_pieces, max_blocks, P.w, P.h);
    }
    ctx->stream = caller;
    return rc;
}

extern "C" uint32_t* cbv_pipeline_host_jpeg_lengths(cbv_pipeline* p)
{
    if (!p || attached(p) || !p->pipe->jpeg) return nullptr;
    return p->pipe->jpeg->h_lengths;
}

// cbv_pipeline_jpeg_status and cbv_pipeline_jpeg_stats: `words` u32 per slot of `dev`, behind the submitted decodes
static int jpeg_slot_words(cbv_pipeline* p, const char* who, int slot0, int count, void* out, int words, bool stats)
{
    int rc;
    Pipe* owner = frames_owner(p, who, "the pipeline is null", &rc);
    if (!owner) return rc;
    Pipe& P = *owner;
    cbv_ctx* ctx = P.ctx;
    if (!out || slot0 < 0 || count <= 0 || slot0 + count > P.max_frames) return cbv_fail(ctx, CBV_ERR_ARG, "%s: bad slot range", who);
    if (!P.jpeg) return cbv_fail(ctx, CBV_ERR_STATE, "%s: no Motion-JPEG frame was ever given to the pipeline", who);
    CBV_ENTER(ctx);
    if (P.copy_stream) CBV_HIP(ctx, hipStreamSynchronize(P.copy_stream));
    const u32* dev = stats ? P.jpeg->d_stats : (const u32*)P.jpeg->d_status;
    CBV_HIP(ctx, hipMemcpy(out, dev + (size_t)words * slot0, (size_t)count * words * sizeof(u32), hipMemcpyDeviceToHost));
    return CBV_OK;
}

extern "C" int cbv_pipeline_jpeg_status(cbv_pipeline* p, int slot0, int count, int32_t* out)
{
    return jpeg_slot_words(p, "cbv_pipeline_jpeg_status", slot0, count, out, 1, false);
}

extern "C" int cbv_pipeline_jpeg_stats(cbv_pipeline* p, int slot0, int count, cbv_jpeg_decode_stats* out)
{
    static_assert(sizeof(cbv_jpeg_decode_stats) == 3 * sizeof(u32), "cbv_jpeg_decode_stats is three words");
    return jpeg_slot_words(p, "cbv_pipeline_jpeg_stats", slot0, count, out, 3, true);
}

extern "C" int cbv_pipeline_set_jpeg_entropy(cbv_pipeline* p, int mode, uint32_t piece_bytes)
{
    const char* who = "cbv_pipeline_set_jpeg_entropy";
    int rc;
    Pipe* P = frames_owner(p, who, "the pipeline is null", &rc);
    if (!P) return rc;
    CBV_ENTER(P->ctx);
    FrameSettings next = P->fs;
    next.entropy = mode;
    next.piece_bytes = piece_bytes;
    return pipeline_set_frames(*P, next, who, false); // (refuses an unknown mode and a bad piece size)
}

extern "C" int cbv_pipeline_set_jpeg_depth(cbv_pipeline* p, int frames)
{
    const char* who = "cbv_pipeline_set_jpeg_depth";
    int rc;
    Pipe* P = frames_owner(p, who, "the pipeline is null", &rc);
    if (!P) return rc;
    if (frames < 1 || frames > CBV_JPEG_DEPTH_MAX) return cbv_fail(P->ctx, CBV_ERR_ARG, "%s: %d frames per launch (1 to %d)", who, frames, CBV_JPEG_DEPTH_MAX);
    CBV_ENTER(P->ctx);
    FrameSettings next = P->fs;
    next.depth = frames;
    return pipeline_set_frames(*P, next, who, false);
}

extern "C" int cbv_pipeline_jpeg_depth(cbv_pipeline* p)
{
    int rc;
    Pipe* P = frames_owner(p, "cbv_pipeline_jpeg_depth", "the pipeline is null", &rc);
    return P ? P->fs.depth : rc;
}

extern "C" int cbv_pipeline_set_jpeg_slot_bytes(cbv_pipeline* p, size_t bytes)
{
    const char* who = "cbv_pipeline_set_jpeg_slot_bytes";
    int rc;
    Pipe* P = frames_owner(p, who, "the pipeline is null", &rc);
    if (!P) return rc;
    if (bytes < 256 || bytes > ((size_t)1 << 30)) return cbv_fail(P->ctx, CBV_ERR_ARG, "%s: %zu bytes", who, bytes);
    CBV_ENTER(P->ctx);
    FrameSettings next = P->fs;
    next.jpeg_slot_bytes = (bytes + 255) & ~(size_t)255;
    return pipeline_set_frames(*P, next, who, next.fmt == CBV_FMT_MJPEG); // frees both ingest rings, as a format change does
}

extern "C" int cbv_pipeline_set_jpeg_planes(cbv_pipeline* p, int mode)
{
    const char* who = "cbv_pipeline_set_jpeg_planes";
    int rc;
    Pipe* P = frames_owner(p, who, "the pipeline is null", &rc);
    if (!P) return rc;
    if (!jpeg_planes_mode_ok(mode)) return cbv_fail(P->ctx, CBV_ERR_ARG, "%s: mode %d", who, mode);
    CBV_ENTER(P->ctx);
    FrameSettings next = P->fs;
    next.planes = mode;
    // without the format the mode is only stored (the ring comes with the format); with it, a new mode is a format change
    return pipeline_set_frames(*P, next, who, next.fmt == CBV_FMT_MJPEG && mode != P->fs.planes);
}

extern "C" int cbv_pipeline_jpeg_planes(cbv_pipeline* p)
{
    int rc;
    Pipe* P = frames_owner(p, "cbv_pipeline_jpeg_planes", "the pipeline is null", &rc);
    return P ? P->fs.planes : rc;
}

extern "C" int cbv_pipeline_upload_jpeg(cbv_pipeline* p, int slot, const uint8_t* data, size_t n)
{
    const char* who = "cbv_pipeline_upload_jpeg";
    int rc;
    Pipe* owner = frames_owner(p, who, "the pipeline is null", &rc);
    if (!owner) return rc;
    Pipe& P = *owner;
    cbv_ctx* ctx = P.ctx;
    if (!data || slot < 0 || slot >= P.max_frames) return cbv_fail(ctx, CBV_ERR_ARG, "%s: bad arguments", who);
    JpegDesc D;
    JpegTables T;
    RC(jpeg_checked_header(P, who, slot, false, data, n, &D, &T));
    CBV_ENTER(ctx);
    if (P.plan.source == FRAMES_RAW)
        return cbv_fail(ctx, CBV_ERR_STATE, "%s: the pipeline's frames are its raw ring (raw mode); it has no BGR frames to decode into", who);
    const bool to_ring = P.plan.source == FRAMES_PLANES; // the decode stops at the slot's planes
    RC(pipeline_jpeg_ensure(P));
    RC(join_scan(P)); // lanes and scan of the last run
    if (P.copy_stream) CBV_HIP(ctx, hipStreamSynchronize(P.copy_stream)); // a submitted decode of this slot lands first
    JpegBatch B;
    u8* bgr = to_ring ? nullptr : P.frames + P.g.frame_stride * slot;
    RC(jpeg_single_dev(ctx, data, n, D, T, P.plan.piece_bytes, P.plan.segments, bgr, P.g, &B, to_ring ? P.plane_ring + P.plan.plane_slot * slot : nullptr, to_ring));
    if (to_ring) // the slot's descriptor for the warp (the runs are joined)
        CBV_HIP(ctx, hipMemcpyAsync(P.jpeg->d_wdesc + slot, B.descs, sizeof(JpegDesc), hipMemcpyDeviceToDevice, ctx->stream));
    CBV_HIP(ctx, hipMemcpyAsync(P.jpeg->d_status + slot, B.status, sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
    CBV_HIP(ctx, hipMemcpyAsync(P.jpeg->d_stats + 3 * (size_t)slot, B.stats, 3 * sizeof(u32), hipMemcpyDeviceToDevice, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}
