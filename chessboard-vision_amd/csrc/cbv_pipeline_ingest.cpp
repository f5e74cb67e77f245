// Frame ingest of the device-resident pipeline: upload, the pinned host ring and the device ring of raw (YUV) frames,
// submit on the copy stream, and the synthetic frames.
#include "cbv_pipeline.h"

// where the raw ring or the plane ring is the frames (FramePlan::raw) there are no BGR frames to write
static const char* const kRawModeMsg = "the pipeline runs without enhancement on a YUV or Bayer input format (raw mode): its frames are the raw "
                                       "ring, written by cbv_pipeline_upload_raw or cbv_pipeline_submit in that format";
static const char* const kJpegRawModeMsg = "the pipeline runs without enhancement on Motion-JPEG input in planes mode (raw mode): its frames are "
                                           "the decoded planes, written by cbv_pipeline_upload_jpeg or cbv_pipeline_submit";
static const char* raw_mode_msg(const Pipe& P) { return P.plan.source == FRAMES_PLANES ? kJpegRawModeMsg : kRawModeMsg; }

// the planes of slot `slot` of the device ring of raw frames
RawPlanes slot_planes(const Pipe& P, int slot)
{
    return tight_raw_planes(P.fs.fmt, P.w, P.h, P.raw_ring + P.plan.slot_bytes * slot);
}

WarpSrc pipeline_raw_warp_src(const Pipe& P, int slot0, const ProfileTabs* ptabs, int np, size_t dst_profile_stride)
{
    if (P.plan.source == FRAMES_PLANES) return pipeline_jpeg_warp_src(P, slot0, ptabs, np, dst_profile_stride);
    const RawGeom rg = tight_raw_geom(P.fs.fmt, P.w, P.h);
    if (raw_fmt_bayer(P.fs.fmt) && bayer_deep(P.fs.fmt, P.bdeep)) return warp_src_raw_deep(slot_planes(P, slot0), rg, P.g, P.bdeep, ptabs, np, dst_profile_stride);
    return ptabs ? warp_src_raw_profile(slot_planes(P, slot0), rg, P.g, ptabs, np, dst_profile_stride, P.fs.cs) : warp_src_raw(slot_planes(P, slot0), rg, P.g, P.fs.cs);
}

extern "C" int cbv_pipeline_upload(cbv_pipeline* p, int slot, const uint8_t* bgr, int stride)
{
    int rc;
    Pipe* owner = frames_owner(p, "cbv_pipeline_upload", nullptr, &rc);
    if (!owner) return rc;
    Pipe& P = *owner;
    cbv_ctx* ctx = P.ctx;
    if (!bgr || slot < 0 || slot >= P.max_frames || stride < P.w * 3) return CBV_ERR_ARG;
    CBV_ENTER(ctx);
    if (P.plan.raw()) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_upload: %s", raw_mode_msg(P));
    RC(join_scan(P)); // lanes and scan of the last run
    RC(rows_h2d(ctx, P.frames + P.g.frame_stride * slot, bgr, stride, P.w * 3, P.h));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

extern "C" int cbv_pipeline_upload_raw(cbv_pipeline* p, int slot, const cbv_raw_frame* raw)
{
    int rc;
    Pipe* owner = frames_owner(p, "cbv_pipeline_upload_raw", "bad arguments", &rc);
    if (!owner) return rc;
    Pipe& P = *owner;
    cbv_ctx* ctx = P.ctx;
    if (!raw || slot < 0 || slot >= P.max_frames) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_upload_raw: bad arguments");
    if (raw->fmt == CBV_FMT_BGR) return cbv_pipeline_upload(p, slot, raw->plane0, raw->stride0);
    RC(check_raw_format(ctx, raw->fmt, P.w, P.h, "cbv_pipeline_upload_raw"));
    const int fmt = raw_fmt_layout(raw->fmt), cs = raw_fmt_cs(raw->fmt);
    CBV_ENTER(ctx);
    RC(join_scan(P)); // lanes and scan of the last run
    if (P.plan.raw()) { // the frame as it is into its slot of the raw ring, rows packed
        if (P.plan.source == FRAMES_PLANES) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_upload_raw: format %d, but %s", raw->fmt, kJpegRawModeMsg);
        if (fmt != P.fs.fmt || cs != P.fs.cs) // (the whole id: an NV12 / BT.709 ring refuses an NV12 / BT.601 frame)
            return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_upload_raw: format %d, but %s (format %d)", raw->fmt, kRawModeMsg, P.fs.fmt | P.fs.cs * CBV_CS_FULL);
        const u8* planes[3];
        int strides[3];
        raw_frame_planes(raw, planes, strides);
        RC(check_raw_planes(ctx, fmt, P.w, planes, strides, "cbv_pipeline_upload_raw"));
        RC(pipeline_raw_ring(P));
        // the raw ring is the only frame store here: a copy of this slot that cbv_pipeline_submit left in flight lands first
        if (P.copy_stream) CBV_HIP(ctx, hipStreamSynchronize(P.copy_stream));
        const RawPlanes dst = slot_planes(P, slot);
        for (int i = 0; i < raw_fmt_planes(fmt); i++)
            RC(rows_h2d(ctx, (u8*)dst.p[i], planes[i], strides[i], raw_plane_wbytes(fmt, P.w, i), raw_plane_rows(fmt, P.h, i)));
        CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return CBV_OK;
    }
    // (a mosaic in the pipeline's own format goes through the pipeline's tables, any other Bayer frame through its format's default)
    RC(raw_h2d_convert(ctx, raw, P.w, P.h, P.frames + P.g.frame_stride * slot, P.g, "cbv_pipeline_upload_raw", fmt == P.fs.fmt ? &P.bdeep : nullptr));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}


extern "C" size_t cbv_pipeline_host_slot_bytes(cbv_pipeline* p)
{
    if (!p || attached(p)) return 0;
    std::lock_guard<std::recursive_mutex> lock(p->pipe->ctx->mu);
    return p->pipe->plan.slot_bytes;
}

extern "C" int cbv_pipeline_set_input_format(cbv_pipeline* p, int fmt)
{
    const char* who = "cbv_pipeline_set_input_format";
    int rc;
    Pipe* P = frames_owner(p, who, "the pipeline is null", &rc);
    if (!P) return rc;
    RC(check_fmt_cs(P->ctx, fmt, who)); // (colour-space bits on BGR or Motion-JPEG)
    if (fmt != CBV_FMT_BGR && fmt != CBV_FMT_MJPEG) RC(check_raw_format(P->ctx, fmt, P->w, P->h, who));
    CBV_ENTER(P->ctx);
    FrameSettings next = P->fs;
    next.fmt = raw_fmt_layout(fmt);
    next.cs = raw_fmt_cs(fmt);
    RC(pipeline_set_frames(*P, next, who, true)); // both ingest rings go, whatever the format was
    // the tables are the new format's default (pipeline_set_frames has waited for everything that read the old ones)
    P->bdeep = BayerDeep();
    if (raw_fmt_bayer(next.fmt)) RC(bayer_tables_upload(P->ctx, &P->d_btab, next.fmt, nullptr, 0, &P->bdeep, who));
    return CBV_OK;
}

extern "C" int cbv_pipeline_set_bayer_tables(cbv_pipeline* p, const uint8_t* tables, int bits)
{
    const char* who = "cbv_pipeline_set_bayer_tables";
    int rc;
    Pipe* owner = frames_owner(p, who, "the pipeline is null", &rc);
    if (!owner) return rc;
    Pipe& P = *owner;
    cbv_ctx* ctx = P.ctx;
    CBV_ENTER(ctx);
    if (!raw_fmt_bayer(P.fs.fmt))
        return cbv_fail(ctx, CBV_ERR_STATE, "%s: the input format is %d (%s), not a Bayer format", who, P.fs.fmt, raw_fmt_name(P.fs.fmt));
    if (tables && !bayer_bits_ok(P.fs.fmt, bits))
        return cbv_fail(ctx, CBV_ERR_ARG, "%s: tables of %d bits do not go with format %d (%s)", who, bits, P.fs.fmt, raw_fmt_name(P.fs.fmt));
    // the runs in flight and the conversions of the copy stream read the tables that change here
    RC(join_scan(P));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (P.copy_stream) CBV_HIP(ctx, hipStreamSynchronize(P.copy_stream));
    BayerDeep next;
    RC(bayer_tables_upload(ctx, &P.d_btab, P.fs.fmt, tables, bits, &next, who));
    P.bdeep = next;
    return CBV_OK;
}

extern "C" uint8_t* cbv_pipeline_host_ring(cbv_pipeline* p)
{
    if (!p) return nullptr;
    std::lock_guard<std::recursive_mutex> lock(p->pipe->ctx->mu);
    int rc;
    Pipe* P = frames_owner(p, "cbv_pipeline_host_ring", nullptr, &rc);
    if (!P || hipSetDevice(P->ctx->device) != hipSuccess || pipeline_host_ring(*P) != CBV_OK) return nullptr;
    return P->host_ring;
}

extern "C" int cbv_pipeline_submit(cbv_pipeline* p, int slot0, int count)
{
    int rc;
    Pipe* owner = frames_owner(p, "cbv_pipeline_submit", nullptr, &rc);
    if (!owner) return rc;
    Pipe& P = *owner;
    cbv_ctx* ctx = P.ctx;
    if (slot0 < 0 || count <= 0 || slot0 + count > P.max_frames) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_submit: bad slot range");
    if (!P.host_ring) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_submit: cbv_pipeline_host_ring() was never called");
    CBV_ENTER(ctx);
    if (!P.copy_stream) RC(ctx_worker_stream(ctx, &ctx->copy_stream, &P.copy_stream));
    // do not overwrite device slots a run that is still in flight reads: ANY such run, not only the last one
    retire_runs(P);
    Pipe::RunRec* reader = newest_run(P, slot0, count, 0);
    // the event of the newest run that reads these slots (null: none does); where each format waits for it is its own
    hipEvent_t read_ev = reader ? (reader->one_event ? reader->scan_ev : reader->lanes_ev) : nullptr;
    if (P.fs.fmt == CBV_FMT_MJPEG) {
        RC(pipeline_jpeg_submit(P, slot0, count, read_ev));
    } else if (P.fs.fmt == CBV_FMT_BGR) {
        if (read_ev) CBV_HIP(ctx, hipStreamWaitEvent(P.copy_stream, read_ev, 0));
        CBV_HIP(ctx, hipMemcpyAsync(P.frames + P.g.frame_stride * slot0, P.host_ring + P.g.frame_stride * slot0,
                                    P.g.frame_stride * count, hipMemcpyHostToDevice, P.copy_stream));
    } else {
        // Raw slots to the device raw ring, then their conversion into the frame ring, both on the copy stream: stream order
        // is the copy -> conversion dependency and keeps a later copy off raw slots an earlier conversion still reads, and
        // the one event below stands for both.  Only the conversion writes the frames the runs in flight read, so the copy
        // itself does not wait for them.
        // In raw mode the copy is all: the runs read the raw ring itself, so it is the copy that waits for them.
        const RawGeom rg = tight_raw_geom(P.fs.fmt, P.w, P.h);
        u8* raw = P.raw_ring + rg.frame_stride * slot0;
        if (read_ev && P.plan.raw()) { // (the wait goes in front of the copy)
            CBV_HIP(ctx, hipStreamWaitEvent(P.copy_stream, read_ev, 0));
            read_ev = nullptr;
        }
        CBV_HIP(ctx, hipMemcpyAsync(raw, P.host_ring + rg.frame_stride * slot0, rg.frame_stride * count, hipMemcpyHostToDevice, P.copy_stream));
        if (read_ev) CBV_HIP(ctx, hipStreamWaitEvent(P.copy_stream, read_ev, 0));
        hipStream_t caller = ctx->stream;
        ctx->stream = P.copy_stream;
        const int rc_ingest = P.plan.raw() ? CBV_OK : launch_ingest_any(ctx, slot_planes(P, slot0), rg, P.frames + P.g.frame_stride * slot0, P.g, count, P.fs.cs, P.bdeep);
        ctx->stream = caller;
        RC(rc_ingest);
    }
    Pipe::CopyRec* rec = nullptr;
    for (auto& c : P.copies)
        if (!c.pending) {
            rec = &c;
            break;
        }
    if (!rec) {
        Pipe::CopyRec c{0, 0, nullptr, false};
        CBV_HIP(ctx, hipEventCreateWithFlags(&c.ev, hipEventDisableTiming));
        P.copies.push_back(c);
        rec = &P.copies.back();
    }
    rec->s0 = slot0;
    rec->cnt = count;
    rec->pending = true;
    CBV_HIP(ctx, hipEventRecord(rec->ev, P.copy_stream));
    return CBV_OK;
}

extern "C" int cbv_pipeline_wait_submitted(cbv_pipeline* p)
{
    if (!p) return CBV_ERR_ARG;
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    CBV_ENTER(ctx);
    if (P.copy_stream) CBV_HIP(ctx, hipStreamSynchronize(P.copy_stream));
    return CBV_OK;
}

extern "C" int cbv_pipeline_synth(cbv_pipeline* p, int slot0, int count, const uint64_t* seeds, const double* Hinv9,
                                  const uint8_t* boards, const cbv_scene* scene)
{
    int rc;
    Pipe* owner = frames_owner(p, "cbv_pipeline_synth", nullptr, &rc);
    if (!owner) return rc;
    Pipe& P = *owner;
    cbv_ctx* ctx = P.ctx;
    if (!seeds || !Hinv9 || !boards || !scene || slot0 < 0 || count <= 0 || slot0 + count > P.max_frames) return CBV_ERR_ARG;
    CBV_ENTER(ctx);
    if (P.plan.raw()) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_synth: %s", raw_mode_msg(P));
    RC(join_scan(P)); // lanes and scan of the last run
    size_t o_seeds = 0, o_h = (size_t)count * 8, o_b = o_h + 72, o_s = (o_b + (size_t)count * 64 + 15) & ~(size_t)15;
    size_t total = o_s + sizeof(cbv_scene);
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    RC(dev_ensure(ctx, &P.d_synth, total));
    std::vector<u8> host(total, 0);
    memcpy(host.data() + o_seeds, seeds, (size_t)count * 8);
    memcpy(host.data() + o_h, Hinv9, 72);
    memcpy(host.data() + o_b, boards, (size_t)count * 64);
    memcpy(host.data() + o_s, scene, sizeof(cbv_scene));
    CBV_HIP(ctx, hipMemcpy(P.d_synth.p, host.data(), total, hipMemcpyHostToDevice));
    u8* base = (u8*)P.d_synth.p;
    RC(launch_synth(ctx, P.frames + P.g.frame_stride * slot0, P.g, (const u64*)(base + o_seeds), (const double*)(base + o_h),
                    base + o_b, (const cbv_scene*)(base + o_s), count));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}
