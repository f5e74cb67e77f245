// Frame ingest of the device-resident pipeline: upload, the pinned host ring and the device ring of raw (YUV) frames,
// submit on the copy stream, and the synthetic frames.
#include "cbv_pipeline.h"

// the raw-frame mode (Pipe::raw_mode) has no BGR frames to write
static const char* const kRawModeMsg = "the pipeline runs without enhancement on a YUV or Bayer input format (raw mode): its frames are the raw "
                                       "ring, written by cbv_pipeline_upload_raw or cbv_pipeline_submit in that format";
static const char* const kJpegRawModeMsg = "the pipeline runs without enhancement on Motion-JPEG input in planes mode (raw mode): its frames are "
                                           "the decoded planes, written by cbv_pipeline_upload_jpeg or cbv_pipeline_submit";
static const char* raw_mode_msg(const Pipe& P) { return P.jpeg_planes_on() ? kJpegRawModeMsg : kRawModeMsg; }

// the planes of slot `slot` of the device ring of raw frames
RawPlanes slot_planes(const Pipe& P, int slot)
{
    return tight_raw_planes(P.in_fmt, P.w, P.h, P.raw_ring + tight_raw_geom(P.in_fmt, P.w, P.h).frame_stride * slot);
}

WarpSrc pipeline_raw_warp_src(const Pipe& P, int slot0, const ProfileTabs* ptabs, int np, size_t dst_profile_stride)
{
    if (P.jpeg_planes_on()) return pipeline_jpeg_warp_src(P, slot0, ptabs, np, dst_profile_stride);
    const RawGeom rg = tight_raw_geom(P.in_fmt, P.w, P.h);
    return ptabs ? warp_src_raw_profile(slot_planes(P, slot0), rg, P.g, ptabs, np, dst_profile_stride) : warp_src_raw(slot_planes(P, slot0), rg, P.g);
}

bool pipeline_raw_frames_exist(const Pipe& P) { return P.jpeg_planes_on() ? pipeline_jpeg_has_planes(P) : P.raw_ring != nullptr; }

// bytes between the slots of the ingest rings in the current input format
static size_t host_slot_bytes(const Pipe& P)
{
    if (P.in_fmt == CBV_FMT_MJPEG) return P.jpeg_slot_bytes;
    return P.in_fmt == CBV_FMT_BGR ? P.g.frame_stride : tight_raw_geom(P.in_fmt, P.w, P.h).frame_stride;
}

// the device ring of raw frames (or of JPEG streams) in the current input format
static int ensure_raw_ring(Pipe& P)
{
    cbv_ctx* ctx = P.ctx;
    if (P.raw_ring) return CBV_OK;
    const size_t bytes = host_slot_bytes(P) * P.max_frames;
    if (hipMalloc((void**)&P.raw_ring, bytes + 256) != hipSuccess) {
        P.raw_ring = nullptr;
        return cbv_fail(ctx, CBV_ERR_HIP, "device ring of %zu bytes for the raw frames could not be allocated", bytes);
    }
    return CBV_OK;
}

extern "C" int cbv_pipeline_upload(cbv_pipeline* p, int slot, const uint8_t* bgr, int stride)
{
    if (p && attached(p)) return cbv_fail(p->pipe->ctx, CBV_ERR_STATE, "cbv_pipeline_upload: frames go to the parent of a board");
    if (!p || !bgr || slot < 0 || slot >= p->pipe->max_frames || stride < p->pipe->w * 3) return CBV_ERR_ARG;
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    CBV_ENTER(ctx);
    if (P.raw_mode()) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_upload: %s", raw_mode_msg(P));
    RC(join_scan(P)); // lanes and scan of the last run
    RC(rows_h2d(ctx, P.frames + P.g.frame_stride * slot, bgr, stride, P.w * 3, P.h));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

extern "C" int cbv_pipeline_upload_raw(cbv_pipeline* p, int slot, const cbv_raw_frame* raw)
{
    if (p && attached(p)) return cbv_fail(p->pipe->ctx, CBV_ERR_STATE, "cbv_pipeline_upload_raw: frames go to the parent of a board");
    if (!p || !raw || slot < 0 || slot >= p->pipe->max_frames) return cbv_fail(p ? p->pipe->ctx : nullptr, CBV_ERR_ARG, "cbv_pipeline_upload_raw: bad arguments");
    if (raw->fmt == CBV_FMT_BGR) return cbv_pipeline_upload(p, slot, raw->plane0, raw->stride0);
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    RC(check_raw_format(ctx, raw->fmt, P.w, P.h, "cbv_pipeline_upload_raw"));
    CBV_ENTER(ctx);
    RC(join_scan(P)); // lanes and scan of the last run
    if (P.raw_mode()) { // the frame as it is into its slot of the raw ring, rows packed
        if (P.jpeg_planes_on()) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_upload_raw: format %d, but %s", raw->fmt, kJpegRawModeMsg);
        if (raw->fmt != P.in_fmt)
            return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_upload_raw: format %d, but %s (format %d)", raw->fmt, kRawModeMsg, P.in_fmt);
        const u8* planes[3];
        int strides[3];
        raw_frame_planes(raw, planes, strides);
        RC(check_raw_planes(ctx, raw->fmt, P.w, planes, strides, "cbv_pipeline_upload_raw"));
        RC(ensure_raw_ring(P));
        // the raw ring is the only frame store here: a copy of this slot that cbv_pipeline_submit left in flight lands first
        if (P.copy_stream) CBV_HIP(ctx, hipStreamSynchronize(P.copy_stream));
        const RawPlanes dst = slot_planes(P, slot);
        for (int i = 0; i < raw_fmt_planes(raw->fmt); i++)
            RC(rows_h2d(ctx, (u8*)dst.p[i], planes[i], strides[i], raw_plane_wbytes(raw->fmt, P.w, i), raw_plane_rows(raw->fmt, P.h, i)));
        CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return CBV_OK;
    }
    RC(raw_h2d_convert(ctx, raw, P.w, P.h, P.frames + P.g.frame_stride * slot, P.g, "cbv_pipeline_upload_raw"));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}


extern "C" size_t cbv_pipeline_host_slot_bytes(cbv_pipeline* p)
{
    if (!p || attached(p)) return 0;
    std::lock_guard<std::recursive_mutex> lock(p->pipe->ctx->mu);
    return host_slot_bytes(*p->pipe);
}

extern "C" int cbv_pipeline_set_input_format(cbv_pipeline* p, int fmt)
{
    if (!p) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_pipeline_set_input_format: the pipeline is null");
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    if (attached(p)) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_set_input_format: frames go to the parent of a board");
    if (fmt != CBV_FMT_BGR && fmt != CBV_FMT_MJPEG) RC(check_raw_format(ctx, fmt, P.w, P.h, "cbv_pipeline_set_input_format"));
    CBV_ENTER(ctx);
    if (fmt == CBV_FMT_MJPEG) { // the decode's scratch is sized here, once: cbv_pipeline_submit never allocates
        RC(pipeline_jpeg_ensure(P));
        if (!P.jpeg_slot_bytes) P.jpeg_slot_bytes = pipeline_jpeg_default_slot_bytes(P.w, P.h);
    }
    // the copies and conversions in flight read the rings that go away here (both run on the copy stream)
    if (P.copy_stream) CBV_HIP(ctx, hipStreamSynchronize(P.copy_stream));
    if (fmt == CBV_FMT_MJPEG) RC(pipeline_jpeg_size_scratch(P, "cbv_pipeline_set_input_format")); // ... for this slot size, entropy setting and depth
    if (P.raw_mode()) { // ... and so do the runs in flight
        RC(join_scan(P));
        CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (P.host_ring) (void)hipHostFree(P.host_ring);
    if (P.raw_ring) (void)hipFree(P.raw_ring);
    P.host_ring = P.raw_ring = nullptr;
    const int fmt_was = P.in_fmt;
    P.in_fmt = fmt;
    if (P.jpeg) { // the plane ring of the planes mode comes with the format and goes with it
        const int rc = pipeline_jpeg_plane_ring(P, "cbv_pipeline_set_input_format");
        if (rc) {
            P.in_fmt = fmt_was == CBV_FMT_MJPEG ? CBV_FMT_BGR : fmt_was; // (the ingest rings are gone: they come back on first use)
            if (pipeline_frame_ring(P) != CBV_OK) P.configured = false;  // no ring for that format either: nothing may run
            return rc;
        }
    }
    return pipeline_frame_ring(P); // (a CBV_SKIP_ENHANCE_PROFILE_RAW pipeline has a BGR ring only while its frames are BGR)
}

extern "C" uint8_t* cbv_pipeline_host_ring(cbv_pipeline* p)
{
    if (!p) return nullptr;
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    if (attached(p)) {
        cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_host_ring: frames go to the parent of a board");
        return nullptr;
    }
    if (!P.host_ring) {
        if (hipSetDevice(ctx->device) != hipSuccess) return nullptr;
        const size_t bytes = host_slot_bytes(P) * P.max_frames;
        if (hipHostMalloc((void**)&P.host_ring, bytes, hipHostMallocDefault) != hipSuccess) {
            cbv_fail(ctx, CBV_ERR_HIP, "pinned host ring of %zu bytes could not be allocated", bytes);
            P.host_ring = nullptr;
        } else if (P.in_fmt != CBV_FMT_BGR && ensure_raw_ring(P) != CBV_OK) {
            (void)hipHostFree(P.host_ring);
            P.host_ring = nullptr;
        }
    }
    return P.host_ring;
}

extern "C" int cbv_pipeline_submit(cbv_pipeline* p, int slot0, int count)
{
    if (!p) return CBV_ERR_ARG;
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    if (attached(p)) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_submit: frames go to the parent of a board");
    if (slot0 < 0 || count <= 0 || slot0 + count > P.max_frames) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_submit: bad slot range");
    if (!P.host_ring) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_submit: cbv_pipeline_host_ring() was never called");
    CBV_ENTER(ctx);
    if (!P.copy_stream) RC(ctx_worker_stream(ctx, &ctx->copy_stream, &P.copy_stream));
    // do not overwrite device slots a run that is still in flight reads: ANY such run, not only the last one
    retire_runs(P);
    Pipe::RunRec* reader = newest_run(P, slot0, count, 0);
    if (P.in_fmt == CBV_FMT_MJPEG) {
        RC(pipeline_jpeg_submit(P, slot0, count, reader ? (reader->one_event ? reader->scan_ev : reader->lanes_ev) : nullptr));
    } else if (P.in_fmt == CBV_FMT_BGR) {
        if (reader) CBV_HIP(ctx, hipStreamWaitEvent(P.copy_stream, reader->one_event ? reader->scan_ev : reader->lanes_ev, 0));
        CBV_HIP(ctx, hipMemcpyAsync(P.frames + P.g.frame_stride * slot0, P.host_ring + P.g.frame_stride * slot0,
                                    P.g.frame_stride * count, hipMemcpyHostToDevice, P.copy_stream));
    } else {
        // Raw slots to the device raw ring, then their conversion into the frame ring, both on the copy stream: stream order
        // is the copy -> conversion dependency and keeps a later copy off raw slots an earlier conversion still reads, and
        // the one event below stands for both.  Only the conversion writes the frames the runs in flight read, so the copy
        // itself does not wait for them.
        // In raw mode the copy is all: the runs read the raw ring itself, so it is the copy that waits for them.
        const RawGeom rg = tight_raw_geom(P.in_fmt, P.w, P.h);
        u8* raw = P.raw_ring + rg.frame_stride * slot0;
        hipEvent_t read_ev = reader ? (reader->one_event ? reader->scan_ev : reader->lanes_ev) : nullptr;
        if (read_ev && P.raw_mode()) { // (the wait goes in front of the copy)
            CBV_HIP(ctx, hipStreamWaitEvent(P.copy_stream, read_ev, 0));
            read_ev = nullptr;
        }
        CBV_HIP(ctx, hipMemcpyAsync(raw, P.host_ring + rg.frame_stride * slot0, rg.frame_stride * count, hipMemcpyHostToDevice, P.copy_stream));
        if (read_ev) CBV_HIP(ctx, hipStreamWaitEvent(P.copy_stream, read_ev, 0));
        hipStream_t caller = ctx->stream;
        ctx->stream = P.copy_stream;
        const int rc = P.raw_mode() ? CBV_OK : launch_ingest(ctx, slot_planes(P, slot0), rg, P.frames + P.g.frame_stride * slot0, P.g, count);
        ctx->stream = caller;
        RC(rc);
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
    if (p && attached(p)) return cbv_fail(p->pipe->ctx, CBV_ERR_STATE, "cbv_pipeline_synth: frames go to the parent of a board");
    if (!p || !seeds || !Hinv9 || !boards || !scene || slot0 < 0 || count <= 0 || slot0 + count > p->pipe->max_frames) return CBV_ERR_ARG;
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    CBV_ENTER(ctx);
    if (P.raw_mode()) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_synth: %s", raw_mode_msg(P));
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
