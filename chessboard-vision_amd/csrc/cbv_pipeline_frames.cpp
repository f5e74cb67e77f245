// The frame store of the device-resident pipeline: the BGR ring, the two ingest rings, the plane ring and the Motion-JPEG
// decode's scratch are allocated and freed here and nowhere else, so that they always match Pipe::plan (frame_plan.h;
// DESIGN.md, "Where the frames live").
#include "cbv_pipeline.h"

static void jpeg_scratch_free(Pipe::JpegScratch& sc)
{
    void* dev[] = {sc.mpos, sc.coef, sc.planes, sc.pieces, sc.segs};
    for (void* q : dev)
        if (q) (void)hipFree(q);
    sc = Pipe::JpegScratch();
}

// a gray frame of the pipeline's size: what the warp reads of a slot that was never decoded, over zeroed planes
static JpegDesc jpeg_gray_desc(int w, int h)
{
    JpegDesc D;
    memset(&D, 0, sizeof(D));
    D.w = w;
    D.h = h;
    D.ncomp = 1;
    D.hs = D.vs = 1;
    D.mcux = (w + 7) / 8;
    D.mcuy = (h + 7) / 8;
    D.nint = 1;
    D.bw[0] = D.mcux;
    D.bh[0] = D.mcuy;
    D.cw[0] = w;
    D.ch[0] = h;
    D.plane_total = (uint32_t)D.mcux * (uint32_t)D.mcuy * 64u;
    D.std_tables = 1;
    return D;
}

static void jpeg_state_free(Pipe& P)
{
    JpegState* J = P.jpeg;
    if (!J) return;
    void* host[] = {J->h_lengths, J->h_desc, J->h_ioff, J->h_tabs};
    for (void* q : host)
        if (q) (void)hipHostFree(q);
    void* dev[] = {J->d_desc, J->d_ioff, J->d_tabs, J->d_status, J->d_nfound, J->d_stats, J->d_wdesc};
    for (void* q : dev)
        if (q) (void)hipFree(q);
    delete J;
    P.jpeg = nullptr;
}

// what lives as long as the slots; the rings and the decode's scratch are pipeline_set_frames'
int pipeline_jpeg_ensure(Pipe& P)
{
    cbv_ctx* ctx = P.ctx;
    if (P.jpeg) return CBV_OK;
    if (P.h > 65535) return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "Motion-JPEG frames of %d rows", P.h);
    JpegState* J = new JpegState;
    const size_t n = (size_t)P.max_frames;
    bool ok = hipHostMalloc((void**)&J->h_lengths, n * sizeof(u32), hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc((void**)&J->h_desc, n * sizeof(JpegDesc), hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc((void**)&J->h_ioff, 2 * n * sizeof(u32), hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc((void**)&J->h_tabs, JpegState::NSETS * sizeof(JpegTables), hipHostMallocDefault) == hipSuccess &&
              hipMalloc((void**)&J->d_desc, n * sizeof(JpegDesc)) == hipSuccess && hipMalloc((void**)&J->d_ioff, 2 * n * sizeof(u32)) == hipSuccess &&
              hipMalloc((void**)&J->d_tabs, JpegState::NSETS * sizeof(JpegTables)) == hipSuccess &&
              hipMalloc((void**)&J->d_status, n * sizeof(int)) == hipSuccess && hipMalloc((void**)&J->d_nfound, n * sizeof(int)) == hipSuccess &&
              hipMalloc((void**)&J->d_stats, n * 3 * sizeof(u32)) == hipSuccess && hipMalloc((void**)&J->d_wdesc, n * sizeof(JpegDesc)) == hipSuccess;
    if (ok) ok = hipMemset(J->d_status, 0, n * sizeof(int)) == hipSuccess && hipMemset(J->d_stats, 0, n * 3 * sizeof(u32)) == hipSuccess;
    P.jpeg = J;
    if (!ok) {
        (void)hipGetLastError();
        jpeg_state_free(P);
        return cbv_fail(ctx, CBV_ERR_HIP, "the Motion-JPEG decode's buffers could not be allocated");
    }
    memset(J->h_lengths, 0, n * sizeof(u32));
    return CBV_OK;
}

int pipeline_raw_ring(Pipe& P)
{
    if (P.raw_ring) return CBV_OK;
    const size_t bytes = P.plan.slot_bytes * P.max_frames;
    if (hipMalloc((void**)&P.raw_ring, bytes + 256) != hipSuccess) {
        P.raw_ring = nullptr;
        return cbv_fail(P.ctx, CBV_ERR_HIP, "device ring of %zu bytes for the raw frames could not be allocated", bytes);
    }
    return CBV_OK;
}

int pipeline_host_ring(Pipe& P)
{
    if (P.host_ring) return CBV_OK;
    const size_t bytes = P.plan.slot_bytes * P.max_frames;
    if (hipHostMalloc((void**)&P.host_ring, bytes, hipHostMallocDefault) != hipSuccess) {
        P.host_ring = nullptr;
        return cbv_fail(P.ctx, CBV_ERR_HIP, "pinned host ring of %zu bytes could not be allocated", bytes);
    }
    if (P.fs.fmt != CBV_FMT_BGR && pipeline_raw_ring(P) != CBV_OK) {
        (void)hipHostFree(P.host_ring);
        P.host_ring = nullptr;
        return CBV_ERR_HIP;
    }
    return CBV_OK;
}

// cbv_pipeline_destroy: every buffer of the store
void pipeline_frames_free(Pipe& P)
{
    jpeg_state_free(P);
    if (P.host_ring) (void)hipHostFree(P.host_ring);
    void* dev[] = {P.raw_ring, P.plane_ring, P.frames};
    for (void* q : dev)
        if (q) (void)hipFree(q);
    jpeg_scratch_free(P.jsc);
    P.host_ring = P.raw_ring = P.plane_ring = P.frames = nullptr;
    P.plan = FramePlan();
}

int pipeline_set_frames(Pipe& P, const FrameSettings& next, const char* who, bool drop_ingest)
{
    cbv_ctx* ctx = P.ctx;
    // 1. the next plan against what exists
    FramePlan np;
    char msg[160];
    const int rc = frame_plan(next, &np, msg, sizeof(msg));
    if (rc) return cbv_fail(ctx, rc, "%s: %s", who, msg);
    if (next.fmt == CBV_FMT_MJPEG) RC(pipeline_jpeg_ensure(P));
    const bool new_bgr = np.bgr_ring && !P.frames, old_bgr = !np.bgr_ring && P.frames;
    const bool ring_changes = np.plane_mode != P.plan.plane_mode; // a mode has one ring from its first moment to its last
    const bool new_ring = ring_changes && np.plane_mode != CBV_JPEG_PLANES_OFF, old_ring = ring_changes && P.plane_ring;
    const bool scratch_changes = !np.same_scratch(P.plan);
    drop_ingest = (drop_ingest || np.slot_bytes != P.plan.slot_bytes) && (P.host_ring || P.raw_ring); // (no ring outlives its slot size)
    // 2. what is in flight reads (or writes) what goes away or changes hands here: the runs, the caller's stream, and the
    // copies, conversions and decodes of the copy stream
    if (old_bgr || old_ring || drop_ingest || (scratch_changes && P.plan.depth)) {
        RC(join_scan(P));
        CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (P.copy_stream) CBV_HIP(ctx, hipStreamSynchronize(P.copy_stream));
    }
    // 3. everything new before anything old is let go (the ingest rings apart: they are made on first use)
    u8 *frames = nullptr, *ring = nullptr;
    Pipe::JpegScratch sc;
    const char* what = nullptr;
    size_t bytes = 0;
    auto dev_alloc = [&](void* q, size_t n, const char* name) { // false, and nothing more is tried, after the first failure
        if (!what && n && hipMalloc((void**)q, n) != hipSuccess) {
            what = name;
            bytes = n;
        }
        return !what;
    };
    if (new_bgr) dev_alloc(&frames, P.g.frame_stride * P.max_frames + 256, "the frame ring");
    const size_t ring_bytes = np.plane_slot * (size_t)P.max_frames + 256; // 256 bytes of slack behind the last slot
    if (new_ring) dev_alloc(&ring, ring_bytes, "the plane ring");
    if (scratch_changes && np.depth) {
        const size_t d = (size_t)np.depth;
        dev_alloc(&sc.mpos, d * np.max_int * sizeof(u32), "the Motion-JPEG decode's scratch");
        dev_alloc(&sc.coef, d * np.frame_elems * sizeof(int16_t), "the Motion-JPEG decode's scratch");
        if (np.own_planes) dev_alloc(&sc.planes, d * np.frame_elems, "the Motion-JPEG decode's scratch");
        dev_alloc(&sc.pieces, d * np.piece_words * sizeof(u32), "the Motion-JPEG decode's scratch");
        dev_alloc(&sc.segs, d * np.seg_words * sizeof(u32), "the Motion-JPEG decode's scratch");
    }
    // a new plane ring is zeroed and the warp's descriptors become gray frames: last of all, since the descriptors are shared
    // with the ring that is still there (if the device fails here it is lost, and the old ring's descriptors with it)
    if (new_ring && !what) {
        const std::vector<JpegDesc> gray((size_t)P.max_frames, jpeg_gray_desc(P.w, P.h));
        if (hipMemset(ring, 0, ring_bytes) != hipSuccess || hipMemcpy(P.jpeg->d_wdesc, gray.data(), gray.size() * sizeof(JpegDesc), hipMemcpyHostToDevice) != hipSuccess) {
            what = "the plane ring";
            bytes = ring_bytes;
        }
    }
    if (what) { // the one failure exit: nothing old has been touched
        (void)hipGetLastError();
        if (frames) (void)hipFree(frames);
        if (ring) (void)hipFree(ring);
        jpeg_scratch_free(sc);
        return cbv_fail(ctx, CBV_ERR_HIP, "%s: %s (%zu bytes) could not be allocated", who, what, bytes);
    }
    // 4. the old buffers go, the new ones take their place
    if (drop_ingest) {
        if (P.host_ring) (void)hipHostFree(P.host_ring);
        if (P.raw_ring) (void)hipFree(P.raw_ring);
        P.host_ring = P.raw_ring = nullptr;
    }
    if (old_bgr) (void)hipFree(P.frames);
    if (old_bgr || new_bgr) P.frames = frames;
    if (old_ring) (void)hipFree(P.plane_ring);
    if (ring_changes) P.plane_ring = ring;
    if (scratch_changes) {
        jpeg_scratch_free(P.jsc);
        P.jsc = sc;
    }
    // 5. and only now the settings
    P.fs = next;
    P.plan = np;
    return CBV_OK;
}
