// Device-resident batched pipeline (include/cbv.h, cbv_pipeline_*): frame ring, enhancement lanes, temporal scan, and the
// boards one camera frame feeds (cbv_pipeline_add_board).
#include <string.h>

#include <algorithm>

#include "../../include/cbv_chess.h"
#include "cbv_internal.h"
#include "piece_sweep_core.h"
#include "session_core.h"

// One board of a pipeline: what configure's squares part sets up (board_setup).  Board 0 is the pipeline's own; the
// boards cbv_pipeline_add_board attaches have the same shape.
struct Board {
    cbv_pipeline_config cfg; // the pipeline's configuration with the board's subset (cbv_board_config) in it
    double Minv[9];
    u8* warped = nullptr; // [max_frames][S][S][3]
    size_t warped_stride = 0;
    std::vector<SquareDesc> descs;
    size_t plane_total = 0;
    int max_px = 0; // pixels of the largest square
    DevBuf d_descs, d_masks, d_gray, d_stats, d_ref, d_state, d_results, d_flags, d_dec, d_mean, d_var, d_noise, d_noise_state, d_hough,
        d_check, d_hough_over;
    u8* h_stage = nullptr; // pinned mirror of d_results ([max_frames] records, then the HoughCircles overflow word): written by
                           // the last kernel of a SHORT run (ResultMirror), by a copy otherwise; read by cbv_pipeline_results
    u32* over_h = nullptr; // the overflow word in h_stage
    std::vector<u8> slot_mirrored; // per slot: the mirror holds the slot's newest record (once its run has finished)
    HoughCfg hough_cfg;
    bool calibrated = false, has_check = false; // has_check: squares_to_check masks were set
    int model_mode = CBV_MODEL_FROZEN;          // cbv_pipeline_set_model_update
    double model_alpha = 0.1;
    // cbv_pipeline_set_change_blur: ChangeDetector.blur_kernel.  With 5 the ChangeDetector stage reads d_gray, the
    // PieceDetector's planes, as it always did; otherwise d_cgray holds its own planes, [max_frames][plane_total], written by
    // k_change_blur_stats.  slot_blur = the kernel each slot was last run with (0: never run).
    int change_k = 5;
    DevBuf d_cgray;
    std::vector<u8> slot_blur;
    bool own_blur() const { return change_k != 5; }
    u8* change_planes() const { return (u8*)(own_blur() ? d_cgray.p : d_gray.p); }
    // game session (cbv_pipeline_session_begin): the device state, the per-frame history records of the scan and how many
    // of the session's move records the host has handed out
    bool session = false;
    cbv_session_config ses_cfg = {};
    DevBuf d_session, d_hist;
    int ses_drained = 0;
    // online play: the board events that wait for their frame (cbv_pipeline_session_sync), the session frames enqueued so
    // far (the session frame index of the next run's first frame) and the radar records, one per slot
    std::vector<cbv_session_event> ses_events;
    int ses_frames = 0;
    DevBuf d_radar;
    bool adaptive() const { return calibrated && model_mode != CBV_MODEL_FROZEN; } // k_model_scan runs for this board
};

struct Pipe;

// The opaque handle: one board of a pipeline.  cbv_pipeline_create returns board 0, which owns the pipeline.
struct cbv_pipeline {
    Pipe* pipe;
    Board b;
};

// What the boards of a pipeline share: frames, enhancement, lanes, ingest, runs, and the boards' kernel arguments.
struct Pipe {
    cbv_ctx* ctx = nullptr;
    int w = 0, h = 0, max_frames = 0;
    Geom g;
    bool configured = false;
    bool keep_enhanced = false;
    bool skip_enhance = false; // cfg.skip_enhance: the warp samples the frames as they are, no enhancement scratch exists
    int chunk = 8;
    u8* frames = nullptr;
    // Lanes: chunk c runs on lane c % n_lanes, each lane with its own HIP stream and scratch, so a
    // VALU-bound bilateral launch of one chunk overlaps the memory-latency-bound kernels of another.
    enum { MAX_LANES = 4 };
    int n_lanes = 1;
    hipStream_t lane_stream[MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t lane_done[MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t start_ev = nullptr;
    u8* A[MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};
    u8* B[MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};
    u8* C[MAX_LANES] = {nullptr, nullptr, nullptr, nullptr}; // third scratch frame set: region-limited enhancement only
    bool use_region = false;                                  // cfg.enhance_region, keep_enhanced == 0, a usable footprint
    PxRect region = {0, 0, 0, 0};                             // source pixels the warps sample (+ margin), clipped
    DevBuf lane_small[MAX_LANES];
    DevBuf lane_work[MAX_LANES]; // HoughCircles worklist of the lane's current chunk: count, then frame << 8 | square
    u8* enhanced = nullptr;      // [max_frames] when keep_enhanced
    DevBuf d_synth;
    // ingest: pinned host mirror of the frame ring, filled by the capture side and copied on its own stream; with a YUV
    // input format (cbv_pipeline_set_input_format) both it and `raw_ring`, its device copy, hold raw frames, which
    // k_ingest converts into `frames` behind the copy
    u8* host_ring = nullptr;
    int in_fmt = CBV_FMT_BGR;
    // Without enhancement (skip_enhance) a YUV input format makes the raw ring THE frames: k_warp_yuv samples it, nothing is
    // converted and `frames` is neither written nor read (raw_mode below).
    u8* raw_ring = nullptr; // [max_frames] raw frames (tight_raw_geom), allocated on first use; null with CBV_FMT_BGR
    hipStream_t copy_stream = nullptr;
    struct CopyRec {
        int s0, cnt;
        hipEvent_t ev;
        bool pending;
    };
    std::vector<CopyRec> copies;
    // The temporal scan (+ NoiseHandler) of a run goes to its own stream behind the lanes' events, so the next run's
    // enhancement of OTHER slots overlaps it; scans of successive runs stay ordered on that stream.  (Runs of one or
    // two frames keep their scan on the caller's stream, after waiting for every run in flight: see cbv_pipeline_run.)
    hipStream_t scan_stream = nullptr;
    hipEvent_t main_done = nullptr;
    // Every run that may still be executing: its slot range and two events on the (in-order) scan stream,
    // `lanes_ev` = all lanes have read the input frames and written the per-slot buffers, `scan_ev` = the scan has
    // read them.  A later run (or ingest copy) that touches overlapping slots waits on the NEWEST overlapping
    // record, which covers the older ones because the scan stream is in order.  Records are recycled once their
    // scan event has completed.
    struct RunRec {
        int s0, cnt;
        unsigned long long seq;
        hipEvent_t lanes_ev, scan_ev;
        bool live;
        bool one_event; // a run of a frame or two, all on the caller's stream: only scan_ev is recorded (an event between two
                        // kernels is a ~5 us bubble in a 150 us chain), and it stands for lanes_ev too
        DevBuf retry; // HoughCircles second-pass list of this run (HoughCfg::retry), frames numbered from the run's slot0
    };
    std::vector<RunRec> runs;
    unsigned long long run_seq = 0;    // sequence number of the newest run
    unsigned long long joined_seq = 0; // runs up to this one are ordered before later work on `joined_stream`
    hipStream_t joined_stream = nullptr;
    // the boards (board 0 = the handle cbv_pipeline_create returned) and their kernel arguments: `tab` holds one BoardDev
    // per board (board_dev), tab[0] feeds the single-board launches; with boards attached it is uploaded to d_boards for the
    // multi-board launches, which also take the maxima over the boards below
    std::vector<cbv_pipeline*> boards;
    std::vector<BoardDev> tab;
    DevBuf d_boards;
    bool any_hough = false;
    bool any_adaptive = false; // some board's model follows the frames: k_model_scan runs in front of the temporal scan
    bool any_session = false;  // some board runs a game session: the boards' scans are launched board by board
    bool any_own_blur = false; // some board's ChangeDetector has a blur kernel of its own: k_change_blur_stats runs behind the statistics
    size_t hough_lds[2] = {0, 0};
    int max_px = 0, max_S = 0;
    Board& b0() const { return boards[0]->b; }
    bool raw_mode() const { return skip_enhance && in_fmt != CBV_FMT_BGR; }
};

// a handle of a board attached by cbv_pipeline_add_board (not board 0, which stands for the whole pipeline)
static bool attached(const cbv_pipeline* p) { return p != p->pipe->boards[0]; }

static bool ranges_overlap(int a0, int an, int b0, int bn) { return a0 < b0 + bn && b0 < a0 + an; }

static void retire_runs(Pipe& P)
{
    for (auto& r : P.runs)
        if (r.live && hipEventQuery(r.scan_ev) == hipSuccess) r.live = false;
}

// newest record that is still in flight, newer than run `after`, and overlaps the slots (cnt <= 0: any slots)
static Pipe::RunRec* newest_run(Pipe& P, int s0, int cnt, unsigned long long after)
{
    Pipe::RunRec* best = nullptr;
    for (auto& r : P.runs)
        if (r.live && r.seq > after && (cnt <= 0 || ranges_overlap(s0, cnt, r.s0, r.cnt)) && (!best || r.seq > best->seq)) best = &r;
    return best;
}

// ... and not yet ordered before the context's stream
static Pipe::RunRec* newest_unjoined(Pipe& P, int s0, int cnt)
{
    if (P.joined_stream != P.ctx->stream) { // the caller switched streams: nothing is ordered before the new one
        P.joined_stream = P.ctx->stream;
        P.joined_seq = 0;
    }
    return newest_run(P, s0, cnt, P.joined_seq);
}

// make the context's stream wait for every run that is still in flight (lanes and scans; they write every board)
static int join_scan(Pipe& P)
{
    cbv_ctx* ctx = P.ctx;
    if (Pipe::RunRec* r = newest_unjoined(P, 0, 0)) {
        CBV_HIP(ctx, hipStreamWaitEvent(ctx->stream, r->scan_ev, 0));
        P.joined_seq = r->seq;
    }
    return CBV_OK;
}

// make the context's stream wait for the runs in flight that touch these slots (older scans of the same slots
// may still be queued: the newest overlapping record covers them)
static int join_slots(Pipe& P, int s0, int cnt)
{
    cbv_ctx* ctx = P.ctx;
    retire_runs(P);
    if (Pipe::RunRec* r = newest_unjoined(P, s0, cnt)) {
        CBV_HIP(ctx, hipStreamWaitEvent(ctx->stream, r->scan_ev, 0));
        // everything up to r is ordered now; records between joined_seq and r.seq that do not overlap are too
        P.joined_seq = std::max(P.joined_seq, r->seq);
    }
    return CBV_OK;
}

// kernel arguments of k_change_blur_stats for an odd k in 1..31: the centre tap and the taps on one side of it
static ChangeBlur change_blur_coef(int k)
{
    ChangeBlur cb;
    memset(&cb, 0, sizeof(cb));
    int coef[32];
    build_gaussian_q8(k, coef);
    cb.k = k;
    for (int j = 0; j <= k / 2; j++) cb.cf[j] = (u32)coef[k / 2 + j];
    return cb;
}

// the kernel arguments of a board: its BoardDev entry, pointers of slot 0 (the launches add their first slot); lds = LDS
// bytes of its HoughCircles passes (0: the squares do not fit)
static BoardDev board_dev(const Board& q, size_t lds[2])
{
    const cbv_pipeline_config& c = q.cfg;
    BoardDev T;
    memset(&T, 0, sizeof(T));
    memcpy(T.Minv, q.Minv, sizeof(T.Minv));
    T.S = c.board_size;
    T.rot180 = c.rot180;
    // launch_warp's block shape of an S x S destination (BLOCK_SZ = 32)
    int bh0 = 16 < T.S ? 16 : T.S;
    const int bw0 = 1024 / bh0 < T.S ? 1024 / bh0 : T.S;
    bh0 = 1024 / bw0 < T.S ? 1024 / bw0 : T.S;
    T.bw0 = bw0;
    T.bh0 = bh0;
    T.warped = q.warped;
    T.warped_stride = q.warped_stride;
    T.descs = (const SquareDesc*)q.d_descs.p;
    T.n = c.n_rois;
    T.want_hough = c.use_hough;
    T.masks = (const u8*)q.d_masks.p;
    T.gray = (u8*)q.d_gray.p;
    T.plane_total = q.plane_total;
    // A board whose model follows the frames gets its z-score statistics from k_model_scan, frame after frame on the scan
    // stream: the statistics kernel of the lanes must not read the model, which the scan of the run before may still write
    // ... and neither does it for a board with a blur kernel of its own: k_change_blur_stats makes those planes and statistics
    const bool frozen = q.calibrated && !q.adaptive();
    T.mean = frozen && !q.own_blur() ? (const float*)q.d_mean.p : nullptr;
    T.sd = frozen && !q.own_blur() ? (const float*)q.d_var.p + q.plane_total : nullptr;
    T.cgray = q.change_planes();
    T.cmean = frozen && q.own_blur() ? (const float*)q.d_mean.p : nullptr;
    T.csd = frozen && q.own_blur() ? (const float*)q.d_var.p + q.plane_total : nullptr;
    T.cb = change_blur_coef(q.change_k);
    T.ms.mode = q.adaptive() ? q.model_mode : CBV_MODEL_FROZEN;
    // (1 - self.alpha) and self.alpha are python doubles turned float32 by numpy (launch_squares_ema)
    T.ms.one_minus = (float)(1.0 - q.model_alpha);
    T.ms.alpha = (float)q.model_alpha;
    T.ms.z_thresh = (float)c.z_threshold;
    T.ms.mean = (float*)q.d_mean.p;
    T.ms.var = (float*)q.d_var.p;
    T.ms.sd = (float*)q.d_var.p + q.plane_total;
    T.z_thresh = (float)c.z_threshold;
    T.stats = (cbv_sq_stats*)q.d_stats.p;
    T.dec = (u8*)q.d_dec.p;
    T.hough = c.use_hough ? (cbv_hough_result*)q.d_hough.p : nullptr;
    lds[0] = lds[1] = 0;
    if (c.use_hough) hough_board_cfgs(q.hough_cfg, T.hcfg, lds);
    T.sp = scan_params(c, q.calibrated);
    T.ref = (u8*)q.d_ref.p;
    T.state = (ScanState*)q.d_state.p;
    T.flags = (u8*)q.d_flags.p;
    T.results = (cbv_frame_result*)q.d_results.p;
    T.check = (const u64*)q.d_check.p; // (all-zero sets = no squares_to_check)
    T.noise_state = (cbv_noise_state*)q.d_noise_state.p;
    T.noise = (cbv_noise_result*)q.d_noise.p;
    T.mirror = (cbv_frame_result*)q.h_stage;
    T.over_src = c.use_hough ? (const u32*)q.d_hough_over.p : nullptr;
    T.over_dst = q.over_h;
    return T;
}

// Rebuild the boards' kernel arguments whenever a board is set up, attached, detached or calibrated, or its model-update
// mode or its ChangeDetector blur kernel changes.  The device table
// and the maxima of the multi-board launches exist only with boards attached.  Nothing may be in flight: the callers
// joined the runs.
static int pipeline_tables(Pipe& P)
{
    cbv_ctx* ctx = P.ctx;
    const int nb = (int)P.boards.size();
    P.tab.resize(nb);
    P.any_hough = P.any_adaptive = P.any_session = P.any_own_blur = false;
    P.hough_lds[0] = P.hough_lds[1] = 0;
    P.max_px = P.max_S = 0;
    for (int k = 0; k < nb; k++) {
        const Board& q = P.boards[k]->b;
        size_t lds[2];
        P.tab[k] = board_dev(q, lds);
        if (q.cfg.use_hough) {
            // (a single board's launchers check the layout themselves, at run time)
            if (nb > 1 && (!lds[0] || !lds[1]))
                return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "HoughCircles stage: %dx%d squares of board %d do not fit the LDS layout",
                                q.hough_cfg.maxw, q.hough_cfg.maxh, k);
            P.any_hough = true;
            P.hough_lds[0] = std::max(P.hough_lds[0], lds[0]);
            P.hough_lds[1] = std::max(P.hough_lds[1], lds[1]);
        }
        P.any_adaptive = P.any_adaptive || q.adaptive();
        P.any_session = P.any_session || q.session;
        P.any_own_blur = P.any_own_blur || q.own_blur();
        P.max_px = std::max(P.max_px, q.max_px);
        P.max_S = std::max(P.max_S, q.cfg.board_size);
    }
    if (nb == 1) return CBV_OK;
    RC(dev_ensure(ctx, &P.d_boards, sizeof(BoardDev) * nb));
    CBV_HIP(ctx, hipMemcpyAsync(P.d_boards.p, P.tab.data(), sizeof(BoardDev) * nb, hipMemcpyHostToDevice, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

// enhance_region: the bounding rectangle of every board's warp footprint (any board without one: the whole frame); the
// third scratch frame set is allocated when the region first becomes usable
static int pipeline_update_region(Pipe& P)
{
    cbv_ctx* ctx = P.ctx;
    const cbv_pipeline_config& cfg = P.b0().cfg;
    bool use = cfg.enhance_region && !P.keep_enhanced && sharpen_region_ok(cfg.enhance.sharpen_kernel);
    PxRect u = {0, 0, 0, 0};
    for (size_t k = 0; use && k < P.boards.size(); k++) {
        const Board& q = P.boards[k]->b;
        PxRect r;
        use = warp_footprint(q.Minv, q.cfg.board_size, q.cfg.board_size, P.w, P.h, &r);
        if (use) u = k == 0 ? r : PxRect{std::min(u.x0, r.x0), std::min(u.y0, r.y0), std::max(u.x1, r.x1), std::max(u.y1, r.y1)};
    }
    if (use)
        for (int l = 0; l < P.n_lanes; l++)
            if (!P.C[l]) CBV_HIP(ctx, hipMalloc((void**)&P.C[l], P.g.frame_stride * P.chunk + 256));
    P.use_region = use;
    if (use) P.region = u;
    return CBV_OK;
}

// the per-board checks of cbv_pipeline_configure (cbv_pipeline_add_board makes the same)
static int check_board_cfg(cbv_ctx* ctx, const cbv_pipeline_config* cfg)
{
    if (cfg->n_rois <= 0 || cfg->n_rois > CBV_MAX_SQUARES || cfg->board_size <= 0 || cfg->board_size > 4096)
        return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_configure: bad board/roi configuration");
    if (cfg->history_size < 1 || cfg->history_size > 7) return cbv_fail(ctx, CBV_ERR_ARG, "history_size must be in 1..7");
    for (int i = 0; i < cfg->n_rois; i++) {
        const cbv_roi& r = cfg->rois[i];
        if (r.w <= 0 || r.h <= 0 || r.w > CBV_MAX_SQUARE_DIM || r.h > CBV_MAX_SQUARE_DIM || r.x0 < 0 || r.y0 < 0 ||
            r.x0 + r.w > cfg->board_size || r.y0 + r.h > cfg->board_size)
            return cbv_fail(ctx, CBV_ERR_ARG, "roi %d is invalid for a %dx%d board", i, cfg->board_size, cfg->board_size);
    }
    return CBV_OK;
}

// a board's part of cbv_pipeline_configure / cbv_pipeline_add_board: warped frames, square descriptors and planes, temporal
// state, results
static int board_setup(const Pipe& P, Board& b, const cbv_pipeline_config& cfg)
{
    cbv_ctx* ctx = P.ctx;
    const int S = cfg.board_size, n = cfg.n_rois;
    b.cfg = cfg;
    if (!host_invert3x3(cfg.M, b.Minv)) memset(b.Minv, 0, sizeof(b.Minv));
    b.warped_stride = ((size_t)S * S * 3 + 255) & ~(size_t)255;
    if (b.warped) (void)hipFree(b.warped);
    b.warped = nullptr;
    CBV_HIP(ctx, hipMalloc((void**)&b.warped, b.warped_stride * P.max_frames));
    // squares
    int ws[CBV_MAX_SQUARES], hs[CBV_MAX_SQUARES];
    for (int i = 0; i < n; i++) {
        ws[i] = cfg.rois[i].w;
        hs[i] = cfg.rois[i].h;
    }
    std::vector<u8> masks;
    const size_t off = square_table(ws, hs, n, &b.descs, &masks);
    b.max_px = 0;
    for (int i = 0; i < n; i++) {
        SquareDesc& d = b.descs[i];
        d.cn = 3;
        d.stride = S * 3;
        d.src_off = cfg.rois[i].y0 * S * 3 + cfg.rois[i].x0 * 3;
        b.max_px = std::max(b.max_px, d.w * d.h);
    }
    b.plane_total = off;
    RC(dev_ensure(ctx, &b.d_descs, sizeof(SquareDesc) * n));
    RC(dev_ensure(ctx, &b.d_masks, off));
    RC(dev_ensure(ctx, &b.d_gray, off * P.max_frames));
    if (b.own_blur()) { // a kernel set before this configuration
        RC(dev_ensure(ctx, &b.d_cgray, off * P.max_frames));
        CBV_HIP(ctx, hipMemset(b.d_cgray.p, 0, off * P.max_frames));
    }
    b.slot_blur.assign((size_t)P.max_frames, 0);
    RC(dev_ensure(ctx, &b.d_stats, sizeof(cbv_sq_stats) * n * P.max_frames));
    RC(dev_ensure(ctx, &b.d_ref, off));
    RC(dev_ensure(ctx, &b.d_mean, off * 4));
    RC(dev_ensure(ctx, &b.d_var, off * 8)); // variance plane, then its square root
    b.calibrated = false;
    b.session = false; // a session belongs to the configuration it began on
    RC(dev_ensure(ctx, &b.d_state, sizeof(ScanState) * n));
    RC(dev_ensure(ctx, &b.d_results, sizeof(cbv_frame_result) * P.max_frames));
    const size_t want = sizeof(cbv_frame_result) * (size_t)P.max_frames + 16; // (max_frames is fixed: allocated once)
    if (!b.h_stage) CBV_HIP(ctx, hipHostMalloc((void**)&b.h_stage, want, hipHostMallocDefault));
    memset(b.h_stage, 0, want);
    b.over_h = (u32*)(b.h_stage + ((sizeof(cbv_frame_result) * (size_t)P.max_frames + 7) & ~(size_t)7));
    b.slot_mirrored.assign((size_t)P.max_frames, 0);
    RC(dev_ensure(ctx, &b.d_flags, (size_t)CBV_MAX_SQUARES * P.max_frames));
    RC(dev_ensure(ctx, &b.d_dec, (size_t)CBV_MAX_SQUARES * P.max_frames));
    if (cfg.use_hough) {
        RC(hough_cfg(ctx, &cfg.hough, b.descs, &b.hough_cfg));
        RC(dev_ensure(ctx, &b.d_hough, sizeof(cbv_hough_result) * CBV_MAX_SQUARES * P.max_frames));
        RC(dev_ensure(ctx, &b.d_hough_over, 256));
        CBV_HIP(ctx, hipMemset(b.d_hough_over.p, 0, 256));
        b.hough_cfg.overflow_count = (u32*)b.d_hough_over.p;
    }
    RC(dev_ensure(ctx, &b.d_noise, sizeof(cbv_noise_result) * P.max_frames));
    RC(dev_ensure(ctx, &b.d_noise_state, sizeof(cbv_noise_state)));
    RC(dev_ensure(ctx, &b.d_check, sizeof(u64) * P.max_frames));
    CBV_HIP(ctx, hipMemset(b.d_check.p, 0, sizeof(u64) * P.max_frames));
    b.has_check = false;
    CBV_HIP(ctx, hipMemset(b.d_noise_state.p, 0, sizeof(cbv_noise_state)));
    CBV_HIP(ctx, hipMemcpy(b.d_descs.p, b.descs.data(), sizeof(SquareDesc) * n, hipMemcpyHostToDevice));
    CBV_HIP(ctx, hipMemcpy(b.d_masks.p, masks.data(), off, hipMemcpyHostToDevice));
    CBV_HIP(ctx, hipMemset(b.d_state.p, 0, sizeof(ScanState) * n));
    // plane padding (planes are rounded to 16 B) must read as zero in every frame: k_scan compares whole vectors
    CBV_HIP(ctx, hipMemset(b.d_gray.p, 0, off * P.max_frames));
    CBV_HIP(ctx, hipMemset(b.d_ref.p, 0, off));
    return CBV_OK;
}

// free a board and its handle (board 0's handle too: the pipeline's shared part is freed by its owner)
static void board_free(cbv_pipeline* p)
{
    Board& b = p->b;
    if (b.h_stage) (void)hipHostFree(b.h_stage);
    if (b.warped) (void)hipFree(b.warped);
    DevBuf* bufs[] = {&b.d_descs, &b.d_masks, &b.d_gray, &b.d_stats, &b.d_ref, &b.d_state, &b.d_results, &b.d_flags, &b.d_dec, &b.d_mean,
                      &b.d_var, &b.d_noise, &b.d_noise_state, &b.d_hough, &b.d_check, &b.d_hough_over, &b.d_session, &b.d_hist, &b.d_radar,
                      &b.d_cgray};
    for (auto d : bufs) dev_free(d);
    delete p;
}

extern "C" int cbv_pipeline_create(cbv_ctx* ctx, int w, int h, int max_frames, cbv_pipeline** out)
{
    if (!ctx || !out || w <= 0 || h <= 0 || max_frames <= 0) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_create: bad arguments");
    CBV_ENTER(ctx);
    Pipe* P = new Pipe();
    P->ctx = ctx;
    P->w = w;
    P->h = h;
    P->max_frames = max_frames;
    P->g = tight_geom(w, h);
    hipError_t e = hipMalloc((void**)&P->frames, P->g.frame_stride * max_frames + 256);
    if (e != hipSuccess) {
        const size_t want = P->g.frame_stride * max_frames;
        delete P;
        return cbv_fail(ctx, CBV_ERR_HIP, "hipMalloc of %zu bytes for the frame ring failed: %s", want, hipGetErrorString(e));
    }
    P->boards.push_back(new cbv_pipeline{P, Board()});
    *out = P->boards[0];
    return CBV_OK;
}

extern "C" void cbv_pipeline_destroy(cbv_pipeline* p)
{
    if (!p) return;
    Pipe* P = p->pipe;
    cbv_ctx* ctx = P->ctx;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    if (P->boards.size() > 1) (void)join_scan(*P); // runs in flight (lanes, scan) write every board
    (void)hipStreamSynchronize(ctx->stream);
    if (attached(p)) { // detach: the other boards and board 0 go on as they were
        P->boards.erase(std::find(P->boards.begin(), P->boards.end(), p));
        (void)pipeline_tables(*P);
        (void)pipeline_update_region(*P);
        board_free(p);
        return;
    }
    for (int l = 0; l < Pipe::MAX_LANES; l++) {
        if (P->lane_stream[l]) (void)hipStreamSynchronize(P->lane_stream[l]);
        if (P->A[l]) (void)hipFree(P->A[l]);
        if (P->B[l]) (void)hipFree(P->B[l]);
        if (P->C[l]) (void)hipFree(P->C[l]);
        dev_free(&P->lane_small[l]);
        dev_free(&P->lane_work[l]);
        if (P->lane_done[l]) (void)hipEventDestroy(P->lane_done[l]);
    }
    if (P->start_ev) (void)hipEventDestroy(P->start_ev);
    if (P->scan_stream) (void)hipStreamSynchronize(P->scan_stream); // (the worker streams belong to the context)
    for (auto& r : P->runs) {
        (void)hipEventDestroy(r.lanes_ev);
        (void)hipEventDestroy(r.scan_ev);
        dev_free(&r.retry);
    }
    if (P->main_done) (void)hipEventDestroy(P->main_done);
    if (P->copy_stream) (void)hipStreamSynchronize(P->copy_stream);
    for (auto& c : P->copies) (void)hipEventDestroy(c.ev);
    if (P->host_ring) (void)hipHostFree(P->host_ring);
    if (P->raw_ring) (void)hipFree(P->raw_ring);
    if (P->frames) (void)hipFree(P->frames);
    if (P->enhanced) (void)hipFree(P->enhanced);
    dev_free(&P->d_synth);
    dev_free(&P->d_boards);
    for (cbv_pipeline* q : P->boards) board_free(q); // board 0 (p) included
    delete P;
}

extern "C" void* cbv_pipeline_frames_dev(cbv_pipeline* p) { return p && !attached(p) ? p->pipe->frames : nullptr; }

extern "C" int cbv_pipeline_configure(cbv_pipeline* p, const cbv_pipeline_config* cfg)
{
    if (!p || !cfg) return CBV_ERR_ARG;
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    CBV_ENTER(ctx);
    RC(join_scan(P)); // lanes and scan of the last run
    if (attached(p)) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_configure: a board handle is configured by cbv_pipeline_add_board");
    if (P.boards.size() > 1) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_configure: boards are attached (destroy them first)");
    RC(check_board_cfg(ctx, cfg));
    if (cfg->skip_enhance && cfg->keep_enhanced)
        return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_configure: skip_enhance with keep_enhanced (there is no enhanced frame to keep)");
    if (cfg->skip_enhance && cfg->enhance_region)
        return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_configure: skip_enhance with enhance_region (there is no enhancement to limit)");
    if (!cfg->skip_enhance) RC(check_params(ctx, &cfg->enhance));
    // every argument check that needs no state is done; from here on a failure leaves the pipeline UNconfigured
    // (run / results / ... return CBV_ERR_STATE) instead of half reconfigured
    P.configured = false;
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    P.keep_enhanced = cfg->keep_enhanced != 0;
    P.skip_enhance = cfg->skip_enhance != 0;
    int chunk = cfg->chunk;
    if (chunk <= 0) chunk = 32;
    if (chunk > P.max_frames) chunk = P.max_frames;
    P.chunk = chunk;
    // (re)allocate
    int lanes = cfg->lanes <= 0 ? 2 : cfg->lanes;
    if (lanes > Pipe::MAX_LANES) lanes = Pipe::MAX_LANES;
    if ((P.max_frames + chunk - 1) / chunk < lanes) lanes = (P.max_frames + chunk - 1) / chunk;
    P.n_lanes = lanes;
    for (int l = 0; l < Pipe::MAX_LANES; l++) {
        if (P.A[l]) (void)hipFree(P.A[l]);
        if (P.B[l]) (void)hipFree(P.B[l]);
        if (P.C[l]) (void)hipFree(P.C[l]);
        P.A[l] = P.B[l] = P.C[l] = nullptr;
    }
    if (P.enhanced) (void)hipFree(P.enhanced);
    P.enhanced = nullptr;
    if (!P.start_ev) CBV_HIP(ctx, hipEventCreateWithFlags(&P.start_ev, hipEventDisableTiming));
    if (P.skip_enhance)
        for (int l = 0; l < Pipe::MAX_LANES; l++) dev_free(&P.lane_small[l]);
    for (int l = 0; l < lanes; l++) {
        if (!P.skip_enhance) { // the enhancement's scratch frames, aux blocks and CLAHE tables
            CBV_HIP(ctx, hipMalloc((void**)&P.A[l], P.g.frame_stride * chunk + 256));
            CBV_HIP(ctx, hipMalloc((void**)&P.B[l], P.g.frame_stride * chunk + 256));
            SmallLayout SL;
            RC(small_layout(ctx, &P.lane_small[l], cfg->enhance.tiles_x * cfg->enhance.tiles_y, chunk, &SL, cfg->enhance.tiles_x, cfg->enhance.tiles_y));
        }
        RC(dev_ensure(ctx, &P.lane_work[l], sizeof(u32) * (1 + (size_t)CBV_MAX_SQUARES * chunk)));
        if (l > 0) RC(ctx_worker_stream(ctx, &ctx->lane_streams[l], &P.lane_stream[l]));
        if (!P.lane_done[l]) CBV_HIP(ctx, hipEventCreateWithFlags(&P.lane_done[l], hipEventDisableTiming));
    }
    if (P.keep_enhanced) CBV_HIP(ctx, hipMalloc((void**)&P.enhanced, P.g.frame_stride * P.max_frames + 256));
    RC(board_setup(P, p->b, *cfg));
    // region-limited enhancement: the source footprint of the S x S warp (warp_footprint)
    RC(pipeline_update_region(P));
    RC(pipeline_tables(P));
    P.configured = true;
    return CBV_OK;
}

extern "C" int cbv_pipeline_add_board(cbv_pipeline* p, const cbv_board_config* bc, cbv_pipeline** out)
{
    if (!p || !bc || !out) return cbv_fail(p ? p->pipe->ctx : nullptr, CBV_ERR_ARG, "cbv_pipeline_add_board: bad arguments");
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    CBV_ENTER(ctx);
    if (attached(p)) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_add_board: the parent is itself a board handle");
    if (!P.configured) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_add_board: the parent is not configured");
    if ((int)P.boards.size() >= CBV_MAX_BOARDS)
        return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_add_board: a pipeline holds at most %d boards", CBV_MAX_BOARDS);
    if (P.max_frames >= (1 << (MB_BOARD_SHIFT - 8)))
        return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_add_board: at most %d frames in a pipeline with boards", (1 << (MB_BOARD_SHIFT - 8)) - 1);
    // the board's configuration = the pipeline's with the board's subset replaced
    cbv_pipeline_config cfg = P.b0().cfg;
    memcpy(cfg.M, bc->M, sizeof(cfg.M));
    cfg.board_size = bc->board_size;
    cfg.rot180 = bc->rot180;
    cfg.n_rois = bc->n_rois;
    memcpy(cfg.rois, bc->rois, sizeof(cfg.rois));
    cfg.history_size = bc->history_size;
    cfg.min_presence = bc->min_presence;
    cfg.change_threshold = bc->change_threshold;
    cfg.z_threshold = bc->z_threshold;
    cfg.initial_variance = bc->initial_variance;
    cfg.use_hough = bc->use_hough;
    cfg.hough = bc->hough;
    RC(check_board_cfg(ctx, &cfg));
    if (cfg.use_hough) RC(hough_params_check(ctx, &cfg.hough));
    RC(join_scan(P));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // the lanes' worklists hold every board's items (grown only: a larger list serves fewer boards as well)
    for (int l = 0; l < P.n_lanes; l++)
        RC(dev_ensure(ctx, &P.lane_work[l], sizeof(u32) * (1 + (size_t)CBV_MAX_SQUARES * P.chunk * (P.boards.size() + 1))));
    cbv_pipeline* b = new cbv_pipeline{&P, Board()};
    int rc = board_setup(P, b->b, cfg);
    if (rc == CBV_OK) {
        P.boards.push_back(b);
        rc = pipeline_tables(P);
        if (rc == CBV_OK) rc = pipeline_update_region(P);
        if (rc != CBV_OK) {
            P.boards.pop_back();
            const std::string err = ctx->err;
            (void)pipeline_tables(P);
            (void)pipeline_update_region(P);
            ctx->err = err;
        }
    }
    if (rc != CBV_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        board_free(b);
        return rc;
    }
    *out = b;
    return CBV_OK;
}

extern "C" int cbv_pipeline_reset_state(cbv_pipeline* p)
{
    if (!p || !p->pipe->configured) return CBV_ERR_STATE;
    Pipe& P = *p->pipe;
    Board& B = p->b;
    cbv_ctx* ctx = P.ctx;
    CBV_ENTER(ctx);
    RC(join_scan(P)); // lanes and scan of the last run
    CBV_HIP(ctx, hipMemsetAsync(B.d_state.p, 0, sizeof(ScanState) * B.cfg.n_rois, ctx->stream));
    CBV_HIP(ctx, hipMemsetAsync(B.d_noise_state.p, 0, sizeof(cbv_noise_state), ctx->stream));
    if (B.d_hough_over.p) {
        CBV_HIP(ctx, hipMemsetAsync(B.d_hough_over.p, 0, 4, ctx->stream));
        CBV_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the runs that could still write the mirror's copy are behind us
        *B.over_h = 0;
    }
    return CBV_OK;
}

extern "C" int cbv_pipeline_calibrate(cbv_pipeline* p, int slot)
{
    if (!p || !p->pipe->configured) return CBV_ERR_STATE;
    Pipe& P = *p->pipe;
    Board& B = p->b;
    cbv_ctx* ctx = P.ctx;
    if (slot < 0 || slot >= P.max_frames) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_calibrate: bad slot");
    CBV_ENTER(ctx);
    if (B.slot_blur[slot] && B.slot_blur[slot] != B.change_k)
        return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_calibrate: slot %d was last run with blur kernel %d, the board's is %d now (run the slot again)",
                        slot, (int)B.slot_blur[slot], B.change_k);
    RC(join_scan(P)); // lanes and scan of the last run
    RC(launch_squares_calibrate(ctx, (const SquareDesc*)B.d_descs.p, B.cfg.n_rois, B.change_planes() + B.plane_total * slot,
                                (float*)B.d_mean.p, (float*)B.d_var.p, (float*)B.d_var.p + B.plane_total, (float)B.cfg.initial_variance, nullptr));
    B.calibrated = true;
    return pipeline_tables(P); // the board's statistics read its model from now on
}

extern "C" int cbv_pipeline_set_model_update(cbv_pipeline* p, int mode, double alpha)
{
    if (!p) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_pipeline_set_model_update: the board is null");
    Pipe& P = *p->pipe;
    Board& B = p->b;
    cbv_ctx* ctx = P.ctx;
    if (mode != CBV_MODEL_FROZEN && mode != CBV_MODEL_EVERY && mode != CBV_MODEL_UNCHANGED)
        return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_set_model_update: unknown mode %d", mode);
    if (!(alpha >= 0.0 && alpha <= 1.0)) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_set_model_update: alpha %g is outside [0, 1]", alpha);
    CBV_ENTER(ctx);
    if (B.model_mode == mode && B.model_alpha == alpha) return CBV_OK;
    // The runs in flight keep their arguments, and what comes next is ordered behind their scans: a board that turns
    // frozen has its model read by the lanes of the next run, which fork from this stream.
    RC(join_scan(P));
    B.model_mode = mode;
    B.model_alpha = alpha;
    return P.configured ? pipeline_tables(P) : CBV_OK;
}

extern "C" int cbv_pipeline_set_change_blur(cbv_pipeline* p, int blur_kernel)
{
    if (!p) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_pipeline_set_change_blur: the board is null");
    Pipe& P = *p->pipe;
    Board& B = p->b;
    cbv_ctx* ctx = P.ctx;
    const int k = std::max(blur_kernel, 1) | 1; // calibrate_sensitivity.py:139
    if (k > 31) return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "cbv_pipeline_set_change_blur: blur kernel %d too large (max 31)", k);
    // (REFLECT_101 folds as often as it takes, d_reflect101: every kernel fits every square)
    CBV_ENTER(ctx);
    if (B.change_k == k) return CBV_OK;
    RC(join_scan(P)); // the runs in flight keep their arguments; the tables are rebuilt behind them
    if (k != 5 && P.configured) { // the board's own plane ring (kept from an earlier kernel other than 5)
        RC(dev_ensure(ctx, &B.d_cgray, B.plane_total * P.max_frames));
        if (!B.own_blur()) CBV_HIP(ctx, hipMemsetAsync(B.d_cgray.p, 0, B.plane_total * P.max_frames, ctx->stream));
    }
    B.change_k = k;
    return P.configured ? pipeline_tables(P) : CBV_OK;
}

extern "C" int cbv_pipeline_model(cbv_pipeline* p, int which, int roi, float* out)
{
    if (!p || !out) return cbv_fail(p ? p->pipe->ctx : nullptr, CBV_ERR_ARG, "cbv_pipeline_model: null argument");
    Pipe& P = *p->pipe;
    const Board& B = p->b;
    cbv_ctx* ctx = P.ctx;
    if (!P.configured || !B.calibrated) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_model: the board is not calibrated");
    if ((which != 0 && which != 1) || roi < 0 || roi >= B.cfg.n_rois) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_model: bad plane %d or square %d", which, roi);
    CBV_ENTER(ctx);
    RC(join_scan(P)); // the model scans of the runs in flight
    const SquareDesc& d = B.descs[roi];
    const float* src = (const float*)(which == 0 ? B.d_mean.p : B.d_var.p) + d.plane_off;
    CBV_HIP(ctx, hipMemcpyAsync(out, src, sizeof(float) * d.w * d.h, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

// ---------------------------------------------------------------------------
// The ChangeDetector sensitivity sweep (include/cbv.h, cbv_pipeline_sweep; kernels in k_sweep.hip).  Everything it allocates
// belongs to the call and is freed when it returns; of the board it reads the warped ring, the square table and slot_blur.
// ---------------------------------------------------------------------------
namespace {
struct SweepCall {
    DevBuf planes, sets, kbeg, hist, rec, sums;
    u8* h_rec = nullptr; // pinned staging of a chunk's records
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    ~SweepCall()
    {
        for (DevBuf* b : {&planes, &sets, &kbeg, &hist, &rec, &sums}) dev_free(b);
        if (h_rec) (void)hipHostFree(h_rec);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};
} // namespace

// `hist_out` != null: cbv_pipeline_change_hist (one frame, one kernel, no evaluation)
static int sweep_run(cbv_pipeline* p, const char* who, int calib_slot, int slot0, int count, const cbv_sweep_setting* settings, int ns,
                     int chunk, cbv_sweep_record* records, cbv_sweep_summary* summaries, cbv_sweep_info* info, u16* hist_out)
{
    if (!p) return cbv_fail(nullptr, CBV_ERR_ARG, "%s: the board is null", who);
    Pipe& P = *p->pipe;
    const Board& B = p->b;
    cbv_ctx* ctx = P.ctx;
    if (!P.configured) return cbv_fail(ctx, CBV_ERR_STATE, "%s: the pipeline is not configured", who);
    if (!settings || ns <= 0 || count <= 0) return cbv_fail(ctx, CBV_ERR_ARG, "%s: no settings or no frames", who);
    if (ns > CBV_SWEEP_MAX_SETTINGS) return cbv_fail(ctx, CBV_ERR_ARG, "%s: %d settings (at most %d)", who, ns, CBV_SWEEP_MAX_SETTINGS);
    if (chunk < 0 || chunk > CBV_SWEEP_MAX_CHUNK) return cbv_fail(ctx, CBV_ERR_ARG, "%s: chunk_frames %d is outside 0..%d", who, chunk, CBV_SWEEP_MAX_CHUNK);
    if (calib_slot < 0 || calib_slot >= P.max_frames || slot0 < 0 || slot0 > P.max_frames - count)
        return cbv_fail(ctx, CBV_ERR_ARG, "%s: slots outside the ring of %d", who, P.max_frames);
    std::vector<int> ks;
    for (int i = 0; i < ns; i++) {
        const float ivf = (float)settings[i].initial_variance;
        if (!(ivf > 0.f) || !(ivf <= 3.402823466e38f))
            return cbv_fail(ctx, CBV_ERR_ARG, "%s: initial_variance %g of setting %d is not a positive finite float32", who, settings[i].initial_variance, i);
        ks.push_back(std::max(settings[i].blur_kernel, 1) | 1);
    }
    std::vector<int> kd(ks);
    std::sort(kd.begin(), kd.end());
    kd.erase(std::unique(kd.begin(), kd.end()), kd.end());
    if (kd.back() > 31) return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "%s: blur kernel %d too large (max 31)", who, kd.back());
    CBV_ENTER(ctx);
    if (!B.slot_blur[calib_slot]) return cbv_fail(ctx, CBV_ERR_STATE, "%s: slot %d was never run", who, calib_slot);
    for (int i = 0; i < count; i++)
        if (!B.slot_blur[slot0 + i]) return cbv_fail(ctx, CBV_ERR_STATE, "%s: slot %d was never run", who, slot0 + i);
    RC(join_scan(P)); // lanes of the runs in flight write the warped ring
    const int nk = (int)kd.size(), n = B.cfg.n_rois;
    if (chunk == 0) chunk = CBV_SWEEP_DEFAULT_CHUNK;
    chunk = std::min(chunk, count);
    // the settings by kernel, each with its place in the caller's list
    std::vector<SweepSet> sets;
    std::vector<int> kbeg(1, 0);
    int max_per_k = 0;
    for (int ki = 0; ki < nk; ki++) {
        for (int i = 0; i < ns; i++)
            if (ks[i] == kd[ki]) sets.push_back(SweepSet{(float)settings[i].z_threshold, (float)settings[i].initial_variance, (u32)i});
        kbeg.push_back((int)sets.size());
        max_per_k = std::max(max_per_k, kbeg[ki + 1] - kbeg[ki]);
    }
    SweepCall S;
    const bool eval = hist_out == nullptr;
    RC(dev_ensure(ctx, &S.planes, B.plane_total * nk));
    RC(dev_ensure(ctx, &S.hist, sizeof(u16) * SWEEP_HIST_WORDS * nk * chunk));
    if (eval) {
        RC(dev_ensure(ctx, &S.sets, sizeof(SweepSet) * ns));
        RC(dev_ensure(ctx, &S.kbeg, sizeof(int) * (nk + 1)));
        CBV_HIP(ctx, hipMemcpyAsync(S.sets.p, sets.data(), sizeof(SweepSet) * ns, hipMemcpyHostToDevice, ctx->stream));
        CBV_HIP(ctx, hipMemcpyAsync(S.kbeg.p, kbeg.data(), sizeof(int) * (nk + 1), hipMemcpyHostToDevice, ctx->stream));
        if (summaries) {
            RC(dev_ensure(ctx, &S.sums, sizeof(cbv_sweep_summary) * ns));
            CBV_HIP(ctx, hipMemsetAsync(S.sums.p, 0, sizeof(cbv_sweep_summary) * ns, ctx->stream));
        }
        if (records) {
            RC(dev_ensure(ctx, &S.rec, sizeof(cbv_sweep_record) * ns * chunk));
            CBV_HIP(ctx, hipHostMalloc((void**)&S.h_rec, sizeof(cbv_sweep_record) * ns * chunk, hipHostMallocDefault));
        }
    }
    for (hipEvent_t& e : S.ev) CBV_HIP(ctx, hipEventCreate(&e));
    const SquareDesc* descs = (const SquareDesc*)B.d_descs.p;
    float ms = 0.f, planes_ms = 0.f, hist_ms = 0.f, eval_ms = 0.f;
    // the calibration planes: ChangeDetector._preprocess of the calibration slot's squares under each kernel
    CBV_HIP(ctx, hipEventRecord(S.ev[0], ctx->stream));
    for (int ki = 0; ki < nk; ki++)
        RC(launch_change_blur_stats(ctx, B.warped + B.warped_stride * calib_slot, B.warped_stride, descs, n, (u8*)S.planes.p + B.plane_total * ki,
                                    B.plane_total, nullptr, nullptr, 0.f, nullptr, 1, nullptr, change_blur_coef(kd[ki]), B.max_px));
    CBV_HIP(ctx, hipEventRecord(S.ev[1], ctx->stream));
    CBV_HIP(ctx, hipEventSynchronize(S.ev[1]));
    CBV_HIP(ctx, hipEventElapsedTime(&planes_ms, S.ev[0], S.ev[1]));
    for (int c0 = 0; c0 < count; c0 += chunk) {
        const int cf = std::min(chunk, count - c0);
        CBV_HIP(ctx, hipEventRecord(S.ev[0], ctx->stream));
        for (int ki = 0; ki < nk; ki++)
            RC(launch_change_hist(ctx, B.warped + B.warped_stride * (slot0 + c0), B.warped_stride, descs, n, (const u8*)S.planes.p + B.plane_total * ki,
                                  (u16*)S.hist.p + (size_t)SWEEP_HIST_WORDS * ki, (size_t)SWEEP_HIST_WORDS * nk, cf, change_blur_coef(kd[ki]), B.max_px));
        CBV_HIP(ctx, hipEventRecord(S.ev[1], ctx->stream));
        if (eval)
            RC(launch_sweep_eval(ctx, (const u16*)S.hist.p, nk, descs, n, (const SweepSet*)S.sets.p, (const int*)S.kbeg.p, max_per_k, cf,
                                 (cbv_sweep_record*)S.rec.p, chunk, (cbv_sweep_summary*)S.sums.p));
        CBV_HIP(ctx, hipEventRecord(S.ev[2], ctx->stream));
        if (eval && records) CBV_HIP(ctx, hipMemcpyAsync(S.h_rec, S.rec.p, sizeof(cbv_sweep_record) * ns * chunk, hipMemcpyDeviceToHost, ctx->stream));
        CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        CBV_HIP(ctx, hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
        hist_ms += ms;
        CBV_HIP(ctx, hipEventElapsedTime(&ms, S.ev[1], S.ev[2]));
        eval_ms += ms;
        if (eval && records)
            for (int s = 0; s < ns; s++)
                memcpy(records + (size_t)s * count + c0, (const cbv_sweep_record*)S.h_rec + (size_t)s * chunk, sizeof(cbv_sweep_record) * cf);
    }
    if (eval && summaries) CBV_HIP(ctx, hipMemcpy(summaries, S.sums.p, sizeof(cbv_sweep_summary) * ns, hipMemcpyDeviceToHost));
    if (hist_out) CBV_HIP(ctx, hipMemcpy(hist_out, S.hist.p, sizeof(u16) * 256 * n, hipMemcpyDeviceToHost));
    if (info) {
        info->planes_ms = planes_ms;
        info->hist_ms = hist_ms;
        info->eval_ms = eval_ms;
        info->kernels_distinct = nk;
        info->chunk_frames = chunk;
    }
    return CBV_OK;
}

extern "C" int cbv_pipeline_sweep(cbv_pipeline* p, int calib_slot, int slot0, int count, const cbv_sweep_setting* settings, int ns, int chunk_frames,
                                  cbv_sweep_record* records, cbv_sweep_summary* summaries, cbv_sweep_info* info)
{
    return sweep_run(p, "cbv_pipeline_sweep", calib_slot, slot0, count, settings, ns, chunk_frames, records, summaries, info, nullptr);
}

extern "C" int cbv_pipeline_change_hist(cbv_pipeline* p, int calib_slot, int slot, int blur_kernel, uint16_t* out)
{
    if (!out) return cbv_fail(p ? p->pipe->ctx : nullptr, CBV_ERR_ARG, "cbv_pipeline_change_hist: null argument");
    const cbv_sweep_setting one = {0.0, 1.0, blur_kernel, 0};
    return sweep_run(p, "cbv_pipeline_change_hist", calib_slot, slot, 1, &one, 1, 1, nullptr, nullptr, nullptr, out);
}

// ---------------------------------------------------------------------------
// The PieceDetector settings sweep (include/cbv.h, cbv_pipeline_piece_sweep; kernels in k_piece_sweep.hip).  Everything it
// allocates belongs to the call and is freed when it returns; of the board it reads the gray ring, the square table, the
// statistics of the slots and slot_blur.
// ---------------------------------------------------------------------------
namespace {
struct PieceSweepCall {
    DevBuf sets, choices, hist, sums, rec, expected;
    u8* h_rec = nullptr; // pinned staging of a chunk's records
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    ~PieceSweepCall()
    {
        for (DevBuf* b : {&sets, &choices, &hist, &sums, &rec, &expected}) dev_free(b);
        if (h_rec) (void)hipHostFree(h_rec);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};
} // namespace

// `choices_out` != null: cbv_pipeline_piece_detail (one setting, one frame: the circle choices, no evaluation)
static int piece_sweep_run(cbv_pipeline* p, const char* who, int slot0, int count, const cbv_hough_params* settings, int ns, const uint64_t* expected,
                           int chunk, cbv_piece_sweep_record* records, cbv_piece_sweep_summary* summary, cbv_piece_sweep_info* info,
                           PieceChoice* choices_out)
{
    if (!p) return cbv_fail(nullptr, CBV_ERR_ARG, "%s: the board is null", who);
    Pipe& P = *p->pipe;
    const Board& B = p->b;
    cbv_ctx* ctx = P.ctx;
    if (!P.configured) return cbv_fail(ctx, CBV_ERR_STATE, "%s: the pipeline is not configured", who);
    if (!settings || ns <= 0 || count <= 0 || (!summary && !choices_out)) return cbv_fail(ctx, CBV_ERR_ARG, "%s: no settings, no frames or no summary", who);
    if (ns > CBV_PIECE_SWEEP_MAX_SETTINGS) return cbv_fail(ctx, CBV_ERR_ARG, "%s: %d settings (at most %d)", who, ns, CBV_PIECE_SWEEP_MAX_SETTINGS);
    if (chunk < 0 || chunk > CBV_SWEEP_MAX_CHUNK) return cbv_fail(ctx, CBV_ERR_ARG, "%s: chunk_frames %d is outside 0..%d", who, chunk, CBV_SWEEP_MAX_CHUNK);
    if (slot0 < 0 || slot0 > P.max_frames - count) return cbv_fail(ctx, CBV_ERR_ARG, "%s: slots outside the ring of %d", who, P.max_frames);
    const int n = B.cfg.n_rois;
    HoughCfg hc;
    memset(&hc, 0, sizeof(hc));
    for (const SquareDesc& d : B.descs) {
        hc.maxw = std::max(hc.maxw, d.w);
        hc.maxh = std::max(hc.maxh, d.h);
    }
    // the settings as the kernel reads them (the casts of hough_cfg), with the layout's worst case over them
    std::vector<PieceSet> sets((size_t)ns);
    for (int i = 0; i < ns; i++) {
        const cbv_hough_params& s = settings[i];
        const bool finite = std::isfinite(s.dp) && std::isfinite(s.param1) && std::isfinite(s.param2) && std::isfinite(s.min_radius_ratio) &&
                            std::isfinite(s.max_radius_ratio);
        if (!finite || !(s.dp > 0) || !(s.param1 > 0) || !(s.param2 > 0) || !(s.min_radius_ratio >= 0) || !(s.max_radius_ratio >= 0))
            return cbv_fail(ctx, CBV_ERR_ARG, "%s: setting %d is invalid (dp %g, param1 %g, param2 %g, ratios %g %g)", who, i, s.dp, s.param1, s.param2,
                            s.min_radius_ratio, s.max_radius_ratio);
        RC(hough_params_check(ctx, &s));
        if (s.min_radius_ratio > 1.0 || s.max_radius_ratio > 1.0) // the radius histogram of the layout is sized for radii inside the square
            return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "%s: setting %d has a radius ratio above 1 (%g, %g)", who, i, s.min_radius_ratio, s.max_radius_ratio);
        if (s.dp > 16.0) // the narrowest radius span is 2: round(2 / dp * 10) bins must be at least one
            return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "%s: setting %d has dp %g (at most 16)", who, i, s.dp);
        PieceSet& t = sets[(size_t)i];
        t.dp = (float)s.dp < 1.f ? 1.f : (float)s.dp;
        t.canny_thr = (int)nearbyint(s.param1);
        t.acc_thr = (int)nearbyint(s.param2);
        t.index = (u32)i;
        t.min_ratio = s.min_radius_ratio;
        t.max_ratio = s.max_radius_ratio;
        hc.dp = i == 0 ? t.dp : std::min(hc.dp, t.dp);
    }
    // The radius histogram of the layout is sized for the widest span any setting can ask of any square: maxRadius is the
    // square's larger side whenever int(min_dim * max_ratio) is 0 (ratios below 1 / min_dim, the trackbars' first positions),
    // and min_radius + 2 when it does not exceed the minimum, so with ratios up to 1 the span is at most max(w, h) + 2:
    // ratios of 0 make hough_layout take that span.
    hc.min_ratio = hc.max_ratio = 0;
    {
        HoughCfg probe = hc;
        int off = 0;
        if (hc.maxw < 2 || hc.maxh < 2 || hc.maxw > 250 || hc.maxh > 250 || piece_sweep_layout(&probe, &off) > 150 * 1024)
            return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "%s: %dx%d squares do not fit the LDS layout of the sweep", who, hc.maxw, hc.maxh);
    }
    CBV_ENTER(ctx);
    for (int i = 0; i < count; i++)
        if (!B.slot_blur[slot0 + i]) return cbv_fail(ctx, CBV_ERR_STATE, "%s: slot %d was never run", who, slot0 + i);
    RC(join_scan(P)); // the runs in flight write the gray ring and the statistics
    // front end shared first (dp, param1), then the accumulator (the integer radii of the first square), then param2
    const int md0 = std::min(B.descs[0].w, B.descs[0].h);
    std::stable_sort(sets.begin(), sets.end(), [md0](const PieceSet& a, const PieceSet& b) {
        if (a.dp != b.dp) return a.dp < b.dp;
        if (a.canny_thr != b.canny_thr) return a.canny_thr < b.canny_thr;
        const int a0 = (int)(md0 * a.min_ratio), b0 = (int)(md0 * b.min_ratio), a1 = (int)(md0 * a.max_ratio), b1 = (int)(md0 * b.max_ratio);
        if (a0 != b0) return a0 < b0;
        if (a1 != b1) return a1 < b1;
        if (a.min_ratio != b.min_ratio) return a.min_ratio < b.min_ratio;
        if (a.max_ratio != b.max_ratio) return a.max_ratio < b.max_ratio;
        return a.acc_thr < b.acc_thr;
    });
    int p1_distinct = 0;
    for (int i = 0; i < ns; i++)
        if (i == 0 || sets[i].dp != sets[i - 1].dp || sets[i].canny_thr != sets[i - 1].canny_thr) p1_distinct++;
    if (chunk == 0) chunk = CBV_SWEEP_DEFAULT_CHUNK;
    chunk = std::min(chunk, count);
    const bool eval = choices_out == nullptr;
    PieceSweepCall S;
    RC(dev_ensure(ctx, &S.sets, sizeof(PieceSet) * ns));
    CBV_HIP(ctx, hipMemcpy(S.sets.p, sets.data(), sizeof(PieceSet) * ns, hipMemcpyHostToDevice)); // (pageable sources: copied before the call returns)
    const size_t choice_bytes = sizeof(PieceChoice) * CBV_MAX_SQUARES * (size_t)ns * chunk;
    RC(dev_ensure(ctx, &S.choices, choice_bytes));
    CBV_HIP(ctx, hipMemsetAsync(S.choices.p, 0, choice_bytes, ctx->stream));
    if (eval) {
        RC(dev_ensure(ctx, &S.hist, sizeof(u32) * CBV_MAX_SQUARES * ns));
        CBV_HIP(ctx, hipMemsetAsync(S.hist.p, 0, sizeof(u32) * CBV_MAX_SQUARES * ns, ctx->stream));
        RC(dev_ensure(ctx, &S.sums, sizeof(cbv_piece_sweep_summary) * ns));
        CBV_HIP(ctx, hipMemsetAsync(S.sums.p, 0, sizeof(cbv_piece_sweep_summary) * ns, ctx->stream));
        if (expected) {
            RC(dev_ensure(ctx, &S.expected, sizeof(u64) * count));
            CBV_HIP(ctx, hipMemcpy(S.expected.p, expected, sizeof(u64) * count, hipMemcpyHostToDevice));
        }
        if (records) {
            RC(dev_ensure(ctx, &S.rec, sizeof(cbv_piece_sweep_record) * ns * chunk));
            CBV_HIP(ctx, hipHostMalloc((void**)&S.h_rec, sizeof(cbv_piece_sweep_record) * ns * chunk, hipHostMallocDefault));
        }
    }
    for (hipEvent_t& e : S.ev) CBV_HIP(ctx, hipEventCreate(&e));
    const SquareDesc* descs = (const SquareDesc*)B.d_descs.p;
    float ms = 0.f, hough_ms = 0.f, eval_ms = 0.f;
    for (int c0 = 0; c0 < count; c0 += chunk) {
        const int cf = std::min(chunk, count - c0);
        const cbv_sq_stats* stats = (const cbv_sq_stats*)B.d_stats.p + (size_t)n * (slot0 + c0);
        CBV_HIP(ctx, hipEventRecord(S.ev[0], ctx->stream));
        RC(launch_piece_sweep_hough(ctx, descs, n, (const u8*)B.d_gray.p + B.plane_total * (slot0 + c0), B.plane_total, stats, hc,
                                    (const PieceSet*)S.sets.p, ns, cf, (PieceChoice*)S.choices.p, chunk));
        CBV_HIP(ctx, hipEventRecord(S.ev[1], ctx->stream));
        if (eval)
            RC(launch_piece_sweep_eval(ctx, descs, n, stats, (const PieceChoice*)S.choices.p, chunk, cf, ns,
                                       expected ? (const u64*)S.expected.p + c0 : nullptr, (u32*)S.hist.p, (cbv_piece_sweep_record*)S.rec.p, chunk,
                                       (cbv_piece_sweep_summary*)S.sums.p));
        CBV_HIP(ctx, hipEventRecord(S.ev[2], ctx->stream));
        if (eval && records) CBV_HIP(ctx, hipMemcpyAsync(S.h_rec, S.rec.p, sizeof(cbv_piece_sweep_record) * ns * chunk, hipMemcpyDeviceToHost, ctx->stream));
        CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        CBV_HIP(ctx, hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
        hough_ms += ms;
        CBV_HIP(ctx, hipEventElapsedTime(&ms, S.ev[1], S.ev[2]));
        eval_ms += ms;
        if (eval && records)
            for (int s = 0; s < ns; s++)
                memcpy(records + (size_t)s * count + c0, (const cbv_piece_sweep_record*)S.h_rec + (size_t)s * chunk, sizeof(cbv_piece_sweep_record) * cf);
    }
    if (eval) CBV_HIP(ctx, hipMemcpy(summary, S.sums.p, sizeof(cbv_piece_sweep_summary) * ns, hipMemcpyDeviceToHost));
    if (choices_out) CBV_HIP(ctx, hipMemcpy(choices_out, S.choices.p, sizeof(PieceChoice) * CBV_MAX_SQUARES, hipMemcpyDeviceToHost));
    if (info) {
        info->hough_ms = hough_ms;
        info->eval_ms = eval_ms;
        info->param1_distinct = p1_distinct;
        info->chunk_frames = chunk;
    }
    return CBV_OK;
}

extern "C" int cbv_pipeline_piece_sweep(cbv_pipeline* p, int slot0, int count, const cbv_hough_params* settings, int ns, const uint64_t* expected,
                                        int chunk_frames, cbv_piece_sweep_record* records, cbv_piece_sweep_summary* summary,
                                        cbv_piece_sweep_info* info)
{
    return piece_sweep_run(p, "cbv_pipeline_piece_sweep", slot0, count, settings, ns, expected, chunk_frames, records, summary, info, nullptr);
}

extern "C" int cbv_pipeline_piece_detail(cbv_pipeline* p, int slot, const cbv_hough_params* setting, cbv_piece_result* out)
{
    if (!out) return cbv_fail(p ? p->pipe->ctx : nullptr, CBV_ERR_ARG, "cbv_pipeline_piece_detail: null argument");
    PieceChoice ch[CBV_MAX_SQUARES];
    RC(piece_sweep_run(p, "cbv_pipeline_piece_detail", slot, 1, setting, 1, nullptr, 1, nullptr, nullptr, nullptr, ch));
    const Board& B = p->b;
    cbv_ctx* ctx = p->pipe->ctx;
    const int n = B.cfg.n_rois;
    std::vector<cbv_sq_stats> st((size_t)n);
    {
        CBV_ENTER(ctx);
        CBV_HIP(ctx, hipMemcpy(st.data(), (const cbv_sq_stats*)B.d_stats.p + (size_t)n * slot, sizeof(cbv_sq_stats) * n, hipMemcpyDeviceToHost));
    }
    bool over = false;
    for (int i = 0; i < n; i++) {
        memset(&out[i], 0, sizeof(out[i]));
        piece_decide_choice(&st[(size_t)i], ch[i], B.descs[i].w, B.descs[i].h, &out[i]);
        out[i].should_process = out[i].evaluated = 1;
        over = over || (ch[i].flags & CBV_HOUGH_OVERFLOW);
    }
    if (over) return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "cbv_pipeline_piece_detail: a HoughCircles candidate list overflowed");
    return CBV_OK;
}

extern "C" int cbv_pipeline_update_references(cbv_pipeline* p, int slot, int reset_noise)
{
    if (!p || !p->pipe->configured) return CBV_ERR_STATE;
    Pipe& P = *p->pipe;
    Board& B = p->b;
    cbv_ctx* ctx = P.ctx;
    if (slot < 0 || slot >= P.max_frames) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_update_references: bad slot");
    CBV_ENTER(ctx);
    RC(join_scan(P)); // lanes and scan of the last run
    RC(launch_scan_update_refs(ctx, (const SquareDesc*)B.d_descs.p, B.cfg.n_rois, (const u8*)B.d_gray.p + B.plane_total * slot,
                               (u8*)B.d_ref.p, (ScanState*)B.d_state.p));
    if (reset_noise) CBV_HIP(ctx, hipMemsetAsync(B.d_noise_state.p, 0, sizeof(cbv_noise_state), ctx->stream)); // NoiseHandler.reset()
    return CBV_OK;
}

// the raw-frame mode (Pipe::raw_mode) has no BGR frames to write
static const char* const kRawModeMsg = "the pipeline runs without enhancement on a YUV input format (raw mode): its frames are the raw "
                                       "ring, written by cbv_pipeline_upload_raw or cbv_pipeline_submit in that format";

// the planes of slot `slot` of the device ring of raw frames
static RawPlanes slot_planes(const Pipe& P, int slot)
{
    return tight_raw_planes(P.in_fmt, P.w, P.h, P.raw_ring + tight_raw_geom(P.in_fmt, P.w, P.h).frame_stride * slot);
}

// the device ring of raw frames in the current (YUV) input format
static int ensure_raw_ring(Pipe& P)
{
    cbv_ctx* ctx = P.ctx;
    if (P.raw_ring) return CBV_OK;
    const size_t bytes = tight_raw_geom(P.in_fmt, P.w, P.h).frame_stride * P.max_frames;
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
    if (P.raw_mode()) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_upload: %s", kRawModeMsg);
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

// bytes between the slots of the ingest rings in the current input format
static size_t host_slot_bytes(const Pipe& P) { return P.in_fmt == CBV_FMT_BGR ? P.g.frame_stride : tight_raw_geom(P.in_fmt, P.w, P.h).frame_stride; }

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
    if (fmt != CBV_FMT_BGR) RC(check_raw_format(ctx, fmt, P.w, P.h, "cbv_pipeline_set_input_format"));
    CBV_ENTER(ctx);
    // the copies and conversions in flight read the rings that go away here (both run on the copy stream)
    if (P.copy_stream) CBV_HIP(ctx, hipStreamSynchronize(P.copy_stream));
    if (P.raw_mode()) { // ... and so do the runs in flight
        RC(join_scan(P));
        CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (P.host_ring) (void)hipHostFree(P.host_ring);
    if (P.raw_ring) (void)hipFree(P.raw_ring);
    P.host_ring = P.raw_ring = nullptr;
    P.in_fmt = fmt;
    return CBV_OK;
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
    if (P.in_fmt == CBV_FMT_BGR) {
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
    if (P.raw_mode()) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_synth: %s", kRawModeMsg);
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

// the per-board stages of a chunk of b frames from slot s0 (warp, square statistics, HoughCircles' first pass): with boards
// attached one launch each for all of them, otherwise the single-board launches with board 0's arguments
// (res = the BGR frames the warp samples; in raw mode null, and the warp samples the chunk's slots of the raw ring)
static int pipeline_chunk_boards(Pipe& P, const u8* res, NormSrc norm, int s0, int b, u32* work, u32* retry0, u32* retry, int retry_base)
{
    cbv_ctx* ctx = P.ctx;
    RawGeom rg = {};
    RawPlanes raw = {{nullptr, nullptr, nullptr}}; // raw mode: the planes of the chunk's first slot
    if (!res) {
        rg = tight_raw_geom(P.in_fmt, P.w, P.h);
        raw = slot_planes(P, s0);
    }
    const u8* raw0 = raw.p[0];
    if (P.boards.size() > 1) {
        const BoardDev* tab = (const BoardDev*)P.d_boards.p;
        const int nb = (int)P.boards.size();
        if (raw0) RC(launch_warp_yuv_mb(ctx, raw, rg, P.g, tab, nb, P.max_S, s0, b, work, retry0));
        else RC(launch_warp_mb(ctx, res, P.g, tab, nb, P.max_S, s0, norm, b, work, retry0));
        RC(launch_squares_pre5_stats_mb(ctx, tab, nb, s0, b, P.any_hough, work, P.max_px));
        if (P.any_own_blur) RC(launch_change_blur_stats_mb(ctx, tab, nb, s0, b, P.max_px));
        if (P.any_hough) RC(launch_hough_mb(ctx, tab, nb, s0, work, CBV_MAX_SQUARES * nb * b, P.hough_lds[0], retry, retry_base, 0));
        return CBV_OK;
    }
    const BoardDev& T = P.tab[0];
    u8* wdst = T.warped + T.warped_stride * s0;
    u8* gray = T.gray + T.plane_total * s0;
    u8* dec = T.dec + (size_t)CBV_MAX_SQUARES * s0;
    cbv_hough_result* hres = T.hough ? T.hough + (size_t)CBV_MAX_SQUARES * s0 : nullptr;
    if (raw0) RC(launch_warp_yuv(ctx, raw, rg, P.g, T.Minv, T.S, T.S, T.rot180, wdst, T.S * 3, T.warped_stride, b, work, retry0));
    else RC(launch_warp(ctx, res, P.g, T.Minv, T.S, T.S, T.rot180, wdst, T.S * 3, T.warped_stride, norm, b, work, retry0));
    RC(launch_squares_pre5_stats(ctx, wdst, T.warped_stride, T.descs, T.n, gray, T.plane_total, T.mean, T.sd, T.masks, T.z_thresh,
                                 T.stats + (size_t)T.n * s0, b, dec, T.want_hough, work, hres, P.b0().max_px));
    if (P.any_own_blur)
        RC(launch_change_blur_stats(ctx, wdst, T.warped_stride, T.descs, T.n, T.cgray + T.plane_total * s0, T.plane_total, T.cmean, T.csd,
                                    T.z_thresh, T.stats + (size_t)T.n * s0, b, dec, T.cb, P.b0().max_px));
    if (T.want_hough) RC(launch_hough(ctx, T.descs, T.n, gray, T.plane_total, P.b0().hough_cfg, hres, dec, work, b, retry, retry_base));
    return CBV_OK;
}

// mark slots [s0, s0 + cnt) of every board as held (or not) by the pinned result mirror
static void mark_mirrored(Pipe& P, int s0, int cnt, bool held)
{
    for (cbv_pipeline* q : P.boards) std::fill(q->b.slot_mirrored.begin() + s0, q->b.slot_mirrored.begin() + s0 + cnt, held ? 1 : 0);
}

// The scan stage of ONE board for a run: HoughCircles' second pass and the model scan (`with_pre`: not yet done by the
// multi-board launches), the temporal scan, packing and NoiseHandler; with a game session the rounds of k_session.hip.
static int board_scan(Pipe& P, Board& q, const BoardDev& T, int slot0, int count, bool mirrored, bool with_pre, const u32* retry)
{
    cbv_ctx* ctx = P.ctx;
    const u8* gray = T.gray + T.plane_total * slot0;
    u8* dec = T.dec + (size_t)CBV_MAX_SQUARES * slot0;
    u8* flags = T.flags + (size_t)CBV_MAX_SQUARES * slot0;
    if (with_pre && T.want_hough)
        RC(launch_hough_second(ctx, T.descs, T.n, gray, T.plane_total, q.hough_cfg, T.hough + (size_t)CBV_MAX_SQUARES * slot0, dec,
                               retry, T.n * count));
    if (with_pre && q.adaptive())
        RC(launch_model_scan(ctx, T.descs, T.n, T.cgray + T.plane_total * slot0, T.plane_total, T.ms, T.stats + (size_t)T.n * slot0, dec, count,
                             q.max_px));
    ResultMirror mir;
    if (mirrored) {
        mir.records = T.mirror + slot0;
        mir.over_src = T.over_src;
        mir.over_dst = T.over_dst;
    }
    const u64* check = q.has_check ? T.check + slot0 : nullptr;
    if (!q.session)
        return launch_scan(ctx, T.descs, T.sp, gray, T.plane_total, dec, T.ref, T.state, flags, T.results + slot0, count, check, T.noise_state,
                           T.noise + slot0, mir);
    // Two accepted moves are at least `gap` frames apart, so `len` frames hold at most ceil(len / gap) of them, and one more
    // round finishes behind the last; rounds that find the frames finished return at once.
    const int gap = std::max(q.ses_cfg.stability_required, q.ses_cfg.cooldown_frames + 1);
    SessionDev* ses = (SessionDev*)q.d_session.p;
    u16* hist = (u16*)q.d_hist.p + (size_t)CBV_MAX_SQUARES * slot0;
    cbv_session_radar* radar = q.ses_cfg.radar ? (cbv_session_radar*)q.d_radar.p + slot0 : nullptr;
    // The run is cut at the board events that fall inside it (cbv_pipeline_session_sync): an event changes the smart mask,
    // so the frames behind it must not be scanned with the check sets of the board that was.  Each segment is the rounds
    // above on its own frames, k_session_event sits between them on the same stream, and nothing waits for the host.  With
    // no event due the one segment is the run.
    const int c0 = q.ses_frames; // session frame index of the run's first frame
    size_t e = 0;
    for (int a = 0; a < count;) {
        for (; e < q.ses_events.size() && q.ses_events[e].at_frame <= c0 + a; e++) {
            prof_begin(ctx, CBV_K_SCAN);
            RC(launch_session_event(ctx, ses, &q.ses_events[e]));
            prof_end(ctx, CBV_K_SCAN);
        }
        int b = count;
        if (e < q.ses_events.size() && q.ses_events[e].at_frame < c0 + count) b = q.ses_events[e].at_frame - c0;
        const int len = b - a;
        ResultMirror smir = mir;
        if (smir.records) smir.records += a;
        const size_t sq0 = (size_t)CBV_MAX_SQUARES * a;
        for (int k = 0, nr = 1 + (len + gap - 1) / gap; k < nr; k++) {
            prof_begin(ctx, CBV_K_SCAN);
            RC(launch_scan_session(ctx, T.descs, T.sp, gray + T.plane_total * a, T.plane_total, dec + sq0, T.ref, T.state, flags + sq0, len,
                                   check ? check + a : nullptr, ses, k == 0, hist + sq0));
            RC(launch_session_walk(ctx, flags + sq0, T.n, T.results + slot0 + a, len, T.noise_state, T.noise + slot0 + a, smir, ses, k == 0,
                                   radar ? radar + a : nullptr));
            prof_end(ctx, CBV_K_SCAN);
        }
        a = b;
    }
    q.ses_events.erase(q.ses_events.begin(), q.ses_events.begin() + e);
    q.ses_frames += count;
    return CBV_OK;
}

// second half of cbv_pipeline_run: join the lanes on the scan's stream, HoughCircles second pass, temporal scan, run record
static int pipeline_run_tail(Pipe& P, Pipe::RunRec* rec, int slot0, int count, bool inline_scan, const bool* lane_used, hipStream_t main_stream)
{
    cbv_ctx* ctx = P.ctx;
    if (!P.scan_stream) {
        RC(ctx_worker_stream(ctx, &ctx->scan_stream, &P.scan_stream));
        CBV_HIP(ctx, hipEventCreateWithFlags(&P.main_done, hipEventDisableTiming));
    }
    hipStream_t scan_on = inline_scan ? main_stream : P.scan_stream;
    if (!inline_scan) {
        CBV_HIP(ctx, hipEventRecord(P.main_done, main_stream));
        CBV_HIP(ctx, hipStreamWaitEvent(scan_on, P.main_done, 0));
    }
    // every forked lane is joined, in the inline case too (chunk = 1 puts the second frame of a two-frame run on lane 1)
    for (int l = 1; l < P.n_lanes; l++)
        if (lane_used[l]) {
            CBV_HIP(ctx, hipEventRecord(P.lane_done[l], P.lane_stream[l]));
            CBV_HIP(ctx, hipStreamWaitEvent(scan_on, P.lane_done[l], 0));
        }
    // every lane has read its frames: a later cbv_pipeline_submit may overwrite these slots after this event
    rec->one_event = inline_scan;
    if (!inline_scan) CBV_HIP(ctx, hipEventRecord(rec->lanes_ev, scan_on));
    ctx->stream = scan_on;
    struct Restore {
        cbv_ctx* c;
        hipStream_t s;
        ~Restore() { c->stream = s; }
    } restore{ctx, main_stream};
    // A short run (the live-camera case) writes its records to the pinned mirror too: reading them back is then a wait and a
    // host copy instead of two more launches.  Not the long runs: their records would cross PCIe as thousands of 8-byte
    // writes inside the scan stream's critical path (512-frame steps: -0.5 % frames/s, alternating A/B runs); they are
    // fetched with one copy when asked for.
    const bool mirrored = count <= 4;
    if (P.any_session) { // boards with a game session scan in rounds of their own: every board's scan is launched by itself
        const int nb = (int)P.boards.size();
        if (nb > 1) {
            const BoardDev* tab = (const BoardDev*)P.d_boards.p;
            if (P.any_hough)
                RC(launch_hough_mb(ctx, tab, nb, slot0, (const u32*)rec->retry.p, CBV_MAX_SQUARES * nb * count, P.hough_lds[1], nullptr, 0, 1));
            if (P.any_adaptive) RC(launch_model_scan_mb(ctx, tab, nb, slot0, count, P.max_px));
        }
        for (int k = 0; k < nb; k++) RC(board_scan(P, P.boards[k]->b, P.tab[k], slot0, count, mirrored, nb == 1, (const u32*)rec->retry.p));
    } else if (P.boards.size() > 1) { // every board's second pass, scan, packing and NoiseHandler: one launch each
        const BoardDev* tab = (const BoardDev*)P.d_boards.p;
        const int nb = (int)P.boards.size();
        if (P.any_hough)
            RC(launch_hough_mb(ctx, tab, nb, slot0, (const u32*)rec->retry.p, CBV_MAX_SQUARES * nb * count, P.hough_lds[1], nullptr, 0, 1));
        if (P.any_adaptive) RC(launch_model_scan_mb(ctx, tab, nb, slot0, count, P.max_px));
        RC(launch_scan_mb(ctx, tab, nb, slot0, count, mirrored ? 1 : 0));
    } else {
        const BoardDev& T = P.tab[0];
        const u8* gray = T.gray + T.plane_total * slot0;
        u8* dec = T.dec + (size_t)CBV_MAX_SQUARES * slot0;
        if (T.want_hough) // squares whose first HoughCircles pass overflowed (normally none), before the scan reads the decisions
            RC(launch_hough_second(ctx, T.descs, T.n, gray, T.plane_total, P.b0().hough_cfg, T.hough + (size_t)CBV_MAX_SQUARES * slot0, dec,
                                   (const u32*)rec->retry.p, T.n * count));
        // the z-score statistics and the model update of a board whose model follows the frames, before the scan reads the classes
        if (P.any_adaptive)
            RC(launch_model_scan(ctx, T.descs, T.n, T.cgray + T.plane_total * slot0, T.plane_total, T.ms, T.stats + (size_t)T.n * slot0, dec, count,
                                 P.b0().max_px));
        ResultMirror mir;
        if (mirrored) {
            mir.records = T.mirror + slot0;
            mir.over_src = T.over_src;
            mir.over_dst = T.over_dst;
        }
        // + NoiseHandler on the frames' visual_changes sets (game_session.py:165)
        RC(launch_scan(ctx, T.descs, T.sp, gray, T.plane_total, dec, T.ref, T.state, T.flags + (size_t)CBV_MAX_SQUARES * slot0,
                       T.results + slot0, count, P.b0().has_check ? T.check + slot0 : nullptr, T.noise_state, T.noise + slot0, mir));
    }
    CBV_HIP(ctx, hipEventRecord(rec->scan_ev, scan_on));
    mark_mirrored(P, slot0, count, mirrored);
    for (cbv_pipeline* q : P.boards) std::fill(q->b.slot_blur.begin() + slot0, q->b.slot_blur.begin() + slot0 + count, (u8)q->b.change_k);
    rec->s0 = slot0;
    rec->cnt = count;
    rec->seq = ++P.run_seq;
    rec->live = true;
    return CBV_OK;
}

extern "C" int cbv_pipeline_run(cbv_pipeline* p, int slot0, int count)
{
    if (!p || !p->pipe->configured) return CBV_ERR_STATE;
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    if (attached(p)) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_run: a board is run by its parent");
    if (slot0 < 0 || count <= 0 || slot0 + count > P.max_frames) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_run: bad slot range");
    CBV_ENTER(ctx);
    if (P.raw_mode() && !P.raw_ring) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_run: no raw frame was ever uploaded or submitted");
    const cbv_enhance_params& enh = P.b0().cfg.enhance;
    // Lane 0 is the context's stream; lanes 1.. are worker streams forked from it and joined before
    // the temporal scan (which needs every frame's statistics, in order).
    hipStream_t main_stream = ctx->stream;
    // A run of one or two frames (the live-camera case) is latency, not throughput: its scan is a few microseconds, less
    // than the hop to the scan stream and back, so everything stays on the caller's stream, behind every run in flight
    // (the scans' state is sequential over runs).
    const bool inline_scan = count <= 2;
    const int chunks = (count + P.chunk - 1) / P.chunk;
    // Chunks go round the lanes, and the round continues from run to run and from pipeline to pipeline of this context
    // (ctx->lane_rr): K camera streams whose runs are one chunk each would otherwise all pile on lane 0 and lose the
    // overlap of the lanes.  Short (latency) runs start on the caller's stream.
    const int lane_base = inline_scan ? 0 : ctx->lane_rr % P.n_lanes;
    if (!inline_scan) ctx->lane_rr = (ctx->lane_rr + chunks) % (12 * 1024);
    bool lane_used[Pipe::MAX_LANES] = {false, false, false, false};
    for (int c = 0; c < chunks && c < P.n_lanes; c++) lane_used[(lane_base + c) % P.n_lanes] = true;
    if (inline_scan) {
        retire_runs(P);
        RC(join_scan(P));
    } else RC(join_slots(P, slot0, count)); // scans in flight that still read these slots' planes, however many runs back
    // until this run's scan is enqueued, the results of its slots come from the device (a failed run leaves them so)
    mark_mirrored(P, slot0, count, false);
    Pipe::RunRec* rec = nullptr; // the record (and second-pass list) of this run
    for (auto& r : P.runs)
        if (!r.live) {
            rec = &r;
            break;
        }
    if (!rec) {
        Pipe::RunRec r{0, 0, 0, nullptr, nullptr, false, false, DevBuf()};
        CBV_HIP(ctx, hipEventCreateWithFlags(&r.lanes_ev, hipEventDisableTiming));
        CBV_HIP(ctx, hipEventCreateWithFlags(&r.scan_ev, hipEventDisableTiming));
        P.runs.push_back(r);
        rec = &P.runs.back();
    }
    // the second-pass list's counter: zeroed before the lanes fork from this stream, or, when the run is ONE chunk, by that
    // chunk's k_warp (a memset is a launch of its own, ~13 us with its bubble in front of a 150 us chain)
    const bool retry_zero_in_warp = chunks == 1;
    if (P.any_hough) {
        RC(dev_ensure(ctx, &rec->retry, sizeof(u32) * (1 + (size_t)CBV_MAX_SQUARES * P.max_frames * P.boards.size())));
        if (!retry_zero_in_warp) CBV_HIP(ctx, hipMemsetAsync(rec->retry.p, 0, sizeof(u32), main_stream));
    }
    for (auto& c : P.copies) // ingest copies of these slots must have landed
        if (c.pending && ranges_overlap(slot0, count, c.s0, c.cnt)) {
            CBV_HIP(ctx, hipStreamWaitEvent(main_stream, c.ev, 0));
            c.pending = false;
        }
    bool forked = false;
    for (int l = 1; l < P.n_lanes; l++) forked = forked || lane_used[l];
    if (forked) {
        CBV_HIP(ctx, hipEventRecord(P.start_ev, main_stream));
        for (int l = 1; l < P.n_lanes; l++)
            if (lane_used[l]) CBV_HIP(ctx, hipStreamWaitEvent(P.lane_stream[l], P.start_ev, 0));
    }
    int ci = 0, rc_all = CBV_OK;
    for (int s0 = slot0; s0 < slot0 + count && rc_all == CBV_OK; s0 += P.chunk, ci++) {
        const int lane = (lane_base + ci) % P.n_lanes;
        ctx->stream = lane == 0 ? main_stream : P.lane_stream[lane];
        const int b = std::min(P.chunk, slot0 + count - s0);
        const u8* src = P.frames + P.g.frame_stride * s0;
        u32* work = P.any_hough ? (u32*)P.lane_work[lane].p : nullptr; // worklist counter: zeroed by k_warp
        u32* retry0 = P.any_hough && retry_zero_in_warp ? (u32*)rec->retry.p : nullptr;
        if (P.skip_enhance) { // the session's chain: the warp samples the frames as they are (in raw mode the raw ring: no BGR source)
            rc_all = pipeline_chunk_boards(P, P.raw_mode() ? nullptr : src, NormSrc(), s0, b, work, retry0, (u32*)rec->retry.p, s0 - slot0);
            continue;
        }
        SmallLayout SL;
        rc_all = small_layout(ctx, &P.lane_small[lane], enh.tiles_x * enh.tiles_y, P.chunk, &SL, enh.tiles_x, enh.tiles_y);
        if (rc_all) break;
        u8* res = nullptr;
        NormSrc norm;
        rc_all = enhance_dev(ctx, src, P.A[lane], P.B[lane], P.g, &enh, SL, b, !P.keep_enhanced, &res, &norm,
                             P.use_region ? &P.region : nullptr, P.C[lane]);
        if (rc_all) break;
        if (P.keep_enhanced) {
            if (hipMemcpyAsync(P.enhanced + P.g.frame_stride * s0, res, P.g.frame_stride * b, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) {
                rc_all = cbv_fail(ctx, CBV_ERR_HIP, "copy of the enhanced frames failed");
                break;
            }
        }
        rc_all = pipeline_chunk_boards(P, res, P.keep_enhanced ? NormSrc() : norm, s0, b, work, retry0, (u32*)rec->retry.p, s0 - slot0);
    }
    ctx->stream = main_stream;
    // A failure after lanes were forked: whatever they already enqueued on these slots and scratch buffers must not outlive
    // the call unordered (no RunRec goes live for a failed run), whether a lane's launch failed or the join / scan below did.
    auto drain = [&](int rc) {
        ctx->stream = main_stream;
        for (int l = 1; l < P.n_lanes; l++)
            if (lane_used[l]) (void)hipStreamSynchronize(P.lane_stream[l]);
        if (P.scan_stream) (void)hipStreamSynchronize(P.scan_stream);
        (void)hipStreamSynchronize(main_stream);
        return rc;
    };
    if (rc_all) return drain(rc_all);
    const int rc_tail = pipeline_run_tail(P, rec, slot0, count, inline_scan, lane_used, main_stream);
    return rc_tail == CBV_OK ? CBV_OK : drain(rc_tail);
}

extern "C" int cbv_pipeline_set_check_squares(cbv_pipeline* p, int slot0, int count, const uint64_t* roi_masks)
{
    if (!p || !p->pipe->configured || slot0 < 0 || count <= 0 || slot0 + count > p->pipe->max_frames) return CBV_ERR_ARG;
    Pipe& P = *p->pipe;
    Board& B = p->b;
    cbv_ctx* ctx = P.ctx;
    CBV_ENTER(ctx);
    if (B.session && B.ses_cfg.smart_scan)
        return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_set_check_squares: the board runs a game session with smart_scan, which owns its "
                                            "check sets (cbv_pipeline_session_begin with smart_scan = 0 leaves them to the caller)");
    RC(join_scan(P)); // the last run's scan may still read the masks
    if (roi_masks) {
        CBV_HIP(ctx, hipMemcpyAsync((u64*)B.d_check.p + slot0, roi_masks, sizeof(u64) * count, hipMemcpyHostToDevice, ctx->stream));
        CBV_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the caller's buffer may go away
        B.has_check = true;
    } else CBV_HIP(ctx, hipMemsetAsync((u64*)B.d_check.p + slot0, 0, sizeof(u64) * count, ctx->stream));
    return CBV_OK;
}

extern "C" int cbv_pipeline_results(cbv_pipeline* p, int slot0, int count, cbv_frame_result* out)
{
    if (!p || !out || slot0 < 0 || count <= 0 || slot0 + count > p->pipe->max_frames) return CBV_ERR_ARG;
    Pipe& P = *p->pipe;
    Board& B = p->b;
    cbv_ctx* ctx = P.ctx;
    CBV_ENTER(ctx);
    RC(join_scan(P)); // lanes and scan of the last run
    if (!P.configured || !B.h_stage) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_results: the pipeline is not configured");
    // short runs left their records in pinned host memory (ResultMirror): wait for the runs, copy on the host; the others
    // are fetched into the same place first (through pinned memory in any case: a copy into the caller's pageable buffer
    // would be staged by the runtime, one blocking copy at a time)
    const size_t bytes = sizeof(cbv_frame_result) * (size_t)count;
    bool have = true;
    for (int t = 0; t < count; t++) have = have && B.slot_mirrored[(size_t)slot0 + t];
    if (!have) {
        CBV_HIP(ctx, hipMemcpyAsync((cbv_frame_result*)B.h_stage + slot0, (cbv_frame_result*)B.d_results.p + slot0, bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (B.cfg.use_hough && B.d_hough_over.p) CBV_HIP(ctx, hipMemcpyAsync(B.over_h, B.d_hough_over.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (!have)
        for (int t = 0; t < count; t++) B.slot_mirrored[(size_t)slot0 + t] = 1;
    memcpy(out, (const cbv_frame_result*)B.h_stage + slot0, bytes);
    const u32 over = *B.over_h;
    if (over) {
        // A truncated candidate list may change has_piece: never hand that over as if it were HoughCircles' answer.  The
        // counter is cleared on read, so the error is reported ONCE, by the first results call after the runs it
        // happened in, and later frames are not poisoned; `out` is filled and valid except for the flagged squares.
        CBV_HIP(ctx, hipMemsetAsync(B.d_hough_over.p, 0, 4, ctx->stream));
        *B.over_h = 0; // (nothing is in flight: the next run's last kernel writes the word again)
        return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "HoughCircles: the candidate list overflowed even the second pass on %u square(s) since the "
                        "previous cbv_pipeline_results; those occupancy bits are not HoughCircles' (cbv_pipeline_hough flags name the squares)", over);
    }
    return CBV_OK;
}

extern "C" int cbv_pipeline_noise_results(cbv_pipeline* p, int slot0, int count, cbv_noise_result* out)
{
    if (!p || !out || !p->pipe->configured || slot0 < 0 || count <= 0 || slot0 + count > p->pipe->max_frames) return CBV_ERR_ARG;
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    CBV_ENTER(ctx);
    RC(join_scan(P)); // lanes and scan of the last run
    CBV_HIP(ctx, hipMemcpyAsync(out, (cbv_noise_result*)p->b.d_noise.p + slot0, sizeof(cbv_noise_result) * count, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

extern "C" int cbv_pipeline_download(cbv_pipeline* p, int which, int slot, uint8_t* out)
{
    if (!p || !out || slot < 0 || slot >= p->pipe->max_frames) return CBV_ERR_ARG;
    Pipe& P = *p->pipe;
    const Board& B = p->b;
    cbv_ctx* ctx = P.ctx;
    CBV_ENTER(ctx);
    RC(join_scan(P)); // lanes and scan of the last run
    const u8* src;
    size_t bytes;
    if (attached(p) && which != 2) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_download: a board holds only its warped frames (which = 2)");
    if (which == 0) {
        src = P.frames + P.g.frame_stride * slot;
        bytes = (size_t)P.w * P.h * 3;
        if (P.raw_mode()) { // the frames are raw: the slot is converted for the caller
            if (!P.raw_ring) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_download: no raw frame was ever uploaded or submitted");
            if (P.copy_stream) CBV_HIP(ctx, hipStreamSynchronize(P.copy_stream)); // submitted copies of the slot
            const RawGeom rg = tight_raw_geom(P.in_fmt, P.w, P.h);
            RC(dev_ensure(ctx, &ctx->a, P.g.frame_stride + 256));
            RC(launch_ingest(ctx, slot_planes(P, slot), rg, (u8*)ctx->a.p, P.g, 1));
            src = (const u8*)ctx->a.p;
        }
    } else if (which == 1) {
        if (P.skip_enhance) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_download: the pipeline runs without enhancement (skip_enhance): there are no enhanced frames");
        if (!P.enhanced) return cbv_fail(ctx, CBV_ERR_STATE, "enhanced frames are not kept (configure with keep_enhanced = 1)");
        src = P.enhanced + P.g.frame_stride * slot;
        bytes = (size_t)P.w * P.h * 3;
    } else if (which == 2) {
        if (!B.warped) return cbv_fail(ctx, CBV_ERR_STATE, "pipeline not configured");
        src = B.warped + B.warped_stride * slot;
        bytes = (size_t)B.cfg.board_size * B.cfg.board_size * 3;
    } else
        return cbv_fail(ctx, CBV_ERR_ARG, "bad buffer selector %d", which);
    CBV_HIP(ctx, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

extern "C" int cbv_pipeline_hough(cbv_pipeline* p, int slot, cbv_hough_result* out)
{
    if (!p || !out || slot < 0 || slot >= p->pipe->max_frames) return CBV_ERR_ARG;
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    if (!P.configured || !p->b.cfg.use_hough) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_hough: the HoughCircles stage is not configured");
    CBV_ENTER(ctx);
    RC(join_scan(P)); // lanes and scan of the last run
    CBV_HIP(ctx, hipMemcpyAsync(out, (const cbv_hough_result*)p->b.d_hough.p + (size_t)CBV_MAX_SQUARES * slot,
                                sizeof(cbv_hough_result) * CBV_MAX_SQUARES, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

extern "C" int cbv_pipeline_square_stats(cbv_pipeline* p, int slot, cbv_sq_stats* out)
{
    if (!p || !out || !p->pipe->configured || slot < 0 || slot >= p->pipe->max_frames) return CBV_ERR_ARG;
    Pipe& P = *p->pipe;
    const Board& B = p->b;
    cbv_ctx* ctx = P.ctx;
    CBV_ENTER(ctx);
    RC(join_scan(P)); // lanes and scan of the last run
    CBV_HIP(ctx, hipMemcpyAsync(out, (cbv_sq_stats*)B.d_stats.p + (size_t)B.cfg.n_rois * slot, sizeof(cbv_sq_stats) * B.cfg.n_rois,
                                hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

// ---------------------------------------------------------------------------
// game session (include/cbv.h): begin / end / moves / state
// ---------------------------------------------------------------------------
static int session_sync(Pipe& P)
{
    cbv_ctx* ctx = P.ctx;
    RC(join_scan(P)); // lanes and scans of the runs in flight
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

extern "C" int cbv_pipeline_session_begin(cbv_pipeline* p, const cbv_session_config* cfg, const char* fen)
{
    if (!p || !cfg) return cbv_fail(p ? p->pipe->ctx : nullptr, CBV_ERR_ARG, "cbv_pipeline_session_begin: null argument");
    Pipe& P = *p->pipe;
    Board& B = p->b;
    cbv_ctx* ctx = P.ctx;
    if (!P.configured) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_session_begin: the pipeline is not configured");
    if (B.cfg.n_rois != 64) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_session_begin: a game session needs the 64 squares of a board, this one has %d", B.cfg.n_rois);
    // (the frame counts are bounded so that board_scan's round count stays far inside an int)
    const int frames_max = 1 << 24;
    if ((cfg->rule != CBV_SESSION_RULE_INFER && cfg->rule != CBV_SESSION_RULE_OCCUPANCY) || cfg->stability_required < 1 ||
        cfg->stability_required > frames_max || cfg->cooldown_frames < 0 || cfg->cooldown_frames > frames_max || cfg->scan_period < 0 || cfg->max_diff < 0 ||
        !ses_config_ok(cfg))
        return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_session_begin: bad configuration (rule %d, stability_required %d, cooldown_frames %d, scan_period %d, max_diff %d, "
                        "online %d, radar %d; online needs CBV_SESSION_RULE_INFER)",
                        cfg->rule, cfg->stability_required, cfg->cooldown_frames, cfg->scan_period, cfg->max_diff, cfg->online, cfg->radar);
    std::vector<SessionDev> host(1);
    memset(host.data(), 0, sizeof(SessionDev));
    host[0].cfg = *cfg;
    if (cbv_session_state_init(&host[0].st, fen) != 0) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_session_begin: not a FEN: %s", fen ? fen : "(null)");
    host[0].st.waiting_for_opponent = ses_initial_waiting(cfg, &host[0].st);
    CBV_ENTER(ctx);
    RC(session_sync(P));
    RC(dev_ensure(ctx, &B.d_session, sizeof(SessionDev)));
    RC(dev_ensure(ctx, &B.d_hist, sizeof(u16) * CBV_MAX_SQUARES * (size_t)P.max_frames));
    if (cfg->radar) {
        RC(dev_ensure(ctx, &B.d_radar, sizeof(cbv_session_radar) * (size_t)P.max_frames));
        CBV_HIP(ctx, hipMemset(B.d_radar.p, 0, sizeof(cbv_session_radar) * (size_t)P.max_frames));
    }
    B.ses_events.clear();
    B.ses_frames = 0;
    CBV_HIP(ctx, hipMemcpy(B.d_session.p, host.data(), sizeof(SessionDev), hipMemcpyHostToDevice));
    B.session = true;
    B.ses_cfg = *cfg;
    B.ses_drained = 0;
    return pipeline_tables(P);
}

extern "C" int cbv_pipeline_session_end(cbv_pipeline* p)
{
    if (!p) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_pipeline_session_end: the board is null");
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    if (!p->b.session) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_session_end: no session is running on this board");
    CBV_ENTER(ctx);
    RC(session_sync(P));
    p->b.session = false;
    p->b.ses_events.clear();
    return pipeline_tables(P);
}

extern "C" int cbv_pipeline_session_sync(cbv_pipeline* p, int at_frame, const cbv_session_pos* pos, int waiting_for_opponent)
{
    if (!p || !pos) return cbv_fail(p ? p->pipe->ctx : nullptr, CBV_ERR_ARG, "cbv_pipeline_session_sync: null argument");
    cbv_ctx* ctx = p->pipe->ctx;
    Board& B = p->b;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu); // (host state only: no device call, no wait)
    if (!B.session) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_session_sync: no session is running on this board");
    cbv_session_event ev;
    ev.at_frame = at_frame;
    ev.waiting_for_opponent = waiting_for_opponent ? 1 : 0;
    ev.pos = *pos;
    bool kings[2] = {false, false};
    for (int i = 0; i < 64; i++) {
        const int pc = pos->sq[i];
        if (pc < 0 || (pc & 7) > 6 || (pc && !(pc & 7))) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_session_sync: square %d holds %d, not a piece", i, pc);
        if ((pc & 7) == 6) kings[(pc & 8) ? 1 : 0] = true;
    }
    if (!kings[0] || !kings[1] || (pos->turn != 0 && pos->turn != 1) || pos->ep < -1 || pos->ep > 63 || (pos->castling & ~15))
        return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_session_sync: not a position (build it with cbv_session_pos_from_moves)");
    const int last = B.ses_events.empty() ? B.ses_frames : B.ses_events.back().at_frame;
    const int rc = ses_events_check(B.ses_frames, last, (int)B.ses_events.size(), &ev, 1);
    if (rc == CBV_ERR_ARG)
        return cbv_fail(ctx, rc, "cbv_pipeline_session_sync: at_frame %d lies in front of %s %d", at_frame,
                        at_frame < B.ses_frames ? "the session's next frame" : "the last queued event's frame", at_frame < B.ses_frames ? B.ses_frames : last);
    if (rc != CBV_OK) return cbv_fail(ctx, rc, "cbv_pipeline_session_sync: %d events are waiting, the queue is full", (int)B.ses_events.size());
    B.ses_events.push_back(ev);
    return CBV_OK;
}

extern "C" int cbv_pipeline_session_frames(cbv_pipeline* p, int* frames)
{
    if (!p || !frames) return cbv_fail(p ? p->pipe->ctx : nullptr, CBV_ERR_ARG, "cbv_pipeline_session_frames: null argument");
    cbv_ctx* ctx = p->pipe->ctx;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    if (!p->b.session) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_session_frames: no session is running on this board");
    *frames = p->b.ses_frames;
    return CBV_OK;
}

extern "C" int cbv_pipeline_session_radar(cbv_pipeline* p, int slot0, int n, cbv_session_radar* out)
{
    if (!p || !out) return cbv_fail(p ? p->pipe->ctx : nullptr, CBV_ERR_ARG, "cbv_pipeline_session_radar: null argument");
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    if (!p->b.session || !p->b.ses_cfg.radar)
        return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_session_radar: no session with radar = 1 is running on this board");
    if (slot0 < 0 || n <= 0 || slot0 + n > P.max_frames) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_session_radar: bad slot range");
    CBV_ENTER(ctx);
    RC(join_scan(P));
    CBV_HIP(ctx, hipMemcpyAsync(out, (cbv_session_radar*)p->b.d_radar.p + slot0, sizeof(cbv_session_radar) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

static int session_fetch(cbv_pipeline* p, const char* who, std::vector<SessionDev>& host)
{
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    if (!p->b.session) return cbv_fail(ctx, CBV_ERR_STATE, "%s: no session is running on this board", who);
    RC(join_scan(P));
    host.resize(1);
    CBV_HIP(ctx, hipMemcpyAsync(host.data(), p->b.d_session.p, sizeof(SessionDev), hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

extern "C" int cbv_pipeline_session_moves(cbv_pipeline* p, cbv_session_move* out, int cap, int* n)
{
    if (n) *n = 0;
    if (!p || !out || cap < 0 || !n) return cbv_fail(p ? p->pipe->ctx : nullptr, CBV_ERR_ARG, "cbv_pipeline_session_moves: bad arguments");
    cbv_ctx* ctx = p->pipe->ctx;
    CBV_ENTER(ctx);
    std::vector<SessionDev> host;
    RC(session_fetch(p, "cbv_pipeline_session_moves", host));
    const int total = host[0].st.n_moves;
    int first = p->b.ses_drained;
    const int waiting = total - first;
    const int keep = std::min(std::min(waiting, cap), (int)CBV_SESSION_RING);
    first = total - keep; // the newest `keep`
    for (int k = 0; k < keep; k++) out[k] = host[0].ring[(u32)(first + k) % CBV_SESSION_RING];
    *n = keep;
    p->b.ses_drained = total;
    if (keep < waiting)
        return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "cbv_pipeline_session_moves: %d moves were waiting, the newest %d are returned (the ring holds %d)", waiting, keep,
                        (int)CBV_SESSION_RING);
    return CBV_OK;
}

extern "C" int cbv_pipeline_session_state(cbv_pipeline* p, cbv_session_state* out)
{
    if (!p || !out) return cbv_fail(p ? p->pipe->ctx : nullptr, CBV_ERR_ARG, "cbv_pipeline_session_state: null argument");
    cbv_ctx* ctx = p->pipe->ctx;
    CBV_ENTER(ctx);
    std::vector<SessionDev> host;
    RC(session_fetch(p, "cbv_pipeline_session_state", host));
    *out = host[0].st;
    return CBV_OK;
}

static int session_legal_setup(cbv_ctx* ctx, const char* fen, const char* who)
{
    cbv_session_state st;
    if (!fen || cbv_session_state_init(&st, fen) != 0) return cbv_fail(ctx, CBV_ERR_ARG, "%s: not a FEN", who);
    RC(dev_ensure(ctx, &ctx->a, sizeof(cbv_session_state) + sizeof(u16) * CBV_MAX_MOVES + 16));
    CBV_HIP(ctx, hipMemcpyAsync(ctx->a.p, &st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (st is a local)
    return CBV_OK;
}

extern "C" int cbv_session_device_legal_moves(cbv_ctx* ctx, const char* fen, uint16_t* out, int cap, int* n)
{
    if (!ctx || !out || cap < 0 || !n) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_session_device_legal_moves: bad arguments");
    CBV_ENTER(ctx);
    RC(session_legal_setup(ctx, fen, "cbv_session_device_legal_moves"));
    u8* base = (u8*)ctx->a.p;
    u16* d_out = (u16*)(base + sizeof(cbv_session_state));
    int* d_n = (int*)(base + sizeof(cbv_session_state) + sizeof(u16) * CBV_MAX_MOVES);
    RC(launch_session_legal(ctx, (const cbv_session_state*)base, d_out, d_n, 1));
    std::vector<u16> host(CBV_MAX_MOVES + 2);
    CBV_HIP(ctx, hipMemcpyAsync(host.data(), d_out, sizeof(u16) * CBV_MAX_MOVES + sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    int cnt;
    memcpy(&cnt, host.data() + CBV_MAX_MOVES, sizeof(int));
    *n = cnt;
    for (int i = 0; i < cnt && i < cap && i < CBV_MAX_MOVES; i++) out[i] = host[i];
    return CBV_OK;
}

extern "C" int cbv_session_generator_time(cbv_ctx* ctx, const char* fen, int reps, double* ms)
{
    if (!ctx || reps < 1 || reps > (1 << 20) || !ms) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_session_generator_time: bad arguments");
    CBV_ENTER(ctx);
    RC(session_legal_setup(ctx, fen, "cbv_session_generator_time"));
    u8* base = (u8*)ctx->a.p;
    hipEvent_t e0, e1;
    CBV_HIP(ctx, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) {
        (void)hipEventDestroy(e0);
        return cbv_fail(ctx, CBV_ERR_HIP, "cbv_session_generator_time: hipEventCreate failed");
    }
    (void)hipEventRecord(e0, ctx->stream);
    const int rc = launch_session_legal(ctx, (const cbv_session_state*)base, (u16*)(base + sizeof(cbv_session_state)),
                                        (int*)(base + sizeof(cbv_session_state) + sizeof(u16) * CBV_MAX_MOVES), reps);
    (void)hipEventRecord(e1, ctx->stream);
    (void)hipStreamSynchronize(ctx->stream);
    float f = 0;
    (void)hipEventElapsedTime(&f, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *ms = f;
    return rc;
}
