// Device-resident batched pipeline (include/cbv.h, cbv_pipeline_*): frame ring, enhancement lanes, temporal scan, and the
// boards one camera frame feeds (cbv_pipeline_add_board).
#include "cbv_pipeline.h"

// a handle of a board attached by cbv_pipeline_add_board (not board 0, which stands for the whole pipeline)
bool attached(const cbv_pipeline* p) { return p != p->pipe->boards[0]; }

Pipe* frames_owner(cbv_pipeline* p, const char* who, const char* null_msg, int* rc)
{
    *rc = !p ? (null_msg ? cbv_fail(nullptr, CBV_ERR_ARG, "%s: %s", who, null_msg) : CBV_ERR_ARG)
             : attached(p) ? cbv_fail(p->pipe->ctx, CBV_ERR_STATE, "%s: frames go to the parent of a board", who) : CBV_OK;
    return *rc ? nullptr : p->pipe;
}

bool ranges_overlap(int a0, int an, int b0, int bn) { return a0 < b0 + bn && b0 < a0 + an; }

void retire_runs(Pipe& P)
{
    for (auto& r : P.runs)
        if (r.live && hipEventQuery(r.scan_ev) == hipSuccess) r.live = false;
}

// newest record that is still in flight, newer than run `after`, and overlaps the slots (cnt <= 0: any slots)
Pipe::RunRec* newest_run(Pipe& P, int s0, int cnt, unsigned long long after)
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
int join_scan(Pipe& P)
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
int join_slots(Pipe& P, int s0, int cnt)
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

// read device memory into a host buffer behind every run in flight; returns when the bytes are there
int pipeline_readback(Pipe& P, void* out, const void* dev, size_t bytes)
{
    cbv_ctx* ctx = P.ctx;
    RC(join_scan(P));
    CBV_HIP(ctx, hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

// kernel arguments of k_change_blur_stats for an odd k in 1..31: the centre tap and the taps on one side of it
ChangeBlur change_blur_coef(int k)
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
    warp_block_shape(T.S, T.S, &T.bw0, &T.bh0); // as launch_warp cuts an S x S destination
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
    T.ptabs = (const ProfileTabs*)q.d_ptabs.p;
    T.tone_sums = q.tones ? (cbv_tone_sums*)q.d_tone_sums.p : nullptr;
    T.tone_res = q.tones ? (cbv_tone_result*)q.d_tone_res.p : nullptr;
    T.tone_model = q.tones ? (const cbv_tone_model*)q.d_tone_model.p : nullptr;
    return T;
}

// Rebuild the boards' kernel arguments whenever a board is set up, attached, detached or calibrated, or its model-update
// mode or its ChangeDetector blur kernel changes, and upload them as the device table (one small copy and a wait, never
// in the frame chain), for a single board too.  Nothing may be in flight: the callers joined the runs.
int pipeline_tables(Pipe& P)
{
    cbv_ctx* ctx = P.ctx;
    const int nb = (int)P.boards.size();
    P.tab.resize(nb);
    P.any_hough = P.any_adaptive = P.any_session = P.any_own_blur = P.profile_on = P.any_tones = false;
    P.hough_lds[0] = P.hough_lds[1] = 0;
    P.max_px = P.max_S = P.n_squares = 0;
    for (int k = 0; k < nb; k++) {
        const Board& q = P.boards[k]->b;
        size_t lds[2];
        P.tab[k] = board_dev(q, lds);
        if (q.cfg.use_hough) {
            // (a single board is configured with such squares, and cbv_pipeline_run refuses it)
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
        P.any_tones = P.any_tones || q.tones;
        P.profile_on = P.profile_on || (P.profile_only && q.profile.enabled); // no board has one: the plain warp, no table is read
        P.max_px = std::max(P.max_px, q.max_px);
        P.max_S = std::max(P.max_S, q.cfg.board_size);
        P.n_squares += q.cfg.n_rois;
    }
    if (P.lens_on) { // the lens kernels' table: the warp's part of every board, a single one included
        std::vector<LensBoard> lt((size_t)nb);
        for (int k = 0; k < nb; k++) {
            const BoardDev& T = P.tab[k];
            lt[k] = lens_board(T.Minv, T.S, T.S, T.rot180, T.warped, T.S * 3, T.warped_stride, T.ptabs);
        }
        RC(dev_ensure(ctx, &P.d_lens_tab, sizeof(LensBoard) * nb));
        CBV_HIP(ctx, hipMemcpyAsync(P.d_lens_tab.p, lt.data(), sizeof(LensBoard) * nb, hipMemcpyHostToDevice, ctx->stream));
        CBV_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (lt is on this stack)
    }
    RC(dev_ensure(ctx, &P.d_boards, sizeof(BoardDev) * nb));
    CBV_HIP(ctx, hipMemcpyAsync(P.d_boards.p, P.tab.data(), sizeof(BoardDev) * nb, hipMemcpyHostToDevice, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

// enhance_region: the bounding rectangle of every board's warp footprint (any board without one: the whole frame); the
// third scratch frame set is allocated when the region first becomes usable
int pipeline_update_region(Pipe& P)
{
    cbv_ctx* ctx = P.ctx;
    const cbv_pipeline_config& cfg = P.b0().cfg;
    bool use = cfg.enhance_region && !P.keep_enhanced && sharpen_region_ok(cfg.enhance.sharpen_kernel);
    PxRect u = {0, 0, 0, 0};
    for (size_t k = 0; use && k < P.boards.size(); k++) {
        const Board& q = P.boards[k]->b;
        PxRect r;
        use = warp_footprint_lens(q.Minv, P.lens_ptr(), q.cfg.board_size, q.cfg.board_size, P.w, P.h, &r);
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
    b.tones = false;   // ... and so do the tones: their model was calibrated on its squares
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

// free the lanes' enhancement scratch: the frame sets, and with `small` the aux blocks and CLAHE tables too (a
// configuration with enhancement keeps those: small_layout reuses a block that is large enough)
static void lanes_free_scratch(Pipe& P, bool small)
{
    for (int l = 0; l < Pipe::MAX_LANES; l++) {
        if (P.A[l]) (void)hipFree(P.A[l]);
        if (P.B[l]) (void)hipFree(P.B[l]);
        if (P.C[l]) (void)hipFree(P.C[l]);
        P.A[l] = P.B[l] = P.C[l] = nullptr;
        if (small) dev_free(&P.lane_small[l]);
    }
}

// free a board and its handle (board 0's handle too: the pipeline's shared part is freed by its owner)
static void board_free(cbv_pipeline* p)
{
    Board& b = p->b;
    if (b.h_stage) (void)hipHostFree(b.h_stage);
    if (b.warped) (void)hipFree(b.warped);
    DevBuf* bufs[] = {&b.d_descs, &b.d_masks, &b.d_gray, &b.d_stats, &b.d_ref, &b.d_state, &b.d_results, &b.d_flags, &b.d_dec, &b.d_mean,
                      &b.d_var, &b.d_noise, &b.d_noise_state, &b.d_hough, &b.d_check, &b.d_hough_over, &b.d_session, &b.d_hist, &b.d_radar,
                      &b.d_cgray, &b.d_ptabs, &b.d_tone_sums, &b.d_tone_res, &b.d_tone_model};
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
    FrameSettings fs;
    fs.w = w;
    fs.h = h;
    fs.max_frames = max_frames;
    const int rc = pipeline_set_frames(*P, fs, "cbv_pipeline_create", false); // the BGR ring
    if (rc) {
        delete P;
        return rc;
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
        dev_free(&P->lane_work[l]);
        if (P->lane_done[l]) (void)hipEventDestroy(P->lane_done[l]);
    }
    lanes_free_scratch(*P, true);
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
    pipeline_frames_free(*P);
    if (P->enhanced) (void)hipFree(P->enhanced);
    dev_free(&P->d_synth);
    dev_free(&P->d_btab);
    dev_free(&P->d_boards);
    dev_free(&P->d_lens_tab);
    for (cbv_pipeline* q : P->boards) board_free(q); // board 0 (p) included
    delete P;
}

// (null where the plan has no BGR ring)
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
    const bool profile_raw = cfg->skip_enhance == CBV_SKIP_ENHANCE_PROFILE_RAW;
    const bool profile_only = cfg->skip_enhance == CBV_SKIP_ENHANCE_PROFILE || profile_raw;
    ProfileTabs ptabs;
    if (profile_only) RC(profile_tabs_checked(ctx, &cfg->enhance.profile, &ptabs, "cbv_pipeline_configure"));
    // every argument check that needs no state is done; from here on a failure leaves the pipeline UNconfigured
    // (run / results / ... return CBV_ERR_STATE) instead of half reconfigured
    P.configured = false;
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    P.keep_enhanced = cfg->keep_enhanced != 0;
    P.skip_enhance = cfg->skip_enhance != 0;
    P.profile_only = profile_only;
    P.profile_raw = profile_raw;
    int chunk = cfg->chunk;
    if (chunk <= 0) chunk = 32;
    if (chunk > P.max_frames) chunk = P.max_frames;
    P.chunk = chunk;
    // (re)allocate
    int lanes = cfg->lanes <= 0 ? 2 : cfg->lanes;
    if (lanes > Pipe::MAX_LANES) lanes = Pipe::MAX_LANES;
    if ((P.max_frames + chunk - 1) / chunk < lanes) lanes = (P.max_frames + chunk - 1) / chunk;
    P.n_lanes = lanes;
    lanes_free_scratch(P, P.skip_enhance);
    if (P.enhanced) (void)hipFree(P.enhanced);
    P.enhanced = nullptr;
    if (!P.start_ev) CBV_HIP(ctx, hipEventCreateWithFlags(&P.start_ev, hipEventDisableTiming));
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
    RC(board_set_profile(P, p->b, &cfg->enhance.profile, "cbv_pipeline_configure"));
    // region-limited enhancement: the source footprint of the S x S warp (warp_footprint)
    RC(pipeline_update_region(P));
    RC(pipeline_tables(P));
    FrameSettings next = P.fs; // the configuration decides where a raw format's frames live
    next.kind = frame_kind(cfg->skip_enhance);
    RC(pipeline_set_frames(P, next, "cbv_pipeline_configure", false));
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
    if (rc == CBV_OK) rc = board_set_profile(P, b->b, &cfg.enhance.profile, "cbv_pipeline_add_board"); // the pipeline's configured profile
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

// The board's profile and its device table (profile modes only; otherwise the board has neither).  Nothing may be in flight
// that reads the table: the callers joined the runs.
int board_set_profile(Pipe& P, Board& b, const cbv_color_profile* profile, const char* who)
{
    cbv_ctx* ctx = P.ctx;
    if (!P.profile_only) {
        memset(&b.profile, 0, sizeof(b.profile));
        dev_free(&b.d_ptabs);
        return CBV_OK;
    }
    ProfileTabs pt;
    RC(profile_tabs_checked(ctx, profile, &pt, who));
    RC(dev_ensure(ctx, &b.d_ptabs, sizeof(ProfileTabs)));
    CBV_HIP(ctx, hipMemcpyAsync(b.d_ptabs.p, &pt, sizeof(pt), hipMemcpyHostToDevice, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (pt is on this stack)
    b.profile = *profile;
    b.profile.enabled = profile->enabled ? 1 : 0;
    return CBV_OK;
}

extern "C" int cbv_pipeline_set_profile(cbv_pipeline* p, const cbv_color_profile* profile)
{
    const char* who = "cbv_pipeline_set_profile";
    if (!p || !profile) return cbv_fail(p ? p->pipe->ctx : nullptr, CBV_ERR_ARG, "%s: null argument", who);
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    if (!P.configured || !P.profile_only)
        return cbv_fail(ctx, CBV_ERR_STATE, "%s: the pipeline is not configured with CBV_SKIP_ENHANCE_PROFILE or CBV_SKIP_ENHANCE_PROFILE_RAW", who);
    ProfileTabs probe;
    RC(profile_tabs_checked(ctx, profile, &probe, who)); // a rejected profile changes nothing
    CBV_ENTER(ctx);
    RC(join_scan(P)); // the runs in flight read the table that is replaced here
    RC(board_set_profile(P, p->b, profile, who));
    return pipeline_tables(P); // (whether any board has an enabled profile decides the warp's kernel)
}

extern "C" int cbv_pipeline_set_lens(cbv_pipeline* p, const cbv_lens* lens)
{
    const char* who = "cbv_pipeline_set_lens";
    if (!p) return cbv_fail(nullptr, CBV_ERR_ARG, "%s: the pipeline is null", who);
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    if (attached(p)) return cbv_fail(ctx, CBV_ERR_STATE, "%s: the lens is the camera's: it goes to the parent of a board", who);
    const bool on = lens && lens->enabled;
    LensDev L = {};
    if (on) RC(lens_checked(ctx, lens, &L, who)); // a rejected lens changes nothing
    CBV_ENTER(ctx);
    RC(join_scan(P)); // the runs in flight keep their table and their region; what comes next is ordered behind them
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    P.lens_on = on;
    P.lens = L;
    if (!P.configured) return CBV_OK;
    RC(pipeline_update_region(P)); // enhance_region's footprint follows the lens
    return pipeline_tables(P);
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
    const SquareDesc& d = B.descs[roi];
    const float* src = (const float*)(which == 0 ? B.d_mean.p : B.d_var.p) + d.plane_off;
    return pipeline_readback(P, out, src, sizeof(float) * d.w * d.h); // behind the model scans of the runs in flight
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
    return pipeline_readback(P, out, (cbv_noise_result*)p->b.d_noise.p + slot0, sizeof(cbv_noise_result) * count);
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
        src = P.plan.raw() ? nullptr : P.frames + P.g.frame_stride * slot;
        bytes = (size_t)P.w * P.h * 3;
        if (P.plan.raw()) { // the frames are raw: the slot is converted for the caller
            if (P.plan.source == FRAMES_RAW && !P.raw_ring) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_download: no raw frame was ever uploaded or submitted");
            if (P.copy_stream) CBV_HIP(ctx, hipStreamSynchronize(P.copy_stream)); // submitted copies of the slot
            RC(dev_ensure(ctx, &ctx->a, P.g.frame_stride + 256));
            if (P.plan.source == FRAMES_PLANES) RC(pipeline_jpeg_slot_bgr(P, slot, (u8*)ctx->a.p)); // k_jpeg_color on the slot's planes
            else RC(launch_ingest_any(ctx, slot_planes(P, slot), tight_raw_geom(P.fs.fmt, P.w, P.h), (u8*)ctx->a.p, P.g, 1, P.fs.cs, P.bdeep));
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
    return pipeline_readback(P, out, src, bytes); // (the runs are joined already)
}

extern "C" int cbv_pipeline_hough(cbv_pipeline* p, int slot, cbv_hough_result* out)
{
    if (!p || !out || slot < 0 || slot >= p->pipe->max_frames) return CBV_ERR_ARG;
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    if (!P.configured || !p->b.cfg.use_hough) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_hough: the HoughCircles stage is not configured");
    CBV_ENTER(ctx);
    return pipeline_readback(P, out, (const cbv_hough_result*)p->b.d_hough.p + (size_t)CBV_MAX_SQUARES * slot, sizeof(cbv_hough_result) * CBV_MAX_SQUARES);
}

extern "C" int cbv_pipeline_square_stats(cbv_pipeline* p, int slot, cbv_sq_stats* out)
{
    if (!p || !out || !p->pipe->configured || slot < 0 || slot >= p->pipe->max_frames) return CBV_ERR_ARG;
    Pipe& P = *p->pipe;
    const Board& B = p->b;
    cbv_ctx* ctx = P.ctx;
    CBV_ENTER(ctx);
    return pipeline_readback(P, out, (cbv_sq_stats*)B.d_stats.p + (size_t)B.cfg.n_rois * slot, sizeof(cbv_sq_stats) * B.cfg.n_rois);
}
