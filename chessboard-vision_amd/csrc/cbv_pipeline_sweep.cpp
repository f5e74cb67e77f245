// The settings sweeps of the device-resident pipeline (include/cbv.h): the ChangeDetector sensitivity sweep and the
// PieceDetector settings sweep.  Both evaluate their settings chunk of frames by chunk of frames on the context's stream.
#include "cbv_pipeline.h"
#include "piece_sweep_core.h"

namespace {
// What a call of either sweep allocates, freed when it returns; `ms` = the time from ev[0] to ev[1] (the first stage of a
// chunk) and from ev[1] to ev[2] (its evaluation), and so on for a sweep of more stages, summed over the chunks.
struct SweepCall {
    DevBuf sets, hist, rec, sums;
    DevBuf planes, kbeg;      // ChangeDetector sweep
    DevBuf choices, expected; // PieceDetector sweep
    DevBuf tabs, boards, gray, stats; // colour profile sweep (four stages: ev[0..4], ms[0..3])
    DevBuf lens_tab;                  // ... with the pipeline's lens on: a LensBoard per profile of the chunk
    u8* h_rec = nullptr; // pinned staging of a chunk's records
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
    ~SweepCall()
    {
        for (DevBuf* b : {&sets, &hist, &rec, &sums, &planes, &kbeg, &choices, &expected, &tabs, &boards, &gray, &stats, &lens_tab}) dev_free(b);
        if (h_rec) (void)hipHostFree(h_rec);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};
} // namespace

// a sweep reads what the runs left in its slots (slot_blur = 0: none ever ran there)
static int sweep_slots_were_run(cbv_ctx* ctx, const Board& B, const char* who, int slot0, int count)
{
    for (int i = 0; i < count; i++)
        if (!B.slot_blur[slot0 + i]) return cbv_fail(ctx, CBV_ERR_STATE, "%s: slot %d was never run", who, slot0 + i);
    return CBV_OK;
}

// The end of a chunk of `cf` frames from frame `c0` of the call's `count`, behind the record of ev[2]: the chunk's records
// (`records` != null: [ns][chunk] of `rec_size` bytes on the device) through the pinned staging into the caller's
// [ns][count], and the chunk's `stages` times (behind the record of ev[stages]).  Returns with the stream idle.
static int sweep_chunk_end(cbv_ctx* ctx, SweepCall& S, void* records, size_t rec_size, int ns, int count, int chunk, int c0, int cf, int stages = 2)
{
    if (records) CBV_HIP(ctx, hipMemcpyAsync(S.h_rec, S.rec.p, rec_size * ns * chunk, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < stages; i++) {
        float ms = 0.f;
        CBV_HIP(ctx, hipEventElapsedTime(&ms, S.ev[i], S.ev[i + 1]));
        S.ms[i] += ms;
    }
    if (records)
        for (int s = 0; s < ns; s++) memcpy((u8*)records + ((size_t)s * count + c0) * rec_size, S.h_rec + (size_t)s * chunk * rec_size, rec_size * cf);
    return CBV_OK;
}

// ---------------------------------------------------------------------------
// The ChangeDetector sensitivity sweep (include/cbv.h, cbv_pipeline_sweep; kernels in k_sweep.hip).  Everything it allocates
// belongs to the call and is freed when it returns; of the board it reads the warped ring, the square table and slot_blur.
// ---------------------------------------------------------------------------
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
    RC(sweep_slots_were_run(ctx, B, who, calib_slot, 1));
    RC(sweep_slots_were_run(ctx, B, who, slot0, count));
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
    for (int i = 0; i < 3; i++) CBV_HIP(ctx, hipEventCreate(&S.ev[i]));
    const SquareDesc* descs = (const SquareDesc*)B.d_descs.p;
    float planes_ms = 0.f;
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
        RC(sweep_chunk_end(ctx, S, eval ? records : nullptr, sizeof(cbv_sweep_record), ns, count, chunk, c0, cf));
    }
    if (eval && summaries) CBV_HIP(ctx, hipMemcpy(summaries, S.sums.p, sizeof(cbv_sweep_summary) * ns, hipMemcpyDeviceToHost));
    if (hist_out) CBV_HIP(ctx, hipMemcpy(hist_out, S.hist.p, sizeof(u16) * 256 * n, hipMemcpyDeviceToHost));
    if (info) {
        info->planes_ms = planes_ms;
        info->hist_ms = S.ms[0];
        info->eval_ms = S.ms[1];
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
// a setting as the kernels read it (the casts of hough_cfg), checked as cbv_pipeline_piece_sweep documents it
static int piece_set_checked(cbv_ctx* ctx, const char* who, const cbv_hough_params& s, int i, PieceSet& t)
{
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
    t.dp = (float)s.dp < 1.f ? 1.f : (float)s.dp;
    t.canny_thr = (int)nearbyint(s.param1);
    t.acc_thr = (int)nearbyint(s.param2);
    t.index = (u32)i;
    t.min_ratio = s.min_radius_ratio;
    t.max_ratio = s.max_radius_ratio;
    return CBV_OK;
}

// the layout's worst case: hc = maxw, maxh and the smallest dp of the settings
static int piece_sweep_fits(cbv_ctx* ctx, const char* who, HoughCfg* hc)
{
    // The radius histogram of the layout is sized for the widest span any setting can ask of any square: maxRadius is the
    // square's larger side whenever int(min_dim * max_ratio) is 0 (ratios below 1 / min_dim, the trackbars' first positions),
    // and min_radius + 2 when it does not exceed the minimum, so with ratios up to 1 the span is at most max(w, h) + 2:
    // ratios of 0 make hough_layout take that span.
    hc->min_ratio = hc->max_ratio = 0;
    HoughCfg probe = *hc;
    int off = 0;
    if (hc->maxw < 2 || hc->maxh < 2 || hc->maxw > 250 || hc->maxh > 250 || piece_sweep_layout(&probe, &off) > 150 * 1024)
        return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "%s: %dx%d squares do not fit the LDS layout of the sweep", who, hc->maxw, hc->maxh);
    return CBV_OK;
}

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
        PieceSet& t = sets[(size_t)i];
        RC(piece_set_checked(ctx, who, settings[i], i, t));
        hc.dp = i == 0 ? t.dp : std::min(hc.dp, t.dp);
    }
    RC(piece_sweep_fits(ctx, who, &hc));
    CBV_ENTER(ctx);
    RC(sweep_slots_were_run(ctx, B, who, slot0, count));
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
    SweepCall S;
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
    for (int i = 0; i < 3; i++) CBV_HIP(ctx, hipEventCreate(&S.ev[i]));
    const SquareDesc* descs = (const SquareDesc*)B.d_descs.p;
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
        RC(sweep_chunk_end(ctx, S, eval ? records : nullptr, sizeof(cbv_piece_sweep_record), ns, count, chunk, c0, cf));
    }
    if (eval) CBV_HIP(ctx, hipMemcpy(summary, S.sums.p, sizeof(cbv_piece_sweep_summary) * ns, hipMemcpyDeviceToHost));
    if (choices_out) CBV_HIP(ctx, hipMemcpy(choices_out, S.choices.p, sizeof(PieceChoice) * CBV_MAX_SQUARES, hipMemcpyDeviceToHost));
    if (info) {
        info->hough_ms = S.ms[0];
        info->eval_ms = S.ms[1];
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

// ---------------------------------------------------------------------------
// The colour profile sweep (include/cbv.h, cbv_pipeline_color_sweep).  Everything it allocates belongs to the call and is
// freed when it returns; of the pipeline it reads the BGR frame ring (in the raw mode of CBV_SKIP_ENHANCE_PROFILE_RAW: the
// raw ring, through k_warp_raw_profile), of the board its geometry, square table, masks and
// Hough settings.  The scratch boards, planes, statistics and circle choices of a chunk are laid out [profile][frame]
// with the chunk's frame count between profiles, so that the statistics kernel and k_piece_sweep_hough (one setting) see
// profiles x frames as one batch of frames and k_piece_sweep_eval sees the profiles as its settings.
// ---------------------------------------------------------------------------
#define COLOR_SWEEP_SCRATCH ((size_t)256 << 20) // bytes of scratch boards, planes and statistics a chunk may take

extern "C" int cbv_pipeline_color_sweep(cbv_pipeline* p, int slot0, int count, const cbv_color_profile* profiles, int np, const uint64_t* expected,
                                        int chunk, cbv_piece_sweep_record* records, cbv_piece_sweep_summary* summary, cbv_color_sweep_info* info)
{
    const char* who = "cbv_pipeline_color_sweep";
    if (!p) return cbv_fail(nullptr, CBV_ERR_ARG, "%s: the board is null", who);
    Pipe& P = *p->pipe;
    const Board& B = p->b;
    cbv_ctx* ctx = P.ctx;
    if (!P.configured) return cbv_fail(ctx, CBV_ERR_STATE, "%s: the pipeline is not configured", who);
    if (!profiles || np <= 0 || count <= 0 || !summary) return cbv_fail(ctx, CBV_ERR_ARG, "%s: no profiles, no frames or no summary", who);
    if (np > CBV_COLOR_SWEEP_MAX_PROFILES) return cbv_fail(ctx, CBV_ERR_ARG, "%s: %d profiles (at most %d)", who, np, CBV_COLOR_SWEEP_MAX_PROFILES);
    if (chunk < 0 || chunk > CBV_SWEEP_MAX_CHUNK) return cbv_fail(ctx, CBV_ERR_ARG, "%s: chunk_frames %d is outside 0..%d", who, chunk, CBV_SWEEP_MAX_CHUNK);
    if (slot0 < 0 || slot0 > P.max_frames - count) return cbv_fail(ctx, CBV_ERR_ARG, "%s: slots outside the ring of %d", who, P.max_frames);
    if (P.plan.raw() && !P.profile_raw)
        return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "%s: the pipeline's frames are raw and it has no profile kernel (there is no BGR ring to read; "
                        "configure CBV_SKIP_ENHANCE_PROFILE_RAW, with a disabled profile for the plain raw warp)", who);
    if (P.plan.source == FRAMES_RAW && !P.raw_ring) return cbv_fail(ctx, CBV_ERR_STATE, "%s: no raw frame was ever uploaded or submitted", who);
    const int n = B.cfg.n_rois, S_ = B.cfg.board_size;
    HoughCfg hc;
    memset(&hc, 0, sizeof(hc));
    for (const SquareDesc& d : B.descs) {
        hc.maxw = std::max(hc.maxw, d.w);
        hc.maxh = std::max(hc.maxh, d.h);
    }
    PieceSet set; // the board's own radii and Hough parameters: the one setting of every profile
    RC(piece_set_checked(ctx, who, B.cfg.hough, 0, set));
    hc.dp = set.dp;
    RC(piece_sweep_fits(ctx, who, &hc));
    {
        ProfileTabs probe;
        for (int i = 0; i < np; i++) RC(profile_tabs_checked(ctx, &profiles[i], &probe, who));
    }
    if (chunk == 0) chunk = CBV_SWEEP_DEFAULT_CHUNK;
    chunk = std::min(chunk, count);
    // profiles per chunk: the scratch's bound, and profiles x frames is the z (y) extent of the launches
    const size_t per_board = B.warped_stride + B.plane_total + sizeof(cbv_sq_stats) * n + sizeof(PieceChoice) * CBV_MAX_SQUARES;
    const int pchunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)np, COLOR_SWEEP_SCRATCH / (per_board * chunk), (size_t)(65535 / chunk)}));
    CBV_ENTER(ctx);
    RC(join_scan(P));
    for (auto& c : P.copies) // ingest copies of these slots must have landed (the copy stays the next run's to acknowledge)
        if (c.pending && ranges_overlap(slot0, count, c.s0, c.cnt)) CBV_HIP(ctx, hipStreamWaitEvent(ctx->stream, c.ev, 0));
    SweepCall S;
    const size_t boards = (size_t)pchunk * chunk;
    RC(dev_ensure(ctx, &S.sets, sizeof(PieceSet)));
    CBV_HIP(ctx, hipMemcpy(S.sets.p, &set, sizeof(set), hipMemcpyHostToDevice));
    RC(dev_ensure(ctx, &S.tabs, sizeof(ProfileTabs) * pchunk));
    RC(dev_ensure(ctx, &S.boards, B.warped_stride * boards + 256));
    RC(dev_ensure(ctx, &S.gray, B.plane_total * boards));
    CBV_HIP(ctx, hipMemsetAsync(S.gray.p, 0, B.plane_total * boards, ctx->stream)); // the planes' padding reads as zero
    RC(dev_ensure(ctx, &S.stats, sizeof(cbv_sq_stats) * n * boards));
    RC(dev_ensure(ctx, &S.choices, sizeof(PieceChoice) * CBV_MAX_SQUARES * boards));
    CBV_HIP(ctx, hipMemsetAsync(S.choices.p, 0, sizeof(PieceChoice) * CBV_MAX_SQUARES * boards, ctx->stream));
    RC(dev_ensure(ctx, &S.hist, sizeof(u32) * CBV_MAX_SQUARES * np));
    CBV_HIP(ctx, hipMemsetAsync(S.hist.p, 0, sizeof(u32) * CBV_MAX_SQUARES * np, ctx->stream));
    RC(dev_ensure(ctx, &S.sums, sizeof(cbv_piece_sweep_summary) * np));
    CBV_HIP(ctx, hipMemsetAsync(S.sums.p, 0, sizeof(cbv_piece_sweep_summary) * np, ctx->stream));
    if (expected) {
        RC(dev_ensure(ctx, &S.expected, sizeof(u64) * count));
        CBV_HIP(ctx, hipMemcpy(S.expected.p, expected, sizeof(u64) * count, hipMemcpyHostToDevice));
    }
    if (records) {
        RC(dev_ensure(ctx, &S.rec, sizeof(cbv_piece_sweep_record) * boards));
        CBV_HIP(ctx, hipHostMalloc((void**)&S.h_rec, sizeof(cbv_piece_sweep_record) * boards, hipHostMallocDefault));
    }
    for (hipEvent_t& e : S.ev) CBV_HIP(ctx, hipEventCreate(&e));
    const SquareDesc* descs = (const SquareDesc*)B.d_descs.p;
    std::vector<ProfileTabs> tabs((size_t)pchunk);
    for (int p0 = 0; p0 < np; p0 += pchunk) {
        const int pc = std::min(pchunk, np - p0);
        for (int i = 0; i < pc; i++) RC(profile_tabs_checked(ctx, &profiles[p0 + i], &tabs[(size_t)i], who));
        CBV_HIP(ctx, hipMemcpy(S.tabs.p, tabs.data(), sizeof(ProfileTabs) * pc, hipMemcpyHostToDevice)); // (the stream is idle: sweep_chunk_end)
        for (int c0 = 0; c0 < count; c0 += chunk) {
            const int cf = std::min(chunk, count - c0), nb = pc * cf; // scratch frame of (profile i, frame f) = i * cf + f
            CBV_HIP(ctx, hipEventRecord(S.ev[0], ctx->stream));
            const ProfileTabs* pt = (const ProfileTabs*)S.tabs.p;
            const WarpSrc src = P.plan.raw() ? pipeline_raw_warp_src(P, slot0 + c0, pt, pc, B.warped_stride * cf)
                                             : warp_src_profile(P.frames + P.g.frame_stride * (slot0 + c0), P.g, pt, pc, B.warped_stride * cf);
            if (P.lens_on) { // the lens kernels are table-driven: profile i of the chunk is entry i, its frames where launch_warp puts them
                std::vector<LensBoard> lt((size_t)pc);
                for (int i = 0; i < pc; i++)
                    lt[(size_t)i] = lens_board(B.Minv, S_, S_, B.cfg.rot180, (u8*)S.boards.p + B.warped_stride * cf * i, S_ * 3, B.warped_stride, pt + i);
                RC(dev_ensure(ctx, &S.lens_tab, sizeof(LensBoard) * pchunk));
                CBV_HIP(ctx, hipMemcpy(S.lens_tab.p, lt.data(), sizeof(LensBoard) * pc, hipMemcpyHostToDevice)); // (the stream is idle: sweep_chunk_end)
                RC(launch_warp_lens(ctx, src, P.lens, (const LensBoard*)S.lens_tab.p, pc, S_, S_, 0, cf, nullptr, nullptr));
            } else
                RC(launch_warp(ctx, src, B.Minv, S_, S_, B.cfg.rot180, (u8*)S.boards.p, S_ * 3, B.warped_stride, cf));
            CBV_HIP(ctx, hipEventRecord(S.ev[1], ctx->stream));
            RC(launch_squares_pre5_stats(ctx, (const u8*)S.boards.p, B.warped_stride, descs, n, (u8*)S.gray.p, B.plane_total, nullptr, nullptr,
                                         (const u8*)B.d_masks.p, (float)B.cfg.z_threshold, (cbv_sq_stats*)S.stats.p, nb, nullptr, 0, nullptr, nullptr,
                                         B.max_px));
            CBV_HIP(ctx, hipEventRecord(S.ev[2], ctx->stream));
            RC(launch_piece_sweep_hough(ctx, descs, n, (const u8*)S.gray.p, B.plane_total, (const cbv_sq_stats*)S.stats.p, hc, (const PieceSet*)S.sets.p, 1,
                                        nb, (PieceChoice*)S.choices.p, nb));
            CBV_HIP(ctx, hipEventRecord(S.ev[3], ctx->stream));
            RC(launch_piece_sweep_eval(ctx, descs, n, (const cbv_sq_stats*)S.stats.p, (const PieceChoice*)S.choices.p, cf, cf, pc,
                                       expected ? (const u64*)S.expected.p + c0 : nullptr, (u32*)S.hist.p + (size_t)CBV_MAX_SQUARES * p0,
                                       (cbv_piece_sweep_record*)S.rec.p, chunk, (cbv_piece_sweep_summary*)S.sums.p + p0, cf));
            CBV_HIP(ctx, hipEventRecord(S.ev[4], ctx->stream));
            RC(sweep_chunk_end(ctx, S, records ? records + (size_t)p0 * count : nullptr, sizeof(cbv_piece_sweep_record), pc, count, chunk, c0, cf, 4));
        }
    }
    CBV_HIP(ctx, hipMemcpy(summary, S.sums.p, sizeof(cbv_piece_sweep_summary) * np, hipMemcpyDeviceToHost));
    if (info) {
        info->warp_ms = S.ms[0];
        info->squares_ms = S.ms[1];
        info->hough_ms = S.ms[2];
        info->eval_ms = S.ms[3];
        info->chunk_frames = chunk;
        info->chunk_profiles = pchunk;
    }
    return CBV_OK;
}
