// The run of the device-resident pipeline (cbv_pipeline_run): the per-board stages of a chunk on the lanes, then the scan
// stage of the run (HoughCircles' second pass, model scan, temporal scan, NoiseHandler, game session).
#include "cbv_pipeline.h"
#include "session_core.h"

// the per-board stages of a chunk of b frames from slot s0 (warp, square statistics, HoughCircles' first pass): with boards
// attached one launch each for all of them, otherwise the single-board launches with board 0's arguments, which measured
// faster on one board than the table-driven kernels with a table of one
// (res = the BGR frames the warp samples; in raw mode null, and the warp samples the chunk's slots of the raw ring;
// with the profile-only mode's enabled profile the warp applies it to its taps)
static int pipeline_chunk_boards(Pipe& P, const u8* res, NormSrc norm, int s0, int b, u32* work, u32* retry0, u32* retry, int retry_base)
{
    cbv_ctx* ctx = P.ctx;
    // what the warp samples (raw mode: the planes of the chunk's first slot)
    // (the profile's table: board 0's for the single-board launch; the multi-board kernels read the boards' own)
    const ProfileTabs* pt = P.profile_on ? (const ProfileTabs*)P.b0().d_ptabs.p : nullptr;
    const WarpSrc src = !res ? pipeline_raw_warp_src(P, s0, pt)
                        : pt ? warp_src_profile(res, P.g, pt)
                             : warp_src_bgr(res, P.g, norm);
    // the camera's lens: one launch of the lens kernels for every board, from the lens table, in place of either warp below
    const int nb = (int)P.boards.size();
    if (P.lens_on) RC(launch_warp_lens(ctx, src, P.lens, (const LensBoard*)P.d_lens_tab.p, nb, P.max_S, P.max_S, s0, b, work, retry0));
    if (nb > 1) {
        const BoardDev* tab = (const BoardDev*)P.d_boards.p;
        if (!P.lens_on) RC(launch_warp_mb(ctx, src, tab, nb, P.max_S, s0, b, work, retry0));
        if (P.any_tones) RC(launch_piece_tone_boards(ctx, tab, nb, s0, b));
        RC(launch_squares_pre5_stats_mb(ctx, tab, nb, P.n_squares, s0, b, P.any_hough, work, P.max_px));
        if (P.any_own_blur) RC(launch_change_blur_stats_mb(ctx, tab, nb, P.n_squares, s0, b, P.max_px));
        if (P.any_hough) RC(launch_hough_mb(ctx, tab, nb, s0, work, CBV_MAX_SQUARES * nb * b, P.hough_lds[0], retry, retry_base, 0));
        return CBV_OK;
    }
    const BoardDev& T = P.tab[0];
    u8* wdst = T.warped + T.warped_stride * s0;
    u8* gray = T.gray + T.plane_total * s0;
    u8* dec = T.dec + (size_t)CBV_MAX_SQUARES * s0;
    cbv_hough_result* hres = T.hough ? T.hough + (size_t)CBV_MAX_SQUARES * s0 : nullptr;
    if (!P.lens_on) RC(launch_warp(ctx, src, T.Minv, T.S, T.S, T.rot180, wdst, T.S * 3, T.warped_stride, b, work, retry0));
    if (P.any_tones) RC(launch_piece_tone_boards(ctx, (const BoardDev*)P.d_boards.p, 1, s0, b)); // (table-driven for one board too)
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

// The scan stage of ONE board for a run: the temporal scan, packing and NoiseHandler; with a game session the rounds of
// k_session.hip (temporal scan, then packing, NoiseHandler and the session's walk).
static int board_scan(Pipe& P, Board& q, const BoardDev& T, int slot0, int count, bool mirrored)
{
    cbv_ctx* ctx = P.ctx;
    const u8* gray = T.gray + T.plane_total * slot0;
    u8* dec = T.dec + (size_t)CBV_MAX_SQUARES * slot0;
    u8* flags = T.flags + (size_t)CBV_MAX_SQUARES * slot0;
    ResultMirror mir;
    if (mirrored) {
        mir.records = T.mirror + slot0;
        mir.over_src = T.over_src;
        mir.over_dst = T.over_dst;
    }
    const u64* check = q.has_check ? T.check + slot0 : nullptr;
    if (!q.session) // + NoiseHandler on the frames' visual_changes sets (game_session.py:165)
        return launch_scan(ctx, T.descs, T.sp, gray, T.plane_total, dec, T.ref, T.state, flags, T.results + slot0, count, check, T.noise_state,
                           T.noise + slot0, mir);
    // Two accepted moves are at least `gap` frames apart, so `len` frames hold at most ceil(len / gap) of them, and one more
    // round finishes behind the last; rounds that find the frames finished return at once.
    const int gap = std::max(q.ses_cfg.stability_required, q.ses_cfg.cooldown_frames + 1);
    SessionDev* ses = (SessionDev*)q.d_session.p;
    u16* hist = (u16*)q.d_hist.p + (size_t)CBV_MAX_SQUARES * slot0;
    cbv_session_radar* radar = q.ses_cfg.radar ? (cbv_session_radar*)q.d_radar.p + slot0 : nullptr;
    const cbv_tone_result* tones = q.ses_cfg.tone ? T.tone_res + slot0 : nullptr; // the rules' tie-break (begin checked that tones are on)
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
                                   radar ? radar + a : nullptr, tones ? tones + a : nullptr));
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
    const int nb = (int)P.boards.size();
    const BoardDev* tab = (const BoardDev*)P.d_boards.p;
    const u32* retry = (const u32*)rec->retry.p;
    // squares whose first HoughCircles pass overflowed (normally none), before the scan reads the decisions: one launch for
    // the boards of a table, the explicit one for a single board (as the first pass)
    const BoardDev& T0 = P.tab[0];
    if (P.any_hough && nb > 1) RC(launch_hough_mb(ctx, tab, nb, slot0, retry, CBV_MAX_SQUARES * nb * count, P.hough_lds[1], nullptr, 0, 1));
    else if (P.any_hough)
        RC(launch_hough_second(ctx, T0.descs, T0.n, T0.gray + T0.plane_total * slot0, T0.plane_total, P.b0().hough_cfg,
                               T0.hough + (size_t)CBV_MAX_SQUARES * slot0, T0.dec + (size_t)CBV_MAX_SQUARES * slot0, retry, T0.n * count));
    // the z-score statistics and the model update of the boards whose model follows the frames, before the scan reads the
    // classes: table-driven for every number of boards, a single board being a table of one
    if (P.any_adaptive) RC(launch_model_scan(ctx, tab, nb, slot0, count, P.max_px));
    // The scan, packing and NoiseHandler of several boards are one launch each too, unless a board runs a game session: a
    // session scans in rounds of its own, so every board's scan is launched by itself.  So is a single board's: the
    // table-driven scan measured 1.5 to 3 % slower on it.
    if (nb > 1 && !P.any_session) RC(launch_scan_mb(ctx, tab, nb, slot0, count, mirrored ? 1 : 0));
    else
        for (int k = 0; k < nb; k++) RC(board_scan(P, P.boards[k]->b, P.tab[k], slot0, count, mirrored));
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
    if (P.plan.source == FRAMES_RAW && !P.raw_ring) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_run: no raw frame was ever uploaded or submitted");
    // Squares HoughCircles cannot run on: with boards attached pipeline_tables refused them; a pipeline of one board is
    // configured with them and refused here, before anything is enqueued
    if (P.any_hough && (!P.hough_lds[0] || !P.hough_lds[1])) {
        const HoughCfg& hc = P.b0().hough_cfg;
        if (hc.maxw < 2 || hc.maxh < 2 || hc.maxw > 250 || hc.maxh > 250) // (hough_dims_ok)
            return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "HoughCircles stage: squares must be 2..250 px (got %dx%d)", hc.maxw, hc.maxh);
        return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "HoughCircles stage: %dx%d squares do not fit the LDS layout", hc.maxw, hc.maxh);
    }
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
        const u8* src = P.plan.raw() ? nullptr : P.frames + P.g.frame_stride * s0; // (raw mode: the warp samples the raw ring)
        u32* work = P.any_hough ? (u32*)P.lane_work[lane].p : nullptr; // worklist counter: zeroed by k_warp
        u32* retry0 = P.any_hough && retry_zero_in_warp ? (u32*)rec->retry.p : nullptr;
        if (P.skip_enhance) { // the session's chain: the warp samples the frames as they are (in raw mode the raw ring: no BGR source)
            rc_all = pipeline_chunk_boards(P, src, NormSrc(), s0, b, work, retry0, (u32*)rec->retry.p, s0 - slot0);
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
