// ---------------------------------------------------------------------------
// game session (include/cbv.h): begin / end / moves / state
// ---------------------------------------------------------------------------
#include "../../include/cbv_chess.h"
#include "cbv_pipeline.h"
#include "session_core.h"

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
                        "online %d, radar %d, tone %d; online needs CBV_SESSION_RULE_INFER)",
                        cfg->rule, cfg->stability_required, cfg->cooldown_frames, cfg->scan_period, cfg->max_diff, cfg->online, cfg->radar, cfg->tone);
    if (cfg->tone && !B.tones)
        return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_session_begin: cfg.tone needs the board's tones (cbv_pipeline_set_tones), which are off");
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
    return pipeline_readback(P, out, (cbv_session_radar*)p->b.d_radar.p + slot0, sizeof(cbv_session_radar) * (size_t)n);
}

static int session_fetch(cbv_pipeline* p, const char* who, std::vector<SessionDev>& host)
{
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    if (!p->b.session) return cbv_fail(ctx, CBV_ERR_STATE, "%s: no session is running on this board", who);
    host.resize(1);
    return pipeline_readback(P, host.data(), p->b.d_session.p, sizeof(SessionDev));
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
