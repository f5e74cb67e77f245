// The game session on the device (include/cbv.h, cbv_pipeline_session_begin): the back half of GameSession.on_frame
// (game_session.py:130-265) for every frame of a run, without a host round trip.
//
// A run with a session is a fixed number of ROUNDS on the scan stream, each k_scan_session (k_squares.hip) followed by
// k_session_walk below.  The scan of a round is speculative: it runs to the end of the run with the references, check
// sets and NoiseHandler state it started from.  The walk packs the records, runs NoiseHandler and the session's
// per-frame logic (session_core.h) in frame order, and stops behind the first accepted move at frame t*: everything up to
// t* is final, everything behind it was scanned with stale state.  It stores resume = t* + 1, the next round redoes
// [resume, count) from {reference = the planes of t*, cache cleared, history as recorded at t*, fresh NoiseHandler, the
// new smart mask}, which is what update_references(squares) + noise.reset() leave (game_session.py:219-223).  A round
// that finds resume > count returns at once.  No workgroup ever waits for another: the rounds are ordered by the stream.
// Two accepted moves are at least max(stability_required, cooldown_frames + 1) frames apart, which bounds the rounds.
//
// The walk is one sequential chain on one wave; the rules use the wave when the walk does reach the generator: lane 0
// lists the pseudo-legal moves in python-chess order, every lane tests the king's safety of one of them, a ballot and
// a prefix count keep the order, and the destinations of the smart mask are OR-reduced across the lanes.
// The list is built once per walk and kept while the board stands (a rejected rule call, the radar); an accepted move
// ends the walk.
// Online play (include/cbv.h): the turn gate is part of ses_frame_rule; a board event (cbv_pipeline_session_sync) is
// k_session_event between two segments of a run, each segment being the rounds above on its own frames (cbv_pipeline_run.cpp,
// board_scan); the radar is computed by the walk in front of the stable-move step of each frame, its destinations as an
// OR across the lanes over the kept list.
#include "cbv_internal.h"
#include "cbv_device.h"
#include "noise_core.h"
#include "session_core.h"

namespace {

struct WalkLds {
    cbv_movelist cand, legal, scratch;
};

__device__ __forceinline__ u64 wave_or_u64(u64 v)
{
    u32 lo = (u32)v, hi = (u32)(v >> 32);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo |= __shfl_xor(lo, o, WAVE);
        hi |= __shfl_xor(hi, o, WAVE);
    }
    return (u64)hi << 32 | lo;
}

// list(board.legal_moves) of *b into L->legal, by the whole (single) wave of the workgroup; returns the OR of the
// destination squares.  *b is uniform and not written meanwhile.
__device__ u64 wave_gen_legal(const cbv_pos* b, WalkLds* L)
{
    const int lane = threadIdx.x;
    if (lane == 0) cc_gen_candidates(b, &L->cand);
    __syncthreads();
    const int n = cc_stored(&L->cand);
    int base = 0;
    u64 dests = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const cbv_move m = i < n ? L->cand.m[i] : (cbv_move)CBV_MOVE_NONE;
        const bool ok = i < n && cc_king_safe(b, m);
        const u64 bal = __ballot(ok);
        if (ok) {
            L->legal.m[base + __popcll(bal & ((1ull << lane) - 1ull))] = m; // base + rank <= i < CBV_MAX_MOVES
            dests |= 1ull << cc_to(m);
        }
        base += __popcll(bal);
    }
    if (lane == 0) L->legal.n = base;
    __syncthreads();
    return wave_or_u64(dests);
}

__global__ __launch_bounds__(64) void k_session_walk(const u8* __restrict__ flags, int n, cbv_frame_result* __restrict__ results, int count,
                                                      cbv_noise_state* __restrict__ noise_state, cbv_noise_result* __restrict__ noise_out,
                                                      ResultMirror mir, SessionDev* __restrict__ ses, int first_round,
                                                      cbv_session_radar* __restrict__ radar, const cbv_tone_result* __restrict__ tones)
{
    __shared__ WalkLds L;
    __shared__ cbv_session_state st;
    __shared__ int sh_t, sh_flag, sh_roi;
    const int lane = threadIdx.x;
    const int r = first_round ? 0 : ses->resume;
    if (r > count) return;
    if (mir.over_dst && lane == 0) *mir.over_dst = mir.over_src ? *mir.over_src : 0u;
    // the records of [r, count): per-square flag bytes -> the eight square sets (pack_results_body of k_squares.hip)
    for (int t = r; t < count; t++) {
        const u32 fl = lane < n ? flags[(size_t)t * CBV_MAX_SQUARES + lane] : 0u;
        u64* rw = (u64*)&results[t];
        u64* hm = mir.records ? (u64*)&mir.records[t] : nullptr;
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const u64 m = __ballot((fl >> b) & 1u);
            if (lane == 0) {
                rw[b] = m;
                if (hm) hm[b] = m;
            }
        }
    }
    const cbv_session_config cfg = ses->cfg;
    if (lane == 0) {
        // NoiseHandler over the same frames (speculative behind a move, like the scan: redone by the next round)
        d_noise_run(&results[r].visual_changes, sizeof(cbv_frame_result) / 8, count - r, noise_state, noise_out + r);
        st = ses->st;
    }
    __syncthreads();
    int t = r;
    bool accepted = false, have_legal = false; // have_legal: L.legal is the list of the board in st
    int radar_done = -1, memo_roi = -1;        // lane 0: the frame whose radar record is written; the last lifted square
    u64 memo_dests = 0;                        // ... and its destinations (the board does not change inside a walk)
    for (;;) {
        if (lane == 0) { // frames up to the next one that needs the wave: 1 the rule has to run, 2 the radar needs the list
            int tt = t, what = 0;
            for (; tt < count; tt++) {
                const u64 vision = results[tt].stable_occupied;
                if (radar && radar_done != tt) {
                    const int roi = ses_radar_lifted(&st, vision);
                    if (roi >= 0 && roi != memo_roi) {
                        sh_roi = roi;
                        what = 2;
                        break;
                    }
                    radar[tt].lifted = (int8_t)roi;
                    radar[tt].destinations = roi >= 0 ? memo_dests : 0ull;
                    radar_done = tt;
                }
                if (ses_frame_pre(&cfg, &st, vision, noise_out[tt].state == 1)) {
                    what = 1;
                    break;
                }
            }
            sh_t = tt;
            sh_flag = what;
        }
        __syncthreads();
        t = sh_t;
        const int what = sh_flag;
        if (!what) break;
        __syncthreads(); // (sh_flag is rewritten below)
        if (!have_legal) wave_gen_legal(ses_pos(&st), &L);
        have_legal = true;
        if (what == 2) { // the lifted piece's destinations: every lane takes its share of the list
            const int roi = sh_roi;
            const u64 d = cc_flip_rows(wave_or_u64(ses_radar_dests(&L.legal, roi ^ 56, lane, 64)));
            if (lane == 0) {
                memo_roi = roi;
                memo_dests = d;
            }
            __syncthreads();
            continue; // frame t again: lane 0 writes its record from the memo and goes on
        }
        if (lane == 0) {
            cbv_session_move rec;
            // the frame's piece tones (k_piece_tone wrote them on the lanes, in front of the scan stage): the rules' tie-break
            const u64 tw = tones ? tones[t].white : 0ull, tb = tones ? tones[t].black : 0ull;
            const bool acc = ses_frame_rule(&cfg, &st, results[t].stable_occupied, tw, tb, &L.legal, &L.scratch, &rec);
            if (acc) ses->ring[(u32)(st.n_moves - 1) % CBV_SESSION_RING] = rec;
            sh_flag = acc ? 1 : 0;
        }
        __syncthreads();
        accepted = sh_flag != 0;
        if (accepted) break;
        t++;
        __syncthreads();
    }
    u64 dests = 0;
    if (accepted) {
        dests = wave_gen_legal(ses_pos(&st), &L); // of the new board: its smart mask
    }
    if (lane == 0) {
        if (accepted) {
            ses_refresh(&st, dests);
            cbv_noise_state z;
            z.state = z.stable_count = z.cooldown_count = 0;
            z.lifted = 0;
            z.pending = 0;
            *noise_state = z; // noise.reset()
            ses->resume = t + 1;
        } else ses->resume = count + 1;
        ses->st = st;
    }
}

// A board event in front of the next segment's first frame: the new board, its legal moves, expected and smart mask.
// `ev` travels in the kernel arguments, so the host's queue entry is free as soon as the launch returns.
__global__ __launch_bounds__(64) void k_session_event(SessionDev* __restrict__ ses, const cbv_session_event ev)
{
    __shared__ WalkLds L;
    __shared__ cbv_session_state st;
    if (threadIdx.x == 0) {
        st = ses->st;
        ses_apply_event(&st, &ev);
    }
    __syncthreads();
    const u64 dests = wave_gen_legal(ses_pos(&st), &L);
    if (threadIdx.x == 0) {
        ses_refresh(&st, dests);
        ses->st = st;
    }
}

// the generator alone, for tests and timing: `reps` calls on the position at the head of *state
__global__ __launch_bounds__(64) void k_session_legal(const cbv_session_state* __restrict__ state, u16* __restrict__ out, int* __restrict__ n_out, int reps)
{
    __shared__ WalkLds L;
    __shared__ cbv_pos pos;
    if (threadIdx.x == 0) pos = *ses_pos(state);
    __syncthreads();
    for (int k = 0; k < reps; k++) wave_gen_legal(&pos, &L);
    const int n = cc_stored(&L.legal);
    for (int i = threadIdx.x; i < n; i += 64) out[i] = L.legal.m[i];
    if (threadIdx.x == 0) *n_out = L.legal.n;
}

} // namespace

int launch_session_walk(cbv_ctx* ctx, const u8* flags, int n, cbv_frame_result* results, int count, cbv_noise_state* noise_state,
                        cbv_noise_result* noise_out, ResultMirror mir, SessionDev* ses, int first_round, cbv_session_radar* radar,
                        const cbv_tone_result* tones)
{
    hipLaunchKernelGGL(k_session_walk, dim3(1), dim3(64), 0, ctx->stream, flags, n, results, count, noise_state, noise_out, mir, ses, first_round,
                       radar, tones);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

int launch_session_event(cbv_ctx* ctx, SessionDev* ses, const cbv_session_event* ev)
{
    hipLaunchKernelGGL(k_session_event, dim3(1), dim3(64), 0, ctx->stream, ses, *ev);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

int launch_session_legal(cbv_ctx* ctx, const cbv_session_state* state_dev, u16* out_dev, int* n_dev, int reps)
{
    hipLaunchKernelGGL(k_session_legal, dim3(1), dim3(64), 0, ctx->stream, state_dev, out_dev, n_dev, reps);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}
