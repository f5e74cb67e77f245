// The PieceDetector radius and Hough settings sweep on the device (include/cbv.h, cbv_pipeline_piece_sweep): what
// calibrate_piece_detector.py shows for every position of its radius and Hough trackbars, from the gray planes and the
// statistics a board's run left for its slots.
//
// k_piece_sweep_hough  one workgroup per (square, frame, slice of the sorted settings).  Once per distinct (dp, param1):
//                      passes P0-P3 of the HoughCircles transform (hough_passes.h), the edge list and per edge the vote
//                      step pair (sx, sy), which depends on neither radii nor param2 and goes into a table beside the
//                      list; the gray plane is dead from then on, so the candidate overlay of P6 / P7 stays valid from
//                      setting to setting.  Per setting: clear the accumulator, vote, P5-P7; a setting whose radii (for
//                      this square) equal its predecessor's keeps the accumulator and redoes P5-P7 only.  8 bytes leave
//                      per (setting, frame, square): PieceChoice.  Squares the statistics gate as uniform leave at once.
// k_piece_sweep_eval   (statistics: [frame][square] shared by the settings, or, stat_stride != 0, one set per setting,
//                      stat_stride frames apart: the colour profile sweep, whose settings change the pixels)
//                      one wave per setting, lane = square: walks the chunk's frames in order with the 5-deep history of
//                      (setting, square) in a register (carried from chunk to chunk in a device buffer), decides
//                      (piece_sweep_core.h), ballots into the six square sets, writes the record and adds to the summary.
//                      A wave owns its setting: no atomics.
// Neither kernel has a profile id (the enumeration is closed): cbv_pipeline_piece_sweep times them with event pairs.
#include <algorithm>
#include <cmath>

#include "hough_passes.h"
#include "piece_sweep_core.h"

namespace {

// the vote step from the table made once per (dp, param1): sx in the low, sy in the high half (|s| <= 1024: dp >= 1)
struct HgStepTable {
    const u32* t;
    __device__ __forceinline__ void operator()(const HgSq& q, int e, int x, int y, int& sx, int& sy) const
    {
        (void)q;
        (void)x;
        (void)y;
        const u32 v = t[e];
        sx = (int)(int16_t)(v & 0xFFFFu);
        sy = (int)v >> 16;
    }
};

__global__ __launch_bounds__(HG_NT) void k_piece_sweep_hough(const SquareDesc* __restrict__ descs, int n, const u8* __restrict__ gray,
                                                             size_t gray_frame_stride, const cbv_sq_stats* __restrict__ stats, HoughCfg cfg,
                                                             int off_steps, const PieceSet* __restrict__ sets, int ns, PieceChoice* __restrict__ out,
                                                             int out_frames)
{
    extern __shared__ __align__(16) u8 smem[];
    __shared__ int s_cnt[4]; // 0 weak, 1 edges, 2 centres, 3 circles
    __shared__ int s_over;
    const int sqi = blockIdx.x, fri = blockIdx.y, tid = threadIdx.x;
    // this workgroup's slice of the sorted settings
    const int per = (ns + (int)gridDim.z - 1) / (int)gridDim.z;
    const int g0 = (int)blockIdx.z * per, g1 = min(ns, g0 + per);
    if (g0 >= g1) return;
    const cbv_sq_stats st = stats[(size_t)fri * n + sqi];
    if (piece_uniform(&st)) { // np.std < 15: detect_piece returns before HoughCircles (workgroup-uniform)
        for (int si = g0 + tid; si < g1; si += HG_NT) out[((size_t)sets[si].index * out_frames + fri) * CBV_MAX_SQUARES + sqi] = PieceChoice{0, 0, 0, 0, 0};
        return;
    }
    const SquareDesc d = descs[sqi];
    u32* steps = (u32*)(smem + off_steps);
    HgCircle* sorted = (HgCircle*)(smem + cfg.off_order);
    HgSq q;
    int nedges = 0, last_min = -1, last_max = -1;
    float cur_dp = 0.f;
    int cur_thr = -1;
    for (int si = g0; si < g1; si++) {
        const PieceSet s = sets[si];
        bool fresh = false;
        if (si == g0 || s.dp != cur_dp || s.canny_thr != cur_thr) { // the front end: once per (dp, param1)
            cur_dp = s.dp;
            cur_thr = s.canny_thr;
            cfg.dp = s.dp;
            hg_square(q, d, cfg, smem, s_cnt, &s_over);
            hg_p0(q, (const u32*)(gray + (size_t)fri * gray_frame_stride + d.plane_off), cfg.mag_bytes);
            __syncthreads();
            hg_p1(q);
            __syncthreads();
            hg_p2(q, max(1, s.canny_thr / 2), s.canny_thr);
            __syncthreads();
            hg_p3(q);
            hg_list_edges(q);
            __syncthreads();
            nedges = s_cnt[1];
            for (int e = tid; e < nedges; e += HG_NT) {
                int sx, sy;
                hg_step(q, q.edges[e] & 255, q.edges[e] >> 8, sx, sy);
                steps[e] = ((u32)sx & 0xFFFFu) | ((u32)sy << 16);
            }
            fresh = true; // (the barrier in front of the vote covers the table)
        }
        int min_radius, max_radius;
        hg_radii(q, s.min_ratio, s.max_ratio, min_radius, max_radius);
        if (fresh || min_radius != last_min || max_radius != last_max) {
            last_min = min_radius;
            last_max = max_radius;
            hg_zero_acc(q);
            __syncthreads();
            hg_vote(q, nedges, min_radius, max_radius, HgStepTable{steps});
        }
        if (tid == 0) {
            s_cnt[2] = 0;
            s_cnt[3] = 0;
            s_over = 0;
        }
        __syncthreads();
        hg_p5(q, s.acc_thr, cfg.maxc);
        __syncthreads();
        const int over = s_over; // no retry list: the flag travels with the choice
        const int ncent = min(s_cnt[2], cfg.maxc);
        hg_p6(q, ncent, nedges, min_radius, max_radius, s.acc_thr, cfg.max_bins);
        const int ncirc = s_cnt[3];
        hg_p7_sort(q, ncirc, sorted);
        __syncthreads();
        if (q.wave == 0) {
            int kept, pick;
            HgCircle pc;
            hg_p7_pick(q, ncirc, sorted, kept, pick, pc);
            if (q.lane == 0) {
                PieceChoice c = {0, (u8)(over ? CBV_HOUGH_OVERFLOW : 0), 0, 0, 0};
                if (pick >= 0) { // int(np.float32): toward zero
                    c.kind = hg_kind(pc, q.min_dim);
                    c.r = (int16_t)(int)pc.r;
                    c.cx = (int16_t)(int)pc.x;
                    c.cy = (int16_t)(int)pc.y;
                }
                out[((size_t)s.index * out_frames + fri) * CBV_MAX_SQUARES + sqi] = c;
            }
        }
        __syncthreads(); // the counters and the candidate planes are reused by the next setting
    }
}

#define PS_EVAL_WAVES 4
__global__ __launch_bounds__(64 * PS_EVAL_WAVES) void k_piece_sweep_eval(const SquareDesc* __restrict__ descs, int n, const cbv_sq_stats* __restrict__ stats,
                                                                         int stat_stride, const PieceChoice* __restrict__ choices, int choice_frames, int frames, int ns,
                                                                         const u64* __restrict__ expected, u32* __restrict__ hist,
                                                                         cbv_piece_sweep_record* __restrict__ rec, int rec_stride,
                                                                         cbv_piece_sweep_summary* __restrict__ sums)
{
    const int lane = threadIdx.x & 63, si = (int)blockIdx.x * PS_EVAL_WAVES + (int)(threadIdx.x >> 6);
    if (si >= ns) return; // wave-uniform
    const bool in = lane < n;
    const int w = in ? descs[lane].w : 1, h = in ? descs[lane].h : 1;
    u32 hs = hist[(size_t)si * CBV_MAX_SQUARES + lane];
    cbv_piece_sweep_summary S = sums[si];
    for (int f = 0; f < frames; f++) {
        cbv_piece_result res;
        PieceChoice c = {0, 0, 0, 0, 0};
        bool raw = false, stable = false;
        if (in) {
            const cbv_sq_stats st = stats[((size_t)si * stat_stride + f) * n + lane];
            c = choices[((size_t)si * choice_frames + f) * CBV_MAX_SQUARES + lane];
            piece_decide_choice(&st, c, w, h, &res);
            raw = res.has_piece != 0;
            stable = piece_history_step(hs, raw);
        }
        const int method = raw ? (int)res.method : CBV_METHOD_NONE;
        const u64 b_raw = __ballot(raw), b_stable = __ballot(stable);
        const u64 b_hough = __ballot(method == CBV_METHOD_HOUGH), b_tower = __ballot(method == CBV_METHOD_TOWER_TOP);
        const u64 b_cdiff = __ballot(method == CBV_METHOD_CENTER_DIFF), b_sym = __ballot(method == CBV_METHOD_SYMMETRY);
        const bool circle = method == CBV_METHOD_HOUGH || method == CBV_METHOD_TOWER_TOP;
        const int r_min = wave_min_i32(circle ? (int)c.r : 0x7FFF), r_max = wave_max_i32(circle ? (int)c.r : -0x8000);
        const u32 r_sum = wave_sum_u32(circle ? (u32)c.r : 0u);
        const u64 b_over = __ballot(in && (c.flags & CBV_HOUGH_OVERFLOW));
        const cbv_piece_sweep_record r = piece_sweep_record(b_raw, b_stable, b_hough, b_tower, b_cdiff, b_sym, r_min, r_max, b_over != 0);
        piece_sweep_sum(&S, r, expected != nullptr, expected ? expected[f] : 0ull, r_sum, (u32)__builtin_popcountll(b_hough | b_tower),
                        (u32)__builtin_popcountll(b_over));
        if (rec && lane == 0) rec[(size_t)si * rec_stride + f] = r;
    }
    hist[(size_t)si * CBV_MAX_SQUARES + lane] = hs;
    if (lane == 0) sums[si] = S;
}

} // namespace

size_t piece_sweep_layout(HoughCfg* cfg, int* off_steps)
{
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t steps = up16((size_t)cfg->maxw * cfg->maxh * 4); // one step pair per edge pixel at most
    cfg->keep_acc = 1; // settings that share their radii share the votes
    *cfg = hough_pass_cfg(*cfg, 1, steps);
    const size_t lds = up16(hough_layout(*cfg));
    *off_steps = (int)lds;
    return lds + steps;
}

int launch_piece_sweep_hough(cbv_ctx* ctx, const SquareDesc* descs, int n, const u8* gray, size_t gray_frame_stride, const cbv_sq_stats* stats,
                             HoughCfg cfg, const PieceSet* sets, int ns, int frames, PieceChoice* out, int out_frames)
{
    if (!hough_dims_ok(cfg))
        return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "piece sweep: squares must be 2..250 px (got %dx%d)", cfg.maxw, cfg.maxh);
    int off_steps = 0;
    const size_t lds = piece_sweep_layout(&cfg, &off_steps);
    if (lds > 150 * 1024)
        return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "piece sweep: %dx%d squares do not fit the LDS layout", cfg.maxw, cfg.maxh);
    if (lds > 64 * 1024) // an upper bound, set on every call: the sweep keeps no state on the context
        CBV_HIP(ctx, hipFuncSetAttribute((const void*)k_piece_sweep_hough, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
    // slices of the settings: enough workgroups to fill the chip, at least 16 settings a workgroup (its front end costs
    // about as much as a few settings)
    int parts = (2 * ctx->num_cus + n * frames - 1) / (n * frames);
    parts = std::max(1, std::min(parts, (ns + 15) / 16));
    hipLaunchKernelGGL(k_piece_sweep_hough, dim3(n, frames, parts), dim3(HG_NT), lds, ctx->stream, descs, n, gray, gray_frame_stride, stats, cfg,
                       off_steps, sets, ns, out, out_frames);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

int launch_piece_sweep_eval(cbv_ctx* ctx, const SquareDesc* descs, int n, const cbv_sq_stats* stats, const PieceChoice* choices, int choice_frames,
                            int frames, int ns, const u64* expected, u32* hist, cbv_piece_sweep_record* rec, int rec_stride,
                            cbv_piece_sweep_summary* sums, int stat_stride)
{
    hipLaunchKernelGGL(k_piece_sweep_eval, dim3((ns + PS_EVAL_WAVES - 1) / PS_EVAL_WAVES), dim3(64 * PS_EVAL_WAVES), 0, ctx->stream, descs, n, stats,
                       stat_stride, choices, choice_frames, frames, ns, expected, hist, rec, rec_stride, sums);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

// the host twin of k_piece_sweep_eval: the same decision, history and bookkeeping (piece_sweep_core.h)
extern "C" int cbv_piece_sweep_eval_host(const cbv_sq_stats* stats, const int32_t* ws, const int32_t* hs, int n, int frames, const void* choices,
                                         int ns, const uint64_t* expected, cbv_piece_sweep_record* records, cbv_piece_sweep_summary* summary)
{
    if (!stats || !ws || !hs || n <= 0 || n > CBV_MAX_SQUARES || frames <= 0 || !choices || ns <= 0 || !summary) return CBV_ERR_ARG;
    for (int i = 0; i < n; i++)
        if (ws[i] <= 0 || hs[i] <= 0) return CBV_ERR_ARG;
    const PieceChoice* ch = (const PieceChoice*)choices;
    for (int si = 0; si < ns; si++) {
        u32 hist[CBV_MAX_SQUARES] = {0};
        cbv_piece_sweep_summary S;
        memset(&S, 0, sizeof(S));
        for (int f = 0; f < frames; f++) {
            u64 sets[6] = {0, 0, 0, 0, 0, 0}, b_over = 0; // raw, stable, then by method
            int r_min = 0x7FFF, r_max = -0x8000;
            u32 r_sum = 0;
            for (int i = 0; i < n; i++) {
                const PieceChoice c = ch[((size_t)si * frames + f) * n + i];
                cbv_piece_result res;
                piece_decide_choice(&stats[(size_t)f * n + i], c, ws[i], hs[i], &res);
                const bool raw = res.has_piece != 0;
                if (raw) sets[0] |= 1ull << i;
                if (piece_history_step(hist[i], raw)) sets[1] |= 1ull << i;
                if (raw) sets[1 + res.method] |= 1ull << i;
                if (raw && (res.method == CBV_METHOD_HOUGH || res.method == CBV_METHOD_TOWER_TOP)) {
                    r_min = std::min(r_min, (int)c.r);
                    r_max = std::max(r_max, (int)c.r);
                    r_sum += (u32)c.r;
                }
                if (c.flags & CBV_HOUGH_OVERFLOW) b_over |= 1ull << i;
            }
            const cbv_piece_sweep_record r = piece_sweep_record(sets[0], sets[1], sets[2], sets[3], sets[4], sets[5], r_min, r_max, b_over != 0);
            piece_sweep_sum(&S, r, expected != nullptr, expected ? expected[f] : 0ull, r_sum, (u32)__builtin_popcountll(sets[2] | sets[3]),
                            (u32)__builtin_popcountll(b_over));
            if (records) records[(size_t)si * frames + f] = r;
        }
        summary[si] = S;
    }
    return CBV_OK;
}
