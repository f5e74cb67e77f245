// cv2.HoughCircles(gray, HOUGH_GRADIENT, dp=1.2, minDist=min_dim//3, param1, param2, minRadius, maxRadius)
// for every square of a frame batch plus the "nearest circle to the square centre" pick of
// PieceDetector._detect_circle_unified (piece_detector.py:216-270).
//
// One workgroup per (square, frame); the whole transform lives in LDS:
//   P0 blurred gray plane -> LDS                         P1 Sobel 3x3 (replicate) -> L1 magnitude
//   P2 Canny non-maximum suppression, weak list          P3 hysteresis sweeps over the weak list
//   P4 edge list, gradient-line votes (LDS atomics)      P5 accumulator local maxima > param2
//   P6 per centre radius histogram (one wave a centre)   P7 sort, minDist suppression, pick
// The arithmetic follows the published OpenCV 4.x HoughCirclesGradient step for step (same fixed
// point, same float expressions, one rounding per operation); the results do not depend on the
// order in which edges or centres are visited, so the parallel order here is free.
#include "hough_passes.h"

// one work item (square sqi of frame fri) of k_hough / k_hough_mb; rtag = the board's bits of a second-pass entry
__device__ __forceinline__ void hough_item(const SquareDesc* __restrict__ descs, const u8* __restrict__ gray,
                                           size_t gray_frame_stride, const HoughCfg& cfg,
                                           cbv_hough_result* __restrict__ out, u8* __restrict__ decisions, int sqi, int fri, u32 rtag)
{
    extern __shared__ __align__(16) u8 smem[];
    __shared__ int s_cnt[4]; // 0 weak, 1 edges, 2 centres, 3 circles
    __shared__ int s_over;
    {
    const size_t oi = (size_t)fri * CBV_MAX_SQUARES + sqi;
    const SquareDesc d = descs[sqi];
    HgSq q;
    hg_square(q, d, cfg, smem, s_cnt, &s_over);
    const int tid = q.tid, lane = q.lane, wave = q.wave, min_dim = q.min_dim;
    int min_radius, max_radius;
    hg_radii(q, cfg.min_ratio, cfg.max_ratio, min_radius, max_radius);
    const int low = max(1, cfg.canny_thr / 2), high = cfg.canny_thr;

#ifdef HG_TIMING
    long long tk[10];
    int tki = 0;
#define HG_TICK() do { __syncthreads(); tk[tki++] = __builtin_readcyclecounter(); } while (0)
#else
#define HG_TICK() do { } while (0)
#endif
    HG_TICK();
    hg_p0(q, (const u32*)(gray + (size_t)fri * gray_frame_stride + d.plane_off), cfg.mag_bytes);
    __syncthreads();
    HG_TICK();
    hg_p1(q);
    __syncthreads();
    HG_TICK();
    hg_p2(q, low, high);
    __syncthreads();
    HG_TICK();
    const int nweak = hg_p3(q);
    (void)nweak;
    HG_TICK();
    hg_zero_acc(q);
    hg_list_edges(q);
    __syncthreads();
    const int nedges = s_cnt[1];
    hg_vote(q, nedges, min_radius, max_radius, HgStepSobel());
    __syncthreads();
    HG_TICK();
    hg_p5(q, cfg.acc_thr, cfg.maxc);
    __syncthreads();
    HG_TICK();
    if (s_over && cfg.retry) { // workgroup-uniform: hand the square to the second pass, decide nothing here
        if (tid == 0) {
            const u32 k = atomicAdd(&cfg.retry[0], 1u);
            cfg.retry[1 + k] = rtag | ((u32)(fri + cfg.retry_frame_base) << 8) | (u32)sqi;
        }
        __syncthreads(); // s_over / s_cnt are reset at the top of the next item
        return;
    }
    const int ncent = min(s_cnt[2], cfg.maxc);
    hg_p6(q, ncent, nedges, min_radius, max_radius, cfg.acc_thr, cfg.max_bins);
    HG_TICK();
    const int ncirc = s_cnt[3];
    HgCircle* sorted = (HgCircle*)(smem + cfg.off_order);
    hg_p7_sort(q, ncirc, sorted);
    __syncthreads();
    if (wave == 0) {
    int kept, pick;
    HgCircle pc;
    hg_p7_pick(q, ncirc, sorted, kept, pick, pc);
    const HgCircle* circ = q.circ;
    if (lane == 0) {
        u8 found = 0, kind = 0;
        if (pick >= 0) {
            found = 1;
            kind = hg_kind(pc, min_dim);
        }
        if (decisions && found) decisions[oi] = decisions[oi] | 1;
        if (out) {
            cbv_hough_result r;
            r.found = found;
            r.kind = kind;
            r.n_circles = (uint16_t)kept;
            r.cx = pc.x;
            r.cy = pc.y;
            r.r = pc.r;
            r.votes = pc.votes;
            r.n_edges = (uint32_t)nedges;
            r.n_centres = (uint16_t)ncent;
            r.flags = (uint16_t)(s_over ? CBV_HOUGH_OVERFLOW : 0);
            if (s_over && cfg.overflow_count) atomicAdd(cfg.overflow_count, 1u);
            for (int i = 0; i < CBV_HOUGH_KEEP; i++) {
                const bool ok = i < kept;
                const HgCircle ci = ok ? circ[i] : HgCircle{0.f, 0.f, 0.f, 0};
                r.circles[i][0] = ci.x;
                r.circles[i][1] = ci.y;
                r.circles[i][2] = ci.r;
                r.circles[i][3] = (float)ci.votes;
            }
#ifdef HG_TIMING
            for (int i = 0; i + 1 < tki && i < 8; i++) r.circles[2 + i / 4][i % 4] = (float)(tk[i + 1] - tk[i]);
            r.circles[4][0] = (float)(__builtin_readcyclecounter() - tk[tki - 1]);
            r.circles[4][1] = (float)nweak;
            r.circles[4][2] = (float)ncirc;
#endif
            out[oi] = r;
        }
    }
    } // wave 0
    __syncthreads(); // LDS is reused by the next item
    }
}

__global__ __launch_bounds__(HG_NT) void k_hough(const SquareDesc* __restrict__ descs, const u8* __restrict__ gray,
                                                size_t gray_frame_stride, HoughCfg cfg,
                                                cbv_hough_result* __restrict__ out, u8* __restrict__ decisions,
                                                const u32* __restrict__ work, int nsq, int total_items)
{
    // Work items: with a worklist (pipeline), work[0] = count and work[1 + i] = frame << 8 | square, filled by
    // k_squares_stats for the squares whose has_piece the statistics left open; otherwise every (square, frame).
    // A fixed grid of workgroups strides over the items, so idle workgroups never hold an LDS slot.
    const int n_items = work ? (int)work[0] : total_items;
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int sqi = work ? (int)(work[1 + item] & 255u) : item % nsq;
        const int fri = work ? (int)(work[1 + item] >> 8) : item / nsq;
        hough_item(descs, gray, gray_frame_stride, cfg, out, decisions, sqi, fri, 0u);
    }
}

// every board of a pipeline in one launch: the items of all boards share one list, board << MB_BOARD_SHIFT | frame << 8 |
// square, and each item runs with its board's descriptors, planes and HoughCfg (`pass`: 0 first, 1 second pass)
__global__ __launch_bounds__(HG_NT) void k_hough_mb(const BoardDev* __restrict__ tab, int s0, const u32* __restrict__ work, int pass,
                                                   u32* __restrict__ retry, int retry_frame_base)
{
    const int n_items = (int)work[0];
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const u32 e = work[1 + item];
        const int b = (int)(e >> MB_BOARD_SHIFT);
        const int sqi = (int)(e & 255u), fri = (int)((e >> 8) & ((1u << (MB_BOARD_SHIFT - 8)) - 1u));
        const BoardDev& T = tab[b];
        HoughCfg cfg = T.hcfg[pass];
        cfg.retry = retry;
        cfg.retry_frame_base = retry_frame_base;
        const size_t s = (size_t)s0;
        hough_item(T.descs, T.gray + s * T.plane_total, T.plane_total, cfg, T.hough + s * CBV_MAX_SQUARES, T.dec + s * CBV_MAX_SQUARES,
                   sqi, fri, (u32)b << MB_BOARD_SHIFT);
    }
}


// as many workgroups as the chip holds at once (LDS-limited), striding over the work items
static int hough_grid(cbv_ctx* ctx, size_t lds, int max_grid, int total)
{
    const int per_cu = (int)(160 * 1024 / (lds + 1024)) < 2 ? ((int)(160 * 1024 / (lds + 1024)) < 1 ? 1 : (int)(160 * 1024 / (lds + 1024))) : 2;
    int grid = ctx->num_cus * per_cu;
    if (grid > max_grid) grid = max_grid;
    if (grid > total) grid = total;
    if (grid < 1) grid = 1;
    return grid;
}

static int launch_hough_pass(cbv_ctx* ctx, const SquareDesc* descs, int n, const u8* gray, size_t gray_frame_stride, HoughCfg cfg,
                             cbv_hough_result* out, u8* decisions, const u32* work, int total, int max_grid)
{
    const size_t lds = hough_layout(cfg);
    if (lds > 150 * 1024)
        return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "HoughCircles stage: %dx%d squares do not fit the LDS layout", cfg.maxw, cfg.maxh);
    if (lds > 64 * 1024 && !ctx->hough_lds_raised) { // once per context: the attribute is an upper bound
        CBV_HIP(ctx, hipFuncSetAttribute((const void*)k_hough, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
        ctx->hough_lds_raised = true;
    }
    const int grid = hough_grid(ctx, lds, max_grid, total);
    hipLaunchKernelGGL(k_hough, dim3(grid), dim3(HG_NT), lds, ctx->stream, descs, gray, gray_frame_stride, cfg, out, decisions, work, n, total);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

int launch_hough(cbv_ctx* ctx, const SquareDesc* descs, int n, const u8* gray, size_t gray_frame_stride, HoughCfg cfg,
                 cbv_hough_result* out, u8* decisions, const u32* work, int batch, u32* retry, int retry_frame_base)
{
    if (!hough_dims_ok(cfg))
        return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "HoughCircles stage: squares must be 2..250 px (got %dx%d)", cfg.maxw, cfg.maxh);
    cfg = hough_pass_cfg(cfg, 0);
    cfg.retry = retry;
    cfg.retry_frame_base = retry_frame_base;
    prof_begin(ctx, CBV_K_HOUGH);
    const int rc = launch_hough_pass(ctx, descs, n, gray, gray_frame_stride, cfg, out, decisions, work, n * batch, 1 << 30);
    prof_end(ctx, CBV_K_HOUGH);
    return rc;
}

int launch_hough_second(cbv_ctx* ctx, const SquareDesc* descs, int n, const u8* gray, size_t gray_frame_stride, HoughCfg cfg,
                        cbv_hough_result* out, u8* decisions, const u32* retry, int max_items)
{
    return launch_hough_pass(ctx, descs, n, gray, gray_frame_stride, hough_pass_cfg(cfg, 1), out, decisions, retry, max_items, 32);
}

void hough_board_cfgs(HoughCfg cfg, HoughCfg out[2], size_t lds[2])
{
    for (int k = 0; k < 2; k++) {
        out[k] = hough_pass_cfg(cfg, k);
        lds[k] = hough_layout(out[k]);
        if (!hough_dims_ok(cfg) || lds[k] > 150 * 1024) lds[k] = 0;
    }
}

int launch_hough_mb(cbv_ctx* ctx, const BoardDev* tab, int nb, int s0, const u32* work, int max_items, size_t lds, u32* retry,
                    int retry_frame_base, int pass)
{
    (void)nb;
    if (lds > 64 * 1024 && !ctx->hough_mb_lds_raised) {
        CBV_HIP(ctx, hipFuncSetAttribute((const void*)k_hough_mb, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
        ctx->hough_mb_lds_raised = true;
    }
    const int grid = hough_grid(ctx, lds, pass == 0 ? 1 << 30 : 32, max_items); // (as launch_hough / launch_hough_second)
    if (pass == 0) prof_begin(ctx, CBV_K_HOUGH);
    hipLaunchKernelGGL(k_hough_mb, dim3(grid), dim3(HG_NT), lds, ctx->stream, tab, s0, work, pass, pass == 0 ? retry : nullptr,
                       retry_frame_base);
    if (pass == 0) prof_end(ctx, CBV_K_HOUGH);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}
