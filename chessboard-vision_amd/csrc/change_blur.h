// ChangeDetector._preprocess of one square in LDS, shared by k_change_blur_stats (k_squares.hip) and k_change_hist
// (k_sweep.hip): the gray stage and the two passes of the separable Gaussian; what happens to a pixel that leaves the
// vertical pass is the caller's (`emit`).
#pragma once
#include "cbv_device.h"

// BGR2GRAY of a square's ROI into LDS (u8, rows packed) by NT lanes: four pixels (12 bytes, any alignment) per lane and load
// instruction, four tasks a lane per round with all their loads issued before the first result is stored
// (k_squares_preprocess5 explains both)
template <int NT>
__device__ __forceinline__ void stage_gray_bgr(const u8* __restrict__ s, const SquareDesc& d, u8* g)
{
    const int w = d.w, h = d.h;
    const int ngx = (w + 3) >> 2, ntask = ngx * h;
    for (int t0 = threadIdx.x; t0 < ntask; t0 += 4 * NT) {
        u32 v[4][3];
        int yy[4], xx[4];
        bool full[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int t = t0 + q * NT;
            full[q] = false;
            if (t < ntask) {
                yy[q] = t / ngx;
                xx[q] = (t - yy[q] * ngx) << 2;
                full[q] = xx[q] + 3 < w;
                if (full[q]) __builtin_memcpy(v[q], s + (size_t)yy[q] * d.stride + 3 * xx[q], 12);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int t = t0 + q * NT;
            if (t >= ntask) continue;
            u8* o = g + yy[q] * w + xx[q];
            if (full[q]) {
                o[0] = (u8)d_gray(v[q][0] & 255, (v[q][0] >> 8) & 255, (v[q][0] >> 16) & 255);
                o[1] = (u8)d_gray(v[q][0] >> 24, v[q][1] & 255, (v[q][1] >> 8) & 255);
                o[2] = (u8)d_gray((v[q][1] >> 16) & 255, v[q][1] >> 24, v[q][2] & 255);
                o[3] = (u8)d_gray((v[q][2] >> 8) & 255, (v[q][2] >> 16) & 255, v[q][2] >> 24);
            } else {
                const u8* p = s + (size_t)yy[q] * d.stride + 3 * xx[q];
                for (int k = 0; xx[q] + k < w; k++) o[k] = (u8)d_gray(p[3 * k], p[3 * k + 1], p[3 * k + 2]);
            }
        }
    }
}

// GaussianBlur((k, k), 0) of the staged gray square `g` (u8, rows packed; the caller's barrier is behind it), REFLECT_101 on
// the square alone, 8.8 coefficients: cf[j] = the coefficient j taps from the centre.  Lanes walk the square as a 16 x 16
// grid; the horizontal pass goes to `hb` as u16, reflected columns / rows are resolved once per column / row and tap, and the
// kernel's symmetry makes it r + 1 multiplies per pixel and pass.  A lane keeps the accumulators of all its rows of a column
// (horizontal) or all its columns of a row (vertical) in registers while the taps go by.  emit(i, gv): pixel i = y * w + x
// of the square has the value gv.
template <int NT, class Emit>
__device__ __forceinline__ void change_blur_passes(const SquareDesc& d, const u8* g, u16* hb, int blur_k, const u32* cf, Emit&& emit)
{
    constexpr int RSTEP = NT / 16;                      // rows between two rows of a lane
    constexpr int ROWS = CBV_MAX_SQUARE_DIM / RSTEP;    // rows of a lane at most
    constexpr int COLS = CBV_MAX_SQUARE_DIM / 16;       // columns of a lane at most
    const int w = d.w, h = d.h;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int r = blur_k >> 1;
    // rows / columns a lane of this wave / workgroup can have: the unrolled loops below skip the rest as whole waves; a
    // lane past the square's edge inside them computes on the edge row / column and stores nothing
    const int nr = __builtin_amdgcn_readfirstlane((h - 1 - (ty & ~3) + RSTEP) / RSTEP);
    const int nc = (w + 15) >> 4;
    if (r > 0) {
        int row[ROWS];
#pragma unroll
        for (int yi = 0; yi < ROWS; yi++) row[yi] = min(ty + yi * RSTEP, h - 1) * w;
        const u32 c0 = cf[0];
        for (int x = tx; x < w; x += 16) {
            u32 acc[ROWS];
#pragma unroll
            for (int yi = 0; yi < ROWS; yi++)
                if (yi < nr) acc[yi] = c0 * g[row[yi] + x];
            for (int j = 1; j <= r; j++) {
                const int xl = d_reflect101(x - j, w), xr = d_reflect101(x + j, w);
                const u32 c = cf[j];
#pragma unroll
                for (int yi = 0; yi < ROWS; yi++)
                    if (yi < nr) acc[yi] += c * ((u32)g[row[yi] + xl] + (u32)g[row[yi] + xr]);
            }
#pragma unroll
            for (int yi = 0; yi < ROWS; yi++)
                if (yi < nr && ty + yi * RSTEP < h) hb[row[yi] + x] = (u16)min(acc[yi], 65535u);
        }
        __syncthreads();
    }
    int col[COLS];
#pragma unroll
    for (int xi = 0; xi < COLS; xi++) col[xi] = min(tx + 16 * xi, w - 1);
    for (int y = ty; y < h; y += RSTEP) {
        if (r == 0) { // k = 1: GaussianBlur((1, 1)) is the gray itself
#pragma unroll
            for (int xi = 0; xi < COLS; xi++)
                if (xi < nc && tx + 16 * xi < w) emit(y * w + col[xi], g[y * w + col[xi]]);
            continue;
        }
        u32 acc[COLS];
        const u32 c0 = cf[0];
#pragma unroll
        for (int xi = 0; xi < COLS; xi++)
            if (xi < nc) acc[xi] = c0 * hb[y * w + col[xi]];
        for (int j = 1; j <= r; j++) {
            const int yu = d_reflect101(y - j, h) * w, yd = d_reflect101(y + j, h) * w;
            const u32 c = cf[j];
#pragma unroll
            for (int xi = 0; xi < COLS; xi++)
                if (xi < nc) acc[xi] += c * ((u32)hb[yu + col[xi]] + (u32)hb[yd + col[xi]]);
        }
#pragma unroll
        for (int xi = 0; xi < COLS; xi++)
            if (xi < nc && tx + 16 * xi < w) emit(y * w + col[xi], (int)min((acc[xi] + (1u << 15)) >> 16, 255u));
    }
}

// LDS of the above by the largest square of the set: u8 gray + u16 horizontal pass
static inline size_t change_blur_lds(int max_px)
{
    if (max_px <= 0 || max_px > CBV_MAX_SQUARE_DIM * CBV_MAX_SQUARE_DIM) max_px = CBV_MAX_SQUARE_DIM * CBV_MAX_SQUARE_DIM;
    return (size_t)((max_px + 15) & ~15) + 2 * (size_t)max_px;
}
