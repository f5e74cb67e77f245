// The warp of camera-native frames through the colour profile: warp(apply_color_profile(to_bgr(raw))), bit for bit, with
// neither the BGR frame nor the profiled frame ever written (pipelines configured with CBV_SKIP_ENHANCE_PROFILE_RAW, their
// colour sweep, cbv_warp_color_profile_raw).  The gather is warp_gather (warp_gather.h) with the source WarpRawProfile<FMT>:
// coordinates, wide loads, the `fast` predicate per family, rot180 and the zeroed words are the gather's own; what this
// source adds is d_profile_px on each converted tap inside the frame, from the 7.5 KB of tables a workgroup stages once for
// its WP_ROWS rows.  A tap outside the frame is BGR 0, not the profile of black; a table with enabled = 0 leaves the taps
// alone.  The kernels live in a file of their own: k_warp.hip's 52 stay what they are.
#include "warp_gather.h"

// (the frames per thread of the many-frames form, per family: raw_profile_fpt, warp_gather.h)

// blockIdx.z = profile * nz + group of frames; profile p writes its frames dst_profile_stride bytes behind profile p - 1's
// (Bayer: p1 = p2 = null)
template <int FMT, int FPT>
__global__ __launch_bounds__(256) void k_warp_raw_profile(const u8* __restrict__ p0, const u8* __restrict__ p1, const u8* __restrict__ p2, RawGeom r, int sw,
                                                           int sh, WarpM M, int dw, int dh, int bw0, int rot180, u8* __restrict__ dst, int dst_stride,
                                                           size_t dst_frame_stride, size_t dst_profile_stride, const StaticTabs* __restrict__ st,
                                                           const ProfileTabs* __restrict__ ptabs, int nz, u32* __restrict__ zero_word,
                                                           u32* __restrict__ zero_word2, int batch)
{
    const int pi = blockIdx.z / nz;
    warp_gather<WarpRawProfile<FMT>, FPT>(WarpRawProfile<FMT>{{p0, p1, p2, r, sw, sh}, st, ptabs + pi},
                                          WarpDst{M.m, dw, dh, bw0, rot180, dst + (size_t)pi * dst_profile_stride, dst_stride, dst_frame_stride},
                                          zero_word, zero_word2, batch, blockIdx.z - pi * nz);
}

// every board of a pipeline in one launch: blockIdx.z = board * nz + group of frames; a workgroup stages its board's table
template <int FMT, int FPT>
__global__ __launch_bounds__(256) void k_warp_raw_profile_mb(const u8* __restrict__ p0, const u8* __restrict__ p1, const u8* __restrict__ p2, RawGeom r,
                                                              int sw, int sh, const BoardDev* __restrict__ tab, int nz, int s0,
                                                              const StaticTabs* __restrict__ st, u32* __restrict__ zero_word,
                                                              u32* __restrict__ zero_word2, int batch)
{
    const int b = blockIdx.z / nz;
    const BoardDev& T = tab[b];
    if (b > 0 && ((int)blockIdx.x * 64 >= T.S || (int)blockIdx.y * WP_ROWS >= T.S)) return;
    warp_gather<WarpRawProfile<FMT>, FPT>(WarpRawProfile<FMT>{{p0, p1, p2, r, sw, sh}, st, T.ptabs}, warp_board_dst(T, s0), zero_word, zero_word2, batch,
                                          blockIdx.z - b * nz);
}

int launch_warp_raw_profile(cbv_ctx* ctx, WarpSrc s, const double* Minv9, int dw, int dh, int rot180, u8* dst, int dst_stride, size_t dst_frame_stride,
                            int batch, u32* zero_word, u32* zero_word2)
{
    if (!s.raw() || !s.ptabs) return cbv_fail(ctx, CBV_ERR_ARG, "launch_warp_raw_profile: not a raw source with a profile");
    WarpM M;
    for (int i = 0; i < 9; i++) M.m[i] = Minv9[i];
    int bw0, bh0;
    warp_block_shape(dw, dh, &bw0, &bh0);
    const int many = raw_profile_many(s.r.fmt);
    if (s.np <= 0 || batch <= 0 || (long long)s.np * warp_groups(batch, many) > 65535)
        return cbv_fail(ctx, CBV_ERR_ARG, "launch_warp_raw_profile: %d profiles x %d frames do not fit a launch", s.np, batch);
    const hipStream_t st = ctx->stream;
    return warp_launch(
        ctx, &s, dw, dh, s.np, batch,
        [&](auto fmt, auto fpt, dim3 grid, int nz) {
            constexpr int FMT = decltype(fmt)::value;
            if constexpr (FMT != CBV_FMT_BGR) {
                constexpr int FPT = decltype(fpt)::value == 1 ? 1 : raw_profile_fpt(FMT);
                hipLaunchKernelGGL((k_warp_raw_profile<FMT, FPT>), grid, dim3(256), 0, st, s.planes.p[0], s.planes.p[1], s.planes.p[2], s.r, s.g.w, s.g.h, M,
                                   dw, dh, bw0, rot180, dst, dst_stride, dst_frame_stride, s.dst_profile_stride, ctx->tabs, s.ptabs, nz, zero_word,
                                   zero_word2, batch);
            }
        },
        many);
}

int launch_warp_raw_profile_mb(cbv_ctx* ctx, WarpSrc s, const BoardDev* tab, int nb, int maxS, int s0, int batch, u32* zero_word, u32* zero_word2)
{
    if (!s.raw() || !s.ptabs) return cbv_fail(ctx, CBV_ERR_ARG, "launch_warp_raw_profile_mb: not a raw source with a profile");
    const hipStream_t st = ctx->stream;
    return warp_launch(
        ctx, &s, maxS, maxS, nb, batch,
        [&](auto fmt, auto fpt, dim3 grid, int nz) {
            constexpr int FMT = decltype(fmt)::value;
            if constexpr (FMT != CBV_FMT_BGR) {
                constexpr int FPT = decltype(fpt)::value == 1 ? 1 : raw_profile_fpt(FMT);
                hipLaunchKernelGGL((k_warp_raw_profile_mb<FMT, FPT>), grid, dim3(256), 0, st, s.planes.p[0], s.planes.p[1], s.planes.p[2], s.r, s.g.w,
                                   s.g.h, tab, nz, s0, ctx->tabs, zero_word, zero_word2, batch);
            }
        },
        raw_profile_many(s.r.fmt));
}
