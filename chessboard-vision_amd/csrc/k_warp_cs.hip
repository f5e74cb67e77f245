// The warp of YUV frames in a colour space other than 0 (include/cbv.h, CBV_CS_*: BT.601 full range, BT.709 limited and
// full range), lens-free: the runtime-matrix forms of k_warp_yuv / k_warp_yuv_mb (k_warp.hip) and of k_warp_raw_profile /
// k_warp_raw_profile_mb (k_warp_raw_profile.hip) for the six YUV layouts the kernels know.  The gather is warp_gather
// (warp_gather.h) with the sources WarpRawCs<FMT> and WarpRawProfileCs<FMT>: everything is their siblings' but the six
// constants of the conversion, which arrive as a kernel argument (YuvCs, cbv_yuv.h), are uniform over the launch and stay in
// scalar registers.  So three colour spaces cost one more form of each kernel, not three, and colour space 0 keeps launching
// the kernels it always launched: the launchers of k_warp.hip hand a source here only when WarpSrc::cs is not 0.  Frames per
// thread: one below batch 8, then what the siblings take (four; with a profile raw_profile_fpt), but for planar 4:2:0 without
// a profile, which takes two to stay at 64 VGPRs (yuv_cs_fpt, warp_gather.h).  The lens forms are
// k_warp_lens_cs.hip's.  tests/test_yuv_cs_resources.py lists the kernels and their registers.
#include "warp_gather.h"

template <int FMT, int FPT>
__global__ __launch_bounds__(256) void k_warp_yuv_cs(const u8* __restrict__ p0, const u8* __restrict__ p1, const u8* __restrict__ p2, RawGeom r, int sw, int sh,
                                                      YuvCs cs, WarpM M, int dw, int dh, int bw0, int rot180, u8* __restrict__ dst, int dst_stride,
                                                      size_t dst_frame_stride, u32* __restrict__ zero_word, u32* __restrict__ zero_word2, int batch)
{
    warp_gather<WarpRawCs<FMT>, FPT>(WarpRawCs<FMT>{{p0, p1, p2, r, sw, sh}, cs}, WarpDst{M.m, dw, dh, bw0, rot180, dst, dst_stride, dst_frame_stride}, zero_word,
                                     zero_word2, batch, blockIdx.z, nullptr, cs);
}

template <int FMT, int FPT>
__global__ __launch_bounds__(256) void k_warp_yuv_cs_mb(const u8* __restrict__ p0, const u8* __restrict__ p1, const u8* __restrict__ p2, RawGeom r, int sw, int sh,
                                                         YuvCs cs, const BoardDev* __restrict__ tab, int nz, int s0, u32* __restrict__ zero_word,
                                                         u32* __restrict__ zero_word2, int batch)
{
    const int b = blockIdx.z / nz;
    const BoardDev& T = tab[b];
    if (b > 0 && ((int)blockIdx.x * 64 >= T.S || (int)blockIdx.y * 4 >= T.S)) return;
    warp_gather<WarpRawCs<FMT>, FPT>(WarpRawCs<FMT>{{p0, p1, p2, r, sw, sh}, cs}, warp_board_dst(T, s0), zero_word, zero_word2, batch, blockIdx.z - b * nz, nullptr, cs);
}

// blockIdx.z = profile * nz + group of frames; profile p writes its frames dst_profile_stride bytes behind profile p - 1's
template <int FMT, int FPT>
__global__ __launch_bounds__(256) void k_warp_raw_profile_cs(const u8* __restrict__ p0, const u8* __restrict__ p1, const u8* __restrict__ p2, RawGeom r,
                                                              int sw, int sh, YuvCs cs, WarpM M, int dw, int dh, int bw0, int rot180, u8* __restrict__ dst,
                                                              int dst_stride, size_t dst_frame_stride, size_t dst_profile_stride,
                                                              const StaticTabs* __restrict__ st, const ProfileTabs* __restrict__ ptabs, int nz,
                                                              u32* __restrict__ zero_word, u32* __restrict__ zero_word2, int batch)
{
    const int pi = blockIdx.z / nz;
    warp_gather<WarpRawProfileCs<FMT>, FPT>(WarpRawProfileCs<FMT>{{{p0, p1, p2, r, sw, sh}, st, ptabs + pi}, cs},
                                            WarpDst{M.m, dw, dh, bw0, rot180, dst + (size_t)pi * dst_profile_stride, dst_stride, dst_frame_stride},
                                            zero_word, zero_word2, batch, blockIdx.z - pi * nz, nullptr, cs);
}

// every board of a pipeline in one launch: blockIdx.z = board * nz + group of frames; a workgroup stages its board's table
template <int FMT, int FPT>
__global__ __launch_bounds__(256) void k_warp_raw_profile_cs_mb(const u8* __restrict__ p0, const u8* __restrict__ p1, const u8* __restrict__ p2, RawGeom r,
                                                                 int sw, int sh, YuvCs cs, const BoardDev* __restrict__ tab, int nz, int s0,
                                                                 const StaticTabs* __restrict__ st, u32* __restrict__ zero_word,
                                                                 u32* __restrict__ zero_word2, int batch)
{
    const int b = blockIdx.z / nz;
    const BoardDev& T = tab[b];
    if (b > 0 && ((int)blockIdx.x * 64 >= T.S || (int)blockIdx.y * WP_ROWS >= T.S)) return;
    warp_gather<WarpRawProfileCs<FMT>, FPT>(WarpRawProfileCs<FMT>{{{p0, p1, p2, r, sw, sh}, st, T.ptabs}, cs}, warp_board_dst(T, s0), zero_word, zero_word2,
                                            batch, blockIdx.z - b * nz, nullptr, cs);
}

static int warp_cs_checked(cbv_ctx* ctx, const WarpSrc& s, const char* who)
{
    if (s.kind != WarpSrc::YUV || s.cs < 1 || s.cs > 3) return cbv_fail(ctx, CBV_ERR_ARG, "%s: not a YUV source in colour space 1 to 3 (%d)", who, s.cs);
    return CBV_OK;
}

int launch_warp_cs(cbv_ctx* ctx, WarpSrc s, const double* Minv9, int dw, int dh, int rot180, u8* dst, int dst_stride, size_t dst_frame_stride, int batch,
                   u32* zero_word, u32* zero_word2)
{
    RC(warp_cs_checked(ctx, s, "launch_warp_cs"));
    WarpM M;
    for (int i = 0; i < 9; i++) M.m[i] = Minv9[i];
    int bw0, bh0;
    warp_block_shape(dw, dh, &bw0, &bh0);
    const bool profile = s.ptabs != nullptr;
    const int many = profile ? raw_profile_many(s.r.fmt) : yuv_cs_many(s.r.fmt), np = profile ? s.np : 1;
    if (np <= 0 || batch <= 0 || (long long)np * warp_groups(batch, many) > 65535)
        return cbv_fail(ctx, CBV_ERR_ARG, "launch_warp_cs: %d profiles x %d frames do not fit a launch", np, batch);
    const hipStream_t st = ctx->stream;
    const YuvCs cs = kYuvCs[s.cs];
    return warp_launch(
        ctx, &s, dw, dh, np, batch,
        [&](auto fmt, auto fpt, dim3 grid, int nz) {
            constexpr int FMT = decltype(fmt)::value;
            if constexpr (raw_fmt_yuv(FMT)) {
                if (profile) {
                    constexpr int FPT = decltype(fpt)::value == 1 ? 1 : raw_profile_fpt(FMT);
                    hipLaunchKernelGGL((k_warp_raw_profile_cs<FMT, FPT>), grid, dim3(256), 0, st, s.planes.p[0], s.planes.p[1], s.planes.p[2], s.r, s.g.w, s.g.h,
                                       cs, M, dw, dh, bw0, rot180, dst, dst_stride, dst_frame_stride, s.dst_profile_stride, ctx->tabs, s.ptabs, nz, zero_word,
                                       zero_word2, batch);
                } else {
                    constexpr int FPT = decltype(fpt)::value == 1 ? 1 : yuv_cs_fpt(FMT);
                    hipLaunchKernelGGL((k_warp_yuv_cs<FMT, FPT>), grid, dim3(256), 0, st, s.planes.p[0], s.planes.p[1], s.planes.p[2], s.r, s.g.w, s.g.h, cs, M,
                                       dw, dh, bw0, rot180, dst, dst_stride, dst_frame_stride, zero_word, zero_word2, batch);
                }
            }
        },
        many);
}

int launch_warp_cs_mb(cbv_ctx* ctx, WarpSrc s, const BoardDev* tab, int nb, int maxS, int s0, int batch, u32* zero_word, u32* zero_word2)
{
    RC(warp_cs_checked(ctx, s, "launch_warp_cs_mb"));
    const bool profile = s.ptabs != nullptr;
    const hipStream_t st = ctx->stream;
    const YuvCs cs = kYuvCs[s.cs];
    return warp_launch(
        ctx, &s, maxS, maxS, nb, batch,
        [&](auto fmt, auto fpt, dim3 grid, int nz) {
            constexpr int FMT = decltype(fmt)::value;
            if constexpr (raw_fmt_yuv(FMT)) {
                if (profile) {
                    constexpr int FPT = decltype(fpt)::value == 1 ? 1 : raw_profile_fpt(FMT);
                    hipLaunchKernelGGL((k_warp_raw_profile_cs_mb<FMT, FPT>), grid, dim3(256), 0, st, s.planes.p[0], s.planes.p[1], s.planes.p[2], s.r, s.g.w,
                                       s.g.h, cs, tab, nz, s0, ctx->tabs, zero_word, zero_word2, batch);
                } else {
                    constexpr int FPT = decltype(fpt)::value == 1 ? 1 : yuv_cs_fpt(FMT);
                    hipLaunchKernelGGL((k_warp_yuv_cs_mb<FMT, FPT>), grid, dim3(256), 0, st, s.planes.p[0], s.planes.p[1], s.planes.p[2], s.r, s.g.w, s.g.h, cs,
                                       tab, nz, s0, zero_word, zero_word2, batch);
                }
            }
        },
        profile ? raw_profile_many(s.r.fmt) : yuv_cs_many(s.r.fmt));
}
