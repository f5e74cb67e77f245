// The lens forms of the warp kernels, for k_warp_lens.hip and k_warp_lens_profile.hip: warp_gather<Src, FPT, true>, whose
// coordinates go through the camera's lens model (lens_core.h) between the homography and the quantisation to 1/32 px.
// Everything behind the coordinates is the gather's own: `interior` and `fast` are decided from sx, sy as before, so the
// wide loads and the slack behind the last frame are those of the lens-free kernels.  One kernel template serves every
// source: the source travels by value as the kernel's first argument and the lens by value behind it (72 bytes of
// scalars), and only the table-driven form exists: a LensBoard per destination.  Private.
#pragma once
#include "warp_gather.h"

template <class Src, int FPT>
__global__ __launch_bounds__(256) void k_warp_lens(Src S, const LensBoard* __restrict__ tab, LensDev lens, int nz, int s0,
                                                    u32* __restrict__ zero_word, u32* __restrict__ zero_word2, int batch)
{
    const int e = blockIdx.z / nz;
    const LensBoard& T = tab[e];
    if (e > 0 && ((int)blockIdx.x * 64 >= T.dw || (int)blockIdx.y * Src::ROWS >= T.dh)) return;
    if constexpr (Src::TABS) S.pt = T.ptabs; // the profile is the entry's: a workgroup stages its entry's table
    const WarpDst D = {T.Minv, T.dw, T.dh, T.bw0, T.rot180, T.dst + (size_t)s0 * T.frame_stride, T.stride, T.frame_stride};
    if constexpr (Src::CS) warp_gather<Src, FPT, true>(S, D, zero_word, zero_word2, batch, blockIdx.z - e * nz, &lens, S.cs); // (a colour space other than 0)
    else warp_gather<Src, FPT, true>(S, D, zero_word, zero_word2, batch, blockIdx.z - e * nz, &lens);
}

// One launch of source S over `ne` table entries: one frame per thread below batch 8, MANY from there on.
template <class Src, int MANY>
static int warp_lens_launch(cbv_ctx* ctx, const Src& S, int prof, const LensDev& lens, const LensBoard* tab, int ne, int max_dw, int max_dh, int s0,
                            int batch, u32* zero_word, u32* zero_word2)
{
    if (!tab || ne <= 0 || batch <= 0 || max_dw < 1 || max_dh < 1) return cbv_fail(ctx, CBV_ERR_ARG, "launch_warp_lens: bad table, batch or destination");
    const int nz = warp_groups(batch, MANY);
    if ((long long)nz * ne > 65535) return cbv_fail(ctx, CBV_ERR_ARG, "launch_warp_lens: %d entries x %d frames do not fit a launch", ne, batch);
    const dim3 grid((max_dw + 63) / 64, (max_dh + Src::ROWS - 1) / Src::ROWS, nz * ne);
    prof_begin(ctx, prof);
    if (batch >= 8) hipLaunchKernelGGL((k_warp_lens<Src, MANY>), grid, dim3(256), 0, ctx->stream, S, tab, lens, nz, s0, zero_word, zero_word2, batch);
    else hipLaunchKernelGGL((k_warp_lens<Src, 1>), grid, dim3(256), 0, ctx->stream, S, tab, lens, nz, s0, zero_word, zero_word2, batch);
    prof_end(ctx, prof);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

// what a source of JPEG planes must be (warp_jpeg_launch of k_warp_jpeg.hip asks the same)
static int warp_lens_jpeg_checked(cbv_ctx* ctx, const WarpSrc& s)
{
    if (s.kind != WarpSrc::JPEG || !s.jpeg_planes || !s.jpeg_descs || (s.jpeg_plane_stride & 7) || s.g.w < 1 || s.g.h < 1)
        return cbv_fail(ctx, CBV_ERR_ARG, "launch_warp_lens: not a source of JPEG planes");
    return CBV_OK;
}
