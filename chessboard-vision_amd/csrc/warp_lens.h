// The lens form of the warp kernels, for k_warp_lens.hip, k_warp_lens_profile.hip and k_warp_lens_cs.hip:
// warp_gather<Src, FPT, true>, whose coordinates go through the camera's lens model (lens_core.h) between the homography and
// the quantisation to 1/32 px.  Everything behind the coordinates is the gather's own: `interior` and `fast` are decided from
// sx, sy as before, so the wide loads and the slack behind the last frame are those of the lens-free kernels.  As in the
// other two kernel templates (warp_gather.h) the source travels by value as the kernel's first argument; the lens travels by
// value behind it (72 bytes of scalars), and only the table-driven form exists: a LensBoard per destination.  Private.
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
    // (not through warp_gather_of: its restrict destination changes these kernels' code and made the BGR form slower;
    // profiles/warp_kernels/README.md)
    const WarpDst D = {T.Minv, T.dw, T.dh, T.bw0, T.rot180, T.dst + (size_t)s0 * T.frame_stride, T.stride, T.frame_stride};
    if constexpr (Src::CS) warp_gather<Src, FPT, true>(S, D, zero_word, zero_word2, batch, blockIdx.z - e * nz, &lens, S.cs); // (a colour space other than 0)
    else warp_gather<Src, FPT, true>(S, D, zero_word, zero_word2, batch, blockIdx.z - e * nz, &lens);
}

// where launch_warp_lens and its kin write: `ne` table entries of at most max_dw x max_dh
struct WarpLensTo {
    const LensDev& lens;
    const LensBoard* tab;
    int ne, max_dw, max_dh, s0;
};

template <class Src, int MANY = warp_many<Src, true>()>
static int warp_launch_lens(cbv_ctx* ctx, const Src& S, const WarpLensTo& to, int batch, u32* zero_word, u32* zero_word2)
{
    if (!to.tab || to.ne <= 0) return cbv_fail(ctx, CBV_ERR_ARG, "launch_warp_lens: bad table, batch or destination");
    return warp_launch_grid<Src, MANY>(ctx, "launch_warp_lens", "entries", to.max_dw, to.max_dh, to.ne, batch, [&](auto fpt, dim3 grid, int nz) {
        hipLaunchKernelGGL((k_warp_lens<Src, decltype(fpt)::value>), grid, dim3(256), 0, ctx->stream, S, to.tab, to.lens, nz, to.s0, zero_word, zero_word2,
                           batch);
    });
}
