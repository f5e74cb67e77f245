// The warp of developed mosaics (include/cbv.h: Bayer frames in a 16-bit container, MIPI RAW10 / RAW12 packed rows, and 8-bit
// mosaics with tables), lens-free: what a pipeline in raw mode runs on such an input format, with a colour profile on the taps
// or without, and what its colour sweep runs.  The gather is warp_gather (warp_gather.h) with the sources WarpDeep<LDS> and
// WarpDeepProfile<LDS>: the Bayer branch with its 4 x 4 bytes made of developed samples.  The layout and the encoding are
// uniform values of the source, so this unit holds k_warp_one and k_warp_boards of the two sources, with the tables in LDS (up
// to 12 bits) and in global memory (14 and 16 bits), with one frame per thread and with two (warp_many): 16 kernels.  The
// launchers of k_warp.hip hand a source here when WarpSrc::deep() holds; the 8-bit ids without tables keep the kernels of
// k_warp.hip and k_warp_raw_profile.hip.  The lens forms are k_warp_lens_deep.hip's.
// tests/test_bayer_deep_resources.py lists the kernels and their registers.
#include "warp_gather.h"

int launch_warp_deep(cbv_ctx* ctx, WarpSrc s, const double* Minv9, int dw, int dh, int rot180, u8* dst, int dst_stride, size_t dst_frame_stride, int batch,
                     u32* zero_word, u32* zero_word2)
{
    const char* who = "launch_warp_deep";
    const WarpOneTo to = {Minv9, dw, dh, rot180, dst, dst_stride, dst_frame_stride, s.np, s.dst_profile_stride};
    return warp_typed_deep(ctx, &s, batch, who, [&](auto S) { return warp_launch_one(ctx, who, S, to, batch, zero_word, zero_word2); });
}

int launch_warp_deep_mb(cbv_ctx* ctx, WarpSrc s, const BoardDev* tab, int nb, int maxS, int s0, int batch, u32* zero_word, u32* zero_word2)
{
    const char* who = "launch_warp_deep_mb";
    return warp_typed_deep(ctx, &s, batch, who, [&](auto S) { return warp_launch_boards(ctx, who, S, tab, nb, maxS, s0, batch, zero_word, zero_word2); });
}
