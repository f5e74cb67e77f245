// The warp of camera-native frames through the colour profile: warp(apply_color_profile(to_bgr(raw))), bit for bit, with
// neither the BGR frame nor the profiled frame ever written (pipelines configured with CBV_SKIP_ENHANCE_PROFILE_RAW, their
// colour sweep, cbv_warp_color_profile_raw).  The gather is warp_gather (warp_gather.h) with the source WarpRawProfile<FMT>:
// coordinates, wide loads, the `fast` predicate per family, rot180 and the zeroed words are the gather's own; what this
// source adds is d_profile_px on each converted tap inside the frame, from the 7.5 KB of tables a workgroup stages once for
// its WP_ROWS rows.  A tap outside the frame is BGR 0, not the profile of black; a table with enabled = 0 leaves the taps
// alone.  This unit holds k_warp_one and k_warp_boards of WarpRawProfile<FMT> for the six YUV and four Bayer layouts, with one
// frame per thread and with the family's many-frames form (warp_many): 40 kernels, in a file of their own for the compile time.
#include "warp_gather.h"

int launch_warp_raw_profile(cbv_ctx* ctx, WarpSrc s, const double* Minv9, int dw, int dh, int rot180, u8* dst, int dst_stride, size_t dst_frame_stride,
                            int batch, u32* zero_word, u32* zero_word2)
{
    const char* who = "launch_warp_raw_profile";
    const WarpOneTo to = {Minv9, dw, dh, rot180, dst, dst_stride, dst_frame_stride, s.np, s.dst_profile_stride};
    return warp_typed_raw_profile(ctx, &s, batch, who, [&](auto S) { return warp_launch_one(ctx, who, S, to, batch, zero_word, zero_word2); });
}

int launch_warp_raw_profile_mb(cbv_ctx* ctx, WarpSrc s, const BoardDev* tab, int nb, int maxS, int s0, int batch, u32* zero_word, u32* zero_word2)
{
    const char* who = "launch_warp_raw_profile_mb";
    return warp_typed_raw_profile(ctx, &s, batch, who, [&](auto S) { return warp_launch_boards(ctx, who, S, tab, nb, maxS, s0, batch, zero_word, zero_word2); });
}
