// The warp of Motion-JPEG frames from their decoded planes: warp(k_jpeg_color(planes)), and with a colour profile
// warp(apply_color_profile(k_jpeg_color(planes))), bit for bit, with no BGR frame ever written (pipelines in planes mode
// without enhancement, their colour sweep, cbv_warp_jpeg).  The gather is warp_gather (warp_gather.h) with the sources
// WarpJpeg and WarpJpegProfile: coordinates, rot180 and the zeroed words are the gather's own; a tap at (x, y) is
// jpeg_pixel(D, planes, x, y) with the frame's own descriptor D, so gray, 4:4:4, 4:2:2 and 4:2:0 frames share a launch.
// Every address comes from the descriptor, which the host parser has validated, and from the pixel's coordinates; none
// depends on a sample, so a damaged stream changes values and nothing else.  A tap outside the frame is BGR 0.  This unit
// holds k_warp_one and k_warp_boards of the two sources, with one frame per thread and with the many-frames form (warp_many:
// four, two with a profile): 8 kernels, in a file of their own for the compile time.
#include "warp_gather.h"

int launch_warp_jpeg(cbv_ctx* ctx, WarpSrc s, const double* Minv9, int dw, int dh, int rot180, u8* dst, int dst_stride, size_t dst_frame_stride, int batch,
                     u32* zero_word, u32* zero_word2)
{
    const char* who = "launch_warp_jpeg";
    const WarpOneTo to = {Minv9, dw, dh, rot180, dst, dst_stride, dst_frame_stride, s.np, s.dst_profile_stride};
    auto go = [&](auto S) { return warp_launch_one(ctx, who, S, to, batch, zero_word, zero_word2); };
    return s.ptabs ? warp_typed_jpeg<true>(ctx, s, who, go) : warp_typed_jpeg<false>(ctx, s, who, go);
}

int launch_warp_jpeg_mb(cbv_ctx* ctx, WarpSrc s, const BoardDev* tab, int nb, int maxS, int s0, int batch, u32* zero_word, u32* zero_word2)
{
    const char* who = "launch_warp_jpeg_mb";
    auto go = [&](auto S) { return warp_launch_boards(ctx, who, S, tab, nb, maxS, s0, batch, zero_word, zero_word2); };
    return s.ptabs ? warp_typed_jpeg<true>(ctx, s, who, go) : warp_typed_jpeg<false>(ctx, s, who, go);
}
