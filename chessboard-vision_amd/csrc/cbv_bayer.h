// One site of an 8-bit Bayer mosaic to BGR: cv2.cvtColor's bilinear COLOR_Bayer??2BGR (include/cbv.h), the ONE definition
// behind k_ingest (whole frames) and the warp of a mosaic (WarpRaw<FMT>, warp_gather.h: the four taps of a warped pixel), and which colour a site carries.
#pragma once
#include "cbv_device.h"

// Which colour site (x, y) carries, from the bit fields of the format's id (include/cbv.h), as compile-time constants of the
// kernels' bodies.  A layout that starts with green (0x20) is its sibling moved one column, so a site is looked up in
// RGGB's 2 x 2 block at (ex(x), y & 1): (0, 0) and (1, 1) carry the two chroma colours C0 and C1, the other two are green,
// with C0 beside them in even rows and above and below them in odd rows.  C0 is red, or blue with bit 0x10.
template <int FMT>
struct BayerLay {
    static constexpr bool BX = (FMT & 0x10) != 0, GF = (FMT & 0x20) != 0;
    __device__ static __forceinline__ int ex(int x) { return (x & 1) ^ (GF ? 1 : 0); }
};

// The demosaiced pixel of site (x, y) as b | g << 8 | r << 16.  ra, rb, rc = the rows y - 1, y, y + 1 of the mosaic, each
// with the bytes of columns x - 1, x, x + 1 in bits 0..7, 8..15, 16..23 (higher bits are ignored).  The site is an
// interior one (1 <= x <= w - 2, 1 <= y <= h - 2): callers clamp an edge site first and pass the clamped site's
// neighbourhood and coordinates, so nothing here reads outside the frame.  The five candidate sums are worked out whatever
// the site's phase and selected: the phase differs from lane to lane in the warp, and is a constant in k_ingest, where
// the unused sums fold away.
template <int FMT>
__device__ __forceinline__ u32 d_bayer_bgr(int x, int y, u32 ra, u32 rb, u32 rc)
{
    typedef BayerLay<FMT> L;
    const int a0 = (int)(ra & 255u), a1 = (int)((ra >> 8) & 255u), a2 = (int)((ra >> 16) & 255u);
    const int b0 = (int)(rb & 255u), b1 = (int)((rb >> 8) & 255u), b2 = (int)((rb >> 16) & 255u);
    const int c0 = (int)(rc & 255u), c1 = (int)((rc >> 8) & 255u), c2 = (int)((rc >> 16) & 255u);
    const int cross = (b0 + b2 + a1 + c1 + 2) >> 2;
    const int diag = (a0 + a2 + c0 + c2 + 2) >> 2;
    const int hp = (b0 + b2 + 1) >> 1, vp = (a1 + c1 + 1) >> 1;
    const bool odd_row = (y & 1) != 0, green = L::ex(x) != (y & 1);
    const int g = green ? b1 : cross;
    const int k0 = green ? (odd_row ? vp : hp) : (odd_row ? diag : b1); // C0
    const int k1 = green ? (odd_row ? hp : vp) : (odd_row ? b1 : diag); // C1
    const int r = L::BX ? k1 : k0, b = L::BX ? k0 : k1;
    return (u32)b | ((u32)g << 8) | ((u32)r << 16);
}
