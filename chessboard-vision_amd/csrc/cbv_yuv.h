// One YUV pixel to BGR: cv2.cvtColor's COLOR_YUV2BGR_NV12 / _NV21 / _I420 / _YV12 / _YUY2 / _YVYU / _UYVY arithmetic on 8-bit
// data (include/cbv.h), the ONE definition behind k_ingest (whole frames) and the warp of a YUV frame (WarpRaw<FMT>, warp_gather.h: the four taps of a warped pixel),
// and where the bytes of each layout lie.  That is colour space 0, BT.601 limited range; the other three (BT.601 full range,
// BT.709 limited and full range) are the same arithmetic with other constants: the second half of this file.
#pragma once
#include "cbv_device.h"

// round(c * 2^20) of 1.164, 2.018, -0.391, -0.813, 1.596
enum { YUV_SHIFT = 20, YUV_CY = 1220542, YUV_CUB = 2116026, YUV_CUG = -409993, YUV_CVG = -852492, YUV_CVR = 1673527 };

// Where a format's bytes lie, from the bit fields of its id (include/cbv.h), as compile-time constants of the kernels' bodies.
// YV12 has no entry of its own: it is YUV420P with the two chroma planes swapped by the host.
template <int FMT>
struct YuvLay {
    static constexpr bool F420 = (FMT & 15) == CBV_FMT_NV12, VU = (FMT & 0x10) != 0, ALT = (FMT & 0x20) != 0;
    static constexpr bool PLANAR = F420 && ALT;
    static constexpr int CU = VU ? 1 : 0, CV = 1 - CU;                                                      // NV12 / NV21: byte of U, V in a chroma pair
    static constexpr int Y0 = ALT ? 1 : 0, Y1 = Y0 + 2, PU = (ALT ? 0 : 1) + (VU ? 2 : 0), PV = PU ^ 2; // packed 4:2:2: bytes of a pair's dword
};

// The chroma part of the three sums, rounding constant included: shared by the pixels of a 2x2 block (4:2:0) or a pair (4:2:2).
// Everything stays inside signed 32 bits: the luma term is at most (255 - 16) * 1220542 = 291 709 538, the rounding
// constant 524 288, and the chroma terms are at most 128 * 2116026 = 270 851 328 (B), 128 * (852492 + 409993) =
// 161 598 080 (G) and 128 * 1673527 = 214 211 456 (R) in magnitude: |sum| <= 563 085 154 < 2^31.
struct Chroma {
    int b, g, r;
};
__device__ __forceinline__ Chroma d_chroma(int U, int V)
{
    const int u = U - 128, v = V - 128, half = 1 << (YUV_SHIFT - 1);
    return Chroma{half + YUV_CUB * u, half + YUV_CVG * v + YUV_CUG * u, half + YUV_CVR * v};
}

// sat_u8(v >> 20) as clamp-then-shift: for v < 0 it is 0, for v >= 256 << 20 it is 255, else v >> 20 (no sign left to shift).
// Not d_sat8(v >> 20): hipcc folds two of those side by side into v_ashr_pk_u8_i32 and ORs the third byte into the same
// register as if the instruction had cleared its upper half; on the MI355X it keeps it (R came out as bits 16..23 of the
// B sum on the all-triples frame of tests/test_gpu_yuv.py, which is the guard for this).
__device__ __forceinline__ u32 d_sat8_shr20(int v) { return (u32)min(max(v, 0), (256 << YUV_SHIFT) - 1) >> YUV_SHIFT; }

// one pixel as b | g << 8 | r << 16
__device__ __forceinline__ u32 d_yuv_bgr(int Y, const Chroma& c)
{
    const int y = max(0, Y - 16) * YUV_CY;
    return d_sat8_shr20(y + c.b) | (d_sat8_shr20(y + c.g) << 8) | (d_sat8_shr20(y + c.r) << 16);
}

// ---------------------------------------------------------------------------
// The other colour spaces (include/cbv.h, CBV_CS_*): the same arithmetic with the six constants taken from a kernel
// argument.  They are uniform over a launch, so they live in scalar registers; the kernels that take them (k_ingest_cs.hip,
// k_warp_cs.hip) exist once per layout, not once per colour space.  Colour space 0 keeps the functions above, whose
// constants are the compiler's.
// Everything stays inside signed 32 bits for every row of the table: the largest magnitude a sum can reach is BT.709
// limited's B, (255 - 16) * 1220945 + 524288 + 128 * 2215014 = 575 851 935 < 2^31.
// ---------------------------------------------------------------------------
struct YuvCs {
    int cy, cub, cug, cvg, cvr, yoff;
};

// row = raw_fmt_cs(fmt), (fmt & CBV_CS_MASK) / CBV_CS_FULL: BT.601 limited (cv2's three-decimal constants, the enum above), BT.601 full (JFIF),
// BT.709 limited, BT.709 full.  Rows 1 to 3 are round(c * 2^20) of the exact coefficients (include/cbv.h has the fractions).
static constexpr YuvCs kYuvCs[4] = {
    {YUV_CY, YUV_CUB, YUV_CUG, YUV_CVG, YUV_CVR, 16},
    {1048576, 1858077, -360853, -748826, 1470104, 0},
    {1220945, 2215014, -223607, -558796, 1879825, 16},
    {1048576, 1945738, -196424, -490864, 1651297, 0},
};

__device__ __forceinline__ Chroma d_chroma(int U, int V, const YuvCs& k)
{
    const int u = U - 128, v = V - 128, half = 1 << (YUV_SHIFT - 1);
    return Chroma{half + k.cub * u, half + k.cvg * v + k.cug * u, half + k.cvr * v};
}

__device__ __forceinline__ u32 d_yuv_bgr(int Y, const Chroma& c, const YuvCs& k)
{
    const int y = max(0, Y - k.yoff) * k.cy;
    return d_sat8_shr20(y + c.b) | (d_sat8_shr20(y + c.g) << 8) | (d_sat8_shr20(y + c.r) << 16);
}
