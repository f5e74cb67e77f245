// cv2.warpPerspective(img, M, (S,S)) INTER_LINEAR / BORDER_CONSTANT(0)
// (board_detection.py:70), optional cv2.rotate(ROTATE_180) (game_session.py:126)
// and — for the fused pipeline — cv2.normalize folded into the gather (a byte
// map commutes with sampling: the four taps are mapped before interpolation).
//
// Coordinates follow WarpPerspectiveInvoker exactly: the destination is cut
// into 64 x 16 blocks (BLOCK_SZ = 32), X0/Y0/W0 are evaluated at the block's
// left edge and advanced by M*x1 inside the block, in double, one rounding per
// operation; coordinates are quantised to 1/32 px and sampled with the 15-bit
// fixed-point bilinear table of remap().
// Also here: the synthetic frame generator used by bench/tests.
#include "cbv_bayer.h"
#include "cbv_profile_px.h"
#include "cbv_yuv.h"

struct WarpM {
    double m[9];
};

// What a destination pixel samples, whatever the format of the frames: the top-left tap, the four weights, which taps are
// inside the source, and where the pixel goes.  (warp_body and warp_yuv_body share it.)
struct WarpTaps {
    int sx, sy;
    int w00, w01, w10, w11;
    bool any_in, x0in, x1in, y0in, y1in, interior;
    size_t out_off; // byte offset of the pixel inside a destination frame
};

// destination pixel (dx, dy) of a dw x dh destination; sw x sh = the source frame
__device__ __forceinline__ WarpTaps warp_taps(int dx, int dy, int sw, int sh, const double* __restrict__ M, int dw, int dh, int bw0, int rot180,
                                              int dst_stride)
{
    WarpTaps t;
    const int bx = (dx / bw0) * bw0, x1 = dx - bx; // block origin and offset inside it
    // (rows are evaluated independently of the block row)
    const double X0 = M[0] * bx + M[1] * dy + M[2];
    const double Y0 = M[3] * bx + M[4] * dy + M[5];
    const double W0 = M[6] * bx + M[7] * dy + M[8];
    double W = W0 + M[6] * x1;
    W = W != 0. ? 32. / W : 0.;
    double fX = (X0 + M[0] * x1) * W;
    double fY = (Y0 + M[3] * x1) * W;
    fX = fmax(-2147483648.0, fmin(2147483647.0, fX));
    fY = fmax(-2147483648.0, fmin(2147483647.0, fY));
    const int X = d_round_d(fX), Y = d_round_d(fY);
    const int sx = min(max(X >> 5, -32768), 32767), sy = min(max(Y >> 5, -32768), 32767);
    const int fx = X & 31, fy = Y & 31;
    t.sx = sx;
    t.sy = sy;
    t.w00 = (32 - fx) * (32 - fy) * 32;
    t.w01 = fx * (32 - fy) * 32;
    t.w10 = (32 - fx) * fy * 32;
    t.w11 = fx * fy * 32;
    t.any_in = !(sx >= sw || sx + 1 < 0 || sy >= sh || sy + 1 < 0);
    t.x0in = sx >= 0 && sx < sw;
    t.x1in = sx + 1 >= 0 && sx + 1 < sw;
    t.y0in = sy >= 0 && sy < sh;
    t.y1in = sy + 1 >= 0 && sy + 1 < sh;
    t.interior = t.x0in && t.x1in && t.y0in && t.y1in;
    const int ox = rot180 ? dw - 1 - dx : dx, oy = rot180 ? dh - 1 - dy : dy;
    t.out_off = (size_t)oy * dst_stride + (size_t)ox * 3;
    return t;
}

// the pipeline's HoughCircles worklist counter, filled by the NEXT kernel in the stream (k_squares_pre5_stats):
// zeroed here instead of by a 4-byte memset, which is one more ~4.5 us launch in a single-frame run
__device__ __forceinline__ void warp_zero_words(u32* __restrict__ zero_word, u32* __restrict__ zero_word2)
{
    if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) {
        if (zero_word) *zero_word = 0u;
        if (zero_word2) *zero_word2 = 0u; // the run's second-pass list, when this launch is the run's only chunk
    }
}

// remap()'s 15-bit fixed-point bilinear of one channel
__device__ __forceinline__ int warp_blend(int t0, int t1, int t2, int t3, const WarpTaps& t)
{
    return d_sat8((t0 * t.w00 + t1 * t.w01 + t2 * t.w10 + t3 * t.w11 + (1 << 14)) >> 15);
}

// FPT frames per thread: the coordinates of a destination pixel depend on the matrix and the pixel, not on the frame, and
// they are most of the kernel's instructions (about 100 of 190 per output pixel, in double precision): a thread works
// them out once and samples FPT consecutive frames of the batch with them (blockIdx.z counts groups of FPT frames).
// CALC: the byte map is worked out here from the frames' [min, max] words (NormSrc::minmax) instead of read from a table.
// (the body of k_warp and k_warp_mb; bz = the group of frames, blockIdx.z of a single-board launch)
template <int FPT, bool CALC>
__device__ __forceinline__ void warp_body(const u8* __restrict__ src, Geom g, const double* __restrict__ M, int dw, int dh, int bw0,
                                          int bh0, int rot180, u8* __restrict__ dst, int dst_stride,
                                          size_t dst_frame_stride, const u8* __restrict__ norm_lut, const u32* __restrict__ minmax,
                                          size_t mm_stride, u32* __restrict__ zero_word, u32* __restrict__ zero_word2, int batch, int bz)
{
    __shared__ u8 lut[FPT][256];
    warp_zero_words(zero_word, zero_word2);
    const bool use_lut = CALC || norm_lut != nullptr;
    const int f0 = bz * FPT;
    const int nf = min(FPT, batch - f0);
    if (CALC) {
#pragma unroll
        for (int k = 0; k < FPT; k++)
            if (k < nf) {
                const u32* mm = minmax + (size_t)(f0 + k) * mm_stride;
                lut[k][threadIdx.x] = d_norm_lut_entry((int)mm[0], (int)mm[1], (int)threadIdx.x);
            }
    } else if (use_lut)
#pragma unroll
        for (int k = 0; k < FPT; k++)
            if (k < nf) lut[k][threadIdx.x] = norm_lut[(size_t)(f0 + k) * 256 + threadIdx.x];
    __syncthreads();
    (void)bh0;
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (dx >= dw || dy >= dh) return;
    const WarpTaps t = warp_taps(dx, dy, g.w, g.h, M, dw, dh, bw0, rot180, dst_stride);
    const size_t tap = (size_t)t.sy * g.stride + (size_t)t.sx * 3; // (only dereferenced where the taps are inside)
    // interior: the two taps of a row are 6 contiguous bytes -> ONE unaligned 8-byte load per row instead of six byte
    // loads (the gather is bound by the number of memory instructions, not by bytes); the two bytes read past the second
    // tap stay inside the buffer (callers keep >= 8 bytes of slack behind the last frame).  All frames' loads are issued
    // before the first is used.
    u64 ta[FPT], tb[FPT];
    if (t.interior)
#pragma unroll
        for (int k = 0; k < FPT; k++)
            if (k < nf) {
                const u8* p00 = src + (size_t)(f0 + k) * g.frame_stride + tap;
                __builtin_memcpy(&ta[k], p00, 8);
                __builtin_memcpy(&tb[k], p00 + g.stride, 8);
            }
#pragma unroll
    for (int k = 0; k < FPT; k++) {
        if (k >= nf) break;
        int o[3] = {0, 0, 0};
        if (t.any_in) {
            int v[4][3]; // taps 00, 01, 10, 11
            if (t.interior) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    v[0][c] = (int)((ta[k] >> (8 * c)) & 255);
                    v[1][c] = (int)((ta[k] >> (8 * (3 + c))) & 255);
                    v[2][c] = (int)((tb[k] >> (8 * c)) & 255);
                    v[3][c] = (int)((tb[k] >> (8 * (3 + c))) & 255);
                }
            } else {
                const u8* p00 = src + (size_t)(f0 + k) * g.frame_stride + tap;
                const u8* p10 = p00 + g.stride;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    v[0][c] = (t.x0in && t.y0in) ? p00[c] : -1;
                    v[1][c] = (t.x1in && t.y0in) ? p00[3 + c] : -1;
                    v[2][c] = (t.x0in && t.y1in) ? p10[c] : -1;
                    v[3][c] = (t.x1in && t.y1in) ? p10[3 + c] : -1;
                }
            }
#pragma unroll
            for (int c = 0; c < 3; c++) {
                int q[4];
#pragma unroll
                for (int i = 0; i < 4; i++) q[i] = v[i][c] < 0 ? 0 : (use_lut ? (int)lut[k][v[i][c]] : v[i][c]); // border taps are 0
                o[c] = warp_blend(q[0], q[1], q[2], q[3], t);
            }
        }
        u8* q = dst + (size_t)(f0 + k) * dst_frame_stride + t.out_off;
        q[0] = (u8)o[0];
        q[1] = (u8)o[1];
        q[2] = (u8)o[2];
    }
}

// ---------------------------------------------------------------------------
// The warp straight from camera-native frames (pipelines without enhancement whose input format is a YUV format): the
// BGR frame k_ingest would write is never made.  The conversion is pointwise (a pixel takes the chroma of its 2x2 block
// or pair, nothing is interpolated), so converting the four taps and blending them is, bit for bit, sampling the
// converted frame: same coordinates (warp_taps), same conversion (d_yuv_bgr), same blend (warp_blend).  A tap outside
// the frame is BGR (0, 0, 0) as in k_warp, not the conversion of zero YUV.
// ---------------------------------------------------------------------------
// pixel (x, y) of one raw frame with byte loads (the taps of pixels on the frame's border)
template <int FMT>
__device__ __forceinline__ u32 d_raw_px(const u8* __restrict__ f0, const u8* __restrict__ f1, const u8* __restrict__ f2, const RawGeom& r, int x,
                                        int y)
{
    typedef YuvLay<FMT> L;
    if (L::PLANAR)
        return d_yuv_bgr(f0[(size_t)y * r.stride0 + x],
                         d_chroma(f1[(size_t)(y >> 1) * r.stride1 + (x >> 1)], f2[(size_t)(y >> 1) * r.stride2 + (x >> 1)]));
    if (L::F420) {
        const u8* c = f1 + (size_t)(y >> 1) * r.stride1 + (x & ~1);
        return d_yuv_bgr(f0[(size_t)y * r.stride0 + x], d_chroma(c[L::CU], c[L::CV]));
    }
    const u8* s = f0 + (size_t)y * r.stride0 + (size_t)(x >> 1) * 4;
    return d_yuv_bgr(s[L::Y0 + (x & 1) * 2], d_chroma(s[L::PU], s[L::PV]));
}

// the chroma of byte pair `p` of an NV12 (U V) / NV21 (V U) row
template <int FMT>
__device__ __forceinline__ Chroma d_chroma_pair(u32 p)
{
    return d_chroma((p >> (8 * YuvLay<FMT>::CU)) & 255, (p >> (8 * YuvLay<FMT>::CV)) & 255);
}

// Interior pixels, per frame and row of taps.  NV12 / NV21: one 2-byte load holds both luma samples and one 4-byte load at
// the even column holds the chroma of the first tap's pair and of the next pair, which is the second tap's when sx is odd
// (when sx is even both taps share the first); the rows share the chroma row when sy is even.  Planar chroma (YUV420P; YV12
// arrives with p1 and p2 swapped): the same 2-byte luma load, and per chroma row one 2-byte load of U and one of V at column
// sx >> 1, which hold the first tap's sample and the next, the second tap's when sx is odd.  Packed 4:2:2: one 8-byte load
// at the first tap's pair, e.g. Y0 U Y1 V | Y2 U Y3 V, holds both taps and their chroma for either parity.  The bytes read
// past the second tap's pair (sx even) stay inside the buffer: the ring keeps 256 bytes of slack behind the last frame.
template <int FMT, int FPT>
__device__ __forceinline__ void warp_yuv_body(const u8* __restrict__ p0, const u8* __restrict__ p1, const u8* __restrict__ p2, RawGeom r, int sw,
                                              int sh, const double* __restrict__ M, int dw, int dh, int bw0, int rot180, u8* __restrict__ dst,
                                              int dst_stride, size_t dst_frame_stride, u32* __restrict__ zero_word,
                                              u32* __restrict__ zero_word2, int batch, int bz)
{
    typedef YuvLay<FMT> L;
    warp_zero_words(zero_word, zero_word2);
    const int f0 = bz * FPT;
    const int nf = min(FPT, batch - f0);
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (dx >= dw || dy >= dh) return;
    const WarpTaps t = warp_taps(dx, dy, sw, sh, M, dw, dh, bw0, rot180, dst_stride);
    const bool odd = t.sx & 1;
    constexpr bool NV12 = L::F420 && !L::PLANAR, PLANAR = L::PLANAR;
    const bool two_crows = L::F420 && (t.sy & 1); // the rows of taps lie in different chroma rows
    // (offsets are only used where the taps are inside)
    const size_t l_off = L::F420 ? (size_t)t.sy * r.stride0 + (size_t)t.sx : (size_t)t.sy * r.stride0 + (size_t)(t.sx >> 1) * 4;
    const size_t c_off = (size_t)(t.sy >> 1) * r.stride1 + (size_t)(PLANAR ? t.sx >> 1 : t.sx & ~1);
    const size_t c2_off = (size_t)(t.sy >> 1) * r.stride2 + (size_t)(t.sx >> 1);
    u64 la[FPT], lb[FPT]; // 4:2:0: 2 luma bytes; 4:2:2: the 8 bytes of two pairs
    u32 ca[FPT], cb[FPT]; // NV12: U V U V; planar: U U
    u32 va[FPT], vb[FPT]; // planar: V V
    if (t.interior)
#pragma unroll
        for (int k = 0; k < FPT; k++)
            if (k < nf) {
                const u8* l = p0 + (size_t)(f0 + k) * r.frame_stride + l_off;
                if (L::F420) {
                    u16 a, b;
                    __builtin_memcpy(&a, l, 2);
                    __builtin_memcpy(&b, l + r.stride0, 2);
                    la[k] = a;
                    lb[k] = b;
                    const u8* c = p1 + (size_t)(f0 + k) * r.frame_stride + c_off;
                    if (NV12) {
                        __builtin_memcpy(&ca[k], c, 4);
                        cb[k] = ca[k];
                        if (two_crows) __builtin_memcpy(&cb[k], c + r.stride1, 4);
                    } else {
                        const u8* c2 = p2 + (size_t)(f0 + k) * r.frame_stride + c2_off;
                        u16 u, v;
                        __builtin_memcpy(&u, c, 2);
                        __builtin_memcpy(&v, c2, 2);
                        ca[k] = cb[k] = u;
                        va[k] = vb[k] = v;
                        if (two_crows) {
                            __builtin_memcpy(&u, c + r.stride1, 2);
                            __builtin_memcpy(&v, c2 + r.stride2, 2);
                            cb[k] = u;
                            vb[k] = v;
                        }
                    }
                } else {
                    __builtin_memcpy(&la[k], l, 8);
                    __builtin_memcpy(&lb[k], l + r.stride0, 8);
                }
            }
#pragma unroll
    for (int k = 0; k < FPT; k++) {
        if (k >= nf) break;
        int o[3] = {0, 0, 0};
        if (t.any_in) {
            u32 q[4] = {0u, 0u, 0u, 0u}; // taps 00, 01, 10, 11 as b | g << 8 | r << 16; border taps are 0
            if (t.interior) {
                if (L::F420) {
                    Chroma a0, a1, b0, b1;
                    if (NV12) {
                        const u32 a = ca[k], sa = odd ? a >> 16 : a;
                        a0 = d_chroma_pair<FMT>(a);
                        a1 = d_chroma_pair<FMT>(sa);
                        b0 = a0;
                        b1 = a1;
                        if (two_crows) {
                            const u32 b = cb[k], sb = odd ? b >> 16 : b;
                            b0 = d_chroma_pair<FMT>(b);
                            b1 = d_chroma_pair<FMT>(sb);
                        }
                    } else {
                        const u32 u = ca[k], v = va[k];
                        a0 = d_chroma(u & 255, v & 255);
                        a1 = d_chroma((odd ? u >> 8 : u) & 255, (odd ? v >> 8 : v) & 255);
                        b0 = a0;
                        b1 = a1;
                        if (two_crows) {
                            const u32 u1 = cb[k], v1 = vb[k];
                            b0 = d_chroma(u1 & 255, v1 & 255);
                            b1 = d_chroma((odd ? u1 >> 8 : u1) & 255, (odd ? v1 >> 8 : v1) & 255);
                        }
                    }
                    q[0] = d_yuv_bgr((int)(la[k] & 255), a0);
                    q[1] = d_yuv_bgr((int)((la[k] >> 8) & 255), a1);
                    q[2] = d_yuv_bgr((int)(lb[k] & 255), b0);
                    q[3] = d_yuv_bgr((int)((lb[k] >> 8) & 255), b1);
                } else {
#pragma unroll
                    for (int row = 0; row < 2; row++) {
                        const u64 w = row ? lb[k] : la[k];
                        const u32 lo = (u32)w, hi = (u32)(w >> 32), s1 = odd ? hi : lo;
                        const Chroma c0 = d_chroma((lo >> (8 * L::PU)) & 255, (lo >> (8 * L::PV)) & 255);
                        const Chroma c1 = d_chroma((s1 >> (8 * L::PU)) & 255, (s1 >> (8 * L::PV)) & 255);
                        q[2 * row] = d_yuv_bgr((int)((odd ? lo >> (8 * L::Y1) : lo >> (8 * L::Y0)) & 255), c0);
                        q[2 * row + 1] = d_yuv_bgr((int)((odd ? hi >> (8 * L::Y0) : lo >> (8 * L::Y1)) & 255), c1);
                    }
                }
            } else {
                const u8* f0p = p0 + (size_t)(f0 + k) * r.frame_stride;
                const u8* f1p = L::F420 ? p1 + (size_t)(f0 + k) * r.frame_stride : nullptr;
                const u8* f2p = PLANAR ? p2 + (size_t)(f0 + k) * r.frame_stride : nullptr;
                if (t.x0in && t.y0in) q[0] = d_raw_px<FMT>(f0p, f1p, f2p, r, t.sx, t.sy);
                if (t.x1in && t.y0in) q[1] = d_raw_px<FMT>(f0p, f1p, f2p, r, t.sx + 1, t.sy);
                if (t.x0in && t.y1in) q[2] = d_raw_px<FMT>(f0p, f1p, f2p, r, t.sx, t.sy + 1);
                if (t.x1in && t.y1in) q[3] = d_raw_px<FMT>(f0p, f1p, f2p, r, t.sx + 1, t.sy + 1);
            }
#pragma unroll
            for (int c = 0; c < 3; c++)
                o[c] = warp_blend((int)((q[0] >> (8 * c)) & 255), (int)((q[1] >> (8 * c)) & 255), (int)((q[2] >> (8 * c)) & 255),
                                  (int)((q[3] >> (8 * c)) & 255), t);
        }
        u8* out = dst + (size_t)(f0 + k) * dst_frame_stride + t.out_off;
        out[0] = (u8)o[0];
        out[1] = (u8)o[1];
        out[2] = (u8)o[2];
    }
}

template <int FMT, int FPT>
__global__ __launch_bounds__(256) void k_warp_yuv(const u8* __restrict__ p0, const u8* __restrict__ p1, const u8* __restrict__ p2, RawGeom r, int sw, int sh, WarpM M,
                                                   int dw, int dh, int bw0, int rot180, u8* __restrict__ dst, int dst_stride,
                                                   size_t dst_frame_stride, u32* __restrict__ zero_word, u32* __restrict__ zero_word2, int batch)
{
    warp_yuv_body<FMT, FPT>(p0, p1, p2, r, sw, sh, M.m, dw, dh, bw0, rot180, dst, dst_stride, dst_frame_stride, zero_word, zero_word2, batch,
                            blockIdx.z);
}

// every board of a pipeline in one launch, as k_warp_mb
template <int FMT, int FPT>
__global__ __launch_bounds__(256) void k_warp_yuv_mb(const u8* __restrict__ p0, const u8* __restrict__ p1, const u8* __restrict__ p2, RawGeom r, int sw, int sh,
                                                      const BoardDev* __restrict__ tab, int nz, int s0, u32* __restrict__ zero_word,
                                                      u32* __restrict__ zero_word2, int batch)
{
    const int b = blockIdx.z / nz;
    const BoardDev& T = tab[b];
    if (b > 0 && ((int)blockIdx.x * 64 >= T.S || (int)blockIdx.y * 4 >= T.S)) return;
    warp_yuv_body<FMT, FPT>(p0, p1, p2, r, sw, sh, T.Minv, T.S, T.S, T.bw0, T.rot180, T.warped + (size_t)s0 * T.warped_stride, T.S * 3,
                            T.warped_stride, zero_word, zero_word2, batch, blockIdx.z - b * nz);
}

// ---------------------------------------------------------------------------
// The warp straight from 8-bit Bayer mosaics (pipelines without enhancement whose input format is a Bayer format):
// k_warp_yuv's gather with the four taps demosaiced (d_bayer_bgr, cbv_bayer.h) before the blend.  A tap is a pixel of the
// frame k_ingest would write, so demosaicing the taps and blending them is, bit for bit, sampling that frame: same
// coordinates (warp_taps), same conversion, same blend (warp_blend).  A tap outside the frame is BGR (0, 0, 0); a tap on
// the frame's outermost rows or columns is the result of the clamped site, as in k_ingest.
// ---------------------------------------------------------------------------
// pixel (x, y) of one mosaic, inside the frame, with byte loads: the site is clamped, its neighbourhood lies inside
template <int FMT>
__device__ __forceinline__ u32 d_bayer_px(const u8* __restrict__ f0, int stride, int w, int h, int x, int y)
{
    const int cx = min(max(x, 1), w - 2), cy = min(max(y, 1), h - 2);
    const u8* m = f0 + (size_t)cy * stride + cx;
    u32 row[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const u8* q = m + (ptrdiff_t)(i - 1) * stride;
        row[i] = (u32)q[-1] | ((u32)q[0] << 8) | ((u32)q[1] << 16);
    }
    return d_bayer_bgr<FMT>(cx, cy, row[0], row[1], row[2]);
}

// Pixels whose four taps are all interior sites (1 <= sx, sx + 1 <= w - 2, the same in y): the taps' 3 x 3 neighbourhoods
// lie in the 4 x 4 bytes at (sx - 1, sy - 1), which is four unaligned 4-byte loads per frame, inside the frame's rows.
// Everything else with a tap inside the frame takes d_bayer_px per tap.
template <int FMT, int FPT>
__device__ __forceinline__ void warp_bayer_body(const u8* __restrict__ p0, RawGeom r, int sw, int sh, const double* __restrict__ M, int dw, int dh,
                                                int bw0, int rot180, u8* __restrict__ dst, int dst_stride, size_t dst_frame_stride,
                                                u32* __restrict__ zero_word, u32* __restrict__ zero_word2, int batch, int bz)
{
    warp_zero_words(zero_word, zero_word2);
    const int f0 = bz * FPT;
    const int nf = min(FPT, batch - f0);
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (dx >= dw || dy >= dh) return;
    const WarpTaps t = warp_taps(dx, dy, sw, sh, M, dw, dh, bw0, rot180, dst_stride);
    const bool inner = t.sx >= 1 && t.sx + 2 < sw && t.sy >= 1 && t.sy + 2 < sh;
    const size_t off = (size_t)(t.sy - 1) * r.stride0 + (size_t)(t.sx - 1); // (only used where inner)
    u32 rows[FPT][4];
    if (inner)
#pragma unroll
        for (int k = 0; k < FPT; k++)
            if (k < nf) {
                const u8* m = p0 + (size_t)(f0 + k) * r.frame_stride + off;
#pragma unroll
                for (int i = 0; i < 4; i++) __builtin_memcpy(&rows[k][i], m + (size_t)i * r.stride0, 4);
            }
#pragma unroll
    for (int k = 0; k < FPT; k++) {
        if (k >= nf) break;
        int o[3] = {0, 0, 0};
        if (t.any_in) {
            u32 q[4] = {0u, 0u, 0u, 0u}; // taps 00, 01, 10, 11 as b | g << 8 | r << 16; border taps are 0
            if (inner) {
                const u32* w = rows[k];
                q[0] = d_bayer_bgr<FMT>(t.sx, t.sy, w[0], w[1], w[2]);
                q[1] = d_bayer_bgr<FMT>(t.sx + 1, t.sy, w[0] >> 8, w[1] >> 8, w[2] >> 8);
                q[2] = d_bayer_bgr<FMT>(t.sx, t.sy + 1, w[1], w[2], w[3]);
                q[3] = d_bayer_bgr<FMT>(t.sx + 1, t.sy + 1, w[1] >> 8, w[2] >> 8, w[3] >> 8);
            } else {
                const u8* fp = p0 + (size_t)(f0 + k) * r.frame_stride;
                if (t.x0in && t.y0in) q[0] = d_bayer_px<FMT>(fp, r.stride0, sw, sh, t.sx, t.sy);
                if (t.x1in && t.y0in) q[1] = d_bayer_px<FMT>(fp, r.stride0, sw, sh, t.sx + 1, t.sy);
                if (t.x0in && t.y1in) q[2] = d_bayer_px<FMT>(fp, r.stride0, sw, sh, t.sx, t.sy + 1);
                if (t.x1in && t.y1in) q[3] = d_bayer_px<FMT>(fp, r.stride0, sw, sh, t.sx + 1, t.sy + 1);
            }
#pragma unroll
            for (int c = 0; c < 3; c++)
                o[c] = warp_blend((int)((q[0] >> (8 * c)) & 255), (int)((q[1] >> (8 * c)) & 255), (int)((q[2] >> (8 * c)) & 255),
                                  (int)((q[3] >> (8 * c)) & 255), t);
        }
        u8* out = dst + (size_t)(f0 + k) * dst_frame_stride + t.out_off;
        out[0] = (u8)o[0];
        out[1] = (u8)o[1];
        out[2] = (u8)o[2];
    }
}

template <int FMT, int FPT>
__global__ __launch_bounds__(256) void k_warp_bayer(const u8* __restrict__ p0, RawGeom r, int sw, int sh, WarpM M, int dw, int dh, int bw0, int rot180,
                                                     u8* __restrict__ dst, int dst_stride, size_t dst_frame_stride, u32* __restrict__ zero_word,
                                                     u32* __restrict__ zero_word2, int batch)
{
    warp_bayer_body<FMT, FPT>(p0, r, sw, sh, M.m, dw, dh, bw0, rot180, dst, dst_stride, dst_frame_stride, zero_word, zero_word2, batch, blockIdx.z);
}

// every board of a pipeline in one launch, as k_warp_mb
template <int FMT, int FPT>
__global__ __launch_bounds__(256) void k_warp_bayer_mb(const u8* __restrict__ p0, RawGeom r, int sw, int sh, const BoardDev* __restrict__ tab, int nz,
                                                        int s0, u32* __restrict__ zero_word, u32* __restrict__ zero_word2, int batch)
{
    const int b = blockIdx.z / nz;
    const BoardDev& T = tab[b];
    if (b > 0 && ((int)blockIdx.x * 64 >= T.S || (int)blockIdx.y * 4 >= T.S)) return;
    warp_bayer_body<FMT, FPT>(p0, r, sw, sh, T.Minv, T.S, T.S, T.bw0, T.rot180, T.warped + (size_t)s0 * T.warped_stride, T.S * 3, T.warped_stride,
                              zero_word, zero_word2, batch, blockIdx.z - b * nz);
}

// ---------------------------------------------------------------------------
// The warp with the colour profile applied to its taps (cbv_warp_color_profile, pipelines configured with
// CBV_SKIP_ENHANCE_PROFILE, cbv_pipeline_color_sweep): apply_color_profile is a function of the pixel alone, so converting
// the four taps and blending them is, byte for byte, sampling the converted frame: same coordinates (warp_taps), same
// conversion (d_profile_px), same blend (warp_blend).  A tap outside the frame is BGR (0, 0, 0) as in k_warp, not the
// profile of black.  This is k_warp_yuv's arrangement with d_profile_px in the place of d_yuv_bgr.
// A workgroup stages the 7.5 KB d_profile_px reads (ProfileLds) and then covers WP_ROWS destination rows of its 64
// columns, FPT frames each: 1920 staged words against 4096 conversions per frame.  The tables are an argument, one
// ProfileTabs per profile of the launch (the grid's z runs over profile x group of frames); a table with enabled = 0
// leaves the taps as they are.
// ---------------------------------------------------------------------------
#define WP_ROWS 16 // destination rows per workgroup: one row of WarpPerspectiveInvoker's 64 x 16 blocks

// bz = the group of frames, pt = the profile's table; src and dst = frame 0 of the batch (for this profile)
template <int FPT>
__device__ __forceinline__ void warp_profile_body(const u8* __restrict__ src, Geom g, const double* __restrict__ M, int dw, int dh, int bw0,
                                                  int rot180, u8* __restrict__ dst, int dst_stride, size_t dst_frame_stride,
                                                  const StaticTabs* __restrict__ st, const ProfileTabs* __restrict__ pt,
                                                  u32* __restrict__ zero_word, u32* __restrict__ zero_word2, int batch, int bz)
{
    __shared__ ProfileLds L;
    warp_zero_words(zero_word, zero_word2);
    lds_copy(L.sdiv, st->sdiv, sizeof(L.sdiv));
    lds_copy(L.hdiv, st->hdiv, sizeof(L.hdiv));
    lds_copy(L.pt.csa, pt->csa, sizeof(L.pt.csa));
    lds_copy(L.pt.hmask, pt->hmask, sizeof(L.pt.hmask));
    lds_copy(L.pt.hsel, pt->hsel, sizeof(L.pt.hsel));
    lds_copy(L.pt.hfr, pt->hfr, sizeof(L.pt.hfr));
    lds_copy(L.pt.s_f, pt->s_f, sizeof(L.pt.s_f));
    lds_copy(L.pt.v_f, pt->v_f, sizeof(L.pt.v_f));
    const bool on = pt->enabled != 0, radical = pt->radical != 0; // uniform
    __syncthreads();
    const int f0 = bz * FPT;
    const int nf = min(FPT, batch - f0);
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63);
    if (dx >= dw) return;
    // a tap as b | g << 8 | r << 16 (the low three bytes of v) through the profile
    auto conv = [&](u32 v) -> u32 { return on ? d_profile_px(L, (int)(v & 255u), (int)((v >> 8) & 255u), (int)((v >> 16) & 255u), radical) : (v & 0xFFFFFFu); };
    for (int dy = blockIdx.y * WP_ROWS + (threadIdx.x >> 6), r = 0; r < WP_ROWS / 4 && dy < dh; r++, dy += 4) {
        const WarpTaps t = warp_taps(dx, dy, g.w, g.h, M, dw, dh, bw0, rot180, dst_stride);
        const size_t tap = (size_t)t.sy * g.stride + (size_t)t.sx * 3; // (only dereferenced where the taps are inside)
        // interior: one unaligned 8-byte load per row of taps, as warp_body (>= 8 bytes of slack behind the last frame)
        u64 ta[FPT], tb[FPT];
        if (t.interior)
#pragma unroll
            for (int k = 0; k < FPT; k++)
                if (k < nf) {
                    const u8* p00 = src + (size_t)(f0 + k) * g.frame_stride + tap;
                    __builtin_memcpy(&ta[k], p00, 8);
                    __builtin_memcpy(&tb[k], p00 + g.stride, 8);
                }
#pragma unroll
        for (int k = 0; k < FPT; k++) {
            if (k >= nf) break;
            int o[3] = {0, 0, 0};
            if (t.any_in) {
                u32 q[4] = {0u, 0u, 0u, 0u}; // taps 00, 01, 10, 11; border taps are 0
                if (t.interior) {
                    q[0] = conv((u32)ta[k]);
                    q[1] = conv((u32)(ta[k] >> 24));
                    q[2] = conv((u32)tb[k]);
                    q[3] = conv((u32)(tb[k] >> 24));
                } else {
                    const u8* p00 = src + (size_t)(f0 + k) * g.frame_stride + tap;
                    const u8* p10 = p00 + g.stride;
                    auto px = [&](const u8* p) -> u32 { return conv((u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16)); };
                    if (t.x0in && t.y0in) q[0] = px(p00);
                    if (t.x1in && t.y0in) q[1] = px(p00 + 3);
                    if (t.x0in && t.y1in) q[2] = px(p10);
                    if (t.x1in && t.y1in) q[3] = px(p10 + 3);
                }
#pragma unroll
                for (int c = 0; c < 3; c++)
                    o[c] = warp_blend((int)((q[0] >> (8 * c)) & 255), (int)((q[1] >> (8 * c)) & 255), (int)((q[2] >> (8 * c)) & 255),
                                      (int)((q[3] >> (8 * c)) & 255), t);
            }
            u8* out = dst + (size_t)(f0 + k) * dst_frame_stride + t.out_off;
            out[0] = (u8)o[0];
            out[1] = (u8)o[1];
            out[2] = (u8)o[2];
        }
    }
}

// blockIdx.z = profile * nz + group of frames; profile p writes its frames dst_profile_stride bytes behind profile p - 1's
template <int FPT>
__global__ __launch_bounds__(256) void k_warp_profile(const u8* __restrict__ src, Geom g, WarpM M, int dw, int dh, int bw0, int rot180,
                                                       u8* __restrict__ dst, int dst_stride, size_t dst_frame_stride, size_t dst_profile_stride,
                                                       const StaticTabs* __restrict__ st, const ProfileTabs* __restrict__ ptabs, int nz,
                                                       u32* __restrict__ zero_word, u32* __restrict__ zero_word2, int batch)
{
    const int pi = blockIdx.z / nz;
    warp_profile_body<FPT>(src, g, M.m, dw, dh, bw0, rot180, dst + (size_t)pi * dst_profile_stride, dst_stride, dst_frame_stride, st, ptabs + pi,
                           zero_word, zero_word2, batch, blockIdx.z - pi * nz);
}

// every board of a pipeline in one launch, as k_warp_mb; the profile is the pipeline's: one table
template <int FPT>
__global__ __launch_bounds__(256) void k_warp_profile_mb(const u8* __restrict__ src, Geom g, const BoardDev* __restrict__ tab, int nz, int s0,
                                                          const StaticTabs* __restrict__ st, const ProfileTabs* __restrict__ pt,
                                                          u32* __restrict__ zero_word, u32* __restrict__ zero_word2, int batch)
{
    const int b = blockIdx.z / nz;
    const BoardDev& T = tab[b];
    if (b > 0 && ((int)blockIdx.x * 64 >= T.S || (int)blockIdx.y * WP_ROWS >= T.S)) return;
    warp_profile_body<FPT>(src, g, T.Minv, T.S, T.S, T.bw0, T.rot180, T.warped + (size_t)s0 * T.warped_stride, T.S * 3, T.warped_stride, st, pt,
                           zero_word, zero_word2, batch, blockIdx.z - b * nz);
}

template <int FPT, bool CALC>
__global__ __launch_bounds__(256) void k_warp(const u8* __restrict__ src, Geom g, WarpM M, int dw, int dh, int bw0,
                                               int bh0, int rot180, u8* __restrict__ dst, int dst_stride,
                                               size_t dst_frame_stride, const u8* __restrict__ norm_lut, const u32* __restrict__ minmax,
                                               size_t mm_stride, u32* __restrict__ zero_word, u32* __restrict__ zero_word2, int batch)
{
    warp_body<FPT, CALC>(src, g, M.m, dw, dh, bw0, bh0, rot180, dst, dst_stride, dst_frame_stride, norm_lut, minmax, mm_stride,
                         zero_word, zero_word2, batch, blockIdx.z);
}

// every board of a pipeline in one launch: blockIdx.z = board * nz + group of frames; the grid covers the largest board
// and the blocks outside a smaller one leave at once (the shared frames' byte map is the same for every board)
template <int FPT, bool CALC>
__global__ __launch_bounds__(256) void k_warp_mb(const u8* __restrict__ src, Geom g, const BoardDev* __restrict__ tab, int nz, int s0,
                                                  const u8* __restrict__ norm_lut, const u32* __restrict__ minmax, size_t mm_stride,
                                                  u32* __restrict__ zero_word, u32* __restrict__ zero_word2, int batch)
{
    const int b = blockIdx.z / nz;
    const BoardDev& T = tab[b];
    if (b > 0 && ((int)blockIdx.x * 64 >= T.S || (int)blockIdx.y * 4 >= T.S)) return;
    warp_body<FPT, CALC>(src, g, T.Minv, T.S, T.S, T.bw0, T.bh0, T.rot180, T.warped + (size_t)s0 * T.warped_stride, T.S * 3,
                         T.warped_stride, norm_lut, minmax, mm_stride, zero_word, zero_word2, batch, blockIdx.z - b * nz);
}

int launch_warp_mb(cbv_ctx* ctx, const u8* src, Geom g, const BoardDev* tab, int nb, int maxS, int s0, NormSrc norm, int batch,
                   u32* zero_word, u32* zero_word2)
{
    prof_begin(ctx, CBV_K_WARP);
    const int fpt = batch >= 8 ? 4 : 1, nz = (batch + fpt - 1) / fpt;
    dim3 grid((maxS + 63) / 64, (maxS + 3) / 4, nz * nb);
    if (fpt == 4) {
        if (norm.minmax)
            hipLaunchKernelGGL((k_warp_mb<4, true>), grid, dim3(256), 0, ctx->stream, src, g, tab, nz, s0, nullptr, norm.minmax, norm.mm_stride,
                               zero_word, zero_word2, batch);
        else
            hipLaunchKernelGGL((k_warp_mb<4, false>), grid, dim3(256), 0, ctx->stream, src, g, tab, nz, s0, norm.lut, nullptr, 0, zero_word,
                               zero_word2, batch);
    } else {
        if (norm.minmax)
            hipLaunchKernelGGL((k_warp_mb<1, true>), grid, dim3(256), 0, ctx->stream, src, g, tab, nz, s0, nullptr, norm.minmax, norm.mm_stride,
                               zero_word, zero_word2, batch);
        else
            hipLaunchKernelGGL((k_warp_mb<1, false>), grid, dim3(256), 0, ctx->stream, src, g, tab, nz, s0, norm.lut, nullptr, 0, zero_word,
                               zero_word2, batch);
    }
    prof_end(ctx, CBV_K_WARP);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

int launch_warp(cbv_ctx* ctx, const u8* src, Geom g, const double* Minv9, int dw, int dh, int rot180, u8* dst,
                int dst_stride, size_t dst_frame_stride, NormSrc norm, int batch, u32* zero_word, u32* zero_word2)
{
    WarpM M;
    for (int i = 0; i < 9; i++) M.m[i] = Minv9[i];
    int bw0, bh0;
    warp_block_shape(dw, dh, &bw0, &bh0);
    prof_begin(ctx, CBV_K_WARP);
    // batched launches: four frames per thread (eight: 13 % fewer instructions again, no change on the path); a launch of
    // a frame or two keeps one thread per pixel and frame
    if (batch >= 8) {
        dim3 grid((dw + 63) / 64, (dh + 3) / 4, (batch + 3) / 4);
        if (norm.minmax)
            hipLaunchKernelGGL((k_warp<4, true>), grid, dim3(256), 0, ctx->stream, src, g, M, dw, dh, bw0, bh0, rot180, dst, dst_stride,
                               dst_frame_stride, nullptr, norm.minmax, norm.mm_stride, zero_word, zero_word2, batch);
        else
            hipLaunchKernelGGL((k_warp<4, false>), grid, dim3(256), 0, ctx->stream, src, g, M, dw, dh, bw0, bh0, rot180, dst, dst_stride,
                               dst_frame_stride, norm.lut, nullptr, 0, zero_word, zero_word2, batch);
    } else {
        dim3 grid((dw + 63) / 64, (dh + 3) / 4, batch);
        if (norm.minmax)
            hipLaunchKernelGGL((k_warp<1, true>), grid, dim3(256), 0, ctx->stream, src, g, M, dw, dh, bw0, bh0, rot180, dst, dst_stride,
                               dst_frame_stride, nullptr, norm.minmax, norm.mm_stride, zero_word, zero_word2, batch);
        else
            hipLaunchKernelGGL((k_warp<1, false>), grid, dim3(256), 0, ctx->stream, src, g, M, dw, dh, bw0, bh0, rot180, dst, dst_stride,
                               dst_frame_stride, norm.lut, nullptr, 0, zero_word, zero_word2, batch);
    }
    prof_end(ctx, CBV_K_WARP);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

// as launch_warp (four frames per thread in batched launches), for `np` profiles at once: ptabs[np] on the device
int launch_warp_profile(cbv_ctx* ctx, const u8* src, Geom g, const double* Minv9, int dw, int dh, int rot180, u8* dst, int dst_stride,
                        size_t dst_frame_stride, size_t dst_profile_stride, const ProfileTabs* ptabs, int np, int batch, u32* zero_word,
                        u32* zero_word2)
{
    WarpM M;
    for (int i = 0; i < 9; i++) M.m[i] = Minv9[i];
    int bw0, bh0;
    warp_block_shape(dw, dh, &bw0, &bh0);
    const int fpt = batch >= 8 ? 4 : 1, nz = (batch + fpt - 1) / fpt;
    if (np <= 0 || batch <= 0 || (long long)np * nz > 65535) return cbv_fail(ctx, CBV_ERR_ARG, "launch_warp_profile: %d profiles x %d frames do not fit a launch", np, batch);
    const dim3 grid((dw + 63) / 64, (dh + WP_ROWS - 1) / WP_ROWS, np * nz);
    prof_begin(ctx, CBV_K_WARP);
    if (fpt == 4)
        hipLaunchKernelGGL((k_warp_profile<4>), grid, dim3(256), 0, ctx->stream, src, g, M, dw, dh, bw0, rot180, dst, dst_stride, dst_frame_stride,
                           dst_profile_stride, ctx->tabs, ptabs, nz, zero_word, zero_word2, batch);
    else
        hipLaunchKernelGGL((k_warp_profile<1>), grid, dim3(256), 0, ctx->stream, src, g, M, dw, dh, bw0, rot180, dst, dst_stride, dst_frame_stride,
                           dst_profile_stride, ctx->tabs, ptabs, nz, zero_word, zero_word2, batch);
    prof_end(ctx, CBV_K_WARP);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

int launch_warp_profile_mb(cbv_ctx* ctx, const u8* src, Geom g, const BoardDev* tab, int nb, int maxS, int s0, const ProfileTabs* pt, int batch,
                           u32* zero_word, u32* zero_word2)
{
    const int fpt = batch >= 8 ? 4 : 1, nz = (batch + fpt - 1) / fpt;
    const dim3 grid((maxS + 63) / 64, (maxS + WP_ROWS - 1) / WP_ROWS, nz * nb);
    prof_begin(ctx, CBV_K_WARP);
    if (fpt == 4)
        hipLaunchKernelGGL((k_warp_profile_mb<4>), grid, dim3(256), 0, ctx->stream, src, g, tab, nz, s0, ctx->tabs, pt, zero_word, zero_word2, batch);
    else
        hipLaunchKernelGGL((k_warp_profile_mb<1>), grid, dim3(256), 0, ctx->stream, src, g, tab, nz, s0, ctx->tabs, pt, zero_word, zero_word2, batch);
    prof_end(ctx, CBV_K_WARP);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

// the raw planes a fused warp may read: what launch_ingest asks of them (YV12 leaves as YUV420P)
static int check_warp_yuv(cbv_ctx* ctx, RawPlanes* pl, RawGeom* r, Geom g, int batch)
{
    RC(check_raw_format(ctx, r->fmt, g.w, g.h, "launch_warp_yuv"));
    if (batch <= 0) return cbv_fail(ctx, CBV_ERR_ARG, "launch_warp_yuv: bad planes or strides");
    const int strides[3] = {r->stride0, r->stride1, r->stride2};
    RC(check_raw_planes(ctx, r->fmt, g.w, pl->p, strides, "launch_warp_yuv"));
    raw_planes_canonical(pl, r);
    return CBV_OK;
}

// one case per layout the kernels have a form for, both frames-per-thread counts each
#define CBV_WARP_YUV_FORMATS(LAUNCH)                   \
    switch (r.fmt) {                                   \
    case CBV_FMT_NV12: LAUNCH(CBV_FMT_NV12); break;    \
    case CBV_FMT_NV21: LAUNCH(CBV_FMT_NV21); break;    \
    case CBV_FMT_YUYV: LAUNCH(CBV_FMT_YUYV); break;    \
    case CBV_FMT_YVYU: LAUNCH(CBV_FMT_YVYU); break;    \
    case CBV_FMT_UYVY: LAUNCH(CBV_FMT_UYVY); break;    \
    default: LAUNCH(CBV_FMT_YUV420P);                  \
    }

// as launch_warp: four frames per thread in batched launches, one thread per pixel and frame in a launch of a frame or two
int launch_warp_yuv(cbv_ctx* ctx, RawPlanes pl, RawGeom r, Geom g, const double* Minv9, int dw, int dh, int rot180, u8* dst, int dst_stride,
                    size_t dst_frame_stride, int batch, u32* zero_word, u32* zero_word2)
{
    RC(check_warp_yuv(ctx, &pl, &r, g, batch));
    WarpM M;
    for (int i = 0; i < 9; i++) M.m[i] = Minv9[i];
    int bw0, bh0;
    warp_block_shape(dw, dh, &bw0, &bh0);
    const int fpt = batch >= 8 ? 4 : 1;
    const dim3 grid((dw + 63) / 64, (dh + 3) / 4, (batch + fpt - 1) / fpt);
    prof_begin(ctx, CBV_K_WARP_YUV);
#define CBV_WARP_YUV_K(FMT, FPT)                                                                                                          \
    hipLaunchKernelGGL((k_warp_yuv<FMT, FPT>), grid, dim3(256), 0, ctx->stream, pl.p[0], pl.p[1], pl.p[2], r, g.w, g.h, M, dw, dh, bw0, rot180, \
                       dst, dst_stride, dst_frame_stride, zero_word, zero_word2, batch)
#define CBV_WARP_YUV(FMT)             \
    if (fpt == 4) CBV_WARP_YUV_K(FMT, 4); \
    else CBV_WARP_YUV_K(FMT, 1)
    CBV_WARP_YUV_FORMATS(CBV_WARP_YUV)
#undef CBV_WARP_YUV
#undef CBV_WARP_YUV_K
    prof_end(ctx, CBV_K_WARP_YUV);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

int launch_warp_yuv_mb(cbv_ctx* ctx, RawPlanes pl, RawGeom r, Geom g, const BoardDev* tab, int nb, int maxS, int s0, int batch, u32* zero_word,
                       u32* zero_word2)
{
    RC(check_warp_yuv(ctx, &pl, &r, g, batch));
    const int fpt = batch >= 8 ? 4 : 1, nz = (batch + fpt - 1) / fpt;
    const dim3 grid((maxS + 63) / 64, (maxS + 3) / 4, nz * nb);
    prof_begin(ctx, CBV_K_WARP_YUV);
#define CBV_WARP_YUV_MB_K(FMT, FPT)                                                                                                        \
    hipLaunchKernelGGL((k_warp_yuv_mb<FMT, FPT>), grid, dim3(256), 0, ctx->stream, pl.p[0], pl.p[1], pl.p[2], r, g.w, g.h, tab, nz, s0, zero_word, \
                       zero_word2, batch)
#define CBV_WARP_YUV_MB(FMT)             \
    if (fpt == 4) CBV_WARP_YUV_MB_K(FMT, 4); \
    else CBV_WARP_YUV_MB_K(FMT, 1)
    CBV_WARP_YUV_FORMATS(CBV_WARP_YUV_MB)
#undef CBV_WARP_YUV_MB
#undef CBV_WARP_YUV_MB_K
    prof_end(ctx, CBV_K_WARP_YUV);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

// the mosaics a fused warp may read: what launch_ingest asks of them
static int check_warp_bayer(cbv_ctx* ctx, const RawPlanes& pl, const RawGeom& r, Geom g, int batch)
{
    RC(check_raw_format(ctx, r.fmt, g.w, g.h, "launch_warp_bayer"));
    if (!raw_fmt_bayer(r.fmt)) return cbv_fail(ctx, CBV_ERR_ARG, "launch_warp_bayer: format %d is not a Bayer format", r.fmt);
    if (batch <= 0) return cbv_fail(ctx, CBV_ERR_ARG, "launch_warp_bayer: bad planes or strides");
    const int strides[3] = {r.stride0, r.stride1, r.stride2};
    return check_raw_planes(ctx, r.fmt, g.w, pl.p, strides, "launch_warp_bayer");
}

#define CBV_WARP_BAYER_FORMATS(LAUNCH)                                 \
    switch (r.fmt) {                                                   \
    case CBV_FMT_BAYER_RGGB: LAUNCH(CBV_FMT_BAYER_RGGB); break;        \
    case CBV_FMT_BAYER_BGGR: LAUNCH(CBV_FMT_BAYER_BGGR); break;        \
    case CBV_FMT_BAYER_GRBG: LAUNCH(CBV_FMT_BAYER_GRBG); break;        \
    default: LAUNCH(CBV_FMT_BAYER_GBRG);                               \
    }

// as launch_warp_yuv: four frames per thread in batched launches, one thread per pixel and frame in a launch of a frame or two
int launch_warp_bayer(cbv_ctx* ctx, RawPlanes pl, RawGeom r, Geom g, const double* Minv9, int dw, int dh, int rot180, u8* dst, int dst_stride,
                      size_t dst_frame_stride, int batch, u32* zero_word, u32* zero_word2)
{
    RC(check_warp_bayer(ctx, pl, r, g, batch));
    WarpM M;
    for (int i = 0; i < 9; i++) M.m[i] = Minv9[i];
    int bw0, bh0;
    warp_block_shape(dw, dh, &bw0, &bh0);
    const int fpt = batch >= 8 ? 4 : 1;
    const dim3 grid((dw + 63) / 64, (dh + 3) / 4, (batch + fpt - 1) / fpt);
    prof_begin(ctx, CBV_K_WARP_YUV);
#define CBV_WARP_BAYER_K(FMT, FPT)                                                                                                      \
    hipLaunchKernelGGL((k_warp_bayer<FMT, FPT>), grid, dim3(256), 0, ctx->stream, pl.p[0], r, g.w, g.h, M, dw, dh, bw0, rot180, dst, dst_stride, \
                       dst_frame_stride, zero_word, zero_word2, batch)
#define CBV_WARP_BAYER(FMT)                 \
    if (fpt == 4) CBV_WARP_BAYER_K(FMT, 4); \
    else CBV_WARP_BAYER_K(FMT, 1)
    CBV_WARP_BAYER_FORMATS(CBV_WARP_BAYER)
#undef CBV_WARP_BAYER
#undef CBV_WARP_BAYER_K
    prof_end(ctx, CBV_K_WARP_YUV);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

int launch_warp_bayer_mb(cbv_ctx* ctx, RawPlanes pl, RawGeom r, Geom g, const BoardDev* tab, int nb, int maxS, int s0, int batch, u32* zero_word,
                         u32* zero_word2)
{
    RC(check_warp_bayer(ctx, pl, r, g, batch));
    const int fpt = batch >= 8 ? 4 : 1, nz = (batch + fpt - 1) / fpt;
    const dim3 grid((maxS + 63) / 64, (maxS + 3) / 4, nz * nb);
    prof_begin(ctx, CBV_K_WARP_YUV);
#define CBV_WARP_BAYER_MB_K(FMT, FPT)                                                                                                  \
    hipLaunchKernelGGL((k_warp_bayer_mb<FMT, FPT>), grid, dim3(256), 0, ctx->stream, pl.p[0], r, g.w, g.h, tab, nz, s0, zero_word, zero_word2, batch)
#define CBV_WARP_BAYER_MB(FMT)                 \
    if (fpt == 4) CBV_WARP_BAYER_MB_K(FMT, 4); \
    else CBV_WARP_BAYER_MB_K(FMT, 1)
    CBV_WARP_BAYER_FORMATS(CBV_WARP_BAYER_MB)
#undef CBV_WARP_BAYER_MB
#undef CBV_WARP_BAYER_MB_K
    prof_end(ctx, CBV_K_WARP_YUV);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

// ---------------------------------------------------------------------------
// synthetic frames; mirrors oracle orc_synth_frame bit for bit
// ---------------------------------------------------------------------------
__device__ __forceinline__ u64 d_mix64(u64 z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void k_synth(u8* __restrict__ dst, Geom g, const u64* __restrict__ seeds,
                                                const double* __restrict__ Hinv, const u8* __restrict__ boards,
                                                const cbv_scene* __restrict__ scp)
{
    __shared__ u8 board[64];
    __shared__ cbv_scene sc;
    if (threadIdx.x < 64) board[threadIdx.x] = boards[(size_t)blockIdx.z * 64 + threadIdx.x];
    if (threadIdx.x == 0) sc = *scp;
    __syncthreads();
    const u64 seed = seeds[blockIdx.z];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= g.w || y >= g.h) return;
    const u64 idx = (u64)y * (u64)g.w + (u64)x;
    const u64 hn = d_mix64(seed + idx * 0x9E3779B97F4A7C15ULL);
    const u64 hb = d_mix64(0x5851F42D4C957F2DULL + (u64)(y >> 4) * 4096 + (u64)(x >> 4));
    const int bgv = sc.bg_lo + (int)(hb % (u64)(sc.bg_span ? sc.bg_span : 1));
    int c0 = bgv, c1 = bgv, c2 = bgv;
    const double W = Hinv[6] * x + Hinv[7] * y + Hinv[8];
    const double u = (Hinv[0] * x + Hinv[1] * y + Hinv[2]) / W;
    const double v = (Hinv[3] * x + Hinv[4] * y + Hinv[5]) / W;
    if (u >= 0.0 && u < 8.0 && v >= 0.0 && v < 8.0) {
        const int fi = (int)u, ri = (int)v;
        const u8* c = ((fi + ri) & 1) ? sc.dark : sc.light;
        const int piece = board[ri * 8 + fi];
        if (piece) {
            const double du = u - (fi + 0.5), dv = v - (ri + 0.5);
            if (du * du + dv * dv <= sc.radius * sc.radius) c = piece == 1 ? sc.white : sc.black;
        }
        c0 = c[0];
        c1 = c[1];
        c2 = c[2];
    }
    const int span = 2 * sc.noise + 1;
    u8* q = dst + (size_t)blockIdx.z * g.frame_stride + (size_t)y * g.stride + (size_t)x * 3;
    q[0] = d_sat8(c0 + (int)((hn >> 0) & 0xFFFF) % span - sc.noise);
    q[1] = d_sat8(c1 + (int)((hn >> 16) & 0xFFFF) % span - sc.noise);
    q[2] = d_sat8(c2 + (int)((hn >> 32) & 0xFFFF) % span - sc.noise);
}

int launch_synth(cbv_ctx* ctx, u8* dst, Geom g, const u64* seeds_dev, const double* hinv_dev, const u8* boards_dev,
                 const cbv_scene* scene_dev, int batch)
{
    dim3 grid((g.w + 63) / 64, (g.h + 3) / 4, batch);
    prof_begin(ctx, CBV_K_SYNTH);
    hipLaunchKernelGGL(k_synth, grid, dim3(256), 0, ctx->stream, dst, g, seeds_dev, hinv_dev, boards_dev, scene_dev);
    prof_end(ctx, CBV_K_SYNTH);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}
