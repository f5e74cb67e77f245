// The warp, for the translation units that hold its kernels (k_warp.hip, k_warp_raw_profile.hip, k_warp_jpeg.hip, k_warp_cs.hip
// and, through warp_lens.h, k_warp_lens.hip, k_warp_lens_profile.hip, k_warp_lens_cs.hip): the sources, the one gather
// (warp_gather), the kernel templates k_warp_one and k_warp_boards (k_warp_lens: warp_lens.h), the frames per thread of every
// source's many-frames form (warp_many), the dispatch from a WarpSrc to the typed source (warp_typed_*) and the launch
// templates.  A unit is its exported launchers: dispatch the source, call the launch template.  Private.
#pragma once
#include "cbv_bayer_deep.h"
#include "cbv_profile_px.h"
#include "cbv_yuv.h"
#include "jpeg_core.h"
#include "lens_core.h"

struct WarpM {
    double m[9];
};

// What a destination pixel samples, whatever the format of the frames: the top-left tap, the four weights, which taps are
// inside the source, and where the pixel goes.
struct WarpTaps {
    int sx, sy;
    int w00, w01, w10, w11;
    bool any_in, x0in, x1in, y0in, y1in, interior;
    size_t out_off; // byte offset of the pixel inside a destination frame
};

// destination pixel (dx, dy) of a dw x dh destination; sw x sh = the source frame.  LENS: the ideal position goes through
// the camera's lens model (lens_core.h, *lens) before it is quantised: one more step in the coordinate, the same taps after it
template <bool LENS = false>
__device__ __forceinline__ WarpTaps warp_taps(int dx, int dy, int sw, int sh, const double* __restrict__ M, int dw, int dh, int bw0, int rot180,
                                              int dst_stride, const LensDev* lens = nullptr)
{
    WarpTaps t;
    const int bx = (dx / bw0) * bw0, x1 = dx - bx; // block origin and offset inside it
    // (rows are evaluated independently of the block row)
    double fX, fY;
    if constexpr (LENS) lens_warp_xy32(*lens, M, bx, x1, dy, &fX, &fY);
    else {
        const double X0 = M[0] * bx + M[1] * dy + M[2];
        const double Y0 = M[3] * bx + M[4] * dy + M[5];
        const double W0 = M[6] * bx + M[7] * dy + M[8];
        double W = W0 + M[6] * x1;
        W = W != 0. ? 32. / W : 0.;
        fX = (X0 + M[0] * x1) * W;
        fY = (Y0 + M[3] * x1) * W;
        fX = fmax(-2147483648.0, fmin(2147483647.0, fX));
        fY = fmax(-2147483648.0, fmin(2147483647.0, fY));
    }
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

// where a launch writes one board: the matrix, the dw x dh destination, frame 0 of the batch
struct WarpDst {
    const double* M;
    int dw, dh, bw0, rot180;
    u8* dst;
    int stride;
    size_t frame_stride;
};

// ---------------------------------------------------------------------------
// The sources: what the frames are and how the BGR value of a tap is obtained.  A source is plain data and constants; what
// it does differently stands in warp_gather under its KIND.  (The text stays in the one function on purpose: the compiler
// simplifies every function on its own before it inlines, and the gather split into per-source functions compiles to
// other instructions than this.)
// ---------------------------------------------------------------------------
enum { WARP_BGR, WARP_PROFILE, WARP_YUV, WARP_BAYER, WARP_JPEG, WARP_DEEP };
#define WP_ROWS 16 // destination rows per workgroup of WarpProfile: one row of WarpPerspectiveInvoker's 64 x 16 blocks

// BGR frames through cv2.normalize's byte map, which is staged in LDS per frame.  CALC: the map is worked out here from the
// frames' [min, max] words (NormSrc::minmax) instead of read from a table ([frame][256]); neither: no mapping.  The taps
// stay channel by channel, as bytes index the map.
template <bool CALC_>
struct WarpBgr {
    static constexpr int KIND = WARP_BGR, ROWS = 4, FMT = CBV_FMT_BGR;
    static constexpr bool CALC = CALC_, TABS = false, CS = false;
    template <int FPT>
    struct Lds {
        u8 lut[FPT][256];
    };
    const u8* src;
    Geom g;
    const u8* norm_lut;
    const u32* minmax;
    size_t mm_stride;
    __device__ __forceinline__ int w() const { return g.w; }
    __device__ __forceinline__ int h() const { return g.h; }
};

// BGR frames through the colour profile (cbv_warp_color_profile, pipelines configured with CBV_SKIP_ENHANCE_PROFILE,
// cbv_pipeline_color_sweep): the loads of WarpBgr, d_profile_px on each tap.  A workgroup stages the 7.5 KB d_profile_px
// reads (ProfileLds) and then covers WP_ROWS destination rows of its 64 columns, FPT frames each: 1920 staged words against
// 4096 conversions per frame.  The tables are an argument, one ProfileTabs per profile of the launch; a table with
// enabled = 0 leaves the taps as they are.
struct WarpProfile {
    static constexpr int KIND = WARP_PROFILE, ROWS = WP_ROWS, FMT = CBV_FMT_BGR;
    static constexpr bool TABS = true, CS = false;
    template <int FPT>
    using Lds = ProfileLds;
    const u8* src;
    Geom g;
    const StaticTabs* st;
    const ProfileTabs* pt; // the profile's table
    __device__ __forceinline__ int w() const { return g.w; }
    __device__ __forceinline__ int h() const { return g.h; }
};

// Camera-native frames (pipelines without enhancement whose input is raw): the BGR frame k_ingest would write is never made.
// YUV: the taps through d_yuv_bgr; the conversion is pointwise (a pixel takes the chroma of its 2x2 block or pair, nothing
// is interpolated).  Bayer: the taps demosaiced (d_bayer_bgr, cbv_bayer.h); a tap on the frame's outermost rows or
// columns is the result of the clamped site, as in k_ingest.  Nothing is staged.
template <int FMT_>
struct WarpRaw {
    static constexpr int KIND = raw_fmt_bayer(FMT_) ? WARP_BAYER : WARP_YUV, ROWS = 4, FMT = FMT_;
    static constexpr bool TABS = false, CS = false;
    template <int FPT>
    struct Lds {
    };
    const u8* p0;
    const u8* p1;
    const u8* p2;
    RawGeom r;
    int sw, sh;
    __device__ __forceinline__ int w() const { return sw; }
    __device__ __forceinline__ int h() const { return sh; }
};

// Camera-native frames through the colour profile (k_warp_raw_profile.hip: pipelines configured with
// CBV_SKIP_ENHANCE_PROFILE_RAW, their colour sweep, cbv_warp_color_profile_raw): the loads and the conversion of WarpRaw,
// then d_profile_px on each converted tap that lies inside the frame, staged and tiled as WarpProfile is.  Neither the BGR
// frame nor the profiled frame is ever made.
template <int FMT_>
struct WarpRawProfile : WarpRaw<FMT_> {
    static constexpr int ROWS = WP_ROWS;
    static constexpr bool TABS = true;
    template <int FPT>
    using Lds = ProfileLds;
    const StaticTabs* st;
    const ProfileTabs* pt; // the profile's table
};

// YUV frames in another colour space than 0 (include/cbv.h, CBV_CS_*; k_warp_cs.hip and k_warp_lens_cs.hip): the loads of
// WarpRaw, the taps converted with the six constants the source carries (cbv_yuv.h, YuvCs), which are uniform and stay in
// scalar registers.  CS tells the kernels to hand `cs` to warp_gather as its last argument (warp_gather_of).
template <int FMT_>
struct WarpRawCs : WarpRaw<FMT_> {
    static constexpr bool CS = true;
    YuvCs cs;
};
template <int FMT_>
struct WarpRawProfileCs : WarpRawProfile<FMT_> {
    static constexpr bool CS = true;
    YuvCs cs;
};

// Developed mosaics (include/cbv.h; k_warp_deep.hip, k_warp_lens_deep.hip: pipelines in raw mode whose input is a Bayer id with a
// sample encoding or with tables): the Bayer branch of the gather with the 4 x 4 bytes of a fast pixel, and the 3 x 3 of a tap
// by byte loads, made of developed samples (cbv_bayer_deep.h: unpack, then the site's colour's table) instead of loaded;
// everything behind them is shared, and the BGR frame k_ingest_deep would write is never made.  The layout's phase bits and the
// encoding are uniform values of the source, so there is one form for the four layouts and the four encodings.  LDS_: tables
// of up to 12 bits are staged per workgroup (12 KB); 14- and 16-bit tables are read from global memory through the cache.
#define WARP_DEEP_LDS_BITS 12
template <bool LDS_>
struct WarpDeep {
    static constexpr int KIND = WARP_DEEP, ROWS = 4, FMT = CBV_FMT_BAYER_RGGB;
    static constexpr bool TABS = false, CS = false, LDS = LDS_;
    template <int FPT>
    struct Lds {
        u8 deep[LDS_ ? (3 << WARP_DEEP_LDS_BITS) : 4];
    };
    const u8* p0;
    RawGeom r;
    int sw, sh;
    DeepDev d;
    __device__ __forceinline__ int w() const { return sw; }
    __device__ __forceinline__ int h() const { return sh; }
};
template <bool LDS_>
struct DeepProfileLds : ProfileLds {
    u8 deep[LDS_ ? (3 << WARP_DEEP_LDS_BITS) : 4];
};
// ... through the colour profile: d_profile_px on each developed, demosaiced tap inside the frame, staged and tiled as WarpProfile is
template <bool LDS_>
struct WarpDeepProfile : WarpDeep<LDS_> {
    static constexpr int ROWS = WP_ROWS;
    static constexpr bool TABS = true;
    template <int FPT>
    using Lds = DeepProfileLds<LDS_>;
    const StaticTabs* st;
    const ProfileTabs* pt; // the profile's table
};

// The decoded planes of Motion-JPEG frames (k_warp_jpeg.hip: pipelines in planes mode without enhancement, cbv_warp_jpeg): a
// tap at (x, y) is jpeg_pixel(D, planes, x, y) of the frame's own descriptor D, so the BGR frame k_jpeg_color would write is
// never made.  Frame f's planes lie at planes + f * plane_stride, its descriptor is descs[f]: gray, 4:4:4, 4:2:2 and 4:2:0
// frames may share a launch.
struct WarpJpeg {
    static constexpr int KIND = WARP_JPEG, ROWS = 4, FMT = CBV_FMT_MJPEG;
    static constexpr bool TABS = false, CS = false;
    template <int FPT>
    struct Lds {
    };
    const u8* planes;
    size_t plane_stride;
    const JpegDesc* descs;
    int sw, sh;
    __device__ __forceinline__ int w() const { return sw; }
    __device__ __forceinline__ int h() const { return sh; }
};

// ... through the colour profile: d_profile_px on each tap inside the frame, staged and tiled as WarpProfile is
struct WarpJpegProfile : WarpJpeg {
    static constexpr int ROWS = WP_ROWS;
    static constexpr bool TABS = true;
    template <int FPT>
    using Lds = ProfileLds;
    const StaticTabs* st;
    const ProfileTabs* pt; // the profile's table
};

// What the taps of one JPEG frame need of its descriptor, read once per thread and frame (the descriptor is the same for the
// whole workgroup): the planes' offsets and row lengths, the chroma planes' true size, and the sampling.  `wide`: the fast
// pixels of the frame take their chroma from 4-byte loads; not so where a subsampled component is 1 or 2 wide, which is
// replicated, not filtered (jpeg_chroma_at): those frames are at most 4 pixels wide and go through jpeg_pixel.
struct JpegTapDesc {
    u32 o0, o1, o2;
    int s0, s1, cw, ch;
    int mode; // 0 gray, 1 4:4:4, 2 4:2:2, 3 4:2:0
    bool wide;
};
__device__ __forceinline__ JpegTapDesc jpeg_tap_desc(const JpegDesc& D)
{
    JpegTapDesc J;
    J.o0 = D.poff[0];
    J.o1 = D.poff[1];
    J.o2 = D.poff[2];
    J.s0 = D.bw[0] * 8;
    J.s1 = D.bw[1] * 8;
    J.cw = D.cw[1];
    J.ch = D.ch[1];
    J.mode = D.ncomp == 1 ? 0 : D.hs == 1 ? 1 : D.vs == 1 ? 2 : 3;
    J.wide = J.mode < 2 || J.cw > 2;
    return J;
}
__device__ __forceinline__ int d_byte(u32 w, int i) { return (int)((w >> (8 * i)) & 255u); }
// what the wide loads of a fast pixel hold of one frame: the rows of luma taps and the rows of the chroma windows, which
// start at column ws (2:1 chroma) and row rs (4:2:0)
struct JpegWin {
    u32 ya, yb;
    u32 cb[3], cr[3];
    int ws, rs;
};
__device__ __forceinline__ u32 d_sel3(const u32 (&w)[3], int i) { return i == 0 ? w[0] : i == 1 ? w[1] : w[2]; }
// tap (sx + tx, sy + ty) of a fast pixel from the window: jpeg_pixel's arithmetic on the loaded bytes
__device__ __forceinline__ u32 d_jpeg_tap(const JpegTapDesc& J, const JpegWin& W, int sx, int sy, int tx, int ty)
{
    const int x = sx + tx, y = sy + ty;
    const int Y = d_byte(ty ? W.yb : W.ya, tx);
    if (J.mode == 0) return (u32)Y * 0x010101u;
    int cb, cr;
    if (J.mode == 1) {
        cb = d_byte(W.cb[ty], tx);
        cr = d_byte(W.cr[ty], tx);
    } else { // jpeg_chroma_at's filter
        const int ci = x >> 1, cn = (x & 1) ? min(ci + 1, J.cw - 1) : max(ci - 1, 0);
        const int ri = ci - W.ws, rn = cn - W.ws;
        if (J.mode == 2) {
            const int rnd = (x & 1) ? 2 : 1;
            cb = (3 * d_byte(W.cb[ty], ri) + d_byte(W.cb[ty], rn) + rnd) >> 2;
            cr = (3 * d_byte(W.cr[ty], ri) + d_byte(W.cr[ty], rn) + rnd) >> 2;
        } else {
            const int cj = y >> 1, cjn = (y & 1) ? min(cj + 1, J.ch - 1) : max(cj - 1, 0);
            const int a = cj - W.rs, b = cjn - W.rs, rnd = (x & 1) ? 7 : 8;
            const u32 b0 = d_sel3(W.cb, a), b1 = d_sel3(W.cb, b), r0 = d_sel3(W.cr, a), r1 = d_sel3(W.cr, b);
            cb = (3 * (3 * d_byte(b0, ri) + d_byte(b1, ri)) + (3 * d_byte(b0, rn) + d_byte(b1, rn)) + rnd) >> 4;
            cr = (3 * (3 * d_byte(r0, ri) + d_byte(r1, ri)) + (3 * d_byte(r0, rn) + d_byte(r1, rn)) + rnd) >> 4;
        }
    }
    u8 o[3];
    jpeg_ycc_to_bgr(Y, cb, cr, o);
    return (u32)o[0] | ((u32)o[1] << 8) | ((u32)o[2] << 16);
}
// pixel (x, y) of one JPEG frame with byte loads, as b | g << 8 | r << 16
__device__ __forceinline__ u32 d_jpeg_px(const JpegDesc& D, const u8* __restrict__ planes, int x, int y)
{
    u8 px[3];
    jpeg_pixel(D, planes, x, y, px);
    return (u32)px[0] | ((u32)px[1] << 8) | ((u32)px[2] << 16);
}

// pixel (x, y) of one raw YUV frame with byte loads (the taps of pixels on the frame's border)
// (K, here and below: nothing, or the YuvCs of a source in another colour space than 0, which every call of d_chroma and
// d_yuv_bgr then takes as its last argument: warp_gather)
template <int FMT, class... K>
__device__ __forceinline__ u32 d_raw_px(const u8* __restrict__ f0, const u8* __restrict__ f1, const u8* __restrict__ f2, const RawGeom& r, int x,
                                        int y, K... k)
{
    typedef YuvLay<FMT> L;
    if (L::PLANAR)
        return d_yuv_bgr(f0[(size_t)y * r.stride0 + x],
                         d_chroma(f1[(size_t)(y >> 1) * r.stride1 + (x >> 1)], f2[(size_t)(y >> 1) * r.stride2 + (x >> 1)], k...), k...);
    if (L::F420) {
        const u8* c = f1 + (size_t)(y >> 1) * r.stride1 + (x & ~1);
        return d_yuv_bgr(f0[(size_t)y * r.stride0 + x], d_chroma(c[L::CU], c[L::CV], k...), k...);
    }
    const u8* s = f0 + (size_t)y * r.stride0 + (size_t)(x >> 1) * 4;
    return d_yuv_bgr(s[L::Y0 + (x & 1) * 2], d_chroma(s[L::PU], s[L::PV], k...), k...);
}

// the chroma of byte pair `p` of an NV12 (U V) / NV21 (V U) row
template <int FMT, class... K>
__device__ __forceinline__ Chroma d_chroma_pair(u32 p, K... k)
{
    return d_chroma((p >> (8 * YuvLay<FMT>::CU)) & 255, (p >> (8 * YuvLay<FMT>::CV)) & 255, k...);
}

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

// pixel (x, y) of one developed mosaic, inside the frame, with byte loads: the site is clamped, its neighbourhood lies inside
__device__ __forceinline__ u32 d_deep_px(const u8* __restrict__ f0, int stride, int w, int h, const u8* __restrict__ tab, const DeepDev& d, int x, int y)
{
    const int cx = min(max(x, 1), w - 2), cy = min(max(y, 1), h - 2);
    u32 row[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const u8* q = f0 + (size_t)(cy + i - 1) * stride;
        row[i] = 0;
#pragma unroll
        for (int j = 0; j < 3; j++) row[i] |= d_deep_byte(tab, d, d_deep_sample(q, cx + j - 1, d.enc), cx + j - 1, cy + i - 1) << (8 * j);
    }
    return d_deep_bgr(d.ph, cx, cy, row[0], row[1], row[2]);
}

// The gather.  FPT frames per thread: the coordinates of a destination pixel depend on the matrix and the pixel, not on the
// frame, and they are most of the kernel's instructions (about 100 of 190 per output pixel, in double precision): a thread
// works them out once and samples FPT consecutive frames of the batch with them (bz = the group of FPT frames, blockIdx.z
// of a single-board launch; the last group of a batch may hold fewer).  A workgroup covers Src::ROWS rows of 64 columns.
// Per source: what is staged in LDS, which pixels fetch their taps with wide loads (`fast`) and what those loads are, the
// taps of a fast pixel, and a tap by byte loads for the pixels with taps outside the frame.  The rest is shared.
//
// The wide loads.  BGR and profile, interior pixels: the two taps of a row are 6 contiguous bytes -> ONE unaligned 8-byte
// load per row instead of six byte loads; the two bytes read past the second tap stay inside the buffer (callers keep >= 8
// bytes of slack behind the last frame).  YUV, interior pixels, per row of taps.  NV12 / NV21: one 2-byte load holds both
// luma samples and one 4-byte load at the even column holds the chroma of the first tap's pair and of the next pair, which
// is the second tap's when sx is odd (when sx is even both taps share the first); the rows share the chroma row when sy is
// even.  Planar chroma (YUV420P; YV12 arrives with p1 and p2 swapped): the same 2-byte luma load, and per chroma row one
// 2-byte load of U and one of V at column sx >> 1, which hold the first tap's sample and the next, the second tap's when sx
// is odd.  Packed 4:2:2: one 8-byte load at the first tap's pair, e.g. Y0 U Y1 V | Y2 U Y3 V, holds both taps and their
// chroma for either parity.  The bytes read past the second tap's pair (sx even) stay inside the buffer: the ring keeps 256
// bytes of slack behind the last frame.  Bayer, pixels whose four taps are all interior sites (1 <= sx, sx + 1 <= w - 2,
// the same in y): the taps' 3 x 3 neighbourhoods lie in the 4 x 4 bytes at (sx - 1, sy - 1), which is four unaligned 4-byte
// loads per frame, inside the frame's rows.  JPEG planes, interior pixels: one 2-byte load per row of taps holds both luma
// samples.  The chroma of a 2 x 2 block of taps and of the neighbours its triangle filter reads lies in 3 columns (4:2:2,
// 4:2:0; 2 for 4:4:4) of 3 rows (4:2:0; 2 otherwise) of each chroma plane: one 4-byte load per row and plane at the window's
// first column, which is the taps' column for 4:4:4 and max(((sx + 1) >> 1) - 1, 0) otherwise; the rows start at
// max(((sy + 1) >> 1) - 1, 0) for 4:2:0 and are clamped to the component's last row, which only moves rows no tap reads.  So
// 4 loads (gray: 2), 6 (4:4:4, 4:2:2) or 8 (4:2:0) per frame.  The planes are whole MCUs, and the bytes a load reads past
// the window belong to the next row, plane or slot: callers keep >= 4 readable bytes behind the last frame's planes.
//
// K: nothing, or the YuvCs of a YUV source in another colour space than 0 (WarpRawCs, WarpRawProfileCs: their `cs`).  `cs...`
// closes every call of the conversion, so colour space 0's calls are the ones with the compile-time constants, as they
// always were, and the others' take the launch's.
template <class Src, int FPT, bool LENS = false, class... K>
__device__ __forceinline__ void warp_gather(Src S, WarpDst D, u32* __restrict__ zero_word, u32* __restrict__ zero_word2, int batch, int bz,
                                            const LensDev* lens = nullptr, K... cs)
{
    constexpr int KIND = Src::KIND, FMT = Src::FMT;
    constexpr bool BGR = KIND == WARP_BGR, PROFILE = KIND == WARP_PROFILE, YUV = KIND == WARP_YUV, JPEG = KIND == WARP_JPEG, DEEP = KIND == WARP_DEEP;
    constexpr bool TABS = Src::TABS, RAW_TABS = TABS && !PROFILE; // the profile's tables are staged; ... for the taps of a raw source
    typedef YuvLay<YUV ? FMT : CBV_FMT_NV12> L; // (only read where YUV)
    constexpr bool NV12 = L::F420 && !L::PLANAR, PLANAR = L::PLANAR;
    __shared__ typename Src::template Lds<FPT> lds;
    warp_zero_words(zero_word, zero_word2);
    bool use_lut = false, on = false, radical = false; // uniform
    if constexpr (BGR) use_lut = Src::CALC || S.norm_lut != nullptr;
    const u8* __restrict__ deep_tab = nullptr; // DEEP: the tables the samples go through, staged or the device's
    if constexpr (DEEP) {
        if constexpr (Src::LDS) {
            lds_copy(lds.deep, S.d.tab, 3 << S.d.bits);
            deep_tab = lds.deep;
            if constexpr (!TABS) __syncthreads(); // (with a profile: behind its tables, below)
        } else deep_tab = S.d.tab;
    }
    if constexpr (TABS) {
        lds_copy(lds.sdiv, S.st->sdiv, sizeof(lds.sdiv));
        lds_copy(lds.hdiv, S.st->hdiv, sizeof(lds.hdiv));
        lds_copy(lds.pt.csa, S.pt->csa, sizeof(lds.pt.csa));
        lds_copy(lds.pt.hmask, S.pt->hmask, sizeof(lds.pt.hmask));
        lds_copy(lds.pt.hsel, S.pt->hsel, sizeof(lds.pt.hsel));
        lds_copy(lds.pt.hfr, S.pt->hfr, sizeof(lds.pt.hfr));
        lds_copy(lds.pt.s_f, S.pt->s_f, sizeof(lds.pt.s_f));
        lds_copy(lds.pt.v_f, S.pt->v_f, sizeof(lds.pt.v_f));
        on = S.pt->enabled != 0;
        radical = S.pt->radical != 0;
        __syncthreads();
    }
    const int f0 = bz * FPT;
    const int nf = min(FPT, batch - f0);
    if constexpr (BGR) {
        if (Src::CALC) {
#pragma unroll
            for (int k = 0; k < FPT; k++)
                if (k < nf) {
                    const u32* mm = S.minmax + (size_t)(f0 + k) * S.mm_stride;
                    lds.lut[k][threadIdx.x] = d_norm_lut_entry((int)mm[0], (int)mm[1], (int)threadIdx.x);
                }
        } else if (use_lut)
#pragma unroll
            for (int k = 0; k < FPT; k++)
                if (k < nf) lds.lut[k][threadIdx.x] = S.norm_lut[(size_t)(f0 + k) * 256 + threadIdx.x];
        __syncthreads();
    }
    // a tap as b | g << 8 | r << 16 (the low three bytes of v) through the profile
    auto conv = [&](u32 v) -> u32 {
        if constexpr (TABS) return on ? d_profile_px(lds, (int)(v & 255u), (int)((v >> 8) & 255u), (int)((v >> 16) & 255u), radical) : (v & 0xFFFFFFu);
        else return v;
    };
    JpegTapDesc jt[JPEG ? FPT : 1]; // JPEG: per frame, outside the loops over rows and taps
    if constexpr (JPEG)
#pragma unroll
        for (int k = 0; k < FPT; k++)
            if (k < nf) jt[k] = jpeg_tap_desc(S.descs[f0 + k]);
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63);
    int dy = blockIdx.y * Src::ROWS + (threadIdx.x >> 6), row = 0;
    if (dx >= D.dw || dy >= D.dh) return;
    do {
        const WarpTaps t = warp_taps<LENS>(dx, dy, S.w(), S.h(), D.M, D.dw, D.dh, D.bw0, D.rot180, D.stride, lens);
        // ---- the offsets of the loads (only used where the taps are inside) and the wide loads of every frame, which are
        // all issued before the first is used: the gather is bound by the number of memory instructions, not by bytes
        bool fast = t.interior;
        size_t tap = 0, c_off = 0, c2_off = 0; // tap: of tap 00 (YUV: its luma, or its pair; Bayer: of the 4 x 4 bytes)
        bool odd = false, two_crows = false;   // YUV; two_crows: the rows of taps lie in different chroma rows
        if constexpr (BGR || PROFILE) tap = (size_t)t.sy * S.g.stride + (size_t)t.sx * 3;
        else if constexpr (YUV) {
            odd = t.sx & 1;
            two_crows = L::F420 && (t.sy & 1);
            tap = L::F420 ? (size_t)t.sy * S.r.stride0 + (size_t)t.sx : (size_t)t.sy * S.r.stride0 + (size_t)(t.sx >> 1) * 4;
            c_off = (size_t)(t.sy >> 1) * S.r.stride1 + (size_t)(PLANAR ? t.sx >> 1 : t.sx & ~1);
            c2_off = (size_t)(t.sy >> 1) * S.r.stride2 + (size_t)(t.sx >> 1);
        } else if constexpr (JPEG) {
            // (the offsets depend on the frame's layout: worked out per frame below)
        } else if constexpr (DEEP) {
            fast = t.sx >= 1 && t.sx + 2 < S.sw && t.sy >= 1 && t.sy + 2 < S.sh;
            tap = (size_t)(t.sy - 1) * S.r.stride0; // of the first of the four rows; the column depends on the encoding
        } else {
            fast = t.sx >= 1 && t.sx + 2 < S.sw && t.sy >= 1 && t.sy + 2 < S.sh;
            tap = (size_t)(t.sy - 1) * S.r.stride0 + (size_t)(t.sx - 1);
        }
        u64 ta[FPT], tb[FPT]; // the rows of taps.  BGR, profile: 8 bytes; YUV 4:2:0: 2 luma bytes; 4:2:2: the 8 bytes of two pairs
        u32 ca[FPT], cb[FPT]; // NV12: U V U V; planar: U U
        u32 va[FPT], vb[FPT]; // planar: V V
        u32 rows[FPT][4];     // Bayer
        u32 jcb[FPT][3], jcr[FPT][3]; // JPEG: the chroma windows' rows
        // JPEG: the first column and row of the chroma windows of a frame with 2:1 chroma (the same for 4:2:2 and 4:2:0)
        const int jws = max(((t.sx + 1) >> 1) - 1, 0), jrs = max(((t.sy + 1) >> 1) - 1, 0);
        if (fast)
#pragma unroll
            for (int k = 0; k < FPT; k++)
                if (k < nf) {
                    if constexpr (BGR || PROFILE) {
                        const u8* p00 = S.src + (size_t)(f0 + k) * S.g.frame_stride + tap;
                        __builtin_memcpy(&ta[k], p00, 8);
                        __builtin_memcpy(&tb[k], p00 + S.g.stride, 8);
                    } else if constexpr (YUV) {
                        const u8* l = S.p0 + (size_t)(f0 + k) * S.r.frame_stride + tap;
                        if (L::F420) {
                            u16 a, b;
                            __builtin_memcpy(&a, l, 2);
                            __builtin_memcpy(&b, l + S.r.stride0, 2);
                            ta[k] = a;
                            tb[k] = b;
                            const u8* c = S.p1 + (size_t)(f0 + k) * S.r.frame_stride + c_off;
                            if (NV12) {
                                __builtin_memcpy(&ca[k], c, 4);
                                cb[k] = ca[k];
                                if (two_crows) __builtin_memcpy(&cb[k], c + S.r.stride1, 4);
                            } else {
                                const u8* c2 = S.p2 + (size_t)(f0 + k) * S.r.frame_stride + c2_off;
                                u16 u, v;
                                __builtin_memcpy(&u, c, 2);
                                __builtin_memcpy(&v, c2, 2);
                                ca[k] = cb[k] = u;
                                va[k] = vb[k] = v;
                                if (two_crows) {
                                    __builtin_memcpy(&u, c + S.r.stride1, 2);
                                    __builtin_memcpy(&v, c2 + S.r.stride2, 2);
                                    cb[k] = u;
                                    vb[k] = v;
                                }
                            }
                        } else {
                            __builtin_memcpy(&ta[k], l, 8);
                            __builtin_memcpy(&tb[k], l + S.r.stride0, 8);
                        }
                    } else if constexpr (JPEG) {
                        const JpegTapDesc& J = jt[k];
                        if (J.wide) {
                            const u8* pl = S.planes + (size_t)(f0 + k) * S.plane_stride;
                            const u8* l = pl + J.o0 + (size_t)t.sy * J.s0 + t.sx;
                            u16 a, b;
                            __builtin_memcpy(&a, l, 2);
                            __builtin_memcpy(&b, l + J.s0, 2);
                            ta[k] = a;
                            tb[k] = b;
                            if (J.mode) {
                                const int ws = J.mode >= 2 ? jws : t.sx, r0 = J.mode == 3 ? jrs : t.sy;
                                const int r1 = J.mode == 3 ? min(r0 + 1, J.ch - 1) : r0 + 1;
                                const u8* c1 = pl + J.o1 + ws;
                                const u8* c2 = pl + J.o2 + ws;
                                __builtin_memcpy(&jcb[k][0], c1 + (size_t)r0 * J.s1, 4);
                                __builtin_memcpy(&jcb[k][1], c1 + (size_t)r1 * J.s1, 4);
                                __builtin_memcpy(&jcr[k][0], c2 + (size_t)r0 * J.s1, 4);
                                __builtin_memcpy(&jcr[k][1], c2 + (size_t)r1 * J.s1, 4);
                                if (J.mode == 3) {
                                    const int r2 = min(r0 + 2, J.ch - 1);
                                    __builtin_memcpy(&jcb[k][2], c1 + (size_t)r2 * J.s1, 4);
                                    __builtin_memcpy(&jcr[k][2], c2 + (size_t)r2 * J.s1, 4);
                                }
                            }
                        }
                    } else if constexpr (DEEP) {
                        // the 4 x 4 bytes of the 8-bit source, made of the developed samples of columns sx - 1 .. sx + 2
                        const u8* m = S.p0 + (size_t)(f0 + k) * S.r.frame_stride + tap;
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            u32 s4[4];
                            d_deep_row4(m + (size_t)i * S.r.stride0, t.sx - 1, S.d.enc, s4);
                            rows[k][i] = 0;
#pragma unroll
                            for (int j = 0; j < 4; j++) rows[k][i] |= d_deep_byte(deep_tab, S.d, s4[j], t.sx - 1 + j, t.sy - 1 + i) << (8 * j);
                        }
                    } else {
                        const u8* m = S.p0 + (size_t)(f0 + k) * S.r.frame_stride + tap;
#pragma unroll
                        for (int i = 0; i < 4; i++) __builtin_memcpy(&rows[k][i], m + (size_t)i * S.r.stride0, 4);
                    }
                }
#pragma unroll
        for (int k = 0; k < FPT; k++) {
            if (k >= nf) break;
            int o[3] = {0, 0, 0};
            bool fastk = fast; // (JPEG: and the frame's layout has the wide loads)
            if constexpr (JPEG) fastk = fast && jt[k].wide;
            if (t.any_in) {
                // ---- the taps 00, 01, 10, 11.  BGR: v, the bytes as they lie in the frame, -1 for a tap outside it; the
                // others: q, converted, as b | g << 8 | r << 16, 0 for a tap outside
                int v[4][3];
                u32 q[4] = {0u, 0u, 0u, 0u};
                if constexpr (BGR) {
                    if (fast) {
#pragma unroll
                        for (int c = 0; c < 3; c++) {
                            v[0][c] = (int)((ta[k] >> (8 * c)) & 255);
                            v[1][c] = (int)((ta[k] >> (8 * (3 + c))) & 255);
                            v[2][c] = (int)((tb[k] >> (8 * c)) & 255);
                            v[3][c] = (int)((tb[k] >> (8 * (3 + c))) & 255);
                        }
                    } else {
                        const u8* p00 = S.src + (size_t)(f0 + k) * S.g.frame_stride + tap;
                        const u8* p10 = p00 + S.g.stride;
#pragma unroll
                        for (int c = 0; c < 3; c++) {
                            v[0][c] = (t.x0in && t.y0in) ? p00[c] : -1;
                            v[1][c] = (t.x1in && t.y0in) ? p00[3 + c] : -1;
                            v[2][c] = (t.x0in && t.y1in) ? p10[c] : -1;
                            v[3][c] = (t.x1in && t.y1in) ? p10[3 + c] : -1;
                        }
                    }
                } else if (fastk) {
                    if constexpr (PROFILE) {
                        q[0] = conv((u32)ta[k]);
                        q[1] = conv((u32)(ta[k] >> 24));
                        q[2] = conv((u32)tb[k]);
                        q[3] = conv((u32)(tb[k] >> 24));
                    } else if constexpr (YUV) {
                        if (L::F420) {
                            Chroma a0, a1, b0, b1;
                            if (NV12) {
                                const u32 a = ca[k], sa = odd ? a >> 16 : a;
                                a0 = d_chroma_pair<FMT>(a, cs...);
                                a1 = d_chroma_pair<FMT>(sa, cs...);
                                b0 = a0;
                                b1 = a1;
                                if (two_crows) {
                                    const u32 b = cb[k], sb = odd ? b >> 16 : b;
                                    b0 = d_chroma_pair<FMT>(b, cs...);
                                    b1 = d_chroma_pair<FMT>(sb, cs...);
                                }
                            } else {
                                const u32 u0 = ca[k], v0 = va[k];
                                a0 = d_chroma(u0 & 255, v0 & 255, cs...);
                                a1 = d_chroma((odd ? u0 >> 8 : u0) & 255, (odd ? v0 >> 8 : v0) & 255, cs...);
                                b0 = a0;
                                b1 = a1;
                                if (two_crows) {
                                    const u32 u1 = cb[k], v1 = vb[k];
                                    b0 = d_chroma(u1 & 255, v1 & 255, cs...);
                                    b1 = d_chroma((odd ? u1 >> 8 : u1) & 255, (odd ? v1 >> 8 : v1) & 255, cs...);
                                }
                            }
                            q[0] = d_yuv_bgr((int)(ta[k] & 255), a0, cs...);
                            q[1] = d_yuv_bgr((int)((ta[k] >> 8) & 255), a1, cs...);
                            q[2] = d_yuv_bgr((int)(tb[k] & 255), b0, cs...);
                            q[3] = d_yuv_bgr((int)((tb[k] >> 8) & 255), b1, cs...);
                        } else {
#pragma unroll
                            for (int r = 0; r < 2; r++) {
                                const u64 w = r ? tb[k] : ta[k];
                                const u32 lo = (u32)w, hi = (u32)(w >> 32), s1 = odd ? hi : lo;
                                const Chroma c0 = d_chroma((lo >> (8 * L::PU)) & 255, (lo >> (8 * L::PV)) & 255, cs...);
                                const Chroma c1 = d_chroma((s1 >> (8 * L::PU)) & 255, (s1 >> (8 * L::PV)) & 255, cs...);
                                q[2 * r] = d_yuv_bgr((int)((odd ? lo >> (8 * L::Y1) : lo >> (8 * L::Y0)) & 255), c0, cs...);
                                q[2 * r + 1] = d_yuv_bgr((int)((odd ? hi >> (8 * L::Y0) : lo >> (8 * L::Y1)) & 255), c1, cs...);
                            }
                        }
                    } else if constexpr (JPEG) {
                        const JpegTapDesc& J = jt[k];
                        const JpegWin W = {(u32)ta[k], (u32)tb[k], {jcb[k][0], jcb[k][1], jcb[k][2]}, {jcr[k][0], jcr[k][1], jcr[k][2]}, jws, jrs};
                        q[0] = d_jpeg_tap(J, W, t.sx, t.sy, 0, 0);
                        q[1] = d_jpeg_tap(J, W, t.sx, t.sy, 1, 0);
                        q[2] = d_jpeg_tap(J, W, t.sx, t.sy, 0, 1);
                        q[3] = d_jpeg_tap(J, W, t.sx, t.sy, 1, 1);
                    } else if constexpr (DEEP) {
                        const u32* w = rows[k];
                        q[0] = d_deep_bgr(S.d.ph, t.sx, t.sy, w[0], w[1], w[2]);
                        q[1] = d_deep_bgr(S.d.ph, t.sx + 1, t.sy, w[0] >> 8, w[1] >> 8, w[2] >> 8);
                        q[2] = d_deep_bgr(S.d.ph, t.sx, t.sy + 1, w[1], w[2], w[3]);
                        q[3] = d_deep_bgr(S.d.ph, t.sx + 1, t.sy + 1, w[1] >> 8, w[2] >> 8, w[3] >> 8);
                    } else {
                        const u32* w = rows[k];
                        q[0] = d_bayer_bgr<FMT>(t.sx, t.sy, w[0], w[1], w[2]);
                        q[1] = d_bayer_bgr<FMT>(t.sx + 1, t.sy, w[0] >> 8, w[1] >> 8, w[2] >> 8);
                        q[2] = d_bayer_bgr<FMT>(t.sx, t.sy + 1, w[1], w[2], w[3]);
                        q[3] = d_bayer_bgr<FMT>(t.sx + 1, t.sy + 1, w[1] >> 8, w[2] >> 8, w[3] >> 8);
                    }
                } else {
                    if constexpr (PROFILE) {
                        const u8* p00 = S.src + (size_t)(f0 + k) * S.g.frame_stride + tap;
                        const u8* p10 = p00 + S.g.stride;
                        auto px = [&](const u8* p) -> u32 { return conv((u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16)); };
                        if (t.x0in && t.y0in) q[0] = px(p00);
                        if (t.x1in && t.y0in) q[1] = px(p00 + 3);
                        if (t.x0in && t.y1in) q[2] = px(p10);
                        if (t.x1in && t.y1in) q[3] = px(p10 + 3);
                    } else if constexpr (YUV) {
                        const u8* f0p = S.p0 + (size_t)(f0 + k) * S.r.frame_stride;
                        const u8* f1p = L::F420 ? S.p1 + (size_t)(f0 + k) * S.r.frame_stride : nullptr;
                        const u8* f2p = PLANAR ? S.p2 + (size_t)(f0 + k) * S.r.frame_stride : nullptr;
                        if (t.x0in && t.y0in) q[0] = d_raw_px<FMT>(f0p, f1p, f2p, S.r, t.sx, t.sy, cs...);
                        if (t.x1in && t.y0in) q[1] = d_raw_px<FMT>(f0p, f1p, f2p, S.r, t.sx + 1, t.sy, cs...);
                        if (t.x0in && t.y1in) q[2] = d_raw_px<FMT>(f0p, f1p, f2p, S.r, t.sx, t.sy + 1, cs...);
                        if (t.x1in && t.y1in) q[3] = d_raw_px<FMT>(f0p, f1p, f2p, S.r, t.sx + 1, t.sy + 1, cs...);
                    } else if constexpr (JPEG) {
                        const JpegDesc& D = S.descs[f0 + k];
                        const u8* pl = S.planes + (size_t)(f0 + k) * S.plane_stride;
                        if (t.x0in && t.y0in) q[0] = d_jpeg_px(D, pl, t.sx, t.sy);
                        if (t.x1in && t.y0in) q[1] = d_jpeg_px(D, pl, t.sx + 1, t.sy);
                        if (t.x0in && t.y1in) q[2] = d_jpeg_px(D, pl, t.sx, t.sy + 1);
                        if (t.x1in && t.y1in) q[3] = d_jpeg_px(D, pl, t.sx + 1, t.sy + 1);
                    } else if constexpr (DEEP) {
                        const u8* fp = S.p0 + (size_t)(f0 + k) * S.r.frame_stride;
                        if (t.x0in && t.y0in) q[0] = d_deep_px(fp, S.r.stride0, S.sw, S.sh, deep_tab, S.d, t.sx, t.sy);
                        if (t.x1in && t.y0in) q[1] = d_deep_px(fp, S.r.stride0, S.sw, S.sh, deep_tab, S.d, t.sx + 1, t.sy);
                        if (t.x0in && t.y1in) q[2] = d_deep_px(fp, S.r.stride0, S.sw, S.sh, deep_tab, S.d, t.sx, t.sy + 1);
                        if (t.x1in && t.y1in) q[3] = d_deep_px(fp, S.r.stride0, S.sw, S.sh, deep_tab, S.d, t.sx + 1, t.sy + 1);
                    } else {
                        const u8* fp = S.p0 + (size_t)(f0 + k) * S.r.frame_stride;
                        if (t.x0in && t.y0in) q[0] = d_bayer_px<FMT>(fp, S.r.stride0, S.sw, S.sh, t.sx, t.sy);
                        if (t.x1in && t.y0in) q[1] = d_bayer_px<FMT>(fp, S.r.stride0, S.sw, S.sh, t.sx + 1, t.sy);
                        if (t.x0in && t.y1in) q[2] = d_bayer_px<FMT>(fp, S.r.stride0, S.sw, S.sh, t.sx, t.sy + 1);
                        if (t.x1in && t.y1in) q[3] = d_bayer_px<FMT>(fp, S.r.stride0, S.sw, S.sh, t.sx + 1, t.sy + 1);
                    }
                }
                // a raw source's profile: on the converted taps inside the frame (a fast pixel has all four there)
                if constexpr (RAW_TABS) {
                    const bool in[4] = {t.x0in && t.y0in, t.x1in && t.y0in, t.x0in && t.y1in, t.x1in && t.y1in};
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (fastk || in[i]) q[i] = conv(q[i]);
                }
                // ---- the blend
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    int b[4] = {(int)((q[0] >> (8 * c)) & 255), (int)((q[1] >> (8 * c)) & 255), (int)((q[2] >> (8 * c)) & 255), (int)((q[3] >> (8 * c)) & 255)};
                    if constexpr (BGR)
#pragma unroll
                        for (int i = 0; i < 4; i++) b[i] = v[i][c] < 0 ? 0 : (use_lut ? (int)lds.lut[k][v[i][c]] : v[i][c]); // border taps are 0
                    o[c] = warp_blend(b[0], b[1], b[2], b[3], t);
                }
            }
            u8* out = D.dst + (size_t)(f0 + k) * D.frame_stride + t.out_off;
            out[0] = (u8)o[0];
            out[1] = (u8)o[1];
            out[2] = (u8)o[2];
        }
        dy += 4;
    } while (Src::ROWS > 4 && ++row < Src::ROWS / 4 && dy < D.dh);
}

// ---------------------------------------------------------------------------
// The kernels: one template per launch shape, whatever the source, which travels by value as the first argument.
//   k_warp_one     one destination, the matrix by value (launch_warp and what it hands over to)
//   k_warp_boards  every board of a pipeline in one launch, from the BoardDev table (launch_warp_mb ...)
//   k_warp_lens    the table-driven lens form (warp_lens.h), which calls warp_gather itself
// ---------------------------------------------------------------------------
// The gather of source S onto the destination that k_warp_one or k_warp_boards names; a source in another colour space than 0
// hands its constants on as the gather's trailing pack.  `dst` is restrict here because the source's pointers, inside a struct, cannot be: that
// no store to the destination changes what the source's pointers read is what lets the compiler keep the uniform reads of a
// source (a JPEG frame's descriptor) in scalar loads where the destination comes out of a table.
template <class Src, int FPT, bool LENS = false>
__device__ __forceinline__ void warp_gather_of(Src S, const double* M, int dw, int dh, int bw0, int rot180, u8* __restrict__ dst, int dst_stride,
                                               size_t dst_frame_stride, u32* __restrict__ zero_word, u32* __restrict__ zero_word2, int batch, int bz,
                                               const LensDev* lens = nullptr)
{
    const WarpDst D = {M, dw, dh, bw0, rot180, dst, dst_stride, dst_frame_stride};
    if constexpr (Src::CS) warp_gather<Src, FPT, LENS>(S, D, zero_word, zero_word2, batch, bz, lens, S.cs);
    else warp_gather<Src, FPT, LENS>(S, D, zero_word, zero_word2, batch, bz, lens);
}

// blockIdx.z = the group of frames.  A source with a profile (Src::TABS): blockIdx.z = profile * nz + group of frames;
// profile p stages S.pt[p] and writes its frames dst_profile_stride bytes behind profile p - 1's
template <class Src, int FPT>
__global__ __launch_bounds__(256) void k_warp_one(Src S, WarpM M, int dw, int dh, int bw0, int rot180, u8* __restrict__ dst, int dst_stride,
                                                   size_t dst_frame_stride, size_t dst_profile_stride, int nz, u32* __restrict__ zero_word,
                                                   u32* __restrict__ zero_word2, int batch)
{
    int bz = blockIdx.z;
    if constexpr (Src::TABS) {
        const int pi = blockIdx.z / nz;
        S.pt += pi;
        dst += (size_t)pi * dst_profile_stride;
        bz -= pi * nz;
    }
    warp_gather_of<Src, FPT>(S, M.m, dw, dh, bw0, rot180, dst, dst_stride, dst_frame_stride, zero_word, zero_word2, batch, bz);
}

// blockIdx.z = board * nz + group of frames; the grid covers the largest board and the blocks outside a smaller one leave
// at once (what is staged for the shared frames is the same for every board).  A profile is the board's: a workgroup stages
// its board's table.  s0 = the slot of the chunk's frame 0
template <class Src, int FPT>
__global__ __launch_bounds__(256) void k_warp_boards(Src S, const BoardDev* __restrict__ tab, int nz, int s0, u32* __restrict__ zero_word,
                                                      u32* __restrict__ zero_word2, int batch)
{
    const int b = blockIdx.z / nz;
    const BoardDev& T = tab[b];
    if (b > 0 && ((int)blockIdx.x * 64 >= T.S || (int)blockIdx.y * Src::ROWS >= T.S)) return;
    if constexpr (Src::TABS) S.pt = T.ptabs;
    warp_gather_of<Src, FPT>(S, T.Minv, T.S, T.S, T.bw0, T.rot180, T.warped + (size_t)s0 * T.warped_stride, T.S * 3, T.warped_stride, zero_word, zero_word2,
                             batch, blockIdx.z - b * nz);
}

// ---------------------------------------------------------------------------
// The frames per thread of the many-frames form (batch >= 8) of every source; a launch of fewer frames keeps one thread
// per pixel and frame.  Four (eight: 13 % fewer instructions again, no change on the path), but for:
//
// The raw sources with a profile (k_warp_raw_profile.hip, and k_warp_cs.hip, whose forms take what their siblings take),
// per family.  The profile's registers come on top of the conversion's: the four-frame form of every family needs more
// than 64 VGPRs (NV12 79, planar 4:2:0 91, packed 4:2:2 71, Bayer 72), and so does the two-frame form of the 4:2:0
// families (68, 77); at or under 64 stay two frames of packed 4:2:2 and Bayer (60, 62) and one frame of the 4:2:0 families
// (58, 62).  Each family ships the form that was fastest INSIDE p.run on an MI355X (1080p, 512 frames, two lanes), and a
// form above 64 only where it beat the best one at or under 64 by more than the runs' range: per frame, 1 / 2 / 4 frames a
// thread, NV12 8.00 / 6.92 / 6.77 us, planar 4:2:0 8.56 / 7.50 / 7.57, packed 4:2:2 7.50 / 6.30 / 6.05, Bayer 7.92 / 6.83 /
// 6.20 (ranges 0.02 - 0.06).  So four frames everywhere but planar 4:2:0, which takes two.  DESIGN.md section 6n has the
// table; tests/test_warp_raw_profile_resources.py pins the counts.  (RAW_PROFILE_FPT = 1, 2 or 4 in the build's environment
// gives every family that form: tools/raw_profile_timing.py's comparison.)
//
// The YUV sources in another colour space than 0 without a profile (k_warp_cs.hip, k_warp_lens_cs.hip): planar 4:2:0 takes
// two, as its family does with a profile.  Its four-frame form needs 65 or 66 VGPRs once the constants are the launch's (63
// with the compiler's: the multiplies no longer fold into 24-bit multiply-adds) and so crosses the 64 of 8 waves per SIMD.
//
// JPEG planes with a profile (k_warp_jpeg.hip): two.  The plain kernels need 44 VGPRs at one frame and 83 at four; with the
// profile's registers on top 70 at one frame and 93 at two, as the planar 4:2:0 family with a profile, whose loads these
// resemble.  The forms were not timed against each other; tests/test_warp_jpeg_resources.py pins
// the counts.
//
// Under a lens (k_warp_lens_profile.hip, k_warp_lens_cs.hip) every raw or JPEG source with a profile: two.  The lens's
// doubles come on top of the profile's registers and the conversion's, and two is what planar 4:2:0 and the JPEG planes
// take lens-free; the lens forms were not timed against each other.
// ---------------------------------------------------------------------------
template <class Src, bool LENS = false>
constexpr int warp_many()
{
    constexpr bool RAW = Src::KIND == WARP_YUV || Src::KIND == WARP_BAYER, JPEG = Src::KIND == WARP_JPEG;
    constexpr bool PLANAR420 = Src::KIND == WARP_YUV && (Src::FMT & 15) == CBV_FMT_NV12 && (Src::FMT & 0x20); // YUV420P
    // developed mosaics: two, with a profile or without, under a lens or not.  Sixteen table reads per frame come on top of the
    // 8-bit source's registers; the forms were not timed against each other
    if (Src::KIND == WARP_DEEP) return 2;
    if ((RAW || JPEG) && Src::TABS && LENS) return 2;
    if (JPEG) return Src::TABS ? 2 : 4;
#ifdef RAW_PROFILE_FPT
    if (RAW && Src::TABS) return RAW_PROFILE_FPT;
#endif
    if (RAW && (Src::TABS || Src::CS)) return PLANAR420 ? 2 : 4;
    return 4;
}

// ---------------------------------------------------------------------------
// From a WarpSrc to the typed source: per family of sources one function that makes the family's refusals and calls
// f(S) with the source struct, which returns the launch's code.  A unit calls its family's from its lens-free launchers
// and from its lens launcher alike, and instantiates what f does for every source of the family, nothing else.
// ---------------------------------------------------------------------------
template <int N>
using WarpInt = std::integral_constant<int, N>;

// f(fmt) with the compile-time form of the id of a raw format that has passed check_raw_format
template <class F>
static int warp_raw_fmt(int fmt, F&& f)
{
    switch (fmt) {
    case CBV_FMT_NV12: return f(WarpInt<CBV_FMT_NV12>());
    case CBV_FMT_NV21: return f(WarpInt<CBV_FMT_NV21>());
    case CBV_FMT_YUYV: return f(WarpInt<CBV_FMT_YUYV>());
    case CBV_FMT_YVYU: return f(WarpInt<CBV_FMT_YVYU>());
    case CBV_FMT_UYVY: return f(WarpInt<CBV_FMT_UYVY>());
    case CBV_FMT_BAYER_RGGB: return f(WarpInt<CBV_FMT_BAYER_RGGB>());
    case CBV_FMT_BAYER_BGGR: return f(WarpInt<CBV_FMT_BAYER_BGGR>());
    case CBV_FMT_BAYER_GRBG: return f(WarpInt<CBV_FMT_BAYER_GRBG>());
    case CBV_FMT_BAYER_GBRG: return f(WarpInt<CBV_FMT_BAYER_GBRG>());
    default: return f(WarpInt<CBV_FMT_YUV420P>());
    }
}

// the refusals of a raw source (what launch_ingest asks of the planes), and YV12 made YUV420P
static int warp_raw_checked(cbv_ctx* ctx, WarpSrc* s, int batch)
{
    const char* what = s->kind == WarpSrc::BAYER ? "launch_warp_bayer" : "launch_warp_yuv";
    if (!s->raw()) return cbv_fail(ctx, CBV_ERR_ARG, "%s: not a raw source", what);
    RC(check_raw_format(ctx, s->r.fmt, s->g.w, s->g.h, what));
    if (s->deep()) return cbv_fail(ctx, CBV_ERR_ARG, "%s: format %d is a developed mosaic (warp_typed_deep)", what, s->r.fmt);
    // (warp_src_raw takes the kind from the format: only a WarpSrc filled by hand can fail this)
    if (s->kind == WarpSrc::BAYER && !raw_fmt_bayer(s->r.fmt)) return cbv_fail(ctx, CBV_ERR_ARG, "%s: format %d is not a Bayer format", what, s->r.fmt);
    if (batch <= 0) return cbv_fail(ctx, CBV_ERR_ARG, "%s: bad planes or strides", what);
    const int strides[3] = {s->r.stride0, s->r.stride1, s->r.stride2};
    RC(check_raw_planes(ctx, s->r.fmt, s->g.w, s->planes.p, strides, what));
    raw_planes_canonical(&s->planes, &s->r);
    return CBV_OK;
}

// (a mosaic has one plane)
template <int FMT>
static WarpRaw<FMT> warp_raw_of(const WarpSrc& s)
{
    const bool bayer = raw_fmt_bayer(FMT);
    return WarpRaw<FMT>{s.planes.p[0], bayer ? nullptr : s.planes.p[1], bayer ? nullptr : s.planes.p[2], s.r, s.g.w, s.g.h};
}

// BGR frames (both byte-map forms), BGR frames through the profile, raw frames without one: k_warp.hip, k_warp_lens.hip
template <class F>
static int warp_typed_plain(cbv_ctx* ctx, WarpSrc* s, int batch, F&& f)
{
    if (s->kind == WarpSrc::PROFILE) return f(WarpProfile{s->bgr, s->g, ctx->tabs, s->ptabs});
    if (s->kind == WarpSrc::BGR) {
        if (s->norm.minmax) return f(WarpBgr<true>{s->bgr, s->g, nullptr, s->norm.minmax, s->norm.mm_stride});
        return f(WarpBgr<false>{s->bgr, s->g, s->norm.lut, nullptr, 0});
    }
    RC(warp_raw_checked(ctx, s, batch));
    return warp_raw_fmt(s->r.fmt, [&](auto fmt) { return f(warp_raw_of<decltype(fmt)::value>(*s)); });
}

// raw frames with a profile: k_warp_raw_profile.hip, k_warp_lens_profile.hip
template <class F>
static int warp_typed_raw_profile(cbv_ctx* ctx, WarpSrc* s, int batch, const char* who, F&& f)
{
    if (!s->raw() || !s->ptabs) return cbv_fail(ctx, CBV_ERR_ARG, "%s: not a raw source with a profile", who);
    RC(warp_raw_checked(ctx, s, batch));
    return warp_raw_fmt(s->r.fmt, [&](auto fmt) {
        constexpr int FMT = decltype(fmt)::value;
        return f(WarpRawProfile<FMT>{warp_raw_of<FMT>(*s), ctx->tabs, s->ptabs});
    });
}

// YUV frames in colour space 1 to 3, with a profile or without: k_warp_cs.hip, k_warp_lens_cs.hip
template <class F>
static int warp_typed_cs(cbv_ctx* ctx, WarpSrc* s, int batch, const char* who, F&& f)
{
    if (s->kind != WarpSrc::YUV || s->cs < 1 || s->cs > 3) return cbv_fail(ctx, CBV_ERR_ARG, "%s: not a YUV source in colour space 1 to 3 (%d)", who, s->cs);
    RC(warp_raw_checked(ctx, s, batch));
    const YuvCs cs = kYuvCs[s->cs];
    return warp_raw_fmt(s->r.fmt, [&](auto fmt) -> int {
        constexpr int FMT = decltype(fmt)::value;
        if constexpr (raw_fmt_yuv(FMT)) {
            if (s->ptabs) return f(WarpRawProfileCs<FMT>{{warp_raw_of<FMT>(*s), ctx->tabs, s->ptabs}, cs});
            return f(WarpRawCs<FMT>{warp_raw_of<FMT>(*s), cs});
        } else return cbv_fail(ctx, CBV_ERR_ARG, "%s: format %d is not a YUV format", who, s->r.fmt);
    });
}

// developed mosaics, with a profile or without: k_warp_deep.hip, k_warp_lens_deep.hip
template <class F>
static int warp_typed_deep(cbv_ctx* ctx, WarpSrc* s, int batch, const char* who, F&& f)
{
    if (!s->deep()) return cbv_fail(ctx, CBV_ERR_ARG, "%s: not a developed mosaic", who);
    RC(check_raw_format(ctx, s->r.fmt, s->g.w, s->g.h, who));
    if (batch <= 0 || !s->planes.p[0] || !s->bdeep.tab || !bayer_bits_ok(s->r.fmt, s->bdeep.bits) || s->r.stride0 < bayer_row_bytes(s->r.fmt, s->g.w))
        return cbv_fail(ctx, CBV_ERR_ARG, "%s: bad planes, strides or tables (%d bits)", who, s->bdeep.bits);
    const DeepDev d = {s->bdeep.tab, s->bdeep.bits, raw_fmt_enc(s->r.fmt), s->r.fmt & 0x30};
    auto go = [&](auto lds) -> int {
        constexpr bool LDS = decltype(lds)::value != 0;
        const WarpDeep<LDS> D = {s->planes.p[0], s->r, s->g.w, s->g.h, d};
        if (s->ptabs) return f(WarpDeepProfile<LDS>{D, ctx->tabs, s->ptabs});
        return f(D);
    };
    return s->bdeep.bits <= WARP_DEEP_LDS_BITS ? go(WarpInt<1>()) : go(WarpInt<0>());
}

// The decoded planes of JPEG frames, PROFILE: with a profile.  Unlike the three above this one decides at compile time, and
// its callers write `s.ptabs ? <true> : <false>` where they want both: k_warp_jpeg.hip holds both sources, but the lens
// forms are split over k_warp_lens.hip (WarpJpeg) and k_warp_lens_profile.hip (WarpJpegProfile), and a dispatch that chose
// at run time would instantiate both in each, which the units' exact kernel lists forbid.  (const WarpSrc&: nothing to
// canonicalise, where the raw families rewrite YV12's planes.)
template <bool PROFILE, class F>
static int warp_typed_jpeg(cbv_ctx* ctx, const WarpSrc& s, const char* who, F&& f)
{
    if (s.kind != WarpSrc::JPEG || !s.jpeg_planes || !s.jpeg_descs || (s.jpeg_plane_stride & 7) || s.g.w < 1 || s.g.h < 1)
        return cbv_fail(ctx, CBV_ERR_ARG, "%s: not a source of JPEG planes", who);
    const WarpJpeg J = {s.jpeg_planes, s.jpeg_plane_stride, s.jpeg_descs, s.g.w, s.g.h};
    if constexpr (PROFILE) return f(WarpJpegProfile{J, ctx->tabs, s.ptabs});
    else return f(J);
}

// ---------------------------------------------------------------------------
// The launches: one template per kernel template.  MANY = the frames per thread of the many-frames form.
// ---------------------------------------------------------------------------
// What every launch does around its kernel: the groups of frames (MANY frames a group from batch 8 on, one below), the
// refusal of more than 65535 layers, the grid of a dw x dh destination with `zmul` layers per group, the profiling bracket.
// launch(fpt, grid, nz) issues the kernel with fpt's frames per thread; `layers` names what zmul counts, for the message.
template <class Src, int MANY, class L>
static int warp_launch_grid(cbv_ctx* ctx, const char* who, const char* layers, int dw, int dh, int zmul, int batch, L&& launch)
{
    if (batch <= 0 || dw < 1 || dh < 1 || zmul < 1) return cbv_fail(ctx, CBV_ERR_ARG, "%s: bad batch or destination", who);
    const int fpt = batch >= 8 ? MANY : 1, nz = (batch + fpt - 1) / fpt;
    if ((long long)nz * zmul > 65535) return cbv_fail(ctx, CBV_ERR_ARG, "%s: %d %s x %d frames do not fit a launch", who, zmul, layers, batch);
    const dim3 grid((dw + 63) / 64, (dh + Src::ROWS - 1) / Src::ROWS, nz * zmul);
    constexpr int prof = Src::KIND == WARP_DEEP ? CBV_K_WARP_BAYER_DEEP : Src::FMT == CBV_FMT_BGR ? CBV_K_WARP : CBV_K_WARP_YUV;
    prof_begin(ctx, prof);
    if (batch >= 8) launch(WarpInt<MANY>(), grid, nz);
    else launch(WarpInt<1>(), grid, nz);
    prof_end(ctx, prof);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

// where launch_warp and its kin write: one dw x dh board; np profiles of a source with a profile, dst_profile_stride apart
struct WarpOneTo {
    const double* Minv9;
    int dw, dh, rot180;
    u8* dst;
    int stride;
    size_t frame_stride;
    int np;
    size_t profile_stride;
};

template <class Src, int MANY = warp_many<Src>()>
static int warp_launch_one(cbv_ctx* ctx, const char* who, const Src& S, const WarpOneTo& to, int batch, u32* zero_word, u32* zero_word2)
{
    WarpM M;
    for (int i = 0; i < 9; i++) M.m[i] = to.Minv9[i];
    int bw0, bh0;
    warp_block_shape(to.dw, to.dh, &bw0, &bh0);
    return warp_launch_grid<Src, MANY>(ctx, who, "profiles", to.dw, to.dh, Src::TABS ? to.np : 1, batch, [&](auto fpt, dim3 grid, int nz) {
        hipLaunchKernelGGL((k_warp_one<Src, decltype(fpt)::value>), grid, dim3(256), 0, ctx->stream, S, M, to.dw, to.dh, bw0, to.rot180, to.dst, to.stride,
                           to.frame_stride, to.profile_stride, nz, zero_word, zero_word2, batch);
    });
}

// nb boards of at most maxS x maxS
template <class Src, int MANY = warp_many<Src>()>
static int warp_launch_boards(cbv_ctx* ctx, const char* who, const Src& S, const BoardDev* tab, int nb, int maxS, int s0, int batch, u32* zero_word,
                              u32* zero_word2)
{
    return warp_launch_grid<Src, MANY>(ctx, who, "boards", maxS, maxS, nb, batch, [&](auto fpt, dim3 grid, int nz) {
        hipLaunchKernelGGL((k_warp_boards<Src, decltype(fpt)::value>), grid, dim3(256), 0, ctx->stream, S, tab, nz, s0, zero_word, zero_word2, batch);
    });
}
