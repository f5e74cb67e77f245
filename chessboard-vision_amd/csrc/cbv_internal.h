// Internal declarations shared by the HIP translation units of libcbv_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/cbv.h"
#include "frame_plan.h"
#include "lens_core.h"

typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;

// ---------------------------------------------------------------------------
// constant tables (device copies live in cbv_ctx::tabs)
// ---------------------------------------------------------------------------
enum {
    LAB_SHIFT = 12, GAMMA_SHIFT = 3, LAB_SHIFT2 = LAB_SHIFT + GAMMA_SHIFT,
    LAB_CBRT_TAB_SIZE_B = 256 * 3 / 2 * (1 << GAMMA_SHIFT),
    INV_GAMMA_SHIFT = 12, INV_GAMMA_TAB_SIZE = 1 << INV_GAMMA_SHIFT,
    LAB_BASE_SHIFT = 14, LAB_BASE = 1 << LAB_BASE_SHIFT
};

struct StaticTabs {
    int sdiv[256];                       // RGB2HSV_b saturation divisors
    int hdiv[256];                       // RGB2HSV_b hue divisors (hrange 180)
    u16 gamma[256];                      // sRGBGammaTab_b
    u16 cbrt[LAB_CBRT_TAB_SIZE_B];       // LabCbrtTab_b
    u16 inv_gamma[INV_GAMMA_TAB_SIZE];   // sRGBInvGammaTab_b
    u16 lab_yf[512];                     // LabToYF_b (y, ify) pairs
    int fwd[9];                          // RGB2Lab_b coefficients (BGR order)
    int inv[9];                          // Lab2RGBinteger coefficients
};

// apply_color_profile reduced to byte->byte tables (frame_enhancer.py:71-97)
struct ProfileTabs {
    u8 csa[256];      // convertScaleAbs(alpha=contrast, beta=brightness)
    u8 hmap[256];     // clip((h + hue_shift) % 180, 0, 179) -> uint8
    u8 vmap[256];     // clip(v * val_scale, 0, 255) -> uint8
    u8 smap[2][256];  // [radical mask][s]: clip(s * {1, 0.5, 2} * sat_scale, 0, 255) -> uint8
    u8 hmask[256];    // radical-mode window membership of h
    int enabled;
    int radical;      // radical_mode of the profile
    // HSV2RGB_b inputs per byte, evaluated on the host in float32 exactly as the device used to:
    u32 hsel[256];    // v_perm selector of (b, g, r) among {v, v(1-s), v(1-s f), v(1-s(1-f))} for hue byte h
    float hfr[256];   // f  = frac(hmap[h] * 6/180)
    float s_f[2][256]; // smap[m][s] * (1/255)
    float v_f[256];    // vmap[v] * (1/255)
};

#define CBV_BL_MAXCLS 10  // distinct dy^2 + dx^2 inside a disc of radius <= 4
struct BilateralTabs {
    float color_w[768];
    float space_w[128];
    signed char dy[128], dx[128];
    int maxk, radius;
    // w = space_w * color_w as ONE table lookup: taps with the same dy^2 + dx^2 share a space weight ("class"), and
    // folded[c][i] = space_w(class c) * color_w[i] is the very float product the filter would form (one IEEE multiply)
    float folded[CBV_BL_MAXCLS][768];
    int tap_off[9][16];  // [dy + radius][dx + radius]: class * 768 (word offset into folded), -1 outside the disc
    int ncls;
};

void build_static_tabs(StaticTabs* t);
void build_profile_tabs(const cbv_color_profile* p, ProfileTabs* t);
int build_bilateral_tabs(int d, double sigma_color, double sigma_space, BilateralTabs* t);
void build_gaussian_q8(int k, int* coef);
void build_piece_mask(int w, int h, u8* mask);
int host_invert3x3(const double* S, double* D);

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    unsigned long long tag = 0; // what the owner knows about the contents; 0 after every (re)allocation
    template <class T> T* as() const { return (T*)p; }
};

struct ProfSlot {
    hipEvent_t a, b;
    int kid;
};

struct cbv_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    char devname[256] = {0};
    int num_cus = 256;

    StaticTabs* tabs = nullptr;          // device
    ProfileTabs* ptabs = nullptr;        // device, current profile
    cbv_color_profile ptabs_key;
    bool ptabs_valid = false;
    BilateralTabs* btabs = nullptr;      // device
    BilateralTabs btabs_host;
    int btabs_offsets_bad = 0;           // bilateral_offsets_mismatch(&btabs_host), worked out when the tables are built
    bool btabs_centre_bad = false;       // bilateral_centre_mismatch(&btabs_host), likewise
    int b_d = -1;
    double b_sc = 0, b_ss = 0;

    // scratch for the host-buffer entry points
    DevBuf in, a, b, c, small;

    // profiling
    int prof_kid = -2;
    std::vector<ProfSlot> prof_pending;
    std::vector<hipEvent_t> prof_pool;
    double prof_ms[CBV_K_END] = {0};
    long long prof_n[CBV_K_END] = {0};

    // One context = one queue of work: its scratch buffers and `stream` are shared by every object created on it, and
    // cbv_pipeline_run points `stream` at its lanes while it enqueues.  Entry points that touch the GPU hold this lock
    // for their whole call (CBV_ENTER), so calls from several threads on one context serialise instead of corrupting it.
    std::recursive_mutex mu;
    bool hough_lds_raised = false; // k_hough's dynamic-LDS limit was raised for this device

    // pinned staging for the small records the one-frame-per-call (class API) entry points move in either direction
    // (square descriptors, worklists, statistics, HoughCircles results): a copy from / to pinned memory is one DMA
    // (12 us for 16 KB against 26 us through the runtime's pageable path); guarded by `mu`, and every call that uses
    // it synchronises before it returns, with an error code too (CBV_ENTER_DRAINED)
    u8* h_stage = nullptr;
    size_t h_stage_cap = 0;
    int debug_poison = 0; // tests: fill partially uploaded staging buffers with 0xA5 first (cbv_debug_poison)

    // Worker streams of the pipelines created on this context (lanes 1.., temporal scan, ingest copies).  They belong to
    // the context, not to a pipeline: a HIP process has four hardware queues by default and streams beyond them share
    // a queue and serialise, so K camera streams on one GPU (K pipelines) must not bring K sets of streams.  All
    // pipelines of a context enqueue from under its lock, in order, so sharing changes no dependency.
    hipStream_t lane_streams[4] = {nullptr, nullptr, nullptr, nullptr};
    hipStream_t scan_stream = nullptr, copy_stream = nullptr;
    int lane_rr = 0; // next lane of the round the pipelines' chunks are dealt on (cbv_pipeline_run)
    bool hough_mb_lds_raised = false; // the same for k_hough's multi-board instance
};
int ctx_worker_stream(cbv_ctx* ctx, hipStream_t* slot, hipStream_t* out);
int ctx_hstage(cbv_ctx* ctx, size_t bytes, u8** p);

extern thread_local std::string g_cbv_err;
int cbv_fail(cbv_ctx* ctx, int code, const char* fmt, ...);

#define CBV_HIP(ctx, call)                                                                          \
    do {                                                                                            \
        hipError_t e__ = (call);                                                                    \
        if (e__ != hipSuccess)                                                                      \
            return cbv_fail(ctx, CBV_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), \
                            __FILE__, __LINE__);                                                    \
    } while (0)

// first statement of every entry point that uses the GPU through `ctx`
#define CBV_ENTER(ctx)                                   \
    std::lock_guard<std::recursive_mutex> lock__((ctx)->mu); \
    CBV_HIP(ctx, hipSetDevice((ctx)->device))

// CBV_ENTER for an entry point that copies from or to the caller's memory or h_stage on ctx->stream: it returns
// `CBV_DONE(rc)` where it is finished, and every return with an error code (RC, CBV_HIP and cbv_fail included) waits for
// the stream first, so nothing is in flight from or to memory the caller, or the next call, may reuse.  The wait's own
// result is dropped: the first error is the one reported.  A successful call never reaches the wait.
struct StreamDrain {
    cbv_ctx* ctx;
    bool armed = true;
    int done(int rc) { armed = rc != CBV_OK; return rc; }
    ~StreamDrain() { if (armed) (void)hipStreamSynchronize(ctx->stream); }
};
#define CBV_ENTER_DRAINED(ctx) \
    CBV_ENTER(ctx);            \
    StreamDrain drain__{ctx}
#define CBV_DONE(rc) drain__.done(rc)

int dev_ensure(cbv_ctx* ctx, DevBuf* b, size_t bytes);
void dev_free(DevBuf* b);
int ctx_set_profile(cbv_ctx* ctx, const cbv_color_profile* p);
int ctx_set_bilateral(cbv_ctx* ctx, int d, double sc, double ss);
int profile_tabs_checked(cbv_ctx* ctx, const cbv_color_profile* p, ProfileTabs* out, const char* who);

// RAII-less helpers to bracket a launch with profiling events
void prof_begin(cbv_ctx* ctx, int kid);
void prof_end(cbv_ctx* ctx, int kid);

// ---------------------------------------------------------------------------
// frame geometry for batched launches: `batch` frames, each frame_stride bytes
// apart, rows `stride` bytes apart.
// ---------------------------------------------------------------------------
struct Geom {
    int w, h;
    int stride;          // bytes per row
    size_t frame_stride; // bytes between consecutive frames of a batch
};

// ---------------------------------------------------------------------------
// Region-limited enhancement (cbv_pipeline_config::enhance_region).  The pipeline's only consumer of the enhanced frame
// is the warp, which samples the board quad; CLAHE apply, the bilateral and the sharpen + min/max pass therefore first
// run on the part of the frame the quad (+ their stencil halos) needs.  normalize needs the min / max of the WHOLE
// sharpened frame, but bytes cannot leave [0, 255]: if the region already holds a 0 and a 255 they ARE the global
// extremes and the rest of the frame cannot change any output.  A second pass over the complement of each kernel's
// region follows; its workgroups leave at once for frames whose region saturated (SatGate) and do the work otherwise,
// so results are identical to whole-frame enhancement in every case.
// ---------------------------------------------------------------------------
struct PxRect {
    int x0, y0, x1, y1; // pixels [x0, x1) x [y0, y1)
};

// up to four rectangles of a kernel's own tiles (one = a region, four = its complement), enumerated as ONE index space
struct TileSet {
    int n;
    int x0[4], y0[4], w[4];
    int cum[5]; // cum[k] = tiles in the rectangles before k; cum[n] = tiles per frame
};

// (constant indices and selects only: the set lives in kernel-argument SGPRs, a dynamic index would turn every call into
// scalar loads from the argument segment with an s_waitcnt behind them)
__host__ __device__ static inline void tileset_at(const TileSet& T, int r, int& tx, int& ty)
{
    int x0 = T.x0[0], y0 = T.y0[0], w = T.w[0], c = 0;
    if (T.n > 1 && r >= T.cum[1]) { x0 = T.x0[1]; y0 = T.y0[1]; w = T.w[1]; c = T.cum[1]; }
    if (T.n > 2 && r >= T.cum[2]) { x0 = T.x0[2]; y0 = T.y0[2]; w = T.w[2]; c = T.cum[2]; }
    if (T.n > 3 && r >= T.cum[3]) { x0 = T.x0[3]; y0 = T.y0[3]; w = T.w[3]; c = T.cum[3]; }
    const int l = r - c;
    const int row = l / w;
    ty = y0 + row;
    tx = x0 + (l - row * w);
}

static inline void tileset_add(TileSet& T, int x0, int y0, int x1, int y1)
{
    if (x1 <= x0 || y1 <= y0) return;
    T.x0[T.n] = x0;
    T.y0[T.n] = y0;
    T.w[T.n] = x1 - x0;
    T.cum[T.n + 1] = T.cum[T.n] + (x1 - x0) * (y1 - y0);
    T.n++;
}

// tiles [x0, x1) x [y0, y1) of a txn x tyn grid, or (invert) every other tile: strips above, below, left, right
static inline TileSet tileset_make(int txn, int tyn, int x0, int y0, int x1, int y1, bool invert)
{
    TileSet T;
    memset(&T, 0, sizeof(T));
    x0 = x0 < 0 ? 0 : x0;
    y0 = y0 < 0 ? 0 : y0;
    x1 = x1 > txn ? txn : x1;
    y1 = y1 > tyn ? tyn : y1;
    if (x1 <= x0 || y1 <= y0) x0 = x1 = y0 = y1 = 0; // empty region: its complement is everything
    if (!invert) tileset_add(T, x0, y0, x1, y1);
    else {
        tileset_add(T, 0, 0, txn, y0);
        tileset_add(T, 0, y1, txn, tyn);
        tileset_add(T, 0, y0, x0, y1);
        tileset_add(T, x1, y0, txn, y1);
    }
    if (T.n == 0) T.w[0] = 1; // no tiles: cum[0] = 0, never dereferenced with r < 0
    return T;
}

// frames whose min / max words (aux, after the region pass of sharpen) already read 0 / 255 are skipped
struct SatGate {
    const u32* mm;       // min word of frame 0 (max follows), or null = no gate
    size_t stride_words; // between frames
};
__device__ static inline bool sat_gate_closed(const SatGate& G, int frame)
{
    return G.mm && G.mm[(size_t)frame * G.stride_words] == 0u && G.mm[(size_t)frame * G.stride_words + 1] == 255u;
}

// k_sharpen_box's region: bytes [b0, b1) of the rows (multiples of 16: a lane's chunk) x rows [y0, y1) (multiples of the
// tile height); invert = everything else
struct ShRegion {
    int b0, b1, y0, y1, invert;
};

struct EnhanceRegion {
    PxRect px;   // what the consumer samples (clipped to the frame)
    int invert;  // 0: the region pass, 1: the complement pass
    SatGate gate;
};

struct ClaheGeom {
    int tiles_x, tiles_y, tw, th; // tile size of the (possibly extended) image
    int clip;                     // integer clip limit (0 = none)
    float lut_scale;
    int divisible;                // image dims divisible by the tile grid
};
ClaheGeom clahe_geom(int w, int h, double clip_limit, int tiles_x, int tiles_y);

// per-frame small device state of the enhancement chain
struct FrameAux {
    u32 hist[1];  // layout helper only
};
// layout of the per-frame aux block (u32 units)
//   [0 .. T*256)         CLAHE histograms
//   then 2               min, max of the sharpen output
//   then 256             otsu histogram
//   then 1               otsu threshold
__host__ __device__ static inline size_t aux_words(int tiles) { return (size_t)tiles * 256 + 2 + 256 + 2; }

// ---------------------------------------------------------------------------
// kernel launchers (device pointers; asynchronous on ctx->stream)
// ---------------------------------------------------------------------------
int launch_reset_aux(cbv_ctx* ctx, u32* aux, int tiles, int batch);
int launch_color_lab_hist(cbv_ctx* ctx, const u8* src, u8* lab, u32* aux, Geom g, ClaheGeom cg, int batch,
                          int do_profile, int do_lab);
// self_clean: the histograms are zeroed once read and [min, max] set to 255, 0, i.e. the kernel leaves the frame's words as
// k_reset_aux would, for the NEXT pass over the same buffer (k_sharpen's min / max come later in this pass)
int launch_clahe_lut(cbv_ctx* ctx, u32* aux, u8* luts, ClaheGeom cg, int batch, u32* packed, int self_clean = 0);
int launch_clahe_apply(cbv_ctx* ctx, const u8* lab, const u32* packed, u8* dst, Geom g, ClaheGeom cg, int batch, const EnhanceRegion* er = nullptr);
int launch_clahe_gray(cbv_ctx* ctx, const u8* src, int w, int h, int stride, ClaheGeom cg, u32* aux, u8* luts, u8* dst);
int launch_bilateral(cbv_ctx* ctx, const u8* src, u8* dst, Geom g, int batch, const EnhanceRegion* er = nullptr);
int launch_sharpen(cbv_ctx* ctx, const u8* src, u8* dst, u32* aux, int tiles, Geom g, const float* k9, int batch, const EnhanceRegion* er = nullptr);
// pixel rectangles the region pass of a kernel covers / must find complete in its input (tile rounding, halos); `out` of
// one stage dilated by its halo is the `need` of the stage before it
bool sharpen_region_ok(const float* k9);
PxRect sharpen_region_cover(Geom g, PxRect need);
PxRect bilateral_region_cover(cbv_ctx* ctx, Geom g, int batch, PxRect need);
// taps whose compile-time table offset in k_bilateral.hip differs from t->tap_off (0: the straight-line rows may run)
int bilateral_offsets_mismatch(const BilateralTabs* t);
// the centre tap's table entry is not exactly 1.0f, the constant the straight-line rows use in its place
bool bilateral_centre_mismatch(const BilateralTabs* t);
PxRect clahe_region_cover(Geom g, PxRect need);
int launch_norm_lut(cbv_ctx* ctx, const u32* aux, int tiles, u8* norm_lut, int batch);
// Where a kernel takes cv2.normalize's byte map from: a table k_norm_lut built ([frame][256]), or the frames' [min, max]
// words themselves (`minmax` = frame 0's, `mm_stride` words apart), from which every workgroup works out the table it needs:
// a launch of a frame or two is launch latency, and that way the chain has one launch fewer.  Neither: no mapping.
struct NormSrc {
    const u8* lut = nullptr;
    const u32* minmax = nullptr;
    size_t mm_stride = 0;
};
static inline NormSrc norm_from_lut(const u8* lut)
{
    NormSrc n;
    n.lut = lut;
    return n;
}
static inline NormSrc norm_from_minmax(const u32* aux, int tiles)
{
    NormSrc n;
    n.minmax = aux + (size_t)tiles * 256;
    n.mm_stride = aux_words(tiles);
    return n;
}
int launch_normalize(cbv_ctx* ctx, const u8* src, u8* dst, NormSrc norm, Geom g, int batch);
// WarpPerspectiveInvoker's block shape of a dw x dh destination (BLOCK_SZ = 32): what the warp launchers pass to their
// kernels and the multi-board table holds per board (BoardDev::bw0, bh0)
static inline void warp_block_shape(int dw, int dh, int* bw0_out, int* bh0_out)
{
    const int BLOCK_SZ = 32;
    int bh0 = BLOCK_SZ / 2 < dh ? BLOCK_SZ / 2 : dh;
    int bw0 = BLOCK_SZ * BLOCK_SZ / bh0 < dw ? BLOCK_SZ * BLOCK_SZ / bh0 : dw;
    bh0 = BLOCK_SZ * BLOCK_SZ / bw0 < dh ? BLOCK_SZ * BLOCK_SZ / bw0 : dh;
    *bw0_out = bw0;
    *bh0_out = bh0;
}
int launch_gray_blur_hist(cbv_ctx* ctx, const u8* src, u8* gray, u8* blur, u32* aux, int tiles, Geom g, int batch);
int launch_otsu(cbv_ctx* ctx, u32* aux, int tiles, int total, int batch);
int launch_threshold(cbv_ctx* ctx, const u8* blur, u8* binary, const u32* aux, int tiles, int w, int h, int batch);
int launch_synth(cbv_ctx* ctx, u8* dst, Geom g, const u64* seeds_dev, const double* hinv_dev, const u8* boards_dev,
                 const cbv_scene* scene_dev, int batch);

// Raw (camera-native) frames of a batch for k_ingest: plane pointers are those of frame 0, frames `frame_stride` bytes apart
struct RawGeom {
    int fmt;                       // CBV_FMT_* of a YUV or Bayer format
    int stride0, stride1, stride2; // bytes per row of plane 0 (luma, the packed 4:2:2 bytes, or the mosaic) / plane 1 / plane 2, in memory order
    size_t frame_stride;
};
// (the bit fields of a format id: frame_plan.h has raw_fmt_bayer, raw_fmt_420 and raw_frame_bytes)
static inline bool raw_fmt_known(int fmt)
{
    return fmt == CBV_FMT_NV12 || fmt == CBV_FMT_NV21 || fmt == CBV_FMT_YUV420P || fmt == CBV_FMT_YV12 || fmt == CBV_FMT_YUYV ||
           fmt == CBV_FMT_YVYU || fmt == CBV_FMT_UYVY || raw_fmt_bayer(fmt);
}
static inline int raw_fmt_planes(int fmt) { return !raw_fmt_420(fmt) ? 1 : (fmt & 0x20) ? 3 : 2; }
static inline const char* raw_fmt_name(int fmt)
{
    switch (fmt) {
    case CBV_FMT_BGR: return "BGR";
    case CBV_FMT_MJPEG: return "MJPEG";
    case CBV_FMT_NV12: return "NV12";
    case CBV_FMT_NV21: return "NV21";
    case CBV_FMT_YUV420P: return "YUV420P";
    case CBV_FMT_YV12: return "YV12";
    case CBV_FMT_YUYV: return "YUYV";
    case CBV_FMT_YVYU: return "YVYU";
    case CBV_FMT_UYVY: return "UYVY";
    case CBV_FMT_BAYER_RGGB: return "BAYER_RGGB";
    case CBV_FMT_BAYER_BGGR: return "BAYER_BGGR";
    case CBV_FMT_BAYER_GRBG: return "BAYER_GRBG";
    case CBV_FMT_BAYER_GBRG: return "BAYER_GBRG";
    }
    if (raw_fmt_bayer(fmt)) { // a layout with a sample encoding (CBV_BAYER_*)
        static const char* const kDeep[3][4] = {{"BAYER_RGGB16", "BAYER_BGGR16", "BAYER_GRBG16", "BAYER_GBRG16"},
                                                {"BAYER_RGGB10P", "BAYER_BGGR10P", "BAYER_GRBG10P", "BAYER_GBRG10P"},
                                                {"BAYER_RGGB12P", "BAYER_BGGR12P", "BAYER_GRBG12P", "BAYER_GBRG12P"}};
        return kDeep[raw_fmt_enc(fmt) - 1][(fmt >> 4) & 3];
    }
    return "?";
}
// bytes per row of plane `i` of a w-wide frame (0: the format has no such plane)
static inline int raw_plane_wbytes(int fmt, int w, int i)
{
    if (i == 0) return raw_fmt_bayer(fmt) ? bayer_row_bytes(fmt, w) : raw_fmt_420(fmt) ? w : 2 * w;
    return i >= raw_fmt_planes(fmt) ? 0 : raw_fmt_planes(fmt) == 3 ? w / 2 : w;
}
static inline int raw_plane_rows(int fmt, int h, int i) { return i == 0 ? h : h / 2; }
// tightly packed raw frames, planes back to back, each frame rounded to 256 bytes (the ingest rings); fmt BGR: tight_geom's frame_stride
static inline RawGeom tight_raw_geom(int fmt, int w, int h)
{
    RawGeom r;
    r.fmt = fmt;
    r.stride0 = raw_plane_wbytes(fmt, w, 0);
    r.stride1 = raw_plane_wbytes(fmt, w, 1);
    r.stride2 = raw_plane_wbytes(fmt, w, 2);
    r.frame_stride = (raw_frame_bytes(fmt, w, h) + 255) & ~(size_t)255;
    return r;
}
// the planes of a tightly packed frame (tight_raw_geom) that starts at `base`; null for the planes the format lacks
struct RawPlanes {
    const u8* p[3];
};
static inline RawPlanes tight_raw_planes(int fmt, int w, int h, const u8* base)
{
    RawPlanes r = {{base, nullptr, nullptr}};
    const int n = raw_fmt_planes(fmt);
    if (n > 1) r.p[1] = base + (size_t)w * h;
    if (n > 2) r.p[2] = r.p[1] + (size_t)(w / 2) * (h / 2);
    return r;
}
// How the samples of a mosaic become bytes (include/cbv.h, "developed mosaics"): the device tables [3][1 << bits], B G R.
// tab == null: none, which only an 8-bit id may have; it then runs k_ingest and the WarpRaw kernels as it always did.
struct BayerDeep {
    const u8* tab = nullptr;
    int bits = 0;
};
static inline bool bayer_deep(int fmt, const BayerDeep& d) { return raw_fmt_enc(fmt) != 0 || d.tab != nullptr; }
// CBV_ERR_ARG, with the format's name, for colour-space bits (CBV_CS_*) on an id that is not one of the YUV formats
int check_fmt_cs(cbv_ctx* ctx, int fmt, const char* what);
// CBV_ERR_ARG unless fmt is a YUV format and w (and h, for the 4:2:0 formats) is even, or a Bayer format and w and h are
// even and at least 4.  fmt: an id as the caller passed it (check_fmt_cs is part of this) or its layout alone
int check_raw_format(cbv_ctx* ctx, int fmt, int w, int h, const char* what);
// CBV_ERR_ARG unless every plane the format has is there with rows of at least their length
int check_raw_planes(cbv_ctx* ctx, int fmt, int w, const u8* const* planes, const int* strides, const char* what);
// YV12 -> YUV420P with the chroma planes (and their strides) swapped: the kernels have no YV12 form
void raw_planes_canonical(RawPlanes* planes, RawGeom* r);
// cv2.cvtColor COLOR_YUV2BGR_* / COLOR_Bayer??2BGR of `batch` raw frames into BGR frames of geometry g (k_ingest.hip); planes
// in memory order.  r.fmt is the layout; cs (raw_fmt_cs: 0 .. 3, YUV only) chooses the colour space: 0 launches k_ingest, the
// others k_ingest_cs (k_ingest_cs.hip) with that row of kYuvCs
int launch_ingest(cbv_ctx* ctx, RawPlanes planes, RawGeom r, u8* dst, Geom g, int batch, int cs = 0);
// the same for developed mosaics (k_ingest_deep.hip): r.fmt a Bayer id of any encoding, deep.tab its tables (never null here),
// deep.bits what bayer_bits_ok admits.  Counted as CBV_K_INGEST_BAYER_DEEP
int launch_ingest_deep(cbv_ctx* ctx, const u8* mosaic, RawGeom r, u8* dst, Geom g, int batch, BayerDeep deep);
// launch_ingest or launch_ingest_deep, as bayer_deep(r.fmt, deep) says
int launch_ingest_any(cbv_ctx* ctx, RawPlanes planes, RawGeom r, u8* dst, Geom g, int batch, int cs, BayerDeep deep);
// The tables of a developed mosaic on the device: `tables` ([3][1 << bits], host) or, null, the default of `fmt` (the neutral
// table of bayer_default_bits; none for an 8-bit id: *out is then empty).  CBV_ERR_ARG for bits that do not go with fmt.
// Synchronous: the copy has landed when it returns.  The caller has made sure nothing in flight reads `buf`.
int bayer_tables_upload(cbv_ctx* ctx, DevBuf* buf, int fmt, const u8* tables, int bits, BayerDeep* out, const char* who);
void launch_ingest_cs(cbv_ctx* ctx, const RawPlanes& planes, const RawGeom& r, u8* dst, const Geom& g, int batch, int cs, bool wide);
// the planes and strides a host frame's format has; null / 0 for the rest, whose fields are not read
void raw_frame_planes(const cbv_raw_frame* raw, const u8** planes, int* strides);
// one raw host frame (any YUV or Bayer format, strided views) into the context's staging buffer (ctx->in), which keeps 256
// readable bytes behind the last plane: its device planes and their strides.  raw->fmt is split here: r->fmt is the layout,
// *cs the colour space
int raw_h2d_stage(cbv_ctx* ctx, const cbv_raw_frame* raw, int w, int h, RawPlanes* dev, RawGeom* r, int* cs, const char* what);
// ... and from there into a BGR device image
// (a Bayer frame: *deep are its tables; null = the default of its format, which for a sample encoding is uploaded to ctx->b)
int raw_h2d_convert(cbv_ctx* ctx, const cbv_raw_frame* raw, int w, int h, u8* dst, Geom g, const char* what, const BayerDeep* deep = nullptr);

// What the warp samples: the frames of a batch, frame 0's pointers.  The launchers turn it into the typed source of the
// kernels (warp_gather.h, warp_typed_*).
struct JpegDesc;
struct WarpSrc {
    enum Kind { BGR, PROFILE, YUV, BAYER, JPEG } kind;
    Geom g;                    // the frames' width and height; BGR, PROFILE: their strides too
    const u8* bgr;             // BGR, PROFILE
    NormSrc norm;              // BGR: cv2.normalize's byte map applied to the taps (none: the plain warp)
    const ProfileTabs* ptabs;  // PROFILE, and YUV / BAYER with a profile (warp_src_raw_profile): device tables [np]
    int np;
    size_t dst_profile_stride;
    RawPlanes planes;          // YUV, BAYER: in memory order
    RawGeom r;                 // (fmt = CBV_FMT_BGR for BGR and PROFILE)
    int cs;                    // YUV: the colour space (raw_fmt_cs); not 0: the runtime-matrix kernels (k_warp_cs.hip, k_warp_lens_cs.hip)
    const u8* jpeg_planes;     // JPEG: the decoded planes of frame 0, frame f's jpeg_plane_stride * f bytes behind
    size_t jpeg_plane_stride;
    const JpegDesc* jpeg_descs; // JPEG: device, frame 0's; each frame has its own layout
    BayerDeep bdeep;           // BAYER: the tables of a developed mosaic (warp_src_raw_deep)
    bool deep() const { return kind == BAYER && bayer_deep(r.fmt, bdeep); } // ... which k_warp_deep.hip and k_warp_lens_deep.hip warp
    bool raw() const { return kind == YUV || kind == BAYER; }
    bool profiled() const { return kind == PROFILE || ((raw() || kind == JPEG) && ptabs); } // the profile kernels' tiling (WP_ROWS rows a workgroup)
};
// BGR frames (WarpBgr), the taps through `norm`
static inline WarpSrc warp_src_bgr(const u8* src, Geom g, NormSrc norm)
{
    WarpSrc s = {};
    s.kind = WarpSrc::BGR;
    s.g = g;
    s.bgr = src;
    s.norm = norm;
    s.r.fmt = CBV_FMT_BGR;
    return s;
}
// BGR frames with the colour profile applied to the taps (WarpProfile): apply_color_profile followed by the warp, byte
// for byte, with no converted frame in between, for `np` profiles at once.  ptabs[np] = device tables (build_profile_tabs),
// the caller's, not ctx->ptabs; profile p writes its `batch` frames at dst + p * dst_profile_stride; a table with
// enabled = 0 is the plain warp.  np x groups of frames (warp_many frames a group from batch 8 on) <= 65535.  The multi-board
// launch reads the boards' own tables (BoardDev::ptabs) instead of `ptabs`.  Counted as CBV_K_WARP: the enumeration of profile
// ids is closed.
static inline WarpSrc warp_src_profile(const u8* src, Geom g, const ProfileTabs* ptabs, int np = 1, size_t dst_profile_stride = 0)
{
    WarpSrc s = warp_src_bgr(src, g, NormSrc());
    s.kind = WarpSrc::PROFILE;
    s.ptabs = ptabs;
    s.np = np;
    s.dst_profile_stride = dst_profile_stride;
    return s;
}
// Raw frames (WarpRaw<FMT>, YUV layouts and mosaics): the output of launch_ingest followed by the warp without a byte
// map, byte for byte, with no BGR frame in between; g = the frames' width and height.  YUV: interior pixels load both taps
// of a row at once: 4 bytes at the even column of an NV12 / NV21 chroma row, 8 bytes at the first tap's pair of a packed
// 4:2:2 row, 2 bytes at column sx >> 1 of each planar chroma row, which at sx = w - 2 reach 2 / 4 / 1 bytes past the row's
// w (2 w, w / 2) bytes.  Callers keep >= 8 readable bytes behind the last row of the last plane of the last frame (the
// pipeline's raw ring has 256); between rows, planes and frames the bytes read belong to the next row, plane or frame.
// Bayer: the four taps are demosaiced before the blend, and no byte outside the frames' rows is read.
static inline WarpSrc warp_src_raw(RawPlanes planes, RawGeom r, Geom g, int cs = 0)
{
    WarpSrc s = {};
    s.kind = raw_fmt_bayer(r.fmt) ? WarpSrc::BAYER : WarpSrc::YUV;
    s.g = g;
    s.planes = planes;
    s.r = r;
    s.cs = cs;
    return s;
}
// A developed mosaic (include/cbv.h; k_warp_deep.hip, k_warp_lens_deep.hip: WarpDeep, WarpDeepProfile): launch_ingest_deep
// followed by the warp (with ptabs: and the colour profile in between), byte for byte.  r.fmt is a Bayer id of any encoding, the
// rows are bayer_row_bytes long, and no byte outside the frames' rows is read.  ptabs / np / dst_profile_stride as
// warp_src_raw_profile takes them.  Counted as CBV_K_WARP_BAYER_DEEP.
static inline WarpSrc warp_src_raw_deep(RawPlanes planes, RawGeom r, Geom g, BayerDeep deep, const ProfileTabs* ptabs = nullptr, int np = 1,
                                        size_t dst_profile_stride = 0)
{
    WarpSrc s = warp_src_raw(planes, r, g, 0);
    s.bdeep = deep;
    s.ptabs = ptabs;
    s.np = np;
    s.dst_profile_stride = dst_profile_stride;
    return s;
}
// Raw frames with the colour profile applied to the converted taps (k_warp_raw_profile.hip): launch_ingest, then
// apply_color_profile, then the warp, byte for byte, with neither frame in between; ptabs / np / dst_profile_stride as
// warp_src_profile takes them, the slack behind the frames as warp_src_raw asks.  The multi-board launch reads the boards'
// own tables (BoardDev::ptabs) instead of `ptabs`, which only has to be non-null there.  Counted as CBV_K_WARP_YUV.
static inline WarpSrc warp_src_raw_profile(RawPlanes planes, RawGeom r, Geom g, const ProfileTabs* ptabs, int np = 1, size_t dst_profile_stride = 0,
                                           int cs = 0)
{
    WarpSrc s = warp_src_raw(planes, r, g, cs);
    s.ptabs = ptabs;
    s.np = np;
    s.dst_profile_stride = dst_profile_stride;
    return s;
}
// The decoded planes of Motion-JPEG frames (k_warp_jpeg.hip): k_jpeg_color followed by the warp (with ptabs: and the colour
// profile in between), byte for byte, with no BGR frame; g = the frames' width and height, which every descriptor has too.
// A chroma window's 4-byte load reaches at most 3 bytes past the last plane's last row: callers keep >= 4 readable bytes
// behind the last frame's planes (the pipeline's plane ring has 256).  ptabs / np / dst_profile_stride as warp_src_profile
// takes them.  Counted as CBV_K_WARP_YUV.
static inline WarpSrc warp_src_jpeg(const u8* planes, size_t plane_stride, const JpegDesc* descs, Geom g, const ProfileTabs* ptabs = nullptr, int np = 1,
                                    size_t dst_profile_stride = 0)
{
    WarpSrc s = {};
    s.kind = WarpSrc::JPEG;
    s.g = g;
    s.r.fmt = CBV_FMT_MJPEG;
    s.jpeg_planes = planes;
    s.jpeg_plane_stride = plane_stride;
    s.jpeg_descs = descs;
    s.ptabs = ptabs;
    s.np = np;
    s.dst_profile_stride = dst_profile_stride;
    return s;
}
// `batch` frames of `src` onto one dw x dh board (k_warp_one): from batch 8 on the source's many-frames form (warp_many,
// warp_gather.h: four frames per thread for most), one thread per pixel and frame below
int launch_warp(cbv_ctx* ctx, WarpSrc src, const double* Minv9, int dw, int dh, int rot180, u8* dst, int dst_stride, size_t dst_frame_stride,
                int batch, u32* zero_word = nullptr, u32* zero_word2 = nullptr);

void build_gaussian_q8_sigma(int k, double sigma, int* coef);
int launch_gray_gauss(cbv_ctx* ctx, const u8* src, int w, int h, int stride, int cn, const int* coef_dev, int k, u8* dst);
int launch_dilate_rect(cbv_ctx* ctx, const u8* src, int w, int h, int r, u8* dst);
int largest_contour_polygon(const uint8_t* img, int w, int h, double eps_frac, int32_t* pts, int cap, double* area_out, int* contour_len);
int board_corners_from_edges(const uint8_t* dilated, int w, int h, int32_t pts[8], int* n_contours);
int external_contours(const uint8_t* img, int w, int h, int32_t* pts, int pts_cap, int32_t* lens, double* areas, double* perims,
                      int contours_cap, int* n_contours, int* n_points);
int approx_poly_closed_pts(const int32_t* pts, int n, double eps, int32_t* out, int cap);
int launch_canny(cbv_ctx* ctx, const u8* src, int w, int h, int stride, int cn, int low, int high, u8* edges, DevBuf* scratch);

// squares
struct SquareDesc {
    int w, h;
    int src_off;   // byte offset of the ROI origin inside the source image / staging
    int stride;    // source row stride in bytes
    int cn;
    int plane_off; // element offset of this square's planes (gray/ref/mean/var)
    int mask_off;  // byte offset into the mask table
    int pad;
    // pixels of each region of the square's mask (centre disc, corners, four rings): they depend on the square's shape
    // only, so the host counts them once (square_region_counts) and the statistics kernels do not count them per frame
    u32 cnt[6];
    int pad2[2];
};
void square_region_counts(const u8* mask, int n, u32 cnt[6]);
// detect_all_pieces' per-square gate for the class API (one frame), evaluated by thread 0 of the statistics kernels:
// bit i of the sets = square i.  dflags == null: not a class-API launch.
struct DetectMasks {
    u64 has_ref = 0;     // pos in reference_squares
    u64 cached = 0;      // pos in cached_results
    u64 check = 0;       // pos in squares_to_check
    int check_given = 0; // squares_to_check is not None
    int use_delta = 1;
    double change_threshold = 25.0;
    u8* dflags = nullptr; // out, per square: the CBV_GATE_* bits
};
// the bits of a dflags byte as k_squares_pre5_stats packs them (k_squares.hip, "dm.dflags[blockIdx.x] =")
enum : u8 { CBV_GATE_CHANGED = 1, CBV_GATE_PROCESS = 2, CBV_GATE_EVALUATED = 4, CBV_GATE_STD_OK = 8 }; // (std >= 15: HoughCircles ran)
int launch_squares_preprocess(cbv_ctx* ctx, const u8* src, size_t src_frame_stride, const SquareDesc* descs, int n,
                              const int* coef_dev, int blur_k, u8* gray, size_t gray_frame_stride, int batch, int max_px = 0);
int launch_squares_stats(cbv_ctx* ctx, const SquareDesc* descs, int n, const u8* gray, size_t gray_frame_stride,
                         const u8* ref, const float* mean, const float* var, const u8* masks, float z_thresh,
                         cbv_sq_stats* out, int batch, u8* decisions = nullptr, int want_hough = 0, u32* hough_work = nullptr,
                         cbv_hough_result* hough_out = nullptr, const DetectMasks* dm = nullptr);

// HoughCircles per square (k_hough.hip).  off_* / max_* are filled by launch_hough.
struct HoughCfg {
    float dp;
    int canny_thr, acc_thr;
    double min_ratio, max_ratio;
    int maxw, maxh; // largest square of the set
    int min_dim;    // shortest side of any square of the set (0: not known, taken as 2)
    int gs, mw, mag_bytes; // padded row strides of the gray/map planes (bytes) and the magnitude plane (u16)
    int off_map, off_mag, off_acc, off_centres, off_bins, off_order, max_bins;
    int off_g, off_circ; // the gray plane; the candidate circles of P6 (over planes that are dead by then)
    int keep_acc;        // the accumulator outlives P6 (k_piece_sweep_hough re-reads it per setting): nothing may overlay it
    u32* overflow_count; // device counter of squares whose candidate list overflowed (CBV_HOUGH_OVERFLOW), or null
    int maxc;            // accumulator maxima / candidate circles kept per square (set by launch_hough)
    u32* retry;          // first pass: squares with more than `maxc` maxima are listed here (count, then frame << 8 | square)
                         // and done again by a second, rarely needed pass with room for every possible maximum
    int retry_frame_base; // added to the frame index of a listed square (the second pass may cover several first passes)
};
// `work` (may be null = every square of every frame): work[0] = number of items, work[1 + i] = frame << 8 | square,
// as k_squares_stats lists them; a found circle sets bit 0 of the square's `decisions` byte.
// `retry`: device list (count, then items) the first pass appends overflowing squares to (see HoughCfg::retry); the
// caller zeroes its count before the first pass that feeds it and runs launch_hough_second over it afterwards, with
// gray / out / decisions pointing at frame 0 of the list's frame numbering and `max_items` = its capacity.
int launch_hough(cbv_ctx* ctx, const SquareDesc* descs, int n, const u8* gray, size_t gray_frame_stride, HoughCfg cfg,
                 cbv_hough_result* out, u8* decisions, const u32* work, int batch, u32* retry, int retry_frame_base);
int launch_hough_second(cbv_ctx* ctx, const SquareDesc* descs, int n, const u8* gray, size_t gray_frame_stride, HoughCfg cfg,
                        cbv_hough_result* out, u8* decisions, const u32* retry, int max_items);
int launch_squares_pre5_stats(cbv_ctx* ctx, const u8* src, size_t src_frame_stride, const SquareDesc* descs, int n, u8* gray,
                              size_t gray_frame_stride, const float* mean, const float* var, const u8* masks, float z_thresh,
                              cbv_sq_stats* out, int batch, u8* decisions, int want_hough, u32* hough_work,
                              cbv_hough_result* hough_out, int max_px, const u8* ref = nullptr, const DetectMasks* dm = nullptr);
// (the statistics launchers' `var` argument is the SD plane: sqrt(var), written by these three next to the variance)
int launch_squares_calibrate(cbv_ctx* ctx, const SquareDesc* descs, int n, const u8* gray, float* mean, float* var, float* sd,
                             float init_var, const u8* select);
int launch_squares_ema(cbv_ctx* ctx, const SquareDesc* descs, int n, const u8* gray, float* mean, float* var, float* sd,
                       double alpha, const u8* select);
int launch_squares_refresh_sd(cbv_ctx* ctx, const SquareDesc* descs, const float* var, float* sd, int index);
int launch_squares_set_ref(cbv_ctx* ctx, const SquareDesc* descs, int n, const u8* gray, u8* ref, const u8* select);
int launch_squares_set_ref_mask(cbv_ctx* ctx, const SquareDesc* descs, int n, const u8* gray, u8* ref, u64 mask);

struct ScanParams {
    int n;               // squares
    int history_size;
    double min_presence;
    double change_threshold;
    int with_model; // z_count of the statistics is valid: classify LEVE / PARCIAL / TOTAL
    // _get_stable_detection's `sum(history) / len(history) >= min_presence` evaluated on the host in double for
    // every (len, sum): bit len * 8 + sum
    u64 stable_table;
    // mean(|diff|) > change_threshold as an exact integer test when the threshold is integral: sad > thr * n
    int thr_is_int;
    int thr_int;
};
struct ScanState {       // per square, device resident
    u32 has_ref, has_cache, cached_raw, hist_len, hist_bits;
};
int launch_scan_update_refs(cbv_ctx* ctx, const SquareDesc* descs, int n, const u8* gray, u8* ref, ScanState* state);
int launch_noise(cbv_ctx* ctx, const u64* changes, size_t stride_words, int count, cbv_noise_state* state, cbv_noise_result* out);
// Pinned host copy of a run's result records (`records` = the run's first slot there) and of HoughCircles' overflow
// counter, written by the run's last kernel beside the device copy: cbv_pipeline_results then waits and copies on the
// host instead of launching two device-to-host copies (~15 us of a 160 us frame).  All null: no mirror.
struct ResultMirror {
    cbv_frame_result* records = nullptr;
    const u32* over_src = nullptr;
    u32* over_dst = nullptr;
};
int launch_scan(cbv_ctx* ctx, const SquareDesc* descs, ScanParams sp, const u8* gray, size_t gray_frame_stride,
                const u8* decisions, u8* ref, ScanState* state, u8* flags, cbv_frame_result* results, int count,
                const u64* check = nullptr, cbv_noise_state* noise_state = nullptr, cbv_noise_result* noise_out = nullptr,
                ResultMirror mir = ResultMirror());

// The game session of a board (include/cbv.h, cbv_pipeline_session_begin; k_session.hip), device resident.  `resume` is
// the feedback inside a run: the walk stops behind an accepted move at frame t* of the run and stores t* + 1; the next
// round of the run scans and walks [resume, count) again from the state the move left, count + 1 = the run is finished.
struct SessionDev {
    cbv_session_config cfg;
    cbv_session_state st;
    int resume;
    cbv_session_move ring[CBV_SESSION_RING]; // record k of the session sits in ring[k % CBV_SESSION_RING]
};
int launch_scan_session(cbv_ctx* ctx, const SquareDesc* descs, ScanParams sp, const u8* gray, size_t gray_frame_stride,
                        const u8* decisions, u8* ref, ScanState* state, u8* flags, int count, const u64* check,
                        const SessionDev* ses, int first_round, u16* hist);
// packing, NoiseHandler and the session's walk of one round: frames [resume, count) of the run; `tones` = the frames' piece
// tones for the rules' tie-break (cfg.tone), or null
int launch_session_walk(cbv_ctx* ctx, const u8* flags, int n, cbv_frame_result* results, int count, cbv_noise_state* noise_state,
                        cbv_noise_result* noise_out, ResultMirror mir, SessionDev* ses, int first_round, cbv_session_radar* radar,
                        const cbv_tone_result* tones);
// a board event between two segments of a run (cbv_pipeline_session_sync): *ev is read now and travels with the launch
int launch_session_event(cbv_ctx* ctx, SessionDev* ses, const cbv_session_event* ev);
// the wave generator alone, `reps` times on the position at the head of *state_dev (tests, timing)
int launch_session_legal(cbv_ctx* ctx, const cbv_session_state* state_dev, u16* out_dev, int* n_dev, int reps);


// ---------------------------------------------------------------------------
// Several boards per frame (cbv_pipeline_add_board): the per-board stages of a chunk are ONE launch each for all boards,
// the board on the grid.  Every per-board input sits in this device table (one entry per board, board 0 = the pipeline
// itself); pointers are those of slot 0, the launches add their first slot.  The multi-board kernels rebind their
// arguments from the entry and then run the single-board bodies unchanged, so a board computes what a pipeline of its
// own computes.  HoughCircles' worklist and second-pass entries carry the board in their top bits (MB_BOARD_SHIFT).
// ---------------------------------------------------------------------------
// ChangeDetector's z-score statistics AND update_all_references over the frames of a run, in frame order (k_model_scan):
// the model after frame t is the input of frame t + 1.  mode = CBV_MODEL_FROZEN: nothing to do (the statistics kernels
// read the model themselves, `mean` / `sd` of the BoardDev), and so for a board that is not calibrated.
struct ModelScan {
    int mode;              // CBV_MODEL_*, FROZEN while the board is not calibrated
    float one_minus, alpha; // (1 - alpha) and alpha narrowed to float32 as launch_squares_ema does
    float z_thresh;
    float* mean;           // the model planes, read and written
    float* var;
    float* sd;
};

// The ChangeDetector stage's own blur (cbv_pipeline_set_change_blur): ChangeDetector._preprocess with a kernel other than the
// PieceDetector's 5 x 5.  cf[j] = the 8.8 fixed-point coefficient (build_gaussian_q8) j taps from the centre: the kernel is
// symmetric, k = 31 has 16 distinct ones.
struct ChangeBlur {
    int k; // odd, 1..31; 5 = the board reads the PieceDetector's planes and k_change_blur_stats does not run for it
    u32 cf[16];
};

#define MB_BOARD_SHIFT 29 // work item = board << 29 | frame << 8 | square: frames of a list < 2^21
struct BoardDev {
    // warp
    double Minv[9];
    int S, rot180, bw0, bh0;
    u8* warped;
    size_t warped_stride;
    // squares + HoughCircles
    const SquareDesc* descs;
    int n;
    int want_hough;              // cbv_pipeline_config::use_hough of the board
    const u8* masks;
    u8* gray;                    // [slot] planes, plane_total apart
    size_t plane_total;
    const float* mean;           // null until the board is calibrated
    const float* sd;
    float z_thresh;
    int pad0;
    cbv_sq_stats* stats;         // [slot][n]
    u8* dec;                     // [slot][CBV_MAX_SQUARES]
    cbv_hough_result* hough;     // [slot][CBV_MAX_SQUARES], null without use_hough
    HoughCfg hcfg[2];            // first / second pass, layout and maxc filled (hough_board_cfgs)
    // temporal scan + NoiseHandler
    ScanParams sp;
    u8* ref;
    ScanState* state;
    u8* flags;                   // [slot][CBV_MAX_SQUARES]
    cbv_frame_result* results;   // [slot]
    const u64* check;            // [slot]
    cbv_noise_state* noise_state;
    cbv_noise_result* noise;     // [slot]
    cbv_frame_result* mirror;    // pinned [slot] (ResultMirror of short runs)
    const u32* over_src;         // HoughCircles overflow counter, null without use_hough
    u32* over_dst;               // its pinned copy
    // per-frame background model update (cbv_pipeline_set_model_update): k_model_scan's arguments
    ModelScan ms;
    // the ChangeDetector planes (k_change_blur_stats writes them, calibrate and k_model_scan read them): `gray` itself
    // while cb.k == 5; cmean / csd = the model for the z-score statistics of a frozen, calibrated board with cb.k != 5
    // (`mean` / `sd` are null for such a board: k_squares_pre5_stats leaves the z statistics to k_change_blur_stats)
    u8* cgray;
    const float* cmean;
    const float* csd;
    ChangeBlur cb;
    // the board's colour profile (cbv_pipeline_set_profile): its device table in the profile modes (enabled = 0 in it: the
    // board's taps stay as they are), null otherwise; read by k_warp_boards of the sources with a profile
    const ProfileTabs* ptabs;
    // piece tones (cbv_pipeline_set_tones; k_tone.hip): all null while the board's tones are off, and k_piece_tone_boards
    // leaves the board at once
    cbv_tone_sums* tone_sums;        // [slot][CBV_MAX_SQUARES]
    cbv_tone_result* tone_res;       // [slot]
    const cbv_tone_model* tone_model; // the board's model (calibrated)
};
// k_piece_tone (k_tone.hip).  The sums of `batch` frames of n squares, explicit arguments: out[frame][CBV_MAX_SQUARES];
// only w, h, src_off, stride and cnt[0] of a descriptor are read, and cn must be 3
int launch_piece_tone(cbv_ctx* ctx, const u8* src, size_t src_frame_stride, const SquareDesc* descs, int n, cbv_tone_sums* out, int batch);
// ... and of every board of `tab` with tones on, then their records: two launches for all boards of a chunk
int launch_piece_tone_boards(cbv_ctx* ctx, const BoardDev* tab, int nb, int s0, int batch);
ScanParams scan_params(const cbv_pipeline_config& cfg, bool calibrated);
// per-pass HoughCfg of a board (layout and maxc as launch_hough / launch_hough_second set them); returns the LDS bytes
// of each pass, 0 when the squares cannot run (the single-board launchers' checks)
void hough_board_cfgs(HoughCfg base, HoughCfg out[2], size_t lds[2]);
// one launch each for `nb` boards; `tab` = device table, `s0` = slot of the chunk's (run's) frame 0 (the warp: k_warp_boards)
int launch_warp_mb(cbv_ctx* ctx, WarpSrc src, const BoardDev* tab, int nb, int maxS, int s0, int batch, u32* zero_word, u32* zero_word2);
// what launch_warp / launch_warp_mb hand a raw source with a profile (warp_src_raw_profile) to: k_warp_raw_profile.hip
int launch_warp_raw_profile(cbv_ctx* ctx, WarpSrc src, const double* Minv9, int dw, int dh, int rot180, u8* dst, int dst_stride,
                            size_t dst_frame_stride, int batch, u32* zero_word, u32* zero_word2);
int launch_warp_raw_profile_mb(cbv_ctx* ctx, WarpSrc src, const BoardDev* tab, int nb, int maxS, int s0, int batch, u32* zero_word, u32* zero_word2);
// ... a YUV source whose colour space is not 0, with or without a profile, to: k_warp_cs.hip
int launch_warp_cs(cbv_ctx* ctx, WarpSrc src, const double* Minv9, int dw, int dh, int rot180, u8* dst, int dst_stride, size_t dst_frame_stride, int batch,
                   u32* zero_word, u32* zero_word2);
int launch_warp_cs_mb(cbv_ctx* ctx, WarpSrc src, const BoardDev* tab, int nb, int maxS, int s0, int batch, u32* zero_word, u32* zero_word2);
// ... a developed mosaic (WarpSrc::deep), with a profile or without, to: k_warp_deep.hip
int launch_warp_deep(cbv_ctx* ctx, WarpSrc src, const double* Minv9, int dw, int dh, int rot180, u8* dst, int dst_stride, size_t dst_frame_stride, int batch,
                     u32* zero_word, u32* zero_word2);
int launch_warp_deep_mb(cbv_ctx* ctx, WarpSrc src, const BoardDev* tab, int nb, int maxS, int s0, int batch, u32* zero_word, u32* zero_word2);
// ... and a source of JPEG planes (warp_src_jpeg), with a profile or without: k_warp_jpeg.hip
int launch_warp_jpeg(cbv_ctx* ctx, WarpSrc src, const double* Minv9, int dw, int dh, int rot180, u8* dst, int dst_stride, size_t dst_frame_stride,
                     int batch, u32* zero_word, u32* zero_word2);
int launch_warp_jpeg_mb(cbv_ctx* ctx, WarpSrc src, const BoardDev* tab, int nb, int maxS, int s0, int batch, u32* zero_word, u32* zero_word2);
// The warp through the camera's lens model (lens_core.h): k_warp_lens.hip, and k_warp_lens_profile.hip for the raw and JPEG
// sources with a profile.  Every source kind has the table-driven form only: entry e of `tab` (device, ne entries) is one
// destination of the launch (k_warp_lens), a board of a pipeline or a profile of a colour sweep, and a single-frame call
// passes a table of one.  blockIdx.z = entry * nz + group of frames; the grid covers max_dw x max_dh.  Frame f of the launch goes
// to dst + (s0 + f) * frame_stride.  A profiled source reads the entries' own tables (ptabs), never WarpSrc::ptabs, which
// only says that the source is profiled.
struct LensBoard {
    double Minv[9];
    int dw, dh, bw0, rot180;
    u8* dst;
    size_t frame_stride;
    int stride, pad;
    const ProfileTabs* ptabs;
};
static inline LensBoard lens_board(const double* Minv9, int dw, int dh, int rot180, u8* dst, int stride, size_t frame_stride, const ProfileTabs* ptabs)
{
    LensBoard T;
    memset(&T, 0, sizeof(T));
    memcpy(T.Minv, Minv9, sizeof(T.Minv));
    int bh0;
    warp_block_shape(dw, dh, &T.bw0, &bh0);
    T.dw = dw, T.dh = dh, T.rot180 = rot180, T.dst = dst, T.stride = stride, T.frame_stride = frame_stride, T.ptabs = ptabs;
    return T;
}
int launch_warp_lens(cbv_ctx* ctx, WarpSrc src, const LensDev& lens, const LensBoard* tab, int ne, int max_dw, int max_dh, int s0, int batch,
                     u32* zero_word, u32* zero_word2);
// what launch_warp_lens hands a raw or JPEG source with a profile to: k_warp_lens_profile.hip
int launch_warp_lens_profile(cbv_ctx* ctx, WarpSrc src, const LensDev& lens, const LensBoard* tab, int ne, int max_dw, int max_dh, int s0, int batch,
                             u32* zero_word, u32* zero_word2);
// what launch_warp_lens hands a YUV source whose colour space is not 0 to: k_warp_lens_cs.hip
int launch_warp_lens_cs(cbv_ctx* ctx, WarpSrc src, const LensDev& lens, const LensBoard* tab, int ne, int max_dw, int max_dh, int s0, int batch,
                        u32* zero_word, u32* zero_word2);
// what launch_warp_lens hands a developed mosaic (WarpSrc::deep) to, with a profile or without: k_warp_lens_deep.hip
int launch_warp_lens_deep(cbv_ctx* ctx, WarpSrc src, const LensDev& lens, const LensBoard* tab, int ne, int max_dw, int max_dh, int s0, int batch,
                          u32* zero_word, u32* zero_word2);
// cbv_lens -> LensDev; CBV_ERR_ARG for a field that is not finite or a focal length that is not positive
int lens_checked(cbv_ctx* ctx, const cbv_lens* lens, LensDev* out, const char* who);
// warp_footprint through the lens: every border pixel of the destination through the full map, one more pixel of margin
bool warp_footprint_lens(const double* Minv, const LensDev* lens, int dw, int dh, int w, int h, PxRect* out);
// (n_squares: the boards' n_rois summed; the statistics launches choose 1024 or 256 lanes a square from n_squares * batch)
int launch_squares_pre5_stats_mb(cbv_ctx* ctx, const BoardDev* tab, int nb, int n_squares, int s0, int batch, int any_hough, u32* hough_work,
                                 int max_px);
int launch_hough_mb(cbv_ctx* ctx, const BoardDev* tab, int nb, int s0, const u32* work, int max_items, size_t lds, u32* retry,
                    int retry_frame_base, int pass);
int launch_scan_mb(cbv_ctx* ctx, const BoardDev* tab, int nb, int s0, int count, int mirrored);
int launch_model_scan(cbv_ctx* ctx, const BoardDev* tab, int nb, int s0, int count, int max_px);
// ChangeDetector._preprocess with the board's own kernel on `batch` warped frames, and (mean != null) the z-score fields of
// the records and the class bits of the decision bytes k_squares_pre5_stats wrote before it on the same stream
int launch_change_blur_stats(cbv_ctx* ctx, const u8* src, size_t src_frame_stride, const SquareDesc* descs, int n, u8* plane,
                             size_t plane_frame_stride, const float* mean, const float* sd, float z_thresh, cbv_sq_stats* stats,
                             int batch, u8* decisions, const ChangeBlur& cb, int max_px);
int launch_change_blur_stats_mb(cbv_ctx* ctx, const BoardDev* tab, int nb, int n_squares, int s0, int batch, int max_px);

// The ChangeDetector sensitivity sweep (cbv_pipeline_sweep, k_sweep.hip).  A setting as the kernels read it: the float32
// casts of cbv_pipeline_configure and the setting's place in the caller's list; the call sorts them by blur kernel.
struct SweepSet {
    float zt, ivf;
    u32 index;
};
#define SWEEP_HIST_WORDS (CBV_MAX_SQUARES * 256) // u16 elements of one (frame, kernel): [square][d]
// |gray - calib| histograms of `batch` warped frames under one blur kernel: out[frame * out_frame_stride + square * 256 + d]
// (u16 elements), `calib` = the plane set (SquareDesc::plane_off) of the calibration frame under the same kernel
int launch_change_hist(cbv_ctx* ctx, const u8* src, size_t src_frame_stride, const SquareDesc* descs, int n, const u8* calib, u16* out,
                       size_t out_frame_stride, int batch, const ChangeBlur& cb, int max_px);
// every setting on `frames` frames: hist[frame][kernel][square][d]; sets sorted by kernel, k_begin[nk + 1] = first setting
// of each kernel; rec (may be null) = [setting index][rec_stride] records, this launch's frames in columns 0..frames - 1;
// sums (may be null) = [setting index], added to
int launch_sweep_eval(cbv_ctx* ctx, const u16* hist, int nk, const SquareDesc* descs, int n, const SweepSet* sets, const int* k_begin,
                      int max_per_k, int frames, cbv_sweep_record* rec, int rec_stride, cbv_sweep_summary* sums);

// The PieceDetector settings sweep (cbv_pipeline_piece_sweep, k_piece_sweep.hip).  A setting as the kernels read it: the
// casts of hough_cfg and the setting's place in the caller's list; the call sorts them so that settings which share the
// Canny front end, and then the accumulator, follow each other.
struct PieceSet {
    float dp;
    int canny_thr, acc_thr;
    u32 index;
    double min_ratio, max_ratio;
};
struct PieceChoice; // piece_sweep_core.h
// LDS bytes of k_piece_sweep_hough for *cfg (maxw, maxh, dp and the ratios set; layout and maxc are filled in):
// the second pass's layout plus the step table at *off_steps
size_t piece_sweep_layout(HoughCfg* cfg, int* off_steps);
// HoughCircles and the pick for every (setting, frame, square): gray / stats = frame 0 of the launch, out[(index *
// out_frames + frame) * CBV_MAX_SQUARES + square]; cfg.dp = the smallest dp, the ratios = the widest radius span of the sets
int launch_piece_sweep_hough(cbv_ctx* ctx, const SquareDesc* descs, int n, const u8* gray, size_t gray_frame_stride, const cbv_sq_stats* stats,
                             HoughCfg cfg, const PieceSet* sets, int ns, int frames, PieceChoice* out, int out_frames);
// decision, history and records of `frames` frames in order: hist[ns][CBV_MAX_SQUARES] and sums[ns] are read and updated,
// rec (may be null) = [setting][rec_stride], expected (may be null) = [frames]; stat_stride = 0: stats[frames][n] serve every
// setting; otherwise setting s reads stats[s * stat_stride + frame][n]
int launch_piece_sweep_eval(cbv_ctx* ctx, const SquareDesc* descs, int n, const cbv_sq_stats* stats, const PieceChoice* choices, int choice_frames,
                            int frames, int ns, const u64* expected, u32* hist, cbv_piece_sweep_record* rec, int rec_stride,
                            cbv_piece_sweep_summary* sums, int stat_stride = 0);

// ---------------------------------------------------------------------------
// Helpers of the host entry points (cbv_api.cpp, cbv_squares.cpp) that the device-resident pipeline (cbv_pipeline*.cpp) shares
// ---------------------------------------------------------------------------
#define RC(x)             \
    do {                  \
        int rc__ = (x);   \
        if (rc__) return rc__; \
    } while (0)

// tightly packed BGR frames, each frame rounded to 256 bytes
static inline Geom tight_geom(int w, int h)
{
    Geom g;
    g.w = w;
    g.h = h;
    g.stride = w * 3;
    g.frame_stride = ((size_t)w * 3 * h + 255) & ~(size_t)255;
    return g;
}

struct SmallLayout {
    u32* aux;
    u8* luts;
    u32* packed; // CLAHE corner words (k_clahe_lut -> k_clahe_apply), null when not reserved
    u8* norm_lut;
    // The buffer's tag says which (tiles, batch) layout of `aux` is known to be as k_reset_aux leaves it: enhance_dev's own
    // kernels restore that state as they go (launch_clahe_lut, self_clean), so a pass over the same layout needs no reset
    // launch.  Everything else that writes `aux` leaves the tag 0 (aux_dirty).
    DevBuf* owner;
};
int small_layout(cbv_ctx* ctx, DevBuf* buf, int tiles, int batch, SmallLayout* L, int tiles_x = 0, int tiles_y = 0);
int enhance_dev(cbv_ctx* ctx, const u8* src, u8* A, u8* B, Geom g, const cbv_enhance_params* P, SmallLayout S, int batch,
                bool fold_norm, u8** result, NormSrc* norm, const PxRect* region = nullptr, u8* C = nullptr);
bool warp_footprint(const double* Minv, int dw, int dh, int w, int h, PxRect* out);
int check_params(cbv_ctx* ctx, const cbv_enhance_params* P);
int rows_h2d(cbv_ctx* ctx, void* dst, const u8* src, int stride, int wbytes, int h);
int hough_params_check(cbv_ctx* ctx, const cbv_hough_params* prm);
int hough_cfg(cbv_ctx* ctx, const cbv_hough_params* prm, const std::vector<SquareDesc>& descs, HoughCfg* hc);
// the square table of n squares ws[i] x hs[i]: descriptors with w, h and the plane / mask offsets (each plane rounded to
// 16 B), the piece masks and their region counts; returns the bytes of one plane set
size_t square_table(const int* ws, const int* hs, int n, std::vector<SquareDesc>* descs, std::vector<u8>* masks);

// Baseline JPEG decode (k_jpeg.hip; the bodies and the descriptor types are jpeg_core.h's).  `nframes` streams, frame f's
// bytes at data + f * data_stride, decoded by restart interval: ioff[nframes + 1] = the prefix sums of the frames' interval
// counts, mpos[ioff[nframes]] = scratch for the restart markers' positions.  Outputs of frame f: coef + f * coef_stride
// (int16 elements; a multiple of 64), planes + f * plane_stride (a multiple of 8), bgr + f * bgr_frame_stride, status[f].
struct JpegDesc;
struct JpegTables;
struct JpegBatch {
    const u8* data;
    size_t data_stride;
    const JpegDesc* descs;
    const JpegTables* tables; // the table sets JpegDesc::table_set names
    const u32* ioff;
    u32* mpos;
    int* nfound;              // [nframes] scratch: restart markers found, at most the frame's intervals - 1
    int* status;              // [nframes] JP_ST_* bits
    int16_t* coef;
    size_t coef_stride;
    u8* planes;
    size_t plane_stride;
    u8* bgr;
    int bgr_stride;
    size_t bgr_frame_stride;
    int nframes;
    // the piece path (k_jpeg_pieces): frames without DRI go it when piece_bytes (a multiple of 4) is not 0, and with
    // `segments` frames with DRI do too, every restart interval cut into pieces.  Frame f's scratch is pieces + f * piece_stride:
    // JPEG_PIECE_WORDS u32 (one more with `segments`: the piece's segment) for each of its pieces, of which it may have
    // piece_cap; and with `segments`, segs + f * seg_stride: JPEG_SEG_WORDS u32 for each of its intervals and one more.
    u32 piece_bytes;
    u32* pieces;
    size_t piece_stride;
    u32 piece_cap;
    int segments;
    u32* segs;
    size_t seg_stride;
    u32* stats;               // [nframes][3]: pieces, rounds, settled in round 0; zeros for a frame decoded by interval
};
// (JPEG_PIECE_WORDS, JPEG_SEG_WORDS, jpeg_piece_words and jpeg_seg_words: frame_plan.h)
// zeroes coef, status, nfound, stats and the segment scratch, then the kernels on ctx->stream; total_intervals = ioff[nframes],
// any_dri / any_pieces: a frame has restart intervals / goes the piece path, max_blocks = the largest plane_total / 64,
// max_w x max_h = the largest frame
// B.bgr null: the decode stops at the planes (k_jpeg_color is not launched)
int launch_jpeg_decode(cbv_ctx* ctx, const JpegBatch& B, u32 total_intervals, int any_dri, int any_pieces, u32 max_blocks, int max_w, int max_h);
// k_jpeg_color alone: the BGR frames of B.nframes decoded frames from B.descs and B.planes
int launch_jpeg_color(cbv_ctx* ctx, const JpegBatch& B, int max_w, int max_h);
