// C-ABI of libcbv_hip.so (include/cbv.h): the host-buffer stage entry points, which enter through CBV_ENTER_DRAINED
// (the context, the per-square detector and the device-resident pipeline have translation units of their own).
#include <math.h>
#include <string.h>

#include <algorithm>

#include "cbv_internal.h"

static int check_img(cbv_ctx* ctx, const void* p, int w, int h, int stride, int cn, const char* what)
{
    if (!ctx) return cbv_fail(nullptr, CBV_ERR_ARG, "%s: ctx is null", what);
    if (!p || w <= 0 || h <= 0 || stride < w * cn) return cbv_fail(ctx, CBV_ERR_ARG, "%s: bad image arguments (w=%d h=%d stride=%d)", what, w, h, stride);
    if ((size_t)w * h > (size_t)1 << 28) return cbv_fail(ctx, CBV_ERR_ARG, "%s: image too large", what);
    return CBV_OK;
}

// rows between a host image (any row stride) and a tight device image, asynchronous.  Tight host rows travel as ONE
// linear copy: the 2-D entry point takes a slower path even when width == pitch (a 1080p frame to pageable memory:
// 365 us against 119 us, tools/ubench_copy.hip).
int rows_h2d(cbv_ctx* ctx, void* dst, const u8* src, int stride, int wbytes, int h)
{
    if (stride == wbytes) CBV_HIP(ctx, hipMemcpyAsync(dst, src, (size_t)wbytes * h, hipMemcpyHostToDevice, ctx->stream));
    else CBV_HIP(ctx, hipMemcpy2DAsync(dst, wbytes, src, stride, wbytes, h, hipMemcpyHostToDevice, ctx->stream));
    return CBV_OK;
}

static int rows_d2h(cbv_ctx* ctx, u8* dst, int stride, const void* src, int wbytes, int h)
{
    if (stride == wbytes) CBV_HIP(ctx, hipMemcpyAsync(dst, src, (size_t)wbytes * h, hipMemcpyDeviceToHost, ctx->stream));
    else CBV_HIP(ctx, hipMemcpy2DAsync(dst, stride, src, wbytes, wbytes, h, hipMemcpyDeviceToHost, ctx->stream));
    return CBV_OK;
}

static int upload(cbv_ctx* ctx, DevBuf* dst, const u8* src, int wbytes, int h, int stride)
{
    int rc = dev_ensure(ctx, dst, (size_t)wbytes * h + 256);
    if (rc) return rc;
    return rows_h2d(ctx, dst->p, src, stride, wbytes, h);
}

static int download(cbv_ctx* ctx, const void* src, u8* dst, int wbytes, int h, int stride)
{
    int rc = rows_d2h(ctx, dst, stride, src, wbytes, h);
    if (rc) return rc;
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

static unsigned long long aux_clean_tag(int tiles, int batch) { return (1ull << 63) | ((unsigned long long)tiles << 32) | (unsigned)batch; }
static int aux_reset(cbv_ctx* ctx, const SmallLayout& S, int tiles, int batch) // reset for a stand-alone stage
{
    S.owner->tag = 0;
    return launch_reset_aux(ctx, S.aux, tiles, batch);
}

// tiles_x / tiles_y > 0 also reserve the packed CLAHE corner words ([batch][tiles_y + 1][tiles_x + 1][256] u32)
int small_layout(cbv_ctx* ctx, DevBuf* buf, int tiles, int batch, SmallLayout* L, int tiles_x, int tiles_y)
{
    size_t aux_b = aux_words(tiles) * 4 * batch;
    aux_b = (aux_b + 255) & ~(size_t)255;
    size_t lut_b = ((size_t)tiles * 256 * batch + 255) & ~(size_t)255;
    size_t nl_b = ((size_t)256 * batch + 255) & ~(size_t)255;
    size_t pk_b = (size_t)(tiles_x + 1) * (tiles_y + 1) * 1024 * batch;
    if (tiles_x <= 0 || tiles_y <= 0) pk_b = 0;
    int rc = dev_ensure(ctx, buf, aux_b + lut_b + nl_b + pk_b);
    if (rc) return rc;
    L->owner = buf;
    L->aux = (u32*)buf->p;
    L->luts = (u8*)buf->p + aux_b;
    L->norm_lut = (u8*)buf->p + aux_b + lut_b;
    L->packed = pk_b ? (u32*)((u8*)buf->p + aux_b + lut_b + nl_b) : nullptr;
    return CBV_OK;
}

extern "C" int cbv_apply_color_profile(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride,
                                       const cbv_color_profile* profile, uint8_t* out, int out_stride)
{
    RC(check_img(ctx, bgr, w, h, stride, 3, "cbv_apply_color_profile"));
    if (!out || !profile) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_apply_color_profile: null argument");
    CBV_ENTER_DRAINED(ctx);
    RC(upload(ctx, &ctx->in, bgr, w * 3, h, stride));
    if (!profile->enabled) return CBV_DONE(download(ctx, ctx->in.p, out, w * 3, h, out_stride)); // `{}` profile: identity
    RC(ctx_set_profile(ctx, profile));
    Geom g = tight_geom(w, h);
    RC(dev_ensure(ctx, &ctx->a, g.frame_stride));
    SmallLayout S;
    RC(small_layout(ctx, &ctx->small, 1, 1, &S));
    S.owner->tag = 0;
    ClaheGeom cg = clahe_geom(w, h, 0.0, 1, 1); // one tile = whole image; only used for the traversal
    RC(launch_color_lab_hist(ctx, (const u8*)ctx->in.p, (u8*)ctx->a.p, S.aux, g, cg, 1, 1, 0));
    return CBV_DONE(download(ctx, ctx->a.p, out, w * 3, h, out_stride));
}

extern "C" int cbv_correct_lighting(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, double clip_limit,
                                    int tiles_x, int tiles_y, uint8_t* out, int out_stride)
{
    RC(check_img(ctx, bgr, w, h, stride, 3, "cbv_correct_lighting"));
    if (!out || tiles_x <= 0 || tiles_y <= 0 || tiles_x > 64 || tiles_y > 64) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_correct_lighting: bad arguments");
    CBV_ENTER_DRAINED(ctx);
    RC(upload(ctx, &ctx->in, bgr, w * 3, h, stride));
    Geom g = tight_geom(w, h);
    RC(dev_ensure(ctx, &ctx->a, g.frame_stride));
    RC(dev_ensure(ctx, &ctx->b, g.frame_stride));
    ClaheGeom cg = clahe_geom(w, h, clip_limit, tiles_x, tiles_y);
    int tiles = tiles_x * tiles_y;
    SmallLayout S;
    RC(small_layout(ctx, &ctx->small, tiles, 1, &S, tiles_x, tiles_y));
    RC(aux_reset(ctx, S, tiles, 1));
    RC(launch_color_lab_hist(ctx, (const u8*)ctx->in.p, (u8*)ctx->a.p, S.aux, g, cg, 1, 0, 1));
    RC(launch_clahe_lut(ctx, S.aux, S.luts, cg, 1, S.packed));
    RC(launch_clahe_apply(ctx, (const u8*)ctx->a.p, S.packed, (u8*)ctx->b.p, g, cg, 1));
    return CBV_DONE(download(ctx, ctx->b.p, out, w * 3, h, out_stride));
}

extern "C" int cbv_clahe_apply(cbv_ctx* ctx, const uint8_t* gray, int w, int h, int stride, double clip_limit, int tiles_x,
                               int tiles_y, uint8_t* out, int out_stride)
{
    RC(check_img(ctx, gray, w, h, stride, 1, "cbv_clahe_apply"));
    if (!out || tiles_x <= 0 || tiles_y <= 0 || tiles_x > 64 || tiles_y > 64) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_clahe_apply: bad arguments");
    CBV_ENTER_DRAINED(ctx);
    RC(upload(ctx, &ctx->in, gray, w, h, stride));
    RC(dev_ensure(ctx, &ctx->a, ((size_t)w * h + 255) & ~(size_t)255));
    ClaheGeom cg = clahe_geom(w, h, clip_limit, tiles_x, tiles_y);
    SmallLayout S;
    RC(small_layout(ctx, &ctx->small, tiles_x * tiles_y, 1, &S));
    S.owner->tag = 0;
    RC(launch_clahe_gray(ctx, (const u8*)ctx->in.p, w, h, w, cg, S.aux, S.luts, (u8*)ctx->a.p));
    return CBV_DONE(download(ctx, ctx->a.p, out, w, h, out_stride));
}

extern "C" int cbv_reduce_noise(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, int d, double sigma_color,
                                double sigma_space, uint8_t* out, int out_stride)
{
    RC(check_img(ctx, bgr, w, h, stride, 3, "cbv_reduce_noise"));
    if (!out) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_reduce_noise: out is null");
    CBV_ENTER_DRAINED(ctx);
    RC(ctx_set_bilateral(ctx, d, sigma_color, sigma_space));
    RC(upload(ctx, &ctx->in, bgr, w * 3, h, stride));
    Geom g = tight_geom(w, h);
    RC(dev_ensure(ctx, &ctx->a, g.frame_stride));
    RC(launch_bilateral(ctx, (const u8*)ctx->in.p, (u8*)ctx->a.p, g, 1));
    return CBV_DONE(download(ctx, ctx->a.p, out, w * 3, h, out_stride));
}

// Not in include/cbv.h: for tests/test_gpu_bilateral_walk.py.  cbv_reduce_noise on `n` tightly packed w x h frames in ONE
// launch, as the pipeline's chunks run it: the batched forms of k_bilateral are selected by the launch's tile count.
// cbv_reduce_noise itself launches one frame, and frames stacked into one tall image are no substitute: every frame
// has its own REFLECT_101 border and its own ragged bottom tile row.  Buffers as in cbv_reduce_noise (the input with
// 256 bytes of slack for the dword prefetch, the output without).
extern "C" CBV_API int cbv_debug_reduce_noise_batch(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int n, int d, double sigma_color,
                                                    double sigma_space, uint8_t* out)
{
    RC(check_img(ctx, bgr, w, h, w * 3, 3, "cbv_debug_reduce_noise_batch"));
    if (!out || n < 1 || n > 4096) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_debug_reduce_noise_batch: bad arguments");
    CBV_ENTER_DRAINED(ctx);
    RC(ctx_set_bilateral(ctx, d, sigma_color, sigma_space));
    const Geom g = tight_geom(w, h);
    const size_t fbytes = (size_t)w * 3 * h;
    RC(dev_ensure(ctx, &ctx->in, g.frame_stride * n + 256));
    RC(dev_ensure(ctx, &ctx->a, g.frame_stride * n));
    CBV_HIP(ctx, hipMemcpy2DAsync(ctx->in.p, g.frame_stride, bgr, fbytes, fbytes, n, hipMemcpyHostToDevice, ctx->stream));
    RC(launch_bilateral(ctx, (const u8*)ctx->in.p, (u8*)ctx->a.p, g, n));
    CBV_HIP(ctx, hipMemcpy2DAsync(out, fbytes, ctx->a.p, g.frame_stride, fbytes, n, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_DONE(CBV_OK);
}

extern "C" int cbv_sharpen(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, const float* kernel9, uint8_t* out,
                           int out_stride)
{
    RC(check_img(ctx, bgr, w, h, stride, 3, "cbv_sharpen"));
    if (!out || !kernel9) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_sharpen: null argument");
    CBV_ENTER_DRAINED(ctx);
    RC(upload(ctx, &ctx->in, bgr, w * 3, h, stride));
    Geom g = tight_geom(w, h);
    RC(dev_ensure(ctx, &ctx->a, g.frame_stride));
    SmallLayout S;
    RC(small_layout(ctx, &ctx->small, 1, 1, &S));
    RC(aux_reset(ctx, S, 1, 1));
    RC(launch_sharpen(ctx, (const u8*)ctx->in.p, (u8*)ctx->a.p, S.aux, 1, g, kernel9, 1));
    return CBV_DONE(download(ctx, ctx->a.p, out, w * 3, h, out_stride));
}

int launch_minmax(cbv_ctx* ctx, const u8* src, u32* aux, int tiles, Geom g, int batch);

extern "C" int cbv_normalize_intensity(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, uint8_t* out,
                                       int out_stride)
{
    RC(check_img(ctx, bgr, w, h, stride, 3, "cbv_normalize_intensity"));
    if (!out) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_normalize_intensity: out is null");
    CBV_ENTER_DRAINED(ctx);
    RC(upload(ctx, &ctx->in, bgr, w * 3, h, stride));
    Geom g = tight_geom(w, h);
    RC(dev_ensure(ctx, &ctx->a, g.frame_stride));
    SmallLayout S;
    RC(small_layout(ctx, &ctx->small, 1, 1, &S));
    RC(aux_reset(ctx, S, 1, 1));
    RC(launch_minmax(ctx, (const u8*)ctx->in.p, S.aux, 1, g, 1));
    RC(launch_normalize(ctx, (const u8*)ctx->in.p, (u8*)ctx->a.p, norm_from_minmax(S.aux, 1), g, 1));
    return CBV_DONE(download(ctx, ctx->a.p, out, w * 3, h, out_stride));
}

extern "C" int cbv_prepare_analysis(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, uint8_t* gray,
                                    int gray_stride, uint8_t* binary, int binary_stride, int* otsu_threshold)
{
    RC(check_img(ctx, bgr, w, h, stride, 3, "cbv_prepare_analysis"));
    if (!gray || !binary) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_prepare_analysis: null output");
    CBV_ENTER_DRAINED(ctx);
    RC(upload(ctx, &ctx->in, bgr, w * 3, h, stride));
    Geom g = tight_geom(w, h);
    size_t plane = ((size_t)w * h + 255) & ~(size_t)255;
    RC(dev_ensure(ctx, &ctx->a, plane * 3));
    u8* dgray = (u8*)ctx->a.p;
    u8* dblur = dgray + plane;
    u8* dbin = dblur + plane;
    SmallLayout S;
    RC(small_layout(ctx, &ctx->small, 1, 1, &S));
    RC(aux_reset(ctx, S, 1, 1));
    RC(launch_gray_blur_hist(ctx, (const u8*)ctx->in.p, dgray, dblur, S.aux, 1, g, 1));
    RC(launch_otsu(ctx, S.aux, 1, w * h, 1));
    RC(launch_threshold(ctx, dblur, dbin, S.aux, 1, w, h, 1));
    RC(rows_d2h(ctx, gray, gray_stride, dgray, w, h));
    RC(rows_d2h(ctx, binary, binary_stride, dbin, w, h));
    u32 t = 0;
    CBV_HIP(ctx, hipMemcpyAsync(&t, S.aux + (size_t)1 * 256 + 2 + 256, 4, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (otsu_threshold) *otsu_threshold = (int)t;
    return CBV_DONE(CBV_OK);
}

extern "C" int cbv_canny(cbv_ctx* ctx, const uint8_t* img, int w, int h, int stride, int cn, double threshold1, double threshold2,
                         uint8_t* edges, int edges_stride)
{
    RC(check_img(ctx, img, w, h, stride, cn, "cbv_canny"));
    if (!edges || (cn != 1 && cn != 3)) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_canny: null output or unsupported channel count");
    CBV_ENTER_DRAINED(ctx);
    RC(upload(ctx, &ctx->in, img, w * cn, h, stride));
    // cv::Canny: thresholds are ordered, then floored (L1 gradient)
    double lo = threshold1 < threshold2 ? threshold1 : threshold2, hi = threshold1 < threshold2 ? threshold2 : threshold1;
    const int low = (int)floor(lo), high = (int)floor(hi);
    size_t plane = ((size_t)w * h + 255) & ~(size_t)255;
    RC(dev_ensure(ctx, &ctx->a, plane));
    RC(launch_canny(ctx, (const u8*)ctx->in.p, w, h, w * cn, cn, low, high, (u8*)ctx->a.p, &ctx->b));
    return CBV_DONE(download(ctx, ctx->a.p, edges, w, h, edges_stride));
}

extern "C" int cbv_board_corners_from_edges(const uint8_t* edges, int w, int h, int stride, int32_t* pts8, int* n_contours)
{
    if (!edges || !pts8 || w <= 0 || h <= 0 || stride < w) return CBV_ERR_ARG;
    std::vector<u8> tight((size_t)w * h);
    for (int y = 0; y < h; y++) memcpy(tight.data() + (size_t)y * w, edges + (size_t)y * stride, (size_t)w);
    return board_corners_from_edges(tight.data(), w, h, pts8, n_contours);
}

extern "C" int cbv_largest_contour_polygon(const uint8_t* edges, int w, int h, int stride, double eps_frac, int32_t* pts, int cap,
                                           double* area, int* contour_len)
{
    if (!edges || !pts || w <= 0 || h <= 0 || stride < w || cap <= 0) return CBV_ERR_ARG;
    std::vector<u8> tight((size_t)w * h);
    for (int y = 0; y < h; y++) memcpy(tight.data() + (size_t)y * w, edges + (size_t)y * stride, (size_t)w);
    return largest_contour_polygon(tight.data(), w, h, eps_frac, pts, cap, area, contour_len);
}

extern "C" int cbv_find_chessboard_corners(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, int32_t* pts8,
                                           uint8_t* dilated_out, int dilated_stride)
{
    RC(check_img(ctx, bgr, w, h, stride, 3, "cbv_find_chessboard_corners"));
    if (!pts8) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_find_chessboard_corners: null output");
    CBV_ENTER_DRAINED(ctx);
    RC(upload(ctx, &ctx->in, bgr, w * 3, h, stride));
    const size_t plane = ((size_t)w * h + 255) & ~(size_t)255;
    RC(dev_ensure(ctx, &ctx->a, plane * 3 + 256));
    u8* blur = (u8*)ctx->a.p;
    u8* edges = blur + plane;
    u8* dil = edges + plane;
    int coef[16] = {0};
    build_gaussian_q8_sigma(7, 1.0, coef);                      // cv2.GaussianBlur(gray, (7, 7), 1)
    int* coef_dev = (int*)(dil + plane);
    CBV_HIP(ctx, hipMemcpyAsync(coef_dev, coef, sizeof(int) * 16, hipMemcpyHostToDevice, ctx->stream));
    RC(launch_gray_gauss(ctx, (const u8*)ctx->in.p, w, h, w * 3, 3, coef_dev, 7, blur));
    RC(launch_canny(ctx, blur, w, h, w, 1, 30, 100, edges, &ctx->b)); // cv2.Canny(blur, 30, 100)
    RC(launch_dilate_rect(ctx, edges, w, h, 6, dil));           // three 5x5 dilations = one 13x13
    std::vector<u8> host((size_t)w * h);
    CBV_HIP(ctx, hipMemcpyAsync(host.data(), dil, (size_t)w * h, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (dilated_out)
        for (int y = 0; y < h; y++) memcpy(dilated_out + (size_t)y * dilated_stride, host.data() + (size_t)y * w, (size_t)w);
    int n_contours = 0;
    return CBV_DONE(board_corners_from_edges(host.data(), w, h, pts8, &n_contours));
}

// calibration / inspection: the stages of cbv_find_chessboard_corners one at a time
static bool gauss_k_ok(int k) { return k >= 1 && k <= 15 && (k & 1); }

extern "C" int cbv_gaussian_q8(int k, double sigma, int32_t* coef)
{
    if (!coef || !gauss_k_ok(k)) return CBV_ERR_ARG;
    int q[16] = {0};
    build_gaussian_q8_sigma(k, sigma, q);
    for (int i = 0; i < k; i++) coef[i] = q[i];
    return CBV_OK;
}

extern "C" int cbv_gaussian_blur(cbv_ctx* ctx, const uint8_t* img, int w, int h, int stride, int cn, int k, double sigma,
                                 uint8_t* out, int out_stride, int32_t* coef_out)
{
    RC(check_img(ctx, img, w, h, stride, cn, "cbv_gaussian_blur"));
    if (!out || out_stride < w || (cn != 1 && cn != 3)) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_gaussian_blur: bad output or unsupported channel count");
    if (!gauss_k_ok(k)) return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "Gaussian kernel size %d is not supported (odd, <= 15)", k);
    CBV_ENTER_DRAINED(ctx);
    RC(upload(ctx, &ctx->in, img, w * cn, h, stride));
    const size_t plane = ((size_t)w * h + 255) & ~(size_t)255;
    RC(dev_ensure(ctx, &ctx->a, plane + 256));
    int coef[16] = {0};
    build_gaussian_q8_sigma(k, sigma, coef);
    if (coef_out)
        for (int i = 0; i < k; i++) coef_out[i] = coef[i];
    int* coef_dev = (int*)((u8*)ctx->a.p + plane);
    CBV_HIP(ctx, hipMemcpyAsync(coef_dev, coef, sizeof(int) * 16, hipMemcpyHostToDevice, ctx->stream));
    RC(launch_gray_gauss(ctx, (const u8*)ctx->in.p, w, h, w * cn, cn, coef_dev, k, (u8*)ctx->a.p));
    return CBV_DONE(download(ctx, ctx->a.p, out, w, h, out_stride));
}

extern "C" int cbv_dilate_rect(cbv_ctx* ctx, const uint8_t* img, int w, int h, int stride, int r, uint8_t* out, int out_stride)
{
    RC(check_img(ctx, img, w, h, stride, 1, "cbv_dilate_rect"));
    if (!out || out_stride < w) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_dilate_rect: bad output");
    if (r < 0 || r > 7) return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "dilation radius %d is not supported (<= 7)", r);
    CBV_ENTER_DRAINED(ctx);
    RC(upload(ctx, &ctx->in, img, w, h, stride));
    RC(dev_ensure(ctx, &ctx->a, ((size_t)w * h + 255) & ~(size_t)255));
    RC(launch_dilate_rect(ctx, (const u8*)ctx->in.p, w, h, r, (u8*)ctx->a.p));
    return CBV_DONE(download(ctx, ctx->a.p, out, w, h, out_stride));
}

extern "C" int cbv_external_contours(const uint8_t* img, int w, int h, int stride, int32_t* pts, int pts_cap, int32_t* lens,
                                     double* areas, double* perims, int contours_cap, int* n_contours, int* n_points)
{
    if (!img || !n_contours || !n_points || w <= 0 || h <= 0 || stride < w || pts_cap < 0 || contours_cap < 0) return CBV_ERR_ARG;
    if ((pts_cap > 0 && !pts) || (contours_cap > 0 && (!lens || !areas || !perims))) return CBV_ERR_ARG;
    if ((size_t)w * h > (size_t)1 << 28) return CBV_ERR_ARG;
    std::vector<u8> tight((size_t)w * h);
    for (int y = 0; y < h; y++) memcpy(tight.data() + (size_t)y * w, img + (size_t)y * stride, (size_t)w);
    return external_contours(tight.data(), w, h, pts, pts_cap, lens, areas, perims, contours_cap, n_contours, n_points);
}

extern "C" int cbv_approx_poly_closed(const int32_t* pts, int n, double eps, int32_t* out, int cap)
{
    if (!pts || n <= 0 || cap < 0 || (cap > 0 && !out) || !(eps >= 0)) return CBV_ERR_ARG;
    return approx_poly_closed_pts(pts, n, eps, out, cap);
}

// enhancement chain on device buffers: src -> (A, B ping-pong) ; result pointer returned.
// When `fold_norm` the final normalize pass is skipped and the caller applies S.norm_lut downstream.
static PxRect px_dilate(PxRect r, int d, Geom g)
{
    PxRect o = {r.x0 - d, r.y0 - d, r.x1 + d, r.y1 + d};
    o.x0 = o.x0 < 0 ? 0 : o.x0;
    o.y0 = o.y0 < 0 ? 0 : o.y0;
    o.x1 = o.x1 > g.w ? g.w : o.x1;
    o.y1 = o.y1 > g.h ? g.h : o.y1;
    return o;
}

// `region` (with a third buffer C, and only when the caller folds normalize into its own gather): the consumer samples
// just these pixels of the enhanced frame; see "Region-limited enhancement" in cbv_internal.h.
// `norm`: where the consumer of a fold_norm result finds cv2.normalize's byte map (NormSrc).
int enhance_dev(cbv_ctx* ctx, const u8* src, u8* A, u8* B, Geom g, const cbv_enhance_params* P, SmallLayout S, int batch,
                bool fold_norm, u8** result, NormSrc* norm, const PxRect* region, u8* C)
{
    ClaheGeom cg = clahe_geom(g.w, g.h, P->clahe_clip_limit, P->tiles_x, P->tiles_y);
    int tiles = P->tiles_x * P->tiles_y;
    if (!S.packed) return cbv_fail(ctx, CBV_ERR_STATE, "enhance_dev: the small-buffer layout lacks the packed CLAHE words");
    // histograms zero, [min, max] = [255, 0]: by a launch the first time this layout of the buffer is used, by the previous
    // pass's k_clahe_lut afterwards (SmallLayout::owner).  The tag stays 0 until every launch of this pass is enqueued.
    const unsigned long long clean = aux_clean_tag(tiles, batch);
    if (S.owner->tag != clean) RC(launch_reset_aux(ctx, S.aux, tiles, batch));
    S.owner->tag = 0;
    struct MarkClean {
        DevBuf* b;
        unsigned long long tag;
        bool ok = false;
        ~MarkClean() { if (ok) b->tag = tag; }
    } mark{S.owner, clean};
    RC(launch_color_lab_hist(ctx, src, A, S.aux, g, cg, batch, P->profile.enabled ? 1 : 0, 1));
    RC(launch_clahe_lut(ctx, S.aux, S.luts, cg, batch, S.packed, 1));
    // a run of a frame or two is launch latency: its consumer works the byte map out of [min, max] itself (NormSrc)
    const bool lut_launch = batch > 2;
    if (region && C && fold_norm && sharpen_region_ok(P->sharpen_kernel) && region->x1 > region->x0 && region->y1 > region->y0) {
        // what each stage must find complete in its input: the stage after it, rounded out to that stage's tiles, plus
        // that stage's halo (sharpen 1 px, bilateral 4 px as staged)
        const PxRect s_need = px_dilate(*region, 0, g);
        const PxRect b_need = px_dilate(sharpen_region_cover(g, s_need), 1, g);
        const PxRect c_need = px_dilate(bilateral_region_cover(ctx, g, batch, b_need), 4, g);
        EnhanceRegion ec = {c_need, 0, {nullptr, 0}}, eb = {b_need, 0, {nullptr, 0}}, es = {s_need, 0, {nullptr, 0}};
        // the sharpened frame goes to a THIRD buffer: the complement pass of the bilateral still reads CLAHE's output
        // (B) in a ring inside the region, and that of sharpen the bilateral's (A)
        RC(launch_clahe_apply(ctx, A, S.packed, B, g, cg, batch, &ec));
        RC(launch_bilateral(ctx, B, A, g, batch, &eb));
        RC(launch_sharpen(ctx, A, C, S.aux, tiles, g, P->sharpen_kernel, batch, &es));
        const SatGate gate = {S.aux + (size_t)tiles * 256, aux_words(tiles)}; // min, max of frame 0 (k_sharpen_box)
        ec.invert = eb.invert = es.invert = 1;
        ec.gate = eb.gate = es.gate = gate;
        RC(launch_clahe_apply(ctx, A, S.packed, B, g, cg, batch, &ec));
        RC(launch_bilateral(ctx, B, A, g, batch, &eb));
        RC(launch_sharpen(ctx, A, C, S.aux, tiles, g, P->sharpen_kernel, batch, &es));
        if (lut_launch) RC(launch_norm_lut(ctx, S.aux, tiles, S.norm_lut, batch));
        *norm = lut_launch ? norm_from_lut(S.norm_lut) : norm_from_minmax(S.aux, tiles);
        *result = C;
        mark.ok = true;
        return CBV_OK;
    }
    RC(launch_clahe_apply(ctx, A, S.packed, B, g, cg, batch));
    RC(launch_bilateral(ctx, B, A, g, batch));
    RC(launch_sharpen(ctx, A, B, S.aux, tiles, g, P->sharpen_kernel, batch));
    if (lut_launch) RC(launch_norm_lut(ctx, S.aux, tiles, S.norm_lut, batch));
    *norm = lut_launch ? norm_from_lut(S.norm_lut) : norm_from_minmax(S.aux, tiles);
    if (fold_norm) {
        *result = B;
        mark.ok = true;
        return CBV_OK;
    }
    RC(launch_normalize(ctx, B, A, *norm, g, batch));
    *result = A;
    mark.ok = true;
    return CBV_OK;
}

// Source pixels a dw x dh warp can sample: the image of the destination rectangle under Minv (a projective map keeps it
// convex while W > 0 on it, so its four corners bound it), + 3 px for the 1/32-px rounding and the bilinear taps, clipped
// to the frame.  False when the map is degenerate on the rectangle or the footprint is empty: callers then take the
// whole frame.
bool warp_footprint(const double* Minv, int dw, int dh, int w, int h, PxRect* out)
{
    double lo[2] = {1e30, 1e30}, hi[2] = {-1e30, -1e30};
    for (int k = 0; k < 4; k++) {
        const double dx = (k & 1) ? dw - 1 : 0, dy = (k & 2) ? dh - 1 : 0;
        const double W = Minv[6] * dx + Minv[7] * dy + Minv[8];
        if (!(W > 1e-12)) return false;
        const double c[2] = {(Minv[0] * dx + Minv[1] * dy + Minv[2]) / W, (Minv[3] * dx + Minv[4] * dy + Minv[5]) / W};
        for (int a = 0; a < 2; a++) {
            lo[a] = std::min(lo[a], c[a]);
            hi[a] = std::max(hi[a], c[a]);
        }
    }
    if (!(lo[0] > -1e8 && lo[1] > -1e8 && hi[0] < 1e8 && hi[1] < 1e8)) return false; // (the casts below stay inside int)
    PxRect r = {(int)floor(lo[0]) - 3, (int)floor(lo[1]) - 3, (int)ceil(hi[0]) + 4, (int)ceil(hi[1]) + 4};
    r.x0 = std::max(r.x0, 0);
    r.y0 = std::max(r.y0, 0);
    r.x1 = std::min(r.x1, w);
    r.y1 = std::min(r.y1, h);
    if (r.x1 <= r.x0 || r.y1 <= r.y0) return false;
    *out = r;
    return true;
}

int check_params(cbv_ctx* ctx, const cbv_enhance_params* P)
{
    if (!P) return cbv_fail(ctx, CBV_ERR_ARG, "enhance params are null");
    if (P->tiles_x <= 0 || P->tiles_y <= 0 || P->tiles_x > 64 || P->tiles_y > 64) return cbv_fail(ctx, CBV_ERR_ARG, "bad CLAHE tile grid");
    RC(ctx_set_profile(ctx, &P->profile));
    RC(ctx_set_bilateral(ctx, P->bilateral_d, P->sigma_color, P->sigma_space));
    return CBV_OK;
}

extern "C" int cbv_process_pipeline(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride,
                                    const cbv_enhance_params* params, uint8_t* out, int out_stride)
{
    RC(check_img(ctx, bgr, w, h, stride, 3, "cbv_process_pipeline"));
    if (!out) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_process_pipeline: out is null");
    CBV_ENTER_DRAINED(ctx);
    RC(check_params(ctx, params));
    RC(upload(ctx, &ctx->in, bgr, w * 3, h, stride));
    Geom g = tight_geom(w, h);
    RC(dev_ensure(ctx, &ctx->a, g.frame_stride));
    RC(dev_ensure(ctx, &ctx->b, g.frame_stride));
    SmallLayout S;
    RC(small_layout(ctx, &ctx->small, params->tiles_x * params->tiles_y, 1, &S, params->tiles_x, params->tiles_y));
    u8* res = nullptr;
    NormSrc norm;
    RC(enhance_dev(ctx, (const u8*)ctx->in.p, (u8*)ctx->a.p, (u8*)ctx->b.p, g, params, S, 1, false, &res, &norm));
    return CBV_DONE(download(ctx, res, out, w * 3, h, out_stride));
}

extern "C" int cbv_warp_perspective(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, const double* M9, int dw,
                                    int dh, int rot180, uint8_t* out, int out_stride)
{
    RC(check_img(ctx, bgr, w, h, stride, 3, "cbv_warp_perspective"));
    if (!out || !M9 || dw <= 0 || dh <= 0 || dw > 8192 || dh > 8192) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_warp_perspective: bad arguments");
    CBV_ENTER_DRAINED(ctx);
    double Minv[9];
    if (!host_invert3x3(M9, Minv)) memset(Minv, 0, sizeof(Minv)); // cv::invert returns a zero matrix when singular
    // Only the rows of the frame the warp can sample cross PCIe (the board quad's rows; whole rows, because a 2-D copy
    // with a wide pitch runs at a fifth of the rate of a contiguous one on this platform: tools/ubench_copy.hip).  The
    // rest of the device buffer is never read.
    PxRect fp;
    int y0 = 0, y1 = h;
    if (warp_footprint(Minv, dw, dh, w, h, &fp)) {
        y0 = fp.y0;
        y1 = fp.y1;
    }
    RC(dev_ensure(ctx, &ctx->in, (size_t)w * 3 * h + 256));
    if (ctx->debug_poison) CBV_HIP(ctx, hipMemsetAsync(ctx->in.p, 0xA5, (size_t)w * 3 * h, ctx->stream));
    RC(rows_h2d(ctx, ctx->in.as<u8>() + (size_t)y0 * w * 3, bgr + (size_t)y0 * stride, stride, w * 3, y1 - y0));
    Geom g = tight_geom(w, h);
    RC(dev_ensure(ctx, &ctx->a, (size_t)dw * dh * 3 + 256));
    RC(launch_warp(ctx, warp_src_bgr(ctx->in.as<u8>(), g, NormSrc()), Minv, dw, dh, rot180, ctx->a.as<u8>(), dw * 3, (size_t)dw * dh * 3, 1));
    return CBV_DONE(download(ctx, ctx->a.p, out, dw * 3, dh, out_stride));
}

extern "C" int cbv_warp_color_profile(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, const cbv_color_profile* profile,
                                      const double* M9, int dw, int dh, int rot180, uint8_t* out, int out_stride)
{
    RC(check_img(ctx, bgr, w, h, stride, 3, "cbv_warp_color_profile"));
    if (!out || !M9 || !profile || dw <= 0 || dh <= 0 || dw > 8192 || dh > 8192 || out_stride < dw * 3)
        return cbv_fail(ctx, CBV_ERR_ARG, "cbv_warp_color_profile: bad arguments");
    if (!profile->enabled) return cbv_warp_perspective(ctx, bgr, w, h, stride, M9, dw, dh, rot180, out, out_stride);
    ProfileTabs pt;
    RC(profile_tabs_checked(ctx, profile, &pt, "cbv_warp_color_profile"));
    CBV_ENTER_DRAINED(ctx);
    double Minv[9];
    if (!host_invert3x3(M9, Minv)) memset(Minv, 0, sizeof(Minv));
    RC(upload(ctx, &ctx->in, bgr, w * 3, h, stride));
    RC(dev_ensure(ctx, &ctx->a, (size_t)dw * dh * 3 + 256));
    RC(dev_ensure(ctx, &ctx->b, sizeof(ProfileTabs))); // the call's tables
    CBV_HIP(ctx, hipMemcpyAsync(ctx->b.p, &pt, sizeof(pt), hipMemcpyHostToDevice, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (pt is on this stack)
    RC(launch_warp(ctx, warp_src_profile((const u8*)ctx->in.p, tight_geom(w, h), ctx->b.as<ProfileTabs>()), Minv, dw, dh, rot180, (u8*)ctx->a.p,
                   dw * 3, (size_t)dw * dh * 3, 1));
    return CBV_DONE(download(ctx, ctx->a.p, out, dw * 3, dh, out_stride));
}

// ---------------------------------------------------------------------------
// camera-native frames (include/cbv.h, CBV_FMT_*): cv2.cvtColor(COLOR_YUV2BGR_*) on the device
// ---------------------------------------------------------------------------
// The rows of one plane into the staging buffer.  Tight rows, and rows with a dword-multiple stride of at most twice their
// length, travel as they lie (padding included) in ONE linear copy and keep their stride on the device: k_ingest takes
// strides, and a 2-D copy runs at a fifth of a linear one's rate (rows_h2d).  Anything else is packed by a 2-D copy.
static int plane_h2d(cbv_ctx* ctx, u8* dst, const u8* src, int stride, int wbytes, int rows, int* dev_stride)
{
    const bool as_is = stride == wbytes || ((stride & 3) == 0 && stride <= 2 * wbytes);
    *dev_stride = as_is ? stride : wbytes;
    if (as_is) CBV_HIP(ctx, hipMemcpyAsync(dst, src, (size_t)stride * (rows - 1) + wbytes, hipMemcpyHostToDevice, ctx->stream));
    else RC(rows_h2d(ctx, dst, src, stride, wbytes, rows));
    return CBV_OK;
}

// the planes and strides of a host frame that its format has (plane2 / stride2 are not read for the other formats: a
// caller may have been built against the struct that ended with plane1)
void raw_frame_planes(const cbv_raw_frame* raw, const u8** planes, int* strides)
{
    const int n = raw_fmt_planes(raw_fmt_layout(raw->fmt));
    planes[0] = raw->plane0, strides[0] = raw->stride0;
    planes[1] = n > 1 ? raw->plane1 : nullptr, strides[1] = n > 1 ? raw->stride1 : 0;
    planes[2] = n > 2 ? raw->plane2 : nullptr, strides[2] = n > 2 ? raw->stride2 : 0;
}

int raw_h2d_stage(cbv_ctx* ctx, const cbv_raw_frame* raw, int w, int h, RawPlanes* dev_out, RawGeom* r_out, int* cs_out, const char* what)
{
    RC(check_raw_format(ctx, raw->fmt, w, h, what));
    const int fmt = raw_fmt_layout(raw->fmt);
    const u8* planes[3];
    int strides[3];
    raw_frame_planes(raw, planes, strides);
    RC(check_raw_planes(ctx, fmt, w, planes, strides, what));
    if ((size_t)w * h > (size_t)1 << 28) return cbv_fail(ctx, CBV_ERR_ARG, "%s: image too large", what);
    // a plane follows the largest possible device copy of the one before (rows of twice their length), on a 256-byte boundary
    const int np = raw_fmt_planes(fmt);
    size_t off[4] = {0, 0, 0, 0};
    for (int i = 0; i < np; i++)
        off[i + 1] = (off[i] + (size_t)2 * raw_plane_wbytes(fmt, w, i) * raw_plane_rows(fmt, h, i) + 255) & ~(size_t)255;
    const size_t total = off[np];
    RC(dev_ensure(ctx, &ctx->in, total + 256));
    if (ctx->debug_poison) CBV_HIP(ctx, hipMemsetAsync(ctx->in.p, 0xA5, total, ctx->stream));
    RawGeom r = {};
    r.fmt = fmt;
    u8* st = (u8*)ctx->in.p;
    RawPlanes dev = {{nullptr, nullptr, nullptr}};
    int dev_stride[3] = {0, 0, 0};
    for (int i = 0; i < np; i++) {
        RC(plane_h2d(ctx, st + off[i], planes[i], strides[i], raw_plane_wbytes(fmt, w, i), raw_plane_rows(fmt, h, i), &dev_stride[i]));
        dev.p[i] = st + off[i];
    }
    r.stride0 = dev_stride[0], r.stride1 = dev_stride[1], r.stride2 = dev_stride[2];
    *dev_out = dev;
    *r_out = r;
    *cs_out = raw_fmt_cs(raw->fmt);
    return CBV_OK;
}

int bayer_tables_upload(cbv_ctx* ctx, DevBuf* buf, int fmt, const u8* tables, int bits, BayerDeep* out, const char* who)
{
    if (!raw_fmt_bayer(fmt)) return cbv_fail(ctx, CBV_ERR_ARG, "%s: format %d is not a Bayer format", who, fmt);
    if (!tables) bits = bayer_default_bits(fmt);
    *out = BayerDeep();
    if (!tables && !bits) return CBV_OK; // an 8-bit id's default: no table
    if (!bayer_bits_ok(fmt, bits)) return cbv_fail(ctx, CBV_ERR_ARG, "%s: tables of %d bits do not go with format %d (%s)", who, bits, fmt, raw_fmt_name(fmt));
    const size_t n = (size_t)1 << bits;
    std::vector<u8> neutral;
    if (!tables) { // the neutral table, the same for the three colours
        neutral.resize(3 * n);
        bayer_neutral_table(bits, neutral.data());
        memcpy(neutral.data() + n, neutral.data(), n);
        memcpy(neutral.data() + 2 * n, neutral.data(), n);
        tables = neutral.data();
    }
    RC(dev_ensure(ctx, buf, 3 * n));
    CBV_HIP(ctx, hipMemcpyAsync(buf->p, tables, 3 * n, hipMemcpyHostToDevice, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (the caller's memory, or this stack's)
    out->tab = buf->as<u8>();
    out->bits = bits;
    return CBV_OK;
}

int raw_h2d_convert(cbv_ctx* ctx, const cbv_raw_frame* raw, int w, int h, u8* dst, Geom g, const char* what, const BayerDeep* deep)
{
    RawPlanes dev;
    RawGeom r;
    int cs;
    RC(raw_h2d_stage(ctx, raw, w, h, &dev, &r, &cs, what));
    BayerDeep d = deep ? *deep : BayerDeep();
    if (!deep && raw_fmt_enc(r.fmt)) RC(bayer_tables_upload(ctx, &ctx->b, r.fmt, nullptr, 0, &d, what)); // the encoding's default table
    return launch_ingest_any(ctx, dev, r, dst, g, 1, cs, d);
}

extern "C" int cbv_yuv_to_bgr(cbv_ctx* ctx, const cbv_raw_frame* raw, int w, int h, uint8_t* bgr, int bgr_stride)
{
    if (!ctx) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_yuv_to_bgr: ctx is null");
    if (!raw || !bgr || w <= 0 || h <= 0 || bgr_stride < w * 3) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_yuv_to_bgr: bad arguments");
    RC(check_raw_format(ctx, raw->fmt, w, h, "cbv_yuv_to_bgr"));
    CBV_ENTER_DRAINED(ctx);
    const Geom g = tight_geom(w, h);
    RC(dev_ensure(ctx, &ctx->a, g.frame_stride));
    RC(raw_h2d_convert(ctx, raw, w, h, (u8*)ctx->a.p, g, "cbv_yuv_to_bgr"));
    return CBV_DONE(download(ctx, ctx->a.p, bgr, w * 3, h, bgr_stride));
}

extern "C" int cbv_bayer_to_bgr(cbv_ctx* ctx, const cbv_raw_frame* raw, int w, int h, const uint8_t* tables, int bits, uint8_t* bgr, int bgr_stride)
{
    const char* who = "cbv_bayer_to_bgr";
    if (!ctx) return cbv_fail(nullptr, CBV_ERR_ARG, "%s: ctx is null", who);
    if (!raw || !bgr || w <= 0 || h <= 0 || bgr_stride < w * 3) return cbv_fail(ctx, CBV_ERR_ARG, "%s: bad arguments", who);
    RC(check_raw_format(ctx, raw->fmt, w, h, who));
    if (!raw_fmt_bayer(raw->fmt)) return cbv_fail(ctx, CBV_ERR_ARG, "%s: format %d (%s) is not a Bayer format", who, raw->fmt, raw_fmt_name(raw_fmt_layout(raw->fmt)));
    if (tables && !bayer_bits_ok(raw->fmt, bits))
        return cbv_fail(ctx, CBV_ERR_ARG, "%s: tables of %d bits do not go with format %d (%s)", who, bits, raw->fmt, raw_fmt_name(raw->fmt));
    CBV_ENTER_DRAINED(ctx);
    BayerDeep deep;
    RC(bayer_tables_upload(ctx, &ctx->b, raw->fmt, tables, bits, &deep, who));
    const Geom g = tight_geom(w, h);
    RC(dev_ensure(ctx, &ctx->a, g.frame_stride));
    RC(raw_h2d_convert(ctx, raw, w, h, (u8*)ctx->a.p, g, who, &deep));
    return CBV_DONE(download(ctx, ctx->a.p, bgr, w * 3, h, bgr_stride));
}

// the single-frame raw warps have no tables: a sample encoding goes through a pipeline (include/cbv.h)
static int refuse_bayer_enc(cbv_ctx* ctx, int fmt, const char* who)
{
    if (!raw_fmt_enc(raw_fmt_layout(fmt))) return CBV_OK;
    return cbv_fail(ctx, CBV_ERR_ARG, "%s: format %d (%s) is a sample encoding of a Bayer mosaic, which a pipeline warps (cbv_pipeline_set_input_format)", who, fmt,
                    raw_fmt_name(raw_fmt_layout(fmt)));
}

extern "C" int cbv_warp_color_profile_raw(cbv_ctx* ctx, const cbv_raw_frame* raw, int w, int h, const cbv_color_profile* profile, const double* M9,
                                          int dw, int dh, int rot180, uint8_t* out, int out_stride)
{
    const char* who = "cbv_warp_color_profile_raw";
    if (!ctx) return cbv_fail(nullptr, CBV_ERR_ARG, "%s: ctx is null", who);
    if (!raw || !out || !M9 || !profile || w <= 0 || h <= 0 || dw <= 0 || dh <= 0 || dw > 8192 || dh > 8192 || out_stride < dw * 3)
        return cbv_fail(ctx, CBV_ERR_ARG, "%s: bad arguments", who);
    RC(check_raw_format(ctx, raw->fmt, w, h, who)); // (a BGR frame goes to cbv_warp_color_profile)
    RC(refuse_bayer_enc(ctx, raw->fmt, who));
    ProfileTabs pt;
    RC(profile_tabs_checked(ctx, profile, &pt, who));
    CBV_ENTER_DRAINED(ctx);
    double Minv[9];
    if (!host_invert3x3(M9, Minv)) memset(Minv, 0, sizeof(Minv));
    RawPlanes dev;
    RawGeom r;
    int cs;
    RC(raw_h2d_stage(ctx, raw, w, h, &dev, &r, &cs, who)); // (the staging buffer keeps 256 bytes behind the last plane: the wide loads' slack)
    RC(dev_ensure(ctx, &ctx->a, (size_t)dw * dh * 3 + 256));
    Geom g = tight_geom(w, h);
    WarpSrc src = warp_src_raw(dev, r, g, cs); // a disabled profile: the plain raw warp
    if (profile->enabled) {
        RC(dev_ensure(ctx, &ctx->b, sizeof(ProfileTabs))); // the call's tables
        CBV_HIP(ctx, hipMemcpyAsync(ctx->b.p, &pt, sizeof(pt), hipMemcpyHostToDevice, ctx->stream));
        CBV_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (pt is on this stack)
        src = warp_src_raw_profile(dev, r, g, ctx->b.as<ProfileTabs>(), 1, 0, cs);
    }
    RC(launch_warp(ctx, src, Minv, dw, dh, rot180, (u8*)ctx->a.p, dw * 3, (size_t)dw * dh * 3, 1));
    return CBV_DONE(download(ctx, ctx->a.p, out, dw * 3, dh, out_stride));
}

// One frame of any format through the lens (include/cbv.h).  The staging buffer holds the frame, ctx->a the board, ctx->b the
// call's profile table and, behind it, the launch's table of one entry.
extern "C" int cbv_warp_lens(cbv_ctx* ctx, const cbv_raw_frame* raw, int w, int h, const cbv_color_profile* profile, const cbv_lens* lens,
                             const double* M9, int dw, int dh, int rot180, uint8_t* out, int out_stride)
{
    const char* who = "cbv_warp_lens";
    if (!ctx) return cbv_fail(nullptr, CBV_ERR_ARG, "%s: ctx is null", who);
    if (!raw || !out || !M9 || w <= 0 || h <= 0 || dw <= 0 || dh <= 0 || dw > 8192 || dh > 8192 || out_stride < dw * 3)
        return cbv_fail(ctx, CBV_ERR_ARG, "%s: bad arguments", who);
    RC(check_fmt_cs(ctx, raw->fmt, who));
    const bool bgr = raw->fmt == CBV_FMT_BGR;
    if (bgr) RC(check_img(ctx, raw->plane0, w, h, raw->stride0, 3, who));
    else RC(check_raw_format(ctx, raw->fmt, w, h, who));
    if (!bgr) RC(refuse_bayer_enc(ctx, raw->fmt, who));
    const cbv_color_profile none = {};
    const bool profiled = profile && profile->enabled;
    if (!lens || !lens->enabled) { // the lens-free call of the format
        if (!bgr) return cbv_warp_color_profile_raw(ctx, raw, w, h, profile ? profile : &none, M9, dw, dh, rot180, out, out_stride);
        if (profiled) return cbv_warp_color_profile(ctx, raw->plane0, w, h, raw->stride0, profile, M9, dw, dh, rot180, out, out_stride);
        return cbv_warp_perspective(ctx, raw->plane0, w, h, raw->stride0, M9, dw, dh, rot180, out, out_stride);
    }
    LensDev L;
    RC(lens_checked(ctx, lens, &L, who));
    ProfileTabs pt;
    RC(profile_tabs_checked(ctx, profile ? profile : &none, &pt, who));
    CBV_ENTER_DRAINED(ctx);
    double Minv[9];
    if (!host_invert3x3(M9, Minv)) memset(Minv, 0, sizeof(Minv));
    const Geom g = tight_geom(w, h);
    WarpSrc src;
    const size_t o_tab = (sizeof(ProfileTabs) + 255) & ~(size_t)255;
    RC(dev_ensure(ctx, &ctx->b, o_tab + sizeof(LensBoard)));
    const ProfileTabs* dpt = profiled ? ctx->b.as<ProfileTabs>() : nullptr;
    if (bgr) {
        // only the rows the warp can sample cross PCIe, as in cbv_warp_perspective; with a lens the footprint is
        // warp_footprint_lens's
        PxRect fp;
        int y0 = 0, y1 = h;
        if (warp_footprint_lens(Minv, &L, dw, dh, w, h, &fp)) y0 = fp.y0, y1 = fp.y1;
        RC(dev_ensure(ctx, &ctx->in, (size_t)w * 3 * h + 256));
        if (ctx->debug_poison) CBV_HIP(ctx, hipMemsetAsync(ctx->in.p, 0xA5, (size_t)w * 3 * h, ctx->stream));
        RC(rows_h2d(ctx, ctx->in.as<u8>() + (size_t)y0 * w * 3, raw->plane0 + (size_t)y0 * raw->stride0, raw->stride0, w * 3, y1 - y0));
        src = profiled ? warp_src_profile(ctx->in.as<u8>(), g, dpt) : warp_src_bgr(ctx->in.as<u8>(), g, NormSrc());
    } else {
        RawPlanes dev;
        RawGeom r;
        int cs;
        RC(raw_h2d_stage(ctx, raw, w, h, &dev, &r, &cs, who)); // (the staging buffer keeps 256 bytes behind the last plane: the wide loads' slack)
        src = profiled ? warp_src_raw_profile(dev, r, g, dpt, 1, 0, cs) : warp_src_raw(dev, r, g, cs);
    }
    RC(dev_ensure(ctx, &ctx->a, (size_t)dw * dh * 3 + 256));
    const LensBoard T = lens_board(Minv, dw, dh, rot180, (u8*)ctx->a.p, dw * 3, (size_t)dw * dh * 3, dpt);
    if (profiled) CBV_HIP(ctx, hipMemcpyAsync(ctx->b.p, &pt, sizeof(pt), hipMemcpyHostToDevice, ctx->stream));
    CBV_HIP(ctx, hipMemcpyAsync((u8*)ctx->b.p + o_tab, &T, sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (pt and T are on this stack)
    RC(launch_warp_lens(ctx, src, L, (const LensBoard*)((u8*)ctx->b.p + o_tab), 1, dw, dh, 0, 1, nullptr, nullptr));
    return CBV_DONE(download(ctx, ctx->a.p, out, dw * 3, dh, out_stride));
}

extern "C" int cbv_noise_run(cbv_ctx* ctx, const uint64_t* changes, int n, cbv_noise_state* state, cbv_noise_result* out)
{
    if (!ctx || !changes || !state || !out || n <= 0) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_noise_run: bad arguments");
    CBV_ENTER_DRAINED(ctx);
    size_t b_in = ((size_t)n * 8 + 255) & ~(size_t)255, b_out = ((size_t)n * sizeof(cbv_noise_result) + 255) & ~(size_t)255;
    RC(dev_ensure(ctx, &ctx->c, b_in + b_out + 256));
    u8* base = (u8*)ctx->c.p;
    CBV_HIP(ctx, hipMemcpyAsync(base, changes, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    CBV_HIP(ctx, hipMemcpyAsync(base + b_in + b_out, state, sizeof(cbv_noise_state), hipMemcpyHostToDevice, ctx->stream));
    RC(launch_noise(ctx, (const u64*)base, 1, n, (cbv_noise_state*)(base + b_in + b_out), (cbv_noise_result*)(base + b_in)));
    CBV_HIP(ctx, hipMemcpyAsync(out, base + b_in, (size_t)n * sizeof(cbv_noise_result), hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipMemcpyAsync(state, base + b_in + b_out, sizeof(cbv_noise_state), hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_DONE(CBV_OK);
}
