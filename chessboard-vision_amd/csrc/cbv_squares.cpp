// C-ABI of libcbv_hip.so (include/cbv.h), the per-square detector state behind the class API: cbv_squares_* and
// cbv_decide_piece.  Entry points that move host memory enter through CBV_ENTER_DRAINED (cbv_internal.h).
#include <math.h>
#include <string.h>

#include <algorithm>

#include "cbv_internal.h"
#include "piece_sweep_core.h"

struct cbv_squares {
    cbv_ctx* ctx = nullptr;
    int n = 0;
    int blur_k = 0;
    std::vector<SquareDesc> descs;
    size_t plane_total = 0, mask_total = 0;
    DevBuf d_descs, d_masks, d_gray, d_ref, d_mean, d_var, d_stats, d_select, d_coef, d_stage, d_hough, d_retry;
    DevBuf d_fast;  // one-call entry points: worklist (1 + 64 u32) | retry list (1 + 64 u32) | dflags (64 B) | second statistics set
    DevBuf d_gray5; // cbv_squares_detect_changes with blur_k != 5: the squares as PieceDetector preprocesses them (k = 5)
    std::vector<SquareDesc> descs_on_dev; // what d_descs holds (a host-image load re-uploads only when it differs)
    std::vector<u8> stage;
    bool has_ref = false, has_model = false;
    int coef_k = -1;

    // the device buffers as what the launchers take
    SquareDesc* ddescs() const { return d_descs.as<SquareDesc>(); }
    u8* masks() const { return d_masks.as<u8>(); }
    u8* gray() const { return d_gray.as<u8>(); }
    u8* ref() const { return d_ref.as<u8>(); }
    float* mean() const { return d_mean.as<float>(); }
    float* var() const { return d_var.as<float>(); }
    float* sd() const { return var() + plane_total; } // np.sqrt(var) of every pixel, kept beside the variance plane by the kernels that write it
    int* coef() const { return d_coef.as<int>(); }
    u8* staged() const { return d_stage.as<u8>(); }
};

extern "C" int cbv_squares_create(cbv_ctx* ctx, cbv_squares** out)
{
    if (!ctx || !out) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_squares_create: null argument");
    cbv_squares* s = new cbv_squares();
    s->ctx = ctx;
    *out = s;
    return CBV_OK;
}

extern "C" void cbv_squares_destroy(cbv_squares* s)
{
    if (!s) return;
    {
        std::lock_guard<std::recursive_mutex> lock(s->ctx->mu);
        (void)hipSetDevice(s->ctx->device);
        (void)hipStreamSynchronize(s->ctx->stream);
    }
    DevBuf* bufs[] = {&s->d_descs, &s->d_masks, &s->d_gray, &s->d_ref, &s->d_mean, &s->d_var, &s->d_stats, &s->d_select, &s->d_coef, &s->d_stage, &s->d_hough, &s->d_retry,
                      &s->d_fast, &s->d_gray5};
    for (auto b : bufs) dev_free(b);
    delete s;
}

static int squares_set_coef(cbv_squares* s, int blur_k)
{
    cbv_ctx* ctx = s->ctx;
    if (blur_k < 1) blur_k = 1;
    blur_k |= 1;
    if (blur_k > 31) return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "blur kernel %d too large (max 31)", blur_k);
    if (s->coef_k != blur_k) {
        int coef[32] = {0};
        build_gaussian_q8(blur_k, coef);
        RC(dev_ensure(ctx, &s->d_coef, sizeof(coef)));
        CBV_HIP(ctx, hipMemcpyAsync(s->d_coef.p, coef, sizeof(coef), hipMemcpyHostToDevice, ctx->stream));
        CBV_HIP(ctx, hipStreamSynchronize(ctx->stream)); // coef is a stack array
        s->coef_k = blur_k;
    }
    s->blur_k = blur_k;
    return CBV_OK;
}

size_t square_table(const int* ws, const int* hs, int n, std::vector<SquareDesc>* descs, std::vector<u8>* masks)
{
    descs->assign(n, SquareDesc());
    size_t off = 0;
    for (int i = 0; i < n; i++) {
        SquareDesc& d = (*descs)[i];
        d.w = ws[i];
        d.h = hs[i];
        d.plane_off = d.mask_off = (int)off;
        off += ((size_t)ws[i] * hs[i] + 15) & ~(size_t)15;
    }
    masks->assign(off, 0);
    for (SquareDesc& d : *descs) {
        build_piece_mask(d.w, d.h, masks->data() + d.mask_off);
        square_region_counts(masks->data() + d.mask_off, d.w * d.h, d.cnt);
    }
    return off;
}

// (re)build geometry-dependent tables when the set of square shapes changes
static int squares_set_geometry(cbv_squares* s, const int* ws, const int* hs, int n)
{
    cbv_ctx* ctx = s->ctx;
    bool same = (n == s->n);
    for (int i = 0; same && i < n; i++) same = s->descs[i].w == ws[i] && s->descs[i].h == hs[i];
    if (same) return CBV_OK;
    for (int i = 0; i < n; i++) // validate before any state changes: a rejected load leaves the set as it was
        if (ws[i] <= 0 || hs[i] <= 0 || ws[i] > CBV_MAX_SQUARE_DIM || hs[i] > CBV_MAX_SQUARE_DIM)
            return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "square %d is %dx%d; supported up to %dx%d", i, ws[i], hs[i], CBV_MAX_SQUARE_DIM, CBV_MAX_SQUARE_DIM);
    std::vector<u8> masks;
    const size_t off = square_table(ws, hs, n, &s->descs, &masks);
    s->n = n;
    s->plane_total = off;
    s->has_ref = s->has_model = false;
    RC(dev_ensure(ctx, &s->d_masks, off));
    RC(dev_ensure(ctx, &s->d_gray, off));
    RC(dev_ensure(ctx, &s->d_ref, off));
    RC(dev_ensure(ctx, &s->d_mean, off * 4));
    RC(dev_ensure(ctx, &s->d_var, off * 8)); // variance plane, then its square root (cbv_squares::sd)
    RC(dev_ensure(ctx, &s->d_stats, sizeof(cbv_sq_stats) * n));
    RC(dev_ensure(ctx, &s->d_select, CBV_MAX_SQUARES * 4));
    RC(dev_ensure(ctx, &s->d_descs, sizeof(SquareDesc) * n));
    CBV_HIP(ctx, hipMemcpy(s->d_masks.p, masks.data(), off, hipMemcpyHostToDevice));
    return CBV_OK;
}

extern "C" int cbv_squares_load(cbv_squares* s, const cbv_square_view* views, int n, int blur_k)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    if (!views || n <= 0 || n > CBV_MAX_SQUARES) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_squares_load: bad arguments (n=%d)", n);
    CBV_ENTER_DRAINED(ctx);
    int ws[CBV_MAX_SQUARES], hs[CBV_MAX_SQUARES];
    for (int i = 0; i < n; i++) {
        if (!views[i].data) { // keep the current gray of this square (its geometry must already be known)
            if (i >= s->n) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_squares_load: view %d is null but the square is unknown", i);
            ws[i] = s->descs[i].w;
            hs[i] = s->descs[i].h;
            continue;
        }
        if ((views[i].cn != 1 && views[i].cn != 3) || views[i].stride < views[i].w * views[i].cn)
            return cbv_fail(ctx, CBV_ERR_ARG, "cbv_squares_load: bad view %d", i);
        ws[i] = views[i].w;
        hs[i] = views[i].h;
    }
    RC(squares_set_geometry(s, ws, hs, n));
    RC(squares_set_coef(s, blur_k));
    // pack the views tightly into one staging buffer (the caller's arrays may be scattered)
    size_t total = 0;
    for (int i = 0; i < n; i++) {
        if (!views[i].data) {
            s->descs[i].cn = 0; // skipped by the kernel
            continue;
        }
        s->descs[i].cn = views[i].cn;
        s->descs[i].stride = views[i].w * views[i].cn;
        s->descs[i].src_off = (int)total;
        total += ((size_t)views[i].w * views[i].cn * views[i].h + 15) & ~(size_t)15;
    }
    if (total == 0) total = 16;
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream)); // staging may still be in flight from the previous call
    s->stage.resize(total);
    for (int i = 0; i < n; i++) {
        if (!views[i].data) continue;
        const int rb = views[i].w * views[i].cn;
        for (int y = 0; y < views[i].h; y++)
            memcpy(s->stage.data() + s->descs[i].src_off + (size_t)y * rb, views[i].data + (size_t)y * views[i].stride, rb);
    }
    RC(dev_ensure(ctx, &s->d_stage, total));
    CBV_HIP(ctx, hipMemcpyAsync(s->d_stage.p, s->stage.data(), total, hipMemcpyHostToDevice, ctx->stream));
    CBV_HIP(ctx, hipMemcpyAsync(s->d_descs.p, s->descs.data(), sizeof(SquareDesc) * n, hipMemcpyHostToDevice, ctx->stream));
    s->descs_on_dev.clear();
    RC(launch_squares_preprocess(ctx, s->staged(), 0, s->ddescs(), n, s->coef(), s->blur_k, s->gray(), 0, 1));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_DONE(CBV_OK);
}

extern "C" int cbv_squares_load_dev(cbv_squares* s, const void* dev_img, int w, int h, int stride, int cn,
                                    const cbv_roi* rois, int n, int blur_k)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    if (!dev_img || !rois || n <= 0 || n > CBV_MAX_SQUARES || (cn != 1 && cn != 3)) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_squares_load_dev: bad arguments");
    CBV_ENTER_DRAINED(ctx);
    int ws[CBV_MAX_SQUARES], hs[CBV_MAX_SQUARES];
    for (int i = 0; i < n; i++) {
        if (rois[i].x0 < 0 || rois[i].y0 < 0 || rois[i].x0 + rois[i].w > w || rois[i].y0 + rois[i].h > h)
            return cbv_fail(ctx, CBV_ERR_ARG, "cbv_squares_load_dev: roi %d outside the image", i);
        ws[i] = rois[i].w;
        hs[i] = rois[i].h;
    }
    RC(squares_set_geometry(s, ws, hs, n));
    RC(squares_set_coef(s, blur_k));
    for (int i = 0; i < n; i++) {
        s->descs[i].cn = cn;
        s->descs[i].stride = stride;
        s->descs[i].src_off = rois[i].y0 * stride + rois[i].x0 * cn;
    }
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    CBV_HIP(ctx, hipMemcpyAsync(s->d_descs.p, s->descs.data(), sizeof(SquareDesc) * n, hipMemcpyHostToDevice, ctx->stream));
    s->descs_on_dev.clear();
    RC(launch_squares_preprocess(ctx, (const u8*)dev_img, 0, s->ddescs(), n, s->coef(), s->blur_k, s->gray(), 0, 1));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_DONE(CBV_OK);
}

static int squares_select(cbv_squares* s, const uint8_t* select, const u8** dev)
{
    *dev = nullptr;
    if (!select) return CBV_OK;
    cbv_ctx* ctx = s->ctx;
    CBV_HIP(ctx, hipMemcpyAsync(s->d_select.p, select, s->n, hipMemcpyHostToDevice, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *dev = s->d_select.as<u8>();
    return CBV_OK;
}

extern "C" int cbv_squares_calibrate(cbv_squares* s, double initial_variance, const uint8_t* select)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    CBV_ENTER_DRAINED(ctx);
    if (s->n == 0) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_squares_calibrate: no squares loaded");
    const u8* sel;
    RC(squares_select(s, select, &sel));
    RC(launch_squares_calibrate(ctx, s->ddescs(), s->n, s->gray(), s->mean(), s->var(), s->sd(), (float)initial_variance, sel));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->has_model = true;
    return CBV_DONE(CBV_OK);
}

extern "C" int cbv_squares_ema(cbv_squares* s, double alpha, const uint8_t* select)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    CBV_ENTER_DRAINED(ctx);
    if (!s->has_model) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_squares_ema: not calibrated");
    const u8* sel;
    RC(squares_select(s, select, &sel));
    RC(launch_squares_ema(ctx, s->ddescs(), s->n, s->gray(), s->mean(), s->var(), s->sd(), alpha, sel));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_DONE(CBV_OK);
}

extern "C" int cbv_squares_set_ref(cbv_squares* s, const uint8_t* select)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    CBV_ENTER_DRAINED(ctx);
    if (s->n == 0) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_squares_set_ref: no squares loaded");
    const u8* sel;
    RC(squares_select(s, select, &sel));
    RC(launch_squares_set_ref(ctx, s->ddescs(), s->n, s->gray(), s->ref(), sel));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->has_ref = true;
    return CBV_DONE(CBV_OK);
}

extern "C" int cbv_squares_stats(cbv_squares* s, int use_ref, int use_model, double z_threshold, cbv_sq_stats* out)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    CBV_ENTER_DRAINED(ctx);
    if (!out || s->n == 0) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_squares_stats: no squares loaded or null output");
    if (use_model && !s->has_model) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_squares_stats: model requested but not calibrated");
    RC(launch_squares_stats(ctx, s->ddescs(), s->n, s->gray(), 0, use_ref ? s->ref() : nullptr, use_model ? s->mean() : nullptr,
                            use_model ? s->sd() : nullptr, s->masks(), (float)z_threshold, s->d_stats.as<cbv_sq_stats>(), 1));
    CBV_HIP(ctx, hipMemcpyAsync(out, s->d_stats.p, sizeof(cbv_sq_stats) * s->n, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_DONE(CBV_OK);
}

// the checks of hough_cfg that need no square geometry (entry points run them before they change any state)
int hough_params_check(cbv_ctx* ctx, const cbv_hough_params* prm)
{
    if (!prm || !(prm->dp > 0) || prm->param1 < 0 || prm->param2 < 0 || !(prm->max_radius_ratio >= 0) || !(prm->min_radius_ratio >= 0))
        return cbv_fail(ctx, CBV_ERR_ARG, "HoughCircles parameters are invalid");
    if (prm->max_radius_ratio > 4.0 || prm->min_radius_ratio > 4.0)
        return cbv_fail(ctx, CBV_ERR_ARG, "HoughCircles radius ratios above 4 squares are not supported (got %g, %g)", prm->min_radius_ratio,
                        prm->max_radius_ratio);
    return CBV_OK;
}

int hough_cfg(cbv_ctx* ctx, const cbv_hough_params* prm, const std::vector<SquareDesc>& descs, HoughCfg* hc)
{
    RC(hough_params_check(ctx, prm));
    memset(hc, 0, sizeof(*hc));
    hc->dp = (float)prm->dp < 1.f ? 1.f : (float)prm->dp;
    hc->canny_thr = (int)nearbyint(prm->param1);
    hc->acc_thr = (int)nearbyint(prm->param2);
    hc->min_ratio = prm->min_radius_ratio;
    hc->max_ratio = prm->max_radius_ratio;
    for (const SquareDesc& d : descs) {
        hc->maxw = std::max(hc->maxw, d.w);
        hc->maxh = std::max(hc->maxh, d.h);
        const int m = std::min(d.w, d.h);
        hc->min_dim = hc->min_dim == 0 ? m : std::min(hc->min_dim, m);
    }
    return CBV_OK;
}

// The second HoughCircles pass, over the squares the first one listed in `retry` (rarely any; a launch of its own), then
// `count` records of `hough` back to `dst` and the wait for them.
static int squares_hough_second(cbv_squares* s, int n, const u8* gray, const HoughCfg& hc, cbv_hough_result* hough, const u32* retry, void* dst, int count)
{
    cbv_ctx* ctx = s->ctx;
    RC(launch_hough_second(ctx, s->ddescs(), n, gray, 0, hc, hough, nullptr, retry, n));
    CBV_HIP(ctx, hipMemcpyAsync(dst, hough, sizeof(cbv_hough_result) * count, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

extern "C" int cbv_squares_hough(cbv_squares* s, const cbv_hough_params* prm, cbv_hough_result* out)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    CBV_ENTER_DRAINED(ctx);
    if (!out || s->n == 0) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_squares_hough: no squares loaded or null output");
    HoughCfg hc;
    RC(hough_cfg(ctx, prm, s->descs, &hc));
    RC(dev_ensure(ctx, &s->d_hough, sizeof(cbv_hough_result) * CBV_MAX_SQUARES));
    RC(dev_ensure(ctx, &s->d_retry, sizeof(u32) * (1 + CBV_MAX_SQUARES)));
    cbv_hough_result* hough = s->d_hough.as<cbv_hough_result>();
    u32* retry = s->d_retry.as<u32>();
    CBV_HIP(ctx, hipMemsetAsync(retry, 0, sizeof(u32), ctx->stream));
    RC(launch_hough(ctx, s->ddescs(), s->n, s->gray(), 0, hc, hough, nullptr, nullptr, 1, retry, 0));
    // no look at the retry count here: the second pass is enqueued behind the first and finds its list empty as a rule
    return CBV_DONE(squares_hough_second(s, s->n, s->gray(), hc, hough, retry, out, s->n));
}

// ---------------------------------------------------------------------------
// one call per frame for the reference's own call pattern (game_session.py:124-161, calibrate_sensitivity.py:142-157):
// the 64 squares are views of ONE host image (split_board of the warped board), so the image's bounding rows are
// uploaded with one copy AT CALL TIME (nothing stale, no host pointer kept) and everything up to the per-square records
// runs behind it with one wait at the end.
// ---------------------------------------------------------------------------
static bool same_desc(const SquareDesc& a, const SquareDesc& b)
{
    return a.w == b.w && a.h == b.h && a.src_off == b.src_off && a.stride == b.stride && a.cn == b.cn && a.plane_off == b.plane_off &&
           a.mask_off == b.mask_off;
}

// geometry + upload of the rows of `img` the ROIs cover + descriptors; leaves the stream with d_stage / d_descs ready.
// `hst` (pinned, >= sizeof(SquareDesc) * n) stages the descriptors when they changed.
static int squares_stage_host_image(cbv_squares* s, const cbv_host_image* img, const cbv_roi* rois, int n, int blur_k, u8* hst)
{
    cbv_ctx* ctx = s->ctx;
    if (!img || !img->data || !rois || n <= 0 || n > CBV_MAX_SQUARES || (img->cn != 1 && img->cn != 3) || img->w <= 0 || img->h <= 0 ||
        img->stride < img->w * img->cn)
        return cbv_fail(ctx, CBV_ERR_ARG, "host image / roi arguments are invalid (n=%d)", n);
    int ws[CBV_MAX_SQUARES], hs[CBV_MAX_SQUARES];
    int y0 = img->h, y1 = 0;
    for (int i = 0; i < n; i++) {
        const cbv_roi& r = rois[i];
        if (r.w <= 0 || r.h <= 0 || r.x0 < 0 || r.y0 < 0 || r.x0 + r.w > img->w || r.y0 + r.h > img->h)
            return cbv_fail(ctx, CBV_ERR_ARG, "roi %d (%d,%d %dx%d) is outside the %dx%d image", i, r.x0, r.y0, r.w, r.h, img->w, img->h);
        ws[i] = r.w;
        hs[i] = r.h;
        y0 = std::min(y0, r.y0);
        y1 = std::max(y1, r.y0 + r.h);
    }
    RC(squares_set_geometry(s, ws, hs, n));
    RC(squares_set_coef(s, blur_k));
    // One contiguous copy of the rows the ROIs cover.  When the image's rows are padded or it is a crop of a wider frame,
    // the bytes between its rows travel too as long as that at most doubles the copy (they lie inside the same
    // allocation: between the first and the last byte of the image); a much wider pitch is gathered by a 2-D copy,
    // which is several times slower per byte on this platform (tools/ubench_copy.hip).
    const int rowb = img->w * img->cn;
    const bool one_d = img->stride <= 2 * rowb;
    const int pitch = one_d ? img->stride : rowb;
    for (int i = 0; i < n; i++) {
        s->descs[i].cn = img->cn;
        s->descs[i].stride = pitch;
        s->descs[i].src_off = (rois[i].y0 - y0) * pitch + rois[i].x0 * img->cn;
    }
    const size_t bytes = (size_t)pitch * (y1 - y0 - 1) + rowb;
    RC(dev_ensure(ctx, &s->d_stage, bytes + 16)); // (+16: the 12-byte loads of the last pixels of the last row)
    if (ctx->debug_poison) CBV_HIP(ctx, hipMemsetAsync(s->d_stage.p, 0xA5, bytes + 16, ctx->stream));
    const u8* src = img->data + (size_t)y0 * img->stride;
    if (one_d) CBV_HIP(ctx, hipMemcpyAsync(s->d_stage.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    else CBV_HIP(ctx, hipMemcpy2DAsync(s->d_stage.p, rowb, src, img->stride, rowb, y1 - y0, hipMemcpyHostToDevice, ctx->stream));
    bool same = (int)s->descs_on_dev.size() == n;
    for (int i = 0; same && i < n; i++) same = same_desc(s->descs_on_dev[i], s->descs[i]);
    if (!same) {
        memcpy(hst, s->descs.data(), sizeof(SquareDesc) * n);
        CBV_HIP(ctx, hipMemcpyAsync(s->d_descs.p, hst, sizeof(SquareDesc) * n, hipMemcpyHostToDevice, ctx->stream));
        s->descs_on_dev = s->descs;
    }
    return CBV_OK;
}

static int max_px_of(const cbv_squares* s)
{
    int m = 0;
    for (const SquareDesc& d : s->descs) m = std::max(m, d.w * d.h);
    return m;
}

// preprocess (k = 5) + statistics of the staged image into `gray` / `out`, as one launch.  k_squares_pre5_stats stages BGR
// pixels whatever the descriptors say, so a single-channel image takes the two launches it fuses.
static int squares_pre5_stats(cbv_squares* s, int n, u8* gray, const float* mean, const float* sd, float z_thresh, cbv_sq_stats* out, int want_hough,
                              u32* work, cbv_hough_result* hough, const u8* ref = nullptr, const DetectMasks* dm = nullptr)
{
    cbv_ctx* ctx = s->ctx;
    if (s->descs[0].cn == 3)
        return launch_squares_pre5_stats(ctx, s->staged(), 0, s->ddescs(), n, gray, 0, mean, sd, s->masks(), z_thresh, out, 1, nullptr, want_hough, work, hough,
                                         max_px_of(s), ref, dm);
    RC(launch_squares_preprocess(ctx, s->staged(), 0, s->ddescs(), n, nullptr, 5, gray, 0, 1, max_px_of(s)));
    return launch_squares_stats(ctx, s->ddescs(), n, gray, 0, ref, mean, sd, s->masks(), z_thresh, out, 1, nullptr, want_hough, work, hough, dm);
}

// device scratch of the one-call entry points: worklist | retry list | then everything that travels back to the host as
// ONE copy: gate flags | statistics | second statistics set (k = 5 planes) | HoughCircles records
struct FastLayout {
    static constexpr size_t o_retry = 512, o_out = 1024; // in d_fast; the worklist is at 0
    static constexpr size_t retry_gap = o_out - o_retry; // (cbv_squares_detect_all copies [retry, out + out_bytes) back as one block)
    // offsets inside the block
    static constexpr size_t o_flags = 0, o_stats = 64, o_stats5 = o_stats + sizeof(cbv_sq_stats) * CBV_MAX_SQUARES,
                            o_hough = o_stats5 + sizeof(cbv_sq_stats) * CBV_MAX_SQUARES, out_bytes = o_hough + sizeof(cbv_hough_result) * CBV_MAX_SQUARES;
    u32* work;
    u32* retry;
    u8* dflags;
    cbv_sq_stats* stats;
    cbv_sq_stats* stats5;
    cbv_hough_result* hough;
};
// The 64 KB pinned staging area (cbv_ctx::h_stage) as these entry points use it: the descriptors on their way to the
// device (squares_stage_host_image), FastLayout's block on its way back, and cbv_squares_detect_changes' worklist.
struct HStage {
    static constexpr size_t descs = 0, bytes = 65536;
    static constexpr size_t out = 8192;                          // FastLayout's block
    static constexpr size_t retry = out - FastLayout::retry_gap; // detect_all: the retry list's count, which travels in front of the block
    static constexpr size_t work = 40960;                        // detect_changes: the worklist the host builds (1 + 64 u32)
    static constexpr size_t retry_back = work + 1024;            // detect_changes: the retry list's count, fetched on its own
};
static_assert(HStage::descs + sizeof(SquareDesc) * CBV_MAX_SQUARES <= HStage::retry, "the descriptors overrun the retry word");
static_assert(HStage::out + FastLayout::out_bytes <= HStage::work, "result block overruns the worklist");
static_assert(HStage::work + 4 * (1 + CBV_MAX_SQUARES) <= HStage::retry_back && HStage::retry_back + 4 <= HStage::bytes, "staging layout");
static_assert(4 * (1 + CBV_MAX_SQUARES) <= FastLayout::o_retry && 4 * (1 + CBV_MAX_SQUARES) <= FastLayout::retry_gap, "device lists overlap");

static int fast_layout(cbv_squares* s, FastLayout* L)
{
    RC(dev_ensure(s->ctx, &s->d_fast, FastLayout::o_out + FastLayout::out_bytes));
    u8* b = s->d_fast.as<u8>();
    L->work = (u32*)b;
    L->retry = (u32*)(b + FastLayout::o_retry);
    L->dflags = b + FastLayout::o_out + FastLayout::o_flags;
    L->stats = (cbv_sq_stats*)(b + FastLayout::o_out + FastLayout::o_stats);
    L->stats5 = (cbv_sq_stats*)(b + FastLayout::o_out + FastLayout::o_stats5);
    L->hough = (cbv_hough_result*)(b + FastLayout::o_out + FastLayout::o_hough);
    return CBV_OK;
}

extern "C" int cbv_squares_load_image(cbv_squares* s, const cbv_host_image* img, const cbv_roi* rois, int n, int blur_k)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    CBV_ENTER_DRAINED(ctx);
    u8* hst;
    RC(ctx_hstage(ctx, HStage::bytes, &hst));
    RC(squares_stage_host_image(s, img, rois, n, blur_k, hst + HStage::descs));
    RC(launch_squares_preprocess(ctx, s->staged(), 0, s->ddescs(), n, s->coef(), s->blur_k, s->gray(), 0, 1, max_px_of(s)));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the host image (and the pinned descriptors) are free again
    return CBV_DONE(CBV_OK);
}

extern "C" int cbv_squares_set_ref_mask(cbv_squares* s, uint64_t mask)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    CBV_ENTER(ctx); // (no host memory moves: nothing to drain)
    if (s->n == 0) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_squares_set_ref_mask: no squares loaded");
    RC(launch_squares_set_ref_mask(ctx, s->ddescs(), s->n, s->gray(), s->ref(), mask));
    s->has_ref = true;
    return CBV_OK; // asynchronous: later calls on this context are ordered behind it
}

// np.std(gray) (piece_detector.py:305) of a C-contiguous uint8 array in numpy's own float64 steps: the mean is the exact
// sum divided once; each deviation is rounded, squared and rounded; the squares are added by numpy's pairwise summation
// (below 8 elements left to right, up to 128 eight interleaved partial sums combined as a tree plus the tail, above that
// halves cut at a multiple of eight) inside chunks of 8192 elements (the ufunc buffer), chunk after chunk onto 0; one
// division, one square root.  This file is compiled without contraction, so every line below rounds once.
static inline double np_sq_dev(u8 x, double mean)
{
    const double d = (double)x - mean;
    return d * d;
}

static double np_pairwise_sq_dev(const u8* px, int n, double mean)
{
    if (n < 8) {
        double res = 0.;
        for (int i = 0; i < n; i++) res = res + np_sq_dev(px[i], mean);
        return res;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; j++) r[j] = np_sq_dev(px[j], mean);
        int i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; j++) r[j] = r[j] + np_sq_dev(px[i + j], mean);
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; i++) res = res + np_sq_dev(px[i], mean);
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    const double a = np_pairwise_sq_dev(px, n2, mean);
    const double b = np_pairwise_sq_dev(px + n2, n - n2, mean);
    return a + b;
}

extern "C" int cbv_np_std_below_15(const uint8_t* gray, int n, double* std_out)
{
    if (!gray || n <= 0) return CBV_ERR_ARG;
    unsigned long long sum = 0;
    for (int i = 0; i < n; i++) sum += gray[i];
    const double mean = (double)sum / (double)n;
    double acc = 0.;
    for (int i = 0; i < n; i += 8192) acc = acc + np_pairwise_sq_dev(gray + i, n - i < 8192 ? n - i : 8192, mean);
    const double sd = sqrt(acc / (double)n);
    if (std_out) *std_out = sd;
    return sd < 15 ? 1 : 0;
}

// The variance of the square is exactly 225: the one case in which numpy's rounded np.std(gray) < 15 can differ from the
// exact integer test of piece_uniform (it then says 14.999999999999998 for some pixel orders; DESIGN.md section 6,
// "Square regions").  With the pixels at hand the one-call entry points follow numpy there.
static bool piece_std_tie(const cbv_sq_stats* st)
{
    const long long n = st->n, sm = st->sum;
    return n * (long long)st->sumsq - sm * sm == 225ll * n * n;
}

// `uniform` of square i of the set whose planes are at `planes`, read back and evaluated as numpy does (rare: ties only);
// the stream is idle when the callers get here
static int squares_uniform_at_tie(cbv_squares* s, const u8* planes, int i, bool* uniform)
{
    cbv_ctx* ctx = s->ctx;
    const SquareDesc& d = s->descs[i];
    std::vector<u8> px((size_t)d.w * d.h);
    CBV_HIP(ctx, hipMemcpyAsync(px.data(), planes + d.plane_off, px.size(), hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *uniform = cbv_np_std_below_15(px.data(), (int)px.size(), nullptr) == 1;
    return CBV_OK;
}

// PieceDetector.detect_piece (piece_detector.py:289-345) for one square from its statistics and its HoughCircles
// record: the decision itself is piece_decide (piece_sweep_core.h), which the settings sweep shares.
extern "C" int cbv_decide_piece(const cbv_sq_stats* st, const cbv_hough_result* hg, int w, int h, double circle_threshold,
                                cbv_piece_result* out)
{
    if (!st || !out) return CBV_ERR_ARG;
    if (hg && (hg->flags & CBV_HOUGH_OVERFLOW) && !piece_uniform(st)) { // never passed on as HoughCircles' answer
        out->has_piece = 0;
        out->method = CBV_METHOD_NONE;
        out->cx = out->cy = out->radius = 0;
        out->confidence = 0.0;
        out->center_border_diff = 0.0;
        return CBV_ERR_UNSUPPORTED;
    }
    const bool found = hg && hg->found;
    // int(np.float32): toward zero
    piece_decide(st, found, found ? hg->kind : 0, found ? (int)hg->cx : 0, found ? (int)hg->cy : 0, found ? (int)hg->r : 0, w, h, circle_threshold, out);
    return CBV_OK;
}

extern "C" int cbv_squares_detect_all(cbv_squares* s, const cbv_host_image* img, const cbv_roi* rois, int n,
                                      const cbv_detect_params* prm, cbv_piece_result* out)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    if (!prm || !out) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_squares_detect_all: null argument");
    CBV_ENTER_DRAINED(ctx);
    RC(hough_params_check(ctx, &prm->hough)); // before anything of the set changes
    u8* hst;
    RC(ctx_hstage(ctx, HStage::bytes, &hst));
    FastLayout L;
    RC(fast_layout(s, &L));
    // worklist and retry counters; in front of the upload, whose host-blocking copy would otherwise leave the GPU idle
    // while this launch is submitted
    CBV_HIP(ctx, hipMemsetAsync(s->d_fast.p, 0, FastLayout::o_out, ctx->stream));
    RC(squares_stage_host_image(s, img, rois, n, 5, hst + HStage::descs));
    HoughCfg hc;
    RC(hough_cfg(ctx, &prm->hough, s->descs, &hc));
    const DetectMasks dm = {s->has_ref ? prm->has_ref : 0, prm->cached, prm->check, prm->check_given, prm->use_delta, prm->change_threshold, L.dflags};
    // preprocess + statistics (+ |gray - reference|) + the gate, one launch; HoughCircles over the squares it listed
    RC(squares_pre5_stats(s, n, s->gray(), nullptr, nullptr, 0.f, L.stats, 1, L.work, L.hough, s->ref(), &dm));
    RC(launch_hough(ctx, s->ddescs(), n, s->gray(), 0, hc, L.hough, nullptr, L.work, 1, L.retry, 0));
    // the second-pass list travels back in front of the results: normally it is empty and the second pass is never enqueued
    CBV_HIP(ctx, hipMemcpyAsync(hst + HStage::retry, L.retry, FastLayout::retry_gap + FastLayout::out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    u8* back = hst + HStage::out;
    if (*(const u32*)(hst + HStage::retry) != 0) RC(squares_hough_second(s, n, s->gray(), hc, L.hough, L.retry, back + FastLayout::o_hough, CBV_MAX_SQUARES));
    const cbv_sq_stats* st = (const cbv_sq_stats*)(back + FastLayout::o_stats);
    const cbv_hough_result* hg = (const cbv_hough_result*)(back + FastLayout::o_hough);
    const u8* fl = back + FastLayout::o_flags;
    for (int i = 0; i < n; i++) {
        cbv_piece_result r;
        memset(&r, 0, sizeof(r));
        bool uniform = false; // (np.std's verdict at a variance of exactly 225; everywhere else piece_decide's integer test is it)
        if ((fl[i] & CBV_GATE_EVALUATED) && piece_std_tie(&st[i])) RC(squares_uniform_at_tie(s, s->gray(), i, &uniform));
        if ((fl[i] & CBV_GATE_EVALUATED) && !uniform) { // detect_piece is evaluated for this square
            const bool hough_ran = (fl[i] & CBV_GATE_STD_OK) != 0;
            if (cbv_decide_piece(&st[i], hough_ran ? &hg[i] : nullptr, s->descs[i].w, s->descs[i].h, prm->circle_threshold, &r) != CBV_OK)
                return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "HoughCircles candidate list overflowed (more accumulator maxima than the second pass holds in a "
                                "%dx%d square)", s->descs[i].w, s->descs[i].h);
        }
        r.changed = (fl[i] & CBV_GATE_CHANGED) != 0;
        r.should_process = (fl[i] & CBV_GATE_PROCESS) != 0;
        r.evaluated = (fl[i] & CBV_GATE_EVALUATED) != 0;
        out[i] = r;
    }
    return CBV_DONE(CBV_OK);
}

extern "C" int cbv_squares_detect_changes(cbv_squares* s, const cbv_host_image* img, const cbv_roi* rois, int n, int blur_k,
                                          const cbv_change_params* prm, cbv_change_result* out)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    if (!prm || !out) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_squares_detect_changes: null argument");
    CBV_ENTER_DRAINED(ctx);
    if (!s->has_model) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_squares_detect_changes: not calibrated");
    RC(hough_params_check(ctx, &prm->hough));
    u8* hst;
    RC(ctx_hstage(ctx, HStage::bytes, &hst));
    const int old_n = s->n;
    RC(squares_stage_host_image(s, img, rois, n, blur_k, hst + HStage::descs));
    if (!s->has_model || s->n != old_n) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_squares_detect_changes: the squares' geometry changed since calibrate");
    FastLayout L;
    RC(fast_layout(s, &L));
    const bool five = s->blur_k == 5;
    if (five) {
        RC(squares_pre5_stats(s, n, s->gray(), s->mean(), s->sd(), (float)prm->z_threshold, L.stats, 0, nullptr, nullptr));
    } else {
        // the detector's own blur for the background model, and the squares as PieceDetector preprocesses them (k = 5)
        // for the is_circular test of the squares that changed
        RC(launch_squares_preprocess(ctx, s->staged(), 0, s->ddescs(), n, s->coef(), s->blur_k, s->gray(), 0, 1, max_px_of(s)));
        RC(launch_squares_stats(ctx, s->ddescs(), n, s->gray(), 0, nullptr, s->mean(), s->sd(), s->masks(), (float)prm->z_threshold, L.stats, 1));
        RC(dev_ensure(ctx, &s->d_gray5, s->plane_total));
        RC(squares_pre5_stats(s, n, s->d_gray5.as<u8>(), nullptr, nullptr, 0.f, L.stats5, 0, nullptr, nullptr));
    }
    u8* back = hst + HStage::out;
    CBV_HIP(ctx, hipMemcpyAsync(back + FastLayout::o_stats, L.stats, sizeof(cbv_sq_stats) * CBV_MAX_SQUARES * (five ? 1 : 2), hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const cbv_sq_stats* st = (const cbv_sq_stats*)(back + FastLayout::o_stats);
    const cbv_sq_stats* st5 = five ? st : (const cbv_sq_stats*)(back + FastLayout::o_stats5);
    // change_detector.py:124-150: squares of the selection whose share of changed pixels reaches 5 %
    u32* work = (u32*)(hst + HStage::work);
    int nwork = 0;
    u64 uniform_ties = 0; // reported squares of variance exactly 225 that np.std calls uniform
    for (int i = 0; i < n; i++) {
        cbv_change_result r;
        memset(&r, 0, sizeof(r));
        r.z_max = st[i].z_max;
        r.z_count = st[i].z_count;
        r.n = st[i].n;
        if ((prm->select >> i) & 1ull) {
            const double pct = ((double)st[i].z_count / (double)st[i].n) * 100.0;
            if (!(pct < 5.0)) {
                r.in_result = 1;
                r.intensity = pct > 75.0 ? 3 : (pct > 15.0 ? 2 : 1);
                bool uniform = piece_uniform(&st5[i]);
                if (piece_std_tie(&st5[i])) {
                    RC(squares_uniform_at_tie(s, five ? s->gray() : s->d_gray5.as<u8>(), i, &uniform));
                    if (uniform) uniform_ties |= 1ull << i;
                }
                if (!uniform) work[1 + nwork++] = (u32)i; // HoughCircles runs on it
            }
        }
        out[i] = r;
    }
    const cbv_hough_result* hg = (const cbv_hough_result*)(back + FastLayout::o_hough);
    if (nwork) {
        HoughCfg hc;
        RC(hough_cfg(ctx, &prm->hough, s->descs, &hc));
        work[0] = (u32)nwork;
        CBV_HIP(ctx, hipMemcpyAsync(L.work, work, sizeof(u32) * (1 + nwork), hipMemcpyHostToDevice, ctx->stream));
        CBV_HIP(ctx, hipMemsetAsync(L.retry, 0, sizeof(u32), ctx->stream));
        const u8* g5 = five ? s->gray() : s->d_gray5.as<u8>();
        RC(launch_hough(ctx, s->ddescs(), n, g5, 0, hc, L.hough, nullptr, L.work, 1, L.retry, 0));
        const u32* retry_back = (const u32*)(hst + HStage::retry_back);
        CBV_HIP(ctx, hipMemcpyAsync(hst + HStage::retry_back, L.retry, sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
        CBV_HIP(ctx, hipMemcpyAsync(back + FastLayout::o_hough, L.hough, sizeof(cbv_hough_result) * n, hipMemcpyDeviceToHost, ctx->stream));
        CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (*retry_back != 0) RC(squares_hough_second(s, n, g5, hc, L.hough, L.retry, back + FastLayout::o_hough, n));
    }
    for (int i = 0; i < n; i++) {
        if (!out[i].in_result || ((uniform_ties >> i) & 1ull)) continue;
        bool ran = false;
        for (int k = 0; k < nwork && !ran; k++) ran = work[1 + k] == (u32)i;
        cbv_piece_result pr;
        if (cbv_decide_piece(&st5[i], ran ? &hg[i] : nullptr, s->descs[i].w, s->descs[i].h, prm->circle_threshold, &pr) != CBV_OK)
            return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "HoughCircles candidate list overflowed in a %dx%d square", s->descs[i].w, s->descs[i].h);
        out[i].is_circular = pr.has_piece;
    }
    return CBV_DONE(CBV_OK);
}

static int squares_plane(cbv_squares* s, int which, int index, void** p, size_t* bytes)
{
    cbv_ctx* ctx = s->ctx;
    if (index < 0 || index >= s->n) return cbv_fail(ctx, CBV_ERR_ARG, "square index %d out of range", index);
    const SquareDesc& d = s->descs[index];
    size_t n = (size_t)d.w * d.h;
    switch (which) {
    case 0: *p = s->gray() + d.plane_off; *bytes = n; break;
    case 1: *p = s->ref() + d.plane_off; *bytes = n; break;
    case 2: *p = s->mean() + d.plane_off; *bytes = n * 4; break;
    case 3: *p = s->var() + d.plane_off; *bytes = n * 4; break;
    case 4: *p = s->sd() + d.plane_off; *bytes = n * 4; break; // sqrt(var) as the statistics kernels read it (read-only: cbv_squares_set)
    default: return cbv_fail(ctx, CBV_ERR_ARG, "bad plane selector %d", which);
    }
    return CBV_OK;
}

extern "C" int cbv_squares_get(cbv_squares* s, int which, int index, void* out)
{
    if (!s || !out) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    void* p;
    size_t bytes;
    CBV_ENTER_DRAINED(ctx);
    RC(squares_plane(s, which, index, &p, &bytes));
    CBV_HIP(ctx, hipMemcpyAsync(out, p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_DONE(CBV_OK);
}

extern "C" int cbv_squares_set(cbv_squares* s, int which, int index, const void* in)
{
    if (!s || !in) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    void* p;
    size_t bytes;
    CBV_ENTER_DRAINED(ctx);
    // plane 4 is derived from plane 3 (which refreshes it below): written on its own it would stop matching the variance
    if (which == 4) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_squares_set: plane 4 (sqrt of the variance) is read-only; write plane 3");
    RC(squares_plane(s, which, index, &p, &bytes));
    CBV_HIP(ctx, hipMemcpyAsync(p, in, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (which == 3) RC(launch_squares_refresh_sd(ctx, s->ddescs(), s->var(), s->sd(), index));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (which == 1) s->has_ref = true;
    return CBV_DONE(CBV_OK);
}

extern "C" int cbv_squares_geometry(cbv_squares* s, int index, int* w, int* h)
{
    if (!s || index < 0 || index >= s->n) return CBV_ERR_ARG;
    if (w) *w = s->descs[index].w;
    if (h) *h = s->descs[index].h;
    return CBV_OK;
}
