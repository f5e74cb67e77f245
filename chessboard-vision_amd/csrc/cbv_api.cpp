// C-ABI of libcbv_hip.so (include/cbv.h): context, host-buffer stage entry
// points and per-square detector state (the device-resident pipeline: cbv_pipeline*.cpp).
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <stdlib.h>

#include "cbv_internal.h"
#include "piece_sweep_core.h"
#include <memory>

thread_local std::string g_cbv_err;

int cbv_fail(cbv_ctx* ctx, int code, const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_cbv_err = buf;
    if (ctx) ctx->err = buf;
    return code;
}

int dev_ensure(cbv_ctx* ctx, DevBuf* b, size_t bytes)
{
    if (b->cap >= bytes && b->p) return CBV_OK;
    if (b->p) {
        CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        (void)hipFree(b->p);
        b->p = nullptr;
        b->cap = 0;
    }
    b->tag = 0;
    // whole 2 MiB units for anything large: the driver can then map the buffer with large GPU pages
    size_t cap = bytes >= (256u << 10) ? (bytes + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1) : (bytes + 4095) & ~(size_t)4095;
    CBV_HIP(ctx, hipMalloc(&b->p, cap));
    b->cap = cap;
    return CBV_OK;
}

int ctx_hstage(cbv_ctx* ctx, size_t bytes, u8** p)
{
    if (ctx->h_stage_cap < bytes) {
        if (ctx->h_stage) {
            CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
            (void)hipHostFree(ctx->h_stage);
        }
        ctx->h_stage = nullptr;
        ctx->h_stage_cap = 0;
        const size_t cap = (bytes + 65535) & ~(size_t)65535;
        CBV_HIP(ctx, hipHostMalloc((void**)&ctx->h_stage, cap, hipHostMallocDefault));
        ctx->h_stage_cap = cap;
    }
    *p = ctx->h_stage;
    return CBV_OK;
}

int ctx_worker_stream(cbv_ctx* ctx, hipStream_t* slot, hipStream_t* out)
{
    if (!*slot) CBV_HIP(ctx, hipStreamCreateWithFlags(slot, hipStreamNonBlocking));
    *out = *slot;
    return CBV_OK;
}

void dev_free(DevBuf* b)
{
    if (b->p) (void)hipFree(b->p);
    b->p = nullptr;
    b->cap = 0;
    b->tag = 0;
}

// ---------------------------------------------------------------------------
// profiling
// ---------------------------------------------------------------------------
static const char* kKernelNames[CBV_K_END] = {
    "k_color_lab_hist", "k_clahe_lut", "k_clahe_apply", "k_bilateral", "k_sharpen", "k_norm_lut", "k_normalize",
    "k_warp", "k_squares", "k_gray_blur_hist", "k_otsu", "k_threshold", "k_scan", "k_synth", "k_reset_aux", "k_hough", "k_ingest", "k_model_scan",
    "k_warp_yuv", "k_change_blur_stats"};

static hipEvent_t prof_get_event(cbv_ctx* ctx)
{
    if (!ctx->prof_pool.empty()) {
        hipEvent_t e = ctx->prof_pool.back();
        ctx->prof_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

void prof_begin(cbv_ctx* ctx, int kid)
{
    if (ctx->prof_kid == -2 || (ctx->prof_kid != -1 && ctx->prof_kid != kid)) return;
    ProfSlot s;
    s.kid = kid;
    s.a = prof_get_event(ctx);
    s.b = prof_get_event(ctx);
    (void)hipEventRecord(s.a, ctx->stream);
    ctx->prof_pending.push_back(s);
}

void prof_end(cbv_ctx* ctx, int kid)
{
    if (ctx->prof_kid == -2 || (ctx->prof_kid != -1 && ctx->prof_kid != kid)) return;
    if (ctx->prof_pending.empty()) return;
    (void)hipEventRecord(ctx->prof_pending.back().b, ctx->stream);
}

static void prof_drain(cbv_ctx* ctx)
{
    for (auto& s : ctx->prof_pending) {
        float ms = 0;
        if (hipEventSynchronize(s.b) == hipSuccess && hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) {
            ctx->prof_ms[s.kid] += ms;
            ctx->prof_n[s.kid] += 1;
        }
        ctx->prof_pool.push_back(s.a);
        ctx->prof_pool.push_back(s.b);
    }
    ctx->prof_pending.clear();
}

extern "C" int cbv_profile_enable(cbv_ctx* ctx, int kid)
{
    if (!ctx) return CBV_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    prof_drain(ctx);
    ctx->prof_kid = kid;
    return CBV_OK;
}

extern "C" int cbv_profile_read(cbv_ctx* ctx, int kid, double* total_ms, long long* launches)
{
    if (!ctx || kid < 0 || kid >= CBV_K_END) return CBV_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    prof_drain(ctx);
    if (total_ms) *total_ms = ctx->prof_ms[kid];
    if (launches) *launches = ctx->prof_n[kid];
    return CBV_OK;
}

extern "C" int cbv_profile_reset(cbv_ctx* ctx)
{
    if (!ctx) return CBV_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    prof_drain(ctx);
    for (int i = 0; i < CBV_K_END; i++) {
        ctx->prof_ms[i] = 0;
        ctx->prof_n[i] = 0;
    }
    return CBV_OK;
}

extern "C" const char* cbv_kernel_name(int kid) { return (kid >= 0 && kid < CBV_K_END) ? kKernelNames[kid] : ""; }

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
extern "C" int cbv_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" const char* cbv_last_error(const cbv_ctx* ctx) { return ctx ? ctx->err.c_str() : g_cbv_err.c_str(); }
extern "C" const char* cbv_device_name(const cbv_ctx* ctx) { return ctx ? ctx->devname : ""; }

extern "C" int cbv_ctx_create(int device_id, cbv_ctx** out)
{
    if (!out) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_ctx_create: out is null");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return cbv_fail(nullptr, CBV_ERR_NODEV, "no HIP device available (%s); this library has no CPU fallback",
                        e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device_id < 0 || device_id >= n) return cbv_fail(nullptr, CBV_ERR_ARG, "device %d out of range (%d devices)", device_id, n);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return cbv_fail(nullptr, CBV_ERR_HIP, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return cbv_fail(nullptr, CBV_ERR_NODEV, "device %d is %s; libcbv_hip.so carries gfx950 (MI355X) code only", device_id,
                        prop.gcnArchName);
    cbv_ctx* ctx = new cbv_ctx();
    ctx->device = device_id;
    ctx->num_cus = prop.multiProcessorCount;
    snprintf(ctx->devname, sizeof(ctx->devname), "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
#define CK(call)                                                                                       \
    do {                                                                                               \
        hipError_t e2 = (call);                                                                        \
        if (e2 != hipSuccess) {                                                                        \
            int rc = cbv_fail(nullptr, CBV_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e2));    \
            delete ctx;                                                                                \
            return rc;                                                                                 \
        }                                                                                              \
    } while (0)
    CK(hipSetDevice(device_id));
    CK(hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
    ctx->stream = ctx->own_stream;
    CK(hipMalloc((void**)&ctx->tabs, sizeof(StaticTabs)));
    CK(hipMalloc((void**)&ctx->ptabs, sizeof(ProfileTabs)));
    CK(hipMalloc((void**)&ctx->btabs, sizeof(BilateralTabs)));
    {
        StaticTabs* st = new StaticTabs();
        build_static_tabs(st);
        hipError_t up = hipMemcpy(ctx->tabs, st, sizeof(StaticTabs), hipMemcpyHostToDevice);
        delete st;
        CK(up);
        cbv_color_profile none;
        memset(&none, 0, sizeof(none));
        ProfileTabs pt;
        build_profile_tabs(&none, &pt);
        CK(hipMemcpy(ctx->ptabs, &pt, sizeof(pt), hipMemcpyHostToDevice));
        ctx->ptabs_key = none;
        ctx->ptabs_valid = true;
    }
#undef CK
    *out = ctx;
    return CBV_OK;
}

extern "C" void cbv_ctx_destroy(cbv_ctx* ctx)
{
    if (!ctx) return;
    {
        std::lock_guard<std::recursive_mutex> lock(ctx->mu); // a call still running on another thread finishes first
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        prof_drain(ctx);
    }
    for (auto e : ctx->prof_pool) (void)hipEventDestroy(e);
    dev_free(&ctx->in);
    dev_free(&ctx->a);
    dev_free(&ctx->b);
    dev_free(&ctx->c);
    dev_free(&ctx->small);
    if (ctx->tabs) (void)hipFree(ctx->tabs);
    if (ctx->ptabs) (void)hipFree(ctx->ptabs);
    if (ctx->btabs) (void)hipFree(ctx->btabs);
    if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
    for (auto& st : ctx->lane_streams)
        if (st) (void)hipStreamDestroy(st);
    if (ctx->scan_stream) (void)hipStreamDestroy(ctx->scan_stream);
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

extern "C" int cbv_ctx_set_stream(cbv_ctx* ctx, void* hip_stream)
{
    if (!ctx) return CBV_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu); // cbv_pipeline_run repoints ctx->stream while it enqueues
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return CBV_OK;
}

extern "C" int cbv_ctx_synchronize(cbv_ctx* ctx)
{
    if (!ctx) return CBV_ERR_ARG;
    hipStream_t st;
    {
        CBV_ENTER(ctx);
        st = ctx->stream; // the caller's stream, never a lane a concurrent cbv_pipeline_run points at for the moment
    }
    CBV_HIP(ctx, hipStreamSynchronize(st));
    return CBV_OK;
}

int ctx_set_profile(cbv_ctx* ctx, const cbv_color_profile* p)
{
    cbv_color_profile key;
    memset(&key, 0, sizeof(key));
    if (p) {
        key.hue_shift = p->hue_shift;
        key.sat_scale = p->sat_scale;
        key.val_scale = p->val_scale;
        key.contrast = p->contrast;
        key.brightness = p->brightness;
        key.radical_mode = p->radical_mode ? 1 : 0;
        key.target_hue = p->target_hue;
        key.hue_window = p->hue_window;
        key.enabled = p->enabled ? 1 : 0;
    }
    if (ctx->ptabs_valid && memcmp(&key, &ctx->ptabs_key, sizeof(key)) == 0) return CBV_OK;
    ProfileTabs pt;
    build_profile_tabs(&key, &pt);
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    CBV_HIP(ctx, hipMemcpy(ctx->ptabs, &pt, sizeof(pt), hipMemcpyHostToDevice));
    ctx->ptabs_key = key;
    ctx->ptabs_valid = true;
    return CBV_OK;
}

// the tables of a profile that belongs to a pipeline or a call (k_warp_profile), never ctx->ptabs: the profile as
// ctx_set_profile reads it (flags as 0 / 1), null = disabled
int profile_tabs_checked(cbv_ctx* ctx, const cbv_color_profile* p, ProfileTabs* out, const char* who)
{
    cbv_color_profile key;
    memset(&key, 0, sizeof(key));
    if (p && p->enabled) {
        const double v[7] = {p->hue_shift, p->sat_scale, p->val_scale, p->contrast, p->brightness, p->target_hue, p->hue_window};
        for (double x : v)
            if (!std::isfinite(x)) return cbv_fail(ctx, CBV_ERR_ARG, "%s: a field of the colour profile is not finite", who);
        key = *p;
        key.radical_mode = p->radical_mode ? 1 : 0;
        key.enabled = 1;
    }
    build_profile_tabs(&key, out);
    return CBV_OK;
}

int ctx_set_bilateral(cbv_ctx* ctx, int d, double sc, double ss)
{
    if (ctx->b_d == d && ctx->b_sc == sc && ctx->b_ss == ss) return CBV_OK;
    if (build_bilateral_tabs(d, sc, ss, &ctx->btabs_host) != 0)
        return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "bilateral d=%d not supported (radius <= 4)", d);
    if (ctx->btabs_host.radius > 4) return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "bilateral d=%d not supported (radius <= 4)", d);
    ctx->btabs_offsets_bad = bilateral_offsets_mismatch(&ctx->btabs_host);
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    CBV_HIP(ctx, hipMemcpy(ctx->btabs, &ctx->btabs_host, sizeof(BilateralTabs), hipMemcpyHostToDevice));
    ctx->b_d = d;
    ctx->b_sc = sc;
    ctx->b_ss = ss;
    return CBV_OK;
}

// ---------------------------------------------------------------------------
// host-buffer stage entry points
// ---------------------------------------------------------------------------
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
    CBV_ENTER(ctx);
    RC(upload(ctx, &ctx->in, bgr, w * 3, h, stride));
    if (!profile->enabled) return download(ctx, ctx->in.p, out, w * 3, h, out_stride); // `{}` profile: identity
    RC(ctx_set_profile(ctx, profile));
    Geom g = tight_geom(w, h);
    RC(dev_ensure(ctx, &ctx->a, g.frame_stride));
    SmallLayout S;
    RC(small_layout(ctx, &ctx->small, 1, 1, &S));
    S.owner->tag = 0;
    ClaheGeom cg = clahe_geom(w, h, 0.0, 1, 1); // one tile = whole image; only used for the traversal
    RC(launch_color_lab_hist(ctx, (const u8*)ctx->in.p, (u8*)ctx->a.p, S.aux, g, cg, 1, 1, 0));
    return download(ctx, ctx->a.p, out, w * 3, h, out_stride);
}

extern "C" int cbv_correct_lighting(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, double clip_limit,
                                    int tiles_x, int tiles_y, uint8_t* out, int out_stride)
{
    RC(check_img(ctx, bgr, w, h, stride, 3, "cbv_correct_lighting"));
    if (!out || tiles_x <= 0 || tiles_y <= 0 || tiles_x > 64 || tiles_y > 64) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_correct_lighting: bad arguments");
    CBV_ENTER(ctx);
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
    return download(ctx, ctx->b.p, out, w * 3, h, out_stride);
}

extern "C" int cbv_clahe_apply(cbv_ctx* ctx, const uint8_t* gray, int w, int h, int stride, double clip_limit, int tiles_x,
                               int tiles_y, uint8_t* out, int out_stride)
{
    RC(check_img(ctx, gray, w, h, stride, 1, "cbv_clahe_apply"));
    if (!out || tiles_x <= 0 || tiles_y <= 0 || tiles_x > 64 || tiles_y > 64) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_clahe_apply: bad arguments");
    CBV_ENTER(ctx);
    RC(upload(ctx, &ctx->in, gray, w, h, stride));
    RC(dev_ensure(ctx, &ctx->a, ((size_t)w * h + 255) & ~(size_t)255));
    ClaheGeom cg = clahe_geom(w, h, clip_limit, tiles_x, tiles_y);
    SmallLayout S;
    RC(small_layout(ctx, &ctx->small, tiles_x * tiles_y, 1, &S));
    S.owner->tag = 0;
    RC(launch_clahe_gray(ctx, (const u8*)ctx->in.p, w, h, w, cg, S.aux, S.luts, (u8*)ctx->a.p));
    return download(ctx, ctx->a.p, out, w, h, out_stride);
}

extern "C" int cbv_reduce_noise(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, int d, double sigma_color,
                                double sigma_space, uint8_t* out, int out_stride)
{
    RC(check_img(ctx, bgr, w, h, stride, 3, "cbv_reduce_noise"));
    if (!out) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_reduce_noise: out is null");
    CBV_ENTER(ctx);
    RC(ctx_set_bilateral(ctx, d, sigma_color, sigma_space));
    RC(upload(ctx, &ctx->in, bgr, w * 3, h, stride));
    Geom g = tight_geom(w, h);
    RC(dev_ensure(ctx, &ctx->a, g.frame_stride));
    RC(launch_bilateral(ctx, (const u8*)ctx->in.p, (u8*)ctx->a.p, g, 1));
    return download(ctx, ctx->a.p, out, w * 3, h, out_stride);
}

extern "C" int cbv_sharpen(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, const float* kernel9, uint8_t* out,
                           int out_stride)
{
    RC(check_img(ctx, bgr, w, h, stride, 3, "cbv_sharpen"));
    if (!out || !kernel9) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_sharpen: null argument");
    CBV_ENTER(ctx);
    RC(upload(ctx, &ctx->in, bgr, w * 3, h, stride));
    Geom g = tight_geom(w, h);
    RC(dev_ensure(ctx, &ctx->a, g.frame_stride));
    SmallLayout S;
    RC(small_layout(ctx, &ctx->small, 1, 1, &S));
    RC(aux_reset(ctx, S, 1, 1));
    RC(launch_sharpen(ctx, (const u8*)ctx->in.p, (u8*)ctx->a.p, S.aux, 1, g, kernel9, 1));
    return download(ctx, ctx->a.p, out, w * 3, h, out_stride);
}

int launch_minmax(cbv_ctx* ctx, const u8* src, u32* aux, int tiles, Geom g, int batch);

extern "C" int cbv_normalize_intensity(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, uint8_t* out,
                                       int out_stride)
{
    RC(check_img(ctx, bgr, w, h, stride, 3, "cbv_normalize_intensity"));
    if (!out) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_normalize_intensity: out is null");
    CBV_ENTER(ctx);
    RC(upload(ctx, &ctx->in, bgr, w * 3, h, stride));
    Geom g = tight_geom(w, h);
    RC(dev_ensure(ctx, &ctx->a, g.frame_stride));
    SmallLayout S;
    RC(small_layout(ctx, &ctx->small, 1, 1, &S));
    RC(aux_reset(ctx, S, 1, 1));
    RC(launch_minmax(ctx, (const u8*)ctx->in.p, S.aux, 1, g, 1));
    RC(launch_normalize(ctx, (const u8*)ctx->in.p, (u8*)ctx->a.p, norm_from_minmax(S.aux, 1), g, 1));
    return download(ctx, ctx->a.p, out, w * 3, h, out_stride);
}

extern "C" int cbv_prepare_analysis(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, uint8_t* gray,
                                    int gray_stride, uint8_t* binary, int binary_stride, int* otsu_threshold)
{
    RC(check_img(ctx, bgr, w, h, stride, 3, "cbv_prepare_analysis"));
    if (!gray || !binary) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_prepare_analysis: null output");
    CBV_ENTER(ctx);
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
    return CBV_OK;
}

extern "C" int cbv_canny(cbv_ctx* ctx, const uint8_t* img, int w, int h, int stride, int cn, double threshold1, double threshold2,
                         uint8_t* edges, int edges_stride)
{
    RC(check_img(ctx, img, w, h, stride, cn, "cbv_canny"));
    if (!edges || (cn != 1 && cn != 3)) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_canny: null output or unsupported channel count");
    CBV_ENTER(ctx);
    RC(upload(ctx, &ctx->in, img, w * cn, h, stride));
    // cv::Canny: thresholds are ordered, then floored (L1 gradient)
    double lo = threshold1 < threshold2 ? threshold1 : threshold2, hi = threshold1 < threshold2 ? threshold2 : threshold1;
    const int low = (int)floor(lo), high = (int)floor(hi);
    size_t plane = ((size_t)w * h + 255) & ~(size_t)255;
    RC(dev_ensure(ctx, &ctx->a, plane));
    RC(launch_canny(ctx, (const u8*)ctx->in.p, w, h, w * cn, cn, low, high, (u8*)ctx->a.p, &ctx->b));
    RC(rows_d2h(ctx, edges, edges_stride, ctx->a.p, w, h));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
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
    CBV_ENTER(ctx);
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
    return board_corners_from_edges(host.data(), w, h, pts8, &n_contours);
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
    CBV_ENTER(ctx);
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
    return download(ctx, res, out, w * 3, h, out_stride);
}

extern "C" int cbv_warp_perspective(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, const double* M9, int dw,
                                    int dh, int rot180, uint8_t* out, int out_stride)
{
    RC(check_img(ctx, bgr, w, h, stride, 3, "cbv_warp_perspective"));
    if (!out || !M9 || dw <= 0 || dh <= 0 || dw > 8192 || dh > 8192) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_warp_perspective: bad arguments");
    CBV_ENTER(ctx);
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
    static const bool tm = getenv("CBV_TIMING") != nullptr;
    auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = tm ? now() : 0;
    RC(rows_h2d(ctx, (u8*)ctx->in.p + (size_t)y0 * w * 3, bgr + (size_t)y0 * stride, stride, w * 3, y1 - y0));
    const double t1 = tm ? now() : 0;
    Geom g = tight_geom(w, h);
    RC(dev_ensure(ctx, &ctx->a, (size_t)dw * dh * 3 + 256));
    RC(launch_warp(ctx, warp_src_bgr((const u8*)ctx->in.p, g, NormSrc()), Minv, dw, dh, rot180, (u8*)ctx->a.p, dw * 3, (size_t)dw * dh * 3, 1));
    const double t2 = tm ? now() : 0;
    RC(rows_d2h(ctx, out, out_stride, ctx->a.p, dw * 3, dh));
    const double t3 = tm ? now() : 0;
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (tm) fprintf(stderr, "warp: h2d %.1f launch %.1f d2h %.1f sync %.1f us (rows %d..%d)\n", t1 - t0, t2 - t1, t3 - t2, now() - t3, y0, y1);
    return CBV_OK;
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
    CBV_ENTER(ctx);
    double Minv[9];
    if (!host_invert3x3(M9, Minv)) memset(Minv, 0, sizeof(Minv));
    RC(upload(ctx, &ctx->in, bgr, w * 3, h, stride));
    RC(dev_ensure(ctx, &ctx->a, (size_t)dw * dh * 3 + 256));
    RC(dev_ensure(ctx, &ctx->b, sizeof(ProfileTabs))); // the call's tables
    CBV_HIP(ctx, hipMemcpyAsync(ctx->b.p, &pt, sizeof(pt), hipMemcpyHostToDevice, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (pt is on this stack)
    RC(launch_warp(ctx, warp_src_profile((const u8*)ctx->in.p, tight_geom(w, h), (const ProfileTabs*)ctx->b.p), Minv, dw, dh, rot180, (u8*)ctx->a.p,
                   dw * 3, (size_t)dw * dh * 3, 1));
    return download(ctx, ctx->a.p, out, dw * 3, dh, out_stride);
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
    const int n = raw_fmt_planes(raw->fmt);
    planes[0] = raw->plane0, strides[0] = raw->stride0;
    planes[1] = n > 1 ? raw->plane1 : nullptr, strides[1] = n > 1 ? raw->stride1 : 0;
    planes[2] = n > 2 ? raw->plane2 : nullptr, strides[2] = n > 2 ? raw->stride2 : 0;
}

int raw_h2d_stage(cbv_ctx* ctx, const cbv_raw_frame* raw, int w, int h, RawPlanes* dev_out, RawGeom* r_out, const char* what)
{
    RC(check_raw_format(ctx, raw->fmt, w, h, what));
    const u8* planes[3];
    int strides[3];
    raw_frame_planes(raw, planes, strides);
    RC(check_raw_planes(ctx, raw->fmt, w, planes, strides, what));
    if ((size_t)w * h > (size_t)1 << 28) return cbv_fail(ctx, CBV_ERR_ARG, "%s: image too large", what);
    // a plane follows the largest possible device copy of the one before (rows of twice their length), on a 256-byte boundary
    const int np = raw_fmt_planes(raw->fmt);
    size_t off[4] = {0, 0, 0, 0};
    for (int i = 0; i < np; i++)
        off[i + 1] = (off[i] + (size_t)2 * raw_plane_wbytes(raw->fmt, w, i) * raw_plane_rows(raw->fmt, h, i) + 255) & ~(size_t)255;
    const size_t total = off[np];
    RC(dev_ensure(ctx, &ctx->in, total + 256));
    if (ctx->debug_poison) CBV_HIP(ctx, hipMemsetAsync(ctx->in.p, 0xA5, total, ctx->stream));
    RawGeom r = {};
    r.fmt = raw->fmt;
    u8* st = (u8*)ctx->in.p;
    RawPlanes dev = {{nullptr, nullptr, nullptr}};
    int dev_stride[3] = {0, 0, 0};
    for (int i = 0; i < np; i++) {
        RC(plane_h2d(ctx, st + off[i], planes[i], strides[i], raw_plane_wbytes(raw->fmt, w, i), raw_plane_rows(raw->fmt, h, i), &dev_stride[i]));
        dev.p[i] = st + off[i];
    }
    r.stride0 = dev_stride[0], r.stride1 = dev_stride[1], r.stride2 = dev_stride[2];
    *dev_out = dev;
    *r_out = r;
    return CBV_OK;
}

int raw_h2d_convert(cbv_ctx* ctx, const cbv_raw_frame* raw, int w, int h, u8* dst, Geom g, const char* what)
{
    RawPlanes dev;
    RawGeom r;
    RC(raw_h2d_stage(ctx, raw, w, h, &dev, &r, what));
    return launch_ingest(ctx, dev, r, dst, g, 1);
}

extern "C" int cbv_yuv_to_bgr(cbv_ctx* ctx, const cbv_raw_frame* raw, int w, int h, uint8_t* bgr, int bgr_stride)
{
    if (!ctx) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_yuv_to_bgr: ctx is null");
    if (!raw || !bgr || w <= 0 || h <= 0 || bgr_stride < w * 3) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_yuv_to_bgr: bad arguments");
    RC(check_raw_format(ctx, raw->fmt, w, h, "cbv_yuv_to_bgr"));
    CBV_ENTER(ctx);
    const Geom g = tight_geom(w, h);
    RC(dev_ensure(ctx, &ctx->a, g.frame_stride));
    RC(raw_h2d_convert(ctx, raw, w, h, (u8*)ctx->a.p, g, "cbv_yuv_to_bgr"));
    return download(ctx, ctx->a.p, bgr, w * 3, h, bgr_stride);
}

extern "C" int cbv_warp_color_profile_raw(cbv_ctx* ctx, const cbv_raw_frame* raw, int w, int h, const cbv_color_profile* profile, const double* M9,
                                          int dw, int dh, int rot180, uint8_t* out, int out_stride)
{
    const char* who = "cbv_warp_color_profile_raw";
    if (!ctx) return cbv_fail(nullptr, CBV_ERR_ARG, "%s: ctx is null", who);
    if (!raw || !out || !M9 || !profile || w <= 0 || h <= 0 || dw <= 0 || dh <= 0 || dw > 8192 || dh > 8192 || out_stride < dw * 3)
        return cbv_fail(ctx, CBV_ERR_ARG, "%s: bad arguments", who);
    RC(check_raw_format(ctx, raw->fmt, w, h, who)); // (a BGR frame goes to cbv_warp_color_profile)
    ProfileTabs pt;
    RC(profile_tabs_checked(ctx, profile, &pt, who));
    CBV_ENTER(ctx);
    double Minv[9];
    if (!host_invert3x3(M9, Minv)) memset(Minv, 0, sizeof(Minv));
    RawPlanes dev;
    RawGeom r;
    RC(raw_h2d_stage(ctx, raw, w, h, &dev, &r, who)); // (the staging buffer keeps 256 bytes behind the last plane: the wide loads' slack)
    RC(dev_ensure(ctx, &ctx->a, (size_t)dw * dh * 3 + 256));
    Geom g = tight_geom(w, h);
    WarpSrc src = warp_src_raw(dev, r, g); // a disabled profile: the plain raw warp
    if (profile->enabled) {
        RC(dev_ensure(ctx, &ctx->b, sizeof(ProfileTabs))); // the call's tables
        CBV_HIP(ctx, hipMemcpyAsync(ctx->b.p, &pt, sizeof(pt), hipMemcpyHostToDevice, ctx->stream));
        CBV_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (pt is on this stack)
        src = warp_src_raw_profile(dev, r, g, (const ProfileTabs*)ctx->b.p);
    }
    RC(launch_warp(ctx, src, Minv, dw, dh, rot180, (u8*)ctx->a.p, dw * 3, (size_t)dw * dh * 3, 1));
    return download(ctx, ctx->a.p, out, dw * 3, dh, out_stride);
}

// ---------------------------------------------------------------------------
// per-square detector state
// ---------------------------------------------------------------------------
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

// np.sqrt(var) of every pixel, kept beside the variance plane by the kernels that write it
static float* sq_sd(cbv_squares* s) { return (float*)s->d_var.p + s->plane_total; }

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
    RC(dev_ensure(ctx, &s->d_var, off * 8)); // variance plane, then its square root (sq_sd)
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
    CBV_ENTER(ctx);
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
    RC(launch_squares_preprocess(ctx, (const u8*)s->d_stage.p, 0, (const SquareDesc*)s->d_descs.p, n, (const int*)s->d_coef.p,
                                 s->blur_k, (u8*)s->d_gray.p, 0, 1));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

extern "C" int cbv_squares_load_dev(cbv_squares* s, const void* dev_img, int w, int h, int stride, int cn,
                                    const cbv_roi* rois, int n, int blur_k)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    if (!dev_img || !rois || n <= 0 || n > CBV_MAX_SQUARES || (cn != 1 && cn != 3)) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_squares_load_dev: bad arguments");
    CBV_ENTER(ctx);
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
    RC(launch_squares_preprocess(ctx, (const u8*)dev_img, 0, (const SquareDesc*)s->d_descs.p, n, (const int*)s->d_coef.p, s->blur_k,
                                 (u8*)s->d_gray.p, 0, 1));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

static int squares_select(cbv_squares* s, const uint8_t* select, const u8** dev)
{
    *dev = nullptr;
    if (!select) return CBV_OK;
    cbv_ctx* ctx = s->ctx;
    CBV_HIP(ctx, hipMemcpyAsync(s->d_select.p, select, s->n, hipMemcpyHostToDevice, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *dev = (const u8*)s->d_select.p;
    return CBV_OK;
}

extern "C" int cbv_squares_calibrate(cbv_squares* s, double initial_variance, const uint8_t* select)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    CBV_ENTER(ctx);
    if (s->n == 0) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_squares_calibrate: no squares loaded");
    const u8* sel;
    RC(squares_select(s, select, &sel));
    RC(launch_squares_calibrate(ctx, (const SquareDesc*)s->d_descs.p, s->n, (const u8*)s->d_gray.p, (float*)s->d_mean.p, (float*)s->d_var.p,
                                sq_sd(s), (float)initial_variance, sel));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->has_model = true;
    return CBV_OK;
}

extern "C" int cbv_squares_ema(cbv_squares* s, double alpha, const uint8_t* select)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    CBV_ENTER(ctx);
    if (!s->has_model) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_squares_ema: not calibrated");
    const u8* sel;
    RC(squares_select(s, select, &sel));
    RC(launch_squares_ema(ctx, (const SquareDesc*)s->d_descs.p, s->n, (const u8*)s->d_gray.p, (float*)s->d_mean.p, (float*)s->d_var.p, sq_sd(s), alpha, sel));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

extern "C" int cbv_squares_set_ref(cbv_squares* s, const uint8_t* select)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    CBV_ENTER(ctx);
    if (s->n == 0) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_squares_set_ref: no squares loaded");
    const u8* sel;
    RC(squares_select(s, select, &sel));
    RC(launch_squares_set_ref(ctx, (const SquareDesc*)s->d_descs.p, s->n, (const u8*)s->d_gray.p, (u8*)s->d_ref.p, sel));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->has_ref = true;
    return CBV_OK;
}

extern "C" int cbv_squares_stats(cbv_squares* s, int use_ref, int use_model, double z_threshold, cbv_sq_stats* out)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    CBV_ENTER(ctx);
    if (!out || s->n == 0) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_squares_stats: no squares loaded or null output");
    if (use_model && !s->has_model) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_squares_stats: model requested but not calibrated");
    RC(launch_squares_stats(ctx, (const SquareDesc*)s->d_descs.p, s->n, (const u8*)s->d_gray.p, 0, use_ref ? (const u8*)s->d_ref.p : nullptr,
                            use_model ? (const float*)s->d_mean.p : nullptr, use_model ? (const float*)sq_sd(s) : nullptr,
                            (const u8*)s->d_masks.p, (float)z_threshold, (cbv_sq_stats*)s->d_stats.p, 1));
    CBV_HIP(ctx, hipMemcpyAsync(out, s->d_stats.p, sizeof(cbv_sq_stats) * s->n, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
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

extern "C" int cbv_squares_hough(cbv_squares* s, const cbv_hough_params* prm, cbv_hough_result* out)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    CBV_ENTER(ctx);
    if (!out || s->n == 0) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_squares_hough: no squares loaded or null output");
    HoughCfg hc;
    RC(hough_cfg(ctx, prm, s->descs, &hc));
    RC(dev_ensure(ctx, &s->d_hough, sizeof(cbv_hough_result) * CBV_MAX_SQUARES));
    RC(dev_ensure(ctx, &s->d_retry, sizeof(u32) * (1 + CBV_MAX_SQUARES)));
    CBV_HIP(ctx, hipMemsetAsync(s->d_retry.p, 0, sizeof(u32), ctx->stream));
    RC(launch_hough(ctx, (const SquareDesc*)s->d_descs.p, s->n, (const u8*)s->d_gray.p, 0, hc, (cbv_hough_result*)s->d_hough.p, nullptr, nullptr, 1,
                    (u32*)s->d_retry.p, 0));
    RC(launch_hough_second(ctx, (const SquareDesc*)s->d_descs.p, s->n, (const u8*)s->d_gray.p, 0, hc, (cbv_hough_result*)s->d_hough.p, nullptr,
                           (const u32*)s->d_retry.p, s->n));
    CBV_HIP(ctx, hipMemcpyAsync(out, s->d_hough.p, sizeof(cbv_hough_result) * s->n, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

// ---------------------------------------------------------------------------
// one call per frame for the reference's own call pattern (game_session.py:124-161, calibrate_sensitivity.py:142-157):
// the 64 squares are views of ONE host image (split_board of the warped board), so the image's bounding rows are
// uploaded with one copy AT CALL TIME (nothing stale, no host pointer kept) and everything up to the per-square records
// runs behind it with one wait at the end.
// ---------------------------------------------------------------------------
extern "C" int cbv_debug_poison(cbv_ctx* ctx, int on)
{
    if (!ctx) return CBV_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    ctx->debug_poison = on ? 1 : 0;
    return CBV_OK;
}

// Not in include/cbv.h: for tests/test_bilateral_offsets_host.py, which needs no device.  Builds the bilateral tables of
// (d, sigma_color, sigma_space) on the host and returns the number of taps whose table offset differs from the one the
// batched d = 9 kernel carries as a compile-time constant (the check launch_bilateral makes); -1: radius not supported.
extern "C" CBV_API int cbv_debug_bilateral_offsets(int d, double sigma_color, double sigma_space)
{
    auto t = std::make_unique<BilateralTabs>();
    if (build_bilateral_tabs(d, sigma_color, sigma_space, t.get()) != 0 || t->radius > 4) return -1;
    return bilateral_offsets_mismatch(t.get());
}

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

extern "C" int cbv_squares_load_image(cbv_squares* s, const cbv_host_image* img, const cbv_roi* rois, int n, int blur_k)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    CBV_ENTER(ctx);
    u8* hst;
    RC(ctx_hstage(ctx, 65536, &hst));
    RC(squares_stage_host_image(s, img, rois, n, blur_k, hst));
    RC(launch_squares_preprocess(ctx, (const u8*)s->d_stage.p, 0, (const SquareDesc*)s->d_descs.p, n, (const int*)s->d_coef.p, s->blur_k,
                                 (u8*)s->d_gray.p, 0, 1, max_px_of(s)));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the host image (and the pinned descriptors) are free again
    return CBV_OK;
}

extern "C" int cbv_squares_set_ref_mask(cbv_squares* s, uint64_t mask)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    CBV_ENTER(ctx);
    if (s->n == 0) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_squares_set_ref_mask: no squares loaded");
    RC(launch_squares_set_ref_mask(ctx, (const SquareDesc*)s->d_descs.p, s->n, (const u8*)s->d_gray.p, (u8*)s->d_ref.p, mask));
    s->has_ref = true;
    return CBV_OK; // asynchronous: later calls on this context are ordered behind it
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

// device scratch of the one-call entry points: worklist | retry list | then everything that travels back to the host as
// ONE copy: gate flags | statistics | second statistics set (k = 5 planes) | HoughCircles records
struct FastLayout {
    u32* work;
    u32* retry;
    u8* out;       // start of the block that is copied back
    u8* dflags;
    cbv_sq_stats* stats;
    cbv_sq_stats* stats5;
    cbv_hough_result* hough;
    size_t o_flags, o_stats, o_stats5, o_hough, out_bytes; // offsets inside the block
};
static int fast_layout(cbv_squares* s, FastLayout* L)
{
    const size_t o_retry = 512, o_out = 1024; // (cbv_squares_detect_all copies [retry, out + out_bytes) back as one block)
    // the block is copied back to offset 8192 of the 64 KB pinned staging area, whose tail (from 40960) holds the host-built worklist
    static_assert(8192 + 64 + (2 * sizeof(cbv_sq_stats) + sizeof(cbv_hough_result)) * CBV_MAX_SQUARES <= 40960, "result block overruns the staging area");
    static_assert(sizeof(SquareDesc) * CBV_MAX_SQUARES <= 8192 && 40960 + 4 * (1 + CBV_MAX_SQUARES) <= 65536, "staging layout");
    L->o_flags = 0;
    L->o_stats = 64;
    L->o_stats5 = L->o_stats + sizeof(cbv_sq_stats) * CBV_MAX_SQUARES;
    L->o_hough = L->o_stats5 + sizeof(cbv_sq_stats) * CBV_MAX_SQUARES;
    L->out_bytes = L->o_hough + sizeof(cbv_hough_result) * CBV_MAX_SQUARES;
    RC(dev_ensure(s->ctx, &s->d_fast, o_out + L->out_bytes));
    u8* b = (u8*)s->d_fast.p;
    L->work = (u32*)b;
    L->retry = (u32*)(b + o_retry);
    L->out = b + o_out;
    L->dflags = L->out + L->o_flags;
    L->stats = (cbv_sq_stats*)(L->out + L->o_stats);
    L->stats5 = (cbv_sq_stats*)(L->out + L->o_stats5);
    L->hough = (cbv_hough_result*)(L->out + L->o_hough);
    return CBV_OK;
}

extern "C" int cbv_squares_detect_all(cbv_squares* s, const cbv_host_image* img, const cbv_roi* rois, int n,
                                      const cbv_detect_params* prm, cbv_piece_result* out)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    if (!prm || !out) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_squares_detect_all: null argument");
    CBV_ENTER(ctx);
    RC(hough_params_check(ctx, &prm->hough)); // before anything of the set changes
    u8* hst;
    const size_t o_back = 8192; // the descriptors (64 x 64 B) are staged in front of it
    RC(ctx_hstage(ctx, 65536, &hst));
    FastLayout L;
    RC(fast_layout(s, &L));
    // worklist and retry counters; in front of the upload, whose host-blocking copy would otherwise leave the GPU idle
    // while this launch is submitted
    CBV_HIP(ctx, hipMemsetAsync(s->d_fast.p, 0, 1024, ctx->stream));
    RC(squares_stage_host_image(s, img, rois, n, 5, hst));
    HoughCfg hc;
    RC(hough_cfg(ctx, &prm->hough, s->descs, &hc));
    DetectMasks dm;
    dm.has_ref = s->has_ref ? prm->has_ref : 0;
    dm.cached = prm->cached;
    dm.check = prm->check;
    dm.check_given = prm->check_given;
    dm.use_delta = prm->use_delta;
    dm.change_threshold = prm->change_threshold;
    dm.dflags = L.dflags;
    // preprocess + statistics (+ |gray - reference|) + the gate, one launch; HoughCircles over the squares it listed
    RC(launch_squares_pre5_stats(ctx, (const u8*)s->d_stage.p, 0, (const SquareDesc*)s->d_descs.p, n, (u8*)s->d_gray.p, 0, nullptr, nullptr,
                                 (const u8*)s->d_masks.p, 0.f, L.stats, 1, nullptr, 1, L.work, L.hough, max_px_of(s), (const u8*)s->d_ref.p, &dm));
    RC(launch_hough(ctx, (const SquareDesc*)s->d_descs.p, n, (const u8*)s->d_gray.p, 0, hc, L.hough, nullptr, L.work, 1, L.retry, 0));
    // the second-pass list travels back in front of the results (it sits 512 bytes before them): normally it is empty
    // and the second pass, a launch of its own, is never enqueued
    const size_t o_retry_back = o_back - 512;
    CBV_HIP(ctx, hipMemcpyAsync(hst + o_retry_back, L.retry, 512 + L.out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (*(const u32*)(hst + o_retry_back) != 0) {
        RC(launch_hough_second(ctx, (const SquareDesc*)s->d_descs.p, n, (const u8*)s->d_gray.p, 0, hc, L.hough, nullptr, L.retry, n));
        CBV_HIP(ctx, hipMemcpyAsync(hst + o_back + L.o_hough, L.hough, sizeof(cbv_hough_result) * CBV_MAX_SQUARES, hipMemcpyDeviceToHost, ctx->stream));
        CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    const cbv_sq_stats* st = (const cbv_sq_stats*)(hst + o_back + L.o_stats);
    const cbv_hough_result* hg = (const cbv_hough_result*)(hst + o_back + L.o_hough);
    const u8* fl = hst + o_back + L.o_flags;
    for (int i = 0; i < n; i++) {
        cbv_piece_result r;
        memset(&r, 0, sizeof(r));
        if (fl[i] & 4) { // detect_piece is evaluated for this square
            const bool hough_ran = (fl[i] & 8) != 0;
            if (cbv_decide_piece(&st[i], hough_ran ? &hg[i] : nullptr, s->descs[i].w, s->descs[i].h, prm->circle_threshold, &r) != CBV_OK)
                return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "HoughCircles candidate list overflowed (more accumulator maxima than the second pass holds in a "
                                "%dx%d square)", s->descs[i].w, s->descs[i].h);
        }
        r.changed = fl[i] & 1;
        r.should_process = (fl[i] >> 1) & 1;
        r.evaluated = (fl[i] >> 2) & 1;
        out[i] = r;
    }
    return CBV_OK;
}

extern "C" int cbv_squares_detect_changes(cbv_squares* s, const cbv_host_image* img, const cbv_roi* rois, int n, int blur_k,
                                          const cbv_change_params* prm, cbv_change_result* out)
{
    if (!s) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    if (!prm || !out) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_squares_detect_changes: null argument");
    CBV_ENTER(ctx);
    if (!s->has_model) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_squares_detect_changes: not calibrated");
    RC(hough_params_check(ctx, &prm->hough));
    u8* hst;
    const size_t o_back = 8192, o_wk = 40960;
    RC(ctx_hstage(ctx, 65536, &hst));
    const int old_n = s->n;
    RC(squares_stage_host_image(s, img, rois, n, blur_k, hst));
    if (!s->has_model || s->n != old_n) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_squares_detect_changes: the squares' geometry changed since calibrate");
    FastLayout L;
    RC(fast_layout(s, &L));
    const int mpx = max_px_of(s);
    const bool five = s->blur_k == 5;
    if (five) {
        RC(launch_squares_pre5_stats(ctx, (const u8*)s->d_stage.p, 0, (const SquareDesc*)s->d_descs.p, n, (u8*)s->d_gray.p, 0, (const float*)s->d_mean.p,
                                     (const float*)sq_sd(s), (const u8*)s->d_masks.p, (float)prm->z_threshold, L.stats, 1, nullptr, 0, nullptr, nullptr,
                                     mpx));
    } else {
        // the detector's own blur for the background model, and the squares as PieceDetector preprocesses them (k = 5)
        // for the is_circular test of the squares that changed
        RC(launch_squares_preprocess(ctx, (const u8*)s->d_stage.p, 0, (const SquareDesc*)s->d_descs.p, n, (const int*)s->d_coef.p, s->blur_k,
                                     (u8*)s->d_gray.p, 0, 1, mpx));
        RC(launch_squares_stats(ctx, (const SquareDesc*)s->d_descs.p, n, (const u8*)s->d_gray.p, 0, nullptr, (const float*)s->d_mean.p,
                                (const float*)sq_sd(s), (const u8*)s->d_masks.p, (float)prm->z_threshold, L.stats, 1));
        RC(dev_ensure(ctx, &s->d_gray5, s->plane_total));
        RC(launch_squares_pre5_stats(ctx, (const u8*)s->d_stage.p, 0, (const SquareDesc*)s->d_descs.p, n, (u8*)s->d_gray5.p, 0, nullptr, nullptr,
                                     (const u8*)s->d_masks.p, 0.f, L.stats5, 1, nullptr, 0, nullptr, nullptr, mpx));
    }
    CBV_HIP(ctx, hipMemcpyAsync(hst + o_back + L.o_stats, L.stats, sizeof(cbv_sq_stats) * CBV_MAX_SQUARES * (five ? 1 : 2), hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const cbv_sq_stats* st = (const cbv_sq_stats*)(hst + o_back + L.o_stats);
    const cbv_sq_stats* st5 = five ? st : (const cbv_sq_stats*)(hst + o_back + L.o_stats5);
    // change_detector.py:124-150: squares of the selection whose share of changed pixels reaches 5 %
    u32* work = (u32*)(hst + o_wk);
    int nwork = 0;
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
                const long long nn = st5[i].n, sm = st5[i].sum;
                if (!(nn * (long long)st5[i].sumsq - sm * sm < 225ll * nn * nn)) work[1 + nwork++] = (u32)i; // HoughCircles runs on it
            }
        }
        out[i] = r;
    }
    const cbv_hough_result* hg = nullptr;
    if (nwork) {
        HoughCfg hc;
        RC(hough_cfg(ctx, &prm->hough, s->descs, &hc));
        work[0] = (u32)nwork;
        CBV_HIP(ctx, hipMemcpyAsync(L.work, work, sizeof(u32) * (1 + nwork), hipMemcpyHostToDevice, ctx->stream));
        CBV_HIP(ctx, hipMemsetAsync(L.retry, 0, sizeof(u32), ctx->stream));
        const u8* g5 = five ? (const u8*)s->d_gray.p : (const u8*)s->d_gray5.p;
        RC(launch_hough(ctx, (const SquareDesc*)s->d_descs.p, n, g5, 0, hc, L.hough, nullptr, L.work, 1, L.retry, 0));
        u32* retry_back = (u32*)(hst + o_wk + 1024);
        CBV_HIP(ctx, hipMemcpyAsync(retry_back, L.retry, sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
        CBV_HIP(ctx, hipMemcpyAsync(hst + o_back + L.o_hough, L.hough, sizeof(cbv_hough_result) * n, hipMemcpyDeviceToHost, ctx->stream));
        CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (*retry_back != 0) { // (normally empty: the second pass is a launch of its own)
            RC(launch_hough_second(ctx, (const SquareDesc*)s->d_descs.p, n, g5, 0, hc, L.hough, nullptr, L.retry, n));
            CBV_HIP(ctx, hipMemcpyAsync(hst + o_back + L.o_hough, L.hough, sizeof(cbv_hough_result) * n, hipMemcpyDeviceToHost, ctx->stream));
            CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        hg = (const cbv_hough_result*)(hst + o_back + L.o_hough);
    }
    for (int i = 0; i < n; i++) {
        if (!out[i].in_result) continue;
        bool ran = false;
        for (int k = 0; k < nwork && !ran; k++) ran = work[1 + k] == (u32)i;
        cbv_piece_result pr;
        if (cbv_decide_piece(&st5[i], ran ? &hg[i] : nullptr, s->descs[i].w, s->descs[i].h, prm->circle_threshold, &pr) != CBV_OK)
            return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "HoughCircles candidate list overflowed in a %dx%d square", s->descs[i].w, s->descs[i].h);
        out[i].is_circular = pr.has_piece;
    }
    return CBV_OK;
}

static int squares_plane(cbv_squares* s, int which, int index, void** p, size_t* bytes)
{
    cbv_ctx* ctx = s->ctx;
    if (index < 0 || index >= s->n) return cbv_fail(ctx, CBV_ERR_ARG, "square index %d out of range", index);
    const SquareDesc& d = s->descs[index];
    size_t n = (size_t)d.w * d.h;
    switch (which) {
    case 0: *p = (u8*)s->d_gray.p + d.plane_off; *bytes = n; break;
    case 1: *p = (u8*)s->d_ref.p + d.plane_off; *bytes = n; break;
    case 2: *p = (float*)s->d_mean.p + d.plane_off; *bytes = n * 4; break;
    case 3: *p = (float*)s->d_var.p + d.plane_off; *bytes = n * 4; break;
    case 4: *p = sq_sd(s) + d.plane_off; *bytes = n * 4; break; // sqrt(var) as the statistics kernels read it (inspection)
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
    CBV_ENTER(ctx);
    RC(squares_plane(s, which, index, &p, &bytes));
    CBV_HIP(ctx, hipMemcpyAsync(out, p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

extern "C" int cbv_squares_set(cbv_squares* s, int which, int index, const void* in)
{
    if (!s || !in) return CBV_ERR_ARG;
    cbv_ctx* ctx = s->ctx;
    void* p;
    size_t bytes;
    CBV_ENTER(ctx);
    RC(squares_plane(s, which, index, &p, &bytes));
    CBV_HIP(ctx, hipMemcpyAsync(p, in, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (which == 3) RC(launch_squares_refresh_sd(ctx, (const SquareDesc*)s->d_descs.p, (const float*)s->d_var.p, sq_sd(s), index));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (which == 1) s->has_ref = true;
    return CBV_OK;
}

extern "C" int cbv_squares_geometry(cbv_squares* s, int index, int* w, int* h)
{
    if (!s || index < 0 || index >= s->n) return CBV_ERR_ARG;
    if (w) *w = s->descs[index].w;
    if (h) *h = s->descs[index].h;
    return CBV_OK;
}

extern "C" int cbv_noise_run(cbv_ctx* ctx, const uint64_t* changes, int n, cbv_noise_state* state, cbv_noise_result* out)
{
    if (!ctx || !changes || !state || !out || n <= 0) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_noise_run: bad arguments");
    CBV_ENTER(ctx);
    size_t b_in = ((size_t)n * 8 + 255) & ~(size_t)255, b_out = ((size_t)n * sizeof(cbv_noise_result) + 255) & ~(size_t)255;
    RC(dev_ensure(ctx, &ctx->c, b_in + b_out + 256));
    u8* base = (u8*)ctx->c.p;
    CBV_HIP(ctx, hipMemcpyAsync(base, changes, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    CBV_HIP(ctx, hipMemcpyAsync(base + b_in + b_out, state, sizeof(cbv_noise_state), hipMemcpyHostToDevice, ctx->stream));
    RC(launch_noise(ctx, (const u64*)base, 1, n, (cbv_noise_state*)(base + b_in + b_out), (cbv_noise_result*)(base + b_in)));
    CBV_HIP(ctx, hipMemcpyAsync(out, base + b_in, (size_t)n * sizeof(cbv_noise_result), hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipMemcpyAsync(state, base + b_in + b_out, sizeof(cbv_noise_state), hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}
