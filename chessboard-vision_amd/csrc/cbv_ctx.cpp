// C-ABI of libcbv_hip.so (include/cbv.h), the context: error string, device buffers, the pinned staging area, worker
// streams, the kernel profiler, cbv_ctx_create / destroy and the colour-profile and bilateral tables.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <memory>

#include "cbv_internal.h"

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
    "k_warp_yuv", "k_change_blur_stats", "", "k_ingest_deep", "k_warp_deep", "", "k_piece_tone"};

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

// the tables of a profile that belongs to a pipeline or a call (the warp of a source with a profile), never ctx->ptabs: the profile as
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
    ctx->btabs_centre_bad = bilateral_centre_mismatch(&ctx->btabs_host);
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    CBV_HIP(ctx, hipMemcpy(ctx->btabs, &ctx->btabs_host, sizeof(BilateralTabs), hipMemcpyHostToDevice));
    ctx->b_d = d;
    ctx->b_sc = sc;
    ctx->b_ss = ss;
    return CBV_OK;
}

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

// Not in include/cbv.h: for tests/test_bilateral_walk_host.py.  1 when the centre tap's entry of the host-built table is
// exactly 1.0f (the constant the batched d = 9 kernel uses in its place), 0 when it is not; -1: radius not supported.
extern "C" CBV_API int cbv_debug_bilateral_centre_is_one(int d, double sigma_color, double sigma_space)
{
    auto t = std::make_unique<BilateralTabs>();
    if (build_bilateral_tabs(d, sigma_color, sigma_space, t.get()) != 0 || t->radius > 4) return -1;
    return bilateral_centre_mismatch(t.get()) ? 0 : 1;
}
