// Ingest: camera-native frames (NV12, YUYV) to the BGR frames every other kernel reads (include/cbv.h, cbv_yuv_to_bgr,
// cbv_pipeline_upload_raw, cbv_pipeline_submit after cbv_pipeline_set_input_format).  cv2.cvtColor's
// COLOR_YUV2BGR_NV12 / COLOR_YUV2BGR_YUY2 on 8-bit data: BT.601 limited range in fixed point, no chroma interpolation.
#include "cbv_yuv.h"

// four pixels (24 bits each) as the 12 bytes of a BGR row
__device__ __forceinline__ Px4 d_pack4(u32 q0, u32 q1, u32 q2, u32 q3)
{
    Px4 p;
    p.d[0] = q0 | (q1 << 24);
    p.d[1] = (q1 >> 8) | (q2 << 16);
    p.d[2] = (q2 >> 16) | (q3 << 8);
    return p;
}

__device__ __forceinline__ void d_store_px(u8* d, u32 q)
{
    d[0] = (u8)q;
    d[1] = (u8)(q >> 8);
    d[2] = (u8)(q >> 16);
}

// A thread owns the pixels that share chroma samples.  WIDE (w % 4 == 0 and every row of the input and the output starts
// on a dword boundary): 4 x 2 pixels of NV12 = two dword luma loads, one dword chroma load, two 12-byte stores; 4 x 1 of
// YUYV = two dword loads, one 12-byte store.  Otherwise (w = 322: a BGR row of 966 bytes starts on any byte) 2 x 2 / 2 x 1
// pixels with byte accesses.  Blocks are numbered row-major over the frame, so a wave reads and writes whole runs of rows.
template <int FMT, bool WIDE>
__global__ __launch_bounds__(256) void k_ingest(const u8* __restrict__ p0, const u8* __restrict__ p1, RawGeom r, u8* __restrict__ dst, Geom g)
{
    constexpr int PX = WIDE ? 4 : 2, ROWS = FMT == CBV_FMT_NV12 ? 2 : 1;
    const int bw = g.w / PX;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= bw * (g.h / ROWS)) return;
    const int by = i / bw, x = (i - by * bw) * PX, y = by * ROWS;
    p0 += (size_t)blockIdx.z * r.frame_stride;
    u8* out = dst + (size_t)blockIdx.z * g.frame_stride + (size_t)y * g.stride + (size_t)x * 3;
    if (FMT == CBV_FMT_NV12) {
        const u8* l0 = p0 + (size_t)y * r.stride0 + x;
        const u8* l1 = l0 + r.stride0;
        const u8* c = p1 + (size_t)blockIdx.z * r.frame_stride + (size_t)by * r.stride1 + x;
        if (WIDE) {
            const u32 a = *(const u32*)l0, b = *(const u32*)l1, uv = *(const u32*)c;
            const Chroma c0 = d_chroma(uv & 255, (uv >> 8) & 255), c1 = d_chroma((uv >> 16) & 255, uv >> 24);
            *(Px4*)out = d_pack4(d_yuv_bgr(a & 255, c0), d_yuv_bgr((a >> 8) & 255, c0), d_yuv_bgr((a >> 16) & 255, c1), d_yuv_bgr(a >> 24, c1));
            *(Px4*)(out + g.stride) = d_pack4(d_yuv_bgr(b & 255, c0), d_yuv_bgr((b >> 8) & 255, c0), d_yuv_bgr((b >> 16) & 255, c1), d_yuv_bgr(b >> 24, c1));
        } else {
            const Chroma c0 = d_chroma(c[0], c[1]);
            d_store_px(out, d_yuv_bgr(l0[0], c0));
            d_store_px(out + 3, d_yuv_bgr(l0[1], c0));
            d_store_px(out + g.stride, d_yuv_bgr(l1[0], c0));
            d_store_px(out + g.stride + 3, d_yuv_bgr(l1[1], c0));
        }
    } else {
        const u8* s = p0 + (size_t)y * r.stride0 + (size_t)x * 2;
        if (WIDE) {
            const u32 a = *(const u32*)s, b = *(const u32*)(s + 4); // Y0 U Y1 V
            const Chroma c0 = d_chroma((a >> 8) & 255, a >> 24), c1 = d_chroma((b >> 8) & 255, b >> 24);
            *(Px4*)out = d_pack4(d_yuv_bgr(a & 255, c0), d_yuv_bgr((a >> 16) & 255, c0), d_yuv_bgr(b & 255, c1), d_yuv_bgr((b >> 16) & 255, c1));
        } else {
            const Chroma c0 = d_chroma(s[1], s[3]);
            d_store_px(out, d_yuv_bgr(s[0], c0));
            d_store_px(out + 3, d_yuv_bgr(s[2], c0));
        }
    }
}

int check_raw_format(cbv_ctx* ctx, int fmt, int w, int h, const char* what)
{
    if (fmt != CBV_FMT_NV12 && fmt != CBV_FMT_YUYV) return cbv_fail(ctx, CBV_ERR_ARG, "%s: unknown raw format %d", what, fmt);
    if (w <= 0 || h <= 0 || (w & 1)) return cbv_fail(ctx, CBV_ERR_ARG, "%s: %s frames need an even width (%dx%d)", what, fmt == CBV_FMT_NV12 ? "NV12" : "YUYV", w, h);
    if (fmt == CBV_FMT_NV12 && (h & 1)) return cbv_fail(ctx, CBV_ERR_ARG, "%s: NV12 frames need an even height (%dx%d)", what, w, h);
    return CBV_OK;
}

template <int FMT>
static void ingest_launch(cbv_ctx* ctx, const u8* p0, const u8* p1, RawGeom r, u8* dst, Geom g, int batch, bool wide)
{
    const int blocks = (g.w / (wide ? 4 : 2)) * (g.h / (FMT == CBV_FMT_NV12 ? 2 : 1));
    const dim3 grid((blocks + 255) / 256, 1, batch);
    if (wide) hipLaunchKernelGGL((k_ingest<FMT, true>), grid, dim3(256), 0, ctx->stream, p0, p1, r, dst, g);
    else hipLaunchKernelGGL((k_ingest<FMT, false>), grid, dim3(256), 0, ctx->stream, p0, p1, r, dst, g);
}

int launch_ingest(cbv_ctx* ctx, const u8* plane0, const u8* plane1, RawGeom r, u8* dst, Geom g, int batch)
{
    RC(check_raw_format(ctx, r.fmt, g.w, g.h, "launch_ingest"));
    const bool nv12 = r.fmt == CBV_FMT_NV12;
    if (batch <= 0 || !plane0 || !dst || (nv12 && !plane1) || r.stride0 < (nv12 ? g.w : 2 * g.w) || (nv12 && r.stride1 < g.w) || g.stride < g.w * 3)
        return cbv_fail(ctx, CBV_ERR_ARG, "launch_ingest: bad planes or strides");
    // the dword path: every row of every plane of every frame starts on a dword boundary
    const size_t mis = (size_t)g.w | (size_t)plane0 | (size_t)r.stride0 | r.frame_stride | (size_t)dst | (size_t)g.stride | g.frame_stride |
                       (nv12 ? (size_t)plane1 | (size_t)r.stride1 : 0);
    const bool wide = (mis & 3) == 0;
    prof_begin(ctx, CBV_K_INGEST);
    if (nv12) ingest_launch<CBV_FMT_NV12>(ctx, plane0, plane1, r, dst, g, batch, wide);
    else ingest_launch<CBV_FMT_YUYV>(ctx, plane0, plane1, r, dst, g, batch, wide);
    prof_end(ctx, CBV_K_INGEST);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}
