// Ingest of YUV frames in a colour space other than 0 (include/cbv.h, CBV_CS_*: BT.601 full range, BT.709 limited and full
// range): k_ingest's YUV paths (k_ingest.hip) with the six constants of the conversion taken from a kernel argument (YuvCs,
// cbv_yuv.h) instead of the compiler's.  They are uniform over the launch and stay in scalar registers, so the three colour
// spaces share one form per layout and load path; colour space 0 keeps k_ingest.  The body is restated here, not shared
// through a header: k_ingest.hip is left compiling to what it compiled to.  Same threads, same loads, same stores: a
// thread owns the pixels that share chroma samples; PX 4 is the dword path (launch_ingest decides), PX 2 the byte path.
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

// the four pixels of dword `y` of luma bytes, whose pairs take chroma c0 and c1
__device__ __forceinline__ Px4 d_luma4(u32 y, const Chroma& c0, const Chroma& c1, const YuvCs& k)
{
    return d_pack4(d_yuv_bgr(y & 255, c0, k), d_yuv_bgr((y >> 8) & 255, c0, k), d_yuv_bgr((y >> 16) & 255, c1, k), d_yuv_bgr(y >> 24, c1, k));
}

// the 2 x 2 pixels of the byte path of a 4:2:0 layout
__device__ __forceinline__ void d_store_2x2(u8* out, int stride, const u8* l0, const u8* l1, const Chroma& c, const YuvCs& k)
{
    d_store_px(out, d_yuv_bgr(l0[0], c, k));
    d_store_px(out + 3, d_yuv_bgr(l0[1], c, k));
    d_store_px(out + stride, d_yuv_bgr(l1[0], c, k));
    d_store_px(out + stride + 3, d_yuv_bgr(l1[1], c, k));
}

template <int FMT, int PX>
__global__ __launch_bounds__(256) void k_ingest_cs(const u8* __restrict__ p0, const u8* __restrict__ p1, const u8* __restrict__ p2, RawGeom r,
                                                   u8* __restrict__ dst, Geom g, YuvCs k)
{
    typedef YuvLay<FMT> L;
    constexpr int ROWS = L::F420 ? 2 : 1;
    constexpr bool WIDE = PX == 4;
    const int bw = g.w / PX;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= bw * (g.h / ROWS)) return;
    const int by = i / bw, x = (i - by * bw) * PX, y = by * ROWS;
    p0 += (size_t)blockIdx.z * r.frame_stride;
    u8* out = dst + (size_t)blockIdx.z * g.frame_stride + (size_t)y * g.stride + (size_t)x * 3;
    if (L::F420) {
        const u8* l0 = p0 + (size_t)y * r.stride0 + x;
        const u8* l1 = l0 + r.stride0;
        if (L::PLANAR) {
            const u8* cu = p1 + (size_t)blockIdx.z * r.frame_stride + (size_t)by * r.stride1 + (x >> 1);
            const u8* cv = p2 + (size_t)blockIdx.z * r.frame_stride + (size_t)by * r.stride2 + (x >> 1);
            if (WIDE) {
                const u32 a = *(const u32*)l0, b = *(const u32*)l1;
                const u32 u = *(const u16*)cu, v = *(const u16*)cv;
                const Chroma c0 = d_chroma(u & 255, v & 255, k), c1 = d_chroma(u >> 8, v >> 8, k);
                *(Px4*)out = d_luma4(a, c0, c1, k);
                *(Px4*)(out + g.stride) = d_luma4(b, c0, c1, k);
            } else
                d_store_2x2(out, g.stride, l0, l1, d_chroma(cu[0], cv[0], k), k);
        } else {
            const u8* c = p1 + (size_t)blockIdx.z * r.frame_stride + (size_t)by * r.stride1 + x;
            if (WIDE) {
                const u32 a = *(const u32*)l0, b = *(const u32*)l1, uv = *(const u32*)c;
                const Chroma c0 = d_chroma((uv >> (8 * L::CU)) & 255, (uv >> (8 * L::CV)) & 255, k);
                const Chroma c1 = d_chroma((uv >> (16 + 8 * L::CU)) & 255, (uv >> (16 + 8 * L::CV)) & 255, k);
                *(Px4*)out = d_luma4(a, c0, c1, k);
                *(Px4*)(out + g.stride) = d_luma4(b, c0, c1, k);
            } else
                d_store_2x2(out, g.stride, l0, l1, d_chroma(c[L::CU], c[L::CV], k), k);
        }
    } else {
        const u8* s = p0 + (size_t)y * r.stride0 + (size_t)x * 2;
        if (WIDE) {
            const u32 a = *(const u32*)s, b = *(const u32*)(s + 4); // a pair each, e.g. Y0 U Y1 V
            const Chroma c0 = d_chroma((a >> (8 * L::PU)) & 255, (a >> (8 * L::PV)) & 255, k);
            const Chroma c1 = d_chroma((b >> (8 * L::PU)) & 255, (b >> (8 * L::PV)) & 255, k);
            *(Px4*)out = d_pack4(d_yuv_bgr((a >> (8 * L::Y0)) & 255, c0, k), d_yuv_bgr((a >> (8 * L::Y1)) & 255, c0, k),
                                 d_yuv_bgr((b >> (8 * L::Y0)) & 255, c1, k), d_yuv_bgr((b >> (8 * L::Y1)) & 255, c1, k));
        } else {
            const Chroma c0 = d_chroma(s[L::PU], s[L::PV], k);
            d_store_px(out, d_yuv_bgr(s[L::Y0], c0, k));
            d_store_px(out + 3, d_yuv_bgr(s[L::Y1], c0, k));
        }
    }
}

template <int FMT>
static void ingest_cs_launch(cbv_ctx* ctx, const RawPlanes& pl, const RawGeom& r, u8* dst, const Geom& g, int batch, const YuvCs& k, bool wide)
{
    const int px = wide ? 4 : 2, blocks = (g.w / px) * (g.h / (YuvLay<FMT>::F420 ? 2 : 1));
    const dim3 grid((blocks + 255) / 256, 1, batch);
    if (wide) hipLaunchKernelGGL((k_ingest_cs<FMT, 4>), grid, dim3(256), 0, ctx->stream, pl.p[0], pl.p[1], pl.p[2], r, dst, g, k);
    else hipLaunchKernelGGL((k_ingest_cs<FMT, 2>), grid, dim3(256), 0, ctx->stream, pl.p[0], pl.p[1], pl.p[2], r, dst, g, k);
}

// what launch_ingest (k_ingest.hip) calls inside its profiling bracket once it has checked the planes, made YV12 YUV420P and
// chosen the load path: r.fmt is one of the six YUV layouts the kernels know, cs is 1 to 3
void launch_ingest_cs(cbv_ctx* ctx, const RawPlanes& pl, const RawGeom& r, u8* dst, const Geom& g, int batch, int cs, bool wide)
{
    const YuvCs k = kYuvCs[cs];
    switch (r.fmt) {
    case CBV_FMT_NV12: return ingest_cs_launch<CBV_FMT_NV12>(ctx, pl, r, dst, g, batch, k, wide);
    case CBV_FMT_NV21: return ingest_cs_launch<CBV_FMT_NV21>(ctx, pl, r, dst, g, batch, k, wide);
    case CBV_FMT_YUYV: return ingest_cs_launch<CBV_FMT_YUYV>(ctx, pl, r, dst, g, batch, k, wide);
    case CBV_FMT_YVYU: return ingest_cs_launch<CBV_FMT_YVYU>(ctx, pl, r, dst, g, batch, k, wide);
    case CBV_FMT_UYVY: return ingest_cs_launch<CBV_FMT_UYVY>(ctx, pl, r, dst, g, batch, k, wide);
    case CBV_FMT_YUV420P: return ingest_cs_launch<CBV_FMT_YUV420P>(ctx, pl, r, dst, g, batch, k, wide);
    }
}
