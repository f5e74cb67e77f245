// Ingest: camera-native frames (NV12, NV21, YUV420P, YV12, YUYV, YVYU, UYVY) to the BGR frames every other kernel reads
// (include/cbv.h, cbv_yuv_to_bgr, cbv_pipeline_upload_raw, cbv_pipeline_submit after cbv_pipeline_set_input_format).
// cv2.cvtColor's COLOR_YUV2BGR_* of these layouts on 8-bit data: BT.601 limited range in fixed point, no chroma interpolation.
#include "cbv_yuv.h"

#include <utility>

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
__device__ __forceinline__ Px4 d_luma4(u32 y, const Chroma& c0, const Chroma& c1)
{
    return d_pack4(d_yuv_bgr(y & 255, c0), d_yuv_bgr((y >> 8) & 255, c0), d_yuv_bgr((y >> 16) & 255, c1), d_yuv_bgr(y >> 24, c1));
}

// A thread owns the pixels that share chroma samples.  PX = pixels per thread and row; where the bytes lie inside a dword
// (NV12 / NV21, YUYV / YVYU / UYVY) is YuvLay<FMT>.  PX 4 (w % 4 == 0 and every row of the input and the output starts on
// a dword boundary): 4 x 2 pixels of NV12 = two dword luma loads, one dword chroma load, two 12-byte stores; 4 x 1 of YUYV =
// two dword loads, one 12-byte store.  Otherwise (w = 322: a BGR row of 966 bytes starts on any byte) 2 x 2 / 2 x 1 pixels
// with byte accesses.  Planar chroma (YUV420P; YV12 arrives with p1 and p2 swapped): PX 4 (w % 4 == 0, luma and output rows
// on a dword boundary, chroma rows on an even address) = two dword luma loads, a 2-byte load of U and one of V, two 12-byte
// stores; PX 2 bytes.  (An 8 x 2 form with dword chroma loads and 8-byte luma loads was measured and is slower: DESIGN.md
// section 4.)  Blocks are numbered row-major over the frame, so a wave reads and writes whole runs of rows.
template <int FMT, int PX>
__global__ __launch_bounds__(256) void k_ingest(const u8* __restrict__ p0, const u8* __restrict__ p1, const u8* __restrict__ p2, RawGeom r,
                                                u8* __restrict__ dst, Geom g)
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
    if (L::PLANAR) {
        const u8* l0 = p0 + (size_t)y * r.stride0 + x;
        const u8* l1 = l0 + r.stride0;
        const u8* cu = p1 + (size_t)blockIdx.z * r.frame_stride + (size_t)by * r.stride1 + (x >> 1);
        const u8* cv = p2 + (size_t)blockIdx.z * r.frame_stride + (size_t)by * r.stride2 + (x >> 1);
        if (WIDE) {
            const u32 a = *(const u32*)l0, b = *(const u32*)l1;
            const u32 u = *(const u16*)cu, v = *(const u16*)cv;
            const Chroma c0 = d_chroma(u & 255, v & 255), c1 = d_chroma(u >> 8, v >> 8);
            *(Px4*)out = d_luma4(a, c0, c1);
            *(Px4*)(out + g.stride) = d_luma4(b, c0, c1);
        } else {
            const Chroma c0 = d_chroma(cu[0], cv[0]);
            d_store_px(out, d_yuv_bgr(l0[0], c0));
            d_store_px(out + 3, d_yuv_bgr(l0[1], c0));
            d_store_px(out + g.stride, d_yuv_bgr(l1[0], c0));
            d_store_px(out + g.stride + 3, d_yuv_bgr(l1[1], c0));
        }
    } else if (L::F420) {
        const u8* l0 = p0 + (size_t)y * r.stride0 + x;
        const u8* l1 = l0 + r.stride0;
        const u8* c = p1 + (size_t)blockIdx.z * r.frame_stride + (size_t)by * r.stride1 + x;
        if (WIDE) {
            const u32 a = *(const u32*)l0, b = *(const u32*)l1, uv = *(const u32*)c;
            const Chroma c0 = d_chroma((uv >> (8 * L::CU)) & 255, (uv >> (8 * L::CV)) & 255);
            const Chroma c1 = d_chroma((uv >> (16 + 8 * L::CU)) & 255, (uv >> (16 + 8 * L::CV)) & 255);
            *(Px4*)out = d_luma4(a, c0, c1);
            *(Px4*)(out + g.stride) = d_luma4(b, c0, c1);
        } else {
            const Chroma c0 = d_chroma(c[L::CU], c[L::CV]);
            d_store_px(out, d_yuv_bgr(l0[0], c0));
            d_store_px(out + 3, d_yuv_bgr(l0[1], c0));
            d_store_px(out + g.stride, d_yuv_bgr(l1[0], c0));
            d_store_px(out + g.stride + 3, d_yuv_bgr(l1[1], c0));
        }
    } else {
        const u8* s = p0 + (size_t)y * r.stride0 + (size_t)x * 2;
        if (WIDE) {
            const u32 a = *(const u32*)s, b = *(const u32*)(s + 4); // a pair each, e.g. Y0 U Y1 V
            const Chroma c0 = d_chroma((a >> (8 * L::PU)) & 255, (a >> (8 * L::PV)) & 255);
            const Chroma c1 = d_chroma((b >> (8 * L::PU)) & 255, (b >> (8 * L::PV)) & 255);
            *(Px4*)out = d_pack4(d_yuv_bgr((a >> (8 * L::Y0)) & 255, c0), d_yuv_bgr((a >> (8 * L::Y1)) & 255, c0),
                                 d_yuv_bgr((b >> (8 * L::Y0)) & 255, c1), d_yuv_bgr((b >> (8 * L::Y1)) & 255, c1));
        } else {
            const Chroma c0 = d_chroma(s[L::PU], s[L::PV]);
            d_store_px(out, d_yuv_bgr(s[L::Y0], c0));
            d_store_px(out + 3, d_yuv_bgr(s[L::Y1], c0));
        }
    }
}

int check_raw_format(cbv_ctx* ctx, int fmt, int w, int h, const char* what)
{
    if (!raw_fmt_known(fmt)) return cbv_fail(ctx, CBV_ERR_ARG, "%s: unknown raw format %d", what, fmt);
    if (w <= 0 || h <= 0 || (w & 1)) return cbv_fail(ctx, CBV_ERR_ARG, "%s: %s frames need an even width (%dx%d)", what, raw_fmt_name(fmt), w, h);
    if (raw_fmt_420(fmt) && (h & 1)) return cbv_fail(ctx, CBV_ERR_ARG, "%s: %s frames need an even height (%dx%d)", what, raw_fmt_name(fmt), w, h);
    return CBV_OK;
}

int check_raw_planes(cbv_ctx* ctx, int fmt, int w, const u8* const* planes, const int* strides, const char* what)
{
    for (int i = 0; i < raw_fmt_planes(fmt); i++)
        if (!planes[i] || strides[i] < raw_plane_wbytes(fmt, w, i))
            return cbv_fail(ctx, CBV_ERR_ARG, "%s: bad planes or strides of the raw frame (plane %d of a %s frame: stride %d)", what, i,
                            raw_fmt_name(fmt), strides[i]);
    return CBV_OK;
}

// YV12 is YUV420P with the chroma planes swapped
void raw_planes_canonical(RawPlanes* pl, RawGeom* r)
{
    if (r->fmt != CBV_FMT_YV12) return;
    std::swap(pl->p[1], pl->p[2]);
    std::swap(r->stride1, r->stride2);
    r->fmt = CBV_FMT_YUV420P;
}

template <int FMT, int PX>
static void ingest_launch(cbv_ctx* ctx, const RawPlanes& pl, RawGeom r, u8* dst, Geom g, int batch)
{
    const int blocks = (g.w / PX) * (g.h / (YuvLay<FMT>::F420 ? 2 : 1));
    const dim3 grid((blocks + 255) / 256, 1, batch);
    hipLaunchKernelGGL((k_ingest<FMT, PX>), grid, dim3(256), 0, ctx->stream, pl.p[0], pl.p[1], pl.p[2], r, dst, g);
}

int launch_ingest(cbv_ctx* ctx, RawPlanes pl, RawGeom r, u8* dst, Geom g, int batch)
{
    RC(check_raw_format(ctx, r.fmt, g.w, g.h, "launch_ingest"));
    const int strides[3] = {r.stride0, r.stride1, r.stride2};
    if (batch <= 0 || !dst || g.stride < g.w * 3) return cbv_fail(ctx, CBV_ERR_ARG, "launch_ingest: bad planes or strides");
    RC(check_raw_planes(ctx, r.fmt, g.w, pl.p, strides, "launch_ingest"));
    raw_planes_canonical(&pl, &r);
    // the dword path: every row of every plane of every frame starts on a dword boundary (planar chroma rows, read two
    // bytes at a time: on an even address)
    const int np = raw_fmt_planes(r.fmt);
    const size_t luma = (size_t)pl.p[0] | (size_t)r.stride0 | r.frame_stride | (size_t)dst | (size_t)g.stride | g.frame_stride;
    const size_t chroma = (np > 1 ? (size_t)pl.p[1] | (size_t)r.stride1 : 0) | (np > 2 ? (size_t)pl.p[2] | (size_t)r.stride2 : 0);
    const bool wide = (((size_t)g.w | luma) & 3) == 0 && (chroma & (np > 2 ? 1 : 3)) == 0;
    prof_begin(ctx, CBV_K_INGEST);
#define CBV_INGEST(FMT)                                                                 \
    case FMT:                                                                           \
        if (wide) ingest_launch<FMT, 4>(ctx, pl, r, dst, g, batch);                      \
        else ingest_launch<FMT, 2>(ctx, pl, r, dst, g, batch);                           \
        break
    switch (r.fmt) {
        CBV_INGEST(CBV_FMT_NV12);
        CBV_INGEST(CBV_FMT_NV21);
        CBV_INGEST(CBV_FMT_YUYV);
        CBV_INGEST(CBV_FMT_YVYU);
        CBV_INGEST(CBV_FMT_UYVY);
        CBV_INGEST(CBV_FMT_YUV420P);
    }
#undef CBV_INGEST
    prof_end(ctx, CBV_K_INGEST);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}
