// Ingest: camera-native frames (NV12, NV21, YUV420P, YV12, YUYV, YVYU, UYVY, the four 8-bit Bayer mosaics) to the BGR frames
// every other kernel reads (include/cbv.h, cbv_yuv_to_bgr, cbv_pipeline_upload_raw, cbv_pipeline_submit after
// cbv_pipeline_set_input_format).
// cv2.cvtColor's COLOR_YUV2BGR_* of the YUV layouts on 8-bit data: BT.601 limited range in fixed point, no chroma interpolation;
// its bilinear COLOR_Bayer??2BGR of the mosaics (cbv_bayer.h).
#include "cbv_bayer.h"
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

// The Bayer family (cbv_bayer.h): a thread owns PX x 2 output pixels at (x, y), y even, and reads the rows y - 1 .. y + 2
// and columns x - 1 .. x + PX of the mosaic; rows outside the frame are the nearest row inside, whose values only reach
// sites that the edge rule replaces.  The outermost rows and columns copy their neighbours' results (the clamp on the
// site): a thread on the frame's edge writes the inner pixel's or row's result twice.
// PX 4: per row the aligned dword and its two neighbour dwords, two 12-byte stores.  At x = 0 and x = w - 4 the neighbour
// outside the row is replaced by the thread's own dword (the address is clamped, not the load skipped: a load under a
// branch waits for the loads before it, and that chain of waits took 2.61 us per 1080p frame against 1.73); its
// bytes only reach the pixel the edge rule replaces.  PX 2: byte loads with the column clamped, byte stores.  The overlap
// with the neighbouring threads' reads is served by the cache.
template <int FMT, int PX>
__device__ __forceinline__ void ingest_bayer(const u8* __restrict__ p0, const RawGeom& r, u8* __restrict__ out, const Geom& g, int x, int y)
{
    u32 q[2][PX]; // the two rows of results
    u32 nb[4][PX]; // per mosaic row: the bytes of columns x + j - 1, x + j, x + j + 1 for pixel j
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const u8* row = p0 + (size_t)min(max(y - 1 + k, 0), g.h - 1) * r.stride0;
        if (PX == 4) {
            const u32 m = *(const u32*)(row + x);
            const u32 l = *(const u32*)(row + max(x - 4, 0));
            const u32 rr = *(const u32*)(row + min(x + 4, g.w - 4));
            nb[k][0] = (l >> 24) | (m << 8);
            nb[k][1] = m;
            nb[k][2] = m >> 8;
            nb[k][3] = (m >> 16) | (rr << 16);
        } else {
            u32 b[PX + 2];
#pragma unroll
            for (int j = 0; j < PX + 2; j++) b[j] = row[min(max(x - 1 + j, 0), g.w - 1)];
#pragma unroll
            for (int j = 0; j < PX; j++) nb[k][j] = b[j] | (b[j + 1] << 8) | (b[j + 2] << 16);
        }
    }
    // row i of the results is the site row y + i (y is even and x a multiple of PX: the phases are constants)
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < PX; j++) q[i][j] = d_bayer_bgr<FMT>(j, i, nb[i][j], nb[i + 1][j], nb[i + 2][j]);
#pragma unroll
    for (int i = 0; i < 2; i++) {
        if (x == 0) q[i][0] = q[i][1];
        if (x + PX == g.w) q[i][PX - 1] = q[i][PX - 2];
    }
    const bool top = y == 0, bottom = y + 2 == g.h;
#pragma unroll
    for (int j = 0; j < PX; j++) {
        const u32 a = top ? q[1][j] : q[0][j], b = bottom ? q[0][j] : q[1][j];
        q[0][j] = a;
        q[1][j] = b;
    }
    if (PX == 4) {
        *(Px4*)out = d_pack4(q[0][0], q[0][1], q[0][2], q[0][3]);
        *(Px4*)(out + g.stride) = d_pack4(q[1][0], q[1][1], q[1][2], q[1][3]);
    } else {
#pragma unroll
        for (int j = 0; j < PX; j++) {
            d_store_px(out + 3 * j, q[0][j]);
            d_store_px(out + g.stride + 3 * j, q[1][j]);
        }
    }
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
    constexpr bool BAYER = (FMT & 15) == CBV_FMT_BAYER_RGGB;
    constexpr int ROWS = L::F420 || BAYER ? 2 : 1;
    constexpr bool WIDE = PX == 4;
    const int bw = g.w / PX;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= bw * (g.h / ROWS)) return;
    const int by = i / bw, x = (i - by * bw) * PX, y = by * ROWS;
    p0 += (size_t)blockIdx.z * r.frame_stride;
    u8* out = dst + (size_t)blockIdx.z * g.frame_stride + (size_t)y * g.stride + (size_t)x * 3;
    if (BAYER) {
        ingest_bayer<FMT, PX>(p0, r, out, g, x, y);
    } else if (L::PLANAR) {
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

int check_fmt_cs(cbv_ctx* ctx, int fmt, const char* what)
{
    if (!raw_fmt_cs(fmt) || (raw_fmt_known(raw_fmt_layout(fmt)) && raw_fmt_yuv(raw_fmt_layout(fmt)))) return CBV_OK;
    return cbv_fail(ctx, CBV_ERR_ARG, "%s: colour-space bits 0x%x on format %d (%s): a colour space goes with the YUV formats only", what, fmt & CBV_CS_MASK,
                    raw_fmt_layout(fmt), raw_fmt_name(raw_fmt_layout(fmt)));
}

int check_raw_format(cbv_ctx* ctx, int fmt, int w, int h, const char* what)
{
    RC(check_fmt_cs(ctx, fmt, what));
    fmt = raw_fmt_layout(fmt); // (the colour space of a YUV id asks nothing of the frame)
    if (!raw_fmt_known(fmt)) return cbv_fail(ctx, CBV_ERR_ARG, "%s: unknown raw format %d", what, fmt);
    if (raw_fmt_bayer(fmt)) {
        if (w < 4 || h < 4 || ((w | h) & 1))
            return cbv_fail(ctx, CBV_ERR_ARG, "%s: %s frames need an even width and height of at least 4 (%dx%d)", what, raw_fmt_name(fmt), w, h);
        if (raw_fmt_enc(fmt) == BAYER_ENC_10P && (w & 3)) // (a RAW10 group is four samples)
            return cbv_fail(ctx, CBV_ERR_ARG, "%s: %s frames need a width that is a multiple of 4 (%dx%d)", what, raw_fmt_name(fmt), w, h);
        return CBV_OK;
    }
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
    const int blocks = (g.w / PX) * (g.h / (YuvLay<FMT>::F420 || raw_fmt_bayer(FMT) ? 2 : 1));
    const dim3 grid((blocks + 255) / 256, 1, batch);
    hipLaunchKernelGGL((k_ingest<FMT, PX>), grid, dim3(256), 0, ctx->stream, pl.p[0], pl.p[1], pl.p[2], r, dst, g);
}

int launch_ingest(cbv_ctx* ctx, RawPlanes pl, RawGeom r, u8* dst, Geom g, int batch, int cs)
{
    RC(check_raw_format(ctx, r.fmt, g.w, g.h, "launch_ingest"));
    if (raw_fmt_cs(r.fmt) || cs < 0 || cs > 3 || (cs && !raw_fmt_yuv(r.fmt)))
        return cbv_fail(ctx, CBV_ERR_ARG, "launch_ingest: colour space %d with layout %d (the layout and the colour space are split where an id enters)", cs, r.fmt);
    if (raw_fmt_enc(r.fmt)) // (a sample encoding: launch_ingest_deep, k_ingest_deep.hip; the switch below knows the 8-bit ids)
        return cbv_fail(ctx, CBV_ERR_ARG, "launch_ingest: format %d (%s) is a developed mosaic", r.fmt, raw_fmt_name(r.fmt));
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
    if (cs) launch_ingest_cs(ctx, pl, r, dst, g, batch, cs, wide); // the runtime-matrix form (k_ingest_cs.hip)
    else switch (r.fmt) {
        CBV_INGEST(CBV_FMT_NV12);
        CBV_INGEST(CBV_FMT_NV21);
        CBV_INGEST(CBV_FMT_YUYV);
        CBV_INGEST(CBV_FMT_YVYU);
        CBV_INGEST(CBV_FMT_UYVY);
        CBV_INGEST(CBV_FMT_YUV420P);
        CBV_INGEST(CBV_FMT_BAYER_RGGB);
        CBV_INGEST(CBV_FMT_BAYER_BGGR);
        CBV_INGEST(CBV_FMT_BAYER_GRBG);
        CBV_INGEST(CBV_FMT_BAYER_GBRG);
    }
#undef CBV_INGEST
    prof_end(ctx, CBV_K_INGEST);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}
