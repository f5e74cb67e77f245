// Ingest of developed mosaics (include/cbv.h: Bayer frames of 10, 12, 14 and 16 bits in a 16-bit container, MIPI RAW10 and
// RAW12 packed rows, and 8-bit mosaics with tables) into the BGR frames every other kernel reads: unpack, the per-colour table,
// then cbv_bayer.h's demosaic.  k_ingest's Bayer path (k_ingest.hip, ingest_bayer) with the fetch of the neighbourhood replaced:
// same threads, same neighbourhood, same edge rule, same stores.  It sits in a unit of its own so that k_ingest.hip compiles to
// what it compiled to, and the 8-bit ids without tables keep launching k_ingest.
// The layout's phase bits and the encoding are uniform kernel arguments (cbv_bayer_deep.h), so the kernels are PX x LDS: four.
#include "cbv_bayer_deep.h"

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

#define DEEP_LDS_BITS 12 // tables of up to 12 bits (3 x 4 KB) are staged in LDS; 14 and 16 bits (48 / 192 KB) stay in global memory
#define DEEP_ITEMS 8     // a workgroup stages its tables once and covers DEEP_ITEMS x 256 threads' worth of pixels

// A thread owns PX x 2 output pixels at (x, y), y even, and reads the samples of rows y - 1 .. y + 2 and columns
// x - 1 .. x + PX; rows and columns outside the frame are the nearest inside, whose values only reach sites that the edge
// rule replaces (ingest_bayer, k_ingest.hip).  Every sample is developed with the colour of the site it was fetched from.
// PX 4 (w % 4 == 0, the BGR rows on dword boundaries): the thread's own four samples of a row with wide loads (d_deep_row4:
// they work at any address, a row of a packed mosaic starts on any byte and a RAW10 group never aligns), the two neighbours
// with byte loads at clamped columns, two 12-byte stores.  PX 2: byte loads, byte stores.
template <int PX, bool LDS>
__global__ __launch_bounds__(256) void k_ingest_deep(const u8* __restrict__ p0, RawGeom r, u8* __restrict__ dst, Geom g, DeepDev d)
{
    __shared__ u8 lt[LDS ? (3 << DEEP_LDS_BITS) : 4];
    if (LDS) {
        lds_copy(lt, d.tab, 3 << d.bits);
        __syncthreads();
    }
    const u8* __restrict__ tab = LDS ? lt : d.tab;
    const int bw = g.w / PX, total = bw * (g.h / 2);
    p0 += (size_t)blockIdx.z * r.frame_stride;
    for (int it = 0; it < DEEP_ITEMS; it++) {
        const int i = (blockIdx.x * DEEP_ITEMS + it) * 256 + threadIdx.x;
        if (i >= total) return;
        const int by = i / bw, x = (i - by * bw) * PX, y = by * 2;
        u8* out = dst + (size_t)blockIdx.z * g.frame_stride + (size_t)y * g.stride + (size_t)x * 3;
        u32 q[2][PX]; // the two rows of results
        u32 nb[4][PX]; // per mosaic row: the developed bytes of columns x + j - 1, x + j, x + j + 1 for pixel j
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int yy = min(max(y - 1 + k, 0), g.h - 1);
            const u8* row = p0 + (size_t)yy * r.stride0;
            u32 b[PX + 2];
            if (PX == 4) {
                u32 s[4];
                d_deep_row4(row, x, d.enc, s);
                const int xl = max(x - 1, 0), xr = min(x + 4, g.w - 1);
                b[0] = d_deep_byte(tab, d, d_deep_sample(row, xl, d.enc), xl, yy);
#pragma unroll
                for (int j = 0; j < 4; j++) b[1 + j] = d_deep_byte(tab, d, s[j], x + j, yy);
                b[5] = d_deep_byte(tab, d, d_deep_sample(row, xr, d.enc), xr, yy);
            } else {
#pragma unroll
                for (int j = 0; j < PX + 2; j++) {
                    const int xx = min(max(x - 1 + j, 0), g.w - 1);
                    b[j] = d_deep_byte(tab, d, d_deep_sample(row, xx, d.enc), xx, yy);
                }
            }
#pragma unroll
            for (int j = 0; j < PX; j++) nb[k][j] = b[j] | (b[j + 1] << 8) | (b[j + 2] << 16);
        }
        // row i of the results is the site row y + i (y is even and x a multiple of PX: the parities are j's and i's)
#pragma unroll
        for (int i2 = 0; i2 < 2; i2++)
#pragma unroll
            for (int j = 0; j < PX; j++) q[i2][j] = d_deep_bgr(d.ph, j, i2, nb[i2][j], nb[i2 + 1][j], nb[i2 + 2][j]);
#pragma unroll
        for (int i2 = 0; i2 < 2; i2++) {
            if (x == 0) q[i2][0] = q[i2][1];
            if (x + PX == g.w) q[i2][PX - 1] = q[i2][PX - 2];
        }
        const bool top = y == 0, bottom = y + 2 == g.h;
#pragma unroll
        for (int j = 0; j < PX; j++) {
            const u32 a = top ? q[1][j] : q[0][j], b2 = bottom ? q[0][j] : q[1][j];
            q[0][j] = a;
            q[1][j] = b2;
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
}

template <int PX, bool LDS>
static void ingest_deep_launch(cbv_ctx* ctx, const u8* mosaic, const RawGeom& r, u8* dst, const Geom& g, int batch, const DeepDev& d)
{
    const int threads = (g.w / PX) * (g.h / 2), per = 256 * DEEP_ITEMS;
    const dim3 grid((threads + per - 1) / per, 1, batch);
    hipLaunchKernelGGL((k_ingest_deep<PX, LDS>), grid, dim3(256), 0, ctx->stream, mosaic, r, dst, g, d);
}

int launch_ingest_deep(cbv_ctx* ctx, const u8* mosaic, RawGeom r, u8* dst, Geom g, int batch, BayerDeep deep)
{
    const char* who = "launch_ingest_deep";
    RC(check_raw_format(ctx, r.fmt, g.w, g.h, who));
    if (!raw_fmt_bayer(r.fmt) || !deep.tab || !bayer_bits_ok(r.fmt, deep.bits))
        return cbv_fail(ctx, CBV_ERR_ARG, "%s: format %d (%s) with tables of %d bits", who, r.fmt, raw_fmt_name(r.fmt), deep.bits);
    if (batch <= 0 || !mosaic || !dst || g.stride < g.w * 3 || r.stride0 < bayer_row_bytes(r.fmt, g.w))
        return cbv_fail(ctx, CBV_ERR_ARG, "%s: bad planes or strides", who);
    // the dword stores: every BGR row of every frame starts on a dword boundary (the loads work at any address)
    const bool wide = (((size_t)g.w | (size_t)dst | (size_t)g.stride | g.frame_stride) & 3) == 0;
    const DeepDev d = {deep.tab, deep.bits, raw_fmt_enc(r.fmt), r.fmt & 0x30};
    const bool lds = deep.bits <= DEEP_LDS_BITS;
    prof_begin(ctx, CBV_K_INGEST_BAYER_DEEP);
    if (wide && lds) ingest_deep_launch<4, true>(ctx, mosaic, r, dst, g, batch, d);
    else if (wide) ingest_deep_launch<4, false>(ctx, mosaic, r, dst, g, batch, d);
    else if (lds) ingest_deep_launch<2, true>(ctx, mosaic, r, dst, g, batch, d);
    else ingest_deep_launch<2, false>(ctx, mosaic, r, dst, g, batch, d);
    prof_end(ctx, CBV_K_INGEST_BAYER_DEEP);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

int launch_ingest_any(cbv_ctx* ctx, RawPlanes planes, RawGeom r, u8* dst, Geom g, int batch, int cs, BayerDeep deep)
{
    if (raw_fmt_bayer(r.fmt) && bayer_deep(r.fmt, deep)) return launch_ingest_deep(ctx, planes.p[0], r, dst, g, batch, deep);
    return launch_ingest(ctx, planes, r, dst, g, batch, cs);
}
