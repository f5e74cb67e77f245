// Developed mosaics on the device (include/cbv.h): the raw sample of a site in every encoding, the colour a site carries with
// the layout as a run-time value, and cbv_bayer.h's demosaic with the layout as a run-time value.  For k_ingest_deep.hip and the
// warp of a developed mosaic (WarpDeep, warp_gather.h).  The encoding and the layout's two phase bits are uniform over a
// launch and travel as kernel arguments, so one kernel serves the four layouts and the four encodings: d_bayer_bgr works out
// all five candidate sums whatever the phase, and the encoding is a uniform switch at the fetch.
#pragma once
#include "cbv_bayer.h"

// what a kernel knows of a developed mosaic; ph = the layout's phase bits as the format id has them (0x10 blue where RGGB
// has red, 0x20 the row starts with green), enc = raw_fmt_enc, tab = [3][1 << bits] bytes, B G R
struct DeepDev {
    const u8* tab;
    int bits, enc, ph;
};

// the colour of site (x, y) as the BGR channel index: BayerLay's rule (cbv_bayer.h) with the layout at run time
__device__ __forceinline__ int d_deep_colour(int ph, int x, int y)
{
    const int ex = (x & 1) ^ ((ph >> 5) & 1);
    if (ex != (y & 1)) return 1;
    return ((y & 1) ^ ((ph >> 4) & 1)) ? 0 : 2; // C0 (even rows) is red, or blue with 0x10
}

// raw sample x of the row that starts at `row`, by byte loads (a 16-bit sample: one two-byte load at any address)
__device__ __forceinline__ u32 d_deep_sample(const u8* __restrict__ row, int x, int enc)
{
    if (enc == BAYER_ENC_16) {
        u16 v;
        __builtin_memcpy(&v, row + 2 * (size_t)x, 2);
        return v;
    }
    if (enc == BAYER_ENC_10P) {
        const u8* g = row + 5 * (size_t)(x >> 2);
        const int i = x & 3;
        return ((u32)g[i] << 2) | (((u32)g[4] >> (2 * i)) & 3u);
    }
    if (enc == BAYER_ENC_12P) {
        const u8* g = row + 3 * (size_t)(x >> 1);
        return (x & 1) ? ((u32)g[1] << 4) | ((u32)g[2] >> 4) : ((u32)g[0] << 4) | ((u32)g[2] & 15u);
    }
    return row[x];
}

// The raw samples x0 .. x0 + 3 of a row (all four inside it), with wide loads at any address, and no byte outside the bytes of
// the groups that hold the four samples.  8-bit: one 4-byte load.  16-bit: one 8-byte load.  RAW10: the samples lie in the
// groups g0 = x0 >> 2 and g1 = (x0 + 3) >> 2 (the same when x0 % 4 == 0); per group one 4-byte load and the byte of low bits.
// RAW12: the pairs p0 = x0 >> 1 and p0 + 1 are six bytes, one 4-byte and one 2-byte load; an odd x0 reaches into the pair
// p0 + 2, whose three bytes are a 2-byte load and a byte (an even x0 loads the pair p0 + 1 again: the address is chosen, the
// load is not skipped).
__device__ __forceinline__ void d_deep_row4(const u8* __restrict__ row, int x0, int enc, u32 (&s)[4])
{
    if (enc == BAYER_ENC_16) {
        u64 v;
        __builtin_memcpy(&v, row + 2 * (size_t)x0, 8);
#pragma unroll
        for (int j = 0; j < 4; j++) s[j] = (u32)(v >> (16 * j)) & 0xFFFFu;
    } else if (enc == BAYER_ENC_10P) {
        const int g0 = x0 >> 2, g1 = (x0 + 3) >> 2;
        const u8* a = row + 5 * (size_t)g0;
        const u8* b = row + 5 * (size_t)g1;
        u32 la, lb;
        __builtin_memcpy(&la, a, 4);
        __builtin_memcpy(&lb, b, 4);
        const u32 ha = a[4], hb = b[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int x = x0 + j, i = x & 3;
            const bool first = (x >> 2) == g0;
            const u32 lo = first ? la : lb, hi = first ? ha : hb;
            s[j] = (((lo >> (8 * i)) & 255u) << 2) | ((hi >> (2 * i)) & 3u);
        }
    } else if (enc == BAYER_ENC_12P) {
        const int p0 = x0 >> 1, p2 = (x0 + 3) >> 1; // p2 = p0 + 1 (x0 even) or p0 + 2
        const u8* a = row + 3 * (size_t)p0;
        const u8* c = row + 3 * (size_t)p2;
        u32 w0;
        u16 w1, w2;
        __builtin_memcpy(&w0, a, 4);
        __builtin_memcpy(&w1, a + 4, 2);
        __builtin_memcpy(&w2, c, 2);
        const u64 ab = (u64)w0 | ((u64)w1 << 32);          // the pairs p0 and p0 + 1
        const u32 cc = (u32)w2 | ((u32)c[2] << 16);        // the pair p2
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int x = x0 + j, p = (x >> 1) - p0;      // 0, 1 or 2
            const u32 t = p == 2 ? cc : (u32)(ab >> (24 * p)) & 0xFFFFFFu;
            s[j] = (x & 1) ? (((t >> 8) & 255u) << 4) | ((t >> 20) & 15u) : ((t & 255u) << 4) | ((t >> 16) & 15u);
        }
    } else {
        u32 v;
        __builtin_memcpy(&v, row + x0, 4);
#pragma unroll
        for (int j = 0; j < 4; j++) s[j] = (v >> (8 * j)) & 255u;
    }
}

// d_bayer_bgr (cbv_bayer.h) with the layout's phase bits at run time: the same sums, the same selects
__device__ __forceinline__ u32 d_deep_bgr(int ph, int x, int y, u32 ra, u32 rb, u32 rc)
{
    const int a0 = (int)(ra & 255u), a1 = (int)((ra >> 8) & 255u), a2 = (int)((ra >> 16) & 255u);
    const int b0 = (int)(rb & 255u), b1 = (int)((rb >> 8) & 255u), b2 = (int)((rb >> 16) & 255u);
    const int c0 = (int)(rc & 255u), c1 = (int)((rc >> 8) & 255u), c2 = (int)((rc >> 16) & 255u);
    const int cross = (b0 + b2 + a1 + c1 + 2) >> 2;
    const int diag = (a0 + a2 + c0 + c2 + 2) >> 2;
    const int hp = (b0 + b2 + 1) >> 1, vp = (a1 + c1 + 1) >> 1;
    const bool odd_row = (y & 1) != 0, green = ((x & 1) ^ ((ph >> 5) & 1)) != (y & 1);
    const int g = green ? b1 : cross;
    const int k0 = green ? (odd_row ? vp : hp) : (odd_row ? diag : b1); // C0
    const int k1 = green ? (odd_row ? hp : vp) : (odd_row ? b1 : diag); // C1
    const bool bx = (ph & 0x10) != 0;
    const int r = bx ? k1 : k0, b = bx ? k0 : k1;
    return (u32)b | ((u32)g << 8) | ((u32)r << 16);
}

// The developed byte of raw sample s at site (x, y): the site's colour's table at min(s, 2^bits - 1).  LDS: `tab` is the
// workgroup's staged copy (tables of up to 12 bits, 12 KB); otherwise the device table, read through the cache.
template <class T>
__device__ __forceinline__ u32 d_deep_byte(const T* __restrict__ tab, const DeepDev& d, u32 s, int x, int y)
{
    const u32 m = (1u << d.bits) - 1u;
    return tab[((u32)d_deep_colour(d.ph, x, y) << d.bits) + min(s, m)];
}
