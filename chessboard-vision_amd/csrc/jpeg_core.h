// Baseline JPEG (Motion-JPEG frames) as include/cbv.h defines it, shared by the kernels (k_jpeg.hip), the host twin
// (cbv_jpeg_decode_host) and the stand-alone host programs under tools/: the bit reader, the Huffman step, the block
// decode, the 1-D IDCT, the upsample taps and the colour step are ONE body each.  The header parser and the serial driver
// of the twin are host code and need neither HIP nor a GPU; this file compiles with a plain C++ compiler.
//
// Arithmetic is int32.  Sums and products are formed in uint32 and read back as int32, so a damaged stream wraps instead
// of running into signed overflow; on a stream encoded from 8-bit pixels nothing wraps (tests/ref_jpeg.py asserts that).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#if defined(__HIPCC__)
#define JP_HD __host__ __device__ static inline
#else
#define JP_HD static inline
#endif

// bits of the per-frame status word
enum { JP_ST_BAD_CODE = 1, JP_ST_NO_DATA = 2, JP_ST_RESTART = 4 };
// return codes of the parser (= CBV_OK, CBV_ERR_ARG, CBV_ERR_UNSUPPORTED)
enum { JP_OK = 0, JP_ERR_ARG = -1, JP_ERR_UNSUPPORTED = -5 };

// One Huffman table in canonical form.  With v = the next 16 bits, the code's length is the first l in 1..16 with
// v < limit[l] (limit[l] = one past the last code of length l, left-aligned; non-decreasing in l), and its symbol is
// vals[(v >> (16 - l)) + delta[l]].  No such l: not a code.
struct JpegHuff {
    uint32_t limit[17];
    int32_t delta[17];
    uint8_t vals[256];
};
struct JpegTables {
    JpegHuff dc[2], ac[2];
    uint16_t q[4][64]; // natural (row-major) order
};

// What the header says about one frame, and where the decode puts it.  Component c has bw x bh blocks (whole MCUs), its
// plane is bw * 8 bytes wide, and both its plane (bytes) and its coefficients (int16) start at element poff[c] of the
// frame's plane / coefficient buffer: a coefficient per sample.
struct JpegDesc {
    int32_t w, h, ncomp;
    int32_t hs, vs;          // luma sampling = the MCU's size in blocks (chroma is 1 x 1); 1, 1 for a gray frame
    int32_t mcux, mcuy;
    int32_t dri, nint;       // restart interval in MCUs (0: none) and the number of intervals (>= 1)
    uint32_t ent_off, ent_len;
    int32_t tq[3], td[3], ta[3];
    int32_t bw[3], bh[3];
    int32_t cw[3], ch[3];    // the component's true size, ceil(w * hs_c / hmax) x ceil(h * vs_c / vmax)
    uint32_t poff[3];
    uint32_t plane_total;
    int32_t std_tables;      // the stream has no DHT segment: Annex K's tables
    int32_t table_set;       // which JpegTables of the launch's array the frame decodes with
};

JP_HD int jpeg_natural(int k)
{
    static const uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return zz[k & 63];
}

// ---------------------------------------------------------------------------------------------------------------------
// bit reader over [pos, end) of the entropy data: FF 00 is the byte FF, FF followed by anything else (or by the end) ends
// the data, and past the end every bit is 0.  `fake` counts the zero bits appended; they sit behind the real ones.
// ---------------------------------------------------------------------------------------------------------------------
struct JpegBits {
    const uint8_t* d;
    uint32_t pos, end;
    uint32_t acc; // the next bits, left-aligned
    int32_t n;    // valid bits in acc
    int32_t fake;
};

JP_HD void jpeg_bits_init(JpegBits& b, const uint8_t* d, uint32_t pos, uint32_t end)
{
    b.d = d;
    b.pos = pos;
    b.end = end;
    b.acc = 0;
    b.n = 0;
    b.fake = 0;
}

// at least 25 bits afterwards: enough for a code (16) or a value (15)
JP_HD void jpeg_bits_fill(JpegBits& b)
{
    while (b.n <= 24) {
        uint32_t byte = 0;
        bool real = false;
        if (b.pos < b.end) {
            byte = b.d[b.pos++];
            real = true;
            if (byte == 0xFF) {
                if (b.pos < b.end && b.d[b.pos] == 0) b.pos++;
                else { // a marker, or FF as the last byte: the data ends here
                    b.pos = b.end;
                    byte = 0;
                    real = false;
                }
            }
        }
        if (!real) b.fake = b.fake > (1 << 20) ? b.fake : b.fake + 8;
        b.acc |= byte << (24 - b.n);
        b.n += 8;
    }
}
JP_HD void jpeg_bits_skip(JpegBits& b, int l)
{
    b.acc <<= l;
    b.n -= l;
}
// were appended bits consumed?  (n <= 32 of the bits are left, the appended ones last)
JP_HD bool jpeg_bits_overran(const JpegBits& b) { return b.n < b.fake; }

// The piece path's reader: the same bits, and it knows where they came from.  `hist` holds two bits for each of the last
// four bytes loaded: the raw bytes it took (1, 2 for FF 00, 0 for an appended zero byte).  After a fill 25..32 bits are
// left, so exactly those four bytes are (partly) unconsumed, and the next bit's raw position follows (jpeg_piece_run).
// At a marker `end` moves to the marker's FF and pos stays there.
struct JpegPieceBits {
    const uint8_t* d;
    uint32_t pos, end;
    uint32_t acc;
    int32_t n;
    int32_t fake;
    uint32_t hist;
};

JP_HD void jpeg_bits_fill(JpegPieceBits& b)
{
    while (b.n <= 24) {
        uint32_t byte = 0, adv = 0;
        if (b.pos < b.end) {
            byte = b.d[b.pos];
            adv = 1;
            if (byte == 0xFF) {
                if (b.pos + 1 < b.end && b.d[b.pos + 1] == 0) adv = 2;
                else { // a marker, or FF as the last byte: the data ends here
                    b.end = b.pos;
                    byte = 0;
                    adv = 0;
                }
            }
            b.pos += adv;
        }
        if (!adv) b.fake = b.fake > (1 << 20) ? b.fake : b.fake + 8;
        b.acc |= byte << (24 - b.n);
        b.n += 8;
        b.hist = (b.hist << 2 | adv) & 0xFFu;
    }
}
JP_HD void jpeg_bits_skip(JpegPieceBits& b, int l)
{
    b.acc <<= l;
    b.n -= l;
}

// the next symbol, or -1 (BR: JpegBits or JpegPieceBits)
template <class BR>
JP_HD int jpeg_huff_symbol(BR& b, const JpegHuff& t)
{
    jpeg_bits_fill(b);
    const uint32_t v = b.acc >> 16;
    int l = 1;
    while (l <= 16 && v >= t.limit[l]) l++;
    if (l > 16) return -1;
    const int idx = (int)(v >> (16 - l)) + t.delta[l];
    jpeg_bits_skip(b, l);
    return t.vals[idx & 255];
}

// s bits (1..15) as a signed value (T.81 F.2.2.1 EXTEND)
template <class BR>
JP_HD int jpeg_receive_extend(BR& b, int s)
{
    jpeg_bits_fill(b);
    const int v = (int)(b.acc >> (32 - s));
    jpeg_bits_skip(b, s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One block into out[64] (natural order), whose other entries the caller has zeroed.  Returns 0 or JP_ST_BAD_CODE; k
// only grows, and the loop ends at k = 64 at the latest.
JP_HD int jpeg_decode_block(JpegBits& b, const JpegHuff& dc, const JpegHuff& ac, int32_t& pred, int16_t* out)
{
    int s = jpeg_huff_symbol(b, dc);
    if (s < 0 || s > 15) return JP_ST_BAD_CODE;
    if (s) pred = (int32_t)((uint32_t)pred + (uint32_t)jpeg_receive_extend(b, s));
    out[0] = (int16_t)(uint16_t)(uint32_t)pred;
    int k = 1;
    while (k < 64) {
        const int rs = jpeg_huff_symbol(b, ac);
        if (rs < 0) return JP_ST_BAD_CODE;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break; // EOB
            k += 16;            // ZRL
            continue;
        }
        k += r;
        if (k > 63) return JP_ST_BAD_CODE;
        out[jpeg_natural(k)] = (int16_t)jpeg_receive_extend(b, s);
        k++;
    }
    return 0;
}

// Restart interval `iv` of a frame: its MCUs' blocks into coef (the frame's coefficient buffer, zeroed by the caller).
// [start, end) = the interval's bytes.  Decoding stops at the first bad code; what is not decoded stays 0.  Returns status bits.
JP_HD int jpeg_decode_interval(const uint8_t* data, const JpegDesc& D, const JpegTables& T, uint32_t start, uint32_t end, int iv,
                               int16_t* coef)
{
    JpegBits b;
    jpeg_bits_init(b, data, start, end);
    const int nmcu = D.mcux * D.mcuy;
    const int m0 = D.dri ? iv * D.dri : 0;
    int m1 = D.dri ? m0 + D.dri : nmcu;
    if (m1 > nmcu) m1 = nmcu;
    int32_t pred0 = 0, pred1 = 0, pred2 = 0;
    int st = 0;
    for (int m = m0; m < m1 && !st; m++) {
        const int my = m / D.mcux, mx = m - my * D.mcux;
        for (int c = 0; c < D.ncomp && !st; c++) {
            const int ch = c == 0 ? D.hs : 1, cv = c == 0 ? D.vs : 1;
            const JpegHuff& dc = T.dc[D.td[c] & 1];
            const JpegHuff& ac = T.ac[D.ta[c] & 1];
            int32_t& pred = c == 0 ? pred0 : c == 1 ? pred1 : pred2;
            for (int by = 0; by < cv && !st; by++)
                for (int bx = 0; bx < ch && !st; bx++) {
                    const size_t blk = (size_t)(my * cv + by) * D.bw[c] + (mx * ch + bx);
                    st |= jpeg_decode_block(b, dc, ac, pred, coef + D.poff[c] + blk * 64);
                }
        }
    }
    if (jpeg_bits_overran(b)) st |= JP_ST_NO_DATA;
    return st;
}

// is data[i], data[i + 1] a restart marker (i + 1 < end)?
JP_HD bool jpeg_is_rst(const uint8_t* data, uint32_t i, uint32_t end) { return i + 1 < end && data[i] == 0xFF && (data[i + 1] & 0xF8) == 0xD0; }

// bytes [*start, *end) of interval iv, given the positions of the first nfound (<= nint - 1) restart markers
JP_HD void jpeg_interval_bytes(const JpegDesc& D, const uint32_t* mpos, int nfound, int iv, uint32_t* start, uint32_t* end)
{
    const uint32_t e = D.ent_off + D.ent_len;
    if (iv > nfound) { // its marker is missing: no data
        *start = *end = e;
        return;
    }
    *start = iv == 0 ? D.ent_off : mpos[iv - 1] + 2;
    *end = iv < nfound ? mpos[iv] : e;
}

// ---------------------------------------------------------------------------------------------------------------------
// The piece path: entropy data decoded by many lanes (include/cbv.h, CBV_JPEG_ENTROPY_PIECES and _SEGMENTS).  A SEGMENT is
// a stretch of entropy data in front of which the decoder's state is known: the whole scan of a frame without DRI, or one
// restart interval (bit 0, block 0 of an MCU, a DC symbol next, predictions 0).  Piece i of a segment is bytes
// [a + i S, a + (i + 1) S) of its bytes [a, b).  The decoder's state between two symbols (a symbol = a Huffman code and its
// value bits) is a JpegPieceState: the raw position of the next bit (never the 00 of an FF 00 pair), the block within the
// MCU and the zig-zag index k (0: a DC symbol is next).  X[i] = the state at the first symbol boundary at or past piece i's
// end.  A lane that meets a bad code, or the end of the data (every real bit consumed), has no such boundary: its X[i] is
// the guess piece i + 1 starts round 0 from, marked JP_PS_DEAD or JP_PS_ENDED.  The mark is not part of the next lane's
// entry, so a mark that came from a wrong guess holds up nobody, and lanes behind a true mark settle like all others.  With
// the true state in front of a segment's piece 0 its X are unique; up to the first marked piece they are the serial decode's
// own, that piece is where the serial decode of the segment dies or runs out of data, and nothing behind it in the segment
// is written.  Segments share nothing: a piece takes its entry from the piece before it in its own segment only.
// ---------------------------------------------------------------------------------------------------------------------
enum { JP_PS_ENDED = 1 << 12, JP_PS_DEAD = 1 << 13 };
enum { JP_PIECE_DEFAULT = 64 }; // bytes; DESIGN.md section 6o has the measurement behind it
struct JpegPieceState {
    uint32_t pos;
    uint32_t w; // bit in byte | block in MCU << 3 | k << 6 | JP_PS_* (marks of an exit, see above)
};
struct JpegPieceStats {
    uint32_t pieces, rounds, settled;
};
// bytes [a, b) of the stream, and the blocks of the scan (MCU by MCU) they hold: `blocks` of them from block `first`
struct JpegSegment {
    uint32_t a, b;
    uint32_t first, blocks;
};
JP_HD bool jpeg_piece_same(const JpegPieceState& a, const JpegPieceState& b) { return a.pos == b.pos && a.w == b.w; }
// pieces of S bytes in `len` bytes; an empty stretch is one (empty) piece
JP_HD uint32_t jpeg_piece_count(uint32_t len, uint32_t S)
{
    const uint32_t n = len / S + (len % S ? 1u : 0u);
    return n ? n : 1u;
}
JP_HD uint32_t jpeg_piece_count(const JpegDesc& D, uint32_t S) { return jpeg_piece_count(D.ent_len, S); }
JP_HD uint32_t jpeg_piece_end(const JpegSegment& G, uint32_t S, uint32_t i, uint32_t npieces)
{
    return i + 1 >= npieces ? G.b : G.a + (i + 1) * S;
}
JP_HD int jpeg_mcu_blocks(const JpegDesc& D) { return D.ncomp == 1 ? 1 : D.hs * D.vs + 2; }
JP_HD uint32_t jpeg_scan_blocks(const JpegDesc& D) { return (uint32_t)(D.mcux * D.mcuy) * (uint32_t)jpeg_mcu_blocks(D); }
// the whole scan as one segment (a frame without DRI)
JP_HD JpegSegment jpeg_scan_segment(const JpegDesc& D)
{
    const JpegSegment G = {D.ent_off, D.ent_off + D.ent_len, 0u, jpeg_scan_blocks(D)};
    return G;
}
// Segment j of a frame: restart interval j with jpeg_interval_bytes' bytes (an interval whose marker is missing is empty, at
// the data's end) and the blocks of its MCUs [j dri, min((j + 1) dri, mcus)); the scan itself for a frame without DRI.
JP_HD JpegSegment jpeg_frame_segment(const JpegDesc& D, const uint32_t* mpos, int nfound, uint32_t j)
{
    if (!D.dri) return jpeg_scan_segment(D);
    JpegSegment G;
    jpeg_interval_bytes(D, mpos, nfound, (int)j, &G.a, &G.b);
    if (G.b < G.a) G.b = G.a; // (markers in order lie two bytes apart at least: cannot happen)
    const uint32_t nmcu = (uint32_t)(D.mcux * D.mcuy), bpm = (uint32_t)jpeg_mcu_blocks(D);
    const uint32_t m0 = j * (uint32_t)D.dri < nmcu ? j * (uint32_t)D.dri : nmcu;
    const uint32_t m1 = nmcu - m0 < (uint32_t)D.dri ? nmcu : m0 + (uint32_t)D.dri;
    G.first = m0 * bpm;
    G.blocks = (m1 - m0) * bpm;
    return G;
}
// the component of block `blk` of an MCU
JP_HD int jpeg_mcu_comp(const JpegDesc& D, int blk)
{
    const int nl = D.ncomp == 1 ? 1 : D.hs * D.vs;
    return blk < nl ? 0 : blk - nl + 1;
}
// where block B of the scan (MCU by MCU, as jpeg_decode_interval walks them) lies in the coefficient buffer
JP_HD size_t jpeg_scan_block_elem(const JpegDesc& D, uint32_t B)
{
    const uint32_t bpm = (uint32_t)jpeg_mcu_blocks(D);
    const uint32_t m = B / bpm;
    const int blk = (int)(B - m * bpm);
    const int c = jpeg_mcu_comp(D, blk);
    const int my = (int)(m / (uint32_t)D.mcux), mx = (int)(m - (uint32_t)my * (uint32_t)D.mcux);
    const int ch = c == 0 ? D.hs : 1, cv = c == 0 ? D.vs : 1;
    const int by = c == 0 ? blk / D.hs : 0, bx = c == 0 ? blk - by * D.hs : 0;
    return D.poff[c] + ((size_t)(my * cv + by) * D.bw[c] + (mx * ch + bx)) * 64;
}
// block j of component c in scan order, as a block number of the scan
JP_HD uint32_t jpeg_comp_block(const JpegDesc& D, int c, uint32_t j)
{
    const uint32_t nl = D.ncomp == 1 ? 1u : (uint32_t)(D.hs * D.vs);
    const uint32_t per = c == 0 ? nl : 1u, first = c == 0 ? 0u : nl + (uint32_t)c - 1u;
    const uint32_t m = j / per;
    return m * (uint32_t)jpeg_mcu_blocks(D) + first + (j - m * per);
}
// how many of the scan's first ndc blocks are component c's
JP_HD uint32_t jpeg_comp_blocks_in(const JpegDesc& D, int c, uint32_t ndc)
{
    const uint32_t bpm = (uint32_t)jpeg_mcu_blocks(D);
    const uint32_t nl = D.ncomp == 1 ? 1u : (uint32_t)(D.hs * D.vs);
    const uint32_t per = c == 0 ? nl : 1u, first = c == 0 ? 0u : nl + (uint32_t)c - 1u;
    const uint32_t m = ndc / bpm, rem = ndc - m * bpm;
    const uint32_t part = rem <= first ? 0u : rem - first > per ? per : rem - first;
    return m * per + part;
}

// what lane i > 0 starts round 0 from: the first bit of its piece (behind the 00 of an FF 00 pair cut by the boundary), a
// DC symbol of block 0
// (i = the number of pieces: the segment's end)
JP_HD JpegPieceState jpeg_piece_guess(const uint8_t* d, const JpegSegment& G, uint32_t S, uint32_t i, uint32_t npieces)
{
    JpegPieceState x;
    x.pos = i >= npieces ? G.b : G.a + i * S;
    x.w = 0;
    if (i && i < npieces && d[x.pos] == 0 && d[x.pos - 1] == 0xFF) x.pos++;
    return x;
}

// One symbol at zig-zag index k (0: the DC symbol) with the block's tables.  Returns the k behind it (64 or more: the
// block is complete) or -1 for a bad code; *at = the zig-zag index of the coefficient it carried (-1: none), *val = its
// value (k = 0: the DC difference).  Consumes what jpeg_decode_block consumes, bad codes included.
JP_HD int jpeg_piece_step(JpegPieceBits& b, const JpegHuff& dc, const JpegHuff& ac, int k, int* at, int* val)
{
    *at = -1;
    *val = 0;
    if (k == 0) {
        const int s = jpeg_huff_symbol(b, dc);
        if (s < 0 || s > 15) return -1;
        if (s) *val = jpeg_receive_extend(b, s);
        *at = 0;
        return 1;
    }
    const int rs = jpeg_huff_symbol(b, ac);
    if (rs < 0) return -1;
    const int r = rs >> 4, s = rs & 15;
    if (s == 0) return r != 15 ? 64 : k + 16; // EOB, ZRL
    k += r;
    if (k > 63) return -1;
    *val = jpeg_receive_extend(b, s);
    *at = k;
    return k + 1;
}

// Piece i of the npieces (S bytes each) of segment G decoded from `entry`, whose marks are ignored.  W false, a round: stops
// at the first symbol boundary at or past the piece's end and returns that state, or the marked guess of piece i + 1 where
// the data ended or a code was bad; *nblocks = the blocks completed on the way.  W true, the write pass from the piece's
// true entry, whose block number in the scan is B: the AC coefficients go in place and the DC DIFFERENCE into out[0]; the
// lane that meets the segment's end goes on through the zero bits behind it as the serial decode does, until the segment's
// blocks are done or a code is bad.  *status gets JP_ST_* bits, *ndc one more than the last block (of the scan) whose DC
// symbol was decoded.  No block outside [G.first, G.first + G.blocks) is touched, and no byte at or past G.b is read (a
// restart marker never is).  max_steps bounds the loop: 8 S + 8 for a round (every symbol takes a bit of the piece),
// 64 (segment blocks + 1) for the write pass (a block has at most 64 symbols).
template <bool W>
JP_HD JpegPieceState jpeg_piece_run(const uint8_t* d, const JpegDesc& D, const JpegTables& T, JpegPieceState entry, const JpegSegment& G, uint32_t S,
                                    uint32_t i, uint32_t npieces, uint32_t max_steps, uint32_t* nblocks, int16_t* coef, uint32_t B, int* status,
                                    uint32_t* ndc)
{
    *nblocks = 0;
    entry.w &= 0xFFFu;
    const uint32_t total = G.first + G.blocks;
    if (W && (B < G.first || B >= total)) return entry;
    const uint32_t pend = jpeg_piece_end(G, S, i, npieces);
    JpegPieceBits b;
    b.d = d;
    b.pos = entry.pos;
    b.end = G.b;
    b.acc = 0;
    b.n = 0;
    b.fake = 0;
    b.hist = 0;
    jpeg_bits_fill(b);
    jpeg_bits_skip(b, (int)(entry.w & 7u));
    int blk = (int)(entry.w >> 3) & 7, k = (int)(entry.w >> 6) & 63;
    const int bpm = jpeg_mcu_blocks(D);
    int16_t* out = (W && k) ? coef + jpeg_scan_block_elem(D, B) : nullptr;
    uint32_t done = 0;
    int st = 0;
    JpegPieceState x = entry;
    for (uint32_t step = 0;; step++) {
        jpeg_bits_fill(b);
        const uint32_t h = b.hist;
        const bool ended = ((h >> 6) & 3u) == 0; // the oldest of the four bytes left is an appended one: no real bit is left
        x.pos = b.pos - ((h & 3u) + ((h >> 2) & 3u) + ((h >> 4) & 3u) + ((h >> 6) & 3u));
        x.w = (uint32_t)(32 - b.n) | (uint32_t)blk << 3 | (uint32_t)k << 6;
        if (ended && !W) {
            x = jpeg_piece_guess(d, G, S, i + 1, npieces);
            x.w |= JP_PS_ENDED;
            break;
        }
        if (!ended && x.pos >= pend) break;
        if (W && B + done >= total) break;
        if (step >= max_steps) break;
        const int c = jpeg_mcu_comp(D, blk);
        int at, val;
        k = jpeg_piece_step(b, T.dc[D.td[c] & 1], T.ac[D.ta[c] & 1], k, &at, &val);
        if (k < 0) {
            st |= JP_ST_BAD_CODE;
            if (!W) {
                x = jpeg_piece_guess(d, G, S, i + 1, npieces);
                x.w |= JP_PS_DEAD;
            }
            break;
        }
        if (W && at >= 0) {
            if (at == 0) {
                out = coef + jpeg_scan_block_elem(D, B + done);
                *ndc = B + done + 1;
            }
            out[jpeg_natural(at)] = (int16_t)val;
        }
        if (k >= 64) {
            k = 0;
            blk = blk + 1 == bpm ? 0 : blk + 1;
            done++;
        }
    }
    if (W) {
        if (b.n < b.fake) st |= JP_ST_NO_DATA;
        *status |= st;
    }
    *nblocks = done;
    return x;
}

// ---------------------------------------------------------------------------------------------------------------------
// IDCT: libjpeg's jidctint (slow integer, CONST_BITS 13, PASS1_BITS 2) on dequantised coefficients
// ---------------------------------------------------------------------------------------------------------------------
JP_HD int32_t jpeg_descale(uint32_t x, int n) { return (int32_t)(x + (1u << (n - 1))) >> n; }

// one 8-point pass, in[] and out[] `step` apart
JP_HD void jpeg_idct_1d(const int32_t* in, int istep, int32_t* out, int ostep, int shift)
{
    typedef uint32_t U;
    U z2 = (U)in[2 * istep], z3 = (U)in[6 * istep];
    U z1 = (z2 + z3) * 4433u;
    U tmp2 = z1 - z3 * 15137u;
    U tmp3 = z1 + z2 * 6270u;
    z2 = (U)in[0];
    z3 = (U)in[4 * istep];
    U tmp0 = (z2 + z3) << 13;
    U tmp1 = (z2 - z3) << 13;
    const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = (U)in[7 * istep];
    tmp1 = (U)in[5 * istep];
    tmp2 = (U)in[3 * istep];
    tmp3 = (U)in[1 * istep];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    U z4 = tmp1 + tmp3;
    const U z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u;
    tmp1 *= 16819u;
    tmp2 *= 25172u;
    tmp3 *= 12299u;
    z1 *= (U)-7373;
    z2 *= (U)-20995;
    z3 *= (U)-16069;
    z4 *= (U)-3196;
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    out[0 * ostep] = jpeg_descale(tmp10 + tmp3, shift);
    out[7 * ostep] = jpeg_descale(tmp10 - tmp3, shift);
    out[1 * ostep] = jpeg_descale(tmp11 + tmp2, shift);
    out[6 * ostep] = jpeg_descale(tmp11 - tmp2, shift);
    out[2 * ostep] = jpeg_descale(tmp12 + tmp1, shift);
    out[5 * ostep] = jpeg_descale(tmp12 - tmp1, shift);
    out[3 * ostep] = jpeg_descale(tmp13 + tmp0, shift);
    out[4 * ostep] = jpeg_descale(tmp13 - tmp0, shift);
}

JP_HD uint8_t jpeg_clamp(int32_t x) { return (uint8_t)(x < 0 ? 0 : x > 255 ? 255 : x); }

// one block: coef[64] (natural order) times q[64] -> ws[64] samples, row-major (the caller stores them)
JP_HD void jpeg_idct_block(const int16_t* coef, const uint16_t* q, int32_t* ws)
{
    int32_t in[64];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 64; i++) in[i] = (int32_t)coef[i] * (int32_t)q[i];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 8; c++) jpeg_idct_1d(in + c, 8, ws + c, 8, 11);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 8; r++) {
        int32_t row[8];
        for (int i = 0; i < 8; i++) row[i] = ws[r * 8 + i];
        jpeg_idct_1d(row, 1, ws + r * 8, 1, 18);
        for (int i = 0; i < 8; i++) ws[r * 8 + i] = jpeg_clamp((int32_t)((uint32_t)ws[r * 8 + i] + 128u));
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// upsampling ("fancy" triangle filter on the component's true size, edges replicated) and the colour step
// ---------------------------------------------------------------------------------------------------------------------
JP_HD int jpeg_chroma_at(const uint8_t* p, int stride, int cw, int ch, int hs, int vs, int x, int y)
{
    if (hs == 1) return p[(size_t)y * stride + x];
    if (cw <= 2) return p[(size_t)(vs == 2 ? y >> 1 : y) * stride + (x >> 1)]; // libjpeg-turbo: no filter on a component 1 or 2 wide
    const int i = x >> 1;
    const int in = (x & 1) ? (i + 1 < cw ? i + 1 : cw - 1) : (i > 0 ? i - 1 : 0);
    if (vs == 1) {
        const uint8_t* row = p + (size_t)y * stride;
        return (3 * row[i] + row[in] + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int j = y >> 1;
    const int jn = (y & 1) ? (j + 1 < ch ? j + 1 : ch - 1) : (j > 0 ? j - 1 : 0);
    const uint8_t* r0 = p + (size_t)j * stride;
    const uint8_t* r1 = p + (size_t)jn * stride;
    const int s = 3 * r0[i] + r1[i], sn = 3 * r0[in] + r1[in];
    return (3 * s + sn + ((x & 1) ? 7 : 8)) >> 4;
}

JP_HD void jpeg_ycc_to_bgr(int y, int cb, int cr, uint8_t* bgr)
{
    cb -= 128;
    cr -= 128;
    bgr[0] = jpeg_clamp(y + ((116130 * cb + 32768) >> 16));
    bgr[1] = jpeg_clamp(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    bgr[2] = jpeg_clamp(y + ((91881 * cr + 32768) >> 16));
}

// pixel (x, y) of the frame from its planes
JP_HD void jpeg_pixel(const JpegDesc& D, const uint8_t* planes, int x, int y, uint8_t* bgr)
{
    const int Y = planes[D.poff[0] + (size_t)y * (D.bw[0] * 8) + x];
    if (D.ncomp == 1) {
        bgr[0] = bgr[1] = bgr[2] = (uint8_t)Y;
        return;
    }
    const int cb = jpeg_chroma_at(planes + D.poff[1], D.bw[1] * 8, D.cw[1], D.ch[1], D.hs, D.vs, x, y);
    const int cr = jpeg_chroma_at(planes + D.poff[2], D.bw[2] * 8, D.cw[2], D.ch[2], D.hs, D.vs, x, y);
    jpeg_ycc_to_bgr(Y, cb, cr, bgr);
}

// =====================================================================================================================
// host only from here: tables, the header parser, the serial twin
// =====================================================================================================================

// false: the counts are not those of a prefix code of at most 256 symbols
static inline bool jpeg_build_huff(const uint8_t bits[16], const uint8_t* vals, int nvals, JpegHuff* t)
{
    memset(t, 0, sizeof(*t));
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; l++) {
        t->delta[l] = k - (int)code;
        code += bits[l - 1];
        k += bits[l - 1];
        if (code > (1u << l) || k > 256 || k > nvals) return false;
        t->limit[l] = code << (16 - l);
        code <<= 1;
    }
    memcpy(t->vals, vals, (size_t)k);
    return true;
}

// Annex K.3's typical tables: what a stream without DHT means (ids: DC 0 / AC 0 luminance, DC 1 / AC 1 chrominance)
static inline void jpeg_std_tables(JpegTables* T)
{
    static const uint8_t dc_l_bits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
    static const uint8_t dc_c_bits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
    static const uint8_t dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    static const uint8_t ac_l_bits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
    static const uint8_t ac_l_vals[162] = {
        0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
        0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
        0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
        0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
        0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
        0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
        0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
        0xfa};
    static const uint8_t ac_c_bits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
    static const uint8_t ac_c_vals[162] = {
        0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
        0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
        0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
        0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
        0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
        0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
        0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
        0xfa};
    jpeg_build_huff(dc_l_bits, dc_vals, 12, &T->dc[0]);
    jpeg_build_huff(dc_c_bits, dc_vals, 12, &T->dc[1]);
    jpeg_build_huff(ac_l_bits, ac_l_vals, 162, &T->ac[0]);
    jpeg_build_huff(ac_c_bits, ac_c_vals, 162, &T->ac[1]);
}

#define JP_FAIL(code, ...)                     \
    do {                                       \
        snprintf(msg, msg_cap, __VA_ARGS__);   \
        return (code);                         \
    } while (0)

// The header of one JPEG stream, up to and including SOS: reads no entropy data.  JP_OK, or JP_ERR_ARG (malformed) /
// JP_ERR_UNSUPPORTED (well-formed, outside what include/cbv.h accepts) with the reason in msg.
static inline int jpeg_parse_header(const uint8_t* d, size_t n, JpegDesc* D, JpegTables* T, char* msg, size_t msg_cap)
{
    memset(D, 0, sizeof(*D));
    memset(T, 0, sizeof(*T));
    if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) JP_FAIL(JP_ERR_ARG, "not a JPEG stream (no SOI)");
    if (n > 0x7FFFFFFFu) JP_FAIL(JP_ERR_ARG, "a stream of 2 GiB or more");
    bool have_sof = false, any_dht = false;
    bool have_q[4] = {false, false, false, false}, have_dc[2] = {false, false}, have_ac[2] = {false, false};
    int comp_id[3] = {0, 0, 0}, comp_h[3] = {1, 1, 1}, comp_v[3] = {1, 1, 1};
    int adobe_transform = -1;
    size_t i = 2;
    for (;;) {
        if (i >= n) JP_FAIL(JP_ERR_ARG, "the header ends before SOS");
        if (d[i] != 0xFF) JP_FAIL(JP_ERR_ARG, "byte 0x%02X at offset %zu where a marker should be", d[i], i);
        while (i < n && d[i] == 0xFF) i++; // fill bytes
        if (i >= n) JP_FAIL(JP_ERR_ARG, "the header ends before SOS");
        const int m = d[i++];
        if (m == 0xD9) JP_FAIL(JP_ERR_ARG, "EOI before SOS");
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD8)) JP_FAIL(JP_ERR_ARG, "marker FF%02X in the header", m);
        if (i + 2 > n) JP_FAIL(JP_ERR_ARG, "segment FF%02X is cut off", m);
        const size_t L = (size_t)d[i] * 256 + d[i + 1];
        if (L < 2 || i + L > n) JP_FAIL(JP_ERR_ARG, "segment FF%02X has length %zu, %zu bytes are left", m, L, n - i);
        const uint8_t* s = d + i + 2;
        const size_t sl = L - 2;
        i += L;
        if (m == 0xC2 || m == 0xC6 || m == 0xCA || m == 0xCE) JP_FAIL(JP_ERR_UNSUPPORTED, "progressive JPEG (SOF%d)", m - 0xC0);
        if (m >= 0xC9 && m <= 0xCF && m != 0xCC) JP_FAIL(JP_ERR_UNSUPPORTED, "arithmetic coding (SOF%d)", m - 0xC0);
        if (m == 0xCC) JP_FAIL(JP_ERR_UNSUPPORTED, "arithmetic coding (DAC)");
        if (m == 0xC1 || m == 0xC3 || m == 0xC5 || m == 0xC7) {
            if (m == 0xC1 && sl >= 1 && s[0] == 12) JP_FAIL(JP_ERR_UNSUPPORTED, "12-bit samples (SOF1)");
            JP_FAIL(JP_ERR_UNSUPPORTED, "SOF%d: only baseline (SOF0) streams are decoded", m - 0xC0);
        }
        if (m == 0xC0) {
            if (have_sof) JP_FAIL(JP_ERR_ARG, "two SOF segments");
            if (sl < 6) JP_FAIL(JP_ERR_ARG, "SOF0 is cut off");
            if (s[0] != 8) JP_FAIL(JP_ERR_UNSUPPORTED, "%d-bit samples", s[0]);
            D->h = s[1] * 256 + s[2];
            D->w = s[3] * 256 + s[4];
            D->ncomp = s[5];
            if (D->ncomp == 4) JP_FAIL(JP_ERR_UNSUPPORTED, "four components (CMYK / YCCK)");
            if (D->ncomp != 1 && D->ncomp != 3) JP_FAIL(JP_ERR_UNSUPPORTED, "%d components", D->ncomp);
            if (sl != (size_t)6 + 3 * D->ncomp) JP_FAIL(JP_ERR_ARG, "SOF0 length does not fit its %d components", D->ncomp);
            if (D->w < 1 || D->h < 1) JP_FAIL(JP_ERR_ARG, "a %d x %d frame", D->w, D->h);
            for (int c = 0; c < D->ncomp; c++) {
                comp_id[c] = s[6 + 3 * c];
                comp_h[c] = s[7 + 3 * c] >> 4;
                comp_v[c] = s[7 + 3 * c] & 15;
                D->tq[c] = s[8 + 3 * c];
                if (comp_h[c] < 1 || comp_h[c] > 4 || comp_v[c] < 1 || comp_v[c] > 4) JP_FAIL(JP_ERR_ARG, "sampling factor %d x %d", comp_h[c], comp_v[c]);
                if (D->tq[c] > 3) JP_FAIL(JP_ERR_ARG, "quantisation table id %d", D->tq[c]);
            }
            have_sof = true;
        } else if (m == 0xDB) {
            size_t p = 0;
            while (p < sl) {
                const int pq = s[p] >> 4, tq = s[p] & 15;
                if (pq == 1) JP_FAIL(JP_ERR_UNSUPPORTED, "16-bit quantisation table");
                if (pq > 1 || tq > 3) JP_FAIL(JP_ERR_ARG, "DQT with precision %d, id %d", pq, tq);
                if (p + 65 > sl) JP_FAIL(JP_ERR_ARG, "DQT is cut off");
                for (int k = 0; k < 64; k++) T->q[tq][jpeg_natural(k)] = s[p + 1 + k];
                have_q[tq] = true;
                p += 65;
            }
        } else if (m == 0xC4) {
            size_t p = 0;
            while (p < sl) {
                const int tc = s[p] >> 4, th = s[p] & 15;
                if (tc > 1) JP_FAIL(JP_ERR_ARG, "DHT with class %d", tc);
                if (th > 1) JP_FAIL(JP_ERR_UNSUPPORTED, "Huffman table id %d: baseline has two tables per class", th);
                if (p + 17 > sl) JP_FAIL(JP_ERR_ARG, "DHT is cut off");
                int cnt = 0;
                for (int k = 0; k < 16; k++) cnt += s[p + 1 + k];
                if (cnt > 256 || p + 17 + cnt > sl) JP_FAIL(JP_ERR_ARG, "DHT with %d symbols is cut off", cnt);
                if (!jpeg_build_huff(s + p + 1, s + p + 17, cnt, tc ? &T->ac[th] : &T->dc[th])) JP_FAIL(JP_ERR_ARG, "DHT code lengths are no prefix code");
                (tc ? have_ac : have_dc)[th] = true;
                any_dht = true;
                p += 17 + (size_t)cnt;
            }
        } else if (m == 0xDD) {
            if (sl != 2) JP_FAIL(JP_ERR_ARG, "DRI of length %zu", L);
            D->dri = s[0] * 256 + s[1];
        } else if (m == 0xEE) {
            if (sl >= 12 && !memcmp(s, "Adobe", 5)) adobe_transform = s[11];
        } else if (m == 0xDA) {
            if (!have_sof) JP_FAIL(JP_ERR_ARG, "SOS before SOF");
            if (sl < 1) JP_FAIL(JP_ERR_ARG, "SOS is cut off");
            const int ns = s[0];
            if (ns < 1 || ns > 4 || sl != (size_t)4 + 2 * ns) JP_FAIL(JP_ERR_ARG, "SOS with %d components and length %zu", ns, L);
            if (ns != D->ncomp) JP_FAIL(JP_ERR_UNSUPPORTED, "several scans (the first has %d of %d components)", ns, D->ncomp);
            for (int c = 0; c < ns; c++) {
                if (s[1 + 2 * c] != comp_id[c]) JP_FAIL(JP_ERR_ARG, "SOS names component %d where the frame has %d", s[1 + 2 * c], comp_id[c]);
                D->td[c] = s[2 + 2 * c] >> 4;
                D->ta[c] = s[2 + 2 * c] & 15;
                if (D->td[c] > 1 || D->ta[c] > 1) JP_FAIL(JP_ERR_UNSUPPORTED, "Huffman table id above 1 in SOS");
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) JP_FAIL(JP_ERR_ARG, "SOS spectral selection / approximation is not a baseline scan's");
            break;
        }
        // APPn, COM and everything else with a length: skipped
    }
    if (D->ncomp == 3 && adobe_transform == 0) JP_FAIL(JP_ERR_UNSUPPORTED, "Adobe marker with transform 0 (RGB / CMYK samples, not YCbCr)");
    if (D->ncomp == 1) D->hs = D->vs = 1; // one component: the scan is not interleaved, its MCU is one block
    else {
        D->hs = comp_h[0];
        D->vs = comp_v[0];
        const bool ok = comp_h[1] == 1 && comp_v[1] == 1 && comp_h[2] == 1 && comp_v[2] == 1 &&
                        ((D->hs == 1 && D->vs == 1) || (D->hs == 2 && D->vs == 1) || (D->hs == 2 && D->vs == 2));
        if (!ok) JP_FAIL(JP_ERR_UNSUPPORTED, "sampling %dx%d,%dx%d,%dx%d (4:4:4, 4:2:2 and 4:2:0 are decoded)", comp_h[0], comp_v[0], comp_h[1],
                         comp_v[1], comp_h[2], comp_v[2]);
    }
    for (int c = 0; c < D->ncomp; c++)
        if (!have_q[D->tq[c]]) JP_FAIL(JP_ERR_ARG, "quantisation table %d is not defined", D->tq[c]);
    D->std_tables = any_dht ? 0 : 1;
    if (!any_dht) jpeg_std_tables(T);
    else
        for (int c = 0; c < D->ncomp; c++)
            if (!have_dc[D->td[c]] || !have_ac[D->ta[c]]) JP_FAIL(JP_ERR_ARG, "Huffman table DC %d / AC %d is not defined", D->td[c], D->ta[c]);
    if ((uint64_t)D->w * (uint64_t)D->h > (1u << 28)) JP_FAIL(JP_ERR_UNSUPPORTED, "a %d x %d frame: more than 2^28 pixels", D->w, D->h);
    D->mcux = (D->w + 8 * D->hs - 1) / (8 * D->hs);
    D->mcuy = (D->h + 8 * D->vs - 1) / (8 * D->vs);
    const int nmcu = D->mcux * D->mcuy;
    D->nint = D->dri ? (nmcu + D->dri - 1) / D->dri : 1;
    D->ent_off = (uint32_t)i;
    D->ent_len = (uint32_t)(n - i);
    uint32_t off = 0;
    for (int c = 0; c < D->ncomp; c++) {
        const int ch = c == 0 ? D->hs : 1, cv = c == 0 ? D->vs : 1;
        D->bw[c] = D->mcux * ch;
        D->bh[c] = D->mcuy * cv;
        D->cw[c] = (D->w * ch + D->hs - 1) / D->hs;
        D->ch[c] = (D->h * cv + D->vs - 1) / D->vs;
        D->poff[c] = off;
        off += (uint32_t)D->bw[c] * (uint32_t)D->bh[c] * 64u;
    }
    D->plane_total = off;
    return JP_OK;
}

// positions of the restart markers of the entropy data, in order, at most nint - 1 of them; *st gets JP_ST_RESTART
// when their count or their numbering (0..7, cycling) is wrong
static inline void jpeg_find_restarts_host(const uint8_t* d, const JpegDesc& D, std::vector<uint32_t>* mpos, int* st)
{
    mpos->clear();
    if (!D.dri) return;
    const uint32_t e = D.ent_off + D.ent_len;
    uint32_t total = 0;
    for (uint32_t i = D.ent_off; i + 1 < e; i++)
        if (jpeg_is_rst(d, i, e)) {
            if ((int)total < D.nint - 1) {
                mpos->push_back(i);
                if ((d[i + 1] & 7) != (int)(total & 7)) *st |= JP_ST_RESTART;
            }
            total++;
        }
    if ((int)total != D.nint - 1) *st |= JP_ST_RESTART;
}

// The piece path on the host, the algorithm k_jpeg_pieces runs, over the frame's segments (one: the scan of a frame without
// DRI; with `segments`, its restart intervals as the markers at mpos[0 .. nfound) bound them): the states in vectors, the
// pieces of all segments flattened; the rounds in Jacobi order (round r reads only round r - 1's exits) over all of them
// until no exit of the frame changes; then per segment the prefix sum, the first marked piece, the write pass and the DC
// pass.  coef is zeroed by the caller.  S = the piece size in bytes, a multiple of 4.  Returns status bits.
static inline int jpeg_decode_pieces_host(const uint8_t* d, const JpegDesc& D, const JpegTables& T, uint32_t S, int16_t* coef, JpegPieceStats* ps,
                                          bool segments = false, const uint32_t* mpos = nullptr, int nfound = 0)
{
    const uint32_t nseg = segments ? (uint32_t)D.nint : 1u;
    std::vector<JpegSegment> seg(nseg);
    std::vector<uint32_t> poff(nseg + 1, 0u); // segment j's pieces are poff[j] .. poff[j + 1] of the flattened ones
    uint32_t maxn = 1;
    for (uint32_t j = 0; j < nseg; j++) {
        seg[j] = segments ? jpeg_frame_segment(D, mpos, nfound, j) : jpeg_scan_segment(D);
        const uint32_t n = jpeg_piece_count(seg[j].b - seg[j].a, S);
        poff[j + 1] = poff[j] + n;
        maxn = n > maxn ? n : maxn;
    }
    const uint32_t np = poff[nseg];
    const uint32_t round_steps = 8 * S + 8;
    std::vector<JpegPieceState> cur(np), nxt(np), ent(np), r0(np);
    std::vector<uint32_t> cnt(np), sof(np);
    for (uint32_t j = 0; j < nseg; j++)
        for (uint32_t p = poff[j]; p < poff[j + 1]; p++) sof[p] = j;
    for (uint32_t p = 0; p < np; p++) { // round 0: the first piece of every segment from the true state
        const JpegSegment& G = seg[sof[p]];
        const uint32_t i = p - poff[sof[p]], n = poff[sof[p] + 1] - poff[sof[p]];
        const JpegPieceState first = {G.a, 0};
        ent[p] = i ? jpeg_piece_guess(d, G, S, i, n) : first;
        cur[p] = r0[p] = jpeg_piece_run<false>(d, D, T, ent[p], G, S, i, n, round_steps, &cnt[p], nullptr, 0, nullptr, nullptr);
    }
    uint32_t rounds = 1;
    for (uint32_t r = 1; r < maxn; r++) { // after round r the exits 0..r of every segment are true: round max n_j could change nothing
        bool changed = false;
        for (uint32_t p = 0; p < np; p++) {
            const JpegSegment& G = seg[sof[p]];
            const uint32_t i = p - poff[sof[p]], n = poff[sof[p] + 1] - poff[sof[p]];
            const JpegPieceState first = {G.a, 0};
            const JpegPieceState e = i ? cur[p - 1] : first;
            if (jpeg_piece_same(e, ent[p])) {
                nxt[p] = cur[p];
                continue;
            }
            ent[p] = e;
            nxt[p] = jpeg_piece_run<false>(d, D, T, e, G, S, i, n, round_steps, &cnt[p], nullptr, 0, nullptr, nullptr);
            changed |= !jpeg_piece_same(nxt[p], cur[p]);
        }
        cur.swap(nxt);
        if (!changed) break;
        rounds++;
    }
    int st = 0;
    uint32_t settled = 0;
    for (uint32_t p = 0; p < np; p++) settled += jpeg_piece_same(r0[p], cur[p]) ? 1u : 0u;
    for (uint32_t j = 0; j < nseg; j++) {
        const JpegSegment& G = seg[j];
        const uint32_t p0 = poff[j], n = poff[j + 1] - p0, write_steps = 64 * (G.blocks + 1);
        const JpegPieceState first = {G.a, 0};
        uint32_t last = n - 1; // the first marked piece: where the serial decode of the segment dies or runs out of data
        for (uint32_t i = 0; i < n; i++)
            if (i < last && (cur[p0 + i].w & (JP_PS_ENDED | JP_PS_DEAD))) last = i;
        uint32_t ndc = 0, B = G.first;
        for (uint32_t i = 0; i <= last; i++) {
            uint32_t done, mine = 0;
            jpeg_piece_run<true>(d, D, T, i ? cur[p0 + i - 1] : first, G, S, i, n, write_steps, &done, coef, B, &st, &mine);
            ndc = mine > ndc ? mine : ndc;
            B += cnt[p0 + i];
        }
        for (int c = 0; c < D.ncomp; c++) { // differences to predictions, mod 2^16, from 0 at the segment's start
            const uint32_t q0 = jpeg_comp_blocks_in(D, c, G.first), q1 = jpeg_comp_blocks_in(D, c, ndc);
            uint16_t pred = 0;
            for (uint32_t q = q0; q < q1; q++) {
                int16_t* o = coef + jpeg_scan_block_elem(D, jpeg_comp_block(D, c, q));
                pred = (uint16_t)(pred + (uint16_t)o[0]);
                o[0] = (int16_t)pred;
            }
        }
    }
    if (ps) {
        ps->pieces = np;
        ps->rounds = rounds;
        ps->settled = settled;
    }
    return st;
}

// The twin: coef[plane_total] and planes[plane_total] are scratch the caller provides (coef is zeroed here), bgr = h rows
// of w * 3 bytes, `stride` apart.  piece_bytes 0: every frame by restart interval; otherwise a frame without DRI goes the
// piece path with pieces of that size, and with `segments` a frame with DRI does too, its restart intervals cut into
// pieces; *ps (may be null) gets the piece path's figures (zeros for a frame by interval).
static inline void jpeg_decode_host(const uint8_t* d, const JpegDesc& D, const JpegTables& T, int16_t* coef, uint8_t* planes, uint8_t* bgr,
                                    size_t stride, int* status, uint32_t piece_bytes = 0, JpegPieceStats* ps = nullptr, bool segments = false)
{
    int st = 0;
    memset(coef, 0, (size_t)D.plane_total * sizeof(int16_t));
    if (ps) memset(ps, 0, sizeof(*ps));
    if (piece_bytes && !D.dri) st |= jpeg_decode_pieces_host(d, D, T, piece_bytes, coef, ps);
    else {
        std::vector<uint32_t> mpos;
        jpeg_find_restarts_host(d, D, &mpos, &st);
        if (piece_bytes && segments) st |= jpeg_decode_pieces_host(d, D, T, piece_bytes, coef, ps, true, mpos.data(), (int)mpos.size());
        else
            for (int iv = 0; iv < D.nint; iv++) {
                uint32_t a, b;
                jpeg_interval_bytes(D, mpos.data(), (int)mpos.size(), iv, &a, &b);
                st |= jpeg_decode_interval(d, D, T, a, b, iv, coef);
            }
    }
    for (int c = 0; c < D.ncomp; c++) {
        const int ps = D.bw[c] * 8;
        for (int by = 0; by < D.bh[c]; by++)
            for (int bx = 0; bx < D.bw[c]; bx++) {
                int32_t ws[64];
                jpeg_idct_block(coef + D.poff[c] + ((size_t)by * D.bw[c] + bx) * 64, T.q[D.tq[c]], ws);
                uint8_t* o = planes + D.poff[c] + (size_t)by * 8 * ps + bx * 8;
                for (int r = 0; r < 8; r++)
                    for (int k = 0; k < 8; k++) o[(size_t)r * ps + k] = (uint8_t)ws[r * 8 + k];
            }
    }
    if (bgr)
        for (int y = 0; y < D.h; y++)
            for (int x = 0; x < D.w; x++) jpeg_pixel(D, planes, x, y, bgr + (size_t)y * stride + (size_t)x * 3);
    *status = st;
}
