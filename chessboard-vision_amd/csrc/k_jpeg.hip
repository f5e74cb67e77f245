// Baseline JPEG decode (include/cbv.h, CBV_FMT_MJPEG): the bodies are jpeg_core.h's, the same the host twin runs.
//   k_jpeg_restarts  a workgroup per frame with DRI: the positions of FF D0..D7 in the entropy data, in order
//   k_jpeg_entropy   a lane per restart interval, (frame, interval) pairs flattened: int16 coefficients, natural order
//   k_jpeg_pieces    a workgroup per frame without DRI (B.piece_bytes > 0): the scan cut into pieces, a lane per piece; with
//                    B.segments a workgroup per frame, every restart interval cut into pieces
//   k_jpeg_idct      a lane per 8 x 8 block: dequantise, jidctint, component planes padded to whole MCUs
//   k_jpeg_color     a lane per pixel: fancy upsampling, YCbCr -> BGR, crop
// The coefficients and the planes rest in device memory between the stages (the single-frame entry point hands them out).
#include "cbv_internal.h"

#include "jpeg_core.h"

// frame f of the launch: its stream, its descriptor, and element f * stride of every output
__global__ __launch_bounds__(256) void k_jpeg_restarts(JpegBatch B)
{
    const int f = blockIdx.x, t = threadIdx.x;
    const JpegDesc& D = B.descs[f];
    if (!D.dri) return; // (the same in every lane)
    const u8* d = B.data + (size_t)f * B.data_stride;
    const u32 a = D.ent_off, e = a + D.ent_len;
    const u32 chunk = (D.ent_len + 255u) / 256u;
    u32 lo = a + (u32)t * chunk;
    if (lo > e) lo = e;
    const u32 hi = e - lo < chunk ? e : lo + chunk;
    u32 mine = 0;
    for (u32 i = lo; i < hi; i++) mine += jpeg_is_rst(d, i, e) ? 1u : 0u;
    __shared__ u32 cnt[256];
    cnt[t] = mine;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) { // inclusive prefix count
        const u32 v = t >= s ? cnt[t - s] : 0u;
        __syncthreads();
        cnt[t] += v;
        __syncthreads();
    }
    const u32 total = cnt[255];
    const u32 want = (u32)(D.nint - 1);
    u32 k = cnt[t] - mine;
    u32* mpos = B.mpos + B.ioff[f];
    bool bad = false;
    for (u32 i = lo; i < hi; i++)
        if (jpeg_is_rst(d, i, e)) {
            if (k < want) {
                mpos[k] = i;
                bad |= (u32)(d[i + 1] & 7) != (k & 7u);
            }
            k++;
        }
    if (t == 0) {
        B.nfound[f] = (int)(total < want ? total : want);
        if (total != want) bad = true;
    }
    if (bad) atomicOr(&B.status[f], JP_ST_RESTART);
}

__global__ __launch_bounds__(64) void k_jpeg_entropy(JpegBatch B)
{
    const u32 gid = blockIdx.x * 64u + threadIdx.x;
    if (gid >= B.ioff[B.nframes]) return;
    int lo = 0, hi = B.nframes; // the frame with ioff[f] <= gid < ioff[f + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (B.ioff[mid] <= gid) lo = mid;
        else hi = mid;
    }
    const int f = lo;
    const int iv = (int)(gid - B.ioff[f]);
    const JpegDesc& D = B.descs[f];
    if (B.piece_bytes && (B.segments || !D.dri)) return; // k_jpeg_pieces' frame
    u32 a, b;
    jpeg_interval_bytes(D, B.mpos + B.ioff[f], B.nfound[f], iv, &a, &b);
    const int st = jpeg_decode_interval(B.data + (size_t)f * B.data_stride, D, B.tables[D.table_set], a, b, iv, B.coef + (size_t)f * B.coef_stride);
    if (st) atomicOr(&B.status[f], st);
}

// inclusive sum of v over the workgroup's JP_PIECE_LANES lanes, through s[]; every lane calls it
#define JP_PIECE_LANES 1024
__device__ static inline u32 wg_scan_1024(u32* s, int t, u32 v)
{
    s[t] = v;
    __syncthreads();
    for (int o = 1; o < JP_PIECE_LANES; o <<= 1) {
        const u32 a = t >= o ? s[t - o] : 0u;
        __syncthreads();
        s[t] += a;
        __syncthreads();
    }
    return s[t];
}

// the same for a sum mod 2^16 that starts again at marked elements: v = the sum in bits 0..15, bit 16 set when a segment
// starts at or inside the lane's elements (the sum is then the one since the last start)
__device__ static inline u32 wg_segscan_1024(u32* s, int t, u32 v)
{
    s[t] = v;
    __syncthreads();
    for (int o = 1; o < JP_PIECE_LANES; o <<= 1) {
        const u32 a = t >= o ? s[t - o] : 0u;
        __syncthreads();
        const u32 c = s[t];
        if (!(c & 0x10000u)) s[t] = (a & 0x10000u) | ((a + c) & 0xFFFFu);
        __syncthreads();
    }
    return s[t];
}

// the segment with poff[j] <= p < poff[j + 1] (poff[0] = 0, p < poff[nseg])
__device__ static inline u32 jpeg_seg_of(const u32* poff, u32 nseg, u32 p)
{
    u32 lo = 0, hi = nseg;
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (poff[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

// flattened piece p of a frame: its segment *j, that segment's bytes and blocks, its number *i among the segment's *n pieces
template <bool SEG>
__device__ static inline JpegSegment jpeg_piece_where(const JpegDesc& D, const JpegSegment& scan, const u32* mpos, int nfound, const u32* poff,
                                                      const u32* sof, u32 p, u32 np, u32* j, u32* i, u32* n)
{
    if (!SEG) { // (`scan` = the whole scan, computed once by the caller)
        *j = 0;
        *i = p;
        *n = np;
        return scan;
    }
    const u32 g = sof[p];
    *j = g;
    *i = p - poff[g];
    *n = poff[g + 1] - poff[g];
    return jpeg_frame_segment(D, mpos, nfound, g);
}

// The piece path (jpeg_core.h).  SEG false: a frame without DRI, its scan one segment.  SEG true (B.segments): every frame,
// segment j = restart interval j as k_jpeg_restarts' markers bound it (launched first on the same stream), n_j pieces each,
// the (segment, piece) pairs flattened.  Lane t takes pieces t, t + 1024, ...  Rounds in Jacobi order, the exits
// double-buffered in the frame's scratch; a round is over at the barrier, so no lane waits for anything but its own
// workgroup.  A piece takes its entry from the piece before it in its own segment, a segment's first piece from the true
// state.  Then, per segment: the block numbers (a prefix sum over all pieces, less its value at the segment's first
// piece), the first marked piece, the write pass, and a DC scan that starts from 0 at every segment.  Every loop's bound is
// known at launch: intervals / 1024 for the segment table, pieces / 1024 per pass, at most max_j n_j rounds (all of the
// pieces for a single segment), jpeg_piece_run's step counts (8 S + 8 for a round's piece, 64 (segment blocks + 1) for a
// write pass).  What SEG true derives from the stream's contents is checked against the launch's sizes: the piece count
// against B.piece_cap, the intervals against B.seg_stride; every block number is checked against its segment inside
// jpeg_piece_run.  SEG false keeps the earlier kernel's loops: the scan's segment formed once, the write pass up to `last`.
template <bool SEG>
__global__ __launch_bounds__(JP_PIECE_LANES) void k_jpeg_pieces(JpegBatch B)
{
    const int f = blockIdx.x, t = threadIdx.x;
    const JpegDesc& D = B.descs[f];
    if (!SEG && D.dri) return; // (the same in every lane)
    const u8* d = B.data + (size_t)f * B.data_stride;
    const JpegTables& T = B.tables[D.table_set];
    const u32 S = B.piece_bytes;
    const u32 round_steps = 8u * S + 8u;
    const JpegSegment scan = jpeg_scan_segment(D); // what SEG false decodes
    int16_t* coef = B.coef + (size_t)f * B.coef_stride;
    __shared__ u32 s_scan[JP_PIECE_LANES];
    __shared__ u32 s_changed, s_ndc, s_settled, s_last, s_maxn;
    __shared__ int s_status;
    if (t == 0) {
        s_changed = 0;
        s_ndc = 0;
        s_settled = 0;
        s_status = 0;
        s_maxn = 1;
    }
    // the segment table: every segment's first piece (the exclusive sum of the n_j), its last piece, no DC symbol yet
    const u32 nseg = SEG ? (u32)D.nint : 1u;
    const u32* mpos = B.mpos + B.ioff[f];
    const int nfound = SEG ? B.nfound[f] : 0;
    u32* poff = SEG ? B.segs + (size_t)f * B.seg_stride : nullptr;
    u32* lastp = SEG ? poff + nseg + 1 : nullptr;
    u32* ndcp = SEG ? lastp + nseg : nullptr;
    u32 np, maxn;
    if (SEG) {
        if ((size_t)nseg * JPEG_SEG_WORDS + 1 > B.seg_stride) { // (the launch sized it for the frame's intervals: cannot happen)
            if (t == 0) atomicOr(&B.status[f], JP_ST_NO_DATA);
            return;
        }
        u32 carry = 0, mx = 1;
        for (u32 j0 = 0; j0 < nseg; j0 += JP_PIECE_LANES) {
            const u32 j = j0 + (u32)t;
            u32 n = 0;
            if (j < nseg) {
                const JpegSegment G = jpeg_frame_segment(D, mpos, nfound, j);
                n = jpeg_piece_count(G.b - G.a, S);
                mx = n > mx ? n : mx;
            }
            const u32 inc = wg_scan_1024(s_scan, t, n);
            if (j < nseg) {
                poff[j] = carry + inc - n;
                lastp[j] = n - 1;
                ndcp[j] = 0;
            }
            carry += s_scan[JP_PIECE_LANES - 1];
            __syncthreads();
        }
        if (t == 0) poff[nseg] = carry;
        if (mx > 1) atomicMax(&s_maxn, mx);
        __syncthreads();
        np = carry;
        maxn = s_maxn;
    } else {
        np = jpeg_piece_count(D, S);
        maxn = np;
    }
    // SEG false: np = ceil(ent_len / S) comes from the header the host parsed and sized the scratch by, as before
    if (SEG && np > B.piece_cap) { // (the same in every lane; the launch sized the scratch by the bound on the pieces: cannot happen)
        if (t == 0) atomicOr(&B.status[f], JP_ST_NO_DATA);
        return;
    }
    u32* base = B.pieces + (size_t)f * B.piece_stride;
    JpegPieceState* cur = reinterpret_cast<JpegPieceState*>(base);
    JpegPieceState* nxt = cur + np;
    JpegPieceState* ent = nxt + np;
    JpegPieceState* r0 = ent + np;
    u32* cnt = base + 8 * (size_t)np;
    u32* sof = SEG ? cnt + np : nullptr;
    if (!SEG && t == 0) s_last = np - 1;
    for (u32 p = t; p < np; p += JP_PIECE_LANES) { // round 0
        if (SEG) sof[p] = jpeg_seg_of(poff, nseg, p);
        u32 j, i, n;
        const JpegSegment G = jpeg_piece_where<SEG>(D, scan, mpos, nfound, poff, sof, p, np, &j, &i, &n);
        const JpegPieceState first = {G.a, 0u};
        const JpegPieceState e = i ? jpeg_piece_guess(d, G, S, i, n) : first;
        u32 c;
        const JpegPieceState x = jpeg_piece_run<false>(d, D, T, e, G, S, i, n, round_steps, &c, nullptr, 0u, nullptr, nullptr);
        ent[p] = e;
        cur[p] = x;
        r0[p] = x;
        cnt[p] = c;
    }
    __syncthreads();
    u32 rounds = 1;
    for (u32 r = 1; r < maxn; r++) {
        bool mine = false;
        for (u32 p = t; p < np; p += JP_PIECE_LANES) {
            u32 j, i, n;
            const JpegSegment G = jpeg_piece_where<SEG>(D, scan, mpos, nfound, poff, sof, p, np, &j, &i, &n);
            const JpegPieceState first = {G.a, 0u};
            const JpegPieceState e = i ? cur[p - 1] : first;
            const JpegPieceState was = cur[p];
            if (jpeg_piece_same(e, ent[p])) {
                nxt[p] = was;
                continue;
            }
            u32 c;
            const JpegPieceState x = jpeg_piece_run<false>(d, D, T, e, G, S, i, n, round_steps, &c, nullptr, 0u, nullptr, nullptr);
            ent[p] = e;
            nxt[p] = x;
            cnt[p] = c;
            mine |= !jpeg_piece_same(x, was);
        }
        if (mine) s_changed = r; // (r >= 1; the word is never reset, so no lane can take one round's mark for another's)
        __syncthreads();
        const bool changed = s_changed == r;
        __syncthreads();
        JpegPieceState* sw = cur;
        cur = nxt;
        nxt = sw;
        if (!changed) break; // (the same in every lane)
        rounds++;
    }
    // the exclusive sum of the blocks completed in the pieces before each piece (less its value at the segment's first
    // piece: the piece's first block within its segment); and every segment's first marked piece, where the serial decode
    // of that interval dies or runs out of data
    u32 carry = 0, settled = 0, marked = np - 1;
    for (u32 p0 = 0; p0 < np; p0 += JP_PIECE_LANES) {
        const u32 p = p0 + (u32)t;
        const u32 v = p < np ? cnt[p] : 0u;
        const u32 inc = wg_scan_1024(s_scan, t, v);
        if (p < np) {
            cnt[p] = carry + inc - v;
            const JpegPieceState x = cur[p];
            settled += jpeg_piece_same(r0[p], x) ? 1u : 0u;
            if (x.w & (JP_PS_ENDED | JP_PS_DEAD)) {
                if (SEG) {
                    const u32 j = sof[p], i = p - poff[j];
                    if (i + 1 < poff[j + 1] - poff[j]) atomicMin(&lastp[j], i);
                } else if (p < marked) marked = p;
            }
        }
        carry += s_scan[JP_PIECE_LANES - 1];
        __syncthreads();
    }
    if (!SEG && marked < np - 1) atomicMin(&s_last, marked);
    __syncthreads();
    // the write pass
    int st = 0;
    u32 ndc = 0;
    if (SEG) {
        for (u32 p = t; p < np; p += JP_PIECE_LANES) {
            u32 j, i, n;
            const JpegSegment G = jpeg_piece_where<SEG>(D, scan, mpos, nfound, poff, sof, p, np, &j, &i, &n);
            if (i > __hip_atomic_load(&lastp[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) continue; // (atomicMin wrote it)
            const JpegPieceState first = {G.a, 0u};
            const u32 blk = G.first + (cnt[p] - cnt[poff[j]]);
            u32 c, mine = 0;
            jpeg_piece_run<true>(d, D, T, i ? cur[p - 1] : first, G, S, i, n, 64u * (G.blocks + 1u), &c, coef, blk, &st, &mine);
            if (mine) atomicMax(&ndcp[j], mine);
        }
    } else {
        const u32 last = s_last, write_steps = 64u * (scan.blocks + 1u);
        const JpegPieceState first = {scan.a, 0u};
        for (u32 i = t; i <= last; i += JP_PIECE_LANES) {
            u32 c, mine = 0;
            jpeg_piece_run<true>(d, D, T, i ? cur[i - 1] : first, scan, S, i, np, write_steps, &c, coef, cnt[i], &st, &mine);
            ndc = mine > ndc ? mine : ndc;
        }
    }
    if (st) atomicOr(&s_status, st);
    if (ndc) atomicMax(&s_ndc, ndc);
    if (settled) atomicAdd(&s_settled, settled);
    __syncthreads();
    // the DC pass: per component, the differences of the blocks whose DC symbol was decoded summed in scan order, mod 2^16;
    // with segments the sum starts from 0 at every segment and covers the blocks decoded in that segment only
    ndc = s_ndc;
    for (int c = 0; c < D.ncomp; c++) {
        const u32 n = jpeg_comp_blocks_in(D, c, SEG ? jpeg_scan_blocks(D) : ndc);
        const u32 per = (n + JP_PIECE_LANES - 1) / JP_PIECE_LANES;
        const u32 lo = (u32)t * per < n ? (u32)t * per : n;
        const u32 hi = n - lo < per ? n : lo + per;
        if (SEG) {
            // block q of the component lies in MCU q / cpm; a segment starts at the first block of an MCU that is a multiple of dri
            const u32 cpm = c == 0 && D.ncomp != 1 ? (u32)(D.hs * D.vs) : 1u;
            const u32 dri = D.dri ? (u32)D.dri : 0xFFFFFFFFu;
            u32 sum = 0, flag = 0;
            for (u32 q = lo; q < hi; q++) {
                const u32 m = q / cpm;
                if (q == m * cpm && m % dri == 0) {
                    sum = 0;
                    flag = 0x10000u;
                }
                sum += (u32)(uint16_t)coef[jpeg_scan_block_elem(D, jpeg_comp_block(D, c, q))];
            }
            wg_segscan_1024(s_scan, t, flag | (sum & 0xFFFFu));
            u32 pred = t ? s_scan[t - 1] & 0xFFFFu : 0u;
            for (u32 q = lo; q < hi; q++) {
                const u32 m = q / cpm;
                if (q == m * cpm && m % dri == 0) pred = 0;
                const u32 j = m / dri;
                if (j < nseg && q < jpeg_comp_blocks_in(D, c, __hip_atomic_load(&ndcp[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                    int16_t* o = coef + jpeg_scan_block_elem(D, jpeg_comp_block(D, c, q));
                    pred += (u32)(uint16_t)o[0];
                    o[0] = (int16_t)(uint16_t)pred;
                }
            }
        } else {
            u32 sum = 0;
            for (u32 q = lo; q < hi; q++) sum += (u32)(uint16_t)coef[jpeg_scan_block_elem(D, jpeg_comp_block(D, c, q))];
            u32 pred = wg_scan_1024(s_scan, t, sum) - sum;
            for (u32 q = lo; q < hi; q++) {
                int16_t* o = coef + jpeg_scan_block_elem(D, jpeg_comp_block(D, c, q));
                pred += (u32)(uint16_t)o[0];
                o[0] = (int16_t)(uint16_t)pred;
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        if (s_status) atomicOr(&B.status[f], s_status);
        u32* o = B.stats + 3 * (size_t)f;
        o[0] = np;
        o[1] = rounds;
        o[2] = s_settled;
    }
}

__global__ __launch_bounds__(64) void k_jpeg_idct(JpegBatch B)
{
    const int f = blockIdx.y;
    const JpegDesc& D = B.descs[f];
    const u32 blk = blockIdx.x * 64u + threadIdx.x;
    if (blk >= D.plane_total / 64u) return;
    const u32 e = blk * 64u;
    const int c = (D.ncomp == 3 && e >= D.poff[2]) ? 2 : (D.ncomp == 3 && e >= D.poff[1]) ? 1 : 0;
    const u32 local = blk - D.poff[c] / 64u;
    const int bw = D.bw[c];
    const int by = (int)(local / (u32)bw), bx = (int)(local - (u32)by * (u32)bw);
    // 64 int16 = eight 16-byte loads (the buffer and every block in it are 128-byte aligned)
    const uint4* src = reinterpret_cast<const uint4*>(B.coef + (size_t)f * B.coef_stride + e);
    int16_t cf[64];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint4 v = src[i];
        const u32 w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            cf[i * 8 + j * 2] = (int16_t)(w4[j] & 0xFFFFu);
            cf[i * 8 + j * 2 + 1] = (int16_t)(w4[j] >> 16);
        }
    }
    int32_t ws[64];
    jpeg_idct_block(cf, B.tables[D.table_set].q[D.tq[c]], ws);
    const int ps = bw * 8;
    u8* o = B.planes + (size_t)f * B.plane_stride + D.poff[c] + (size_t)by * 8 * ps + bx * 8;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        uint2 v;
        v.x = (u32)ws[r * 8] | (u32)ws[r * 8 + 1] << 8 | (u32)ws[r * 8 + 2] << 16 | (u32)ws[r * 8 + 3] << 24;
        v.y = (u32)ws[r * 8 + 4] | (u32)ws[r * 8 + 5] << 8 | (u32)ws[r * 8 + 6] << 16 | (u32)ws[r * 8 + 7] << 24;
        *reinterpret_cast<uint2*>(o + (size_t)r * ps) = v;
    }
}

__global__ __launch_bounds__(256) void k_jpeg_color(JpegBatch B)
{
    const int f = blockIdx.z;
    const JpegDesc& D = B.descs[f];
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= D.w || y >= D.h) return;
    u8 px[3];
    jpeg_pixel(D, B.planes + (size_t)f * B.plane_stride, x, y, px);
    u8* o = B.bgr + (size_t)f * B.bgr_frame_stride + (size_t)y * B.bgr_stride + (size_t)x * 3;
    o[0] = px[0];
    o[1] = px[1];
    o[2] = px[2];
}

int launch_jpeg_decode(cbv_ctx* ctx, const JpegBatch& B, u32 total_intervals, int any_dri, int any_pieces, u32 max_blocks, int max_w, int max_h)
{
    if (any_pieces && (!B.piece_bytes || (B.piece_bytes & 3u) || !B.pieces || !B.stats)) return cbv_fail(ctx, CBV_ERR_ARG, "launch_jpeg_decode: no piece scratch");
    if (B.segments && (!any_pieces || !B.segs)) return cbv_fail(ctx, CBV_ERR_ARG, "launch_jpeg_decode: no segment scratch");
    if (B.nframes <= 0 || B.nframes > 65535 || max_h > 65535 || total_intervals == 0 || (B.coef_stride & 63) || (B.plane_stride & 7))
        return cbv_fail(ctx, CBV_ERR_ARG, "launch_jpeg_decode: bad batch");
    hipStream_t s = ctx->stream;
    CBV_HIP(ctx, hipMemsetAsync(B.coef, 0, (size_t)B.nframes * B.coef_stride * sizeof(int16_t), s));
    CBV_HIP(ctx, hipMemsetAsync(B.status, 0, (size_t)B.nframes * sizeof(int), s));
    CBV_HIP(ctx, hipMemsetAsync(B.nfound, 0, (size_t)B.nframes * sizeof(int), s));
    CBV_HIP(ctx, hipMemsetAsync(B.stats, 0, (size_t)B.nframes * 3 * sizeof(u32), s));
    if (any_dri) hipLaunchKernelGGL(k_jpeg_restarts, dim3(B.nframes), dim3(256), 0, s, B);
    if (B.segments) { // every frame goes the piece path
        CBV_HIP(ctx, hipMemsetAsync(B.segs, 0, (size_t)B.nframes * B.seg_stride * sizeof(u32), s));
        hipLaunchKernelGGL(k_jpeg_pieces<true>, dim3(B.nframes), dim3(JP_PIECE_LANES), 0, s, B);
    } else if (any_pieces) hipLaunchKernelGGL(k_jpeg_pieces<false>, dim3(B.nframes), dim3(JP_PIECE_LANES), 0, s, B);
    if (!B.segments && (any_dri || !any_pieces)) hipLaunchKernelGGL(k_jpeg_entropy, dim3((total_intervals + 63u) / 64u), dim3(64), 0, s, B);
    hipLaunchKernelGGL(k_jpeg_idct, dim3((max_blocks + 63u) / 64u, B.nframes), dim3(64), 0, s, B);
    if (B.bgr) hipLaunchKernelGGL(k_jpeg_color, dim3((max_w + 255) / 256, max_h, B.nframes), dim3(256), 0, s, B);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

int launch_jpeg_color(cbv_ctx* ctx, const JpegBatch& B, int max_w, int max_h)
{
    if (B.nframes <= 0 || B.nframes > 65535 || max_w < 1 || max_h < 1 || max_h > 65535 || !B.bgr || !B.planes || !B.descs)
        return cbv_fail(ctx, CBV_ERR_ARG, "launch_jpeg_color: bad batch");
    hipLaunchKernelGGL(k_jpeg_color, dim3((max_w + 255) / 256, max_h, B.nframes), dim3(256), 0, ctx->stream, B);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}
