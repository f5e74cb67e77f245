// Baseline JPEG decode (include/cbv.h, CBV_FMT_MJPEG): the bodies are jpeg_core.h's, the same the host twin runs.
//   k_jpeg_restarts  a workgroup per frame with DRI: the positions of FF D0..D7 in the entropy data, in order
//   k_jpeg_entropy   a lane per restart interval, (frame, interval) pairs flattened: int16 coefficients, natural order
//   k_jpeg_pieces    a workgroup per frame without DRI (B.piece_bytes > 0): the scan cut into pieces, a lane per piece
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
    if (B.piece_bytes && !D.dri) return; // k_jpeg_pieces' frame
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

// The piece path (jpeg_core.h): lane t takes pieces t, t + 1024, ...  Rounds in Jacobi order, the exits double-buffered in
// the frame's scratch; a round is over at the barrier, so no lane waits for anything but its own workgroup.  Every loop's
// bound is known at launch: pieces / 1024 per pass, at most `pieces` rounds, jpeg_piece_run's step counts.
__global__ __launch_bounds__(JP_PIECE_LANES) void k_jpeg_pieces(JpegBatch B)
{
    const int f = blockIdx.x, t = threadIdx.x;
    const JpegDesc& D = B.descs[f];
    if (D.dri) return; // (the same in every lane)
    const u8* d = B.data + (size_t)f * B.data_stride;
    const JpegTables& T = B.tables[D.table_set];
    const u32 S = B.piece_bytes, np = jpeg_piece_count(D, S), total = jpeg_scan_blocks(D);
    const u32 round_steps = 8u * S + 8u, write_steps = 64u * (total + 1u);
    u32* base = B.pieces + (size_t)f * B.piece_stride;
    JpegPieceState* cur = reinterpret_cast<JpegPieceState*>(base);
    JpegPieceState* nxt = cur + np;
    JpegPieceState* ent = nxt + np;
    JpegPieceState* r0 = ent + np;
    u32* cnt = base + 8 * (size_t)np;
    int16_t* coef = B.coef + (size_t)f * B.coef_stride;
    __shared__ u32 s_scan[JP_PIECE_LANES];
    __shared__ u32 s_changed, s_ndc, s_settled, s_last;
    __shared__ int s_status;
    const JpegPieceState first = {D.ent_off, 0u};
    if (t == 0) {
        s_changed = 0;
        s_ndc = 0;
        s_settled = 0;
        s_status = 0;
        s_last = np - 1;
    }
    for (u32 i = t; i < np; i += JP_PIECE_LANES) { // round 0
        const JpegPieceState e = i ? jpeg_piece_guess(d, D, S, i, np) : first;
        u32 c;
        const JpegPieceState x = jpeg_piece_run<false>(d, D, T, e, S, i, np, round_steps, &c, nullptr, 0u, nullptr, nullptr);
        ent[i] = e;
        cur[i] = x;
        r0[i] = x;
        cnt[i] = c;
    }
    __syncthreads();
    u32 rounds = 1;
    for (u32 r = 1; r < np; r++) {
        bool mine = false;
        for (u32 i = t; i < np; i += JP_PIECE_LANES) {
            const JpegPieceState e = i ? cur[i - 1] : first;
            const JpegPieceState was = cur[i];
            if (jpeg_piece_same(e, ent[i])) {
                nxt[i] = was;
                continue;
            }
            u32 c;
            const JpegPieceState x = jpeg_piece_run<false>(d, D, T, e, S, i, np, round_steps, &c, nullptr, 0u, nullptr, nullptr);
            ent[i] = e;
            nxt[i] = x;
            cnt[i] = c;
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
    // every piece's first block: the exclusive sum of the blocks completed in the pieces before it; and the first marked
    // piece, where the serial decode dies or runs out of data
    u32 carry = 0, settled = 0, marked = np - 1;
    for (u32 i0 = 0; i0 < np; i0 += JP_PIECE_LANES) {
        const u32 i = i0 + (u32)t;
        const u32 v = i < np ? cnt[i] : 0u;
        const u32 inc = wg_scan_1024(s_scan, t, v);
        if (i < np) {
            cnt[i] = carry + inc - v;
            const JpegPieceState x = cur[i];
            settled += jpeg_piece_same(r0[i], x) ? 1u : 0u;
            if ((x.w & (JP_PS_ENDED | JP_PS_DEAD)) && i < marked) marked = i;
        }
        carry += s_scan[JP_PIECE_LANES - 1];
        __syncthreads();
    }
    if (marked < np - 1) atomicMin(&s_last, marked);
    __syncthreads();
    // the write pass
    const u32 last = s_last;
    int st = 0;
    u32 ndc = 0;
    for (u32 i = t; i <= last; i += JP_PIECE_LANES) {
        u32 c, mine = 0;
        jpeg_piece_run<true>(d, D, T, i ? cur[i - 1] : first, S, i, np, write_steps, &c, coef, cnt[i], &st, &mine);
        ndc = mine > ndc ? mine : ndc;
    }
    if (st) atomicOr(&s_status, st);
    if (ndc) atomicMax(&s_ndc, ndc);
    if (settled) atomicAdd(&s_settled, settled);
    __syncthreads();
    // the DC pass: per component, the differences of the blocks whose DC symbol was decoded summed in scan order, mod 2^16
    ndc = s_ndc;
    for (int c = 0; c < D.ncomp; c++) {
        const u32 n = jpeg_comp_blocks_in(D, c, ndc);
        const u32 per = (n + JP_PIECE_LANES - 1) / JP_PIECE_LANES;
        const u32 lo = (u32)t * per < n ? (u32)t * per : n;
        const u32 hi = n - lo < per ? n : lo + per;
        u32 sum = 0;
        for (u32 j = lo; j < hi; j++) sum += (u32)(uint16_t)coef[jpeg_scan_block_elem(D, jpeg_comp_block(D, c, j))];
        u32 pred = wg_scan_1024(s_scan, t, sum) - sum;
        for (u32 j = lo; j < hi; j++) {
            int16_t* o = coef + jpeg_scan_block_elem(D, jpeg_comp_block(D, c, j));
            pred += (u32)(uint16_t)o[0];
            o[0] = (int16_t)(uint16_t)pred;
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
    if (B.nframes <= 0 || B.nframes > 65535 || max_h > 65535 || total_intervals == 0 || (B.coef_stride & 63) || (B.plane_stride & 7))
        return cbv_fail(ctx, CBV_ERR_ARG, "launch_jpeg_decode: bad batch");
    hipStream_t s = ctx->stream;
    CBV_HIP(ctx, hipMemsetAsync(B.coef, 0, (size_t)B.nframes * B.coef_stride * sizeof(int16_t), s));
    CBV_HIP(ctx, hipMemsetAsync(B.status, 0, (size_t)B.nframes * sizeof(int), s));
    CBV_HIP(ctx, hipMemsetAsync(B.nfound, 0, (size_t)B.nframes * sizeof(int), s));
    CBV_HIP(ctx, hipMemsetAsync(B.stats, 0, (size_t)B.nframes * 3 * sizeof(u32), s));
    if (any_dri) hipLaunchKernelGGL(k_jpeg_restarts, dim3(B.nframes), dim3(256), 0, s, B);
    if (any_pieces) hipLaunchKernelGGL(k_jpeg_pieces, dim3(B.nframes), dim3(JP_PIECE_LANES), 0, s, B);
    if (any_dri || !any_pieces) hipLaunchKernelGGL(k_jpeg_entropy, dim3((total_intervals + 63u) / 64u), dim3(64), 0, s, B);
    hipLaunchKernelGGL(k_jpeg_idct, dim3((max_blocks + 63u) / 64u, B.nframes), dim3(64), 0, s, B);
    hipLaunchKernelGGL(k_jpeg_color, dim3((max_w + 255) / 256, max_h, B.nframes), dim3(256), 0, s, B);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}
