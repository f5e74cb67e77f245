// Piece colour per square (include/cbv.h, "piece colour per square").
//
// k_piece_tone: the tone sums of a square, one workgroup of four waves per (square, frame[, board]).  The disc of
// _detect_center_vs_border has radius r = min(w, h) / 4 around (w / 2, h / 2), so only the rows cy - r .. cy + r and the
// columns cx - r .. cx + r of the square can hold a pixel of it (39 x 39 of a 77 x 77 square).  The 3 * (2 r + 1) bytes of
// each of those rows are read as ALIGNED 32-bit words, whatever the row's own alignment: the words of all rows of the box
// are one list (30 words a row for a 77 x 77 square, 1170 in all), dealt to the 256 lanes five at a time, independent of
// one another, so their latencies overlap; a byte-per-lane form with a wave per row measured 1.66 us per 1080p frame and
// board against the warp's 2.75.  A byte of a word counts when it lies in the row's part of the box and its pixel in the
// disc, into the sum of its channel (byte index mod 3).  The sums are exact in u32 (at most 65 * 65 pixels of 255); they
// are reduced across the wave with shuffles and across the four waves through 48 bytes of LDS, and the record is written
// by one lane as one 16-byte store.  No atomics, no scratch, no dynamic LDS.
// Bounds: the box lies inside the square (cy + r <= h / 2 + h / 4 < h, and so in x) and the square inside its board (the
// callers check the ROIs).  A word is read only when it holds at least one byte of the box, so it lies inside every
// allocation that starts and ends on a multiple of four bytes, which the board buffers do (hipMalloc; sizes rounded to 256).
//
// k_piece_tone_classify: the frame's cbv_tone_result from its 64 sums, one wave per (frame, board): lane i classifies
// ROI i (tone_core.h, the host's very code) and two ballots are the two words.  A launch of its own behind the sums:
// the record of a frame needs the sums of its 64 workgroups, and the alternative inside one launch is an arrival counter
// per frame (a global atomic, a fence and a word to zero per launch) to save a launch of `frames` single waves.
#include "cbv_internal.h"
#include "cbv_device.h"
#include "tone_core.h"

namespace {

constexpr int TONE_NT = 256;

__device__ __forceinline__ void tone_square_body(const u8* __restrict__ frame, const SquareDesc& d, cbv_tone_sums* __restrict__ out, u32 (*part)[3])
{
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int cx = d.w / 2, cy = d.h / 2, r = min(d.w, d.h) / 4, r2 = r * r;
    const int row_bytes = 3 * (2 * r + 1);
    const u8* box = frame + d.src_off + (size_t)(cy - r) * d.stride + 3 * (cx - r);
    // words that cover a row at any alignment: up to 3 bytes in front of it; 50 at most (r = 32)
    const int wpr = (row_bytes + 3 + 3) / 4, items = (2 * r + 1) * wpr;
    const float inv = 1.0f / (float)wpr; // (idx + 0.5) * inv truncates to idx / wpr exactly: idx < 65 * 50, far inside float's 24 bits
    u32 s0 = 0, s1 = 0, s2 = 0;
#pragma unroll 5
    for (int idx = threadIdx.x; idx < items; idx += TONE_NT) {
        const int y = (int)(((float)idx + 0.5f) * inv), wi = idx - y * wpr;
        const u8* row = box + (size_t)y * d.stride;
        const int off = (int)((size_t)row & 3u);
        const int j0 = 4 * wi - off; // index in the row of the word's first byte: -3 .. row_bytes + 2
        const u32 v = j0 < row_bytes ? *(const u32*)(row + j0) : 0u; // (a word past the row's last byte is not read)
        const int dy = y - r, rem = r2 - dy * dy; // a pixel of this row is in the disc iff dx^2 <= rem
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int j = j0 + k, px = (j + 3) / 3 - 1, c = j - 3 * px, dx = px - r; // (j + 3 >= 0: the division is unsigned-safe)
            const u32 byte = (v >> (8 * k)) & 255u;
            const u32 t = (j >= 0 && j < row_bytes && dx * dx <= rem) ? byte : 0u;
            s0 += c == 0 ? t : 0u;
            s1 += c == 1 ? t : 0u;
            s2 += c == 2 ? t : 0u;
        }
    }
    s0 = wave_sum_u32(s0);
    s1 = wave_sum_u32(s1);
    s2 = wave_sum_u32(s2);
    if (lane == 0) {
        part[wave][0] = s0;
        part[wave][1] = s1;
        part[wave][2] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint4 rec;
        rec.x = part[0][0] + part[1][0] + part[2][0] + part[3][0];
        rec.y = part[0][1] + part[1][1] + part[2][1] + part[3][1];
        rec.z = part[0][2] + part[1][2] + part[2][2] + part[3][2];
        rec.w = d.cnt[0];
        *(uint4*)out = rec; // (records are 16 bytes in a 16-byte aligned array)
    }
}

// explicit arguments: grid (n, frames); out[frame][CBV_MAX_SQUARES]
__global__ __launch_bounds__(TONE_NT) void k_piece_tone(const u8* __restrict__ src, size_t src_frame_stride, const SquareDesc* __restrict__ descs,
                                                        cbv_tone_sums* __restrict__ out)
{
    __shared__ u32 part[TONE_NT / WAVE][3];
    const size_t f = blockIdx.y;
    tone_square_body(src + f * src_frame_stride, descs[blockIdx.x], out + f * CBV_MAX_SQUARES + blockIdx.x, part);
}

// every board of a pipeline in one launch: grid (CBV_MAX_SQUARES, boards, frames); a board with tones off leaves at once
__global__ __launch_bounds__(TONE_NT) void k_piece_tone_boards(const BoardDev* __restrict__ tab, int s0)
{
    __shared__ u32 part[TONE_NT / WAVE][3];
    const BoardDev& T = tab[blockIdx.y];
    if (!T.tone_sums || (int)blockIdx.x >= T.n) return;
    const size_t s = (size_t)s0 + blockIdx.z;
    tone_square_body(T.warped + s * T.warped_stride, T.descs[blockIdx.x], T.tone_sums + s * CBV_MAX_SQUARES + blockIdx.x, part);
}

// grid (frames, boards), one wave: the records of the frames whose sums the launch in front of this one wrote
__global__ __launch_bounds__(WAVE) void k_piece_tone_classify(const BoardDev* __restrict__ tab, int s0)
{
    const BoardDev& T = tab[blockIdx.y];
    if (!T.tone_sums) return;
    const size_t s = (size_t)s0 + blockIdx.x;
    const int lane = threadIdx.x;
    const cbv_tone_sums sums = T.tone_sums[s * CBV_MAX_SQUARES + lane];
    const int tone = lane < T.n ? tone_classify(T.tone_model, lane, &sums) : TONE_UNDECIDED;
    const u64 white = __ballot(tone == TONE_WHITE), black = __ballot(tone == TONE_BLACK);
    if (lane == 0) {
        cbv_tone_result rec;
        rec.white = white;
        rec.black = black;
        T.tone_res[s] = rec;
    }
}

} // namespace

int launch_piece_tone(cbv_ctx* ctx, const u8* src, size_t src_frame_stride, const SquareDesc* descs, int n, cbv_tone_sums* out, int batch)
{
    prof_begin(ctx, CBV_K_TONE);
    hipLaunchKernelGGL(k_piece_tone, dim3(n, batch), dim3(TONE_NT), 0, ctx->stream, src, src_frame_stride, descs, out);
    prof_end(ctx, CBV_K_TONE);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

int launch_piece_tone_boards(cbv_ctx* ctx, const BoardDev* tab, int nb, int s0, int batch)
{
    prof_begin(ctx, CBV_K_TONE);
    hipLaunchKernelGGL(k_piece_tone_boards, dim3(CBV_MAX_SQUARES, nb, batch), dim3(TONE_NT), 0, ctx->stream, tab, s0);
    hipLaunchKernelGGL(k_piece_tone_classify, dim3(batch, nb), dim3(WAVE), 0, ctx->stream, tab, s0);
    prof_end(ctx, CBV_K_TONE);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}
