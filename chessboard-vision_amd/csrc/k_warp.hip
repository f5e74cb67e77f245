// cv2.warpPerspective(img, M, (S,S)) INTER_LINEAR / BORDER_CONSTANT(0)
// (board_detection.py:70), optional cv2.rotate(ROTATE_180) (game_session.py:126)
// and — for the fused pipeline — cv2.normalize folded into the gather (a byte
// map commutes with sampling: the four taps are mapped before interpolation).
//
// Coordinates follow WarpPerspectiveInvoker exactly: the destination is cut
// into 64 x 16 blocks (BLOCK_SZ = 32), X0/Y0/W0 are evaluated at the block's
// left edge and advanced by M*x1 inside the block, in double, one rounding per
// operation; coordinates are quantised to 1/32 px and sampled with the 15-bit
// fixed-point bilinear table of remap().
//
// One gather (warp_gather, warp_gather.h) serves every kind of source frame.  What a tap is worth is a function of the source pixel alone
// for every kind (a byte map, a pointwise YUV conversion, the demosaic of a site, the colour profile), so converting the
// four taps and blending them is, bit for bit, sampling the converted frame: same coordinates (warp_taps), same conversion,
// same blend (warp_blend).  A tap outside the frame is BGR (0, 0, 0) for every source, not the conversion of zero.
// This unit holds k_warp_one and k_warp_boards (warp_gather.h) of WarpBgr (BGR frames through cv2.normalize's byte map, both
// forms), WarpProfile (BGR frames through apply_color_profile) and WarpRaw<FMT> (camera-native YUV frames and Bayer mosaics:
// the BGR frame k_ingest would write is never made), with one frame per thread and with four: 52 kernels.  launch_warp and
// launch_warp_mb hand the other sources to their units: the raw sources that carry a colour profile (WarpRawProfile<FMT>) to
// k_warp_raw_profile.hip, YUV frames in a colour space other than 0 (WarpSrc::cs) to k_warp_cs.hip, JPEG planes to
// k_warp_jpeg.hip, developed mosaics (WarpSrc::deep) to k_warp_deep.hip.
// Also here: the synthetic frame generator used by bench/tests.
#include "warp_gather.h"

int launch_warp(cbv_ctx* ctx, WarpSrc s, const double* Minv9, int dw, int dh, int rot180, u8* dst, int dst_stride, size_t dst_frame_stride,
                int batch, u32* zero_word, u32* zero_word2)
{
    if (s.cs) return launch_warp_cs(ctx, s, Minv9, dw, dh, rot180, dst, dst_stride, dst_frame_stride, batch, zero_word, zero_word2);
    if (s.deep()) return launch_warp_deep(ctx, s, Minv9, dw, dh, rot180, dst, dst_stride, dst_frame_stride, batch, zero_word, zero_word2);
    if (s.kind == WarpSrc::JPEG) return launch_warp_jpeg(ctx, s, Minv9, dw, dh, rot180, dst, dst_stride, dst_frame_stride, batch, zero_word, zero_word2);
    if (s.raw() && s.ptabs) return launch_warp_raw_profile(ctx, s, Minv9, dw, dh, rot180, dst, dst_stride, dst_frame_stride, batch, zero_word, zero_word2);
    const char* who = s.kind == WarpSrc::PROFILE ? "launch_warp_profile" : "launch_warp";
    const WarpOneTo to = {Minv9, dw, dh, rot180, dst, dst_stride, dst_frame_stride, s.np, s.dst_profile_stride};
    return warp_typed_plain(ctx, &s, batch, [&](auto S) { return warp_launch_one(ctx, who, S, to, batch, zero_word, zero_word2); });
}

int launch_warp_mb(cbv_ctx* ctx, WarpSrc s, const BoardDev* tab, int nb, int maxS, int s0, int batch, u32* zero_word, u32* zero_word2)
{
    if (s.cs) return launch_warp_cs_mb(ctx, s, tab, nb, maxS, s0, batch, zero_word, zero_word2);
    if (s.deep()) return launch_warp_deep_mb(ctx, s, tab, nb, maxS, s0, batch, zero_word, zero_word2);
    if (s.kind == WarpSrc::JPEG) return launch_warp_jpeg_mb(ctx, s, tab, nb, maxS, s0, batch, zero_word, zero_word2);
    if (s.raw() && s.ptabs) return launch_warp_raw_profile_mb(ctx, s, tab, nb, maxS, s0, batch, zero_word, zero_word2);
    return warp_typed_plain(ctx, &s, batch, [&](auto S) { return warp_launch_boards(ctx, "launch_warp_mb", S, tab, nb, maxS, s0, batch, zero_word, zero_word2); });
}

// ---------------------------------------------------------------------------
// synthetic frames; mirrors oracle orc_synth_frame bit for bit
// ---------------------------------------------------------------------------
__device__ __forceinline__ u64 d_mix64(u64 z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void k_synth(u8* __restrict__ dst, Geom g, const u64* __restrict__ seeds,
                                                const double* __restrict__ Hinv, const u8* __restrict__ boards,
                                                const cbv_scene* __restrict__ scp)
{
    __shared__ u8 board[64];
    __shared__ cbv_scene sc;
    if (threadIdx.x < 64) board[threadIdx.x] = boards[(size_t)blockIdx.z * 64 + threadIdx.x];
    if (threadIdx.x == 0) sc = *scp;
    __syncthreads();
    const u64 seed = seeds[blockIdx.z];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= g.w || y >= g.h) return;
    const u64 idx = (u64)y * (u64)g.w + (u64)x;
    const u64 hn = d_mix64(seed + idx * 0x9E3779B97F4A7C15ULL);
    const u64 hb = d_mix64(0x5851F42D4C957F2DULL + (u64)(y >> 4) * 4096 + (u64)(x >> 4));
    const int bgv = sc.bg_lo + (int)(hb % (u64)(sc.bg_span ? sc.bg_span : 1));
    int c0 = bgv, c1 = bgv, c2 = bgv;
    const double W = Hinv[6] * x + Hinv[7] * y + Hinv[8];
    const double u = (Hinv[0] * x + Hinv[1] * y + Hinv[2]) / W;
    const double v = (Hinv[3] * x + Hinv[4] * y + Hinv[5]) / W;
    if (u >= 0.0 && u < 8.0 && v >= 0.0 && v < 8.0) {
        const int fi = (int)u, ri = (int)v;
        const u8* c = ((fi + ri) & 1) ? sc.dark : sc.light;
        const int piece = board[ri * 8 + fi];
        if (piece) {
            const double du = u - (fi + 0.5), dv = v - (ri + 0.5);
            if (du * du + dv * dv <= sc.radius * sc.radius) c = piece == 1 ? sc.white : sc.black;
        }
        c0 = c[0];
        c1 = c[1];
        c2 = c[2];
    }
    const int span = 2 * sc.noise + 1;
    u8* q = dst + (size_t)blockIdx.z * g.frame_stride + (size_t)y * g.stride + (size_t)x * 3;
    q[0] = d_sat8(c0 + (int)((hn >> 0) & 0xFFFF) % span - sc.noise);
    q[1] = d_sat8(c1 + (int)((hn >> 16) & 0xFFFF) % span - sc.noise);
    q[2] = d_sat8(c2 + (int)((hn >> 32) & 0xFFFF) % span - sc.noise);
}

int launch_synth(cbv_ctx* ctx, u8* dst, Geom g, const u64* seeds_dev, const double* hinv_dev, const u8* boards_dev,
                 const cbv_scene* scene_dev, int batch)
{
    dim3 grid((g.w + 63) / 64, (g.h + 3) / 4, batch);
    prof_begin(ctx, CBV_K_SYNTH);
    hipLaunchKernelGGL(k_synth, grid, dim3(256), 0, ctx->stream, dst, g, seeds_dev, hinv_dev, boards_dev, scene_dev);
    prof_end(ctx, CBV_K_SYNTH);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}
