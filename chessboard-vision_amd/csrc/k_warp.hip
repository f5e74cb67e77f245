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
// same blend (warp_blend).  A tap outside the frame is BGR (0, 0, 0) for every source, not the conversion of zero.  The
// sources: WarpBgr (BGR frames through cv2.normalize's byte map), WarpProfile (BGR frames through apply_color_profile) and
// WarpRaw<FMT> (camera-native YUV frames and Bayer mosaics: the BGR frame k_ingest would write is never made).  The raw
// sources that carry a colour profile (WarpRawProfile<FMT>) have their kernels in k_warp_raw_profile.hip, and YUV frames in
// a colour space other than 0 (WarpSrc::cs) theirs in k_warp_cs.hip.
// Also here: the synthetic frame generator used by bench/tests.
#include "warp_gather.h"


template <int FPT, bool CALC>
__global__ __launch_bounds__(256) void k_warp(const u8* __restrict__ src, Geom g, WarpM M, int dw, int dh, int bw0,
                                               int bh0, int rot180, u8* __restrict__ dst, int dst_stride,
                                               size_t dst_frame_stride, const u8* __restrict__ norm_lut, const u32* __restrict__ minmax,
                                               size_t mm_stride, u32* __restrict__ zero_word, u32* __restrict__ zero_word2, int batch)
{
    (void)bh0;
    warp_gather<WarpBgr<CALC>, FPT>(WarpBgr<CALC>{src, g, norm_lut, minmax, mm_stride}, WarpDst{M.m, dw, dh, bw0, rot180, dst, dst_stride, dst_frame_stride},
                                    zero_word, zero_word2, batch, blockIdx.z);
}

template <int FPT, bool CALC>
__global__ __launch_bounds__(256) void k_warp_mb(const u8* __restrict__ src, Geom g, const BoardDev* __restrict__ tab, int nz, int s0,
                                                  const u8* __restrict__ norm_lut, const u32* __restrict__ minmax, size_t mm_stride,
                                                  u32* __restrict__ zero_word, u32* __restrict__ zero_word2, int batch)
{
    const int b = blockIdx.z / nz;
    const BoardDev& T = tab[b];
    if (b > 0 && ((int)blockIdx.x * 64 >= T.S || (int)blockIdx.y * 4 >= T.S)) return;
    warp_gather<WarpBgr<CALC>, FPT>(WarpBgr<CALC>{src, g, norm_lut, minmax, mm_stride}, warp_board_dst(T, s0), zero_word, zero_word2, batch,
                                    blockIdx.z - b * nz);
}

template <int FMT, int FPT>
__global__ __launch_bounds__(256) void k_warp_yuv(const u8* __restrict__ p0, const u8* __restrict__ p1, const u8* __restrict__ p2, RawGeom r, int sw, int sh, WarpM M,
                                                   int dw, int dh, int bw0, int rot180, u8* __restrict__ dst, int dst_stride,
                                                   size_t dst_frame_stride, u32* __restrict__ zero_word, u32* __restrict__ zero_word2, int batch)
{
    warp_gather<WarpRaw<FMT>, FPT>(WarpRaw<FMT>{p0, p1, p2, r, sw, sh}, WarpDst{M.m, dw, dh, bw0, rot180, dst, dst_stride, dst_frame_stride}, zero_word,
                                   zero_word2, batch, blockIdx.z);
}

template <int FMT, int FPT>
__global__ __launch_bounds__(256) void k_warp_yuv_mb(const u8* __restrict__ p0, const u8* __restrict__ p1, const u8* __restrict__ p2, RawGeom r, int sw, int sh,
                                                      const BoardDev* __restrict__ tab, int nz, int s0, u32* __restrict__ zero_word,
                                                      u32* __restrict__ zero_word2, int batch)
{
    const int b = blockIdx.z / nz;
    const BoardDev& T = tab[b];
    if (b > 0 && ((int)blockIdx.x * 64 >= T.S || (int)blockIdx.y * 4 >= T.S)) return;
    warp_gather<WarpRaw<FMT>, FPT>(WarpRaw<FMT>{p0, p1, p2, r, sw, sh}, warp_board_dst(T, s0), zero_word, zero_word2, batch, blockIdx.z - b * nz);
}

template <int FMT, int FPT>
__global__ __launch_bounds__(256) void k_warp_bayer(const u8* __restrict__ p0, RawGeom r, int sw, int sh, WarpM M, int dw, int dh, int bw0, int rot180,
                                                     u8* __restrict__ dst, int dst_stride, size_t dst_frame_stride, u32* __restrict__ zero_word,
                                                     u32* __restrict__ zero_word2, int batch)
{
    warp_gather<WarpRaw<FMT>, FPT>(WarpRaw<FMT>{p0, nullptr, nullptr, r, sw, sh}, WarpDst{M.m, dw, dh, bw0, rot180, dst, dst_stride, dst_frame_stride},
                                   zero_word, zero_word2, batch, blockIdx.z);
}

template <int FMT, int FPT>
__global__ __launch_bounds__(256) void k_warp_bayer_mb(const u8* __restrict__ p0, RawGeom r, int sw, int sh, const BoardDev* __restrict__ tab, int nz,
                                                        int s0, u32* __restrict__ zero_word, u32* __restrict__ zero_word2, int batch)
{
    const int b = blockIdx.z / nz;
    const BoardDev& T = tab[b];
    if (b > 0 && ((int)blockIdx.x * 64 >= T.S || (int)blockIdx.y * 4 >= T.S)) return;
    warp_gather<WarpRaw<FMT>, FPT>(WarpRaw<FMT>{p0, nullptr, nullptr, r, sw, sh}, warp_board_dst(T, s0), zero_word, zero_word2, batch,
                                   blockIdx.z - b * nz);
}

// blockIdx.z = profile * nz + group of frames; profile p writes its frames dst_profile_stride bytes behind profile p - 1's
template <int FPT>
__global__ __launch_bounds__(256) void k_warp_profile(const u8* __restrict__ src, Geom g, WarpM M, int dw, int dh, int bw0, int rot180,
                                                       u8* __restrict__ dst, int dst_stride, size_t dst_frame_stride, size_t dst_profile_stride,
                                                       const StaticTabs* __restrict__ st, const ProfileTabs* __restrict__ ptabs, int nz,
                                                       u32* __restrict__ zero_word, u32* __restrict__ zero_word2, int batch)
{
    const int pi = blockIdx.z / nz;
    warp_gather<WarpProfile, FPT>(WarpProfile{src, g, st, ptabs + pi},
                                  WarpDst{M.m, dw, dh, bw0, rot180, dst + (size_t)pi * dst_profile_stride, dst_stride, dst_frame_stride}, zero_word,
                                  zero_word2, batch, blockIdx.z - pi * nz);
}

// the profile is the board's: a workgroup stages its board's table
template <int FPT>
__global__ __launch_bounds__(256) void k_warp_profile_mb(const u8* __restrict__ src, Geom g, const BoardDev* __restrict__ tab, int nz, int s0,
                                                          const StaticTabs* __restrict__ st, u32* __restrict__ zero_word,
                                                          u32* __restrict__ zero_word2, int batch)
{
    const int b = blockIdx.z / nz;
    const BoardDev& T = tab[b];
    if (b > 0 && ((int)blockIdx.x * 64 >= T.S || (int)blockIdx.y * WP_ROWS >= T.S)) return;
    warp_gather<WarpProfile, FPT>(WarpProfile{src, g, st, T.ptabs}, warp_board_dst(T, s0), zero_word, zero_word2, batch, blockIdx.z - b * nz);
}


int launch_warp(cbv_ctx* ctx, WarpSrc s, const double* Minv9, int dw, int dh, int rot180, u8* dst, int dst_stride, size_t dst_frame_stride,
                int batch, u32* zero_word, u32* zero_word2)
{
    if (s.cs) return launch_warp_cs(ctx, s, Minv9, dw, dh, rot180, dst, dst_stride, dst_frame_stride, batch, zero_word, zero_word2);
    if (s.kind == WarpSrc::JPEG) return launch_warp_jpeg(ctx, s, Minv9, dw, dh, rot180, dst, dst_stride, dst_frame_stride, batch, zero_word, zero_word2);
    if (s.raw() && s.ptabs) return launch_warp_raw_profile(ctx, s, Minv9, dw, dh, rot180, dst, dst_stride, dst_frame_stride, batch, zero_word, zero_word2);
    WarpM M;
    for (int i = 0; i < 9; i++) M.m[i] = Minv9[i];
    int bw0, bh0;
    warp_block_shape(dw, dh, &bw0, &bh0);
    const bool profile = s.kind == WarpSrc::PROFILE;
    if (profile && (s.np <= 0 || batch <= 0 || (long long)s.np * warp_groups(batch) > 65535))
        return cbv_fail(ctx, CBV_ERR_ARG, "launch_warp_profile: %d profiles x %d frames do not fit a launch", s.np, batch);
    const hipStream_t st = ctx->stream;
    return warp_launch(ctx, &s, dw, dh, profile ? s.np : 1, batch, [&](auto fmt, auto fpt, dim3 grid, int nz) {
        constexpr int FMT = decltype(fmt)::value, FPT = decltype(fpt)::value;
        if constexpr (FMT == CBV_FMT_BGR) {
            if (profile)
                hipLaunchKernelGGL((k_warp_profile<FPT>), grid, dim3(256), 0, st, s.bgr, s.g, M, dw, dh, bw0, rot180, dst, dst_stride, dst_frame_stride,
                                   s.dst_profile_stride, ctx->tabs, s.ptabs, nz, zero_word, zero_word2, batch);
            else if (s.norm.minmax)
                hipLaunchKernelGGL((k_warp<FPT, true>), grid, dim3(256), 0, st, s.bgr, s.g, M, dw, dh, bw0, bh0, rot180, dst, dst_stride,
                                   dst_frame_stride, nullptr, s.norm.minmax, s.norm.mm_stride, zero_word, zero_word2, batch);
            else
                hipLaunchKernelGGL((k_warp<FPT, false>), grid, dim3(256), 0, st, s.bgr, s.g, M, dw, dh, bw0, bh0, rot180, dst, dst_stride,
                                   dst_frame_stride, s.norm.lut, nullptr, 0, zero_word, zero_word2, batch);
        } else if constexpr (raw_fmt_bayer(FMT))
            hipLaunchKernelGGL((k_warp_bayer<FMT, FPT>), grid, dim3(256), 0, st, s.planes.p[0], s.r, s.g.w, s.g.h, M, dw, dh, bw0, rot180, dst,
                               dst_stride, dst_frame_stride, zero_word, zero_word2, batch);
        else
            hipLaunchKernelGGL((k_warp_yuv<FMT, FPT>), grid, dim3(256), 0, st, s.planes.p[0], s.planes.p[1], s.planes.p[2], s.r, s.g.w, s.g.h, M, dw,
                               dh, bw0, rot180, dst, dst_stride, dst_frame_stride, zero_word, zero_word2, batch);
    });
}

int launch_warp_mb(cbv_ctx* ctx, WarpSrc s, const BoardDev* tab, int nb, int maxS, int s0, int batch, u32* zero_word, u32* zero_word2)
{
    if (s.cs) return launch_warp_cs_mb(ctx, s, tab, nb, maxS, s0, batch, zero_word, zero_word2);
    if (s.kind == WarpSrc::JPEG) return launch_warp_jpeg_mb(ctx, s, tab, nb, maxS, s0, batch, zero_word, zero_word2);
    if (s.raw() && s.ptabs) return launch_warp_raw_profile_mb(ctx, s, tab, nb, maxS, s0, batch, zero_word, zero_word2);
    const hipStream_t st = ctx->stream;
    return warp_launch(ctx, &s, maxS, maxS, nb, batch, [&](auto fmt, auto fpt, dim3 grid, int nz) {
        constexpr int FMT = decltype(fmt)::value, FPT = decltype(fpt)::value;
        if constexpr (FMT == CBV_FMT_BGR) {
            if (s.kind == WarpSrc::PROFILE)
                hipLaunchKernelGGL((k_warp_profile_mb<FPT>), grid, dim3(256), 0, st, s.bgr, s.g, tab, nz, s0, ctx->tabs, zero_word, zero_word2, batch);
            else if (s.norm.minmax)
                hipLaunchKernelGGL((k_warp_mb<FPT, true>), grid, dim3(256), 0, st, s.bgr, s.g, tab, nz, s0, nullptr, s.norm.minmax, s.norm.mm_stride,
                                   zero_word, zero_word2, batch);
            else
                hipLaunchKernelGGL((k_warp_mb<FPT, false>), grid, dim3(256), 0, st, s.bgr, s.g, tab, nz, s0, s.norm.lut, nullptr, 0, zero_word,
                                   zero_word2, batch);
        } else if constexpr (raw_fmt_bayer(FMT))
            hipLaunchKernelGGL((k_warp_bayer_mb<FMT, FPT>), grid, dim3(256), 0, st, s.planes.p[0], s.r, s.g.w, s.g.h, tab, nz, s0, zero_word, zero_word2,
                               batch);
        else
            hipLaunchKernelGGL((k_warp_yuv_mb<FMT, FPT>), grid, dim3(256), 0, st, s.planes.p[0], s.planes.p[1], s.planes.p[2], s.r, s.g.w, s.g.h, tab, nz,
                               s0, zero_word, zero_word2, batch);
    });
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
