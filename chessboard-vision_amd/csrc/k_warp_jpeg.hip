// The warp of Motion-JPEG frames from their decoded planes: warp(k_jpeg_color(planes)), and with a colour profile
// warp(apply_color_profile(k_jpeg_color(planes))), bit for bit, with no BGR frame ever written (pipelines in planes mode
// without enhancement, their colour sweep, cbv_warp_jpeg).  The gather is warp_gather (warp_gather.h) with the sources
// WarpJpeg and WarpJpegProfile: coordinates, rot180 and the zeroed words are the gather's own; a tap at (x, y) is
// jpeg_pixel(D, planes, x, y) with the frame's own descriptor D, so gray, 4:4:4, 4:2:2 and 4:2:0 frames share a launch.
// Every address comes from the descriptor, which the host parser has validated, and from the pixel's coordinates; none
// depends on a sample, so a damaged stream changes values and nothing else.  A tap outside the frame is BGR 0.  The kernels
// live in a file of their own: the counts of k_warp.hip and k_warp_raw_profile.hip stay what they are.
#include "warp_gather.h"

// Frames per thread of the many-frames forms (batch >= 8).  The plain kernels take four, as every plain source does (44
// VGPRs at one frame, 83 at four); with the profile's registers on top the kernels take two (70 VGPRs at one frame, 93 at
// two), as the planar 4:2:0 family of k_warp_raw_profile.hip does, whose loads these resemble.  The forms were not timed
// against each other; tests/test_warp_jpeg_resources.py pins the counts.
enum { JPEG_FPT = 4, JPEG_PROFILE_FPT = 2 };

template <int FPT>
__global__ __launch_bounds__(256) void k_warp_jpeg(const u8* __restrict__ planes, size_t plane_stride, const JpegDesc* __restrict__ descs, int sw, int sh,
                                                    WarpM M, int dw, int dh, int bw0, int rot180, u8* __restrict__ dst, int dst_stride,
                                                    size_t dst_frame_stride, u32* __restrict__ zero_word, u32* __restrict__ zero_word2, int batch)
{
    warp_gather<WarpJpeg, FPT>(WarpJpeg{planes, plane_stride, descs, sw, sh}, WarpDst{M.m, dw, dh, bw0, rot180, dst, dst_stride, dst_frame_stride},
                               zero_word, zero_word2, batch, blockIdx.z);
}

// every board of a pipeline in one launch: blockIdx.z = board * nz + group of frames
template <int FPT>
__global__ __launch_bounds__(256) void k_warp_jpeg_mb(const u8* __restrict__ planes, size_t plane_stride, const JpegDesc* __restrict__ descs, int sw,
                                                       int sh, const BoardDev* __restrict__ tab, int nz, int s0, u32* __restrict__ zero_word,
                                                       u32* __restrict__ zero_word2, int batch)
{
    const int b = blockIdx.z / nz;
    const BoardDev& T = tab[b];
    if (b > 0 && ((int)blockIdx.x * 64 >= T.S || (int)blockIdx.y * 4 >= T.S)) return;
    warp_gather<WarpJpeg, FPT>(WarpJpeg{planes, plane_stride, descs, sw, sh}, warp_board_dst(T, s0), zero_word, zero_word2, batch, blockIdx.z - b * nz);
}

// blockIdx.z = profile * nz + group of frames; profile p writes its frames dst_profile_stride bytes behind profile p - 1's
template <int FPT>
__global__ __launch_bounds__(256) void k_warp_jpeg_profile(const u8* __restrict__ planes, size_t plane_stride, const JpegDesc* __restrict__ descs, int sw,
                                                            int sh, WarpM M, int dw, int dh, int bw0, int rot180, u8* __restrict__ dst, int dst_stride,
                                                            size_t dst_frame_stride, size_t dst_profile_stride, const StaticTabs* __restrict__ st,
                                                            const ProfileTabs* __restrict__ ptabs, int nz, u32* __restrict__ zero_word,
                                                            u32* __restrict__ zero_word2, int batch)
{
    const int pi = blockIdx.z / nz;
    warp_gather<WarpJpegProfile, FPT>(WarpJpegProfile{{planes, plane_stride, descs, sw, sh}, st, ptabs + pi},
                                      WarpDst{M.m, dw, dh, bw0, rot180, dst + (size_t)pi * dst_profile_stride, dst_stride, dst_frame_stride}, zero_word,
                                      zero_word2, batch, blockIdx.z - pi * nz);
}

// the profile is the board's: a workgroup stages its board's table
template <int FPT>
__global__ __launch_bounds__(256) void k_warp_jpeg_profile_mb(const u8* __restrict__ planes, size_t plane_stride, const JpegDesc* __restrict__ descs,
                                                               int sw, int sh, const BoardDev* __restrict__ tab, int nz, int s0,
                                                               const StaticTabs* __restrict__ st, u32* __restrict__ zero_word,
                                                               u32* __restrict__ zero_word2, int batch)
{
    const int b = blockIdx.z / nz;
    const BoardDev& T = tab[b];
    if (b > 0 && ((int)blockIdx.x * 64 >= T.S || (int)blockIdx.y * WP_ROWS >= T.S)) return;
    warp_gather<WarpJpegProfile, FPT>(WarpJpegProfile{{planes, plane_stride, descs, sw, sh}, st, T.ptabs}, warp_board_dst(T, s0), zero_word, zero_word2,
                                      batch, blockIdx.z - b * nz);
}

// what both launchers do around their kernels: the refusals, the groups of frames, the grid, the profiling bracket;
// launch(many, grid, nz) issues the many-frames form (or the one-frame form) of the source's kind
template <class F>
static int warp_jpeg_launch(cbv_ctx* ctx, const WarpSrc& s, const char* who, int dw, int dh, int zmul, int batch, F&& launch)
{
    if (s.kind != WarpSrc::JPEG || !s.jpeg_planes || !s.jpeg_descs || (s.jpeg_plane_stride & 7) || s.g.w < 1 || s.g.h < 1)
        return cbv_fail(ctx, CBV_ERR_ARG, "%s: not a source of JPEG planes", who);
    if (batch <= 0 || dw < 1 || dh < 1 || zmul < 1) return cbv_fail(ctx, CBV_ERR_ARG, "%s: bad batch or destination", who);
    const bool prof = s.ptabs != nullptr;
    const int nz = warp_groups(batch, prof ? JPEG_PROFILE_FPT : JPEG_FPT), rows = prof ? WP_ROWS : 4;
    if ((long long)nz * zmul > 65535) return cbv_fail(ctx, CBV_ERR_ARG, "%s: %d x %d frames do not fit a launch", who, zmul, batch);
    const dim3 grid((dw + 63) / 64, (dh + rows - 1) / rows, nz * zmul);
    prof_begin(ctx, CBV_K_WARP_YUV);
    launch(batch >= 8, grid, nz);
    prof_end(ctx, CBV_K_WARP_YUV);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

int launch_warp_jpeg(cbv_ctx* ctx, WarpSrc s, const double* Minv9, int dw, int dh, int rot180, u8* dst, int dst_stride, size_t dst_frame_stride, int batch,
                     u32* zero_word, u32* zero_word2)
{
    WarpM M;
    for (int i = 0; i < 9; i++) M.m[i] = Minv9[i];
    int bw0, bh0;
    warp_block_shape(dw, dh, &bw0, &bh0);
    if (s.ptabs && s.np <= 0) return cbv_fail(ctx, CBV_ERR_ARG, "launch_warp_jpeg: %d profiles", s.np);
    const hipStream_t st = ctx->stream;
    return warp_jpeg_launch(ctx, s, "launch_warp_jpeg", dw, dh, s.ptabs ? s.np : 1, batch, [&](bool many, dim3 grid, int nz) {
        auto plain = [&](auto fpt) {
            hipLaunchKernelGGL((k_warp_jpeg<decltype(fpt)::value>), grid, dim3(256), 0, st, s.jpeg_planes, s.jpeg_plane_stride, s.jpeg_descs, s.g.w, s.g.h,
                               M, dw, dh, bw0, rot180, dst, dst_stride, dst_frame_stride, zero_word, zero_word2, batch);
        };
        auto profile = [&](auto fpt) {
            hipLaunchKernelGGL((k_warp_jpeg_profile<decltype(fpt)::value>), grid, dim3(256), 0, st, s.jpeg_planes, s.jpeg_plane_stride, s.jpeg_descs,
                               s.g.w, s.g.h, M, dw, dh, bw0, rot180, dst, dst_stride, dst_frame_stride, s.dst_profile_stride, ctx->tabs, s.ptabs, nz,
                               zero_word, zero_word2, batch);
        };
        if (s.ptabs) many ? profile(WarpInt<JPEG_PROFILE_FPT>()) : profile(WarpInt<1>());
        else many ? plain(WarpInt<JPEG_FPT>()) : plain(WarpInt<1>());
    });
}

int launch_warp_jpeg_mb(cbv_ctx* ctx, WarpSrc s, const BoardDev* tab, int nb, int maxS, int s0, int batch, u32* zero_word, u32* zero_word2)
{
    const hipStream_t st = ctx->stream;
    return warp_jpeg_launch(ctx, s, "launch_warp_jpeg_mb", maxS, maxS, nb, batch, [&](bool many, dim3 grid, int nz) {
        auto plain = [&](auto fpt) {
            hipLaunchKernelGGL((k_warp_jpeg_mb<decltype(fpt)::value>), grid, dim3(256), 0, st, s.jpeg_planes, s.jpeg_plane_stride, s.jpeg_descs, s.g.w,
                               s.g.h, tab, nz, s0, zero_word, zero_word2, batch);
        };
        auto profile = [&](auto fpt) {
            hipLaunchKernelGGL((k_warp_jpeg_profile_mb<decltype(fpt)::value>), grid, dim3(256), 0, st, s.jpeg_planes, s.jpeg_plane_stride, s.jpeg_descs,
                               s.g.w, s.g.h, tab, nz, s0, ctx->tabs, zero_word, zero_word2, batch);
        };
        if (s.ptabs) many ? profile(WarpInt<JPEG_PROFILE_FPT>()) : profile(WarpInt<1>());
        else many ? plain(WarpInt<JPEG_FPT>()) : plain(WarpInt<1>());
    });
}
