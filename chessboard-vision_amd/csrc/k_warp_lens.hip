// The warp with the camera's lens distortion corrected in the gather (include/cbv.h, cbv_lens): the sources without a colour
// profile of their own kernels' kind, WarpBgr (both byte-map forms), WarpProfile, WarpRaw<FMT> for the six YUV and four
// Bayer layouts, and WarpJpeg; the raw and JPEG sources WITH a profile are k_warp_lens_profile.hip's.  The kernels live in
// files of their own: the counts of k_warp.hip, k_warp_raw_profile.hip and k_warp_jpeg.hip stay what they are.  One frame
// per thread below batch 8, four from there on (as the lens-free kernels of these sources take; not timed against each
// other for the lens forms).  tests/test_warp_lens_resources.py lists the kernels; DESIGN.md section 6r has their registers.
#include "warp_lens.h"

int launch_warp_lens(cbv_ctx* ctx, WarpSrc s, const LensDev& lens, const LensBoard* tab, int ne, int max_dw, int max_dh, int s0, int batch,
                     u32* zero_word, u32* zero_word2)
{
    if (s.cs) return launch_warp_lens_cs(ctx, s, lens, tab, ne, max_dw, max_dh, s0, batch, zero_word, zero_word2);
    if ((s.raw() || s.kind == WarpSrc::JPEG) && s.ptabs) return launch_warp_lens_profile(ctx, s, lens, tab, ne, max_dw, max_dh, s0, batch, zero_word, zero_word2);
    if (s.kind == WarpSrc::JPEG) {
        RC(warp_lens_jpeg_checked(ctx, s));
        return warp_lens_launch<WarpJpeg, 4>(ctx, WarpJpeg{s.jpeg_planes, s.jpeg_plane_stride, s.jpeg_descs, s.g.w, s.g.h}, CBV_K_WARP_YUV, lens, tab, ne,
                                             max_dw, max_dh, s0, batch, zero_word, zero_word2);
    }
    if (s.kind == WarpSrc::PROFILE)
        return warp_lens_launch<WarpProfile, 4>(ctx, WarpProfile{s.bgr, s.g, ctx->tabs, nullptr}, CBV_K_WARP, lens, tab, ne, max_dw, max_dh, s0, batch,
                                                zero_word, zero_word2);
    if (s.kind == WarpSrc::BGR) {
        if (s.norm.minmax)
            return warp_lens_launch<WarpBgr<true>, 4>(ctx, WarpBgr<true>{s.bgr, s.g, nullptr, s.norm.minmax, s.norm.mm_stride}, CBV_K_WARP, lens, tab, ne,
                                                      max_dw, max_dh, s0, batch, zero_word, zero_word2);
        return warp_lens_launch<WarpBgr<false>, 4>(ctx, WarpBgr<false>{s.bgr, s.g, s.norm.lut, nullptr, 0}, CBV_K_WARP, lens, tab, ne, max_dw, max_dh, s0,
                                                   batch, zero_word, zero_word2);
    }
    RC(warp_raw_checked(ctx, &s, batch));
    int rc = CBV_OK;
    warp_dispatch(s.r.fmt, batch, [&](auto fmt, auto) {
        constexpr int FMT = decltype(fmt)::value;
        if constexpr (FMT != CBV_FMT_BGR) {
            const bool bayer = raw_fmt_bayer(FMT);
            rc = warp_lens_launch<WarpRaw<FMT>, 4>(ctx, WarpRaw<FMT>{s.planes.p[0], bayer ? nullptr : s.planes.p[1], bayer ? nullptr : s.planes.p[2], s.r, s.g.w, s.g.h},
                                                   CBV_K_WARP_YUV, lens, tab, ne, max_dw, max_dh, s0, batch, zero_word, zero_word2);
        }
    });
    return rc;
}
