// The lens forms (warp_lens.h) of the raw and JPEG sources that carry a colour profile: WarpRawProfile<FMT> for the six YUV
// and four Bayer layouts and WarpJpegProfile.  A unit of its own for the compile time.  One frame per thread below batch 8
// and two from there on for every family: the profile's registers and the lens's doubles come on top of the conversion's,
// and two is what the planar 4:2:0 family and the JPEG planes take lens-free; the forms were not timed against each other.
#include "warp_lens.h"

int launch_warp_lens_profile(cbv_ctx* ctx, WarpSrc s, const LensDev& lens, const LensBoard* tab, int ne, int max_dw, int max_dh, int s0, int batch,
                             u32* zero_word, u32* zero_word2)
{
    if (!(s.raw() || s.kind == WarpSrc::JPEG) || !s.ptabs) return cbv_fail(ctx, CBV_ERR_ARG, "launch_warp_lens_profile: not a raw or JPEG source with a profile");
    if (s.kind == WarpSrc::JPEG) {
        RC(warp_lens_jpeg_checked(ctx, s));
        return warp_lens_launch<WarpJpegProfile, 2>(ctx, WarpJpegProfile{{s.jpeg_planes, s.jpeg_plane_stride, s.jpeg_descs, s.g.w, s.g.h}, ctx->tabs, nullptr},
                                                    CBV_K_WARP_YUV, lens, tab, ne, max_dw, max_dh, s0, batch, zero_word, zero_word2);
    }
    RC(warp_raw_checked(ctx, &s, batch));
    int rc = CBV_OK;
    warp_dispatch(s.r.fmt, batch, [&](auto fmt, auto) {
        constexpr int FMT = decltype(fmt)::value;
        if constexpr (FMT != CBV_FMT_BGR) {
            const bool bayer = raw_fmt_bayer(FMT);
            rc = warp_lens_launch<WarpRawProfile<FMT>, 2>(
                ctx, WarpRawProfile<FMT>{{s.planes.p[0], bayer ? nullptr : s.planes.p[1], bayer ? nullptr : s.planes.p[2], s.r, s.g.w, s.g.h}, ctx->tabs, nullptr},
                CBV_K_WARP_YUV, lens, tab, ne, max_dw, max_dh, s0, batch, zero_word, zero_word2);
        }
    });
    return rc;
}
