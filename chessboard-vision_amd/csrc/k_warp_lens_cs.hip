// The lens forms (warp_lens.h) of the YUV sources in a colour space other than 0 (include/cbv.h, CBV_CS_*): WarpRawCs<FMT>
// and WarpRawProfileCs<FMT> for the six YUV layouts, beside k_warp_cs.hip's lens-free kernels and in a unit of its own for
// the compile time.  Frames per thread as the siblings of k_warp_lens.hip and k_warp_lens_profile.hip take them: one below
// batch 8, then four without a profile (planar 4:2:0: two, yuv_cs_fpt) and two with one.  launch_warp_lens hands a source
// here when WarpSrc::cs is not 0.
#include "warp_lens.h"

int launch_warp_lens_cs(cbv_ctx* ctx, WarpSrc s, const LensDev& lens, const LensBoard* tab, int ne, int max_dw, int max_dh, int s0, int batch,
                        u32* zero_word, u32* zero_word2)
{
    if (s.kind != WarpSrc::YUV || s.cs < 1 || s.cs > 3) return cbv_fail(ctx, CBV_ERR_ARG, "launch_warp_lens_cs: not a YUV source in colour space 1 to 3 (%d)", s.cs);
    RC(warp_raw_checked(ctx, &s, batch));
    const YuvCs cs = kYuvCs[s.cs];
    int rc = CBV_OK;
    warp_dispatch(s.r.fmt, batch, [&](auto fmt, auto) {
        constexpr int FMT = decltype(fmt)::value;
        if constexpr (raw_fmt_yuv(FMT)) {
            const WarpRaw<FMT> raw = {s.planes.p[0], s.planes.p[1], s.planes.p[2], s.r, s.g.w, s.g.h};
            if (s.ptabs)
                rc = warp_lens_launch<WarpRawProfileCs<FMT>, 2>(ctx, WarpRawProfileCs<FMT>{{raw, ctx->tabs, nullptr}, cs}, CBV_K_WARP_YUV, lens, tab, ne, max_dw,
                                                               max_dh, s0, batch, zero_word, zero_word2);
            else
                rc = warp_lens_launch<WarpRawCs<FMT>, yuv_cs_fpt(FMT)>(ctx, WarpRawCs<FMT>{raw, cs}, CBV_K_WARP_YUV, lens, tab, ne, max_dw, max_dh, s0, batch, zero_word,
                                                        zero_word2);
        }
    });
    return rc;
}
