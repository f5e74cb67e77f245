// The warp with the camera's lens distortion corrected in the gather (include/cbv.h, cbv_lens): k_warp_lens (warp_lens.h)
// of the sources without a colour profile of their own kernels' kind, WarpBgr (both byte-map forms), WarpProfile, WarpRaw<FMT>
// for the six YUV and four Bayer layouts, and WarpJpeg, with one frame per thread and with four (warp_many; as the lens-free
// kernels of these sources take, not timed against each other for the lens forms): 28 kernels, in a file of their own for
// the compile time.  The raw and JPEG sources WITH a profile are k_warp_lens_profile.hip's, YUV frames in a colour space
// other than 0 k_warp_lens_cs.hip's.  tests/test_warp_lens_resources.py lists the kernels; DESIGN.md section 6r has their
// registers.
#include "warp_lens.h"

int launch_warp_lens(cbv_ctx* ctx, WarpSrc s, const LensDev& lens, const LensBoard* tab, int ne, int max_dw, int max_dh, int s0, int batch,
                     u32* zero_word, u32* zero_word2)
{
    if (s.cs) return launch_warp_lens_cs(ctx, s, lens, tab, ne, max_dw, max_dh, s0, batch, zero_word, zero_word2);
    if (s.deep()) return launch_warp_lens_deep(ctx, s, lens, tab, ne, max_dw, max_dh, s0, batch, zero_word, zero_word2); // (k_warp_lens_deep.hip)
    if ((s.raw() || s.kind == WarpSrc::JPEG) && s.ptabs) return launch_warp_lens_profile(ctx, s, lens, tab, ne, max_dw, max_dh, s0, batch, zero_word, zero_word2);
    const WarpLensTo to = {lens, tab, ne, max_dw, max_dh, s0};
    auto go = [&](auto S) { return warp_launch_lens(ctx, S, to, batch, zero_word, zero_word2); };
    if (s.kind == WarpSrc::JPEG) return warp_typed_jpeg<false>(ctx, s, "launch_warp_lens", go);
    return warp_typed_plain(ctx, &s, batch, go);
}
