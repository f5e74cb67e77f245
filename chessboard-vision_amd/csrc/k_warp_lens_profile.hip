// The lens form (warp_lens.h) of the raw and JPEG sources that carry a colour profile: k_warp_lens of WarpRawProfile<FMT> for
// the six YUV and four Bayer layouts and of WarpJpegProfile, with one frame per thread and with two (warp_many, which says
// why): 22 kernels, in a unit of their own for the compile time.
#include "warp_lens.h"

int launch_warp_lens_profile(cbv_ctx* ctx, WarpSrc s, const LensDev& lens, const LensBoard* tab, int ne, int max_dw, int max_dh, int s0, int batch,
                             u32* zero_word, u32* zero_word2)
{
    const char* who = "launch_warp_lens_profile";
    const WarpLensTo to = {lens, tab, ne, max_dw, max_dh, s0};
    auto go = [&](auto S) { return warp_launch_lens(ctx, S, to, batch, zero_word, zero_word2); };
    if (s.kind == WarpSrc::JPEG && s.ptabs) return warp_typed_jpeg<true>(ctx, s, who, go);
    return warp_typed_raw_profile(ctx, &s, batch, who, go);
}
