// The lens form (warp_lens.h) of the YUV sources in a colour space other than 0 (include/cbv.h, CBV_CS_*): k_warp_lens of
// WarpRawCs<FMT> and WarpRawProfileCs<FMT> for the six YUV layouts, with one frame per thread and with the many-frames form
// (warp_many: four without a profile, planar 4:2:0 two; two with one): 24 kernels, beside k_warp_cs.hip's lens-free kernels
// and in a unit of their own for the compile time.  launch_warp_lens hands a source here when WarpSrc::cs is not 0.
#include "warp_lens.h"

int launch_warp_lens_cs(cbv_ctx* ctx, WarpSrc s, const LensDev& lens, const LensBoard* tab, int ne, int max_dw, int max_dh, int s0, int batch,
                        u32* zero_word, u32* zero_word2)
{
    const WarpLensTo to = {lens, tab, ne, max_dw, max_dh, s0};
    return warp_typed_cs(ctx, &s, batch, "launch_warp_lens_cs", [&](auto S) { return warp_launch_lens(ctx, S, to, batch, zero_word, zero_word2); });
}
