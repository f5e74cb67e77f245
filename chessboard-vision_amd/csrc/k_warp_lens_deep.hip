// The lens form (warp_lens.h) of the developed mosaics (include/cbv.h): k_warp_lens of WarpDeep<LDS> and WarpDeepProfile<LDS>,
// with the tables in LDS and in global memory, with one frame per thread and with two (warp_many): 8 kernels, beside
// k_warp_deep.hip's lens-free kernels and in a unit of their own for the compile time.  launch_warp_lens hands a source here
// when WarpSrc::deep() holds.
#include "warp_lens.h"

int launch_warp_lens_deep(cbv_ctx* ctx, WarpSrc s, const LensDev& lens, const LensBoard* tab, int ne, int max_dw, int max_dh, int s0, int batch,
                          u32* zero_word, u32* zero_word2)
{
    const WarpLensTo to = {lens, tab, ne, max_dw, max_dh, s0};
    return warp_typed_deep(ctx, &s, batch, "launch_warp_lens_deep", [&](auto S) { return warp_launch_lens(ctx, S, to, batch, zero_word, zero_word2); });
}
