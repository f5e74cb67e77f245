// The warp of YUV frames in a colour space other than 0 (include/cbv.h, CBV_CS_*: BT.601 full range, BT.709 limited and
// full range), lens-free: the runtime-matrix forms of what k_warp.hip and k_warp_raw_profile.hip hold for colour space 0, for
// the six YUV layouts the kernels know.  The gather is warp_gather (warp_gather.h) with the sources WarpRawCs<FMT> and
// WarpRawProfileCs<FMT>: everything is their siblings' but the six constants of the conversion, which arrive inside the
// source (YuvCs, cbv_yuv.h), are uniform over the launch and stay in scalar registers.  So three colour spaces cost one more
// form of each kernel, not three, and colour space 0 keeps launching the kernels it always launched: the launchers of
// k_warp.hip hand a source here only when WarpSrc::cs is not 0.  This unit holds k_warp_one and k_warp_boards of the two
// sources for the six layouts, with one frame per thread and with the many-frames form (warp_many: what the siblings take,
// but two for planar 4:2:0 without a profile too, to stay at 64 VGPRs): 48 kernels.  The lens forms are k_warp_lens_cs.hip's.
// tests/test_yuv_cs_resources.py lists the kernels and their registers.
#include "warp_gather.h"

int launch_warp_cs(cbv_ctx* ctx, WarpSrc s, const double* Minv9, int dw, int dh, int rot180, u8* dst, int dst_stride, size_t dst_frame_stride, int batch,
                   u32* zero_word, u32* zero_word2)
{
    const char* who = "launch_warp_cs";
    const WarpOneTo to = {Minv9, dw, dh, rot180, dst, dst_stride, dst_frame_stride, s.np, s.dst_profile_stride};
    return warp_typed_cs(ctx, &s, batch, who, [&](auto S) { return warp_launch_one(ctx, who, S, to, batch, zero_word, zero_word2); });
}

int launch_warp_cs_mb(cbv_ctx* ctx, WarpSrc s, const BoardDev* tab, int nb, int maxS, int s0, int batch, u32* zero_word, u32* zero_word2)
{
    const char* who = "launch_warp_cs_mb";
    return warp_typed_cs(ctx, &s, batch, who, [&](auto S) { return warp_launch_boards(ctx, who, S, tab, nb, maxS, s0, batch, zero_word, zero_word2); });
}
