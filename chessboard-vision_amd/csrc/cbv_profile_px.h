// apply_color_profile for one pixel, shared by k_color_lab_hist (k_enhance.hip) and the warp of the sources with a profile (warp_gather.h).
#pragma once
#include "cbv_device.h"

// What d_profile_px reads, and nothing else of StaticTabs / ProfileTabs (7.5 KB): the LDS block of a kernel that applies
// the profile and does nothing else with the tables.  Lds = any struct with these members under these names.
struct ProfileLds {
    int sdiv[256];
    int hdiv[256];
    struct {
        u8 csa[256];
        u8 hmask[256];
        u32 hsel[256];
        float hfr[256];
        float s_f[2][256];
        float v_f[256];
    } pt;
};

// apply_color_profile for one pixel: byte maps, integer RGB2HSV_b, float HSV2RGB_b whose per-byte
// front end (sector, fraction, s/255, v/255) is tabulated.  Returns b | g << 8 | r << 16.
template <class Lds>
__device__ __forceinline__ u32 d_profile_px(const Lds& L, int b, int g, int r, bool radical)
{
    b = L.pt.csa[b];
    g = L.pt.csa[g];
    r = L.pt.csa[r];
    const int v = max(b, max(g, r)), vmin = min(b, min(g, r));
    const int diff = v - vmin;
    const int vr = v == r ? -1 : 0, vg = v == g ? -1 : 0;
    const int s = (diff * L.sdiv[v] + (1 << 11)) >> 12;
    int h = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + ((~vg) & (r - g + 4 * diff))));
    h = (h * L.hdiv[diff] + (1 << 11)) >> 12;
    h += h < 0 ? 180 : 0; // 0 <= h <= 180: saturate_cast<uchar> is the identity
    const int m = radical ? L.pt.hmask[h] : 0;
    const float fs = L.pt.s_f[m][s & 255];
    const float fv = L.pt.v_f[v];
    const float f = L.pt.hfr[h], f1 = 1.f - f;
    // tab = {v, v(1-s), v(1-s f), v(1-s(1-f))}; with s == 0 every entry equals v, as OpenCV's branch returns
    const float t1 = fv * (1.f - fs);
    const float t2 = fv * (1.f - fs * f);
    const float t3 = fv * (1.f - fs * f1);
    u32 T = __builtin_amdgcn_cvt_pk_u8_f32(fv * 255.0f, 0, 0u); // round-half-even + saturate + pack
    T = __builtin_amdgcn_cvt_pk_u8_f32(t1 * 255.0f, 1, T);
    T = __builtin_amdgcn_cvt_pk_u8_f32(t2 * 255.0f, 2, T);
    T = __builtin_amdgcn_cvt_pk_u8_f32(t3 * 255.0f, 3, T);
    return __builtin_amdgcn_perm(T, T, L.pt.hsel[h]);
}
