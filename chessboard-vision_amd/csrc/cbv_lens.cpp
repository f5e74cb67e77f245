// The host side of the lens model (include/cbv.h, cbv_lens): the checks, the point functions, the host twin of the kernels'
// coordinates and the footprint of a warp through the lens.  The arithmetic is lens_core.h's, the body the kernels run.
#include <math.h>

#include <algorithm>

#include "cbv_internal.h"

static LensDev lens_dev(const cbv_lens* l) { return LensDev{l->fx, l->fy, l->cx, l->cy, l->k1, l->k2, l->p1, l->p2, l->k3}; }

int lens_checked(cbv_ctx* ctx, const cbv_lens* lens, LensDev* out, const char* who)
{
    if (!lens) return cbv_fail(ctx, CBV_ERR_ARG, "%s: lens is null", who);
    const LensDev L = lens_dev(lens);
    if (!lens_valid(L)) return cbv_fail(ctx, CBV_ERR_ARG, "%s: a lens field is not finite, or fx or fy is not positive", who);
    *out = L;
    return CBV_OK;
}

extern "C" int cbv_lens_distort_points(const cbv_lens* lens, const double* xy_in, int n, double* xy_out)
{
    LensDev L;
    RC(lens_checked(nullptr, lens, &L, "cbv_lens_distort_points"));
    if (n < 0 || (n > 0 && (!xy_in || !xy_out))) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_lens_distort_points: bad arguments");
    for (int i = 0; i < n; i++) lens_distort_px(L, xy_in[2 * i], xy_in[2 * i + 1], &xy_out[2 * i], &xy_out[2 * i + 1]);
    return CBV_OK;
}

extern "C" int cbv_lens_undistort_points(const cbv_lens* lens, const double* xy_in, int n, double* xy_out)
{
    LensDev L;
    RC(lens_checked(nullptr, lens, &L, "cbv_lens_undistort_points"));
    if (n < 0 || (n > 0 && (!xy_in || !xy_out))) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_lens_undistort_points: bad arguments");
    for (int i = 0; i < n; i++) lens_undistort_px(L, xy_in[2 * i], xy_in[2 * i + 1], &xy_out[2 * i], &xy_out[2 * i + 1]);
    return CBV_OK;
}

extern "C" int cbv_lens_warp_coords(const cbv_lens* lens, const double* M9, int dw, int dh, int32_t* XY)
{
    LensDev L;
    RC(lens_checked(nullptr, lens, &L, "cbv_lens_warp_coords"));
    if (!M9 || !XY || dw <= 0 || dh <= 0 || dw > 8192 || dh > 8192) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_lens_warp_coords: bad arguments");
    int bw0, bh0;
    warp_block_shape(dw, dh, &bw0, &bh0);
    lens_warp_coords_host(L, M9, dw, dh, bw0, XY);
    return CBV_OK;
}

// warp_footprint through the lens (lens_core.h, lens_warp_footprint); no lens: the projective footprint
bool warp_footprint_lens(const double* Minv, const LensDev* lens, int dw, int dh, int w, int h, PxRect* out)
{
    if (!lens) return warp_footprint(Minv, dw, dh, w, h, out);
    int r[4];
    if (!lens_warp_footprint(*lens, Minv, dw, dh, w, h, r)) return false;
    *out = PxRect{r[0], r[1], r[2], r[3]};
    return true;
}

extern "C" int cbv_lens_warp_footprint(const cbv_lens* lens, const double* Minv9, int dw, int dh, int w, int h, int32_t* rect4)
{
    if (!Minv9 || !rect4 || dw <= 0 || dh <= 0 || w <= 0 || h <= 0) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_lens_warp_footprint: bad arguments");
    LensDev L;
    if (lens && lens->enabled) RC(lens_checked(nullptr, lens, &L, "cbv_lens_warp_footprint"));
    PxRect r;
    if (!warp_footprint_lens(Minv9, lens && lens->enabled ? &L : nullptr, dw, dh, w, h, &r)) return 0;
    rect4[0] = r.x0, rect4[1] = r.y0, rect4[2] = r.x1, rect4[3] = r.y1;
    return 1;
}
