// The lens model of the warp (include/cbv.h, cbv_lens): OpenCV's five-coefficient Brown-Conrady distortion, one body for
// the host (cbv_lens_warp_coords, the point functions, the footprint, tools/lens_fuzz_host.cpp) and the device
// (warp_taps<true> of warp_gather.h).  Everything is float64, one rounding per operation, never fused (the build's
// -ffp-contract=off), in the order the header states.  Plain C++: no HIP type is needed to include this.  Private.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LENS_HD __host__ __device__ static inline
#else
#define LENS_HD static inline
#endif

// cbv_lens without the switch: what the kernels take by value
struct LensDev {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
};

// the forward model on a normalised point: (x, y) ideal -> (xd, yd) as the lens delivers it
LENS_HD void lens_distort_norm(const LensDev& L, double x, double y, double* xd, double* yd)
{
    const double r2 = x * x + y * y;
    const double kr = 1.0 + ((L.k3 * r2 + L.k2) * r2 + L.k1) * r2;
    const double xy2 = 2.0 * x * y;
    *xd = x * kr + L.p1 * xy2 + L.p2 * (r2 + 2.0 * x * x);
    *yd = y * kr + L.p1 * (r2 + 2.0 * y * y) + L.p2 * xy2;
}

// ... on a pixel position of the ideal (pinhole) frame: where the delivered frame shows it
LENS_HD void lens_distort_px(const LensDev& L, double u, double v, double* ud, double* vd)
{
    const double x = (u - L.cx) / L.fx, y = (v - L.cy) / L.fy;
    double xd, yd;
    lens_distort_norm(L, x, y, &xd, &yd);
    *ud = xd * L.fx + L.cx;
    *vd = yd * L.fy + L.cy;
}

// The source position of destination pixel (bx + x1, dy), in 1/32 px, clamped to the int32 range, before the rounding:
// M = the inverse homography (ideal frame <- board), bx = the origin of the pixel's block (warp_taps).  A position that is
// not a number becomes the lowest int32 in both coordinates: far outside every frame, the pixel reads nothing.
LENS_HD void lens_warp_xy32(const LensDev& L, const double* M, int bx, int x1, int dy, double* fX_out, double* fY_out)
{
    const double X0 = M[0] * bx + M[1] * dy + M[2];
    const double Y0 = M[3] * bx + M[4] * dy + M[5];
    const double W0 = M[6] * bx + M[7] * dy + M[8];
    const double W = W0 + M[6] * x1;
    const double Wi = W != 0. ? 1.0 / W : 0.;
    const double u = (X0 + M[0] * x1) * Wi, v = (Y0 + M[3] * x1) * Wi;
    double ud, vd;
    lens_distort_px(L, u, v, &ud, &vd);
    double fX = ud * 32.0, fY = vd * 32.0;
    if (fX != fX || fY != fY) fX = fY = -2147483648.0;
    *fX_out = fmax(-2147483648.0, fmin(2147483647.0, fX));
    *fY_out = fmax(-2147483648.0, fmin(2147483647.0, fY));
}

// The inverse on a pixel position of the delivered frame: cv2.undistortPoints' fixed-point iteration, exactly LENS_UNDISTORT_ROUNDS
// rounds, so the result is a function of the input alone.  Host only in practice (the corner points of a board).
#define LENS_UNDISTORT_ROUNDS 40
LENS_HD void lens_undistort_px(const LensDev& L, double ud, double vd, double* u, double* v)
{
    const double xd = (ud - L.cx) / L.fx, yd = (vd - L.cy) / L.fy;
    double x = xd, y = yd;
    for (int i = 0; i < LENS_UNDISTORT_ROUNDS; i++) {
        const double r2 = x * x + y * y;
        const double kr = 1.0 + ((L.k3 * r2 + L.k2) * r2 + L.k1) * r2;
        const double xy2 = 2.0 * x * y;
        const double tx = L.p1 * xy2 + L.p2 * (r2 + 2.0 * x * x);
        const double ty = L.p1 * (r2 + 2.0 * y * y) + L.p2 * xy2;
        x = (xd - tx) / kr;
        y = (yd - ty) / kr;
    }
    *u = x * L.fx + L.cx;
    *v = y * L.fy + L.cy;
}

// every field finite, fx and fy positive
LENS_HD bool lens_valid(const LensDev& L)
{
    const double f[9] = {L.fx, L.fy, L.cx, L.cy, L.k1, L.k2, L.p1, L.p2, L.k3};
    for (int i = 0; i < 9; i++)
        if (!(f[i] - f[i] == 0.0)) return false;
    return L.fx > 0.0 && L.fy > 0.0;
}

// The host twin of the kernels' coordinates: XY[dh][dw][2] = the rounded 1/32-px X, Y of every destination pixel; bw0 = the
// block width of the destination (warp_block_shape).  nearbyint under the default rounding mode rounds half to even, as the
// kernels' __double2int_rn does; its argument lies inside int32 after the clamp.
static inline void lens_warp_coords_host(const LensDev& L, const double* M, int dw, int dh, int bw0, int32_t* XY)
{
    for (int dy = 0; dy < dh; dy++)
        for (int dx = 0; dx < dw; dx++) {
            const int bx = (dx / bw0) * bw0;
            double fX, fY;
            lens_warp_xy32(L, M, bx, dx - bx, dy, &fX, &fY);
            int32_t* o = XY + ((size_t)dy * dw + dx) * 2;
            o[0] = (int32_t)nearbyint(fX);
            o[1] = (int32_t)nearbyint(fY);
        }
}

// Source pixels a dw x dh warp through the lens can sample, r4 = x0, y0, x1, y1 (exclusive), clipped to the w x h frame.  A
// lens bends the image of the destination's edges, so four corners no longer bound it: every border pixel of the
// destination, 2 (dw + dh) of them, goes through the full map, and the bounding box takes the 3 pixels of the projective
// footprint (the 1/32-px rounding and the bilinear taps) and one more for the bow of the curve between neighbouring border
// samples, which is far below a pixel for a lens that is monotone over the frame.  False: W not positive on the border, a
// position that is not finite or far outside, an empty footprint; callers then take the whole frame.
static inline bool lens_warp_footprint(const LensDev& L, const double* Minv, int dw, int dh, int w, int h, int* r4)
{
    if (dw <= 0 || dh <= 0) return false;
    double lo[2] = {1e30, 1e30}, hi[2] = {-1e30, -1e30};
    const long nborder = 2L * dw + 2L * dh;
    for (long k = 0; k < nborder; k++) {
        int dx, dy;
        if (k < dw) dx = (int)k, dy = 0;
        else if (k < 2L * dw) dx = (int)(k - dw), dy = dh - 1;
        else if (k < 2L * dw + dh) dx = 0, dy = (int)(k - 2L * dw);
        else dx = dw - 1, dy = (int)(k - 2L * dw - dh);
        const double W = Minv[6] * dx + Minv[7] * dy + Minv[8];
        if (!(W > 1e-12)) return false;
        double c[2];
        lens_distort_px(L, (Minv[0] * dx + Minv[1] * dy + Minv[2]) / W, (Minv[3] * dx + Minv[4] * dy + Minv[5]) / W, &c[0], &c[1]);
        for (int a = 0; a < 2; a++) {
            if (!(c[a] > -1e8 && c[a] < 1e8)) return false; // (not finite included; the casts below stay inside int)
            lo[a] = fmin(lo[a], c[a]);
            hi[a] = fmax(hi[a], c[a]);
        }
    }
    int r[4] = {(int)floor(lo[0]) - 4, (int)floor(lo[1]) - 4, (int)ceil(hi[0]) + 5, (int)ceil(hi[1]) + 5};
    r[0] = r[0] > 0 ? r[0] : 0;
    r[1] = r[1] > 0 ? r[1] : 0;
    r[2] = r[2] < w ? r[2] : w;
    r[3] = r[3] < h ? r[3] : h;
    if (r[2] <= r[0] || r[3] <= r[1]) return false;
    for (int i = 0; i < 4; i++) r4[i] = r[i];
    return true;
}
