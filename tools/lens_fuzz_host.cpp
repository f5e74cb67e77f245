// The host pieces of the lens model (csrc/lens_core.h: the forward model, the point functions, the host twin of the warp's
// coordinates and the footprint) over extreme inputs, for a run under AddressSanitizer and UBSan:
//
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//         -I chessboard-vision_amd/csrc tools/lens_fuzz_host.cpp -o lens_fuzz_host && ./lens_fuzz_host 400
//
// N rounds from a fixed generator: lenses from mild to absurd (huge and tiny focal lengths, coefficients up to 1e300),
// homographies that are degenerate, huge or hold infinities and NaNs, points far outside.  What is checked: no out-of-bounds
// access into the exact-size coordinate buffer, no undefined float-to-int cast (every coordinate is clamped, a position that
// is not a number becomes the lowest int32), a footprint that is refused or lies inside the frame, and point functions that
// return (possibly non-finite) numbers without a fault.  Needs no GPU and no HIP.  tests/test_lens_sanitizers.py builds and
// runs it.
#include <stdio.h>
#include <stdlib.h>

#include <limits>
#include <vector>

#include "lens_core.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 16);
}
static double unit() { return (rnd() & 0xFFFFFF) / (double)0x1000000; } // [0, 1)

// a value of a wild range: mostly moderate, sometimes huge, tiny, infinite or not a number (`special`)
static double wild(double scale, bool special)
{
    const uint32_t k = rnd() % 16;
    const double s = (rnd() & 1) ? 1.0 : -1.0;
    if (special && k == 0) return std::numeric_limits<double>::infinity() * s;
    if (special && k == 1) return std::numeric_limits<double>::quiet_NaN();
    if (k == 2) return s * 1e300 * unit();
    if (k == 3) return s * 1e-300 * unit();
    if (k == 4) return 0.0;
    return s * scale * unit();
}

int main(int argc, char** argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 400;
    long refused = 0, footprints = 0, outside = 0;
    for (int r = 0; r < rounds; r++) {
        // a lens that passes lens_valid: finite fields, positive focal lengths; the rest is free
        LensDev L;
        do {
            L = LensDev{fabs(wild(2000, false)) + (rnd() % 4 ? 1.0 : 1e-300), fabs(wild(2000, false)) + (rnd() % 4 ? 1.0 : 1e-300), wild(2000, false),
                        wild(2000, false),           wild(rnd() % 3 ? 0.5 : 1e6, false), wild(rnd() % 3 ? 0.5 : 1e6, false),
                        wild(0.01, false),           wild(0.01, false),                  wild(rnd() % 3 ? 0.5 : 1e6, false)};
        } while (!lens_valid(L));
        // lens_valid itself on fields that are not finite
        LensDev bad = L;
        (&bad.fx)[rnd() % 9] = wild(1, true);
        if (!lens_valid(bad)) refused++;
        double M[9];
        const bool tame = rnd() % 3 == 0;
        for (int i = 0; i < 9; i++) M[i] = tame ? (i % 4 == 0 ? 1.0 + unit() : unit() * (i < 6 ? 50 : 1e-3)) : wild(i < 6 ? 500 : 1, true);
        const int dw = 1 + (int)(rnd() % 130), dh = 1 + (int)(rnd() % 40);
        const int bw0 = 1 + (int)(rnd() % dw);
        // the coordinates, into a buffer of the exact size
        std::vector<int32_t> xy((size_t)dw * dh * 2);
        lens_warp_coords_host(L, M, dw, dh, bw0, xy.data());
        for (size_t i = 0; i < xy.size(); i += 2) {
            const int sx = xy[i] >> 5, sy = xy[i + 1] >> 5;
            if (sx < -1 || sx > 32767 || sy < -1 || sy > 32767) outside++;
        }
        // the footprint: refused, or inside the frame and not empty
        const int w = 1 + (int)(rnd() % 4000), h = 1 + (int)(rnd() % 3000);
        int r4[4] = {-7, -7, -7, -7};
        if (lens_warp_footprint(L, M, dw, dh, w, h, r4)) {
            footprints++;
            if (!(0 <= r4[0] && r4[0] < r4[2] && r4[2] <= w && 0 <= r4[1] && r4[1] < r4[3] && r4[3] <= h)) {
                fprintf(stderr, "round %d: footprint %d %d %d %d outside %d x %d\n", r, r4[0], r4[1], r4[2], r4[3], w, h);
                return 1;
            }
        } else if (r4[0] != -7 || r4[3] != -7) {
            fprintf(stderr, "round %d: a refused footprint was written\n", r);
            return 1;
        }
        // the point functions, points far outside and not finite included
        for (int k = 0; k < 16; k++) {
            const double px = wild(5000, true), py = wild(5000, true);
            double a, b, c, d;
            lens_undistort_px(L, px, py, &a, &b);
            lens_distort_px(L, a, b, &c, &d);
            lens_distort_px(L, px, py, &a, &b);
            volatile double sink = a + b + c + d;
            (void)sink;
        }
    }
    // one fixed case with a known answer: a pinhole lens leaves the centre where it is
    const LensDev P = {200, 200, 128, 96, 0, 0, 0, 0, 0};
    double u, v;
    lens_distort_px(P, 128, 96, &u, &v);
    if (u != 128 || v != 96) return 1;
    printf("%d rounds: %ld bad lenses refused, %ld footprints, %ld coordinates outside every frame\n", rounds, refused, footprints, outside);
    return 0;
}
