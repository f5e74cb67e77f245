// cv2.bilateralFilter(d, sigmaColor, sigmaSpace) on 8UC3 (frame_enhancer.py:131).
//
// VALU/LDS-bound stencil (49 taps at d = 9), not an HBM-bound one.  Structure:
//   - persistent workgroups of 768 lanes (12 waves = 3 per SIMD), one per CU, each walking 128x48-pixel tiles;
//     consecutive tiles of one XCD are neighbours, so halo rows are re-read from that XCD's L2.  Three waves per SIMD,
//     not four, on purpose: see bilateral_nt;
//   - the tile (+4 px halo, REFLECT_101 at the image border) sits in LDS as
//     packed BGRx dwords: |db|+|dg|+|dr| is ONE v_sad_u8; the next tile is
//     prefetched into registers while the current one is filtered;
//   - the tap weight w = space * colour is ONE table lookup: taps with the same
//     dy^2 + dx^2 share their space weight, so there are only 10 distinct space
//     weights at d = 9, and folded[class][sad] (10 x 766 floats, 30 KB, built on
//     the host with the same single float multiply) replaces the colour-table
//     lookup AND the multiply.  The class offset rides in v_sad_u8's accumulator
//     operand (an SGPR), the byte address is one full-rate shift: per tap and
//     output 6 vector ops (sad, lshl, 3 fma, add) instead of 8.
//     The table is NOT replicated per bank any more (round 1 kept 32 copies of
//     the colour table, 98 KB, to make the gather conflict-free): lanes of a
//     half-wave read neighbouring pixels of one row at one tap, whose colour
//     distances are close, identical addresses broadcast, and addresses less
//     than 32 entries apart fall into different banks, so conflicts only arise
//     between lanes whose distances differ by a multiple of 32
//     (profiles/r02/sq_counters.txt has the measured conflict rate);
//   - each lane owns a 4-pixel strip on TWO adjacent rows; per tap row it reads
//     12 packed pixels with three aligned ds_read_b128 and converts them to
//     float once for all eight outputs (v_cvt_f32_ubyte is a half-rate op on
//     gfx950, like v_sad_u8; only f32 add/mul and simple integer ops are full
//     rate — tools/ubench_valu.hip);
//   - taps are accumulated per output in row-major (dy, dx) order exactly like
//     OpenCV's FMA3-dispatched body: w = space * colour (one rounding, here done
//     when the table is built), sum = fma(px, w, sum), wsum += w: bit-equal to
//     the oracle;
//   - PAIRS (the batched form at d = 9; build with BL_NO_PAIRS=1 for the 768-lane form without it): w(p -> q) and
//     w(q -> p) are the same table entry (the class depends on dx^2 + dy^2 only, the SAD is symmetric), so a weight
//     that connects two of a lane's OWN eight outputs is looked up once, by the output whose accumulation order
//     meets it first, and stays in a register for the other: 6 pairs on each of the two output rows and 16 between
//     them, 28 of the lane's 392 sad + shift + gather triples (7.1 %), with no LDS traffic, no barrier and no halo
//     lanes.  Sharing across lanes (a stash in LDS that a wave fills walking down a band) would reach half of all
//     lookups, but a weight that crosses dy rows lives dy row steps: 40 dwords per pixel column, far more than a CU's
//     LDS at any tiling that keeps the lanes busy;
//   - the PAIRS form is straight-line code for the whole tile: every tile row is instantiated with its dy, so the
//     disc's extent and the class offset of each tap (bl_class_off) are compile-time constants: no scalar branch per
//     tap, no tap_off loads.  It walks a row's 12 pixels in the outer loop, in half steps (one output row's four
//     outputs), looks the weights of the next half step up before the current one accumulates, reads the row in
//     pixel pairs one pair ahead and issues the next tile's prefetch after the lane's two own rows (its registers
//     are free while the 22 shared weights are live): 93 VGPRs (119 before), no scratch, 61 184 B of LDS, so beside
//     its three waves per SIMD (3 x 96 allocated registers) 224 registers stay free for the other lane's kernels, 152 before.
//     BL_NT1024=1 builds it with 1024 lanes on 128x64 tiles, held to 96 registers (five waves per SIMD by registers,
//     amdgpu_waves_per_eu on that instantiation only: 94 VGPRs, no scratch, 69 888 B), BL_NO_CAP=1 on top of it without
//     that cap, for A/B runs: both are slower on the path.
//   - round 6 takes out work the result does not need (94 VGPRs, no scratch, the same LDS):
//     the straight-line form takes tap (0, 0)'s weight as the constant 1.0f (8 of a lane step's 364 sad + shift + gather
//     triples; the launcher checks the table's entry once per table) and starts its sums from their first tap instead
//     of zeroing them; in every form a wave whose four tile rows lie below the frame (half of the waves of the 23rd
//     tile row at 1080 rows) commits and prefetches but does not filter.  BL_NO_CENTRE=1, BL_ZERO_INIT=1 and
//     BL_FULL_TILES=1 build the kernel without the one part, for A/B runs.
#include "cbv_device.h"
#include <type_traits>

#define BL_TW 128        // tile width in pixels (32 strips of 4)
#define BL_HALO 4        // halo in pixels (radius <= 4; 4 keeps ds_read_b128 aligned)
#define BL_PITCH (BL_TW + 2 * BL_HALO)
#define BL_LUT_WORDS (CBV_BL_MAXCLS * 768)

// Round 6: three pieces of work the result does not need, each behind its own switch for A/B runs (tools/ab.sh); the
// switch builds the form WITHOUT the part.  None of them changes an operand or the order of an accumulation.
#ifdef BL_NO_CENTRE
constexpr bool BL_CENTRE_FREE = false; // tap (0, 0) is looked up like any other
#else
constexpr bool BL_CENTRE_FREE = true;  // straight-line form: tap (0, 0) has SAD 0 and weight folded[class(0, 0)][0] == 1.0f
#endif
#ifdef BL_ZERO_INIT
constexpr bool BL_FIRST_TAP_INIT = false; // the sums start from 0.f
#else
constexpr bool BL_FIRST_TAP_INIT = true;  // straight-line form: the sums start from their first tap, (-R, 0)
#endif
#ifdef BL_FULL_TILES
constexpr bool BL_SKIP_BELOW = false; // rows below the frame are filtered and dropped by the store
#else
constexpr bool BL_SKIP_BELOW = true;  // a wave whose four tile rows all lie below the frame only commits and prefetches
#endif

__host__ __device__ constexpr int bl_row_reach(int R, int dy)
{
    int rx = 0;
    while ((rx + 1) * (rx + 1) + dy * dy <= R * R) rx++;
    return rx;
}

// Table offset of tap (dy, dx), known when compiling: cbv_tables.cpp's rule restated.  A class is a distinct dy^2 + dx^2,
// numbered by first occurrence in raster tap order; the offset is class x 768, -1 outside the disc.  The straight-line
// rows use it in place of bt->tap_off (scalar loads there cost SGPRs and, through them, VGPRs); launch_bilateral compares
// the two before it selects that form.
__host__ __device__ constexpr int bl_class_off(int R, int dy, int dx)
{
    int r2_of_cls[CBV_BL_MAXCLS] = {}, ncls = 0;
    for (int i = -R; i <= R; i++)
        for (int j = -R; j <= R; j++) {
            const int r2 = i * i + j * j;
            if (r2 > R * R) continue;
            int c = 0;
            while (c < ncls && r2_of_cls[c] != r2) c++;
            if (c == ncls) r2_of_cls[ncls++] = r2;
            if (i == dy && j == dx) return c * 768;
        }
    return -1;
}

int bilateral_offsets_mismatch(const BilateralTabs* t)
{
    const int R = t->radius;
    int bad = 0;
    for (int dy = -R; dy <= R; dy++)
        for (int dx = -R; dx <= R; dx++) bad += bl_class_off(R, dy, dx) != t->tap_off[dy + R][dx + R];
    return bad;
}

// The straight-line rows take the centre tap's weight as the constant 1.0f (space 1 x colour 1, SAD 0) instead of looking
// it up: true when the table's entry is anything else.
bool bilateral_centre_mismatch(const BilateralTabs* t)
{
    if (t->radius < 1 || t->radius > 4) return true;
    const int off = bl_class_off(t->radius, 0, 0);
    return off < 0 || off >= t->ncls * 768 || (&t->folded[0][0])[off] != 1.0f;
}

// bl_class_off for every tap of radius R, as a constant the unrolled straight-line rows index with literal subscripts
struct BlOffsets {
    int v[9][9];
};
template <int R>
constexpr BlOffsets bl_make_offsets()
{
    BlOffsets t = {};
    for (int dy = -R; dy <= R; dy++)
        for (int dx = -R; dx <= R; dx++) t.v[dy + R][dx + R] = bl_class_off(R, dy, dx);
    return t;
}
template <int R>
__device__ constexpr BlOffsets bl_offsets = bl_make_offsets<R>();

// the disc's extent (bl_row_reach) and the offsets (bl_class_off) are two statements of one rule: they must name the same taps
constexpr bool bl_disc_rules_agree(int R)
{
    for (int dy = -R; dy <= R; dy++)
        for (int dx = -R; dx <= R; dx++)
            if ((bl_class_off(R, dy, dx) >= 0) != ((dx < 0 ? -dx : dx) <= bl_row_reach(R, dy < 0 ? -dy : dy))) return false;
    return true;
}
static_assert(bl_disc_rules_agree(1) && bl_disc_rules_agree(2) && bl_disc_rules_agree(3) && bl_disc_rules_agree(4), "bl_class_off and bl_row_reach disagree");

template <int B, int E, class F>
__device__ __forceinline__ void bl_static_for(F&& f)
{
    if constexpr (B < E) {
        f(std::integral_constant<int, B>());
        bl_static_for<B + 1, E>(f);
    }
}

// NT lanes per workgroup (a multiple of 64): 32 strips x NT / 32 row pairs, i.e. tiles of 128 x NT / 16 pixels
// PAIRS: the lane's eight outputs share the tap weights that connect two of them (see the header comment)
// WAVES: waves per SIMD the register allocation must allow (0 = whatever NT needs)
template <int R, int NT, bool PAIRS = false, int WAVES = 0>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void k_bilateral(const u8* __restrict__ src, u8* __restrict__ dst, Geom g,
                                                           const BilateralTabs* __restrict__ bt, TileSet ts, int batch,
                                                           SatGate gate)
{
    static_assert((2 * R + 1) * (2 * R + 1) < 128, "the epilogue's d_rcp_1_64 is verified for weight sums in [1, 128)");
    static_assert(bl_row_reach(R, R) == 0, "an output's first tap in raster order is (-R, 0): accumulate starts the sums there");
    // static LDS (69 KB): compile-time addresses let the table gather use the ds_read immediate offset
#ifdef BL_TWO_COPIES
    // experiment (profiles/r03/bilateral_two_copies.txt): a second copy of the table 16 banks further on, used by the odd
    // strips, so that two lanes of a half-wave whose distances differ by a multiple of 32 no longer meet in one bank
    __shared__ __attribute__((aligned(16))) float fw[2 * BL_LUT_WORDS + 16];
#else
    __shared__ __attribute__((aligned(16))) float fw[BL_LUT_WORDS];              // [class][768] folded weights
#endif
    constexpr int BL_TH = NT / 16, BL_THREADS = NT;
    __shared__ __attribute__((aligned(16))) u32 tile[(BL_TH + 2 * R) * BL_PITCH];
    constexpr int ROWS = BL_TH + 2 * R;
    constexpr int GROUPS = BL_PITCH / 4;                        // 4-pixel groups per tile row
    constexpr int NG = ROWS * GROUPS;                           // groups per tile (<= 2448)
    constexpr int GPT = (NG + BL_THREADS - 1) / BL_THREADS;     // groups per thread (3)

    const int tid = threadIdx.x;
    for (int i = tid; i < bt->ncls * 768; i += BL_THREADS) fw[i] = (&bt->folded[0][0])[i];
#ifdef BL_TWO_COPIES
    for (int i = tid; i < bt->ncls * 768; i += BL_THREADS) fw[BL_LUT_WORDS + 16 + i] = (&bt->folded[0][0])[i];
    const u32 copy_off = (tid & 1) ? (u32)(BL_LUT_WORDS + 16) : 0u;
#endif

    const int tiles_per_frame = ts.cum[ts.n]; // the tiles of this launch's region (TileSet), not of the whole frame
    const int ntiles = tiles_per_frame * batch;
    const bool aligned = (g.stride & 3) == 0;

    // Interior 4-pixel groups are prefetched as 3 raw dwords; groups that touch the image border
    // (REFLECT_101) are rare and are fetched synchronously, byte-wise, when the tile is written.
    // a tile: frame and pixel origin (wave-uniform; worked out once per tile)
    struct TileAt {
        int f, px0, py0;
    };
    auto tile_at = [&](int t) {
        TileAt a;
        a.f = t / tiles_per_frame;
        int tyi, txi;
        tileset_at(ts, t - a.f * tiles_per_frame, txi, tyi);
        a.px0 = txi * BL_TW;
        a.py0 = tyi * BL_TH;
        return a;
    };
    auto group_origin = [&](const TileAt& ta, int gi, int& f, int& y, int& gx) {
        f = ta.f;
        const int r = gi / GROUPS, gc = gi - r * GROUPS;
        y = ta.py0 - R + r;
        gx = ta.px0 - BL_HALO + gc * 4;
    };
    auto prefetch = [&](const TileAt& t, int gi, u32* d) {
        int f, y, gx;
        group_origin(t, gi, f, y, gx);
        if (aligned && gx >= 0 && gx + 3 < g.w && y >= 0 && y < g.h) {
            const u32* q = (const u32*)(src + (size_t)f * g.frame_stride + (size_t)y * g.stride + (size_t)gx * 3);
            d[0] = q[0];
            d[1] = q[1];
            d[2] = q[2];
        }
    };
    auto commit = [&](const TileAt& t, int gi, const u32* d) {
        int f, y, gx;
        group_origin(t, gi, f, y, gx);
        u32 p0, p1, p2, p3;
        if (aligned && gx >= 0 && gx + 3 < g.w && y >= 0 && y < g.h) {
            p0 = d[0] & 0xFFFFFFu;
            p1 = (d[0] >> 24) | ((d[1] & 0xFFFFu) << 8);
            p2 = (d[1] >> 16) | ((d[2] & 0xFFu) << 16);
            p3 = d[2] >> 8;
        } else {
            const u8* sf = src + (size_t)f * g.frame_stride + (size_t)d_reflect101(y, g.h) * g.stride;
            u32 pp[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const u8* q = sf + (size_t)d_reflect101(gx + k, g.w) * 3;
                pp[k] = (u32)q[0] | ((u32)q[1] << 8) | ((u32)q[2] << 16);
            }
            p0 = pp[0];
            p1 = pp[1];
            p2 = pp[2];
            p3 = pp[3];
        }
        const int r = gi / GROUPS, gc = gi - r * GROUPS;
        *(uint4*)&tile[r * BL_PITCH + gc * 4] = make_uint4(p0, p1, p2, p3);
    };

    // persistent walk: sequence number s = i * gridDim + block; XCD x owns a contiguous tile range.  Tiles of frames
    // whose gate is closed (complement pass of a frame whose region already holds 0 and 255) are stepped over.
    auto next_open = [&](int s) {
        while (s < ntiles && sat_gate_closed(gate, xcd_remap(s, ntiles) / tiles_per_frame)) s += gridDim.x;
        return s;
    };
    int s = next_open(blockIdx.x);
    u32 pre[GPT][3];
    TileAt cur = {0, 0, 0};
    if (s < ntiles) {
        cur = tile_at(xcd_remap(s, ntiles));
#pragma unroll
        for (int k = 0; k < GPT; k++) {
            const int gi = tid + k * BL_THREADS;
            if (gi < NG) prefetch(cur, gi, pre[k]);
        }
    }
    const int sx = tid & 31;  // strip: pixels 4*sx .. 4*sx+3
    const int ly = (tid >> 5) * 2; // first of the lane's two tile rows
    const int wrow = __builtin_amdgcn_readfirstlane(tid >> 6) * 4; // first of the wave's four tile rows (wave-uniform)

    while (s < ntiles) {
        const TileAt here = cur;
        __syncthreads(); // previous tile fully consumed (and the LUT is written on the first pass)
#pragma unroll
        for (int k = 0; k < GPT; k++) {
            const int gi = tid + k * BL_THREADS;
            if (gi < NG) commit(here, gi, pre[k]);
        }
        __syncthreads();
        // prefetch the next tile while this one is filtered (PAIRS does it further down)
        if constexpr (!PAIRS) {
            s = next_open(s + gridDim.x);
            if (s < ntiles) {
                cur = tile_at(xcd_remap(s, ntiles));
#pragma unroll
                for (int k = 0; k < GPT; k++) {
                    const int gi = tid + k * BL_THREADS;
                    if (gi < NG) prefetch(cur, gi, pre[k]);
                }
            }
        }

        // No work below the frame: a wave owns four tile rows, and when all four lie below the frame (half of the waves on
        // the 23rd tile row of a 1080-row frame) the store would drop everything it computes.  Such a wave has committed
        // its part of the tile and prefetches its part of the next one, and filters nothing (wave-uniform).
        const bool live = !BL_SKIP_BELOW || here.py0 + wrow < g.h;

        // outputs: [row a/b][pixel 0..3]
        float sb[2][4], sg[2][4], sr[2][4], sw[2][4];
        u32 ctr[2][4];
        if (live) {
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int o = 0; o < 4; o++) {
                    if (!PAIRS || !BL_FIRST_TAP_INIT) sb[a][o] = sg[a][o] = sr[a][o] = sw[a][o] = 0.f; // else: from the first tap (accumulate)
                    ctr[a][o] = tile[(ly + a + R) * BL_PITCH + BL_HALO + sx * 4 + o];
                }
        }
        // One tile row per iteration, NOT unrolled (a fully unrolled body makes hipcc schedule ~250
        // live registers).  Tile row ly + i is tap row dy = i - R of output row a and dy = i - 1 - R of
        // output row b; every output still sees its taps in ascending (dy, dx) order.
        const u32* rowp0 = &tile[ly * BL_PITCH + sx * 4];
        // One tile row: looks up, for both output rows, the weight of every tap on it and accumulates.
        auto tile_row = [&](const int i) __attribute__((always_inline)) {
            const uint4* rowp = (const uint4*)(rowp0 + i * BL_PITCH);
            const uint4 q0 = rowp[0], q1 = rowp[1], q2 = rowp[2];
            // table offsets of this row's taps for both output rows: wave-uniform scalar loads (-1 = outside the disc)
            int off[2][2 * R + 1];
#pragma unroll
            for (int a = 0; a < 2; a++) {
                const int dyi = min(max(i - a, 0), 2 * R);
#pragma unroll
                for (int d = 0; d <= 2 * R; d++) off[a][d] = bt->tap_off[dyi][d];
            }
            const u32 p[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
            float fb[12], fg[12], fr[12];
#pragma unroll
            for (int j = 0; j < 12; j++) {
                fb[j] = (float)(p[j] & 255u);
                fg[j] = (float)((p[j] >> 8) & 255u);
                fr[j] = (float)((p[j] >> 16) & 255u);
            }
#pragma unroll
            for (int a = 0; a < 2; a++) {
                const int dyi = i - a; // tap-row index of output row a (0 .. 2R), wave-uniform
                if (dyi < 0 || dyi > 2 * R) continue;
#pragma unroll
                for (int dx = -R; dx <= R; dx++) {
                    const int toff = off[a][dx + R];
                    if (toff < 0) continue; // scalar branch
#ifdef BL_TWO_COPIES
                    const u32 tacc = (u32)toff + copy_off; // one vector add per tap, shared by the four outputs of the row
#else
                    const u32 tacc = (u32)toff;
#endif
#pragma unroll
                    for (int o = 0; o < 4; o++) {
                        const int j = o + 4 + dx;
                        // word index class * 768 + |db| + |dg| + |dr| in one v_sad_u8 (the class offset is its accumulator)
                        const u32 idx = __builtin_amdgcn_sad_u8(p[j], ctr[a][o], tacc);
                        const float wgt = *(const float*)((const u8*)fw + (idx << 2));
                        // v_muladd(v_cvt_f32(b), w, sum_b): fused, like OpenCV's FMA3-dispatched body
                        sb[a][o] = __fmaf_rn(fb[j], wgt, sb[a][o]);
                        sg[a][o] = __fmaf_rn(fg[j], wgt, sg[a][o]);
                        sr[a][o] = __fmaf_rn(fr[j], wgt, sr[a][o]);
                        sw[a][o] = sw[a][o] + wgt;
                    }
                }
            }
        };
        // PAIRS: every tile row is straight-line code, one instantiation per row I: tap row dy = I - a - R of output row a
        // and the disc's extent on it are known when compiling, so there are no per-tap scalar branches and no tap_off
        // loads.  It walks the row's 12 pixels in the OUTER loop: every output still meets its taps in ascending dx (its
        // accumulation order, the only order that fixes the result), and a pixel's three floats die before the next
        // one's are made.
        // The lane's two OWN tile rows are I = R (output row a's dy = 0, row b's dy = -1) and I = R + 1 (row a's dy = +1,
        // row b's dy = 0).  A tap of one of the lane's outputs that is another of its outputs has the same weight in
        // both directions (the class depends on dx^2 + dy^2 only, the SAD is symmetric), so only the output that needs
        // it FIRST looks it up and leaves it in a register for the other:
        //   wh[lo][hi]: pixels lo < hi of one output row; hi takes it at dx = lo - hi, lo at dx = hi - lo, later on the row;
        //   wv[ob][oa]: pixel ob of row b and pixel oa of row a; row b takes it at dy = -1, row a at dy = +1, one row later.
        float wh[4][4], wv[4][4];
        // Step U: pixel j of tile row I for output row a, U = (12 * I + j) * 2 + a.  look_up(U) makes the step's four
        // weights, accumulate(U) uses them; the weights of step U + 1 are looked up before step U accumulates, so the
        // gathers' latency is covered by a step's FMAs at the price of four more live weights.
        constexpr int STEPS = 12 * (2 * R + 2) * 2;
        u32 pq[2];          // the pixel of step U, by the parity of U / 2
        float wt[2][2][4];  // the weight of step U for output [a][o], by the parity of U
        float fb = 0.f, fg = 0.f, fr = 0.f;
        uint2 qa, qb;       // this pixel pair of the tile row and the next one
        auto look_up = [&](auto step) __attribute__((always_inline)) {
            constexpr int U = decltype(step)::value, T = U / 2, I = T / 12, j = T % 12, B = U & 1;
            if (U % 2 == 0) {
                // the row's 12 pixels come in pairs, one pair ahead: two pairs are live instead of three quads
                if (T == 0) qb = *(const uint2*)rowp0;
                if (T % 2 == 0) {
                    constexpr int P = T / 2 + 1; // the pair after this one: pair P % 6 of tile row P / 6
                    qa = qb;
                    if (P < 6 * (2 * R + 2)) qb = *(const uint2*)(rowp0 + (P / 6) * BL_PITCH + (P % 6) * 2);
                }
                pq[T & 1] = (T & 1) ? qa.y : qa.x;
            }
            const u32 pj = pq[T & 1];
#pragma unroll
            // Deliberately plain: a one-trip loop, plain `if`s on constants and the clamped index pc.  The same steps written with
            // `if constexpr` and a compile-time o compile to 114 VGPRs at 768 lanes and to scratch at 1024 (the front end then
            // unrolls, and hipcc schedules what it sees differently); tests/test_bilateral_resources.py guards the figures.
            for (int a = U % 2; a <= U % 2; a++) { // one output row per step; a loop so that `continue` skips the step
                const int dy = I - a - R; // of output row a on this tile row
                if (dy < -R || dy > R) continue;
#pragma unroll
                for (int o = 0; o < 4; o++) {
                    const int dx = j - 4 - o, po = j - 4; // po: the tap's index in the lane's strip, if 0 .. 3
                    const int pc = po & 3;                // po where `mine` holds; keeps the untaken branches' subscripts inside the arrays
                    if ((dx < 0 ? -dx : dx) > bl_row_reach(R, dy < 0 ? -dy : dy)) continue; // outside the disc
                    // the tap is another of the lane's own outputs (on output row a + dy)
                    const bool mine = po >= 0 && po < 4 && (a + dy == 0 || a + dy == 1) && (dx != 0 || dy != 0);
                    if (mine && dy == 0 && dx > 0)
                        wt[B][a][o] = wh[o][pc];
                    else if (mine && dy > 0)
                        wt[B][a][o] = wv[pc][o];
                    else if (BL_CENTRE_FREE && dy == 0 && dx == 0)
                        // the pixel against itself: SAD 0, space 1 x colour 1 (launch_bilateral checks the table's entry): no
                        // v_sad_u8, no shift, no gather, and fma(px, 1.0f, sum) and sum + 1.0f round as with the looked-up 1.0f
                        wt[B][a][o] = 1.0f;
                    else {
                        const u32 idx = __builtin_amdgcn_sad_u8(pj, ctr[a][o], (u32)bl_offsets<R>.v[dy + R][dx + R]);
                        const float wgt = *(const float*)((const u8*)fw + (idx << 2));
                        wt[B][a][o] = wgt;
                        if (mine && dy == 0) wh[pc][o] = wgt;
                        if (mine && dy < 0) wv[o][pc] = wgt;
                    }
                }
            }
        };
        auto accumulate = [&](auto step) __attribute__((always_inline)) {
            constexpr int U = decltype(step)::value, T = U / 2, I = T / 12, j = T % 12, B = U & 1;
            if (U % 2 == 0) {
                const u32 pj = pq[T & 1];
                fb = (float)(pj & 255u), fg = (float)((pj >> 8) & 255u), fr = (float)((pj >> 16) & 255u);
            }
#pragma unroll
            for (int a = U % 2; a <= U % 2; a++) { // one output row per step; a loop so that `continue` skips the step
                const int dy = I - a - R;
                if (dy < -R || dy > R) continue;
#pragma unroll
                for (int o = 0; o < 4; o++) {
                    const int dx = j - 4 - o;
                    if ((dx < 0 ? -dx : dx) > bl_row_reach(R, dy < 0 ? -dy : dy)) continue;
                    const float wgt = wt[B][a][o];
                    if (BL_FIRST_TAP_INIT && dy == -R && dx == 0) { // the only tap of row -R (static_assert above)
                        // the output's first tap in raster order: px * w and w are the bits of fma(px, w, 0.f) and 0.f + w
                        // (every operand is >= +0), so the sums start here and are never zeroed
                        sb[a][o] = fb * wgt;
                        sg[a][o] = fg * wgt;
                        sr[a][o] = fr * wgt;
                        sw[a][o] = wgt;
                        continue;
                    }
                    sb[a][o] = __fmaf_rn(fb, wgt, sb[a][o]);
                    sg[a][o] = __fmaf_rn(fg, wgt, sg[a][o]);
                    sr[a][o] = __fmaf_rn(fr, wgt, sr[a][o]);
                    sw[a][o] = sw[a][o] + wgt;
                }
                // The step's sums are complete at this point of the instruction stream.  Without it hipcc looks up the
                // weights of the whole tile first and accumulates afterwards: 168 VGPRs and 1.8 KB of scratch.
                // It names all 16 sums of the output row, so it starts with the step that gives the last of them (o = 3) its
                // first tap: the three pixel steps before it have one tap each and nothing to hold back.
                if (BL_FIRST_TAP_INIT && dy == -R && j < 7) continue; // output o's first tap is pixel j = 4 + o
                asm volatile("" : "+v"(sb[a][0]), "+v"(sg[a][0]), "+v"(sr[a][0]), "+v"(sw[a][0]), "+v"(sb[a][1]), "+v"(sg[a][1]), "+v"(sr[a][1]), "+v"(sw[a][1]),
                             "+v"(sb[a][2]), "+v"(sg[a][2]), "+v"(sr[a][2]), "+v"(sw[a][2]), "+v"(sb[a][3]), "+v"(sg[a][3]), "+v"(sr[a][3]), "+v"(sw[a][3]));
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        if constexpr (PAIRS) {
            constexpr int HALF = 12 * (R + 2) * 2; // the lane's two own rows end here
            auto step = [&](auto t) __attribute__((always_inline)) {
                constexpr int U = decltype(t)::value;
                if constexpr (U + 1 < STEPS) look_up(std::integral_constant<int, U + 1>());
                accumulate(t);
            };
            if (live) {
                look_up(std::integral_constant<int, 0>());
                bl_static_for<0, HALF>(step);
            }
            // the next tile's prefetch, issued only now: pre is dead while wh and wv are live, and the R tile rows that
            // follow still cover the loads (the same statements as above: as a lambda shared by both places they cost the
            // forms without PAIRS six registers)
            s = next_open(s + gridDim.x);
            if (s < ntiles) {
                cur = tile_at(xcd_remap(s, ntiles));
#pragma unroll
                for (int k = 0; k < GPT; k++) {
                    const int gi = tid + k * BL_THREADS;
                    if (gi < NG) prefetch(cur, gi, pre[k]);
                }
            }
            if (live) bl_static_for<HALF, STEPS>(step);
        } else if (live) {
#pragma unroll 1
            for (int i = 0; i <= 2 * R + 1; i++) tile_row(i);
        }
        if (!live) continue;
        const int f = here.f;
        const int x = here.px0 + sx * 4;
#pragma unroll
        for (int a = 0; a < 2; a++) {
            const int y = here.py0 + ly + a;
            if (y < g.h && x < g.w) {
                Px4 out;
                out.d[0] = out.d[1] = out.d[2] = 0;
#pragma unroll
                for (int o = 0; o < 4; o++) {
                    // the weight sum lies in [1, 49]: the centre tap's weight is exactly 1.0 (space 1 x colour 1) and no
                    // weight exceeds 1, so the exact reciprocal of that interval applies
                    const float inv = d_rcp_1_64(sw[a][o]);
                    // v_cvt_pk_u8_f32: cvRound (half to even) + pack; the value is a weighted mean of bytes, already in range
                    out.d[(3 * o) >> 2] = __builtin_amdgcn_cvt_pk_u8_f32(sb[a][o] * inv, (3 * o) & 3, out.d[(3 * o) >> 2]);
                    out.d[(3 * o + 1) >> 2] = __builtin_amdgcn_cvt_pk_u8_f32(sg[a][o] * inv, (3 * o + 1) & 3, out.d[(3 * o + 1) >> 2]);
                    out.d[(3 * o + 2) >> 2] = __builtin_amdgcn_cvt_pk_u8_f32(sr[a][o] * inv, (3 * o + 2) & 3, out.d[(3 * o + 2) >> 2]);
                }
                u8* q = dst + (size_t)f * g.frame_stride + (size_t)y * g.stride + (size_t)x * 3;
                const int npx = min(4, g.w - x);
                if (aligned && npx == 4) {
                    u32* qw = (u32*)q;
                    qw[0] = out.d[0];
                    qw[1] = out.d[1];
                    qw[2] = out.d[2];
                } else {
#pragma unroll
                    for (int j = 0; j < 12; j++)
                        if (j < npx * 3) q[j] = (u8)px_get(out, j);
                }
            }
        }
    }
}

// NT and workgroups per CU for a launch.  A batched launch has one persistent workgroup per CU, of 768 lanes = 3 waves
// per SIMD.  Alone the kernel is faster with 1024 lanes (4 waves hide the LDS gather better), but the other lane's
// kernels run BESIDE it and the whole path is what counts.  At 116-120 VGPRs 1024 lanes left them 48 registers per SIMD
// and lost 2-3 % (sweep, 1080p x 512: 640 lanes 26.0 k frames/s, 768 27.8 k, 896 25.5 k, 1024 27.2 k, 2 x 512 25.9 k).
// Round 5 brought the d = 9 form under 96 VGPRs, where 1024 lanes leave 128 registers and a wave slot: 768 lanes still
// win, by 1.7 % (BL_NT1024=1 builds the other form).
// One or two frames (the live-camera case) are too few 128 x 48 tiles for 256 persistent workgroups (a 1080p frame has
// 345: the second round is a third full).  128 x 32 tiles on TWO 512-lane workgroups per CU (2 x 52 KB of LDS, the same
// 4 waves per SIMD as one 1024-lane workgroup) put 510 tiles on 512 workgroups in one round.
#if defined(BL_NT1024) && !defined(BL_NO_PAIRS)
#define BL_NT9 1024
#ifdef BL_NO_CAP
#define BL_WAVES9 0
#else
#define BL_WAVES9 5
#endif
#else
#define BL_NT9 768
#define BL_WAVES9 0
#endif
static int bilateral_nt(cbv_ctx* ctx, Geom g, int batch)
{
    const long long t768 = (long long)((g.w + BL_TW - 1) / BL_TW) * ((g.h + 768 / 16 - 1) / (768 / 16)) * batch;
    return t768 < 2ll * ctx->num_cus ? 512 : ctx->btabs_host.radius == 4 ? BL_NT9 : 768;
}

// tiles of the launch: the whole frame, or (region-limited enhancement) the tiles covering er->px / all the others
static TileSet bilateral_tiles(Geom g, int nt, const EnhanceRegion* er)
{
    const int th = nt / 16;
    const int txn = (g.w + BL_TW - 1) / BL_TW, tyn = (g.h + th - 1) / th;
    if (!er) return tileset_make(txn, tyn, 0, 0, txn, tyn, false);
    return tileset_make(txn, tyn, er->px.x0 / BL_TW, er->px.y0 / th, (er->px.x1 + BL_TW - 1) / BL_TW, (er->px.y1 + th - 1) / th, er->invert != 0);
}

PxRect bilateral_region_cover(cbv_ctx* ctx, Geom g, int batch, PxRect need)
{
    const int th = bilateral_nt(ctx, g, batch) / 16;
    PxRect c = {need.x0 / BL_TW * BL_TW, need.y0 / th * th, (need.x1 + BL_TW - 1) / BL_TW * BL_TW, (need.y1 + th - 1) / th * th};
    c.x1 = c.x1 > g.w ? g.w : c.x1;
    c.y1 = c.y1 > g.h ? g.h : c.y1;
    return c;
}

template <int R, int NT, bool PAIRS = false, int WAVES = 0>
static int launch_bilateral_r(cbv_ctx* ctx, const u8* src, u8* dst, Geom g, int batch, int wgs_per_cu, const EnhanceRegion* er)
{
    const TileSet ts = bilateral_tiles(g, NT, er);
    const long long ntiles = (long long)ts.cum[ts.n] * batch;
    if (ntiles == 0) return CBV_OK;
    long long grid = (long long)ctx->num_cus * wgs_per_cu < ntiles ? (long long)ctx->num_cus * wgs_per_cu : ntiles; // persistent workgroups
    grid = (grid + 7) & ~7ll;                                 // whole XCD groups
    if (grid > ntiles) grid = ntiles;
    const SatGate gate = er ? er->gate : SatGate{nullptr, 0};
    prof_begin(ctx, CBV_K_BILATERAL);
    hipLaunchKernelGGL((k_bilateral<R, NT, PAIRS, WAVES>), dim3((unsigned)grid), dim3(NT), 0, ctx->stream, src, dst, g, ctx->btabs, ts, batch, gate);
    prof_end(ctx, CBV_K_BILATERAL);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

int launch_bilateral(cbv_ctx* ctx, const u8* src, u8* dst, Geom g, int batch, const EnhanceRegion* er)
{
    const int R = ctx->btabs_host.radius;
    if (R < 1 || R > 4) return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "bilateral radius %d not supported (d <= 9)", R);
    if (bilateral_nt(ctx, g, batch) == 512) switch (R) {
        case 1: return launch_bilateral_r<1, 512>(ctx, src, dst, g, batch, 2, er);
        case 2: return launch_bilateral_r<2, 512>(ctx, src, dst, g, batch, 2, er);
        case 3: return launch_bilateral_r<3, 512>(ctx, src, dst, g, batch, 2, er);
        default: return launch_bilateral_r<4, 512>(ctx, src, dst, g, batch, 2, er);
        }
    switch (R) {
    case 1: return launch_bilateral_r<1, 768>(ctx, src, dst, g, batch, 1, er);
    case 2: return launch_bilateral_r<2, 768>(ctx, src, dst, g, batch, 1, er);
    case 3: return launch_bilateral_r<3, 768>(ctx, src, dst, g, batch, 1, er);
#ifdef BL_NO_PAIRS
    default: return launch_bilateral_r<4, 768>(ctx, src, dst, g, batch, 1, er); // the batched form without weight sharing, for A/B runs
#else
    default:
        // the straight-line rows carry their table offsets as compile-time constants: never compute with a table they do not fit
        if (ctx->btabs_offsets_bad) return cbv_fail(ctx, CBV_ERR_STATE, "bilateral: compile-time tap offsets differ from the table's");
        if (BL_CENTRE_FREE && ctx->btabs_centre_bad) return cbv_fail(ctx, CBV_ERR_STATE, "bilateral: the table's centre weight is not 1.0f");
        return launch_bilateral_r<4, BL_NT9, true, BL_WAVES9>(ctx, src, dst, g, batch, 1, er);
#endif
    }
}
