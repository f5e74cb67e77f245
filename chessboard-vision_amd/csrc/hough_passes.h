// The passes of the per-square HoughCircles transform (k_hough.hip's header comment names them), as pieces that
// hough_item (k_hough, k_hough_mb) strings together once per square and k_piece_sweep_hough (k_piece_sweep.hip) strings
// together once per Canny threshold and once per setting.  The arithmetic exists here only.  Every piece is called by all
// HG_NT lanes of the workgroup unless it says otherwise; barriers a piece needs inside are its own, the barrier behind a
// piece is the caller's.
#pragma once
#include "cbv_device.h"

#define HG_MAXC 512 // accumulator maxima / candidate circles the FIRST pass keeps per square; a square with more
                    // (white noise, never a board square) is redone by the second pass, sized for the worst case
#define HG_NT 512   // lanes per workgroup: the phases are chains of LDS round trips; 8 waves hide them as well as 16 did (1.19 -> 0.95 us/frame alone)
#define HG_NW (HG_NT / 64)

struct HgCircle {
    float x, y, r;
    int votes;
};

__device__ __forceinline__ bool hg_before(const HgCircle& a, const HgCircle& b)
{
    if (a.votes != b.votes) return a.votes > b.votes;
    if (a.r != b.r) return a.r > b.r;
    if (a.x != b.x) return a.x < b.x;
    return a.y < b.y;
}

// wave-aggregated append of up to four items per lane: ONE LDS atomic per wave (all 64 lanes must call it).
// slot[k] = position of item k in the list, or -1.
__device__ __forceinline__ void hg_append4(int* counter, const bool pred[4], int slot[4])
{
    u64 m[4];
    int total = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        m[k] = __ballot(pred[k]);
        total += __popcll(m[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) slot[k] = -1;
    if (total == 0) return;
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0) base = atomicAdd(counter, total);
    base = __builtin_amdgcn_readfirstlane(base);
    const u64 below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (pred[k]) slot[k] = base + __popcll(m[k] & below);
        base += __popcll(m[k]);
    }
}

// Sobel at image pixel (x, y) from the padded gray plane (replicated borders are stored)
__device__ __forceinline__ void hg_sobel(const u8* g, int gs, int x, int y, int& dx, int& dy)
{
    const u8* r0 = g + y * gs + 3 + x; // row y-1, column x-1
    const u8* r1 = r0 + gs;
    const u8* r2 = r1 + gs;
    const int a = r0[0], b = r0[1], c = r0[2], d = r1[0], f = r1[2], p = r2[0], q = r2[1], r = r2[2];
    dx = (c - a) + 2 * (f - d) + (r - p);
    dy = (p - a) + 2 * (q - b) + (r - c);
}

// n / d by the reciprocal ceil(2^32 / d) that hg_square stores.  For d = 1 (a square at most four pixels wide has one
// group a row; an accumulator with dp >= w has one column) that is 2^32, which a u32 holds as 0: the quotient is n itself.
__device__ __forceinline__ int hg_div(int n, u32 inv) { return inv ? (int)__umulhi((u32)n, inv) : n; }

__device__ __forceinline__ int hg_sel4(int i, int a, int b, int c, int d) { return i == 0 ? a : (i == 1 ? b : (i == 2 ? c : d)); }

// One square in LDS: its geometry, the planes of the layout (hough_layout) and the counters of the workgroup.
// LDS planes, sized on the host for the largest square of the set (hough_layout).  Rows are padded so that
// image column 4k starts a dword: gray/map column x is byte 4 + x of a row of gs bytes (rows -1 .. h stored,
// gray with replicated borders), magnitude column x is element 2 + x of a row of mw u16 (zero borders).
struct HgSq {
    int w, h, n, tid, lane, wave, gs, mw;
    u8* g;        // P0..P4
    u8* map;      // P1 direction class, P2.. 0 weak / 1 none / 2 edge
    u16* mag;     // P1..P2, then the edge list
    int* acc;     // accumulator; the weak list before P4
    u16* centres;
    int* bins;    // [HG_NW][max_bins]
    HgCircle* circ; // P6..P7, over g + map (both dead by then) and, where hough_layout lets it, the accumulator
    u16* weak;
    u16* edges;
    float dp, idp;
    int min_dim, arows, acols, astep, acells;
    u32 inv_w, inv_ac;
    int ngx, ngroups; // 4-pixel groups of a row / of the square
    u32 inv_ngx;
    int* cnt;  // 0 weak, 1 edges, 2 centres, 3 circles
    int* over;
};

__device__ __forceinline__ void hg_square(HgSq& q, const SquareDesc& d, const HoughCfg& cfg, u8* smem, int* s_cnt, int* s_over)
{
    q.w = d.w;
    q.h = d.h;
    q.n = q.w * q.h;
    q.tid = threadIdx.x;
    q.lane = q.tid & 63;
    q.wave = q.tid >> 6;
    q.gs = cfg.gs;
    q.mw = cfg.mw;
    q.g = smem + cfg.off_g;
    q.map = smem + cfg.off_map;
    q.mag = (u16*)(smem + cfg.off_mag);
    q.acc = (int*)(smem + cfg.off_acc);
    q.centres = (u16*)(smem + cfg.off_centres);
    q.bins = (int*)(smem + cfg.off_bins);
    q.circ = (HgCircle*)(smem + cfg.off_circ);
    q.weak = (u16*)q.acc;
    q.edges = q.mag;
    q.dp = cfg.dp;
    q.idp = 1.f / q.dp;
    q.min_dim = min(q.w, q.h);
    q.arows = (int)ceilf(q.h * q.idp);
    q.acols = (int)ceilf(q.w * q.idp);
    q.astep = q.acols + 2;
    q.acells = (q.arows + 2) * q.astep;
    q.inv_w = (u32)((0x100000000ull + (u32)q.w - 1) / (u32)q.w);
    q.inv_ac = (u32)((0x100000000ull + (u32)q.acols - 1) / (u32)q.acols);
    q.ngx = (q.w + 3) >> 2;
    q.ngroups = q.ngx * q.h;
    q.inv_ngx = (u32)((0x100000000ull + (u32)q.ngx - 1) / (u32)q.ngx);
    q.cnt = s_cnt;
    q.over = s_over;
}

// minRadius / maxRadius of a square as PieceDetector passes them and as HoughCircles reads them
__device__ __forceinline__ void hg_radii(const HgSq& q, double min_ratio, double max_ratio, int& min_radius, int& max_radius)
{
    const int min_r = (int)((double)q.min_dim * min_ratio), max_r0 = (int)((double)q.min_dim * max_ratio);
    min_radius = max(min_r, 0);
    max_radius = max_r0 <= 0 ? max(q.w, q.h) : (max_r0 <= min_radius ? min_radius + 2 : max_r0);
}

// P0: plane (tight, 16-byte aligned and zero padded to 16) -> padded rows; zero the magnitude plane; counters to zero
__device__ __forceinline__ void hg_p0(const HgSq& q, const u32* __restrict__ src, int mag_bytes)
{
    const int w = q.w, h = q.h, n = q.n, tid = q.tid, gs = q.gs;
    u8* g = q.g;
    for (int i = tid; i < (n + 3) >> 2; i += HG_NT) {
        const u32 v = src[i];
        int y = __umulhi((u32)(4 * i), q.inv_w), x = 4 * i - y * w;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            if (4 * i + b < n) g[(y + 1) * gs + 4 + x] = (u8)(v >> (8 * b));
            if (++x == w) {
                x = 0;
                y++;
            }
        }
    }
    {
        uint4* mz = (uint4*)q.mag;
        const int nq = (mag_bytes + 15) >> 4;
        for (int i = tid; i < nq; i += HG_NT) mz[i] = make_uint4(0, 0, 0, 0);
        u32* mp = (u32*)q.map;
        const int nm = ((h + 2) * gs) >> 2;
        for (int i = tid; i < nm; i += HG_NT) mp[i] = 0x01010101u;
    }
    if (tid < 4) q.cnt[tid] = 0;
    if (tid == 0) *q.over = 0;
    __syncthreads();
    for (int y = tid; y < h; y += HG_NT) {
        u8* row = g + (y + 1) * gs;
        row[3] = row[4];
        row[4 + w] = row[3 + w];
    }
    __syncthreads();
    for (int x = tid; x < w + 2; x += HG_NT) {
        g[3 + x] = g[gs + 3 + x];
        g[(h + 1) * gs + 3 + x] = g[h * gs + 3 + x];
    }
}

// P1: Sobel, L1 magnitude and the non-maximum-suppression direction class, four pixels per lane
__device__ __forceinline__ void hg_p1(const HgSq& q)
{
    const int w = q.w, tid = q.tid, gs = q.gs, mw = q.mw, ngx = q.ngx, ngroups = q.ngroups;
    const u8* g = q.g;
    u8* map = q.map;
    u16* mag = q.mag;
    for (int t = tid; t < ngroups; t += HG_NT) {
        const int y = hg_div(t, q.inv_ngx), x0 = (t - y * ngx) << 2;
        int S[6], D[6];
        {
            int T[6], M[6], B[6];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const u32* row = (const u32*)(g + (y + r) * gs + x0);
                const u32 d0 = row[0], d1 = row[1], d2 = row[2];
                int* V = r == 0 ? T : (r == 1 ? M : B);
                V[0] = d0 >> 24;
                V[1] = d1 & 255;
                V[2] = (d1 >> 8) & 255;
                V[3] = (d1 >> 16) & 255;
                V[4] = d1 >> 24;
                V[5] = d2 & 255;
            }
#pragma unroll
            for (int i = 0; i < 6; i++) {
                S[i] = T[i] + 2 * M[i] + B[i];
                D[i] = B[i] - T[i];
            }
        }
        u32 mg[4], dirs = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int dx = S[k + 2] - S[k], dy = D[k] + 2 * D[k + 1] + D[k + 2];
            const int ax = abs(dx), ay = abs(dy) << 15;
            const int tg22x = ax * 13573; // (int)(0.4142135623730950488016887242097 * (1 << 15) + 0.5)
            const int tg67x = tg22x + (ax << 16);
            const u32 dir = ay < tg22x ? 0u : (ay > tg67x ? 1u : (((dx ^ dy) < 0) ? 3u : 2u));
            const bool in = x0 + k < w;
            mg[k] = in ? (u32)(ax + abs(dy)) : 0u;
            dirs |= dir << (8 * k);
        }
        u32* mrow = (u32*)(mag + (y + 1) * mw + 2 + x0);
        mrow[0] = mg[0] | (mg[1] << 16);
        mrow[1] = mg[2] | (mg[3] << 16);
        *(u32*)(map + (y + 1) * gs + 4 + x0) = dirs;
    }
}

// P2: non-maximum suppression in registers
__device__ __forceinline__ void hg_p2(const HgSq& q, int low, int high)
{
    const int w = q.w, tid = q.tid, gs = q.gs, mw = q.mw, ngx = q.ngx, ngroups = q.ngroups;
    u8* map = q.map;
    const u16* mag = q.mag;
    u16* weak = q.weak;
    for (int t0 = 0; t0 < ngroups; t0 += HG_NT) { // uniform trip count: hg_append uses wave ballots
        const int t = t0 + tid;
        const bool act = t < ngroups;
        const int y = act ? hg_div(t, q.inv_ngx) : 0, x0 = act ? (t - y * ngx) << 2 : 0;
        int E[3][6];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const u32* row = (const u32*)(mag + (y + r) * mw + x0);
            const u32 a = row[0], b = row[1], c = row[2], e = row[3];
            E[r][0] = a >> 16;
            E[r][1] = b & 0xFFFF;
            E[r][2] = b >> 16;
            E[r][3] = c & 0xFFFF;
            E[r][4] = c >> 16;
            E[r][5] = e & 0xFFFF;
        }
        u32* mp = (u32*)(map + (y + 1) * gs + 4 + x0);
        const u32 dirs = *mp;
        u32 codes = 0;
        bool isweak[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int dir = (dirs >> (8 * k)) & 3, m = E[1][k + 1];
            const int na = hg_sel4(dir, E[1][k], E[0][k + 1], E[0][k], E[0][k + 2]);
            const int nb = hg_sel4(dir, E[1][k + 2], E[2][k + 1], E[2][k + 2], E[2][k]);
            const bool keep = act && x0 + k < w && m > low && m > na && (dir < 2 ? m >= nb : m > nb);
            const u32 code = !keep ? 1u : (m > high ? 2u : 0u);
            codes |= code << (8 * k);
            isweak[k] = code == 0u;
        }
        int slot[4];
        hg_append4(&q.cnt[0], isweak, slot);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (slot[k] >= 0) weak[slot[k]] = (u16)((y + 1) * gs + 4 + x0 + k);
        if (act) *mp = codes;
    }
}

// P3: grow strong edges through 8-connected weak candidates until nothing changes.  A chain of weak pixels
// advances one pixel a sweep, so sweeps are many and short: with few candidates one wave floods alone (LDS
// operations of a wave are ordered, no barrier a sweep), the others wait at the barrier below.  Returns the number
// of weak candidates; ends behind a barrier.
__device__ __forceinline__ int hg_p3(const HgSq& q)
{
    const int tid = q.tid, lane = q.lane, wave = q.wave, gs = q.gs;
    u8* map = q.map;
    const u16* weak = q.weak;
    const int nweak = q.cnt[0];
    if (nweak <= 256) {
        if (wave == 0) {
            int idx[4];
#pragma unroll
            for (int k = 0; k < 4; k++) idx[k] = lane + 64 * k < nweak ? (int)weak[lane + 64 * k] : -1;
            for (;;) {
                bool ch = false;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (idx[k] < 0) continue;
                    const u8* c = map + idx[k];
                    const int any2 = (c[-gs - 1] | c[-gs] | c[-gs + 1] | c[-1] | c[1] | c[gs - 1] | c[gs] | c[gs + 1]) & 2;
                    if (any2) {
                        map[idx[k]] = 2;
                        idx[k] = -1;
                        ch = true;
                    }
                }
                if (!__ballot(ch)) break;
            }
        }
        __syncthreads();
    } else {
        for (;;) {
            int changed = 0;
            for (int k = tid; k < nweak; k += HG_NT) {
                const int idx = weak[k];
                if (map[idx] != 0) continue;
                const u8* c = map + idx;
                const int any2 = (c[-gs - 1] | c[-gs] | c[-gs + 1] | c[-1] | c[1] | c[gs - 1] | c[gs] | c[gs + 1]) & 2;
                if (any2) {
                    map[idx] = 2;
                    changed = 1;
                }
            }
            if (!__syncthreads_or(changed)) break;
        }
    }
    return nweak;
}

// P4: zero the accumulator (over the dead weak list) ...
__device__ __forceinline__ void hg_zero_acc(const HgSq& q)
{
    uint4* az = (uint4*)q.acc;
    for (int i = q.tid; i < (q.acells + 3) >> 2; i += HG_NT) az[i] = make_uint4(0, 0, 0, 0);
}

// ... list the edges (over the dead magnitude plane) ...
__device__ __forceinline__ void hg_list_edges(const HgSq& q)
{
    const int w = q.w, tid = q.tid, gs = q.gs, ngx = q.ngx, ngroups = q.ngroups;
    const u8* map = q.map;
    u16* edges = q.edges;
    for (int t0 = 0; t0 < ngroups; t0 += HG_NT) {
        const int t = t0 + tid;
        const bool act = t < ngroups;
        const int y = act ? hg_div(t, q.inv_ngx) : 0, x0 = act ? (t - y * ngx) << 2 : 0;
        const u32 codes = act ? *(const u32*)(map + (y + 1) * gs + 4 + x0) : 0x01010101u;
        bool isedge[4];
        int slot[4];
#pragma unroll
        for (int k = 0; k < 4; k++) isedge[k] = ((codes >> (8 * k)) & 255u) == 2u && x0 + k < w;
        hg_append4(&q.cnt[1], isedge, slot);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (slot[k] >= 0) edges[slot[k]] = (u16)((x0 + k) | (y << 8));
    }
}

// the vote step of the edge pixel (x, y): 1024 / dp accumulator cells along its gradient
__device__ __forceinline__ void hg_step(const HgSq& q, int x, int y, int& sx, int& sy)
{
    int ix, iy;
    hg_sobel(q.g, q.gs, x, y, ix, iy);
    const float vx = (float)ix, vy = (float)iy;
    const float mg = d_sqrt_rn(vx * vx + vy * vy);
    sx = d_round_f((vx * q.idp) * 1024.f / mg);
    sy = d_round_f((vy * q.idp) * 1024.f / mg);
}

// where the vote takes an edge's step from: the gray plane (hough_item), or a table made once (k_piece_sweep_hough)
struct HgStepSobel {
    __device__ __forceinline__ void operator()(const HgSq& q, int e, int x, int y, int& sx, int& sy) const
    {
        (void)e;
        hg_step(q, x, y, sx, sy);
    }
};

// ... and vote: one lane per (edge, direction) walks r = min_radius..max_radius along the gradient line
template <class Step>
__device__ __forceinline__ void hg_vote(const HgSq& q, int nedges, int min_radius, int max_radius, const Step& step)
{
    const u16* edges = q.edges;
    int* acc = q.acc;
    const float idp = q.idp;
    const int acols = q.acols, arows = q.arows, astep = q.astep;
    for (int t = q.tid; t < 2 * nedges; t += HG_NT) {
        const int e = t >> 1;
        const int x = edges[e] & 255, y = edges[e] >> 8;
        int sx, sy;
        step(q, e, x, y, sx, sy);
        if (t & 1) {
            sx = -sx;
            sy = -sy;
        }
        int x1 = d_round_f((x * idp) * 1024.f) + min_radius * sx, y1 = d_round_f((y * idp) * 1024.f) + min_radius * sy;
        for (int r = min_radius; r <= max_radius; x1 += sx, y1 += sy, r++) {
            const int x2 = x1 >> 10, y2 = y1 >> 10;
            if ((unsigned)x2 >= (unsigned)acols || (unsigned)y2 >= (unsigned)arows) break;
            atomicAdd(&acc[y2 * astep + x2], 1);
        }
    }
}

// P5: accumulator local maxima above the threshold, at most maxc of them (more: *q.over)
__device__ __forceinline__ void hg_p5(const HgSq& q, int acc_thr, int maxc)
{
    const int* acc = q.acc;
    const int acols = q.acols, astep = q.astep;
    for (int i = q.tid; i < q.arows * acols; i += HG_NT) {
        const int yy = hg_div(i, q.inv_ac), xx = i - yy * acols;
        const int base = (yy + 1) * astep + xx + 1;
        const int a = acc[base];
        if (a > acc_thr && a > acc[base - 1] && a >= acc[base + 1] && a > acc[base - astep] && a >= acc[base + astep]) {
            const int k = atomicAdd(&q.cnt[2], 1);
            if (k < maxc) q.centres[k] = (u16)base;
            else *q.over = 1;
        }
    }
}

// P6: radius of every centre.  Wave `wave` histograms centre c0 + wave into its own bins, turns them into
// inclusive prefix sums plus "highest non-empty bin <= i"; then 16 lanes of wave 0 walk one centre each the way
// the reference does: the highest non-empty bin opens a window of 10 bins, the walk resumes two bins below it.
// Ends behind a barrier.
__device__ __forceinline__ void hg_p6(const HgSq& q, int ncent, int nedges, int min_radius, int max_radius, int acc_thr, int max_bins)
{
    const int lane = q.lane, wave = q.wave, astep = q.astep;
    const float dp = q.dp;
    const u16* edges = q.edges;
    const u16* centres = q.centres;
    int* bins = q.bins;
    HgCircle* circ = q.circ;
    const int nbins = d_round_f((max_radius - min_radius) / dp * 10);
    const float minR2 = (float)min_radius * min_radius, maxR2 = (float)max_radius * max_radius;
    int* mybins = bins + wave * max_bins; // counts, then (inclusive prefix sum << 16) | highest non-empty bin <= i
    const int per_lane = (nbins + 63) >> 6;
    for (int c0 = 0; c0 < ncent; c0 += HG_NW) {
        const int c = c0 + wave;
        if (c < ncent) { // wave-uniform; the wave's bins are private, LDS operations of a wave are ordered
            for (int b = lane; b < nbins; b += 64) mybins[b] = 0;
            const int ofs = centres[c];
            const int cy = ofs / astep, cx = ofs - cy * astep;
            const float ccx = (cx + 0.5f) * dp, ccy = (cy + 0.5f) * dp;
            for (int j = lane; j < nedges; j += 64) {
                const float ex = ccx - (float)(edges[j] & 255), ey = ccy - (float)(edges[j] >> 8);
                const float r2 = ex * ex + ey * ey;
                if (minR2 <= r2 && r2 <= maxR2) {
                    const int bin = max(0, min(nbins - 1, d_round_f((d_sqrt_rn(r2) - min_radius) / dp * 10)));
                    atomicAdd(&mybins[bin], 1);
                }
            }
            // lane l owns bins [l * per_lane, (l + 1) * per_lane)
            const int b0 = lane * per_lane, b1 = min(b0 + per_lane, nbins);
            int tot = 0, last = 0;
            for (int b = b0; b < b1; b++) {
                const int v = mybins[b];
                tot += v;
                if (v) last = b; // bin 0 never opens a window: "none" and "bin 0" may share the value 0
            }
            int run = tot, pv = last;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(run, o, WAVE), p = __shfl_up(pv, o, WAVE);
                if (lane >= o) {
                    run += t;
                    pv = max(pv, p);
                }
            }
            int sum = run - tot;                      // exclusive prefix of the lane's chunk
            int prev = __shfl_up(pv, 1, WAVE);        // highest non-empty bin below the chunk
            if (lane == 0) prev = 0;
            for (int b = b0; b < b1; b++) {
                const int v = mybins[b];
                sum += v;
                if (v) prev = b;
                mybins[b] = (sum << 16) | prev; // both < 65536: at most 128 x 128 edges, bins < 64 K
            }
        }
        __syncthreads();
        if (wave == 0 && lane < HG_NW && c0 + lane < ncent) {
            const u32* W = (const u32*)(bins + lane * max_bins);
            int max_count = 0;
            float r_best = 0;
            int j = nbins - 1;
            u32 wj = W[j];
            while (j > 0) {
                const int up = (int)(wj & 0xFFFFu); // bins (up, j] are empty: prefix(up) == prefix(j)
                if (up < 1) break;
                const int lo = max(up - 10, -1);
                const u32 wlo = lo >= 0 ? W[lo] : 0u, wnext = lo >= 1 ? W[lo - 1] : 0u; // one round trip a window
                const int cur = (int)(wj >> 16) - (int)(wlo >> 16);
                const float r_cur = (up + lo) / 2.f / 10 * dp + min_radius;
                if ((cur * r_best >= max_count * r_cur) || (r_best < 1.1920929e-07f && cur >= max_count)) {
                    r_best = r_cur;
                    max_count = cur;
                }
                j = lo - 1;
                wj = wnext;
            }
            if (max_count > acc_thr) {
                const int ofs = centres[c0 + lane];
                const int cy = ofs / astep, cx = ofs - cy * astep;
                const int k = atomicAdd(&q.cnt[3], 1);
                // candidates live over g/map, which are dead now; every wave is past P4
                circ[k].x = (cx + 0.5f) * dp;
                circ[k].y = (cy + 0.5f) * dp;
                circ[k].r = r_best;
                circ[k].votes = max_count;
            }
        }
        __syncthreads();
    }
}

// P7, first half: rank sort (total order) of the ncirc candidates into `sorted`
__device__ __forceinline__ void hg_p7_sort(const HgSq& q, int ncirc, HgCircle* sorted)
{
    const HgCircle* circ = q.circ;
    for (int i = q.tid; i < ncirc; i += HG_NT) {
        const HgCircle ci = circ[i];
        int rank = 0;
        for (int j = 0; j < ncirc; j++) rank += (j != i && hg_before(circ[j], ci)) ? 1 : 0;
        sorted[rank] = ci;
    }
}

// P7, second half, wave 0 only: minDist suppression and the pick.  Up to 64 candidates one wave does it in registers
// (lane i = i-th circle); more fall back to one thread.  kept = circles HoughCircles returns (the first CBV_HOUGH_KEEP of
// them go to q.circ), pick = index of the chosen circle among them or -1, pc = that circle.
__device__ __forceinline__ void hg_p7_pick(const HgSq& q, int ncirc, HgCircle* sorted, int& kept, int& pick, HgCircle& pc)
{
    const int w = q.w, h = q.h, lane = q.lane, min_dim = q.min_dim;
    const float dp = q.dp;
    HgCircle* circ = q.circ;
    float md = (float)(min_dim / 3);
    if (md < dp) md = dp;
    const float md2 = md * md;
    const float max_off = (float)((double)min_dim * 0.3); // float32, as numpy evaluates the comparison
    kept = 0;
    pick = -1;
    pc = HgCircle{0.f, 0.f, 0.f, 0};
    if (ncirc <= 64) {
        const HgCircle me = lane < ncirc ? sorted[lane] : HgCircle{0.f, 0.f, 0.f, 0};
        bool alive = lane < ncirc;
        for (int i = 0; i < ncirc; i++) {
            // circle i survives iff no earlier survivor is closer than minDist; it then suppresses later ones
            const u64 am = __ballot(alive);
            if (!((am >> i) & 1)) continue;
            const float xi = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, me.x), i));
            const float yi = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, me.y), i));
            const float ex = xi - me.x, ey = yi - me.y;
            if (lane > i && ex * ex + ey * ey < md2) alive = false;
        }
        const u64 am = __ballot(alive);
        kept = __popcll(am);
        const int pos = __popcll(am & ((1ull << lane) - 1ull)); // index among the survivors
        const float ex = me.x - (float)(w / 2), ey = me.y - (float)(h / 2);
        const float dist = d_sqrt_rn(ex * ex + ey * ey);
        const bool cand = alive && dist < max_off;
        float best = cand ? dist : __builtin_inff();
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) best = fminf(best, __shfl_xor(best, o, WAVE));
        const u64 bm = __ballot(cand && dist == best); // first survivor with the smallest distance
        if (bm) {
            const int pl = __builtin_ctzll(bm);
            pick = __builtin_amdgcn_readlane(pos, pl);
            pc.x = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, me.x), pl));
            pc.y = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, me.y), pl));
            pc.r = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, me.r), pl));
            pc.votes = __builtin_amdgcn_readlane(me.votes, pl);
        }
        if (alive && pos < CBV_HOUGH_KEEP) circ[pos] = me; // survivors in order, for the result record
    } else if (lane == 0) {
        for (int i = 0; i < ncirc; i++) {
            const HgCircle ci = sorted[i];
            bool close = false;
            for (int j = 0; j < kept && !close; j++) {
                const float ex = sorted[j].x - ci.x, ey = sorted[j].y - ci.y;
                close = ex * ex + ey * ey < md2;
            }
            if (!close) sorted[kept++] = ci;
        }
        float best = __builtin_inff();
        for (int i = 0; i < kept; i++) {
            const HgCircle ci = sorted[i];
            const float ex = ci.x - (float)(w / 2), ey = ci.y - (float)(h / 2);
            const float dist = d_sqrt_rn(ex * ex + ey * ey);
            if (dist < max_off && dist < best) {
                best = dist;
                pick = i;
            }
        }
        if (pick >= 0) pc = sorted[pick];
        for (int i = 0; i < CBV_HOUGH_KEEP && i < kept; i++) circ[i] = sorted[i];
    }
    if (ncirc > 64) { // the serial branch ran on lane 0 only
        kept = __builtin_amdgcn_readfirstlane(kept);
        pick = __builtin_amdgcn_readfirstlane(pick);
    }
}

// _detect_circle_unified's kind of a picked circle: 1 'hough', 2 'tower_top' (piece_detector.py:262-266)
__device__ __forceinline__ u8 hg_kind(const HgCircle& pc, int min_dim) { return ((double)(int)pc.r < (double)min_dim * 0.20) ? 2 : 1; }

// ---------------------------------------------------------------------------
// host: the LDS layout and the per-pass capacity, shared by the launchers of k_hough.hip and k_piece_sweep.hip
// ---------------------------------------------------------------------------
// LDS layout for squares up to maxw x maxh
static inline size_t hough_layout(HoughCfg& cfg)
{
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    cfg.gs = (cfg.maxw + 11) & ~3;
    cfg.mw = ((cfg.maxw + 3) & ~3) + 4;
    const size_t maxn = (size_t)cfg.maxw * cfg.maxh;
    const size_t gbytes = (size_t)(cfg.maxh + 2) * cfg.gs;
    cfg.mag_bytes = (int)up16((size_t)(cfg.maxh + 2) * cfg.mw * 2);
    const float idp = 1.f / cfg.dp;
    const int arows = (int)ceilf(cfg.maxh * idp), acols = (int)ceilf(cfg.maxw * idp);
    const size_t acells = (size_t)(arows + 2) * (acols + 2);
    // bins of the radius histogram: round((max_radius - min_radius) / dp * 10) for the largest square
    const int md = cfg.maxw > cfg.maxh ? cfg.maxw : cfg.maxh, mind = cfg.maxw < cfg.maxh ? cfg.maxw : cfg.maxh;
    int span = md + 2;
    // (a square so small that int(min_dim * max_ratio) is 0 takes max(w, h) for its maximum, as with a ratio of 0)
    if (cfg.max_ratio > 0 && cfg.max_ratio <= 4 && (int)((cfg.min_dim > 0 ? cfg.min_dim : 2) * cfg.max_ratio) > 0) {
        span = (int)(mind * cfg.max_ratio) - (int)(mind * cfg.min_ratio) + 2;
        if (span < 4) span = 4; // (ratios above 1 ask for more bins than a side has pixels: every bin is zeroed and walked)
    }
    cfg.max_bins = (int)(span / cfg.dp * 10) + 16;
    const size_t acc_bytes = up16(acells * 4 > maxn * 2 ? acells * 4 : maxn * 2); // the weak list (u16 a pixel) shares it
    const size_t bin_bytes = (size_t)HG_NW * cfg.max_bins * 4, circ_bytes = cfg.maxc * sizeof(HgCircle);
    size_t off = 0;
    if (!cfg.keep_acc) {
        // The planes in the order of their deaths: magnitude / edge list (to P6) and centres (P5..P6) stay apart; gray and
        // map die with the vote, the accumulator with P5.  From P6 on the three are one region: candidates, then the bins of
        // P6, and over the bins (dead behind P6's last barrier) the candidates in HoughCircles' order.  A 128 x 128 square at
        // dp = 1 fits this way, with room for some 3 000 maxima in the second pass.
        cfg.off_mag = 0;
        cfg.off_centres = cfg.mag_bytes; // >= 2 bytes a pixel: the edge list reuses the magnitude plane
        cfg.off_g = cfg.off_centres + (int)up16((size_t)cfg.maxc * 2);
        cfg.off_map = cfg.off_g + (int)up16(gbytes);
        cfg.off_acc = cfg.off_map + (int)up16(gbytes);
        cfg.off_circ = cfg.off_g;
        cfg.off_bins = cfg.off_circ + (int)circ_bytes;
        cfg.off_order = cfg.off_bins;
        const size_t planes = (size_t)cfg.off_acc + acc_bytes, lists = (size_t)cfg.off_bins + (bin_bytes > circ_bytes ? bin_bytes : circ_bytes);
        return planes > lists ? planes : lists;
    }
    cfg.off_g = 0;
    cfg.off_circ = 0;
    cfg.off_map = (int)up16(gbytes);
    off = cfg.off_map + up16(gbytes);
    if (off < circ_bytes) off = circ_bytes; // candidates overlay g + map
    cfg.off_mag = (int)off;
    off += (size_t)cfg.mag_bytes; // >= 2 bytes a pixel: the edge list reuses it
    cfg.off_acc = (int)off;
    off += acc_bytes;
    cfg.off_centres = (int)off;
    off += up16((size_t)cfg.maxc * 2);
    cfg.off_bins = (int)off;
    off += bin_bytes;
    cfg.off_order = (int)off; // candidates in HoughCircles' order
    off += circ_bytes;
    return off;
}

// The set-up shared by the single- and the multi-board launches, so that a board computes what a pipeline of its own does.
static inline bool hough_dims_ok(const HoughCfg& cfg) { return !(cfg.maxw < 2 || cfg.maxh < 2 || cfg.maxw > 250 || cfg.maxh > 250); }

// maxc of a pass (retry fields cleared: the launch sets them).  First pass: small candidate lists (two workgroups per CU);
// squares that overflow them go to `retry`.  Second pass, over the listed squares only (normally none: the workgroups read
// a zero count and leave): no two 4-neighbours can both be maxima (a > left and a >= right exclude each other), so half
// the cells + 1 is room for every possible maximum; larger squares are capped by LDS and can still flag an overflow.
// `extra`: LDS bytes the caller needs beside the layout (k_piece_sweep_hough's step table).
static inline HoughCfg hough_pass_cfg(HoughCfg cfg, int pass, size_t extra = 0)
{
    cfg.retry = nullptr;
    cfg.retry_frame_base = 0;
    if (pass == 0) {
        cfg.maxc = HG_MAXC;
        return cfg;
    }
    const float idp = 1.f / (cfg.dp < 1.f ? 1.f : cfg.dp);
    const int cells = (int)ceilf(cfg.maxh * idp) * (int)ceilf(cfg.maxw * idp);
    cfg.maxc = (cells + 1) / 2 + 1;
    for (;;) {
        HoughCfg probe = cfg;
        if (hough_layout(probe) + extra <= 150 * 1024 || cfg.maxc <= HG_MAXC) break;
        cfg.maxc = cfg.maxc * 3 / 4;
    }
    if (cfg.maxc < HG_MAXC) cfg.maxc = HG_MAXC;
    return cfg;
}
