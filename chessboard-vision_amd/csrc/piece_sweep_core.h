// The decision and smoothing arithmetic of the PieceDetector settings sweep (include/cbv.h, cbv_pipeline_piece_sweep),
// compiled for the device (k_piece_sweep_eval) and for the host (cbv_decide_piece, cbv_piece_sweep_eval_host,
// cbv_pipeline_piece_detail): PieceDetector.detect_piece from a square's statistics and the circle HoughCircles left it,
// the 5-frame history with _get_stable_detection, and the record / summary bookkeeping.
#pragma once
#include <math.h>

#include "cbv_internal.h"

// What k_piece_sweep_hough leaves per (setting, frame, square): _detect_circle_unified's answer after its int() casts.
struct PieceChoice {
    u8 kind;    // 0 no circle (or the square is uniform: HoughCircles not run), 1 'hough', 2 'tower_top'
    u8 flags;   // CBV_HOUGH_OVERFLOW
    int16_t r;  // int(r)
    int16_t cx, cy; // int(cx), int(cy)
};

// a fresh PieceDetector (piece_detector.py:36-41)
#define PS_HISTORY 5
#define PS_MIN_PRESENCE 0.6
#define PS_CIRCLE_THRESHOLD 0.6

// np.std(gray) < 15 as an exact integer test (piece_detector.py:305): nothing else is tried for such a square
__host__ __device__ static inline bool piece_uniform(const cbv_sq_stats* st)
{
    const long long n = st->n, sm = st->sum;
    return n * (long long)st->sumsq - sm * sm < 225ll * n * n;
}

// PieceDetector.detect_piece (piece_detector.py:289-345) for one square from its statistics and the circle
// _detect_circle_unified chose (found: kind 1 'hough' / 2 'tower_top' with its int() centre and radius), in the reference's
// arithmetic: np.std as an exact integer test, means and differences as float64 quotients, np.var of the ring means summed
// left to right like numpy does for fewer than eight elements.
__host__ __device__ static inline void piece_decide(const cbv_sq_stats* st, bool found, int kind, int cx, int cy, int radius, int w, int h,
                                                    double circle_threshold, cbv_piece_result* out)
{
    out->has_piece = 0;
    out->method = CBV_METHOD_NONE;
    out->cx = out->cy = out->radius = 0;
    out->confidence = 0.0;
    out->center_border_diff = 0.0;
    if (piece_uniform(st)) return; // np.std(gray) < 15: nothing else is tried
    if (found) {
        out->has_piece = 1;
        out->method = kind == 2 ? CBV_METHOD_TOWER_TOP : CBV_METHOD_HOUGH;
        out->cx = cx;
        out->cy = cy;
        out->radius = radius;
        out->confidence = kind == 2 ? 0.75 : 0.9;
        return;
    }
    const double zero = 0.0;
    const double cm = st->center_cnt ? (double)st->center_sum / (double)st->center_cnt : zero / zero; // np.mean of nothing is nan
    const double bm = st->border_cnt ? (double)st->border_sum / (double)st->border_cnt : zero / zero;
    const double diff = fabs(cm - bm);
    out->center_border_diff = diff;
    const int md = w < h ? w : h;
    if (diff > 40) {
        out->has_piece = 1;
        out->method = CBV_METHOD_CENTER_DIFF;
        out->cx = w / 2;
        out->cy = h / 2;
        out->radius = md / 3;
        out->confidence = diff / 80 < 1.0 ? diff / 80 : 1.0;
        return;
    }
    double rm[4];
    int nr = 0;
    for (int k = 0; k < 4; k++)
        if (st->ring_cnt[k] > 0) rm[nr++] = (double)st->ring_sum[k] / (double)st->ring_cnt[k];
    double symmetry = 0.0;
    if (nr >= 2) {
        double sum = 0;
        for (int k = 0; k < nr; k++) sum = sum + rm[k];
        const double mean = sum / nr;
        double sq = 0;
        for (int k = 0; k < nr; k++) {
            const double x = rm[k] - mean;
            sq = sq + x * x;
        }
        const double var = sq / nr;
        symmetry = var / 500 < 1.0 ? var / 500 : 1.0;
    }
    if (symmetry > circle_threshold) {
        out->has_piece = 1;
        out->method = CBV_METHOD_SYMMETRY;
        out->cx = w / 2;
        out->cy = h / 2;
        out->radius = md / 3;
        out->confidence = symmetry;
    }
}

// detect_piece of the sweep: the statistics of (frame, square) and the choice of (setting, frame, square)
__host__ __device__ static inline void piece_decide_choice(const cbv_sq_stats* st, const PieceChoice& c, int w, int h, cbv_piece_result* out)
{
    piece_decide(st, c.kind != 0, c.kind, c.cx, c.cy, c.r, w, h, PS_CIRCLE_THRESHOLD, out);
}

// _update_history + _get_stable_detection (piece_detector.py:99-122) of one square: hist = len << 8 | bits, bit 0 = newest
__host__ __device__ static inline bool piece_history_step(u32& hist, bool raw)
{
    u32 len = hist >> 8, bits = hist & 255u;
    bits = ((bits << 1) | (raw ? 1u : 0u)) & ((1u << PS_HISTORY) - 1u);
    if (len < PS_HISTORY) len++;
    hist = (len << 8) | bits;
    if (len < 3) return raw;
    return (double)__builtin_popcount(bits) / (double)len >= PS_MIN_PRESENCE;
}

// the record of one (setting, frame) from its six square sets and the radii of its circles
__host__ __device__ static inline cbv_piece_sweep_record piece_sweep_record(u64 raw, u64 stable, u64 hough, u64 tower, u64 cdiff, u64 sym,
                                                                            int r_min, int r_max, bool overflow)
{
    cbv_piece_sweep_record r;
    r.raw_occupied = raw;
    r.stable_occupied = stable;
    r.hough = hough;
    r.tower_top = tower;
    r.center_diff = cdiff;
    r.symmetry = sym;
    const bool any = ((hough | tower) != 0);
    r.r_min = (int16_t)(any ? r_min : 0);
    r.r_max = (int16_t)(any ? r_max : 0);
    r.n_raw = (uint8_t)__builtin_popcountll(raw);
    r.n_stable = (uint8_t)__builtin_popcountll(stable);
    r.flags = (uint8_t)(overflow ? CBV_PIECE_SWEEP_OVERFLOW : 0);
    r.pad = 0;
    return r;
}

// one frame's record into the setting's summary; r_sum / n_r / n_over = the frame's sum and count of int(r) over the squares
// with a circle, and its squares with an overflow
__host__ __device__ static inline void piece_sweep_sum(cbv_piece_sweep_summary* S, const cbv_piece_sweep_record& r, bool have_expected, u64 expected,
                                                       u32 r_sum, u32 n_r, u32 n_over)
{
    S->frames++;
    if (have_expected) {
        if (r.stable_occupied == expected) S->frames_exact++;
        S->missed += (u32)__builtin_popcountll(expected & ~r.stable_occupied);
        S->false_pos += (u32)__builtin_popcountll(r.stable_occupied & ~expected);
    }
    S->n_hough += (u32)__builtin_popcountll(r.hough);
    S->n_tower_top += (u32)__builtin_popcountll(r.tower_top);
    S->n_center_diff += (u32)__builtin_popcountll(r.center_diff);
    S->n_symmetry += (u32)__builtin_popcountll(r.symmetry);
    if (n_r) {
        if (S->n_r == 0 || r.r_min < S->r_min) S->r_min = r.r_min;
        if (S->n_r == 0 || r.r_max > S->r_max) S->r_max = r.r_max;
        S->n_r += n_r;
        S->r_sum += r_sum;
    }
    S->overflow += n_over;
}
