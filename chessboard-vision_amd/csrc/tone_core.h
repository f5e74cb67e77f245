// Piece colour per square (include/cbv.h, "piece colour per square"): the classification of one square, compiled for the
// host (cbv_tone.cpp: cbv_tone_classify_host, cbv_tone_calibrate_host) and for the device (k_tone.hip).  Every operation is
// a float64 multiply, add, subtract or divide rounded by itself: the translation units are built with -ffp-contract=off,
// and the expressions below are written one operation per statement so that nothing invites a fused form.
#ifndef CBV_TONE_CORE_H
#define CBV_TONE_CORE_H
#include "../../include/cbv.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CBV_TONE_HD __host__ __device__
#else
#define CBV_TONE_HD
#endif

enum { TONE_UNDECIDED = 0, TONE_WHITE = 1, TONE_BLACK = 2 };

// ROI 8 * row + col is dark iff row + col is odd
CBV_TONE_HD inline int tone_square_colour(int roi) { return ((roi >> 3) + (roi & 7)) & 1; }

// (a[0]-b[0])^2 + (a[1]-b[1])^2 + (a[2]-b[2])^2, accumulated left to right
CBV_TONE_HD inline double tone_dist2(const double* a, const double* b)
{
    const double e0 = a[0] - b[0], e1 = a[1] - b[1], e2 = a[2] - b[2];
    const double q0 = e0 * e0, q1 = e1 * e1, q2 = e2 * e2;
    const double s01 = q0 + q1;
    return s01 + q2;
}

CBV_TONE_HD inline void tone_mean(const cbv_tone_sums* s, double* f)
{
    const double n = (double)s->cnt;
    f[0] = (double)s->sum[0] / n;
    f[1] = (double)s->sum[1] / n;
    f[2] = (double)s->sum[2] / n;
}

// TONE_* of ROI `roi` with sums *s under *m
CBV_TONE_HD inline int tone_classify(const cbv_tone_model* m, int roi, const cbv_tone_sums* s)
{
    if (s->cnt == 0) return TONE_UNDECIDED;
    const int k = tone_square_colour(roi);
    const double* cW = m->centroid[k][0];
    const double* cB = m->centroid[k][1];
    double f[3];
    tone_mean(s, f);
    const double dW = tone_dist2(f, cW), dB = tone_dist2(f, cB), D = tone_dist2(cW, cB);
    const double m2 = 2.0 * m->margin;
    const double T = m2 * D;
    const double up = dB - dW, down = dW - dB;
    if (up >= T) return TONE_WHITE;
    if (down >= T) return TONE_BLACK;
    return TONE_UNDECIDED;
}

#endif // CBV_TONE_CORE_H
