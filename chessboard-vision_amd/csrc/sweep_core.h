// The arithmetic of the ChangeDetector sensitivity sweep (include/cbv.h, cbv_pipeline_sweep), compiled for the device
// (k_sweep_eval) and for the host (cbv_sweep_eval_host).  Against a frozen model calibrated from a u8 plane with the constant
// variance iv, a pixel's score is z(d) = fdiv_rn((float)d, sqrt_rn(iv)) with d = |gray - mean| in 0..255 (ms_z_px), so a
// square's count over the threshold is a suffix sum of its histogram of d at the setting's cut, and its z_max is z of its
// highest occupied bin.
#pragma once
#include <math.h>

#include "cbv_internal.h"

#include "cbv_device.h"

// (overloads by target: the device forms are ms_z_px's, the host forms are correctly rounded under the build's
// -ffp-contract=off -fno-fast-math)
__device__ __forceinline__ float sweep_sd(float ivf) { return d_sqrt_rn(ivf); }
__device__ __forceinline__ float sweep_z(int d, float sd) { return __fdiv_rn((float)d, sd); }
__host__ inline float sweep_sd(float ivf) { return sqrtf(ivf); }
__host__ inline float sweep_z(int d, float sd) { return (float)d / sd; }

// a square with `cnt` of its n pixels over the threshold: 0 = not in the result dict, 1 LEVE, 2 PARCIAL, 3 TOTAL
// (ms_frame_finish: pct_changed as a Python float)
__host__ __device__ static inline int sweep_class(u32 cnt, u32 n)
{
    const double pct = ((double)cnt / (double)n) * 100.0;
    if (pct < 5.0) return 0;
    return pct > 75.0 ? 3 : (pct > 15.0 ? 2 : 1);
}

// the record of a frame from its three square sets and the largest z_score of the reported squares: the counts and
// classify_hand_pattern (change_detector.py:169-201)
__host__ __device__ static inline cbv_sweep_record sweep_record(u64 changed, u64 parcial, u64 total, float z_max)
{
    cbv_sweep_record r;
    r.changed = changed;
    r.parcial = parcial;
    r.total = total;
    r.z_max = z_max;
    const int n = __builtin_popcountll(changed), nt = __builtin_popcountll(total);
    r.n_changed = (uint8_t)n;
    r.n_total = (uint8_t)nt;
    const bool hand = nt >= 2 || n >= 4 || n > 2;
    r.flags = (uint8_t)(hand ? CBV_SWEEP_HAND : (n == 2 ? CBV_SWEEP_MOVE : 0));
    r.lifted = (int8_t)(n == 1 && !hand ? __builtin_ctzll(changed) : -1);
    return r;
}
