"""What the ChangeDetector sensitivity sweep (cbv_pipeline_sweep) costs, and what the per-setting loop it replaces costs:
1080p, `enhance=False`, a 512-frame clip already run.
  - the full trackbar grid of calibrate_sensitivity.py (51 x 80 x 8 settings) in one sweep: GPU time of the three stages
    (cbv_sweep_info) and wall time, with records and with `records=False`; the k-only and the (z, iv)-only grids;
  - the per-setting loop as it is without the sweep: configure + run one frame + calibrate + run the clip + results, for a
    sample of settings, per setting;
  - k_change_hist per frame and blur kernel (hist_ms of one-kernel sweeps), next to k_change_blur_stats (cbv_profile_read).

    python tools/sweep_timing.py [--reps N] [--loop-settings M] [--lib PATH] [--json OUT]      (GPU box)

`--lib`: another build of the library, e.g. one compiled with SW_HIST_PLAIN=1 (every lane adds to the histogram itself).
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chessboard_vision_amd import _native as N  # noqa: E402

W, H = 1920, 1080
FRAMES, RUN = 512, 128


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def run_clip(p):
    for s0 in range(0, FRAMES, RUN):
        p.run(s0, RUN)


def time_sweep(p, reps, **kw):
    p.sensitivity_sweep(0, 0, FRAMES, **kw)  # warm-up
    wall, infos = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = p.sensitivity_sweep(0, 0, FRAMES, **kw)
        wall.append(1e3 * (time.perf_counter() - t0))
        infos.append(r.info)
    out = dict(settings=len(r.settings), wall_ms=spread(wall))
    for name in ("planes_ms", "hist_ms", "eval_ms"):
        out[name] = spread([i[name] for i in infos])
    out["kernels_distinct"] = infos[0]["kernels_distinct"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-settings", type=int, default=24)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--hist-only", action="store_true", help="only the k_change_hist figures (comparing two builds)")
    a = ap.parse_args()
    if a.lib:
        N.LIB_PATH = os.path.abspath(a.lib)
    from chessboard_vision_amd import synth as S
    from chessboard_vision_amd.stream import BoardPipeline, sensitivity_trackbar_grid
    pts = S.scaled_corners(W, H)
    z, iv, k = sensitivity_trackbar_grid()
    p = BoardPipeline(W, H, FRAMES)
    p.configure(pts, enhance=False)
    p.synth(0, FRAMES, scene="normal", frames_per_ply=32)
    run_clip(p)
    p.results(0, FRAMES)
    out = {}
    # k_change_hist per frame and kernel, next to k_change_blur_stats on the same frames
    out["hist_us_per_frame"] = {}
    for kk in (1, 3, 5, 13, 31):
        r = time_sweep(p, a.reps, settings=[(2.55, 600, kk)], records=False)
        out["hist_us_per_frame"][kk] = {n: 1e3 * v / FRAMES for n, v in r["hist_ms"].items()}
        print("k_change_hist k = %2d: %.2f us per frame (%.2f .. %.2f)" % (kk, out["hist_us_per_frame"][kk]["median"],
                                                                             out["hist_us_per_frame"][kk]["min"], out["hist_us_per_frame"][kk]["max"]), flush=True)
    if not a.hist_only:
        out["blur_stats_us_per_frame"] = {}
        for kk in (3, 13, 31):
            p.set_change_blur(kk)
            p.run(0, 1)
            p.calibrate_changes(0)
            run_clip(p)  # warm-up
            p.ctx.profile_reset()
            p.ctx.profile_enable(N.K_CHANGE_BLUR)
            try:
                run_clip(p)
                p.results(0, FRAMES)
                ms, _ = p.ctx.profile_read(N.K_CHANGE_BLUR)
            finally:
                p.ctx.profile_enable(-2)
                p.ctx.profile_reset()
            out["blur_stats_us_per_frame"][kk] = 1e3 * ms / FRAMES
            print("k_change_blur_stats k = %2d: %.2f us per frame" % (kk, out["blur_stats_us_per_frame"][kk]), flush=True)
        # the sweeps
        for name, kw in (("full grid", dict(z_thresholds=z, initial_variances=iv, blur_kernels=k)),
                         ("full grid, records=False", dict(z_thresholds=z, initial_variances=iv, blur_kernels=k, records=False)),
                         ("k only", dict(z_thresholds=[2.55], initial_variances=[600], blur_kernels=k)),
                         ("(z, iv) only", dict(z_thresholds=z, initial_variances=iv, blur_kernels=[13]))):
            out[name] = r = time_sweep(p, a.reps, **kw)
            print("%-26s %6d settings, %d kernels: planes %.2f ms, hist %.2f ms, eval %.2f ms, wall %.1f ms (%.1f .. %.1f)"
                  % (name, r["settings"], r["kernels_distinct"], r["planes_ms"]["median"], r["hist_ms"]["median"], r["eval_ms"]["median"],
                     r["wall_ms"]["median"], r["wall_ms"]["min"], r["wall_ms"]["max"]), flush=True)
        # the per-setting loop
        grid = [(zz, vv, kk) for zz in z for vv in iv for kk in k]
        sample = random.Random(1).sample(grid, a.loop_settings + 1)
        per = []
        for i, (zz, vv, kk) in enumerate(sample):  # (the first one is the warm-up: its configure allocates)
            p.ctx.synchronize()
            t0 = time.perf_counter()
            p.configure(pts, enhance=False, z_threshold=zz, initial_variance=vv, blur_kernel=kk)
            p.run(0, 1)
            p.calibrate_changes(0)
            p.reset_state()
            run_clip(p)
            p.results(0, FRAMES)
            if i:
                per.append(1e3 * (time.perf_counter() - t0))
        out["loop_ms_per_setting"] = dict(spread(per), settings=len(per))
        sweep_per = out["full grid"]["wall_ms"]["median"] / out["full grid"]["settings"]
        out["sweep_ms_per_setting"] = sweep_per
        out["ratio_per_setting"] = {n: out["loop_ms_per_setting"][n] / sweep_per for n in ("median", "min", "max")}
        print("per-setting loop over %d settings: %.1f ms per setting (%.1f .. %.1f); the sweep: %.4f ms per setting; ratio %.0f (%.0f .. %.0f)"
              % (len(per), out["loop_ms_per_setting"]["median"], out["loop_ms_per_setting"]["min"], out["loop_ms_per_setting"]["max"], sweep_per,
                 out["ratio_per_setting"]["median"], out["ratio_per_setting"]["min"], out["ratio_per_setting"]["max"]), flush=True)
    p.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
