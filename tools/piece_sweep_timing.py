"""What the PieceDetector settings sweep (cbv_pipeline_piece_sweep) costs, and what the per-setting loop it replaces costs:
1080p, `enhance=False`, a clip of --frames frames (512) already run, --reps repetitions (5), median and range.
  - the full trackbar grid of calibrate_piece_detector.py (50 x 70 radius positions) in one sweep, with records and with
    `records=False`: GPU time of the two kernels (cbv_piece_sweep_info) and wall time; a coarse grid (every 5th position)
    runs first, and a full-grid leg whose time projected from it does not fit --budget-s is reported as not measured;
  - param2 = 1..100 at fixed radii (one accumulator, P5-P7 per setting);
  - the two kernels per frame, from `info`;
  - the per-setting loop as it is without the sweep: configure + reset_state + set_check_squares + run + results, for a
    sample of settings, per setting (MaxRadius positions that truncate to 0 pixels are kept out of the sample: the
    per-setting path is not safe for them).

    python tools/piece_sweep_timing.py [--frames N] [--reps N] [--loop-settings M] [--coarse-step N] [--budget-s S] [--json OUT]      (GPU box)
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

W, H = 1920, 1080
RUN = 128


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def run_clip(p, frames):
    for s0 in range(0, frames, RUN):
        p.run(s0, min(RUN, frames - s0))


def time_sweep(p, frames, reps, **kw):
    p.piece_sweep(0, frames, **kw)  # warm-up
    wall, infos = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = p.piece_sweep(0, frames, **kw)
        wall.append(1e3 * (time.perf_counter() - t0))
        infos.append(r.info)
    out = dict(settings=len(r.settings), frames=frames, wall_ms=spread(wall))
    for name in ("hough_ms", "eval_ms"):
        out[name] = spread([i[name] for i in infos])
        out[name.replace("_ms", "_us_per_frame")] = {n: 1e3 * v / frames for n, v in out[name].items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-settings", type=int, default=24)
    ap.add_argument("--coarse-step", type=int, default=5, help="the coarse radius grid takes every n-th trackbar position")
    ap.add_argument("--budget-s", type=float, default=400, help="sweep legs whose projected time does not fit are left out and reported as not measured")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from chessboard_vision_amd import synth as S
    from chessboard_vision_amd.stream import BoardPipeline, piece_trackbar_grid
    pts = S.scaled_corners(W, H)
    lo, hi = piece_trackbar_grid()
    p = BoardPipeline(W, H, a.frames)
    p.configure(pts, enhance=False)
    p.synth(0, a.frames, scene="normal", frames_per_ply=32)
    run_clip(p, a.frames)
    p.results(0, a.frames)
    out = {}
    coarse = dict(min_radius_ratios=lo[a.coarse_step - 1::a.coarse_step], max_radius_ratios=hi[a.coarse_step - 1::a.coarse_step])
    legs = (("param2 1..100", dict(min_radius_ratios=[.20], max_radius_ratios=[.55], param2s=range(1, 101)), False),
            ("param2 1..100, records=False", dict(min_radius_ratios=[.20], max_radius_ratios=[.55], param2s=range(1, 101), records=False), False),
            ("every %dth radius position" % a.coarse_step, coarse, False),
            ("full grid", dict(min_radius_ratios=lo, max_radius_ratios=hi), True),
            ("full grid, records=False", dict(min_radius_ratios=lo, max_radius_ratios=hi, records=False), True))
    t_begin = time.perf_counter()
    for name, kw, gated in legs:
        if gated:  # projected from the coarse grid's wall time per setting; a leg that would not fit the budget is left out
            c = out["every %dth radius position" % a.coarse_step]
            need = 1e-3 * c["wall_ms"]["median"] / c["settings"] * len(lo) * len(hi) * (a.reps + 1)
            left = a.budget_s - (time.perf_counter() - t_begin)
            if need > left:
                out[name] = dict(not_measured="projected %.0f s, %.0f s of the budget left" % (need, left))
                print("%-30s not measured: projected %.0f s for %d repetitions, %.0f s of --budget-s left" % (name, need, a.reps + 1, left), flush=True)
                continue
        out[name] = r = time_sweep(p, a.frames, a.reps, **kw)
        print("%-30s %5d settings x %d frames: hough %.1f ms (%.1f .. %.1f), eval %.2f ms (%.2f .. %.2f), wall %.1f ms (%.1f .. %.1f); per frame hough %.1f us, eval %.2f us"
              % (name, r["settings"], a.frames, r["hough_ms"]["median"], r["hough_ms"]["min"], r["hough_ms"]["max"], r["eval_ms"]["median"],
                 r["eval_ms"]["min"], r["eval_ms"]["max"], r["wall_ms"]["median"], r["wall_ms"]["min"], r["wall_ms"]["max"],
                 r["hough_us_per_frame"]["median"], r["eval_us_per_frame"]["median"]), flush=True)
    # the per-setting loop
    # The loop runs k_hough, whose radius histogram is sized from the ratios: a MaxRadius position whose int(min_dim * ratio)
    # is 0 on some square opens maxRadius to the square's larger side and overruns it.  Such pairs stay out.
    md = min(min(p._cfg.rois[i].w, p._cfg.rois[i].h) for i in range(len(p.rois_rc)))
    grid = [(a_, b_) for a_ in lo for b_ in hi if int(md * b_) > 0]
    sample = random.Random(1).sample(grid, a.loop_settings + 1)
    every = [set((f, r) for f in range(8) for r in range(8))] * a.frames
    per = []
    for i, (a_, b_) in enumerate(sample):  # (the first one is the warm-up: its configure allocates)
        p.ctx.synchronize()
        t0 = time.perf_counter()
        p.configure(pts, enhance=False, use_hough=2, min_radius_ratio=a_, max_radius_ratio=b_)
        p.reset_state()
        p.set_check_squares(0, every)
        run_clip(p, a.frames)
        p.results(0, a.frames)
        if i:
            per.append(1e3 * (time.perf_counter() - t0))
    out["loop_ms_per_setting"] = dict(spread(per), settings=len(per))
    ref_leg = "full grid" if "wall_ms" in out["full grid"] else "every %dth radius position" % a.coarse_step
    out["sweep_leg"] = ref_leg
    sweep_per = out[ref_leg]["wall_ms"]["median"] / out[ref_leg]["settings"]
    out["sweep_ms_per_setting"] = sweep_per
    out["ratio_per_setting"] = {n: out["loop_ms_per_setting"][n] / sweep_per for n in ("median", "min", "max")}
    print(("per-setting loop over %d settings: %.1f ms per setting (%.1f .. %.1f); the sweep (" + ref_leg + "): %.4f ms per setting; ratio %.1f (%.1f .. %.1f)")
          % (len(per), out["loop_ms_per_setting"]["median"], out["loop_ms_per_setting"]["min"], out["loop_ms_per_setting"]["max"], sweep_per,
             out["ratio_per_setting"]["median"], out["ratio_per_setting"]["min"], out["ratio_per_setting"]["max"]), flush=True)
    p.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
