"""What the profile-only pipeline mode and the colour profile sweep (cbv_pipeline_color_sweep) cost: 1080p, a clip of
--frames frames (512) resident, --reps repetitions (5), median and range.
  - k_warp_profile per frame beside k_warp and beside k_color_lab_hist (profile only) + k_warp, per kernel id (event pairs);
  - frames/s of enhance="profile" beside enhance=False and enhance=True, alternating in one session;
  - the sweep's wall time and its four stage times (cbv_color_sweep_info) for one trackbar axis (sat_scale, 301 profiles) and
    for a coordinate-descent round (the five scalar trackbars: 361 + 3 x 301 + 201 profiles); a probe of 16 profiles runs
    first, and a leg whose time projected from it does not fit --budget-s is reported as not measured;
  - this tree's own per-profile loop (configure + reset_state + set_check_squares + run + results) on a sample of profiles.

    python tools/color_sweep_timing.py [--frames N] [--reps N] [--loop-profiles M] [--budget-s S] [--json OUT]      (GPU box)
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
SHIPPED = {"hue_shift": -86, "sat_scale": 0.91, "val_scale": 2.46, "contrast": 1.48, "brightness": -30, "radical_mode": 0, "target_hue": 0,
           "hue_window": 26}


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def fmt(s, unit=""):
    return "%.4g%s (%.4g .. %.4g)" % (s["median"], unit, s["min"], s["max"])


def run_clip(p, frames):
    for s0 in range(0, frames, RUN):
        p.run(s0, min(RUN, frames - s0))


def kernel_us_per_frame(p, frames, reps, kids):
    """GPU time of the kernels `kids` per frame over a run of the clip"""
    out = []
    for _ in range(reps):
        p.ctx.profile_reset()
        p.ctx.profile_enable(-1)
        run_clip(p, frames)
        p.results(0, frames)
        out.append(1e3 * sum(p.ctx.profile_read(k)[0] for k in kids) / frames)
        p.ctx.profile_enable(-2)
    p.ctx.profile_reset()
    return spread(out)


def fps(p, frames):
    p.ctx.synchronize()
    t0 = time.perf_counter()
    run_clip(p, frames)
    p.results(0, frames)
    return frames / (time.perf_counter() - t0)


def time_sweep(p, frames, reps, profiles, **kw):
    wall, infos = [], []
    for i in range(reps + 1):  # (the first one is the warm-up)
        t0 = time.perf_counter()
        r = p.color_sweep(0, frames, profiles, **kw)
        if i:
            wall.append(1e3 * (time.perf_counter() - t0))
            infos.append(r.info)
    out = dict(profiles=len(profiles), frames=frames, wall_ms=spread(wall), chunk_frames=r.info["chunk_frames"], chunk_profiles=r.info["chunk_profiles"])
    for name in ("warp_ms", "squares_ms", "hough_ms", "eval_ms"):
        out[name] = spread([i_[name] for i_ in infos])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-profiles", type=int, default=24)
    ap.add_argument("--budget-s", type=float, default=300, help="sweep legs whose projected time does not fit are left out and reported as not measured")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd import synth as S
    from chessboard_vision_amd.stream import BoardPipeline, color_axis_profiles
    pts = S.scaled_corners(W, H)
    out = {}
    p = BoardPipeline(W, H, a.frames)
    modes = {"enhance=False": dict(enhance=False), 'enhance="profile"': dict(enhance="profile", profile=SHIPPED), "enhance=True": dict(enhance=True, profile=SHIPPED)}

    # 1. the warp kernels per frame
    for name, kids in (("enhance=False", ("WARP",)), ('enhance="profile"', ("WARP",)), ("enhance=True", ("WARP", "COLOR_LAB_HIST"))):
        p.configure(pts, **modes[name])
        p.synth(0, a.frames, scene="normal", frames_per_ply=32)
        run_clip(p, a.frames)
        for kid in kids:
            out["%s %s us/frame" % (name, kid)] = r = kernel_us_per_frame(p, a.frames, a.reps, (N.K_ALL[kid],))
            print("%-18s kernel id %-15s %s per frame" % (name, kid, fmt(r, " us")), flush=True)
    # k_color_lab_hist with do_profile only (one frame per launch: the stage entry point apply_color_profile), kernel time alone
    from chessboard_vision_amd.frame_enhancer import ImageEnhancerHIP
    enh = ImageEnhancerHIP()
    enh.profile = SHIPPED
    frame = p.download(0, 0)
    enh.apply_color_profile(frame)
    per = []
    for _ in range(a.reps):
        p.ctx.profile_reset()
        p.ctx.profile_enable(N.K_ALL["COLOR_LAB_HIST"])
        for _ in range(16):
            enh.apply_color_profile(frame)
        ms, n = p.ctx.profile_read(N.K_ALL["COLOR_LAB_HIST"])
        per.append(1e3 * ms / n)
        p.ctx.profile_enable(-2)
    p.ctx.profile_reset()
    out["k_color_lab_hist profile only us/frame"] = r = spread(per)
    print("k_color_lab_hist (profile only, one frame a launch) %s per frame" % fmt(r, " us"), flush=True)

    # 2. frames/s of the three modes, alternating
    rates = {name: [] for name in modes}
    for _ in range(a.reps):
        for name in modes:
            p.configure(pts, **modes[name])
            p.synth(0, a.frames, scene="normal", frames_per_ply=32)
            fps(p, a.frames)  # warm-up of this configuration
            rates[name].append(fps(p, a.frames))
    for name in modes:
        out["%s frames/s" % name] = r = spread(rates[name])
        print("%-18s %s frames/s" % (name, fmt(r)), flush=True)

    # 3. the sweep
    p.configure(pts, enhance=False)
    p.synth(0, a.frames, scene="normal", frames_per_ply=32)
    expected = [set(S.position_for_frame(i, 32).keys()) for i in range(a.frames)]
    axis = color_axis_profiles(SHIPPED, "sat_scale")
    round_ = [q for ax in ("hue_shift", "sat_scale", "val_scale", "contrast", "brightness") for q in color_axis_profiles(SHIPPED, ax)]
    t_begin = time.perf_counter()
    probe = time_sweep(p, a.frames, 1, axis[::20], expected=expected)
    out["probe"] = probe
    per_profile_s = 1e-3 * probe["wall_ms"]["median"] / probe["profiles"]
    print("probe: %d profiles x %d frames, wall %.1f ms" % (probe["profiles"], a.frames, probe["wall_ms"]["median"]), flush=True)
    for name, profs, kw in (("one axis (sat_scale)", axis, {}), ("one axis, records=False", axis, dict(records=False)), ("coordinate-descent round", round_, {})):
        need, left = per_profile_s * len(profs) * (a.reps + 1), a.budget_s - (time.perf_counter() - t_begin)
        reps = a.reps
        if need > left:
            reps = int(left / (per_profile_s * len(profs))) - 1
            if reps < 1:
                out[name] = dict(not_measured="projected %.0f s, %.0f s of the budget left" % (need, left))
                print("%-28s not measured: projected %.0f s, %.0f s of --budget-s left" % (name, need, left), flush=True)
                continue
        out[name] = r = time_sweep(p, a.frames, reps, profs, expected=expected, **kw)
        r["reps"] = reps
        print("%-28s %5d profiles x %d frames (%d reps, chunks %d x %d): wall %s ms; warp %s, squares %s, hough %s, eval %s ms; %.3f ms per profile"
              % (name, r["profiles"], a.frames, reps, r["chunk_profiles"], r["chunk_frames"], fmt(r["wall_ms"]), fmt(r["warp_ms"]), fmt(r["squares_ms"]),
                 fmt(r["hough_ms"]), fmt(r["eval_ms"]), r["wall_ms"]["median"] / r["profiles"]), flush=True)

    # 4. the per-profile loop
    sample = random.Random(1).sample(round_, a.loop_profiles + 1)
    every = [set((f, r) for f in range(8) for r in range(8))] * a.frames
    per = []
    for i, prof in enumerate(sample):  # (the first one is the warm-up: its configure allocates)
        p.ctx.synchronize()
        t0 = time.perf_counter()
        p.configure(pts, enhance="profile", profile=prof, use_hough=2)
        p.reset_state()
        p.set_check_squares(0, every)
        run_clip(p, a.frames)
        p.results(0, a.frames)
        if i:
            per.append(1e3 * (time.perf_counter() - t0))
    out["loop_ms_per_profile"] = r = dict(spread(per), profiles=len(per))
    print("per-profile loop over %d profiles (frames already resident): %s ms per profile" % (len(per), fmt(r)), flush=True)
    p.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
