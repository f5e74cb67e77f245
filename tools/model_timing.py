"""What the per-frame model update (cbv_pipeline_set_model_update) costs: frames/s of the bench's 1080p workload (512
frames in flight as 4 runs of 128, shipped profile, every board calibrated on frame 0) with the model frozen, updated
after every frame, and updated on the unchanged squares, with 1 board and with 4 boards on one pipeline; the time of
k_model_scan per frame (cbv_profile_read, a pass of its own: the event pairs cost time); and the one-frame latency
(run + results of a single frame, wall time) in each mode.

    python tools/model_timing.py [--reps N] [--json OUT]      (GPU box)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chessboard_vision_amd import _native as N  # noqa: E402
from chessboard_vision_amd import synth as S  # noqa: E402
from chessboard_vision_amd.stream import BoardPipeline  # noqa: E402

W, H = 1920, 1080
FRAMES, RUN = 512, 128
MODES = ("frozen", "every", "unchanged")


def step(p):
    for s0 in range(0, FRAMES, RUN):
        p.run(s0, RUN)
    p.results(0, FRAMES)


def timed(p, reps):
    step(p)  # warm-up
    t = []
    for _ in range(reps):
        p.ctx.synchronize()
        t0 = time.perf_counter()
        step(p)
        t.append(time.perf_counter() - t0)
    return FRAMES / float(np.median(t))


def kernel_us_per_frame(p):
    """k_model_scan's time per frame (and board launch) over one step, from the library's event pairs"""
    ctx = p.ctx
    ctx.profile_reset()
    ctx.profile_enable(N.K["MODEL_SCAN"])
    try:
        step(p)
        ms, launches = ctx.profile_read(N.K["MODEL_SCAN"])
    finally:
        ctx.profile_enable(-2)
        ctx.profile_reset()
    return 1e3 * ms / FRAMES, launches


def latency(p, n=300):
    t = []
    for i in range(n):
        s = i % FRAMES
        t0 = time.perf_counter()
        p.run(s, 1)
        p.results(s, 1)
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t[30:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    print("%-7s %-10s %10s %14s %9s %10s" % ("boards", "mode", "frames/s", "scan us/frame", "launches", "1-frame"))
    for k in (1, 4):
        p = BoardPipeline(W, H, FRAMES)
        pts = S.scaled_corners(W, H)
        p.configure(pts, profile=S.SHIPPED_PROFILE)
        boards = [p] + [p.add_board(pts + np.float32(2 * i)) for i in range(1, k)]
        p.synth(0, FRAMES, scene="normal", frames_per_ply=32)
        p.run(0, 1)
        for b in boards:
            b.calibrate_changes(0)
        for mode in MODES:
            for b in boards:
                b.set_model_update(mode, 0.1)
                b.reset_state()
            fps = timed(p, a.reps)
            us, launches = kernel_us_per_frame(p)
            row = dict(boards=k, mode=mode, fps=fps, scan_us_per_frame=us, scan_launches=launches, latency_ms=latency(p))
            rows.append(row)
            print("%-7d %-10s %10.0f %14.2f %9d %7.3f ms" % (k, mode, fps, us, launches, row["latency_ms"]))
            sys.stdout.flush()
        p.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
