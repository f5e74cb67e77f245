"""What a ChangeDetector blur kernel of its own (cbv_pipeline_set_change_blur) costs: frames/s of the bench's 1080p workload
(512 frames resident, 4 runs of 128, every board calibrated on frame 0) with k = 5 (the board as it always was: the new
kernel does not run) and k = 3, 13, 31, with 1 board and with 4 boards on one pipeline, with and without enhancement
(`enhance=False`: the session's chain, where the per-square stages are most of the work), with the model frozen (the new
kernel also takes the z-score statistics) and updated after every frame (it only writes the planes); and the time of
k_change_blur_stats per frame (cbv_profile_read, a pass of its own: the event pairs cost time).

    python tools/change_blur_timing.py [--reps N] [--json OUT]      (GPU box)
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
KERNELS = (5, 3, 13, 31)
MODES = ("frozen", "every")


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
    """k_change_blur_stats' time per frame over one step, from the library's event pairs"""
    ctx = p.ctx
    ctx.profile_reset()
    ctx.profile_enable(N.K_CHANGE_BLUR)
    try:
        step(p)
        ms, launches = ctx.profile_read(N.K_CHANGE_BLUR)
    finally:
        ctx.profile_enable(-2)
        ctx.profile_reset()
    return 1e3 * ms / FRAMES, launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    print("%-7s %-8s %-7s %3s %10s %8s %14s %9s" % ("boards", "enhance", "mode", "k", "frames/s", "vs k=5", "blur us/frame", "launches"))
    pts = S.scaled_corners(W, H)
    for nb in (1, 4):
        for enhance in (True, False):
            p = BoardPipeline(W, H, FRAMES)
            p.configure(pts, profile=S.SHIPPED_PROFILE, enhance=enhance)
            boards = [p] + [p.add_board(pts + np.float32(2 * i)) for i in range(1, nb)]
            p.synth(0, FRAMES, scene="normal", frames_per_ply=32)
            for mode in MODES:
                base = None
                for k in KERNELS:
                    for b in boards:
                        b.set_model_update("frozen")
                        b.set_change_blur(k)
                    p.run(0, 1)
                    for b in boards:
                        b.calibrate_changes(0)
                        b.set_model_update(mode, 0.13)
                        b.reset_state()
                    fps = timed(p, a.reps)
                    us, launches = kernel_us_per_frame(p)
                    base = fps if k == 5 else base
                    row = dict(boards=nb, enhance=enhance, mode=mode, k=k, fps=fps, rel=fps / base, blur_us_per_frame=us, blur_launches=launches)
                    rows.append(row)
                    print("%-7d %-8s %-7s %3d %10.0f %7.1f%% %14.2f %9d" % (nb, enhance, mode, k, fps, 100 * (fps / base - 1), us, launches))
                    sys.stdout.flush()
            p.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
