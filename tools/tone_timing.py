"""What the piece-tone stage (k_piece_tone; include/cbv.h "piece colour per square") costs.
Prints ONE JSON object per configuration (1080p, enhance=False, 512 resident frames, one and four boards):

  tone_us_per_frame   k_piece_tone's time per frame from the profile counters (cbv_profile_read event pairs around the
                      two launches of each chunk: the sums of all boards, then their records), `--rounds` rounds
  warp_us_per_frame   the warp's, the same way, beside it
  fps_off / fps_on    frames/s of steps of 512 frames with the tones off and on, alternating in the same session
                      (median, min and max of `--reps` steps each)

    python tools/tone_timing.py [--frames 512] [--reps 7] [--rounds 3] [--boards 1,4] [--chunk 16]      (GPU box)
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


def spread(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def profiled(ctx, kid, fn):
    ctx.profile_reset()
    ctx.profile_enable(kid)
    try:
        fn()
        ctx.synchronize()
        return ctx.profile_read(kid)
    finally:
        ctx.profile_enable(-2)
        ctx.profile_reset()


def step_seconds(p, frames):
    p.ctx.synchronize()
    t0 = time.perf_counter()
    p.run(0, frames)
    p.results(0, frames)
    return time.perf_counter() - t0


def measure(nboards, frames, reps, rounds, chunk):
    w, h = 1920, 1080
    pts = S.scaled_corners(w, h)
    p = BoardPipeline(w, h, frames)
    p.configure(pts, enhance=False, chunk=chunk, use_hough=False)
    boards = [p] + [p.add_board(pts + np.float32(2 * i)) for i in range(1, nboards)]
    p.synth(0, frames, scene="normal", frames_per_ply=32)
    p.run(0, frames)
    models = []
    for b in boards:
        rep = b.calibrate_tones(0)
        assert not rep["misclassified"] and not rep["undecided"], rep
        models.append(b.tone_model)

    def tones(on):
        for b, m in zip(boards, models):
            b.set_tones(m if on else None)

    step_seconds(p, frames)  # warm
    tone_us, warp_us = [], []
    for _ in range(rounds):
        ms, n = profiled(p.ctx, N.K_TONE, lambda: p.run(0, frames))
        assert n == (frames + chunk - 1) // chunk, n
        tone_us.append(1e3 * ms / frames)
        ms, n = profiled(p.ctx, N.K["WARP"], lambda: p.run(0, frames))
        warp_us.append(1e3 * ms / frames)
    fps = {False: [], True: []}
    for _ in range(reps):
        for on in (False, True):
            tones(on)
            step_seconds(p, frames)  # (the first step behind a switch rebuilds nothing, but keep the pairs alike)
            fps[on].append(frames / step_seconds(p, frames))
    p.close()
    return dict(boards=nboards, frames=frames, chunk=chunk, size="1080p", tone_us_per_frame=spread(tone_us), warp_us_per_frame=spread(warp_us),
                fps_off=spread(fps[False]), fps_on=spread(fps[True]), fps_on_over_off=float(np.median(fps[True]) / np.median(fps[False])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--boards", default="1,4")
    ap.add_argument("--chunk", type=int, default=16)
    a = ap.parse_args()
    for k in (int(x) for x in a.boards.split(",")):
        print(json.dumps(measure(k, a.frames, a.reps, a.rounds, a.chunk)), flush=True)


if __name__ == "__main__":
    main()
