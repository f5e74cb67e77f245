"""Several boards per camera frame, measured: K = 1, 2, 4 boards attached to ONE pipeline (each frame uploaded and
enhanced once) against the same K boards as K independent pipelines on the same frames, at 1080p and 4K with 512
frames in flight (4 runs of 128 frames, as bench.py enqueues a step), with enhance_region off and on.

The boards do not overlap: K = 1 is the calibration quad over the whole frame, K = 2 one board in each half, K = 4 one in
each quarter.  The frames are composites of device-rendered boards (synth), one board per part of the frame.  Prints
frames/s and boards/s per row, and the one-frame latency (run + results of a single frame, wall time) of the one
pipeline with K = 1 and K = 4.

    python tools/multiboard_timing.py [--reps N] [--json OUT]      (GPU box)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chessboard_vision_amd import synth as S  # noqa: E402
from chessboard_vision_amd.stream import BoardPipeline  # noqa: E402

FRAMES, RUN, DISTINCT = 512, 128, 8


def layout(w, h, k):
    """[(quad, (x0, y0, x1, y1) = the part of the frame the board is rendered into)] for K boards."""
    if k == 1:
        return [(S.scaled_corners(w, h), (0, 0, w, h))]
    cols, rows = (2, 1) if k == 2 else (2, 2)
    cw, ch = w // cols, h // rows
    return [(S.scaled_corners(cw, ch) + np.float32([c * cw, r * ch]), (c * cw, r * ch, (c + 1) * cw, (r + 1) * ch))
            for r in range(rows) for c in range(cols)]


def frames_for(w, h, lay):
    """DISTINCT composite frames: board i (its own game, stream i) rendered into its part of the frame."""
    out = np.zeros((DISTINCT, h, w, 3), np.uint8)
    r = BoardPipeline(w, h, DISTINCT)
    r.configure(S.scaled_corners(w, h))
    for i, (quad, (x0, y0, x1, y1)) in enumerate(lay):
        r.synth(0, DISTINCT, stream_id=i, frame0=16 * i, points=quad)
        for t in range(DISTINCT):
            out[t, y0:y1, x0:x1] = r.download(0, t)[y0:y1, x0:x1]
    r.close()
    return out


def ring(w, h, frames):
    p = BoardPipeline(w, h, FRAMES)
    for s in range(FRAMES):
        p.upload(s, frames[s % DISTINCT])
    return p


def step(pipes):
    for s0 in range(0, FRAMES, RUN):
        for p in pipes:
            p.run(s0, RUN)
    for p in pipes:
        p.results(0, FRAMES)


def timed(pipes, reps):
    step(pipes)  # warm-up
    t = []
    for _ in range(reps):
        pipes[0].ctx.synchronize()
        t0 = time.perf_counter()
        step(pipes)
        t.append(time.perf_counter() - t0)
    return FRAMES / float(np.median(t))


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    print("%-6s %-6s %2s %-12s %10s %10s %9s" % ("size", "region", "K", "layout", "frames/s", "boards/s", "1-frame"))
    for (w, h) in ((1920, 1080), (3840, 2160)):
        for k in (1, 2, 4):
            lay = layout(w, h, k)
            frames = frames_for(w, h, lay)
            one = ring(w, h, frames)
            pipes = [ring(w, h, frames) for _ in lay] if k > 1 else []
            for region in (False, True):
                kw = dict(profile=S.SHIPPED_PROFILE, enhance_region=region)
                one.configure(lay[0][0], **kw)
                boards = [one.add_board(q) for q, _ in lay[1:]]
                fps = timed([one], a.reps)
                row = dict(size="%dp" % h, region=region, K=k, layout="one pipeline", fps=fps, boards_per_s=fps * k)
                if h == 1080 and k in (1, 4):
                    row["latency_ms"] = latency(one)
                rows.append(row)
                for b in boards:
                    b.close()
                if pipes:
                    for p, (q, _) in zip(pipes, lay):
                        p.configure(q, **kw)
                    fps = timed(pipes, a.reps)
                    rows.append(dict(size="%dp" % h, region=region, K=k, layout="K pipelines", fps=fps, boards_per_s=fps * k))
                for r in rows[-2 if pipes else -1:]:
                    print("%-6s %-6s %2d %-12s %10.0f %10.0f %9s" % (r["size"], "on" if r["region"] else "off", r["K"], r["layout"],
                                                                   r["fps"], r["boards_per_s"],
                                                                   "%.3f ms" % r["latency_ms"] if "latency_ms" in r else ""))
                sys.stdout.flush()
            one.close()
            for p in pipes:
                p.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
