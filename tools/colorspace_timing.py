"""What a colour space other than "bt601" costs (include/cbv.h, CBV_CS_*): the runtime-matrix kernels against their
compile-time siblings at 1080p on one GPU, in one session with the colour spaces alternating, --rounds rounds (5), median
and range per frame:
  - k_ingest against k_ingest_cs: the event pairs around the launches of `submit` (cbv_profile_*), 64 frames a submit;
  - k_warp_yuv against k_warp_yuv_cs (the four-frames form; planar 4:2:0: two frames in the _cs form): the event pairs
    around the warp's launches inside p.run of a raw-mode pipeline (enhance=False), one lane;
  - a raw-mode run (enhance=False, two lanes): wall-clock of run + results on the same resident frames in "bt601" and in
    "bt709".
The frames are one synthetic frame turned into the layout (synth.bgr_to_yuv) and repeated; the same bytes serve both colour
spaces: the kernels' work does not depend on the values.

    python tools/colorspace_timing.py [--formats nv12,yuyv] [--rounds 5] [--frames 64] [--json OUT]         (GPU box)
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
SPACES = ("bt601", "bt709")


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def show(s):
    return "%.3f (%.3f .. %.3f)" % (s["median"], s["min"], s["max"])


def pipeline(fmt, cs, n, raw_frame, lanes, **mode):
    p = BoardPipeline(W, H, n)
    p.configure(S.scaled_corners(W, H), profile=None, chunk=16, lanes=lanes, **mode)
    p.set_input_format(fmt, colorspace=cs)
    ring = p.host_ring()
    for i in range(n):
        ring[i] = raw_frame
    p.submit(0, n)
    p.wait_submitted()
    return p


def kernel_us(ctx, kid, n, work, reps):
    ctx.profile_reset()
    ctx.profile_enable(kid)
    for _ in range(reps):
        work()
    ms, launches = ctx.profile_read(kid)
    ctx.profile_enable(-2)
    return ms * 1e3 / (reps * n), launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--formats", default="nv12,yuyv,yuv420p")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--json")
    args = ap.parse_args()
    n = args.frames
    ctx = N.context()
    probe = BoardPipeline(W, H, 1)
    probe.synth(0, 1)
    bgr = probe.download(0, 0)
    probe.close()
    out = {"size": [W, H], "frames": n, "rounds": args.rounds, "device": ctx.name}
    for fmt in args.formats.split(","):
        raw = S.bgr_to_yuv(bgr, fmt)
        ing = {cs: pipeline(fmt, cs, n, raw, 2) for cs in SPACES}                       # enhancement on: submit converts
        one = {cs: pipeline(fmt, cs, n, raw, 1, enhance=False) for cs in SPACES}        # raw mode, one lane: the warp's kernel
        two = {cs: pipeline(fmt, cs, n, raw, 2, enhance=False) for cs in SPACES}        # raw mode as it is run
        for p in list(one.values()) + list(two.values()):                                # warm up
            p.run(0, n)
            p.results(0, n)
        seen = {(k, cs): [] for k in ("ingest_us", "warp_us", "run_us") for cs in SPACES}
        for rnd in range(args.rounds):
            for cs in SPACES:
                p = ing[cs]

                def submit(p=p):
                    p.submit(0, n)
                    p.wait_submitted()
                seen["ingest_us", cs].append(kernel_us(ctx, N.K_ALL["INGEST"], n, submit, 5)[0])
                p = one[cs]

                def run(p=p):
                    p.run(0, n)
                    p.results(0, n)
                seen["warp_us", cs].append(kernel_us(ctx, N.K_ALL["WARP_YUV"], n, run, 3)[0])
                p = two[cs]
                t0 = time.perf_counter()
                for _ in range(3):
                    p.run(0, n)
                    p.results(0, n)
                seen["run_us", cs].append((time.perf_counter() - t0) * 1e6 / (3 * n))
        res = out[fmt] = {k: {cs: spread(seen[k, cs]) for cs in SPACES} for k in ("ingest_us", "warp_us", "run_us")}
        for k, what in (("ingest_us", "k_ingest / k_ingest_cs"), ("warp_us", "k_warp_yuv / k_warp_yuv_cs"), ("run_us", "raw-mode run + results")):
            print("%-8s %-28s us/frame: bt601 %s   bt709 %s" % (fmt, what, show(res[k]["bt601"]), show(res[k]["bt709"])), flush=True)
        for p in list(ing.values()) + list(one.values()) + list(two.values()):
            p.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
