"""Developed mosaics (include/cbv.h: 10/12/16-bit and MIPI-packed Bayer frames, per-colour tables) timed beside their yardsticks in
ONE process: the 8-bit Bayer mosaic and NV12.  Three parts, each alternating the formats round by round so that every figure
stands beside its counterpart of the same session, every round printed, then min / median / max:

  ingest   microseconds per frame of the conversion kernel alone (k_ingest / k_ingest_deep), from the library's event pairs
           around the launches of cbv_pipeline_submit, at 1080p and 4K
  warp     microseconds per frame of the warp alone in raw mode (plain, through a lens, with the profile on the raw taps), from
           the event pairs around the launches of cbv_pipeline_run
  fed      host-fed frames per second: submit of one half of the ring overlapped with the run of the other, wall clock, and the
           ratio to the 8-bit mosaic beside what the byte counts alone predict (0.80 / 0.67 / 0.50 if the link is the limit)

The container is measured with a 12-bit table (staged in LDS) and with a 16-bit table (read from global memory).

    python tools/bayer_deep_timing.py [--rounds 3] [--parts ingest,warp,fed] [--sizes 1080p,4k]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from chessboard_vision_amd import _native as N  # noqa: E402
from chessboard_vision_amd import synth as S  # noqa: E402
from chessboard_vision_amd.stream import BoardPipeline, Develop, Lens  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--parts", default="ingest,warp,fed")
ap.add_argument("--sizes", default="1080p,4k")
args = ap.parse_args()
parts = args.parts.split(",")
SIZES = {"1080p": (1920, 1080, 32), "4k": (3840, 2160, 8)}

# name -> (format, develop or None)
CASES = {"nv12": ("nv12", None), "bayer8": ("bayer_rggb", None), "bayer8+table": ("bayer_rggb", Develop(8, gamma=2.2)),
         "10p": ("bayer_rggb10p", Develop(10, black_level=64, gains=(1.9, 1, 1.5), gamma=2.2)),
         "12p": ("bayer_rggb12p", Develop(12, black_level=256, gains=(1.9, 1, 1.5), gamma=2.2)),
         "16/12-bit table": ("bayer_rggb16", Develop(12, black_level=256, gains=(1.9, 1, 1.5), gamma=2.2)),
         "16/16-bit table": ("bayer_rggb16", Develop(16, black_level=4096, gains=(1.9, 1, 1.5), gamma=2.2))}
ctx = N.context()
rng = np.random.default_rng(0)


def fill(p, dev):
    """one random frame in every slot of the host ring (samples below the table's size)"""
    ring = p.host_ring()
    if ring.dtype == np.uint16:
        ring[0] = rng.integers(0, 1 << dev.bits, ring[0].shape, dtype=np.uint16)
    else:
        ring[0] = rng.integers(0, 256, ring[0].shape, dtype=np.uint8)
    for i in range(1, p.max_frames):
        ring[i] = ring[0]


def make(name, w, h, n, **cfg):
    fmt, dev = CASES[name]
    p = BoardPipeline(w, h, n)
    if cfg:
        p.configure(S.scaled_corners(w, h), **cfg)
    p.set_input_format(fmt, develop=dev) if N.is_bayer(fmt) else p.set_input_format(fmt)
    fill(p, dev)
    p.submit(0, n)
    p.wait_submitted()
    return p


def kernel_us(p, kids, fn, frames):
    """microseconds per frame that the kernels `kids` took inside fn()"""
    ctx.profile_reset()
    ctx.profile_enable(-1)
    fn()
    got = [ctx.profile_read(k) for k in kids]
    ctx.profile_enable(-2)
    ms, launches = sum(g[0] for g in got), sum(g[1] for g in got)
    assert launches, "none of the kernels %s was launched" % (kids,)
    return ms * 1e3 / frames


def report(title, seen):
    for name, v in seen.items():
        print("%-34s %-16s min %8.2f  median %8.2f  max %8.2f over %d rounds" % (title, name, min(v), float(np.median(v)), max(v), len(v)), flush=True)


for size in args.sizes.split(","):
    w, h, n = SIZES[size]
    if "ingest" in parts:
        pipes = {name: make(name, w, h, n) for name in CASES}
        seen = {name: [] for name in CASES}
        for rnd in range(args.rounds):
            for name, p in pipes.items():
                reps = 5

                def submits(p=p):
                    for _ in range(reps):
                        p.submit(0, n)
                    p.wait_submitted()
                us = kernel_us(p, (N.K["INGEST"], N.K_INGEST_BAYER_DEEP), submits, reps * n)
                seen[name].append(us)
                print("ingest %s %-16s round %d: %8.2f us/frame (%d B in, %d B out)" % (size, name, rnd + 1, us, p.host_ring()[0].nbytes, w * h * 3), flush=True)
        report("ingest %s us/frame" % size, seen)
        for p in pipes.values():
            p.close()
    if "warp" in parts:
        lens = Lens(0.9 * w, 0.9 * w, w / 2, h / 2, -0.25, 0.08, 0.001, -0.0005, 0.0)
        for mode, cfg in (("plain", dict(enhance=False)), ("lens", dict(enhance=False, lens=lens)),
                          ("profile", dict(enhance="profile", raw=True, profile=S.SHIPPED_PROFILE))):
            pipes = {name: make(name, w, h, n, lanes=1, use_hough=0, **cfg) for name in CASES}
            seen = {name: [] for name in CASES}
            for p in pipes.values():
                p.run(0, n)
                p.results(0, n)
            for rnd in range(args.rounds):
                for name, p in pipes.items():
                    reps = 5

                    def runs(p=p):
                        for _ in range(reps):
                            p.run(0, n)
                        p.results(0, n)
                    us = kernel_us(p, (N.K_WARP_YUV, N.K_WARP_BAYER_DEEP), runs, reps * n)
                    seen[name].append(us)
                    print("warp/%s %s %-16s round %d: %8.2f us/frame" % (mode, size, name, rnd + 1, us), flush=True)
            report("warp/%s %s us/frame" % (mode, size), seen)
            for p in pipes.values():
                p.close()
    if "fed" in parts:
        pipes = {name: make(name, w, h, n, enhance=False) for name in CASES}
        seen = {name: [] for name in CASES}
        half = n // 2
        for rnd in range(args.rounds):
            for name, p in pipes.items():
                p.submit(0, half)
                p.wait_submitted()
                loops = 6
                t0 = time.perf_counter()
                for i in range(loops):
                    a, b = (0, half) if i % 2 == 0 else (half, 0)
                    p.submit(b, half)      # the other half crosses the link ...
                    p.run(a, half)         # ... while this half is warped and judged
                    p.results(a, half)
                    p.wait_submitted()
                dt = time.perf_counter() - t0
                fps = loops * half / dt
                seen[name].append(fps)
                print("fed %s %-16s round %d: %9.1f frames/s (%d B a frame, %.2f GB/s over the link)"
                      % (size, name, rnd + 1, fps, p.host_ring()[0].nbytes, fps * p.host_ring()[0].nbytes / 1e9), flush=True)
        report("fed %s frames/s" % size, seen)
        base = float(np.median(seen["bayer8"]))
        for name, p in pipes.items():
            print("fed %s %-16s median / bayer8 median = %.2f; by bytes alone %.2f"
                  % (size, name, float(np.median(seen[name])) / base, pipes["bayer8"].host_ring()[0].nbytes / p.host_ring()[0].nbytes), flush=True)
        for p in pipes.values():
            p.close()
