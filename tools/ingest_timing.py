"""PCIe-inclusive throughput of the ingest front end (never bench.py's `value`): 1080p frames sit in the pinned
host ring; batch k+1 is copied (cbv_pipeline_submit) while batch k runs.  Prints H2D-only, compute-only and
overlapped rates per input format, all from one process:

    python tools/ingest_timing.py --format all --reps 3

With a YUV format ("nv12", "nv21", "yuv420p", "yv12", "yuyv", "yvyu", "uyvy") or a Bayer format ("bayer_rggb",
"bayer_bggr", "bayer_grbg", "bayer_gbrg": the frames sampled to a mosaic, synth.bayer_mosaic) the ring holds raw frames (BoardPipeline.set_input_format) and a submit is the copy plus the
conversion kernel; "H2D only" then includes that kernel.  `--reps` alternates the formats and prints every repetition
and, for each format, the ratio to BGR of the same repetition."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from chessboard_vision_amd import _native as N  # noqa: E402
from chessboard_vision_amd import synth as S  # noqa: E402
from chessboard_vision_amd.stream import BoardPipeline  # noqa: E402

ap = argparse.ArgumentParser()
ALL = list(N.FORMATS) + list(N.BAYER_FORMATS)
ap.add_argument("--format", default="bgr", help="one of %s, a comma-separated list of them, or all" % ", ".join(ALL))
ap.add_argument("--reps", type=int, default=1)
args = ap.parse_args()
formats = ALL if args.format == "all" else args.format.split(",")
for f in formats:
    N.format_id(f)

W, H, HALF, ROUNDS = 1920, 1080, 128, 6
n = 2 * HALF
p = BoardPipeline(W, H, n)
p.configure(S.scaled_corners(W, H), profile=S.SHIPPED_PROFILE, grid_lines=(S.CALIB_GRID_X, S.CALIB_GRID_Y), **S.SHIPPED_DETECTOR)
p.synth(0, n, scene="dim")
bgr = [p.download(0, i) for i in range(n)]


def to_raw(f, fmt):
    """a camera-native frame of a BGR one (float BT.601 forward transform, chroma of the first pixel of each block)"""
    if fmt == "bgr":
        return f
    if fmt in N.BAYER_FORMATS:
        return S.bayer_mosaic(f, fmt)
    b, g, r = (f[..., i].astype(np.float32) for i in range(3))
    q = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    y, u, v = q(16 + 0.257 * r + 0.504 * g + 0.098 * b), q(128 - 0.148 * r - 0.291 * g + 0.439 * b), q(128 + 0.439 * r - 0.368 * g - 0.071 * b)
    if fmt in N.FORMATS_420:
        c = (u[::2, ::2], v[::2, ::2]) if fmt in ("nv12", "yuv420p") else (v[::2, ::2], u[::2, ::2])
        chroma = np.stack(c, axis=-1) if fmt in ("nv12", "nv21") else np.stack(c)  # interleaved pairs, or one plane after the other
        return np.concatenate([y, chroma.reshape(H // 2, W)])
    first, second = (u[:, ::2], v[:, ::2]) if fmt != "yvyu" else (v[:, ::2], u[:, ::2])
    out = np.empty((H, W, 2), np.uint8)
    yb, cb = (1, 0) if fmt == "uyvy" else (0, 1)   # UYVY carries the chroma byte first
    out[..., yb], out[:, 0::2, cb], out[:, 1::2, cb] = y, first, second
    return out


def sync():
    p.ctx.check(p.ctx.lib.cbv_ctx_synchronize(p.ctx.h))
    p.wait_submitted()
    p.results(0, 1)


def measure(fmt):
    p.set_input_format(fmt)
    ring = p.host_ring()
    for i in range(n):
        ring[i] = raw[fmt][i]
    p.submit(0, n)
    p.run(0, n)
    sync()
    # H2D only (+ the conversion of a YUV or Bayer format)
    t0 = time.perf_counter()
    for r in range(ROUNDS):
        p.submit(0, HALF)
        p.submit(HALF, HALF)
    p.run(0, 1)
    sync()
    t_copy = time.perf_counter() - t0
    # compute only
    t0 = time.perf_counter()
    for r in range(ROUNDS):
        p.run(0, HALF)
        p.run(HALF, HALF)
    sync()
    t_run = time.perf_counter() - t0
    # overlapped: submit the other half, run this half
    p.submit(0, HALF)
    t0 = time.perf_counter()
    for r in range(ROUNDS):
        p.submit(HALF, HALF)
        p.run(0, HALF)
        p.submit(0, HALF)
        p.run(HALF, HALF)
    sync()
    t_ovl = time.perf_counter() - t0
    frames = ROUNDS * n
    gb = frames * raw[fmt][0].size / 1e9
    return frames / t_copy, gb / t_copy, frames / t_run, frames / t_ovl


raw = {fmt: [to_raw(f, fmt) for f in bgr[:8]] * (n // 8) for fmt in formats}
for rep in range(args.reps):
    got = {fmt: measure(fmt) for fmt in formats}
    for fmt in formats:
        c, gbs, r, o = got[fmt]
        tag = "[%s, rep %d] " % (fmt, rep + 1)
        print(tag + "H2D only      : %8.0f frames/s  (%.1f GB/s)" % (c, gbs))
        print(tag + "compute only  : %8.0f frames/s" % r)
        print(tag + "submit || run : %8.0f frames/s  (PCIe-inclusive)" % o)
        if fmt != "bgr" and "bgr" in got:
            print(tag + "ratio to bgr  : H2D only %.3f, submit || run %.3f" % (c / got["bgr"][0], o / got["bgr"][3]), flush=True)
p.close()
