"""k_ingest on its own: microseconds per frame and achieved bytes/s (raw bytes read + BGR bytes written) at 1080p and
4K per format (the YUV layouts and the four 8-bit Bayer mosaics), from the library's event pairs around the launches of cbv_pipeline_submit (cbv_profile_*).  Each submit
converts a batch whose frames (raw + BGR, 530 MB and more) do not fit the 256 MiB Infinity Cache.  `--rounds` alternates
the formats, so that a layout and its sibling (NV21, yuv420p, YV12 beside NV12; YVYU, UYVY beside YUYV) are measured in
the same session; every round is printed, then min / median / max per format.

    python tools/ingest_kernel_timing.py [--formats nv12,yuv420p] [--rounds 3]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from chessboard_vision_amd import _native as N  # noqa: E402
from chessboard_vision_amd.stream import BoardPipeline  # noqa: E402

ALL = [f for f in N.FORMATS if f != "bgr"] + list(N.BAYER_FORMATS)
ap = argparse.ArgumentParser()
ap.add_argument("--formats", default=",".join(ALL))
ap.add_argument("--rounds", type=int, default=1)
args = ap.parse_args()
formats = args.formats.split(",")

HBM_GBPS = 8000.0  # the peak the other roofline rows of DESIGN.md use
ctx = N.context()
rng = np.random.default_rng(0)
for (w, h, n) in ((1920, 1080, 64), (3840, 2160, 16)):
    pipes = {}
    for fmt in formats:
        p = pipes[fmt] = BoardPipeline(w, h, n)
        p.set_input_format(fmt)
        ring = p.host_ring()
        ring[0] = rng.integers(0, 256, ring[0].shape, dtype=np.uint8)
        for i in range(1, n):
            ring[i] = ring[0]
        p.submit(0, n)
        p.wait_submitted()
    seen = {fmt: [] for fmt in formats}
    for rnd in range(args.rounds):
        for fmt in formats:
            p = pipes[fmt]
            ctx.profile_reset()
            ctx.profile_enable(N.K["INGEST"])
            for rep in range(10):
                p.submit(0, n)
            p.wait_submitted()
            ms, launches = ctx.profile_read(N.K["INGEST"])
            ctx.profile_enable(-2)
            us = ms * 1e3 / (launches * n)
            raw_bytes = p.host_ring()[0].size
            gbps = (raw_bytes + w * h * 3) / us / 1e3
            seen[fmt].append(us)
            print("%-10s %4dx%-4d round %d: %7.2f us/frame, %.0f GB/s (%d B read + %d B written per frame) = %.1f %% of %d GB/s; %d launches of %d frames"
                  % (fmt, w, h, rnd + 1, us, gbps, raw_bytes, w * h * 3, 100 * gbps / HBM_GBPS, HBM_GBPS, launches, n), flush=True)
    for fmt in formats:
        print("%-10s %4dx%-4d: min %.2f  median %.2f  max %.2f us/frame over %d rounds"
              % (fmt, w, h, min(seen[fmt]), float(np.median(seen[fmt])), max(seen[fmt]), args.rounds), flush=True)
        pipes[fmt].close()
