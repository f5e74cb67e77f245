"""What the warp's multi-board launch costs per source: per-frame GPU time of the warp (event pairs around every launch,
kernel ids WARP / WARP_YUV) on two-board pipelines at 1080p, 64 frames resident, chunks of 32 (the many-frames forms), one
lane, the lens off (k_warp_boards: `<row>_boards_us`) and on (k_warp_lens with two entries: `<row>_lens_us`) in turn on the
same pipeline; five repetitions, their median; both boards' warp per frame.  Rows: BGR, BGR with a profile, NV12, Bayer
RGGB, NV12 and YUV420P with a profile, NV12 and YUV420P in BT.709, and (with --jpeg) JPEG planes.  tools/multiboard_timing.py
measures whole runs with the enhancement, where the warp is a few percent; this is the warp alone.  Prints ONE JSON line.

    python tools/lens_timing.py --make-jpeg frame1080.jpg                        (anywhere)
    python tools/warp_boards_timing.py [--jpeg frame1080.jpg] [--json OUT]       (GPU box)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from chessboard_vision_amd import _native as N  # noqa: E402
from chessboard_vision_amd import synth as S  # noqa: E402
from chessboard_vision_amd.stream import BoardPipeline, Lens  # noqa: E402
from lens_timing import LENS_1080P, SHIPPED  # noqa: E402
from raw_profile_timing import raw_of  # noqa: E402

W, H, n, REPS = 1920, 1080, 64, 5
ROWS = {  # row -> (configure keywords, input format, colour space, kernel id)
    "bgr": (dict(enhance=False), "bgr", None, "WARP"),
    "bgr_profile": (dict(enhance="profile", profile=SHIPPED), "bgr", None, "WARP"),
    "nv12": (dict(enhance=False), "nv12", None, "WARP_YUV"),
    "bayer_rggb": (dict(enhance=False), "bayer_rggb", None, "WARP_YUV"),
    "nv12_profile": (dict(enhance="profile", raw=True, profile=SHIPPED), "nv12", None, "WARP_YUV"),
    "yuv420p_profile": (dict(enhance="profile", raw=True, profile=SHIPPED), "yuv420p", None, "WARP_YUV"),
    "nv12_bt709": (dict(enhance=False), "nv12", "bt709", "WARP_YUV"),
    "yuv420p_bt709": (dict(enhance=False), "yuv420p", "bt709", "WARP_YUV"),
    "mjpeg_planes": (dict(enhance=False), "mjpeg", None, "WARP_YUV"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jpeg", default=None, help="a 1080p JPEG frame (tools/lens_timing.py --make-jpeg); without it the mjpeg_planes row is left out")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    jpeg = open(a.jpeg, "rb").read() if a.jpeg else None
    pts = S.scaled_corners(W, H)
    src = BoardPipeline(W, H, 1)
    src.configure(pts, enhance=False)
    src.synth(0, 1, scene="normal", frames_per_ply=32)
    bgr = src.download(0, 0)
    src.close()
    lens = Lens(*LENS_1080P)
    out = {}
    for row, (kw, fmt, cs, kid) in ROWS.items():
        if fmt == "mjpeg" and jpeg is None:
            continue
        p = BoardPipeline(W, H, n)
        p.configure(pts, chunk=32, lanes=1, **kw)
        p.add_board(pts + np.float32([12, 8]))
        if fmt == "bgr":
            for i in range(n):
                p.upload(i, bgr)
        else:
            if fmt == "mjpeg":
                p.set_input_format("mjpeg", planes=True)
                ring, lengths = p.host_ring(), p.jpeg_lengths()
                ring[:, :len(jpeg)] = np.frombuffer(jpeg, np.uint8)
                lengths[:] = len(jpeg)
            else:
                p.set_input_format(fmt, **(dict(colorspace=cs) if cs else {}))
                p.host_ring()[:] = raw_of(bgr, fmt)
            p.submit(0, n)
            p.wait_submitted()
        for on in (False, True):
            p.set_lens(lens if on else None)
            p.run(0, n)
            p.results(0, n)
            t = []
            for _ in range(REPS):
                p.ctx.profile_reset()
                p.ctx.profile_enable(-1)
                p.run(0, n)
                p.results(0, n)
                t.append(1e3 * p.ctx.profile_read(N.K_ALL[kid])[0] / n)
                p.ctx.profile_enable(-2)
            p.ctx.profile_reset()
            out[row + ("_lens" if on else "_boards") + "_us"] = float(np.median(t))
        p.close()
    print(json.dumps(out), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
