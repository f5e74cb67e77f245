"""What the lens model in the warp's gather costs (cbv_pipeline_set_lens, k_warp_lens.hip), in one session on the same
resident 1080p frames, the lens switched on and off in turn on the SAME pipeline (set_lens; the boards' matrices stay):
  - per-frame GPU time (event pairs around every launch, one lane) of each lens kernel against its lens-free kernel:
    k_warp (BGR), k_warp_yuv (NV12), k_warp_bayer, k_warp_profile and k_warp_jpeg (planes mode), and the share of the lens
    kernel's time that the double-precision coordinate step accounts for, taken as (lens - lens-free) / lens: the two
    kernels differ in that step and in nothing else;
  - frames/s of whole runs with the lens on and off: enhance=False (the warp is most of a frame), enhance=True (a few
    percent of it), and enhance=True with four boards.
--reps repetitions (5), median and range.  The Motion-JPEG stream is encoded by tests/ref_jpeg.py, in Python and slowly:
--make-jpeg FILE writes it once where no GPU is needed, --jpeg FILE reads it (without it the k_warp_jpeg row is left out).

    python tools/lens_timing.py --make-jpeg frame1080.jpg                                   (anywhere)
    python tools/lens_timing.py [--frames N] [--reps N] [--jpeg frame1080.jpg] [--json OUT]  (GPU box)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

W, H = 1920, 1080
LENS_1080P = (1400.0, 1400.0, 960.0, 540.0, -0.28, 0.09, 0.001, -0.0005, -0.012)  # the barrel lens of the tests at 1080p
SHIPPED = {"hue_shift": -86, "sat_scale": 0.91, "val_scale": 2.46, "contrast": 1.48, "brightness": -30, "radical_mode": 0, "target_hue": 0,
           "hue_window": 26}
KERNELS = {  # row -> (configure keywords, input format, kernel id the warp is counted under)
    "k_warp": (dict(enhance=False), "bgr", "WARP"),
    "k_warp_yuv nv12": (dict(enhance=False), "nv12", "WARP_YUV"),
    "k_warp_bayer": (dict(enhance=False), "bayer_rggb", "WARP_YUV"),
    "k_warp_profile": (dict(enhance="profile", profile=SHIPPED), "bgr", "WARP"),
    "k_warp_jpeg": (dict(enhance=False), "mjpeg", "WARP_YUV"),
}


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def fmt_s(s, unit=""):
    return "%.4g%s (%.4g .. %.4g)" % (s["median"], unit, s["min"], s["max"])


def fill(p, fmt, bgr, jpeg):
    """the same frame in every slot, resident on the device"""
    from raw_profile_timing import raw_of
    n = p.max_frames
    if fmt == "bgr":
        for i in range(n):
            p.upload(i, bgr)
        return
    if fmt == "mjpeg":
        p.set_input_format("mjpeg", planes=True)
        ring, lengths = p.host_ring(), p.jpeg_lengths()
        ring[:, :len(jpeg)] = np.frombuffer(jpeg, np.uint8)
        lengths[:] = len(jpeg)
    else:
        p.set_input_format(fmt)
        p.host_ring()[:] = raw_of(bgr, fmt)
    p.submit(0, n)
    p.wait_submitted()


def warp_us(p, kid, reps):
    n = p.max_frames
    out = []
    for _ in range(reps):
        p.ctx.profile_reset()
        p.ctx.profile_enable(-1)
        p.run(0, n)
        p.results(0, n)
        out.append(1e3 * p.ctx.profile_read(kid)[0] / n)
        p.ctx.profile_enable(-2)
    p.ctx.profile_reset()
    return out


def fps(p):
    n = p.max_frames
    p.ctx.synchronize()
    t0 = time.perf_counter()
    p.run(0, n)
    p.results(0, n)
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--jpeg", default=None)
    ap.add_argument("--make-jpeg", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.make_jpeg:
        import ref_jpeg as R
        from helpers import oracle_frame
        with open(a.make_jpeg, "wb") as f:
            f.write(R.encode_image(oracle_frame(W, H), quality=90, sampling="420"))
        return
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd import synth as S
    from chessboard_vision_amd.stream import BoardPipeline, Lens
    lens, pts, n = Lens(*LENS_1080P), S.scaled_corners(W, H), a.frames
    src = BoardPipeline(W, H, 1)
    src.configure(pts, enhance=False)
    src.synth(0, 1, scene="normal", frames_per_ply=32)
    bgr = src.download(0, 0)
    src.close()
    jpeg = open(a.jpeg, "rb").read() if a.jpeg else None
    out = {"kernels_us_per_frame": {}, "runs_fps": {}}
    # 1. the kernels: one lane, chunks of 32 (the many-frames forms), lens off and on in turn
    for row, (kw, fmt, kid) in KERNELS.items():
        if fmt == "mjpeg" and jpeg is None:
            continue
        p = BoardPipeline(W, H, n)
        p.configure(pts, chunk=32, lanes=1, **kw)
        fill(p, fmt, bgr, jpeg)
        t = {False: [], True: []}
        for _ in range(a.reps):
            for on in (False, True):
                p.set_lens(lens if on else None)
                p.run(0, n)  # warm-up of this state
                t[on] += warp_us(p, N.K_ALL[kid], 1)
        p.close()
        off, on = spread(t[False]), spread(t[True])
        share = (on["median"] - off["median"]) / on["median"]
        out["kernels_us_per_frame"][row] = dict(lens_free=off, lens=on, coordinate_step_share=share)
        print("%-18s lens-free %s, lens %s per frame; the coordinate step: %.1f %% of the lens kernel" % (row, fmt_s(off, " us"), fmt_s(on, " us"), 100 * share),
              flush=True)
    # 2. whole runs
    runs = {"enhance=False": (dict(enhance=False), 1), "enhance=True": (dict(profile=SHIPPED), 1), "enhance=True, four boards": (dict(profile=SHIPPED), 4)}
    for row, (kw, boards) in runs.items():
        p = BoardPipeline(W, H, n)
        p.configure(pts, chunk=32, lanes=2, **kw)
        for k in range(1, boards):
            p.add_board(pts + np.float32([12 * k, 8 * k]))
        fill(p, "bgr", bgr, None)
        r = {False: [], True: []}
        for _ in range(a.reps):
            for on in (False, True):
                p.set_lens(lens if on else None)
                fps(p)  # warm-up of this state
                r[on].append(fps(p))
        p.close()
        off, on = spread(r[False]), spread(r[True])
        out["runs_fps"][row] = dict(lens_free=off, lens=on)
        print("%-26s lens-free %s frames/s, lens %s frames/s (%+.2f %%)" % (row, fmt_s(off), fmt_s(on), 100 * (on["median"] / off["median"] - 1)), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
