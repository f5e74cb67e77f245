"""What the raw-frame profile mode (configure(enhance="profile", raw=True), k_warp_raw_profile) costs beside mode 2
(enhance="profile" on the same camera-native frames: k_ingest into the BGR ring, then k_warp_profile), in one session with
the modes alternating: --frames frames resident (512; --frames-4k for 4K, 128), --reps repetitions (5), median and range.
  - per-frame GPU time of the kernels (event pairs around every launch): k_warp_raw_profile of mode 3 against k_ingest +
    k_warp_profile of mode 2, with one lane (the warp has the device to itself but for the scan of the run before) and with
    two lanes inside p.run (beside the square-statistics and HoughCircles kernels of the other lane);
  - frames/s of the two modes, device resident (run + results) and host fed (submit + run + results);
  - device memory each pipeline holds (the difference of the free memory around its creation and first run).
A library built with RAW_PROFILE_FPT = 1, 2 or 4 in the environment gives every family that many frames per thread in the
many-frames form: run this tool with --kernels-only on each build to compare the forms.

    python tools/raw_profile_timing.py [--formats nv12,yuyv,bayer_rggb] [--sizes 1080p,4k] [--frames N] [--reps N]
                                       [--kernels-only] [--json OUT]                                              (GPU box)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"1080p": (1920, 1080), "4k": (3840, 2160)}
RUN = 128
SHIPPED = {"hue_shift": -86, "sat_scale": 0.91, "val_scale": 2.46, "contrast": 1.48, "brightness": -30, "radical_mode": 0, "target_hue": 0,
           "hue_window": 26}
MODES = {2: dict(enhance="profile"), 3: dict(enhance="profile", raw=True)}


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def fmt_s(s, unit=""):
    return "%.4g%s (%.4g .. %.4g)" % (s["median"], unit, s["min"], s["max"])


def raw_of(bgr, fmt):
    """a plausible camera-native frame of a BGR picture (BT.601 limited range, chroma of the top-left sample; a mosaic keeps
    each site's own colour): an input for timing, nothing is compared with it"""
    b, g, r = (bgr[..., i].astype(np.float32) for i in range(3))
    h, w = b.shape
    if fmt.startswith("bayer"):
        first = {"bayer_rggb": (2, 1, 1, 0), "bayer_bggr": (0, 1, 1, 2), "bayer_grbg": (1, 2, 0, 1), "bayer_gbrg": (1, 0, 2, 1)}[fmt]
        out = np.empty((h, w), np.uint8)
        for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            out[dy::2, dx::2] = bgr[dy::2, dx::2, first[k]]
        return out
    to8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)  # noqa: E731
    y, u, v = to8(16 + .257 * r + .504 * g + .098 * b), to8(128 - .148 * r - .291 * g + .439 * b), to8(128 + .439 * r - .368 * g - .071 * b)
    if fmt in ("nv12", "nv21", "yuv420p", "yv12"):
        out = np.empty((h * 3 // 2, w), np.uint8)
        out[:h] = y
        cu, cv = u[::2, ::2], v[::2, ::2]
        if fmt in ("nv12", "nv21"):
            out[h:, 0::2], out[h:, 1::2] = (cu, cv) if fmt == "nv12" else (cv, cu)
        else:
            a, c = (cu, cv) if fmt == "yuv420p" else (cv, cu)
            out[h:] = np.concatenate([a.ravel(), c.ravel()]).reshape(h // 2, w)
        return out
    out = np.empty((h, w, 2), np.uint8)
    cu, cv = u[:, ::2], v[:, ::2]
    if fmt == "uyvy":
        out[..., 1], out[:, 0::2, 0], out[:, 1::2, 0] = y, cu, cv
    else:
        out[..., 0] = y
        out[:, 0::2, 1], out[:, 1::2, 1] = (cu, cv) if fmt == "yuyv" else (cv, cu)
    return out


def free_bytes():
    """free device memory as the HIP runtime of this process reports it"""
    import ctypes as C
    try:
        free, total = C.c_size_t(), C.c_size_t()
        return free.value if C.CDLL("libamdhip64.so").hipMemGetInfo(C.byref(free), C.byref(total)) == 0 else None
    except OSError:
        return None


def run_clip(p, frames, submit=False):
    for s0 in range(0, frames, RUN):
        n = min(RUN, frames - s0)
        if submit:
            p.submit(s0, n)
        p.run(s0, n)


def kernel_us(p, frames, reps, kids, submit):
    """per-frame GPU time of each kernel id of `kids` over the clip (the submit, where k_ingest runs, included)"""
    out = {k: [] for k in kids}
    for _ in range(reps):
        p.ctx.profile_reset()
        p.ctx.profile_enable(-1)
        run_clip(p, frames, submit)
        p.results(0, frames)
        for k, kid in kids.items():
            out[k].append(1e3 * p.ctx.profile_read(kid)[0] / frames)
        p.ctx.profile_enable(-2)
    p.ctx.profile_reset()
    return {k: spread(v) for k, v in out.items()}


def fps(p, frames, submit):
    p.ctx.synchronize()
    t0 = time.perf_counter()
    run_clip(p, frames, submit)
    p.results(0, frames)
    return frames / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--formats", default="nv12,yuyv,bayer_rggb")
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--frames-4k", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd import synth as S
    from chessboard_vision_amd.stream import BoardPipeline
    out = {}
    for size in a.sizes.split(","):
        w, h = SIZES[size]
        frames = a.frames_4k if size == "4k" else a.frames
        pts = S.scaled_corners(w, h)
        src = BoardPipeline(w, h, 1)
        src.configure(pts, enhance=False)
        src.synth(0, 1, scene="normal", frames_per_ply=32)
        bgr = src.download(0, 0)
        src.close()
        for fmt in a.formats.split(","):
            raw = raw_of(bgr, fmt)
            pipes, mem = {}, {}
            for mode in (2, 3):
                before = free_bytes()
                p = BoardPipeline(w, h, frames)
                p.configure(pts, profile=SHIPPED, chunk=32, lanes=2, **MODES[mode])
                p.set_input_format(fmt)
                p.host_ring()[:] = raw
                run_clip(p, frames, submit=True)
                p.results(0, frames)
                after = free_bytes()
                mem[mode] = None if before is None else before - after
                pipes[mode] = p
            key = "%s %s" % (size, fmt)
            out[key] = res = dict(frames=frames, device_bytes={str(m): mem[m] for m in mem})
            if mem[2] is not None:
                print("%-18s device memory: mode 2 %.1f MB, mode 3 %.1f MB" % (key, mem[2] / 1e6, mem[3] / 1e6), flush=True)
            # 1. the kernels, one lane and two lanes, the modes alternating
            for lanes in (1, 2):
                for mode in (2, 3):
                    pipes[mode].configure(pts, profile=SHIPPED, chunk=32, lanes=lanes, **MODES[mode])
                    run_clip(pipes[mode], frames, submit=True)
                kids = {2: {"INGEST": N.K_ALL["INGEST"], "WARP": N.K_ALL["WARP"]}, 3: {"WARP_YUV": N.K_ALL["WARP_YUV"]}}
                got = {m: kernel_us(pipes[m], frames, a.reps, kids[m], submit=True) for m in (2, 3)}
                pair = got[2]["INGEST"]["median"] + got[2]["WARP"]["median"]
                res["kernels lanes=%d" % lanes] = {"mode 2": got[2], "mode 3": got[3]}
                print("%-18s lanes=%d  mode 2: k_ingest %s + k_warp_profile %s = %.4g us;  mode 3: k_warp_raw_profile %s per frame"
                      % (key, lanes, fmt_s(got[2]["INGEST"], " us"), fmt_s(got[2]["WARP"], " us"), pair, fmt_s(got[3]["WARP_YUV"], " us")), flush=True)
            if not a.kernels_only:
                # 2. frames/s, device resident and host fed
                for submit in (False, True):
                    rates = {2: [], 3: []}
                    for _ in range(a.reps):
                        for mode in (2, 3):
                            fps(pipes[mode], frames, submit)  # warm-up of this configuration
                            rates[mode].append(fps(pipes[mode], frames, submit))
                    what = "host fed" if submit else "device resident"
                    res["frames/s " + what] = {str(m): spread(rates[m]) for m in rates}
                    print("%-18s %-15s mode 2 %s frames/s, mode 3 %s frames/s" % (key, what, fmt_s(spread(rates[2])), fmt_s(spread(rates[3]))), flush=True)
            for p in pipes.values():
                p.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
