"""What the session chain (BoardPipeline.configure(enhance=False)) and the warp from raw frames (k_warp_yuv, k_warp_bayer)
are worth.
Prints ONE JSON object:

  fused     per-frame kernel time of k_warp_yuv / k_warp_bayer against k_ingest + k_warp (cbv_profile_read event pairs), every YUV and Bayer format
            (`--formats` picks some), 1080p and 4K, batches larger than the Infinity Cache, `--rounds` alternating rounds, each listed
  resident  frames/s with enhance=False against enhance=True: device-resident BGR, 512 frames in flight, 1080p and 4K,
            1 and 4 boards (median and spread of `--reps` steps)
  host_fed  frames/s of YUV and Bayer frames fed through the pinned ring in two halves, the copy of one half overlapping the
            run of the other; the copy alone and the runs alone beside it say which of the two limits the rate
  latency   wall time of run + results of one frame
  mjpeg     (`--only mjpeg`, 1080p) the session chain fed Motion-JPEG streams through the pinned ring, planes off (the decode
            fills the BGR ring, k_warp samples it) and planes on (the decode stops at the plane ring, k_warp_jpeg samples it),
            measured alternately: frames/s as in host_fed, and the latency of submit + run + results of one frame.  The
            streams are those of `tools/jpeg_timing.py --make-streams FILE.npz` (`--mjpeg-streams FILE.npz`, variant
            `--mjpeg-variant`), or, without a file, one synthetic frame encoded here by tests/ref_jpeg.py.

    python tools/session_timing.py [--quick] [--rounds N] [--reps N] [--formats nv12,yuv420p] [--sizes 1080p]      (GPU box)
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

SIZES = {"1080p": (1920, 1080), "4k": (3840, 2160)}
FMTS = tuple(f for f in N.FORMATS if f != "bgr") + tuple(N.BAYER_FORMATS)


def spread(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def profiled(ctx, kid, fn):
    """(total ms, launches) of kernel `kid` over fn()"""
    ctx.profile_reset()
    ctx.profile_enable(kid)
    try:
        fn()
        ctx.synchronize()
        return ctx.profile_read(kid)
    finally:
        ctx.profile_enable(-2)
        ctx.profile_reset()


def fused_against_unfused(size, fmt, n, rounds):
    w, h = SIZES[size]
    pts = S.scaled_corners(w, h)
    ing = BoardPipeline(w, h, n)  # enhancement on: its submit converts (k_ingest); never run
    ing.configure(pts, profile=S.SHIPPED_PROFILE, chunk=1, lanes=1)
    ing.set_input_format(fmt)
    ing.host_ring()[:] = 96
    if fmt in N.BAYER_FORMATS:  # a mosaic of a scene instead of one level: the frames k_warp samples, as a sensor would deliver them
        bgr0 = BoardPipeline(w, h, 1)
        bgr0.synth(0, 1, scene="normal")
        ing.host_ring()[:] = S.bayer_mosaic(bgr0.download(0, 0), fmt)
        bgr0.close()
    bgr = BoardPipeline(w, h, n)  # k_warp on BGR frames, no byte map: the unfused chain's second kernel
    bgr.configure(pts, chunk=n, lanes=1, use_hough=False, enhance=False)
    bgr.synth(0, n, scene="normal", frames_per_ply=32)
    raw = BoardPipeline(w, h, n)
    raw.configure(pts, chunk=n, lanes=1, use_hough=False, enhance=False)
    raw.set_input_format(fmt)
    raw.host_ring()[:] = ing.host_ring()
    raw.submit(0, n)
    raw.wait_submitted()
    out = []
    for r in range(rounds + 1):  # round 0 warms up
        a = profiled(ing.ctx, N.K["INGEST"], lambda: (ing.submit(0, n), ing.wait_submitted()))
        b = profiled(bgr.ctx, N.K["WARP"], lambda: bgr.run(0, n))
        c = profiled(raw.ctx, N.K_ALL["WARP_YUV"], lambda: raw.run(0, n))
        assert a[1] == b[1] == c[1] == 1, (a, b, c)
        if r:
            out.append(dict(ingest_us=1e3 * a[0] / n, warp_us=1e3 * b[0] / n, warp_yuv_us=1e3 * c[0] / n))
    for p in (ing, bgr, raw):
        p.close()
    return dict(size=size, fmt=fmt, frames=n, rounds=out,
                unfused_us=spread([o["ingest_us"] + o["warp_us"] for o in out]), fused_us=spread([o["warp_yuv_us"] for o in out]))


def boards_on(p, pts, k):
    return [p] + [p.add_board(pts + np.float32(2 * i)) for i in range(1, k)]


def step_fps(p, frames, run, reps):
    def step():
        for s0 in range(0, frames, run):
            p.run(s0, min(run, frames - s0))
        p.results(0, frames)
    step()
    t = []
    for _ in range(reps):
        p.ctx.synchronize()
        t0 = time.perf_counter()
        step()
        t.append(time.perf_counter() - t0)
    return spread([frames / x for x in t])


def latency_ms(p, n=200):
    t = []
    for i in range(n):
        t0 = time.perf_counter()
        p.run(i % 2, 1)
        p.results(i % 2, 1)
        t.append(time.perf_counter() - t0)
    return spread([1e3 * x for x in t[20:]])


def resident(size, k, frames, reps):
    w, h = SIZES[size]
    pts = S.scaled_corners(w, h)
    p = BoardPipeline(w, h, frames)
    p.synth(0, frames, scene="normal", frames_per_ply=32)
    row = dict(size=size, boards=k, frames=frames)
    for enhance in (True, False, True, False):  # alternating; the second pair is the one reported beside the first
        p.configure(pts, profile=S.SHIPPED_PROFILE, chunk=64, enhance=enhance, **S.SHIPPED_DETECTOR)
        extra = boards_on(p, pts, k)[1:]
        row.setdefault("fps_enhance_%s" % ("on" if enhance else "off"), []).append(step_fps(p, frames, frames // 4, reps))
        row["latency_ms_enhance_%s" % ("on" if enhance else "off")] = latency_ms(p)
        for b in extra:
            b.close()
    p.close()
    return row


def host_fed(size, fmt, ring, reps):
    """`ring` slots in two halves; per step every half is submitted once and run once"""
    w, h = SIZES[size]
    pts = S.scaled_corners(w, h)
    half = ring // 2
    row = dict(size=size, fmt=fmt, ring=ring)
    for enhance in (True, False):
        p = BoardPipeline(w, h, ring)
        p.configure(pts, profile=S.SHIPPED_PROFILE, chunk=min(64, half), enhance=enhance, **S.SHIPPED_DETECTOR)
        p.set_input_format(fmt)
        p.host_ring()[:] = 96
        slot_bytes = p.ctx.lib.cbv_pipeline_host_slot_bytes(p.h_)

        def both(rounds=4):
            p.submit(0, half)
            for r in range(rounds):
                for hf in (0, 1):
                    if r + 1 < rounds or hf == 0:
                        p.submit((1 - hf) * half, half)  # the other half crosses the link while this one runs
                    p.run(hf * half, half)
            p.results(0, ring)
            return 2 * rounds * half

        def copies(rounds=4):
            for _ in range(rounds):
                p.submit(0, half)
                p.submit(half, half)
            p.wait_submitted()
            return 2 * rounds * half

        def runs(rounds=4):
            for _ in range(rounds):
                p.run(0, half)
                p.run(half, half)
            p.results(0, ring)
            return 2 * rounds * half

        res = {}
        for name, fn in (("overlapped", both), ("copy_only", copies), ("run_only", runs)):
            fn(1)
            t = []
            for _ in range(reps):
                p.ctx.synchronize()
                t0 = time.perf_counter()
                nfr = fn()
                p.ctx.synchronize()
                t.append(nfr / (time.perf_counter() - t0))
            res[name] = spread(t)
        res["link_GBps"] = res["copy_only"]["median"] * slot_bytes / 1e9
        res["limit"] = "link" if res["copy_only"]["median"] < res["run_only"]["median"] else "gpu"
        res["latency_ms"] = latency_ms(p)
        row["enhance_%s" % ("on" if enhance else "off")] = res
        p.close()
    return row


def mjpeg_fed(ring, reps, streams_file, variant, rounds):
    """the session chain at 1080p fed JPEG streams, planes off and on alternately, `rounds` times each"""
    w, h = SIZES["1080p"]
    pts = S.scaled_corners(w, h)
    half = ring // 2
    if streams_file:
        z = np.load(streams_file)
        data = [z[k] for k in sorted(z.files) if k.startswith(variant + "_")]
    else:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import ref_jpeg as R
        q, sampling = variant.split("-")[:2]
        src = BoardPipeline(w, h, 1)
        src.synth(0, 1, scene="normal")
        data = [np.frombuffer(R.encode_image(src.download(0, 0), quality=int(q[1:]), sampling=sampling), np.uint8)]
        src.close()
    assert data, "no stream of variant %s" % variant
    planes_on = variant.split("-")[1]
    row = dict(size="1080p", variant=variant, ring=ring, stream_bytes=[int(len(d)) for d in data], planes_off=[], planes_on=[])
    for r in range(rounds):
        for planes in (False, planes_on):
            p = BoardPipeline(w, h, ring)
            p.configure(pts, profile=S.SHIPPED_PROFILE, chunk=min(64, half), enhance=False, **S.SHIPPED_DETECTOR)
            p.set_input_format("mjpeg", slot_bytes=max(len(d) for d in data), planes=planes)
            hr, lengths = p.host_ring(), p.jpeg_lengths()
            for i in range(ring):
                d = data[i % len(data)]
                hr[i, :len(d)] = d
                lengths[i] = len(d)

            def both(n=4):
                p.submit(0, half)
                for k in range(n):
                    for hf in (0, 1):
                        if k + 1 < n or hf == 0:
                            p.submit((1 - hf) * half, half)  # the other half is copied and decoded while this one runs
                        p.run(hf * half, half)
                p.results(0, ring)
                return 2 * n * half

            def copies(n=4):
                for _ in range(n):
                    p.submit(0, half)
                    p.submit(half, half)
                p.wait_submitted()
                return 2 * n * half

            def runs(n=4):
                for _ in range(n):
                    p.run(0, half)
                    p.run(half, half)
                p.results(0, ring)
                return 2 * n * half

            res = {}
            for name, fn in (("overlapped", both), ("submit_only", copies), ("run_only", runs)):
                fn(1)
                t = []
                for _ in range(reps):
                    p.ctx.synchronize()
                    t0 = time.perf_counter()
                    nfr = fn()
                    p.ctx.synchronize()
                    t.append(nfr / (time.perf_counter() - t0))
                res[name] = spread(t)
            t = []
            for i in range(120):  # one frame from the ring to its results
                t0 = time.perf_counter()
                p.submit(i % 2, 1)
                p.run(i % 2, 1)
                p.results(i % 2, 1)
                t.append(time.perf_counter() - t0)
            res["one_frame_ms"] = spread([1e3 * x for x in t[20:]])
            row["planes_on" if planes else "planes_off"].append(res)
            p.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="1080p only, small batches: a functional check of the tool")
    ap.add_argument("--only", default="fused,resident,host_fed")
    ap.add_argument("--formats", default=",".join(FMTS))
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--mjpeg-streams", help="npz of 1080p streams from tools/jpeg_timing.py --make-streams (the mjpeg rows)")
    ap.add_argument("--mjpeg-variant", default="q90-422-nodri")
    a = ap.parse_args()
    sizes = ["1080p"] if a.quick else a.sizes.split(",")
    fmts = a.formats.split(",")
    ctx = N.context()
    out = dict(device=ctx.lib.cbv_device_name(ctx.h).decode())
    if "fused" in a.only:
        # raw batches of 384 / 512 MiB (NV12 / YUYV at 1080p: 128 frames; a Bayer batch is 253 MiB of mosaics, and the warped
        # frames written beside it are 141 MiB more) and more: beyond the 256 MiB Infinity Cache
        out["fused"] = [fused_against_unfused(s, f, 16 if a.quick else {"1080p": 128, "4k": 40}[s], a.rounds) for s in sizes for f in fmts]
    if "resident" in a.only:
        out["resident"] = [resident(s, k, 32 if a.quick else 512, a.reps) for s in sizes for k in (1, 4)]
    if "host_fed" in a.only:
        out["host_fed"] = [host_fed(s, f, 16 if a.quick else {"1080p": 128, "4k": 64}[s], a.reps) for s in sizes for f in fmts]
    if "mjpeg" in a.only:
        out["mjpeg"] = [mjpeg_fed(16 if a.quick else 128, a.reps, a.mjpeg_streams, a.mjpeg_variant, 1 if a.quick else a.rounds)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
