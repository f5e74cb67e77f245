"""Host-fed throughput of the Motion-JPEG ingest beside NV12 and Bayer, in one session (never bench.py's `value`): 1080p
frames sit in the pinned host ring; batch k+1 is copied and decoded (cbv_pipeline_submit) while batch k runs.

    python tools/jpeg_timing.py [--streams FILE.npz] [--make-streams FILE.npz] [--reps 2]
                                [--entropy auto|interval|pieces|segments] [--piece-bytes N] [--depth N]
                                [--planes MODE[,MODE...]]

Per variant (quality 75 / 90, 4:2:2 / 4:2:0; without DRI, with a restart interval of one MCU row ("-dri") and with one of
eight MCU rows ("-dri8": a few long intervals, as a hardware encoder emits them) it prints the submit-only
rate (copy + decode), the overlapped submit || run rate, the bytes that crossed the link per frame, and the latency of ONE
frame in flight (submit of a single slot until its decode has completed).  --entropy and --piece-bytes choose the entropy
path (BoardPipeline.set_jpeg_entropy; "interval" is one lane for a stream without DRI, "segments" cuts restart intervals
into pieces too), --depth the frames a submit decodes per launch (BoardPipeline.set_jpeg_depth), and every JPEG row ends
with the decode's scratch in bytes (include/cbv.h's formula for the row's slot size) and the piece path's figures for the
streams of the variant: pieces, rounds and the share of pieces settled in round 0.  The
per-kernel times come from a kernel trace of this script (rocprofv3 --kernel-trace --stats).

--planes measures the session chain instead (configure(enhance=False), what GameSession.on_frame runs) with the planes mode
of the Motion-JPEG format as named: off, gray, 420, 422 or 444 (set_input_format("mjpeg", planes=...)).  Several modes,
e.g. --planes off,422, are measured alternately in the one session, every repetition one after the other: "off" is the
decode into the BGR ring (k_jpeg_color, then k_warp), any other mode the decode into the plane ring and k_warp_jpeg.  A
stream whose sampling a mode does not admit is left out of that mode's rows.

Encoding 1080p frames with tests/ref_jpeg.py takes a few seconds each, so the streams can be made once on any machine
(--make-streams, no GPU: the frames are then the CPU oracle's synthetic scene) and loaded with --streams."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--streams", help="npz of encoded streams (from --make-streams)")
ap.add_argument("--make-streams", help="encode the streams into this npz and exit (needs no GPU)")
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--frames", type=int, default=2, help="distinct source frames per variant")
ap.add_argument("--entropy", default="auto", choices=("auto", "interval", "pieces", "segments"))
ap.add_argument("--depth", type=int, default=0, help="frames a Motion-JPEG submit decodes per launch (0: the library's default)")
ap.add_argument("--piece-bytes", type=int, default=0, help="piece size of the piece path (0: the library's default)")
ap.add_argument("--planes", help="comma-separated planes modes of the session chain (off, gray, 420, 422, 444) to measure alternately")
ap.add_argument("--only", help="comma-separated variants to run (default: bgr, nv12, bayer_rggb and every JPEG variant)")
args = ap.parse_args()

W, H, HALF, ROUNDS = 1920, 1080, 64, 4
VARIANTS = [(q, s, dri) for q in (75, 90) for s in ("422", "420") for dri in (0, 1, 8)]  # dri: the restart interval in MCU rows


def vname(q, s, dri):
    return "q%d-%s-%s" % (q, s, "dri8" if dri == 8 else "dri" if dri else "nodri")


def make_streams(frames):
    import ref_jpeg as R
    out = {}
    for q, s, dri in VARIANTS:
        row = W // 16  # MCUs per row, both samplings
        for i, f in enumerate(frames):
            out["%s_%d" % (vname(q, s, dri), i)] = np.frombuffer(R.encode_image(f, quality=q, sampling=s, dri=row * dri), np.uint8)
    return out


if args.make_streams:
    from helpers import oracle_frame
    frames = [oracle_frame(W, H, "dim", frame_idx=i) for i in range(args.frames)]
    np.savez_compressed(args.make_streams, **make_streams(frames))
    sys.exit(0)

from chessboard_vision_amd import synth as S  # noqa: E402
from chessboard_vision_amd.stream import BoardPipeline  # noqa: E402

n = 2 * HALF
p = BoardPipeline(W, H, n)
PLANES = args.planes.split(",") if args.planes else [None]  # None: the enhanced pipeline, as before --planes existed
p.configure(S.scaled_corners(W, H), profile=S.SHIPPED_PROFILE, grid_lines=(S.CALIB_GRID_X, S.CALIB_GRID_Y),
            **(dict(enhance=False) if args.planes else {}), **S.SHIPPED_DETECTOR)
p.set_jpeg_entropy(args.entropy, args.piece_bytes)
if args.depth:
    p.set_jpeg_depth(args.depth)
if args.streams:
    z = np.load(args.streams)
    streams = {k: z[k] for k in z.files}
    nsrc = len([k for k in streams if k.startswith(vname(*VARIANTS[0]))])
    from chessboard_vision_amd.board_detection import jpeg_decode
    bgr = [jpeg_decode(streams["%s_%d" % (vname(90, "422", 0), i)], host=True)[0] for i in range(nsrc)]
else:
    p.synth(0, args.frames, scene="dim")
    bgr = [p.download(0, i) for i in range(args.frames)]
    streams, nsrc = make_streams(bgr), args.frames


def nv12(f):
    b, g, r = (f[..., i].astype(np.float32) for i in range(3))
    q = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    y, u, v = q(16 + 0.257 * r + 0.504 * g + 0.098 * b), q(128 - 0.148 * r - 0.291 * g + 0.439 * b), q(128 + 0.439 * r - 0.368 * g - 0.071 * b)
    return np.concatenate([y, np.stack((u[::2, ::2], v[::2, ::2]), axis=-1).reshape(H // 2, W)])


def scratch_bytes(slot_bytes, planes=None):
    """the decode's device scratch for the pipeline's settings (include/cbv.h, cbv_pipeline_set_jpeg_depth)"""
    pw, ph = (W + 15) // 16 * 16, (H + 15) // 16 * 16
    max_int = (W + 7) // 8 * ((H + 7) // 8)
    S = 0 if args.entropy == "interval" else args.piece_bytes or 64
    seg = args.entropy == "segments"
    pieces = (-(-slot_bytes // S) + (max_int if seg else 0)) if S else 0
    per_sample = 2 if planes not in (None, "off") else 3  # the planes go to the plane ring: the scratch holds the coefficients alone
    return p.jpeg_depth * (per_sample * 3 * pw * ph + 4 * max_int + pieces * (40 if seg else 36) + (4 * (3 * max_int + 1) if seg else 0))


def sync():
    p.ctx.check(p.ctx.lib.cbv_ctx_synchronize(p.ctx.h))
    p.wait_submitted()
    p.results(0, 1)


ADMITS = {"gray": (), "420": ("420",), "422": ("420", "422"), "444": ("420", "422", "444")}


def load(fmt, planes=None):
    """the ring filled in `fmt`; returns the bytes a submit of one frame moves, on average"""
    if fmt in ("nv12", "bayer_rggb", "bgr"):
        p.set_input_format(fmt)
        ring = p.host_ring()
        src = [nv12(f) if fmt == "nv12" else S.bayer_mosaic(f, fmt) if fmt != "bgr" else f for f in bgr]
        for i in range(n):
            ring[i] = src[i % nsrc]
        return src[0].size
    data = [streams["%s_%d" % (fmt, i)] for i in range(nsrc)]
    p.set_input_format("mjpeg", slot_bytes=max(len(d) for d in data), planes=planes if planes not in (None, "off") else False)
    ring, lengths = p.host_ring(), p.jpeg_lengths()
    for i in range(n):
        d = data[i % nsrc]
        ring[i, :len(d)] = d
        lengths[i] = len(d)
    return sum((len(d) + 255) // 256 * 256 for d in data) / nsrc


def measure(fmt, planes=None):
    link = load(fmt, planes)
    p.submit(0, n)
    p.run(0, n)
    sync()
    t0 = time.perf_counter()
    for r in range(ROUNDS):
        p.submit(0, HALF)
        p.submit(HALF, HALF)
    sync()
    t_copy = time.perf_counter() - t0
    p.submit(0, HALF)
    t0 = time.perf_counter()
    for r in range(ROUNDS):
        p.submit(HALF, HALF)
        p.run(0, HALF)
        p.submit(0, HALF)
        p.run(HALF, HALF)
    sync()
    t_ovl = time.perf_counter() - t0
    t0 = time.perf_counter()
    for r in range(20):
        p.submit(r % n, 1)
        p.wait_submitted()
    t_one = (time.perf_counter() - t0) / 20
    frames = ROUNDS * n
    stats = p.jpeg_stats(0, nsrc) if p.input_format == "mjpeg" else None
    scratch = scratch_bytes(p.ctx.lib.cbv_pipeline_host_slot_bytes(p.h_), planes) if p.input_format == "mjpeg" else 0
    return frames / t_copy, frames / t_ovl, link, t_one, stats, scratch


formats = args.only.split(",") if args.only else ["bgr", "nv12", "bayer_rggb"] + [vname(*v) for v in VARIANTS]
for rep, fmt, planes in ((r, f, m) for r in range(args.reps) for f in formats for m in PLANES):
    if planes not in (None, "off") and fmt.startswith("q") and fmt.split("-")[1] not in ADMITS[planes]:
        continue
    c, o, link, one, stats, scratch = measure(fmt, planes)
    row = fmt if planes is None else "%s planes %s" % (fmt, planes)
    tail = "   depth %d scratch %d bytes" % (p.jpeg_depth, scratch) if scratch else ""
    if stats is not None and stats[:, 0].any():
        tail += "   pieces %s rounds %s settled in round 0 %.2f" % (stats[:, 0].tolist(), stats[:, 1].tolist(), stats[:, 2].sum() / stats[:, 0].sum())
    print("[%s, rep %d] submit only %8.0f frames/s   submit || run %8.0f frames/s   link %9.0f bytes/frame   one frame in flight %7.1f us%s"
          % (row, rep + 1, c, o, link, one * 1e6, tail), flush=True)
p.close()
