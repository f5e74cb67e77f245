"""Camera-native frames on the GPU: cbv_yuv_to_bgr bit-exact against the int64 definition (tests/ref64_yuv.py, the only
source of expected values here), and pipelines fed NV12 / YUYV through the ingest ring against pipelines fed the
reference-converted BGR frames."""
import ctypes as C

import numpy as np
import pytest

import ref64_yuv as R
from chessboard_vision_amd import synth as S

pytestmark = pytest.mark.gpu

FMTS = ("nv12", "yuyv")


def _random_raw(fmt, w, h, seed):
    """uniformly random bytes: Y < 16, Y > 235 and chroma that saturates every channel all occur"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h * 3 // 2, w) if fmt == "nv12" else (h, w, 2), dtype=np.uint8)


def _assert_same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d bytes differ, first at %s: got %d, want %d"
                             % (what, len(bad), want.size, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def test_whole_cube_nv12(gpu_ctx):
    """one 4096 x 4096 NV12 frame holds every (Y, U, V) triple once"""
    from chessboard_vision_amd.board_detection import yuv_to_bgr
    f = R.cube_nv12()
    _assert_same(yuv_to_bgr(f, "nv12"), R.nv12_to_bgr(f), "NV12 cube")


def test_whole_cube_yuyv(gpu_ctx):
    """the same 2^24 triples as four 4096 x 1024 YUYV frames"""
    from chessboard_vision_amd.board_detection import yuv_to_bgr
    for part in range(4):
        f = R.cube_yuyv(part)
        _assert_same(yuv_to_bgr(f, "yuyv"), R.yuyv_to_bgr(f), "YUYV cube, part %d" % part)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", [(2, 2), (6, 4), (322, 242), (640, 480), (1920, 1080), (3840, 2160)], ids=lambda s: "%dx%d" % s)
def test_random_bytes(gpu_ctx, fmt, size):
    """w % 4 == 0 takes the dword path, 2, 6 and 322 the byte path"""
    from chessboard_vision_amd.board_detection import yuv_to_bgr
    w, h = size
    f = _random_raw(fmt, w, h, 7 * w + h)
    got = yuv_to_bgr(f, fmt)
    assert got.shape == (h, w, 3) and got.dtype == np.uint8
    _assert_same(got, R.to_bgr(f, fmt), "%s %dx%d" % (fmt, w, h))


@pytest.mark.parametrize("size", [(640, 480), (322, 242)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("pad", [4, 64, 7, 1500], ids=lambda p: "pad%d" % p)
def test_strided_views_with_poisoned_staging(gpu_ctx, size, pad):
    """Planes that are views of larger buffers filled with other bytes: dword-multiple row strides travel as they lie,
    odd and very long ones are packed; with the staging buffer poisoned first, a read outside the rows shows."""
    from chessboard_vision_amd.board_detection import yuv_to_bgr
    w, h = size
    rng = np.random.default_rng(w + pad)
    gpu_ctx.check(gpu_ctx.lib.cbv_debug_poison(gpu_ctx.h, 1))
    try:
        ybuf = rng.integers(0, 256, (h + 3, w + pad), dtype=np.uint8)
        cbuf = rng.integers(0, 256, (h // 2 + 2, w + 2 * pad), dtype=np.uint8)
        y, uv = ybuf[2:2 + h, pad // 2:pad // 2 + w], cbuf[1:1 + h // 2, pad:pad + w]
        tight = np.concatenate([y, uv])
        _assert_same(yuv_to_bgr((y, uv), "nv12"), R.nv12_to_bgr(tight), "NV12 views")
        _assert_same(yuv_to_bgr((y, uv.reshape(h // 2, w // 2, 2)), "nv12"), R.nv12_to_bgr(tight), "NV12 views, [h/2, w/2, 2] chroma")
        _assert_same(yuv_to_bgr(tight, "nv12"), R.nv12_to_bgr(tight), "NV12 tight")
        qbuf = rng.integers(0, 256, (h + 1, w + pad, 2), dtype=np.uint8)
        q = qbuf[1:, pad // 3:pad // 3 + w]
        _assert_same(yuv_to_bgr(q, "yuyv"), R.yuyv_to_bgr(q), "YUYV view")
    finally:
        gpu_ctx.check(gpu_ctx.lib.cbv_debug_poison(gpu_ctx.h, 0))


def _synth_bgr(w, h, n, frames_per_ply=2, scene="normal"):
    """n synthetic camera frames of a scripted game (input preparation)"""
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(w, h, n)
    p.synth(0, n, scene=scene, frames_per_ply=frames_per_ply)
    out = [p.download(0, i) for i in range(n)]
    p.close()
    return out


def _everything(p, n):
    """every observable of the boards of a pipeline after its runs"""
    out = []
    for b in [p] + list(p._boards):
        out.append([bytes(b.results(0, n)), repr(b.noise_results(0, n))] + [bytes(b.square_stats(i)) for i in range(n)]
                   + [bytes(b.hough(i)) for i in range(n)] + [b.download(2, i).tobytes() for i in range(n)])
    return out


@pytest.mark.parametrize("boards", [1, 2], ids=lambda b: "%dboard" % b)
@pytest.mark.parametrize("region", [False, True], ids=["whole", "region"])
@pytest.mark.parametrize("size", [(640, 480), (322, 242)], ids=lambda s: "%dx%d" % s)
def test_pipeline_fed_yuv_equals_pipeline_fed_converted_bgr(gpu_ctx, size, region, boards):
    from chessboard_vision_amd.stream import BoardPipeline
    w, h = size
    n = 6
    pts = S.scaled_corners(w, h)
    bgr = _synth_bgr(w, h, n)

    def make():
        p = BoardPipeline(w, h, n)
        p.configure(pts, profile=S.SHIPPED_PROFILE, chunk=2, lanes=2, enhance_region=region)
        if boards == 2:
            p.add_board(pts + np.float32(2), rot180=True)
        return p

    for fmt in FMTS:
        raw = [R.from_bgr(f, fmt) for f in bgr]
        want_bgr = [R.to_bgr(f, fmt) for f in raw]
        ref = make()
        for i in range(n):
            ref.upload(i, want_bgr[i])
        ref.run(0, 4)
        ref.run(4, 2)
        want = _everything(ref, n)
        ref.close()
        p = make()
        p.set_input_format(fmt)
        ring = p.host_ring()
        assert ring.shape == ((n, h * 3 // 2, w) if fmt == "nv12" else (n, h, w, 2))
        assert ring.strides[0] == gpu_ctx.lib.cbv_pipeline_host_slot_bytes(p.h_) == (raw[0].size + 255) // 256 * 256
        for i in range(n):
            ring[i] = raw[i]
        p.submit(0, 4)
        p.submit(4, 2)
        p.run(0, 4)
        p.run(4, 2)
        for i in range(n):
            _assert_same(p.download(0, i), want_bgr[i], "%s slot %d" % (fmt, i))
        assert _everything(p, n) == want, fmt
        # the synchronous path: the same frames through upload(fmt=...), one array or planes
        p.reset_state()
        for b in p._boards:
            b.reset_state()
        for i in range(n):
            p.upload(i, np.zeros((h, w, 3), np.uint8))
        for i in range(n):
            p.upload(i, (raw[i][:h], raw[i][h:]) if fmt == "nv12" and i % 2 else raw[i], fmt=fmt)
        p.run(0, 4)
        p.run(4, 2)
        assert _everything(p, n) == want, fmt
        p.close()


def _tuples(res):
    return [(r.raw_occupied, r.stable_occupied, r.visual_changes, r.processed, r.changed, r.parcial, r.total, r.circular) for r in res]


def test_ingest_ring_three_partitions_nv12(gpu_ctx):
    """submit() of NV12 slots into a partition whose last reader is THREE runs back waits for that reader, and runs wait
    for the copy and its conversion: equal to the synchronous sequence on the reference-converted frames."""
    from chessboard_vision_amd.stream import BoardPipeline
    w, h, per = 322, 242, 4
    n = 3 * per
    pts = S.scaled_corners(w, h)
    raw = [R.bgr_to_nv12(f) for f in _synth_bgr(w, h, 5 * per)]
    bgr = [R.nv12_to_bgr(f) for f in raw]
    batches = [np.stack(raw[b * per:(b + 1) * per]) for b in range(5)]
    ref = BoardPipeline(w, h, n)
    ref.configure(pts, profile={}, chunk=2)
    want = []
    for b in range(5):
        s0 = (b % 3) * per
        for i in range(per):
            ref.upload(s0 + i, bgr[b * per + i])
        ref.run(s0, per)
        want.append(_tuples(ref.results(s0, per)))
    ref.close()
    a = BoardPipeline(w, h, n)
    a.configure(pts, profile={}, chunk=2)
    a.set_input_format("nv12")
    ring = a.host_ring()
    for b in range(3):
        ring[b * per:(b + 1) * per] = batches[b]
    a.submit(0, n)
    a.wait_submitted()                # the host ring is rewritten below: its copies must have left (runs are not waited for)
    for b in range(3):
        a.run(b * per, per)           # three runs in flight, nothing collected
    got = {}
    ring[0:per] = batches[3]
    a.submit(0, per)                  # reader of partition 0 is three runs back
    ring[per:2 * per] = batches[4]
    a.submit(per, per)
    got[2] = _tuples(a.results(2 * per, per))
    a.run(0, per)
    a.run(per, per)
    got[3] = _tuples(a.results(0, per))
    got[4] = _tuples(a.results(per, per))
    assert got[2] == want[2] and got[3] == want[3] and got[4] == want[4]
    _assert_same(a.download(0, 1), bgr[3 * per + 1], "slot 1")
    _assert_same(a.download(0, per + 2), bgr[4 * per + 2], "slot per + 2")
    a.close()


def test_set_input_format_error_paths_and_switching_back(gpu_ctx):
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.stream import BoardPipeline
    lib = gpu_ctx.lib
    # odd sizes: refused, nothing changes, and the BGR ring goes on working
    for (w, h), refused in (((321, 240), ("nv12", "yuyv")), ((320, 241), ("nv12",))):
        p = BoardPipeline(w, h, 2)
        ring = p.host_ring()
        for fmt in refused:
            with pytest.raises(RuntimeError, match=r"cbv_pipeline_set_input_format.*code -1\)"):
                p.set_input_format(fmt)
        assert p.input_format == "bgr" and lib.cbv_pipeline_host_slot_bytes(p.h_) == (w * h * 3 + 255) // 256 * 256
        ring[0] = 77                                     # the ring is still alive
        p.submit(0, 1)
        p.wait_submitted()
        assert (p.download(0, 0) == 77).all()
        if "yuyv" not in refused:
            p.set_input_format("yuyv")
            assert p.host_ring().shape == (2, h, w, 2)
        p.close()
    w, h, n = 640, 480, 4
    pts = S.scaled_corners(w, h)
    bgr = _synth_bgr(w, h, n)
    p = BoardPipeline(w, h, n)
    p.configure(pts, profile=S.SHIPPED_PROFILE, chunk=2)
    board = p.add_board(pts + np.float32(2))

    def through_bgr_ring():
        p.reset_state()
        board.reset_state()
        ring = p.host_ring()
        assert ring.shape == (n, h, w, 3)
        for i in range(n):
            ring[i] = bgr[i]
        p.submit(0, n)
        p.run(0, n)
        return bytes(p.results(0, n)), bytes(board.results(0, n)), [p.download(0, i).tobytes() for i in range(n)]

    today = through_bgr_ring()
    assert today[2] == [f.tobytes() for f in bgr]
    # an unknown format, a board handle: refused, the pipeline as it was
    with pytest.raises(ValueError):
        p.set_input_format("i420")
    for bad in (3, -1, 99):
        assert lib.cbv_pipeline_set_input_format(p.h_, bad) == -1
        assert b"cbv_pipeline_set_input_format" in lib.cbv_last_error(gpu_ctx.h)
    raw = N.raw_frame(R.bgr_to_nv12(bgr[0]), "nv12")[0]
    assert lib.cbv_pipeline_set_input_format(board.h_, N.FMT_NV12) == -4
    assert lib.cbv_pipeline_upload_raw(board.h_, 0, raw) == -4
    assert lib.cbv_pipeline_host_slot_bytes(board.h_) == 0
    raw.fmt = 5
    assert lib.cbv_pipeline_upload_raw(p.h_, 0, raw) == -1
    assert lib.cbv_pipeline_host_slot_bytes(p.h_) == w * h * 3 and p.input_format == "bgr"
    assert through_bgr_ring() == today
    # bgr -> nv12 -> bgr: today's results again
    p.set_input_format("nv12")
    nv = [R.bgr_to_nv12(f) for f in bgr]
    p.reset_state()
    ring = p.host_ring()
    for i in range(n):
        ring[i] = nv[i]
    p.submit(0, n)
    p.run(0, n)
    for i in range(n):
        _assert_same(p.download(0, i), R.nv12_to_bgr(nv[i]), "slot %d" % i)
    p.set_input_format("bgr")
    assert through_bgr_ring() == today
    p.close()


def _submit_launches(ctx, fmt):
    """launches of every kernel that two submits of two slots add"""
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.stream import BoardPipeline
    w, h = 640, 480
    p = BoardPipeline(w, h, 4)
    p.configure(S.scaled_corners(w, h), profile=S.SHIPPED_PROFILE)
    p.set_input_format(fmt)
    p.host_ring()[:] = 128
    p.submit(0, 4)
    p.run(0, 4)  # warm-up
    p.results(0, 4)
    ctx.profile_reset()
    ctx.profile_enable(-1)
    try:
        p.submit(0, 2)
        p.submit(2, 2)
        p.wait_submitted()
        counts = {name: ctx.profile_read(kid)[1] for kid, name in enumerate(N.KERNEL_IDS)}
    finally:
        ctx.profile_enable(-2)
        ctx.profile_reset()
    p.run(0, 4)
    p.results(0, 4)
    p.close()
    return {k: v for k, v in counts.items() if v}


def test_bgr_submit_launches_no_kernel(gpu_ctx):
    """CBV_FMT_BGR is today's behaviour: copies only.  A YUV format adds one k_ingest launch per submit, nothing else."""
    assert _submit_launches(gpu_ctx, "bgr") == {}
    assert _submit_launches(gpu_ctx, "nv12") == {"INGEST": 2}
    assert _submit_launches(gpu_ctx, "yuyv") == {"INGEST": 2}
