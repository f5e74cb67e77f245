"""8-bit Bayer frames on the GPU: bayer_to_bgr, the ingest ring and the warp from the mosaic, bit for bit (tolerance 0)
against tests/ref64_bayer.py's float64 definition and against pipelines fed the reference-demosaiced BGR frames."""
import functools

import numpy as np
import pytest

import ref64_bayer as RB
from chessboard_vision_amd import synth as S

pytestmark = pytest.mark.gpu

FMTS = RB.FORMATS


def _assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d bytes differ, first at %s: got %d, want %d"
                             % (what, len(bad), want.size, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


# ------------------------------------------------------------------------------------------------------------------
# 1. bayer_to_bgr
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(fmt, w, h, name):
    """(mosaic, expected BGR): computed once, shared, read-only"""
    f = RB.inputs(w, h)[name]
    want = RB.to_bgr(f, fmt)
    f.setflags(write=False)
    want.setflags(write=False)
    return f, want


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", RB.SHAPES, ids=lambda s: "%dx%d" % s)
def test_bayer_to_bgr(gpu_ctx, fmt, size):
    """4 x 4 (every pixel an edge copy or one of the four phases) up to 320 x 240; w % 4 != 0 takes the byte form"""
    from chessboard_vision_amd.board_detection import bayer_to_bgr
    w, h = size
    for name in ("noise", "zeros", "ones", "checker1", "checker2"):
        f, want = _case(fmt, w, h, name)
        _assert_same(bayer_to_bgr(f, fmt), want, "%s %dx%d %s" % (fmt, w, h, name))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("pad", [3, 4], ids=lambda p: "stride_w+%d" % p)
def test_bayer_to_bgr_strided_view(gpu_ctx, fmt, pad):
    """64 x 48 cut out of a parent of other bytes: with stride w + 3 the rows start on any byte, w + 4 keeps the stride on
    the device; the staging buffer is poisoned first, so a read outside the rows shows"""
    from chessboard_vision_amd.board_detection import bayer_to_bgr
    w, h = 64, 48
    gpu_ctx.check(gpu_ctx.lib.cbv_debug_poison(gpu_ctx.h, 1))
    try:
        for name in ("noise", "zeros", "ones", "checker1", "checker2"):
            f, want = _case(fmt, w, h, name)
            parent = np.random.default_rng(pad).integers(0, 256, (h + 2, w + pad), dtype=np.uint8)
            view = parent[1:1 + h, pad - 2:pad - 2 + w]
            view[...] = f
            assert view.strides == (w + pad, 1)
            _assert_same(bayer_to_bgr(view, fmt), want, "%s stride %d %s" % (fmt, w + pad, name))
    finally:
        gpu_ctx.check(gpu_ctx.lib.cbv_debug_poison(gpu_ctx.h, 0))


def test_bayer_to_bgr_1080p(gpu_ctx):
    from chessboard_vision_amd.board_detection import bayer_to_bgr
    f = np.random.default_rng(1080).integers(0, 256, (1080, 1920), dtype=np.uint8)
    for fmt in FMTS:
        _assert_same(bayer_to_bgr(f, fmt), RB.to_bgr(f, fmt), "%s 1920x1080" % fmt)


# ------------------------------------------------------------------------------------------------------------------
# 2. upload and the ring, with enhancement
# ------------------------------------------------------------------------------------------------------------------
W, H = 320, 240


@functools.lru_cache(maxsize=None)
def _game(n, fmt):
    """n frames of a scripted game as mosaics (input preparation) and their reference demosaic; read-only"""
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, n)
    p.synth(0, n, scene="normal", frames_per_ply=2)
    raw = [RB.mosaic(p.download(0, i), fmt) for i in range(n)]
    p.close()
    bgr = [RB.to_bgr(f, fmt) for f in raw]
    for a in raw + bgr:
        a.setflags(write=False)
    return raw, bgr


@functools.lru_cache(maxsize=None)
def _noise(n, fmt, seed):
    rng = np.random.default_rng(seed)
    raw = [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(n)]
    bgr = [RB.to_bgr(f, fmt) for f in raw]
    for a in raw + bgr:
        a.setflags(write=False)
    return raw, bgr


def _everything(p, n, hough):
    """every observable of the boards of a pipeline for slots 0 .. n - 1"""
    out = []
    for b in [p] + list(p._boards):
        out.append([bytes(b.results(0, n)), repr(b.noise_results(0, n))] + [bytes(b.square_stats(i)) for i in range(n)]
                   + ([bytes(b.hough(i)) for i in range(n)] if hough else []) + [b.download(2, i).tobytes() for i in range(n)])
    return out


@pytest.mark.parametrize("enhance,fmt", [(True, "bayer_rggb"), ("profile", "bayer_gbrg")], ids=["enhance-rggb", "profile-gbrg"])
def test_pipeline_fed_mosaics_equals_pipeline_fed_demosaiced_bgr(gpu_ctx, enhance, fmt):
    from chessboard_vision_amd.stream import BoardPipeline
    n = 6
    raw, bgr = _game(n, fmt)
    pts = S.scaled_corners(W, H)

    def make():
        p = BoardPipeline(W, H, n)
        p.configure(pts, profile=S.SHIPPED_PROFILE, chunk=2, lanes=2, enhance=enhance)
        return p, p.add_board(pts + np.float32(2), rot180=True)

    ref, ref_board = make()
    ring = ref.host_ring()
    for i in range(n):
        ring[i] = bgr[i]
    ref.submit(0, n)
    ref.run(0, 4)
    ref.run(4, 2)
    today = _everything(ref, n, True)
    ref.close()

    p, board = make()
    p.set_input_format(fmt)
    ring = p.host_ring()
    assert ring.shape == (n, H, W)
    assert ring.strides[0] == gpu_ctx.lib.cbv_pipeline_host_slot_bytes(p.h_) == (W * H + 255) // 256 * 256
    for i in range(n):
        ring[i] = raw[i]
    p.submit(0, 4)
    p.submit(4, 2)
    p.run(0, 4)
    p.run(4, 2)
    for i in range(n):
        _assert_same(p.download(0, i), bgr[i], "%s slot %d" % (fmt, i))
    got = _everything(p, n, True)
    assert got[0][0] == today[0][0] and got[1][0] == today[1][0], "results / board.results"
    assert got == today
    # the synchronous path: the slots overwritten, then the same frames through upload(fmt=...)
    p.reset_state()
    board.reset_state()
    for i in range(n):
        p.upload(i, np.zeros((H, W, 3), np.uint8))
    for i in range(n):
        p.upload(i, raw[i], fmt=fmt)
    for i in range(n):
        _assert_same(p.download(0, i), bgr[i], "%s uploaded slot %d" % (fmt, i))
    p.run(0, 4)
    p.run(4, 2)
    assert _everything(p, n, True) == today
    p.close()


# ------------------------------------------------------------------------------------------------------------------
# 3. raw mode: the warp straight from the mosaic
# ------------------------------------------------------------------------------------------------------------------
def _quads():
    pts = S.scaled_corners(W, H)
    return {"inside": pts,
            "over_left": pts + np.float32([-0.42 * W, 0]), "over_right": pts + np.float32([0.42 * W, 0]),
            "over_top": pts + np.float32([0, -0.3 * H]), "over_bottom": pts + np.float32([0, 0.3 * H]),
            "mirrored": pts[[1, 0, 3, 2]].copy()}


def test_overhanging_quads_reach_the_edge_taps():
    """the four overhanging quads put taps on columns / rows -1, 0, size - 1 and size (the continuous map crosses them)"""
    from chessboard_vision_amd.board_detection import get_perspective_transform
    Sz = 620
    for name, axis, size in (("over_left", 0, W), ("over_right", 0, W), ("over_top", 1, H), ("over_bottom", 1, H)):
        M = np.linalg.inv(get_perspective_transform(np.float32(_quads()[name]), np.float32([[0, 0], [Sz, 0], [0, Sz], [Sz, Sz]])))
        yy, xx = np.mgrid[0:Sz, 0:Sz].astype(np.float64)
        den = M[2, 0] * xx + M[2, 1] * yy + M[2, 2]
        src = ((M[0, 0] * xx + M[0, 1] * yy + M[0, 2]) / den, (M[1, 0] * xx + M[1, 1] * yy + M[1, 2]) / den)[axis]
        top_left = np.floor(src).astype(int)
        wanted = (-1, 0) if name in ("over_left", "over_top") else (size - 2, size - 1)
        for v in wanted + ((-2,) if wanted[0] < 0 else (size,)):
            assert (top_left == v).any(), (name, v)


RUNS = (1, 3, 4, 5, 9, 8, 11)     # one frame per thread below 8; from 8 on groups of four: whole groups, remainders 1 and 3
N_SLOTS = max(RUNS)


def _raw_pipeline(quad, rot180, hough, attached):
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, N_SLOTS)
    p.configure(_quads()[quad], rot180=rot180, use_hough=hough, lanes=2, enhance=False)
    if attached:
        p.add_board(_quads()[quad] + np.float32(3), use_hough=hough, display_size=(800, 600), margin=100, rot180=not rot180)
    return p


def _runs(p, hough):
    out = []
    for length in RUNS:
        p.run(0, length)
        out.append(_everything(p, length, hough))
    return out


def _check_raw_mode(gpu_ctx, fmt, content, quad, rot180, attached):
    hough = content == "game"      # (noise can overflow HoughCircles' candidate lists)
    raw, bgr = _game(N_SLOTS, fmt) if content == "game" else _noise(N_SLOTS, fmt, 17)
    ref = _raw_pipeline(quad, rot180, hough, attached)     # k_warp on the demosaiced frames
    for i in range(N_SLOTS):
        ref.upload(i, bgr[i])
    want = _runs(ref, hough)
    ref.close()
    p = _raw_pipeline(quad, rot180, hough, attached)
    p.set_input_format(fmt)
    ring = p.host_ring()
    assert ring.shape == (N_SLOTS, H, W)
    for i in range(N_SLOTS):
        ring[i] = raw[i]
    p.submit(0, N_SLOTS - 1)
    p.submit(N_SLOTS - 1, 1)
    got = _runs(p, hough)
    what = (fmt, content, quad, rot180, attached)
    for length, g_run, w_run in zip(RUNS, got, want):
        for b, (g_, w_) in enumerate(zip(g_run, w_run)):
            for i in range(length):
                assert g_[-length + i] == w_[-length + i], what + ("run of", length, "board", b, "warped frame", i)
            assert g_ == w_, what + ("run of", length, "board", b)
    for i in (0, N_SLOTS - 1):
        _assert_same(p.download(0, i), bgr[i], "%s download(0, %d)" % (what, i))
    # the synchronous path: the slots overwritten, then the same frames through upload(fmt=...)
    for b in [p] + list(p._boards):
        b.reset_state()
    for i in range(N_SLOTS):
        p.upload(i, np.zeros_like(raw[i]), fmt=fmt)
    for i in range(N_SLOTS):
        p.upload(i, raw[i], fmt=fmt)
    p.run(0, N_SLOTS)
    ref = _raw_pipeline(quad, rot180, hough, attached)
    for i in range(N_SLOTS):
        ref.upload(i, bgr[i])
    ref.run(0, N_SLOTS)
    assert _everything(p, N_SLOTS, hough) == _everything(ref, N_SLOTS, hough), what + ("upload",)
    ref.close()
    p.close()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("quad", ["inside", "over_left", "over_right", "over_top", "over_bottom"])
def test_raw_mode_equals_ingest_then_warp(gpu_ctx, fmt, quad):
    _check_raw_mode(gpu_ctx, fmt, "noise", quad, False, 0)


@pytest.mark.parametrize("case", [("game", "inside", False, 0), ("noise", "mirrored", False, 0), ("noise", "inside", True, 0),
                                  ("noise", "over_left", False, 1), ("game", "over_bottom", True, 1)],
                         ids=lambda c: "%s-%s-rot%d-%dattached" % c)
def test_raw_mode_mirrored_rotated_two_boards(gpu_ctx, case):
    _check_raw_mode(gpu_ctx, "bayer_grbg", *case)


# ------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(321, 240), (320, 241)], ids=lambda s: "%dx%d" % s)
def test_odd_sizes_are_refused_and_nothing_changes(gpu_ctx, size):
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.stream import BoardPipeline
    w, h = size
    lib = gpu_ctx.lib
    p = BoardPipeline(w, h, 2)
    p.configure(S.scaled_corners(w, h), enhance=False)

    def results():
        p.reset_state()
        p.synth(0, 2)
        p.run(0, 2)
        return bytes(p.results(0, 2)), p.download(2, 1).tobytes()

    before = results()
    for fmt in FMTS:
        assert lib.cbv_pipeline_set_input_format(p.h_, RB.IDS[fmt]) == -1
        assert b"cbv_pipeline_set_input_format" in lib.cbv_last_error(gpu_ctx.h)
        with pytest.raises(RuntimeError, match=r"cbv_pipeline_set_input_format.*even.*code -1\)"):
            p.set_input_format(fmt)
        r = N.RawFrame()
        buf = np.zeros((h, w), np.uint8)
        r.fmt, r.stride0, r.plane0 = RB.IDS[fmt], w, buf.ctypes.data
        assert lib.cbv_pipeline_upload_raw(p.h_, 0, r) == -1
        out = np.zeros((h, w, 3), np.uint8)
        assert lib.cbv_yuv_to_bgr(gpu_ctx.h, r, w, h, N.ptr(out), w * 3) == -1
    assert p.input_format == "bgr" and lib.cbv_pipeline_host_slot_bytes(p.h_) == (w * h * 3 + 255) // 256 * 256
    assert results() == before
    p.close()


@pytest.mark.parametrize("size", [(2, 240), (320, 2)], ids=lambda s: "%dx%d" % s)
def test_sizes_below_4_are_refused_and_nothing_changes(gpu_ctx, size):
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.stream import BoardPipeline
    w, h = size
    lib = gpu_ctx.lib
    p = BoardPipeline(w, h, 2)
    frame = np.random.default_rng(2).integers(0, 256, (h, w, 3), dtype=np.uint8)
    p.upload(0, frame)
    for fmt in FMTS:
        assert lib.cbv_pipeline_set_input_format(p.h_, RB.IDS[fmt]) == -1
        assert b"cbv_pipeline_set_input_format" in lib.cbv_last_error(gpu_ctx.h)
        r = N.RawFrame()
        buf = np.zeros((h, w), np.uint8)
        r.fmt, r.stride0, r.plane0 = RB.IDS[fmt], w, buf.ctypes.data
        assert lib.cbv_pipeline_upload_raw(p.h_, 0, r) == -1
        out = np.zeros((h, w, 3), np.uint8)
        assert lib.cbv_yuv_to_bgr(gpu_ctx.h, r, w, h, N.ptr(out), w * 3) == -1
    assert p.input_format == "bgr" and lib.cbv_pipeline_host_slot_bytes(p.h_) == (w * h * 3 + 255) // 256 * 256
    _assert_same(p.download(0, 0), frame, "slot 0 after the refusals")
    p.set_input_format("yuyv")       # ... while a format that takes the size is still taken
    assert p.host_ring().shape == (2, h, w, 2)
    p.close()


def test_board_handles_other_formats_and_unassigned_ids(gpu_ctx):
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.stream import BoardPipeline
    lib = gpu_ctx.lib
    pts = S.scaled_corners(W, H)
    p = BoardPipeline(W, H, 2)
    p.configure(pts, enhance=False)
    board = p.add_board(pts + np.float32(2))
    raw, bgr = _noise(2, "bayer_bggr", 3)
    for fmt in FMTS:
        r = N.raw_frame(raw[0], fmt)[0]
        assert lib.cbv_pipeline_set_input_format(board.h_, RB.IDS[fmt]) == -4
        assert lib.cbv_pipeline_upload_raw(board.h_, 0, r) == -4
    # the unassigned ids of the family's neighbourhood
    r = N.raw_frame(raw[0], "bayer_rggb")[0]
    out = np.zeros((H, W, 3), np.uint8)
    for bad in (0x44, 0x05, 0x104):
        assert lib.cbv_pipeline_set_input_format(p.h_, bad) == -1, hex(bad)
        assert b"cbv_pipeline_set_input_format" in lib.cbv_last_error(gpu_ctx.h)
        r.fmt = bad
        assert lib.cbv_pipeline_upload_raw(p.h_, 0, r) == -1, hex(bad)
        assert lib.cbv_yuv_to_bgr(gpu_ctx.h, r, W, H, N.ptr(out), W * 3) == -1, hex(bad)
    assert p.input_format == "bgr"
    # raw mode takes its own format only
    p.set_input_format("bayer_bggr")
    for other, shape in (("bayer_rggb", (H, W)), ("bayer_gbrg", (H, W)), ("nv12", (H * 3 // 2, W)), ("yuyv", (H, W, 2))):
        with pytest.raises(RuntimeError, match=r"raw mode.*code -4\)"):
            p.upload(0, np.zeros(shape, np.uint8), fmt=other)
    with pytest.raises(RuntimeError, match="raw mode"):
        p.upload(0, np.zeros((H, W, 3), np.uint8))
    with pytest.raises(RuntimeError, match="no raw frame"):
        p.run(0, 1)
    p.upload(0, raw[0], fmt="bayer_bggr")
    p.upload(1, raw[1], fmt="BAYER_BGGR")
    p.run(0, 2)
    _assert_same(p.download(0, 1), bgr[1], "download(0, 1)")
    p.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. launch counts
# ------------------------------------------------------------------------------------------------------------------
def _counted(ctx, fn):
    from chessboard_vision_amd import _native as N
    ctx.profile_reset()
    ctx.profile_enable(-1)
    try:
        fn()
        return {k: ctx.profile_read(kid)[1] for k, kid in N.K_ALL.items() if ctx.profile_read(kid)[1]}
    finally:
        ctx.profile_enable(-2)
        ctx.profile_reset()


def test_launch_counts(gpu_ctx):
    from chessboard_vision_amd.stream import BoardPipeline
    n = 4
    pts = S.scaled_corners(W, H)
    for fmt in FMTS + ("bgr",):
        p = BoardPipeline(W, H, n)
        p.configure(pts, profile=S.SHIPPED_PROFILE)
        p.set_input_format(fmt)
        p.host_ring()[:] = 128
        p.submit(0, n)
        p.run(0, n)  # warm-up
        p.results(0, n)

        def submits():
            p.submit(0, 2)
            p.submit(2, 2)
            p.wait_submitted()
        assert _counted(gpu_ctx, submits) == ({} if fmt == "bgr" else {"INGEST": 2}), fmt
        p.run(0, n)
        p.results(0, n)
        p.close()
    # raw mode: a submit launches nothing, a run launches the warp under WARP_YUV and neither k_ingest nor k_warp
    for attached in (0, 1):
        p = BoardPipeline(W, H, n)
        p.configure(pts, enhance=False, lanes=2)
        if attached:
            p.add_board(pts + np.float32(3))
        p.set_input_format("bayer_grbg")
        p.host_ring()[:] = 128
        p.submit(0, n)
        p.run(0, n)  # warm-up
        p.results(0, n)

        def submit():
            p.submit(0, n)
            p.wait_submitted()
        assert _counted(gpu_ctx, submit) == {}

        def run():
            p.run(0, n)
            p.results(0, n)
        counts = _counted(gpu_ctx, run)
        assert counts.get("WARP_YUV", 0) >= 1 and "INGEST" not in counts and "WARP" not in counts, counts
        p.close()
