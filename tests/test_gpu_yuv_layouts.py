"""NV21, yuv420p, YV12, YVYU and UYVY frames on the GPU: cbv_yuv_to_bgr, the ingest ring and the warp from raw frames, byte
for byte against tests/ref64_yuv.py's int64 definition (the only source of expected values; ref64_yuv_layouts.py only says
where the bytes lie) and against pipelines fed the reference-converted BGR frames."""
import functools

import numpy as np
import pytest

import ref64_yuv as R
import ref64_yuv_layouts as L
from chessboard_vision_amd import synth as S

pytestmark = pytest.mark.gpu

FMTS = L.NEW


def _shape(fmt, w, h):
    return (h * 3 // 2, w) if fmt in L.FAMILY_420 else (h, w, 2)


def _random_raw(fmt, w, h, seed):
    """uniformly random bytes: Y < 16, Y > 235 and chroma that saturates every channel all occur"""
    return np.random.default_rng(seed).integers(0, 256, _shape(fmt, w, h), dtype=np.uint8)


def _assert_same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d bytes differ, first at %s: got %d, want %d"
                             % (what, len(bad), want.size, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


# ------------------------------------------------------------------------------------------------------------------
# 1. every (Y, U, V) triple
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cube(family, part):
    """(the NV12 cube frame / part `part` of the YUYV cube, its expected BGR image): computed once, shared, read-only"""
    f = R.cube_nv12() if family == "nv12" else R.cube_yuyv(part)
    want = R.to_bgr(f, family)
    f.setflags(write=False)
    want.setflags(write=False)
    return f, want


@pytest.mark.parametrize("fmt", FMTS)
def test_whole_cube(gpu_ctx, fmt):
    """all 2^24 triples: relayouts of the 4096 x 4096 NV12 frame, and of the four 4096 x 1024 YUYV frames"""
    from chessboard_vision_amd.board_detection import yuv_to_bgr
    sib = L.SIBLING[fmt]
    for part in range(1 if sib == "nv12" else 4):
        f, want = _cube(sib, part)
        _assert_same(yuv_to_bgr(L.relayout(f, sib, fmt), fmt), want, "%s cube, part %d" % (fmt, part))


# ------------------------------------------------------------------------------------------------------------------
# 2. random bytes
# ------------------------------------------------------------------------------------------------------------------
SIZES = [(2, 2), (6, 4), (8, 2), (12, 6), (322, 6), (324, 6), (326, 6), (328, 6), (322, 242), (640, 480), (1920, 1080)]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_random_bytes(gpu_ctx, fmt, size):
    """every even width residue mod 8, planar chroma rows of 3 and 6 bytes (6x4, 12x6), the byte and the dword paths"""
    from chessboard_vision_amd.board_detection import yuv_to_bgr
    w, h = size
    f = _random_raw(fmt, w, h, 7 * w + h)
    got = yuv_to_bgr(f, fmt)
    assert got.shape == (h, w, 3) and got.dtype == np.uint8
    _assert_same(got, L.to_bgr(f, fmt), "%s %dx%d" % (fmt, w, h))


def test_random_bytes_4k_yuv420p(gpu_ctx):
    """offsets of the second and third plane in a large frame"""
    from chessboard_vision_amd.board_detection import yuv_to_bgr
    f = _random_raw("yuv420p", 3840, 2160, 5)
    _assert_same(yuv_to_bgr(f, "yuv420p"), L.to_bgr(f, "yuv420p"), "yuv420p 3840x2160")


def test_two_plane_formats_do_not_read_plane2(gpu_ctx):
    """a caller built against the struct that ended with plane1 has padding where stride2 is and nothing where plane2 is:
    with garbage in both, every format but the three-plane ones converts as before"""
    from chessboard_vision_amd import _native as N
    w, h = 12, 6
    for fmt in ("nv12", "nv21", "yuyv", "yvyu", "uyvy"):
        f = _random_raw(fmt, w, h, 3)
        r = N.raw_frame(f, fmt)[0]
        r.stride2, r.plane2 = -12345, 1
        out = np.zeros((h, w, 3), np.uint8)
        gpu_ctx.check(gpu_ctx.lib.cbv_yuv_to_bgr(gpu_ctx.h, r, w, h, N.ptr(out), w * 3))
        _assert_same(out, L.to_bgr(f, fmt) if fmt in FMTS else R.to_bgr(f, fmt), fmt)
    # ... and the three-plane ones do read them: a missing plane or a short stride is CBV_ERR_ARG
    for fmt in ("yuv420p", "yv12"):
        r = N.raw_frame(_random_raw(fmt, w, h, 3), fmt)[0]
        out = np.zeros((h, w, 3), np.uint8)
        r.stride2 = w // 2 - 1
        assert gpu_ctx.lib.cbv_yuv_to_bgr(gpu_ctx.h, r, w, h, N.ptr(out), w * 3) == -1
        r.stride2, r.plane2 = w // 2, None
        assert gpu_ctx.lib.cbv_yuv_to_bgr(gpu_ctx.h, r, w, h, N.ptr(out), w * 3) == -1
        assert b"plane 2" in gpu_ctx.lib.cbv_last_error(gpu_ctx.h)


# ------------------------------------------------------------------------------------------------------------------
# 3. strided views, the staging buffer poisoned
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(640, 480), (322, 242)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("pad", [4, 7], ids=lambda p: "pad%d" % p)
def test_strided_views_with_poisoned_staging(gpu_ctx, size, pad):
    """Planes cut out of larger buffers filled with other bytes, each with its own row stride (dword multiples travel as
    they lie, odd ones are packed); with the staging buffer poisoned first, a read outside the rows shows."""
    from chessboard_vision_amd.board_detection import yuv_to_bgr
    w, h = size
    rng = np.random.default_rng(w + pad)
    gpu_ctx.check(gpu_ctx.lib.cbv_debug_poison(gpu_ctx.h, 1))
    try:
        ybuf = rng.integers(0, 256, (h + 3, w + pad), dtype=np.uint8)
        b1 = rng.integers(0, 256, (h // 2 + 2, w // 2 + 2 * pad), dtype=np.uint8)
        b2 = rng.integers(0, 256, (h // 2 + 1, w // 2 + 3 * pad + 1), dtype=np.uint8)
        y, c1, c2 = ybuf[2:2 + h, pad // 2:pad // 2 + w], b1[1:1 + h // 2, pad:pad + w // 2], b2[1:, pad + 1:pad + 1 + w // 2]
        assert len({y.strides[0], c1.strides[0], c2.strides[0]}) == 3
        tight = np.concatenate([y.ravel(), c1.ravel(), c2.ravel()]).reshape(h * 3 // 2, w)
        for fmt in ("yuv420p", "yv12"):
            want = L.to_bgr(tight, fmt)
            _assert_same(yuv_to_bgr((y, c1, c2), fmt), want, "%s triple of views" % fmt)
            _assert_same(yuv_to_bgr(tight, fmt), want, "%s single array" % fmt)
        cbuf = rng.integers(0, 256, (h // 2 + 2, w + 2 * pad), dtype=np.uint8)
        vu = cbuf[1:1 + h // 2, pad:pad + w]
        tight = np.concatenate([y, vu])
        _assert_same(yuv_to_bgr((y, vu), "nv21"), L.to_bgr(tight, "nv21"), "NV21 views")
        _assert_same(yuv_to_bgr(tight, "nv21"), L.to_bgr(tight, "nv21"), "NV21 tight")
        qbuf = rng.integers(0, 256, (h + 1, w + pad, 2), dtype=np.uint8)
        q = qbuf[1:, pad // 3:pad // 3 + w]
        for fmt in ("yvyu", "uyvy"):
            _assert_same(yuv_to_bgr(q, fmt), L.to_bgr(q, fmt), "%s view" % fmt)
    finally:
        gpu_ctx.check(gpu_ctx.lib.cbv_debug_poison(gpu_ctx.h, 0))


# ------------------------------------------------------------------------------------------------------------------
# 4. the pipeline with enhancement, fed through the host ring and through upload(fmt=)
# ------------------------------------------------------------------------------------------------------------------
def _everything(p, n, hough=True):
    """every observable of the boards of a pipeline after its runs (as tests/test_gpu_yuv.py collects them)"""
    out = []
    for b in [p] + list(p._boards):
        out.append([bytes(b.results(0, n)), repr(b.noise_results(0, n))] + [bytes(b.square_stats(i)) for i in range(n)]
                   + ([bytes(b.hough(i)) for i in range(n)] if hough else []) + [b.download(2, i).tobytes() for i in range(n)])
    return out


@functools.lru_cache(maxsize=None)
def _game(w, h, n, family):
    """n frames of a scripted game as NV12 / YUYV (input preparation) and their reference conversion; read-only"""
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(w, h, n)
    p.synth(0, n, scene="normal", frames_per_ply=2)
    raw = [R.from_bgr(p.download(0, i), family) for i in range(n)]
    p.close()
    bgr = [R.to_bgr(f, family) for f in raw]
    for a in raw + bgr:
        a.setflags(write=False)
    return raw, bgr


def _enhanced_pipeline(w, h, n, boards):
    from chessboard_vision_amd.stream import BoardPipeline
    pts = S.scaled_corners(w, h)
    p = BoardPipeline(w, h, n)
    p.configure(pts, profile=S.SHIPPED_PROFILE, chunk=2, lanes=2)
    if boards == 2:
        p.add_board(pts + np.float32(2), rot180=True)
    return p


@functools.lru_cache(maxsize=None)
def _enhanced_reference(w, h, n, boards, family):
    """what the pipeline computes on the reference-converted BGR frames: once per family, shared by its formats"""
    ref = _enhanced_pipeline(w, h, n, boards)
    for i, f in enumerate(_game(w, h, n, family)[1]):
        ref.upload(i, f)
    ref.run(0, 4)
    ref.run(4, 2)
    want = _everything(ref, n)
    ref.close()
    return want


def _upload_form(frame, fmt, i):
    """the frame as upload(fmt=) takes it: the single array, or (odd i) its planes as separate arrays"""
    return L.planes(frame, fmt) if fmt in L.FAMILY_420 and i % 2 else frame


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("boards", [1, 2], ids=lambda b: "%dboard" % b)
@pytest.mark.parametrize("size", [(640, 480), (322, 242)], ids=lambda s: "%dx%d" % s)
def test_pipeline_fed_new_layout_equals_pipeline_fed_converted_bgr(gpu_ctx, size, boards, fmt):
    w, h = size
    n = 6
    sib = L.SIBLING[fmt]
    src, want_bgr = _game(w, h, n, sib)
    raw = [L.relayout(f, sib, fmt) for f in src]
    want = _enhanced_reference(w, h, n, boards, sib)
    p = _enhanced_pipeline(w, h, n, boards)
    p.set_input_format(fmt)
    ring = p.host_ring()
    assert ring.shape == (n,) + _shape(fmt, w, h)
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
        p.upload(i, _upload_form(raw[i], fmt, i), fmt=fmt)
    p.run(0, 4)
    p.run(4, 2)
    assert _everything(p, n) == want, fmt
    p.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. raw mode: the warp straight from the raw frames
# ------------------------------------------------------------------------------------------------------------------
def _quads(w, h):
    pts = S.scaled_corners(w, h)
    return {"inside": pts,
            "partly_outside": pts + np.float32([0.42 * w, -0.3 * h]),     # the right and top parts of the quad leave the frame
            "partly_outside_lb": pts + np.float32([-0.42 * w, 0.3 * h]),  # ... and the left and bottom parts
            "mirrored": pts[[1, 0, 3, 2]].copy()}


# boards attached next to board 0: different sizes (S = min(display_size) - margin), geometry and rotation
ATTACHED = [dict(display_size=(800, 600), margin=100, rot180=True), dict(display_size=(640, 480), margin=80),
            dict(display_size=(1280, 420), margin=100, rot180=True), dict(display_size=(1280, 720), margin=100)]


def _raw_pipeline(w, h, n, quad, rot180, hough, attached):
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(w, h, n)
    p.configure(_quads(w, h)[quad], rot180=rot180, use_hough=hough, lanes=2, enhance=False)
    for k in range(attached):
        p.add_board(_quads(w, h)[quad] + np.float32(3 * (k + 1)), use_hough=hough, **ATTACHED[k])
    return p


def _pieces(n):
    """a run of n >= 12 slots in uneven pieces: groups of four frames per thread with a short last group, then launches
    of one frame per thread"""
    return [(0, n - 3), (n - 3, 2), (n - 1, 1)]


@functools.lru_cache(maxsize=None)
def _raw_inputs(w, h, n, content, family, seed):
    """(NV12 / YUYV frames, their reference conversion): a scripted game, or uniformly random bytes"""
    if content == "game":
        return _game(w, h, n, family)
    rng = np.random.default_rng(seed)
    raw = [rng.integers(0, 256, _shape(family, w, h), dtype=np.uint8) for _ in range(n)]
    bgr = [R.to_bgr(f, family) for f in raw]
    for a in raw + bgr:
        a.setflags(write=False)
    return raw, bgr


@functools.lru_cache(maxsize=None)
def _raw_reference(w, h, n, content, family, seed, quad, rot180, attached):
    """an enhance=False pipeline fed the reference-converted BGR frames: once per family"""
    hough = content == "game"   # (noise can overflow HoughCircles' candidate lists)
    ref = _raw_pipeline(w, h, n, quad, rot180, hough, attached)
    for i, f in enumerate(_raw_inputs(w, h, n, content, family, seed)[1]):
        ref.upload(i, f)
    for s0, cnt in _pieces(n):
        ref.run(s0, cnt)
    want = _everything(ref, n, hough)
    ref.close()
    return want


def _check_raw_mode(gpu_ctx, fmt, w, h, n, content, quad, rot180, attached, seed=0):
    sib = L.SIBLING[fmt]
    hough = content == "game"
    src, bgr = _raw_inputs(w, h, n, content, sib, seed)
    raw = [L.relayout(f, sib, fmt) for f in src]
    want = _raw_reference(w, h, n, content, sib, seed, quad, rot180, attached)
    p = _raw_pipeline(w, h, n, quad, rot180, hough, attached)
    p.set_input_format(fmt)
    ring = p.host_ring()
    for i in range(n):
        ring[i] = raw[i]
    p.submit(0, n - 1)
    p.submit(n - 1, 1)
    for s0, cnt in _pieces(n):
        p.run(s0, cnt)
    got = _everything(p, n, hough)
    what = (fmt, w, h, content, quad, rot180, attached)
    for b, (g_, w_) in enumerate(zip(got, want)):
        for i in range(n):
            assert g_[-n + i] == w_[-n + i], what + ("board", b, "warped frame", i)
        assert g_ == w_, what + ("board", b)
    for i in (0, n - 1):
        _assert_same(p.download(0, i), bgr[i], "%s download(0, %d)" % (what, i))
    # the synchronous path: the slots overwritten, then the same frames through upload(fmt=...)
    for b in [p] + list(p._boards):
        b.reset_state()
    for i in range(n):
        p.upload(i, np.zeros_like(raw[i]), fmt=fmt)
    for i in range(n):
        p.upload(i, _upload_form(raw[i], fmt, i), fmt=fmt)
    for s0, cnt in _pieces(n):
        p.run(s0, cnt)
    assert _everything(p, n, hough) == want, what + ("upload",)
    p.close()


RAW_CASES = [((640, 480), "game", "partly_outside", False, 0), ((322, 242), "noise", "mirrored", True, 1),
             ((322, 242), "game", "partly_outside_lb", True, 0), ((640, 480), "noise", "inside", False, 1)]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("case", RAW_CASES, ids=lambda c: "%dx%d-%s-%s-rot%d-%dattached" % (c[0] + c[1:]))
def test_raw_mode_equals_converted_bgr(gpu_ctx, fmt, case):
    """widths 0 and 2 mod 4, quads partly outside the frame and mirrored, both rotations, 1 and 2 boards, runs in uneven
    pieces"""
    (w, h), content, quad, rot180, attached = case
    _check_raw_mode(gpu_ctx, fmt, w, h, 12, content, quad, rot180, attached, seed=len(quad))


def test_raw_mode_five_boards(gpu_ctx):
    _check_raw_mode(gpu_ctx, "yuv420p", 322, 242, 12, "noise", "partly_outside", True, 4, seed=3)


def test_raw_mode_4k_frame(gpu_ctx):
    """one 3840 x 2160 frame: plane offsets beyond 2^23 bytes"""
    from chessboard_vision_amd.stream import BoardPipeline
    w, h = 3840, 2160
    src = R.from_bgr(np.random.default_rng(11).integers(0, 256, (h, w, 3), dtype=np.uint8), "nv12")
    bgr = R.nv12_to_bgr(src)
    pts = S.scaled_corners(w, h)
    ref = BoardPipeline(w, h, 1)
    ref.configure(pts, rot180=True, use_hough=False, enhance=False)
    ref.upload(0, bgr)
    ref.run(0, 1)
    want = _everything(ref, 1, False)
    ref.close()
    for fmt in ("yuv420p", "nv21"):
        p = BoardPipeline(w, h, 1)
        p.configure(pts, rot180=True, use_hough=False, enhance=False)
        p.set_input_format(fmt)
        p.host_ring()[0] = L.relayout(src, "nv12", fmt)
        p.submit(0, 1)
        p.run(0, 1)
        assert _everything(p, 1, False) == want, fmt
        _assert_same(p.download(0, 0), bgr, "%s download(0, 0)" % fmt)
        p.close()


# ------------------------------------------------------------------------------------------------------------------
# 6. state and errors
# ------------------------------------------------------------------------------------------------------------------
def test_switching_formats_and_error_paths(gpu_ctx):
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.stream import BoardPipeline
    lib = gpu_ctx.lib
    w, h, n = 640, 480, 4
    pts = S.scaled_corners(w, h)
    src, bgr = _game(w, h, 6, "nv12")
    src2, bgr2 = _game(w, h, 6, "yuyv")
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
    for fmt in FMTS:
        # bgr -> fmt -> bgr: the ring is reallocated in the format's shape, and BGR gives today's results again
        p.set_input_format(fmt)
        assert p.input_format == fmt
        sib = L.SIBLING[fmt]
        raw = [L.relayout(f, sib, fmt) for f in (src if sib == "nv12" else src2)[:n]]
        assert lib.cbv_pipeline_host_slot_bytes(p.h_) == (raw[0].size + 255) // 256 * 256
        p.reset_state()
        ring = p.host_ring()
        assert ring.shape == (n,) + _shape(fmt, w, h)
        for i in range(n):
            ring[i] = raw[i]
        p.submit(0, n)
        p.run(0, n)
        for i in range(n):
            _assert_same(p.download(0, i), (bgr if sib == "nv12" else bgr2)[i], "%s slot %d" % (fmt, i))
        # a board handle: refused
        r = N.raw_frame(raw[0], fmt)[0]
        assert lib.cbv_pipeline_set_input_format(board.h_, N.FORMATS[fmt]) == -4
        assert lib.cbv_pipeline_upload_raw(board.h_, 0, r) == -4
        assert lib.cbv_pipeline_host_slot_bytes(board.h_) == 0
        # ids that are not assigned (VYUY's bits, a stray high bit, a family without layouts): refused, nothing changes
        for bad in (0x32, 0x41, 0x61, 0x10, 0x20, 0x13, 0x23, 0x121):
            assert lib.cbv_pipeline_set_input_format(p.h_, bad) == -1, hex(bad)
            assert b"cbv_pipeline_set_input_format" in lib.cbv_last_error(gpu_ctx.h)
            r.fmt = bad
            assert lib.cbv_pipeline_upload_raw(p.h_, 0, r) == -1, hex(bad)
            out = np.zeros((h, w, 3), np.uint8)
            assert lib.cbv_yuv_to_bgr(gpu_ctx.h, r, w, h, N.ptr(out), w * 3) == -1, hex(bad)
        assert p.input_format == fmt and lib.cbv_pipeline_host_slot_bytes(p.h_) == (raw[0].size + 255) // 256 * 256
        with pytest.raises(ValueError):
            p.set_input_format("i420")
        p.set_input_format("bgr")
        assert lib.cbv_pipeline_host_slot_bytes(p.h_) == w * h * 3
        assert through_bgr_ring() == today, fmt
    p.close()
    # odd sizes: refused, nothing changes
    for (ww, hh), refused in (((321, 240), FMTS), ((320, 241), ("nv21", "yuv420p", "yv12"))):
        q = BoardPipeline(ww, hh, 2)
        for fmt in refused:
            with pytest.raises(RuntimeError, match=r"cbv_pipeline_set_input_format.*even.*code -1\)"):
                q.set_input_format(fmt)
        assert q.input_format == "bgr" and lib.cbv_pipeline_host_slot_bytes(q.h_) == (ww * hh * 3 + 255) // 256 * 256
        if len(refused) == 3:
            for fmt in ("yvyu", "uyvy"):
                q.set_input_format(fmt)
                assert q.host_ring().shape == (2, hh, ww, 2)
        q.close()


def test_raw_mode_refuses_another_format(gpu_ctx):
    from chessboard_vision_amd.stream import BoardPipeline
    w, h = 640, 480
    p = BoardPipeline(w, h, 2)
    p.configure(S.scaled_corners(w, h), enhance=False)
    p.synth(0, 2)
    p.run(0, 2)
    # a gray level per format, more than PieceDetector's change threshold (25) apart from each other: whichever earlier
    # frame a square's reference is, the frame differs from it and the square is processed
    for fmt, level in zip(FMTS, (40, 90, 140, 190, 240)):
        p.set_input_format(fmt)
        for other in ("nv12", "yuyv") + tuple(f for f in FMTS if f != fmt):
            with pytest.raises(RuntimeError, match=r"raw mode.*code -4\)"):
                p.upload(0, np.zeros(_shape(other, w, h), np.uint8), fmt=other)
        with pytest.raises(RuntimeError, match="raw mode"):
            p.upload(0, np.zeros((h, w, 3), np.uint8))
        with pytest.raises(RuntimeError, match="no raw frame"):
            p.run(0, 1)
        frame = np.full(_shape(fmt, w, h), 128, np.uint8)
        (frame[:h] if fmt in L.FAMILY_420 else frame[..., 1 if fmt == "uyvy" else 0])[...] = level
        p.upload(0, frame, fmt=fmt)
        p.run(0, 1)
        _assert_same(p.download(0, 0), L.to_bgr(frame, fmt), fmt)
        assert np.all(p.download(0, 0) == p.download(0, 0)[0, 0]) and p.results(0, 1)[0].processed
    p.close()


# ------------------------------------------------------------------------------------------------------------------
# 7. launch counts
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


def _raw_mode_launches(ctx, fmt, attached):
    w, h, n = 640, 480, 12
    p = _raw_pipeline(w, h, n, "inside", False, True, attached)
    p.set_input_format(fmt)
    p.host_ring()[:] = 128
    p.submit(0, n)
    p.run(0, n)  # warm-up
    p.results(0, n)

    def step():
        p.submit(0, n)
        p.run(0, n)
        p.results(0, n)
    counts = _counted(ctx, step)
    p.close()
    return counts


def test_launch_counts(gpu_ctx):
    """raw mode launches what NV12 raw mode launches; a host-fed enhanced pipeline one k_ingest per submit, nothing else"""
    from chessboard_vision_amd.stream import BoardPipeline
    for attached in (0, 1):
        nv12 = _raw_mode_launches(gpu_ctx, "nv12", attached)
        assert nv12["WARP_YUV"] >= 1 and "INGEST" not in nv12 and "WARP" not in nv12, nv12
        for fmt in FMTS:
            assert _raw_mode_launches(gpu_ctx, fmt, attached) == nv12, (fmt, attached)
    w, h = 640, 480
    for fmt in FMTS:
        p = BoardPipeline(w, h, 4)
        p.configure(S.scaled_corners(w, h), profile=S.SHIPPED_PROFILE)
        p.set_input_format(fmt)
        p.host_ring()[:] = 128
        p.submit(0, 4)
        p.run(0, 4)  # warm-up
        p.results(0, 4)

        def submits():
            p.submit(0, 2)
            p.submit(2, 2)
            p.wait_submitted()
        assert _counted(gpu_ctx, submits) == {"INGEST": 2}, fmt
        p.run(0, 4)
        p.results(0, 4)
        p.close()
