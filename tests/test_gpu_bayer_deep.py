"""Developed mosaics on the GPU (include/cbv.h: Bayer samples of 10 to 16 bits in a 16-bit container, MIPI RAW10 / RAW12 packed
rows, per-colour tables in front of the 8-bit demosaic): bayer_to_bgr, the ingest ring and the warp from the packed mosaic, bit
for bit (tolerance 0) against tests/ref64_bayer_deep.py's restatement and against pipelines fed the reference-developed,
reference-demosaiced BGR frames."""
import functools

import numpy as np
import pytest

import ref64_bayer as RB
import ref64_bayer_deep as RD
from chessboard_vision_amd import synth as S

pytestmark = pytest.mark.gpu

LAYOUTS = RD.LAYOUTS
ENCS = RD.ENCODINGS
ARG, STATE = -1, -4


def _assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d bytes differ, first at %s: got %d, want %d"
                             % (what, len(bad), want.size, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def _develop(bits):
    """black level, unequal gains and gamma 2.2 for samples of `bits` bits"""
    from chessboard_vision_amd.stream import Develop
    top = (1 << bits) - 1
    return Develop(bits, black_level=top // 16, white_level=top - top // 8, gains=(1.9, 1.0, 1.45), gamma=2.2)


@functools.lru_cache(maxsize=None)
def _tables(kind, bits):
    """name -> (what bayer_to_bgr takes as `develop`, the uint8 [3, 2^bits] tables the reference uses); read-only"""
    if kind == "neutral":
        t = RD.neutral(bits)
        t.setflags(write=False)
        return None, t
    if kind == "random":
        t = RD.random_tables(bits, 7)
        t.setflags(write=False)
        return t, t
    d = _develop(bits)
    t = RD.develop_tables(bits, d.black_level, d.white_level, d.gains, d.gamma)
    t.setflags(write=False)
    return d, t


# ------------------------------------------------------------------------------------------------------------------
# 1. bayer_to_bgr
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _packed(enc, w, h, sample_bits, name):
    s = RD.inputs(w, h, sample_bits)[name]
    raw = RD.pack(s, enc)
    raw.setflags(write=False)
    return raw


def _table_cases(enc):
    """(kind of tables, their bits, the bits the samples fill) for one encoding"""
    if enc == "10p":
        return [("neutral", 10, 10), ("random", 10, 10), ("develop", 10, 10)]
    if enc == "12p":
        return [("neutral", 12, 12), ("random", 12, 12), ("develop", 12, 12)]
    # the container: the default table is 16 bits; every admitted size of table; and tables of 10 and 12 bits under samples
    # that fill all 16, so that the clamp on the index is what keeps the read inside the table
    return [("neutral", 16, 16), ("random", 10, 10), ("random", 12, 12), ("random", 14, 14), ("random", 16, 16), ("develop", 12, 12), ("develop", 16, 16),
            ("random", 10, 16), ("random", 12, 16)]


@pytest.mark.parametrize("enc", ENCS)
@pytest.mark.parametrize("size", RD.SHAPES, ids=lambda s: "%dx%d" % s)
def test_bayer_to_bgr(gpu_ctx, enc, size):
    """4 x 4 (every pixel an edge copy) up to 320 x 240; w % 4 != 0 and rows of an odd number of bytes take the byte form"""
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.board_detection import bayer_to_bgr
    w, h = size
    if enc == "10p" and w % 4:
        r = N.RawFrame()
        buf = np.zeros((h, 5 * w // 4 + 2), np.uint8)
        out = np.zeros((h, w, 3), np.uint8)
        for lay in LAYOUTS:
            r.fmt, r.stride0, r.plane0 = RD.IDS[lay + enc], buf.strides[0], buf.ctypes.data
            assert gpu_ctx.lib.cbv_yuv_to_bgr(gpu_ctx.h, r, w, h, N.ptr(out), w * 3) == ARG
            assert b"multiple of 4" in gpu_ctx.lib.cbv_last_error(gpu_ctx.h)
            assert gpu_ctx.lib.cbv_bayer_to_bgr(gpu_ctx.h, r, w, h, None, 0, N.ptr(out), w * 3) == ARG
        assert not out.any()
        return
    for lay in LAYOUTS:
        fmt = lay + enc
        for kind, bits, sample_bits in _table_cases(enc):
            dev, t = _tables(kind, bits)
            names = ("noise",) if sample_bits != bits else ("noise", "zeros", "ones", "checker1", "checker2")
            for name in names:
                raw = _packed(enc, w, h, sample_bits, name)
                want = RD.expected(raw, fmt, t, bits)
                _assert_same(bayer_to_bgr(raw, fmt, develop=dev), want, "%s %dx%d %s %s/%d" % (fmt, w, h, name, kind, bits))
                if name == "noise" and kind == "random":
                    _assert_same(want, RD.expected_int(raw, fmt, t, bits), "the two restatements")


@pytest.mark.parametrize("enc", ENCS)
def test_yuv_to_bgr_entry_point_uses_the_default_table(gpu_ctx, enc):
    from chessboard_vision_amd import _native as N
    w, h = 64, 48
    bits = RD.DEFAULT_BITS[enc]
    raw = _packed(enc, w, h, bits, "noise")
    r, w_, h_, keep = N.raw_frame(raw, "bayer_gbrg" + enc)
    out = np.zeros((h, w, 3), np.uint8)
    gpu_ctx.check(gpu_ctx.lib.cbv_yuv_to_bgr(gpu_ctx.h, r, w, h, N.ptr(out), w * 3))
    _assert_same(out, RD.expected(raw, "bayer_gbrg" + enc, RD.neutral(bits), bits), "cbv_yuv_to_bgr %s" % enc)


@pytest.mark.parametrize("enc", ENCS)
@pytest.mark.parametrize("pad", [3, 4], ids=lambda p: "stride+%d" % p)
def test_bayer_to_bgr_strided_view(gpu_ctx, enc, pad):
    """64 x 48 cut out of a parent of other bytes: with stride row bytes + 3 the rows start on any byte (a uint16 view that is
    not aligned), + 4 keeps the stride on the device; the staging buffer is poisoned first, so a read outside the rows shows"""
    from chessboard_vision_amd.board_detection import bayer_to_bgr
    w, h = 64, 48
    bits = RD.DEFAULT_BITS[enc] if enc != "16" else 12
    dev, t = _tables("random", bits)
    rb = RD.row_bytes(enc, w)
    gpu_ctx.check(gpu_ctx.lib.cbv_debug_poison(gpu_ctx.h, 1))
    try:
        for lay in LAYOUTS:
            for name in ("noise", "ones", "checker1"):
                raw = _packed(enc, w, h, bits, name)
                parent = np.random.default_rng(pad).integers(0, 256, (h + 2) * (rb + pad), dtype=np.uint8)
                off = (rb + pad) + pad - 2
                view = np.ndarray((h, w) if enc == "16" else (h, rb), np.uint16 if enc == "16" else np.uint8, parent, off,
                                  (rb + pad, 2 if enc == "16" else 1))
                view[...] = raw
                assert view.strides[0] == rb + pad
                _assert_same(bayer_to_bgr(view, lay + enc, develop=dev), RD.expected(raw, lay + enc, t, bits), "%s stride %d %s" % (lay + enc, rb + pad, name))
    finally:
        gpu_ctx.check(gpu_ctx.lib.cbv_debug_poison(gpu_ctx.h, 0))


@pytest.mark.parametrize("enc", ENCS)
def test_bayer_to_bgr_1080p(gpu_ctx, enc):
    from chessboard_vision_amd.board_detection import bayer_to_bgr
    bits = {"16": 14, "10p": 10, "12p": 12}[enc]
    raw = RD.pack(np.random.default_rng(1080).integers(0, 1 << bits, (1080, 1920), dtype=np.int64), enc)
    dev, t = _tables("random", bits)
    fmt = {"16": "bayer_bggr", "10p": "bayer_grbg", "12p": "bayer_gbrg"}[enc] + enc
    _assert_same(bayer_to_bgr(raw, fmt, develop=dev), RD.expected(raw, fmt, t, bits), "%s 1920x1080" % fmt)


def _counted(ctx, fn):
    from chessboard_vision_amd import _native as N
    ctx.profile_reset()
    ctx.profile_enable(-1)
    try:
        fn()
        return {k: ctx.profile_read(kid)[1] for k, kid in N.K_EVERY.items() if ctx.profile_read(kid)[1]}
    finally:
        ctx.profile_enable(-2)
        ctx.profile_reset()


@pytest.mark.parametrize("size", [(12, 6), (64, 48)], ids=lambda s: "%dx%d" % s)
def test_tabled_8_bit(gpu_ctx, size):
    """bayer_to_bgr(f, fmt, develop=T) = to_bgr(T[c][f]); without tables today's result, by today's kernel"""
    from chessboard_vision_amd.board_detection import bayer_to_bgr
    w, h = size
    for lay in LAYOUTS:
        for name, f in RB.inputs(w, h).items():
            for kind in ("random", "develop"):
                dev, t = _tables(kind, 8)
                _assert_same(bayer_to_bgr(f, lay, develop=dev), RB.to_bgr(RD.develop(f, lay, t, 8), lay), "%s %s %s" % (lay, name, kind))
            _assert_same(bayer_to_bgr(f, lay), RB.to_bgr(f, lay), "%s %s no tables" % (lay, name))
    f = RB.inputs(w, h)["noise"]
    assert _counted(gpu_ctx, lambda: bayer_to_bgr(f, "bayer_rggb")) == {"INGEST": 1}
    assert _counted(gpu_ctx, lambda: bayer_to_bgr(f, "bayer_rggb", develop=_tables("random", 8)[0])) == {"INGEST_BAYER_DEEP": 1}


# ------------------------------------------------------------------------------------------------------------------
# 2. upload and the ring, with enhancement
# ------------------------------------------------------------------------------------------------------------------
W, H = 320, 240


@functools.lru_cache(maxsize=None)
def _game8(n, lay):
    """n frames of a scripted game as 8-bit mosaics of layout `lay` (input preparation); read-only"""
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, n)
    p.synth(0, n, scene="normal", frames_per_ply=2)
    m = [RB.mosaic(p.download(0, i), lay) for i in range(n)]
    p.close()
    return m


@functools.lru_cache(maxsize=None)
def _frames(content, n, fmt, kind, bits, seed=17):
    """(the packed frames, the BGR frames the reference makes of them, what set_develop takes); read-only.  "game": the scripted
    game's mosaics widened to `bits` bits with noise in the new low bits; "noise": samples over the encoding's whole range"""
    lay, enc = RD.FORMATS[fmt] if fmt in RD.FORMATS else (fmt, "8")
    rng = np.random.default_rng(seed + bits)
    if content == "game":
        sh = bits - 8
        s = [(m.astype(np.int64) << sh) | rng.integers(0, 1 << sh, m.shape) for m in _game8(n, lay)]
    else:
        s = [rng.integers(0, 1 << RD.SAMPLE_BITS[enc], (H, W), dtype=np.int64) for _ in range(n)]
    dev, t = _tables(kind, bits)
    raw = [RD.pack(x, enc) for x in s]
    bgr = [RD.expected(r, fmt, t, bits) for r in raw]
    for a in raw + bgr:
        a.setflags(write=False)
    return raw, bgr, dev


def _everything(p, n, hough):
    """every observable of the boards of a pipeline for slots 0 .. n - 1"""
    out = []
    for b in [p] + list(p._boards):
        out.append([bytes(b.results(0, n)), repr(b.noise_results(0, n))] + [bytes(b.square_stats(i)) for i in range(n)]
                   + ([bytes(b.hough(i)) for i in range(n)] if hough else []) + [b.download(2, i).tobytes() for i in range(n)])
    return out


def _ring_shape(fmt, n):
    lay, enc = RD.FORMATS[fmt]
    return (n, H, W) if enc == "16" else (n, H, RD.row_bytes(enc, W))


@pytest.mark.parametrize("enhance,fmt,kind,bits", [(True, "bayer_rggb10p", "develop", 10), ("profile", "bayer_gbrg16", "develop", 12), (True, "bayer_bggr12p", "neutral", 12)],
                         ids=["enhance-rggb10p", "profile-gbrg16", "enhance-bggr12p-neutral"])
def test_pipeline_fed_packed_mosaics_equals_pipeline_fed_developed_bgr(gpu_ctx, enhance, fmt, kind, bits):
    from chessboard_vision_amd.stream import BoardPipeline
    n = 6
    raw, bgr, dev = _frames("game", n, fmt, kind, bits)
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
    p.set_input_format(fmt, develop=dev)
    ring = p.host_ring()
    assert ring.shape == _ring_shape(fmt, n) and ring.dtype == raw[0].dtype
    lay, enc = RD.FORMATS[fmt]
    assert ring.strides[0] == gpu_ctx.lib.cbv_pipeline_host_slot_bytes(p.h_) == (RD.row_bytes(enc, W) * H + 255) // 256 * 256
    for i in range(n):
        ring[i] = raw[i]
    counts = _counted(gpu_ctx, lambda: (p.submit(0, 4), p.submit(4, 2), p.wait_submitted()))
    assert counts == {"INGEST_BAYER_DEEP": 2}, counts
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
# 3. raw mode: the warp straight from the packed mosaic
# ------------------------------------------------------------------------------------------------------------------
def _quads():
    pts = S.scaled_corners(W, H)
    return {"inside": pts,
            "over_left": pts + np.float32([-0.42 * W, 0]), "over_right": pts + np.float32([0.42 * W, 0]),
            "over_top": pts + np.float32([0, -0.3 * H]), "over_bottom": pts + np.float32([0, 0.3 * H]),
            "mirrored": pts[[1, 0, 3, 2]].copy()}
# (tests/test_gpu_bayer.py::test_overhanging_quads_reach_the_edge_taps shows that these quads put taps on columns and rows
# -1, 0, size - 1 and size of a 320 x 240 frame)


RUNS = (1, 3, 4, 5, 9, 8, 11)     # one frame per thread below 8; from 8 on groups of two: whole groups, and a last group of one
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


def _check_raw_mode(gpu_ctx, fmt, kind, bits, content, quad, rot180, attached):
    hough = content == "game"      # (noise can overflow HoughCircles' candidate lists)
    raw, bgr, dev = _frames(content, N_SLOTS, fmt, kind, bits)
    ref = _raw_pipeline(quad, rot180, hough, attached)     # k_warp on the developed, demosaiced frames
    for i in range(N_SLOTS):
        ref.upload(i, bgr[i])
    want = _runs(ref, hough)
    ref.close()
    p = _raw_pipeline(quad, rot180, hough, attached)
    p.set_input_format(fmt, develop=dev)
    ring = p.host_ring()
    for i in range(N_SLOTS):
        ring[i] = raw[i]
    p.submit(0, N_SLOTS - 1)
    p.submit(N_SLOTS - 1, 1)
    got = _runs(p, hough)
    what = (fmt, kind, bits, content, quad, rot180, attached)
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


# every encoding with the inside quad and one overhanging quad, RAW10 with all five; random tables, so that a wrong phase
# in the gather shows; the container once with 16-bit tables (read from global memory) and once with 10-bit tables under samples
# that fill all 16 bits (the clamp); an 8-bit mosaic with tables, which takes the same kernels
RAW_CASES = [("bayer_rggb10p", 10, "inside"), ("bayer_bggr10p", 10, "over_left"), ("bayer_grbg10p", 10, "over_right"), ("bayer_gbrg10p", 10, "over_top"),
             ("bayer_rggb10p", 10, "over_bottom"), ("bayer_bggr12p", 12, "inside"), ("bayer_grbg12p", 12, "over_bottom"), ("bayer_gbrg16", 16, "inside"),
             ("bayer_rggb16", 10, "over_right"), ("bayer_grbg", 8, "over_top")]


@pytest.mark.parametrize("fmt,bits,quad", RAW_CASES, ids=lambda v: str(v))
def test_raw_mode_equals_ingest_then_warp(gpu_ctx, fmt, bits, quad):
    _check_raw_mode(gpu_ctx, fmt, "random", bits, "noise", quad, False, 0)


@pytest.mark.parametrize("case", [("bayer_grbg12p", "develop", 12, "game", "inside", False, 0), ("bayer_rggb10p", "random", 10, "noise", "mirrored", False, 0),
                                  ("bayer_bggr16", "random", 14, "noise", "inside", True, 0), ("bayer_gbrg12p", "random", 12, "noise", "over_left", False, 1),
                                  ("bayer_rggb10p", "develop", 10, "game", "over_bottom", True, 1)],
                         ids=lambda c: "%s-%s%d-%s-%s-rot%d-%dattached" % c)
def test_raw_mode_mirrored_rotated_two_boards(gpu_ctx, case):
    _check_raw_mode(gpu_ctx, *case)


# ------------------------------------------------------------------------------------------------------------------
# 4. the lens, the profile on raw taps, the colour sweep
# ------------------------------------------------------------------------------------------------------------------
LW, LH, LN = 324, 242, 13      # 324 = 4 * 81: RAW10 takes it; a 12p row is 486 bytes, a 10p row 405


@functools.lru_cache(maxsize=None)
def _lens_frames(fmt, bits):
    lay, enc = RD.FORMATS[fmt]
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(LW, LH, LN)
    p.synth(0, LN, frames_per_ply=2)
    sh = bits - 8
    rng = np.random.default_rng(bits)
    s = [(RB.mosaic(p.download(0, i), lay).astype(np.int64) << sh) | rng.integers(0, 1 << sh, (LH, LW)) for i in range(LN)]
    p.close()
    dev, t = _tables("develop", bits)
    raw = [RD.pack(x, enc) for x in s]
    return raw, [RD.expected(r, fmt, t, bits) for r in raw], dev


def _lens_boards(fmt, frames, dev, profile, lens):
    """the warped boards of two boards of a pipeline fed `frames` in `fmt`: one run of 11 frames in one chunk, then one of 2"""
    import ref_lens as R
    from chessboard_vision_amd.stream import BoardPipeline, Lens
    quad = S.scaled_corners(LW, LH) + np.float32([0.42 * LW, -0.3 * LH])
    kw = dict(enhance="profile", raw=True) if profile else dict(enhance=False)
    radical = dict(S.SHIPPED_PROFILE, radical_mode=1, target_hue=30, hue_window=40)
    p = BoardPipeline(LW, LH, LN)
    p.configure(quad, profile=radical, chunk=11, lanes=1, lens=Lens(*(R.BARREL[:2] + (LW / 2, LH / 2) + R.BARREL[4:])) if lens else None, **kw)
    b = p.add_board(quad + np.float32(3), rot180=True, display_size=(800, 600), margin=100, **(dict(profile=S.SHIPPED_PROFILE) if profile else {}))
    if fmt != "bgr":
        p.set_input_format(fmt, develop=dev)
    for i, f in enumerate(frames):
        p.upload(i, f, fmt=fmt)
    p.run(0, 11)
    p.run(11, 2)
    out = [x.download(2, i) for x in (p, b) for i in range(LN)]
    p.close()
    return out


@pytest.mark.parametrize("lens,profile", [(True, False), (False, True), (True, True)], ids=["lens", "profile", "lens-profile"])
@pytest.mark.parametrize("fmt,bits", [("bayer_rggb10p", 10), ("bayer_gbrg12p", 12), ("bayer_bggr16", 14)], ids=lambda v: str(v))
def test_lens_and_profile_on_raw_taps(gpu_ctx, fmt, bits, lens, profile):
    """two boards (the second smaller and rotated) whose quads leave the frame to the right and at the top, a run of 11 frames in
    one chunk and a run of 2, against the same pipeline fed the BGR frames the reference makes of the packed ones"""
    raw, bgr, dev = _lens_frames(fmt, bits)
    got = _lens_boards(fmt, raw, dev, profile, lens)
    want = _lens_boards("bgr", bgr, None, profile, lens)
    assert len(got) == 2 * LN
    for k, (g, w_) in enumerate(zip(got, want)):
        assert np.array_equal(g, w_), (fmt, profile, lens, k, int((g != w_).sum()))
        black = (~g.any(2)).mean()  # the part of the board that lies outside the frame
        assert 0.05 < black < 0.9, (k, black)


def test_color_sweep_on_a_12p_raw_pipeline(gpu_ctx):
    """three profiles over four frames: the sweep of a raw-mode RAW12 pipeline against the same sweep on the BGR-fed pipeline"""
    from chessboard_vision_amd.stream import BoardPipeline
    fmt, bits, n = "bayer_grbg12p", 12, 4
    raw, bgr, dev = _frames("game", n, fmt, "develop", bits)
    profs = [S.SHIPPED_PROFILE, dict(S.SHIPPED_PROFILE, radical_mode=1, target_hue=30, hue_window=40), dict(S.SHIPPED_PROFILE, sat_scale=3.0, hue_shift=20)]
    pts = S.scaled_corners(W, H)
    q = BoardPipeline(W, H, n)
    q.configure(pts, profile=S.SHIPPED_PROFILE, enhance="profile")
    for i in range(n):
        q.upload(i, bgr[i])
    want = q.color_sweep(0, n, profs)
    q.close()
    p = BoardPipeline(W, H, n)
    p.configure(pts, profile=S.SHIPPED_PROFILE, enhance="profile", raw=True)
    p.set_input_format(fmt, develop=dev)
    assert not p.frames_ptr()                       # raw mode under the profile holds no BGR ring
    for i in range(n):
        p.upload(i, raw[i], fmt=fmt)
    counts = _counted(gpu_ctx, lambda: setattr(p, "_swept", p.color_sweep(0, n, profs)))
    got = p._swept
    assert counts.get("WARP_BAYER_DEEP", 0) > 0 and "WARP" not in counts and "WARP_YUV" not in counts and "INGEST" not in counts, counts
    assert got.records.shape == want.records.shape == (3, n)
    for name in got.records.dtype.names:
        assert got.records[name].tobytes() == want.records[name].tobytes(), name
    assert got.summary.tobytes() == want.summary.tobytes()
    p.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. the tables between runs
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enhance", [True, False], ids=["enhance", "raw"])
def test_set_bayer_tables_between_runs(gpu_ctx, enhance):
    from chessboard_vision_amd.stream import BoardPipeline
    fmt, bits, n = "bayer_rggb10p", 10, 4
    raw, bgr_a, dev_a = _frames("game", n, fmt, "develop", bits)
    _, bgr_b, dev_b = _frames("game", n, fmt, "random", bits)
    pts = S.scaled_corners(W, H)

    def fresh(dev):
        p = BoardPipeline(W, H, n)
        p.configure(pts, profile=S.SHIPPED_PROFILE, enhance=enhance, lanes=2)
        p.set_input_format(fmt, develop=dev)
        return p

    def feed_and_run(p):
        ring = p.host_ring()
        for i in range(n):
            ring[i] = raw[i]
        p.submit(0, n)
        p.run(0, n)
        return _everything(p, n, True), [p.download(0, i) for i in range(n)]

    p = fresh(dev_a)
    first, frames = feed_and_run(p)
    for i in range(n):
        _assert_same(frames[i], bgr_a[i], "tables A, slot %d" % i)
    # other tables: what a fresh pipeline with them computes from the same frames
    p.set_develop(dev_b)
    p.reset_state()
    second, frames = feed_and_run(p)
    for i in range(n):
        _assert_same(frames[i], bgr_b[i], "tables B, slot %d" % i)
    q = fresh(dev_b)
    want, _ = feed_and_run(q)
    q.close()
    assert second == want and second != first
    # None restores the default, the neutral table
    p.set_develop(None)
    p.submit(0, 1)
    p.run(0, 1)
    _assert_same(p.download(0, 0), RD.expected(raw[0], fmt, RD.neutral(bits), bits), "the default again")
    p.close()
    # detector state is kept: calibrate the ChangeDetector, set identical tables, and nothing moves against a pipeline that made
    # the same calls but that one
    noise = _frames("noise", n, fmt, "develop", bits)[0]

    def calibrated(change_tables):
        p = fresh(dev_a)
        feed_and_run(p)
        p.calibrate_changes(0)
        p.run(0, n)
        if change_tables:
            p.set_develop(_tables("develop", bits)[1].copy())      # the same tables, as an array
        ring = p.host_ring()
        for i in range(1, n):                                      # frames that differ from the model everywhere
            ring[i] = noise[i]
        p.submit(0, n)
        p.run(0, n)
        out = _everything(p, n, True)
        changed = [r.changed for r in p.results(0, n)]
        p.close()
        return out, changed

    got, changed = calibrated(True)
    want, _ = calibrated(False)
    assert got == want
    assert changed[0] == 0 and all(changed[1:]), "the model of slot 0 is in force: the noise frames report changes against it"


# ------------------------------------------------------------------------------------------------------------------
# 6. launch counts
# ------------------------------------------------------------------------------------------------------------------
def test_launch_counts(gpu_ctx):
    from chessboard_vision_amd.stream import BoardPipeline
    n = 4
    pts = S.scaled_corners(W, H)
    # with enhancement a submit launches the new ingest once, and nothing of the 8-bit path
    for fmt in ("bayer_rggb16", "bayer_bggr10p", "bayer_grbg12p"):
        p = BoardPipeline(W, H, n)
        p.configure(pts, profile=S.SHIPPED_PROFILE)
        p.set_input_format(fmt)
        p.host_ring()[:] = 77
        p.submit(0, n)
        p.run(0, n)  # warm-up
        p.results(0, n)
        assert _counted(gpu_ctx, lambda: (p.submit(0, n), p.wait_submitted())) == {"INGEST_BAYER_DEEP": 1}, fmt
        p.close()
    # raw mode: a submit launches nothing; a run launches the new warp and neither k_ingest nor k_warp nor the 8-bit raw warp
    for attached in (0, 1):
        for fmt, kw in (("bayer_rggb10p", dict(enhance=False)), ("bayer_gbrg12p", dict(enhance="profile", raw=True, profile=S.SHIPPED_PROFILE))):
            p = BoardPipeline(W, H, n)
            p.configure(pts, lanes=2, **kw)
            if attached:
                p.add_board(pts + np.float32(3))
            p.set_input_format(fmt)
            assert bool(p.frames_ptr()) == (kw["enhance"] is False)          # enhance=False keeps its idle BGR ring, the profile mode holds none
            p.host_ring()[:] = 77
            p.submit(0, n)
            p.run(0, n)  # warm-up
            p.results(0, n)
            assert _counted(gpu_ctx, lambda: (p.submit(0, n), p.wait_submitted())) == {}
            c = _counted(gpu_ctx, lambda: (p.run(0, n), p.results(0, n)))
            assert c.get("WARP_BAYER_DEEP", 0) >= 1 and not {"INGEST", "INGEST_BAYER_DEEP", "WARP", "WARP_YUV"} & set(c), (fmt, attached, c)
            p.close()
    # the default path launches neither new kernel: 8-bit mosaics without tables, with enhancement and in raw mode
    for kw in (dict(profile=S.SHIPPED_PROFILE), dict(enhance=False)):
        p = BoardPipeline(W, H, n)
        p.configure(pts, **kw)
        p.set_input_format("bayer_grbg")
        p.host_ring()[:] = 77
        c = _counted(gpu_ctx, lambda: (p.submit(0, n), p.run(0, n), p.results(0, n)))
        assert not {"INGEST_BAYER_DEEP", "WARP_BAYER_DEEP"} & set(c) and ("INGEST" in c) == ("enhance" not in kw) and ("WARP_YUV" in c) == ("enhance" in kw), c
        # ... and with tables both take the new kernels
        p.set_develop(_tables("random", 8)[0])
        c = _counted(gpu_ctx, lambda: (p.submit(0, n), p.run(0, n), p.results(0, n)))
        assert ("INGEST_BAYER_DEEP" in c) == ("enhance" not in kw) and ("WARP_BAYER_DEEP" in c) == ("enhance" in kw) and "INGEST" not in c and "WARP_YUV" not in c, c
        p.close()


# ------------------------------------------------------------------------------------------------------------------
# 7. refusals, with nothing changed afterwards
# ------------------------------------------------------------------------------------------------------------------
def _raw_struct(fmt_id, buf, stride=None):
    from chessboard_vision_amd import _native as N
    r = N.RawFrame()
    r.fmt, r.stride0, r.plane0 = fmt_id, buf.strides[0] if stride is None else stride, buf.ctypes.data
    return r


@pytest.mark.parametrize("size", [(322, 240), (321, 240), (320, 241), (2, 240), (320, 2)], ids=lambda s: "%dx%d" % s)
def test_sizes_are_refused_and_nothing_changes(gpu_ctx, size):
    """w % 4 == 2 (RAW10 only), odd sizes and sizes below 4 (every encoding)"""
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.stream import BoardPipeline
    w, h = size
    lib = gpu_ctx.lib
    p = BoardPipeline(w, h, 2)
    frame = np.random.default_rng(2).integers(0, 256, (h, w, 3), dtype=np.uint8)
    p.upload(0, frame)
    only_10p = size == (322, 240)
    buf = np.zeros((h, 2 * w + 8), np.uint8)
    out = np.zeros((h, w, 3), np.uint8)
    for lay in LAYOUTS:
        for enc in ENCS:
            fid = RD.IDS[lay + enc]
            r = _raw_struct(fid, buf)
            if only_10p and enc != "10p":
                continue
            assert lib.cbv_pipeline_set_input_format(p.h_, fid) == ARG, (lay, enc)
            assert b"cbv_pipeline_set_input_format" in lib.cbv_last_error(gpu_ctx.h)
            assert lib.cbv_pipeline_upload_raw(p.h_, 0, r) == ARG
            assert lib.cbv_yuv_to_bgr(gpu_ctx.h, r, w, h, N.ptr(out), w * 3) == ARG
            assert lib.cbv_bayer_to_bgr(gpu_ctx.h, r, w, h, None, 0, N.ptr(out), w * 3) == ARG
    assert not out.any()
    assert p.input_format == "bgr" and lib.cbv_pipeline_host_slot_bytes(p.h_) == (w * h * 3 + 255) // 256 * 256
    _assert_same(p.download(0, 0), frame, "slot 0 after the refusals")
    if only_10p:                      # ... while the encodings that take the width are still taken
        p.set_input_format("bayer_rggb12p")
        assert p.host_ring().shape == (2, h, 3 * w // 2)
        p.set_input_format("bayer_rggb16")
        assert p.host_ring().shape == (2, h, w) and p.host_ring().dtype == np.uint16
    p.close()


def test_strides_bits_handles_and_ids_are_refused_and_nothing_changes(gpu_ctx):
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.stream import BoardPipeline
    lib = gpu_ctx.lib
    pts = S.scaled_corners(W, H)
    p = BoardPipeline(W, H, 2)
    p.configure(pts, profile=S.SHIPPED_PROFILE)
    board = p.add_board(pts + np.float32(2))
    frame = np.random.default_rng(3).integers(0, 256, (H, W, 3), dtype=np.uint8)
    p.upload(0, frame)
    out = np.zeros((H, W, 3), np.uint8)
    buf = np.zeros((H, 2 * W), np.uint8)
    t16 = np.zeros((3, 1 << 16), np.uint8)

    def unchanged(fmt="bgr", slot=W * H * 3):
        assert p.input_format == fmt and lib.cbv_pipeline_host_slot_bytes(p.h_) == (slot + 255) // 256 * 256
        if fmt == "bgr":
            _assert_same(p.download(0, 0), frame, "slot 0 after the refusals")
        assert not out.any()

    # a stride below the row bytes
    for enc in ENCS:
        r = _raw_struct(RD.IDS["bayer_rggb" + enc], buf, RD.row_bytes(enc, W) - 1)
        assert lib.cbv_pipeline_upload_raw(p.h_, 0, r) == ARG, enc
        assert lib.cbv_yuv_to_bgr(gpu_ctx.h, r, W, H, N.ptr(out), W * 3) == ARG
        assert lib.cbv_bayer_to_bgr(gpu_ctx.h, r, W, H, None, 0, N.ptr(out), W * 3) == ARG
    # bits that do not go with the encoding: 12 on 10p, 8 on the container, 11 anywhere
    for enc, bad in (("10p", 12), ("10p", 11), ("12p", 10), ("12p", 11), ("16", 8), ("16", 11), ("16", 13)):
        r = _raw_struct(RD.IDS["bayer_rggb" + enc], buf)
        assert lib.cbv_bayer_to_bgr(gpu_ctx.h, r, W, H, N.ptr(t16), bad, N.ptr(out), W * 3) == ARG, (enc, bad)
    r8 = _raw_struct(RB.IDS["bayer_rggb"], buf)
    assert lib.cbv_bayer_to_bgr(gpu_ctx.h, r8, W, H, N.ptr(t16), 10, N.ptr(out), W * 3) == ARG
    # not a Bayer id
    assert lib.cbv_bayer_to_bgr(gpu_ctx.h, _raw_struct(N.FMT_YUYV, buf), W, H, None, 0, N.ptr(out), W * 3) == ARG
    unchanged()
    # tables on a BGR and on an NV12 pipeline
    assert lib.cbv_pipeline_set_bayer_tables(p.h_, N.ptr(t16), 16) == STATE
    p.set_input_format("nv12")
    assert lib.cbv_pipeline_set_bayer_tables(p.h_, N.ptr(t16), 16) == STATE and lib.cbv_pipeline_set_bayer_tables(p.h_, None, 0) == STATE
    with pytest.raises(RuntimeError, match=r"not a Bayer format.*code -4\)"):
        p.set_develop(None)
    with pytest.raises(ValueError):
        p.set_input_format("nv12", develop=np.zeros((3, 256), np.uint8))
    p.set_input_format("bgr")
    # a board handle
    assert lib.cbv_pipeline_set_bayer_tables(board.h_, None, 0) == STATE
    for enc in ENCS:
        assert lib.cbv_pipeline_set_input_format(board.h_, RD.IDS["bayer_rggb" + enc]) == STATE
        assert lib.cbv_pipeline_upload_raw(board.h_, 0, _raw_struct(RD.IDS["bayer_rggb" + enc], buf)) == STATE
    # colour-space bits on the new ids, ids with an unassigned encoding field, the field on other families
    bad_ids = [RD.IDS["bayer_rggb10p"] | N.CS_FULL, RD.IDS["bayer_gbrg16"] | N.CS_BT709, RD.IDS["bayer_bggr12p"] | N.CS_MASK,
               0x4004, 0x5014, 0xF034, 0x8004, 0x1000, 0x1001, 0x2002, 0x3008, 0x1044, 0x2005, 0x10004]
    for bad in bad_ids:
        assert lib.cbv_pipeline_set_input_format(p.h_, bad) == ARG, hex(bad)
        assert b"cbv_pipeline_set_input_format" in lib.cbv_last_error(gpu_ctx.h)
        r = _raw_struct(bad, buf)
        assert lib.cbv_pipeline_upload_raw(p.h_, 0, r) == ARG, hex(bad)
        assert lib.cbv_yuv_to_bgr(gpu_ctx.h, r, W, H, N.ptr(out), W * 3) == ARG, hex(bad)
        assert lib.cbv_bayer_to_bgr(gpu_ctx.h, r, W, H, None, 0, N.ptr(out), W * 3) == ARG, hex(bad)
    for bad in (0x44, 0x05, 0x104):                                    # (tests/test_gpu_bayer.py's, still refused)
        assert lib.cbv_pipeline_set_input_format(p.h_, bad) == ARG, hex(bad)
    unchanged()
    # bits on a pipeline: refused, and the tables in force stay in force
    p.set_input_format("bayer_rggb10p", develop=_tables("random", 10)[0])
    raw, bgr, _ = _frames("noise", 1, "bayer_rggb10p", "random", 10)
    for bad in (12, 11, 8, 16):
        assert lib.cbv_pipeline_set_bayer_tables(p.h_, N.ptr(t16), bad) == ARG, bad
        assert b"cbv_pipeline_set_bayer_tables" in lib.cbv_last_error(gpu_ctx.h)
    with pytest.raises(ValueError):
        p.set_develop(np.zeros((3, 4096), np.uint8))
    p.upload(0, raw[0], fmt="bayer_rggb10p")
    _assert_same(p.download(0, 0), bgr[0], "the tables set before the refusals")
    assert p.input_format == "bayer_rggb10p" and lib.cbv_pipeline_host_slot_bytes(p.h_) == (W * 5 // 4 * H + 255) // 256 * 256
    # raw mode takes its own format only
    q = BoardPipeline(W, H, 2)
    q.configure(pts, enhance=False)
    q.set_input_format("bayer_rggb10p")
    for other, shape, dt in (("bayer_rggb12p", (H, W * 3 // 2), np.uint8), ("bayer_rggb", (H, W), np.uint8), ("bayer_bggr10p", (H, W * 5 // 4), np.uint8),
                             ("bayer_rggb16", (H, W), np.uint16)):
        with pytest.raises(RuntimeError, match=r"raw mode.*code -4\)"):
            q.upload(0, np.zeros(shape, dt), fmt=other)
    with pytest.raises(RuntimeError, match="no raw frame"):
        q.run(0, 1)
    q.close()
    p.close()


def test_single_frame_raw_warps_refuse_the_new_encodings(gpu_ctx):
    from chessboard_vision_amd import _native as N
    lib = gpu_ctx.lib
    w, h = 64, 48
    M = np.eye(3)
    out = np.zeros((32, 32, 3), np.uint8)
    prof = N.ColorProfile.from_dict(None)
    lens = N.LensStruct(1, 0, 60.0, 60.0, 32.0, 24.0, -0.2, 0.05, 0.0, 0.0, 0.0)
    buf = np.zeros((h, 2 * w), np.uint8)
    for enc in ENCS:
        r = _raw_struct(RD.IDS["bayer_grbg" + enc], buf)
        assert lib.cbv_warp_color_profile_raw(gpu_ctx.h, r, w, h, prof, N.ptr(M), 32, 32, 0, N.ptr(out), 96) == ARG, enc
        assert b"pipeline" in lib.cbv_last_error(gpu_ctx.h)
        assert lib.cbv_warp_lens(gpu_ctx.h, r, w, h, prof, lens, N.ptr(M), 32, 32, 0, N.ptr(out), 96) == ARG, enc
        assert lib.cbv_warp_lens(gpu_ctx.h, r, w, h, prof, None, N.ptr(M), 32, 32, 0, N.ptr(out), 96) == ARG, enc
    assert not out.any()
    # ... while the 8-bit id is still taken
    r = _raw_struct(RB.IDS["bayer_grbg"], buf, w)
    assert lib.cbv_warp_color_profile_raw(gpu_ctx.h, r, w, h, prof, N.ptr(M), 32, 32, 0, N.ptr(out), 96) == 0
