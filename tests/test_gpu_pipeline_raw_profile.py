"""The raw-frame profile mode of the pipeline (configure(enhance="profile", raw=True), CBV_SKIP_ENHANCE_PROFILE_RAW:
k_warp_raw_profile in the run and in the colour sweep) and the profile per board (set_profile, add_board(profile=...)).
640 x 480 frames throughout: color_sweep_ref's frames and corners, turned into NV12 / YUYV / Bayer frames by
tests/raw_profile_ref.py.  The yardstick is the oracle's apply_color_profile -> warp_image on the int64 conversion of those
raw frames, and the restated reference class (ref_logic.RefPieceDetector) on its boards; the same pipeline in mode 2, which
converts the raw frames into its BGR ring, must agree with mode 3 to the byte in everything a board reports (square
statistics and NoiseHandler records are compared between the two modes; the boards and the eight result words against the
yardstick as well).  Tolerance 0."""
import functools

import numpy as np
import pytest

from chessboard_vision_amd import _native as Nat
from chessboard_vision_amd import synth as S
import color_sweep_ref as CS
import piece_sweep_ref as PS
import raw_profile_ref as RP

pytestmark = pytest.mark.gpu

ARG, STATE, UNSUPPORTED = -1, -4, -5
W, H = CS.W, CS.H
N10 = 10
PTS = S.scaled_corners(W, H)
GRID = (tuple(S.CALIB_GRID_X), tuple(S.CALIB_GRID_Y))
FMTS = ("nv12", "yuyv", "bayer_grbg")
PROFS = [CS.PROFILES[name] for name in CS.NAMES]
BLACK = {"contrast": 0.0, "brightness": 0}  # every pixel black: no square holds a piece under it
PROFILES = dict(CS.PROFILES, black=BLACK)
# (chunk, lanes, the runs): a chunk of 10 takes the many-frames-per-thread form with a short last group
CONFIGS = ((1, 1, (10,)), (4, 2, (10,)), (10, 1, (10,)), (4, 1, (3, 7)), (10, 2, (10,)))
_same = PS.same_records


# --- the yardstick ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _raw(palette, fmt, i):
    r = RP.from_bgr(np.array(CS.frame(palette, i)), fmt)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _converted(palette, fmt, i):
    return np.array(CS.frame(palette, i)) if fmt == "bgr" else np.ascontiguousarray(RP.to_bgr(_raw(palette, fmt, i), fmt))


@functools.lru_cache(maxsize=None)
def _board(palette, fmt, name, i):
    """warp_image(apply_color_profile(to_bgr(raw frame i)))"""
    from oracle import cbv_oracle as O
    w = O.warp_image(CS.profiled(_converted(palette, fmt, i), PROFILES[name]), PTS)[0]
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _ref_words(palette, fmt, names, grid=None):
    """the eight result words of every frame: RefPieceDetector driven as the pipeline drives it (use_delta=True, nothing
    checked) on the yardstick's boards; names[i] = the profile frame i is seen through (the ChangeDetector words are 0:
    nothing is calibrated)"""
    from ref_logic import RefPieceDetector
    det, ge = RefPieceDetector(hough=PS.hough_kw(CS.HOUGH)), CS.extractor(grid)
    out = []
    for i, name in enumerate(names):
        res, vis = det.detect_all_pieces(ge.split_board(_board(palette, fmt, name, i)), use_delta=True)
        out.append((PS.bits(p for p, r in det.cached_results.items() if r["has_piece"]), PS.bits(p for p, r in res.items() if r["has_piece"]),
                    PS.bits(vis), PS.bits(det.last_processed)) + (0, 0, 0, 0))
    return out


# --- the pipelines ---------------------------------------------------------------------------------------------------------
def _feed(p, palette, fmt, n, ring=False):
    if fmt != "bgr":
        p.set_input_format(fmt)
    if ring:
        host = p.host_ring()
        for i in range(n):
            host[i] = _raw(palette, fmt, i) if fmt != "bgr" else CS.frame(palette, i)
        p.submit(0, n)
    else:
        for i in range(n):
            p.upload(i, _raw(palette, fmt, i) if fmt != "bgr" else CS.frame(palette, i), fmt=fmt)


def _pipeline(fmt, mode, profile, palette="low", n=N10, chunk=4, lanes=2, ring=False, run=False, **kw):
    """mode 3: enhance="profile", raw=True; 2: enhance="profile"; 1: enhance=False; 0: enhance=True"""
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, n)
    p.configure(PTS, profile=profile, chunk=chunk, lanes=lanes, **_mode(mode), **kw)
    _feed(p, palette, fmt, n, ring)
    if run:
        p.run(0, n)
    return p


def _mode(mode):
    return {0: dict(enhance=True), 1: dict(enhance=False), 2: dict(enhance="profile"), 3: dict(enhance="profile", raw=True)}[mode]


def _words(res):
    return [(r.raw_occupied, r.stable_occupied, r.visual_changes, r.processed, r.changed, r.parcial, r.total, r.circular) for r in res]


def _snapshot(b, n=N10, s0=0):
    return (bytes(b.results(s0, n)), [bytes(b.square_stats(s0 + i)) for i in range(n)], [bytes(b.hough(s0 + i)) for i in range(n)],
            [b.download(2, s0 + i).tobytes() for i in range(n)], [(st.name, sorted(d.items(), key=str)) for st, d in b.noise_results(s0, n)])


def _to_bgr(raw, fmt):
    from chessboard_vision_amd.board_detection import bayer_to_bgr, yuv_to_bgr
    return bayer_to_bgr(raw, fmt) if fmt.startswith("bayer") else yuv_to_bgr(raw, fmt)


# 1 --- mode 3 against mode 2 and the yardstick -------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_mode_3_equals_mode_2_and_the_yardstick(gpu_ctx, fmt):
    """the lilac palette under its radical profile: there the pieces' moves change the words within ten frames"""
    pal, name = "lilac", "radical_lilac"
    want = _ref_words(pal, fmt, (name,) * N10)
    assert len({w_[1] for w_ in want}) > 1 and any(w_[2] for w_ in want[1:])  # pieces move, changes are seen
    assert not np.array_equal(_board(pal, fmt, name, 0), _board(pal, fmt, "none", 0))  # the profile acts
    snaps = []
    for mode in (3, 2):
        for ring in (False, True):
            p = _pipeline(fmt, mode, CS.PROFILES[name], palette=pal, ring=ring)
            for chunk, lanes, split in CONFIGS:
                p.configure(PTS, profile=CS.PROFILES[name], chunk=chunk, lanes=lanes, **_mode(mode))
                s0 = 0
                for cnt in split:
                    p.run(s0, cnt)
                    s0 += cnt
                got = _words(p.results(0, N10))
                assert got == want, (fmt, mode, ring, chunk, lanes, split, [i for i in range(N10) if got[i] != want[i]])
                for i in range(N10):
                    assert np.array_equal(p.download(2, i), _board(pal, fmt, name, i)), (fmt, mode, ring, chunk, lanes, split, i)
                snaps.append(((mode, ring, chunk, lanes, split), _snapshot(p)))
            # the frame itself, unprofiled: converted on demand in mode 3
            for i in (0, N10 - 1):
                assert np.array_equal(p.download(0, i), _to_bgr(_raw(pal, fmt, i), fmt)), (fmt, mode, i)
                assert np.array_equal(p.download(0, i), _converted(pal, fmt, i))
            if mode == 3:  # the raw ring is the only frame store
                with pytest.raises(RuntimeError, match=r"code -4\b"):
                    p.upload(0, CS.frame(pal, 0))
                with pytest.raises(RuntimeError, match=r"code -4\b"):
                    p.synth(0, 1)
                with pytest.raises(RuntimeError, match=r"code -4\b"):
                    other = "yuyv" if fmt == "nv12" else "nv12"
                    p.upload(0, _raw(pal, other, 0), fmt=other)
                with pytest.raises(RuntimeError, match=r"code -4\b"):
                    p.download(1, 0)
            p.close()
    for what, snap in snaps[1:]:
        assert snap == snaps[0][1], (fmt, what)


@pytest.mark.parametrize("fmt", RP.FORMATS)
def test_the_many_frames_form_of_every_format(gpu_ctx, fmt):
    """a chunk of 10 frames (groups of four or two frames a thread with a short last group, by family) in every raw format,
    one board (k_warp_raw_profile) and with a smaller, rotated board attached (k_warp_raw_profile_mb): the yardstick's
    boards, and everything the same boards report in mode 2"""
    snaps = {}
    for mode in (3, 2):
        p = _pipeline(fmt, mode, CS.PROFILES["radical"], chunk=N10, lanes=1, run=True)
        snaps[mode, 1] = _snapshot(p)
        b = p.add_board(PTS + np.float32(3), rot180=True, display_size=(800, 600), profile=CS.PROFILES["sat3"])
        p.run(0, N10)
        snaps[mode, 2] = [_snapshot(p), _snapshot(b)]
        if mode == 3:
            for i in (0, 7, 9):
                assert np.array_equal(p.download(2, i), _board("low", fmt, "radical", i)), (fmt, i)
        b.close()
        p.close()
    assert snaps[3, 1] == snaps[2, 1] and snaps[3, 2] == snaps[2, 2], fmt
    assert snaps[3, 2][1][3][0] != snaps[3, 2][0][3][0]


def test_rotated_and_bgr_input(gpu_ctx):
    """rot180 in mode 3; and with BGR input 3 is 2: the BGR ring, upload and synth as ever"""
    from oracle import cbv_oracle as O
    p = _pipeline("nv12", 3, CS.SHIPPED, chunk=10, lanes=1, rot180=True, run=True)
    for i in (0, 9):
        assert np.array_equal(p.download(2, i), O.rotate180(_board("low", "nv12", "shipped", i))), i
    p.close()
    out = []
    for mode in (3, 2):
        p = _pipeline("bgr", mode, CS.SHIPPED, n=8)
        p.synth(0, 8, scene=CS.native_scene("low"), frames_per_ply=CS.FRAMES_PER_PLY)
        p.upload(0, CS.frame("low", 0))
        p.run(0, 8)
        out.append(_snapshot(p, 8))
        assert np.array_equal(p.download(2, 5), CS.warped("low", "shipped", 5))
        p.close()
    assert out[0] == out[1]


def test_mode_3_holds_no_bgr_ring(gpu_ctx):
    """the raw ring holds every byte: in mode 3 with raw frames there is no BGR ring; it is back when the mode or the input
    format needs it, and what the pipeline computes does not depend on the way it got there"""
    p = _pipeline("nv12", 3, CS.SHIPPED, run=True)
    assert not p.frames_ptr()
    want = _snapshot(p)
    p.configure(PTS, profile=CS.SHIPPED, chunk=4, lanes=2, enhance="profile")  # mode 2: converts into a BGR ring
    assert p.frames_ptr()
    _feed(p, "low", "nv12", N10)
    p.run(0, N10)
    assert _snapshot(p) == want
    p.configure(PTS, profile=CS.SHIPPED, chunk=4, lanes=2, enhance="profile", raw=True)
    assert not p.frames_ptr()
    _feed(p, "low", "nv12", N10, ring=True)
    p.run(0, N10)
    assert _snapshot(p) == want
    p.set_input_format("bgr")  # with BGR input 3 is 2
    assert p.frames_ptr()
    for i in range(N10):
        p.upload(i, _converted("low", "nv12", i))
    p.run(0, N10)
    assert _snapshot(p)[3] == want[3]
    p.close()
    q = _pipeline("nv12", 1, None)  # skip_enhance = 1 keeps its ring in raw mode, as it always did
    assert q.frames_ptr()
    q.close()


# 2 --- launch counts -----------------------------------------------------------------------------------------------------------
ENHANCEMENT = ("COLOR_LAB_HIST", "CLAHE_LUT", "CLAHE_APPLY", "BILATERAL", "SHARPEN", "NORM_LUT", "NORMALIZE", "RESET")
# Launches per kernel of one run of 12 frames (chunk 4, one lane: three chunks) after a warm-up run, counted on the commit
# before this feature: mode 0 as tests/test_gpu_session_chain.py wrote it down, modes 1 and 2 what is left of it without the
# enhancement (tests/test_gpu_color_sweep.py::test_off_means_off holds mode 2 to mode 1).
PARENT_COUNTS = {0: {"COLOR_LAB_HIST": 3, "CLAHE_LUT": 3, "CLAHE_APPLY": 3, "BILATERAL": 3, "SHARPEN": 3, "NORM_LUT": 3, "WARP": 3,
                     "SQUARES": 3, "SCAN": 1, "HOUGH": 3}}
PARENT_COUNTS[1] = PARENT_COUNTS[2] = {"WARP": 3, "SQUARES": 3, "SCAN": 1, "HOUGH": 3}


def _counted(ctx, p, n, submit=False):
    p.run(0, n)
    p.results(0, n)
    ctx.profile_reset()
    ctx.profile_enable(-1)
    try:
        if submit:
            p.submit(0, n)
        p.run(0, n)
        p.results(0, n)
        return {k: ctx.profile_read(kid)[1] for k, kid in Nat.K_ALL.items() if ctx.profile_read(kid)[1]}
    finally:
        ctx.profile_enable(-2)
        ctx.profile_reset()


def test_launch_counts(gpu_ctx):
    from chessboard_vision_amd.stream import BoardPipeline
    n = 12

    def make(mode, profile=S.SHIPPED_PROFILE):
        p = BoardPipeline(W, H, n)
        p.configure(PTS, profile=profile, chunk=4, lanes=1, **_mode(mode))
        return p
    for mode in (0, 1, 2):
        p = make(mode)
        p.synth(0, n, scene="normal", frames_per_ply=2)
        assert _counted(gpu_ctx, p, n) == PARENT_COUNTS[mode], mode
        p.close()
    for fmt in FMTS:
        for profile in (S.SHIPPED_PROFILE, None):  # the profile kernel and, with a disabled profile, the plain raw warp
            p = make(3, profile)
            p.set_input_format(fmt)
            p.host_ring()[:] = 128
            p.submit(0, n)
            got = _counted(gpu_ctx, p, n, submit=True)
            p.close()
            assert got == {"WARP_YUV": 3, "SQUARES": 3, "SCAN": 1, "HOUGH": 3}, (fmt, profile, got)  # no k_ingest, no k_warp
    # mode 2 fed NV12 converts as it did: one k_ingest per submit
    p = make(2)
    p.set_input_format("nv12")
    p.host_ring()[:] = 128
    p.submit(0, n)
    got = _counted(gpu_ctx, p, n, submit=True)
    p.close()
    assert got == dict(PARENT_COUNTS[2], INGEST=1), got


# 3 --- a profile per board -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,mode", [("bgr", 2), ("nv12", 3)], ids=["mode2_bgr", "mode3_nv12"])
@pytest.mark.parametrize("chunk", [4, 10])
def test_attached_boards_with_profiles_of_their_own(gpu_ctx, fmt, mode, chunk):
    """board 0 with the shipped profile, an attached board with the irregular 76 - 80 px grid and the radical profile, a
    second attached board with no profile: each is a pipeline of its own configured with that profile"""
    p = _pipeline(fmt, mode, CS.SHIPPED, chunk=chunk)
    b1 = p.add_board(PTS, grid_lines=GRID, profile=CS.PROFILES["radical"])
    b2 = p.add_board(PTS, profile=None)
    b3 = p.add_board(PTS)  # not given: the pipeline's configured profile
    p.run(0, N10)
    assert len({(b1._cfg.rois[i].w, b1._cfg.rois[i].h) for i in range(64)}) > 1
    for b, name, grid in ((p, "shipped", None), (b1, "radical", GRID), (b2, "none", None), (b3, "shipped", None)):
        own = _pipeline(fmt, mode, CS.PROFILES[name], chunk=chunk, grid_lines=grid, run=True)
        assert _words(b.results(0, N10)) == _words(own.results(0, N10)) == _ref_words("low", fmt, (name,) * N10, grid), name
        for i in range(N10):
            assert np.array_equal(b.download(2, i), _board("low", fmt, name, i)), (name, i)
            assert np.array_equal(b.download(2, i), own.download(2, i)) and bytes(b.square_stats(i)) == bytes(own.square_stats(i)), (name, i)
        own.close()
    assert not np.array_equal(b1.download(2, 0), p.download(2, 0)) and not np.array_equal(b2.download(2, 0), p.download(2, 0))
    # every board's profile switched off: the plain warp is launched again, and the boards are the unprofiled ones
    for b in (p, b1, b3):
        b.set_profile(None)
    p.run(0, N10)
    for b in (p, b1, b2, b3):
        assert np.array_equal(b.download(2, 3), _board("low", fmt, "none", 3))
    # ... and one of them on again, beside disabled ones
    b2.set_profile(CS.PROFILES["sat3"])
    p.run(0, N10)
    assert np.array_equal(b2.download(2, 3), _board("low", fmt, "sat3", 3)) and np.array_equal(p.download(2, 3), _board("low", fmt, "none", 3))
    for q in (b1, b2, b3, p):
        q.close()


# 4 --- set_profile between runs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,mode", [("bgr", 2), ("nv12", 3)], ids=["mode2_bgr", "mode3_nv12"])
def test_set_profile_between_runs_keeps_the_state(gpu_ctx, fmt, mode):
    """five frames under a profile that blackens the frame, then the shipped one: from that frame on the warped boards are a
    fresh pipeline's, and the detector history is kept: the words are the reference class's on that sequence of boards, whose
    stable occupancy lags a reset pipeline's; the ChangeDetector model stays what calibrate made it"""
    k = 5
    names = ("black",) * k + ("shipped",) * (N10 - k)
    want = _ref_words("low", fmt, names)
    p = _pipeline(fmt, mode, BLACK)
    p.run(0, k)
    p.calibrate_changes(k - 1)
    model = [p.model((0, 0))[j].tobytes() for j in (0, 1)]
    p.set_profile(CS.SHIPPED)
    p.run(k, N10 - k)
    got = _words(p.results(0, N10))
    assert [g[:4] for g in got] == [w_[:4] for w_ in want], [i for i in range(N10) if got[i][:4] != want[i][:4]]
    assert [p.model((0, 0))[j].tobytes() for j in (0, 1)] == model
    assert any(g[4] for g in got[k:])  # calibrated on a black board: the ChangeDetector sees the profile change
    fresh = _pipeline(fmt, mode, CS.SHIPPED, run=True)
    for i in range(k, N10):
        assert np.array_equal(p.download(2, i), fresh.download(2, i)) and np.array_equal(p.download(2, i), _board("low", fmt, "shipped", i)), i
    for i in range(k):
        assert not p.download(2, i).any()
    fresh.close()
    reset = _pipeline(fmt, mode, CS.SHIPPED)
    reset.run(k, N10 - k)
    lag = [(g[1], r[1]) for g, r in zip(got[k:], _words(reset.results(k, N10 - k)))]
    assert lag[0][0] == 0 and lag[0][1] != 0 and lag[-1][0] != 0, lag  # three of five frames must show the piece
    reset.close()
    # a rejected profile changes nothing
    with pytest.raises(RuntimeError, match=r"code -1\b"):
        p.set_profile(dict(CS.SHIPPED, sat_scale=float("nan")))
    p.run(k, N10 - k)
    assert np.array_equal(p.download(2, N10 - 1), _board("low", fmt, "shipped", N10 - 1))
    p.close()


def test_set_profile_needs_a_profile_mode(gpu_ctx):
    for mode in (0, 1):
        p = _pipeline("bgr", mode, CS.SHIPPED, n=2)
        with pytest.raises(RuntimeError, match=r"code -4\b"):
            p.set_profile(CS.SHIPPED)
        with pytest.raises(RuntimeError, match=r"code -4\b"):
            p.add_board(PTS, profile=CS.SHIPPED)
        p.close()
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, 2)
    with pytest.raises(RuntimeError, match=r"code -4\b"):
        p.set_profile(CS.SHIPPED)  # not configured
    p.close()


# 5 --- the colour sweep on the raw ring ------------------------------------------------------------------------------------------
N8 = CS.N_FRAMES


@functools.lru_cache(maxsize=None)
def _yardstick_records(palette, fmt):
    """color_sweep_ref.run_profile on the converted frames: a fresh RefPieceDetector per profile, every square checked"""
    from ref_logic import RefPieceDetector
    rows = []
    for name in CS.NAMES:
        det, ge, row = RefPieceDetector(hough=PS.hough_kw(CS.HOUGH)), CS.extractor(None), []
        for i in range(N8):
            sq = ge.split_board(_board(palette, fmt, name, i))
            res, _ = det.detect_all_pieces(sq, use_smoothing=True, squares_to_check=set(sq.keys()))
            row.append(PS.record_of(res, {pos: dict(r) for pos, r in det.cached_results.items()}))
        rows.append(row)
    return rows


@pytest.fixture(scope="module", params=list(CS.PALETTES))
def swept(request, gpu_ctx):
    """A mode-3 NV12 pipeline that has run, its snapshot, and ONE sweep of the eleven profiles over the 8 frames"""
    p = _pipeline("nv12", 3, CS.SHIPPED, palette=request.param, n=N8, run=True)
    before = _snapshot(p, N8)
    res = p.color_sweep(0, N8, PROFS, expected=CS.expected_bits())
    yield request.param, p, res, before
    p.close()


def test_sweep_equals_the_yardstick_on_the_converted_frames(swept):
    palette, p, res, _ = swept
    Y = _yardstick_records(palette, "nv12")
    rec = res.records
    assert rec.shape == (len(PROFS), N8) and res.info["chunk_frames"] == N8 and res.info["chunk_profiles"] == len(PROFS)
    PS.assert_records_equal(rec, Y, "device against the reference class")
    exp = CS.expected_bits()
    want = PS.reduce_records(rec, exp, [[r["_radii"] for r in row] for row in Y])
    for name in PS.SUM_FIELDS:
        assert np.array_equal(res.summary[name], want[name]), name
    assert res.summary.tobytes() == want.tobytes()
    for j, name in enumerate(CS.NAMES):
        assert (int(res.summary["missed"][j]), int(res.summary["false_pos"][j]), int(res.summary["frames_exact"][j])) == CS.summary_of(Y[j], exp), name
    assert all(res.info[k] > 0 for k in ("warp_ms", "squares_ms", "hough_ms", "eval_ms"))


def test_sweep_equals_a_mode_2_pipelines(swept):
    palette, p, res, _ = swept
    exp = CS.expected_bits()
    q = _pipeline("nv12", 2, CS.SHIPPED, palette=palette, n=N8)
    got = q.color_sweep(0, N8, PROFS, expected=exp)
    assert _same(got.records, res.records) and got.summary.tobytes() == res.summary.tobytes()
    q.close()


def test_sweep_chunks_records_and_slot0(swept):
    palette, p, res, _ = swept
    exp = CS.expected_bits()
    for chunk in (1, 5, 16):
        got = p.color_sweep(0, N8, PROFS, expected=exp, chunk_frames=chunk)
        assert got.info["chunk_frames"] == min(chunk, N8)
        assert _same(got.records, res.records) and got.summary.tobytes() == res.summary.tobytes(), chunk
    only = p.color_sweep(0, N8, PROFS, expected=exp, records=False)
    assert only.records is None and only.summary.tobytes() == res.summary.tobytes()
    late = p.color_sweep(3, N8 - 3, PROFS[:4], expected=exp[3:])
    assert np.array_equal(late.raw_occupied, res.raw_occupied[:4, 3:]) and np.array_equal(late.hough, res.hough[:4, 3:])
    assert np.array_equal(late.stable_occupied[:, 4], res.stable_occupied[:4, 7])  # five frames on, the histories hold the same frames


def test_sweep_leaves_the_board_as_it_was(swept):
    palette, p, res, before = swept
    assert _snapshot(p, N8) == before
    p.run(0, N8)  # a later run continues from the state the first run left, not from anything the sweep touched
    q = _pipeline("nv12", 3, CS.SHIPPED, palette=palette, n=N8, run=True)
    q.run(0, N8)
    assert _snapshot(p, N8) == _snapshot(q, N8)
    q.close()


def test_sweep_the_way_round_and_the_refusal(gpu_ctx, swept):
    """a mode-3 pipeline with a disabled profile runs the plain raw warp and can sweep; a raw pipeline without a profile mode
    (enhance=False) still cannot"""
    palette, _, res, _ = swept
    q = _pipeline("nv12", 3, None, palette=palette, n=N8, run=True)
    assert np.array_equal(q.download(2, 2), _board(palette, "nv12", "none", 2))
    got = q.color_sweep(0, N8, PROFS, expected=CS.expected_bits())
    assert _same(got.records, res.records) and got.summary.tobytes() == res.summary.tobytes()
    q.close()
    q = _pipeline("nv12", 1, None, palette=palette, n=N8, run=True)
    profs = (Nat.ColorProfile * 1)(Nat.ColorProfile.from_dict(CS.SHIPPED))
    summ = np.zeros(1, Nat.record_dtype(Nat.PieceSweepSummary))
    assert q.ctx.lib.cbv_pipeline_color_sweep(q.h_, 0, 1, profs, 1, None, 0, None, Nat.ptr(summ), None) == UNSUPPORTED
    q.close()
