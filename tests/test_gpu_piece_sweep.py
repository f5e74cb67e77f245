"""The PieceDetector settings sweep on the device (cbv_pipeline_piece_sweep, cbv_pipeline_piece_detail; k_piece_sweep_hough
and k_piece_sweep_eval) against the yardstick of tests/piece_sweep_ref.py: the restated reference class driven setting by
setting, the recorded run of the reference's own class, the host twin, and the product's own per-setting path.  640x480, 12
frames, raw chain (enhance=False).  Tolerance 0.  tests/test_piece_sweep_host.py shows on the CPU what the settings reach."""
import random

import numpy as np
import pytest

from chessboard_vision_amd import _native as Nat
from chessboard_vision_amd import synth as S
import piece_sweep_ref as PS
import refrun

pytestmark = pytest.mark.gpu

ARG, STATE, UNSUPPORTED = -1, -4, -5
W, H, N = PS.W, PS.H, PS.N_FRAMES
PTS = S.scaled_corners(W, H)
SETTINGS = list(PS.SETTINGS)
ALL = [(f, r) for f in range(8) for r in range(8)]


def _pipeline(n=N, frames_per_ply=PS.FRAMES_PER_PLY, run=True, **kw):
    """A pipeline on the raw chain holding the yardstick stream, run once."""
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, n)
    p.configure(PTS, chunk=4, lanes=2, enhance=False, **kw)
    p.synth(0, n, scene=PS.native_scene(), frames_per_ply=frames_per_ply)
    if run:
        p.run(0, n)
    return p


_same = PS.same_records


def _snapshot(b, n=N):
    return (bytes(b.results(0, n)), [bytes(b.square_stats(i)) for i in range(n)], [bytes(b.hough(i)) for i in range(n)],
            [(st.name, sorted(d.items(), key=str)) for st, d in b.noise_results(0, n)])


@pytest.fixture(scope="module")
def swept(gpu_ctx):
    """The pipeline, its snapshot, and ONE sweep of the 18 settings over the 12 frames with the scripted positions."""
    p = _pipeline()
    before = _snapshot(p)
    res = p.piece_sweep(0, N, settings=SETTINGS, expected=PS.expected_bits())
    yield p, res, before
    p.close()


# 1 ------------------------------------------------------------------------------------------------------------------
def test_one_sweep_equals_the_yardsticks(swept):
    _, res, _ = swept
    rec = res.records
    Y = PS.yardstick_records()
    assert rec.shape == (len(SETTINGS), N) and res.info["param1_distinct"] == 3 and res.info["chunk_frames"] == N
    PS.assert_records_equal(rec, Y, "device against the reference class")
    exp = PS.expected_bits()
    want = PS.reduce_records(rec, exp, [[r["_radii"] for r in row] for row in Y])
    for name in PS.SUM_FIELDS:
        assert np.array_equal(res.summary[name], want[name]), name
    assert res.summary.tobytes() == want.tobytes()
    stats, ws, hs, ch = PS.oracle_inputs()
    h_rec, h_sum = PS.eval_host(stats, ws, hs, ch, exp)
    assert _same(rec, h_rec) and res.summary.tobytes() == h_sum.tobytes()
    assert not res.summary["overflow"].any() and not rec["flags"].any()  # param2 = 1 (setting 12) included
    assert res.best() == 0 and res.summary["frames_exact"][0] == 8
    # the recorded run of the reference's own class: has_piece of every row is the smoothed value, the method the raw one's
    fx = refrun.load_json("ref_piece_settings.json")
    for run in fx["runs"]:
        j = run["setting_index"]
        for i, rows in enumerate(run["frames"]):
            assert PS.bits((r[0], r[1]) for r in rows if r[2]) == int(rec["stable_occupied"][j, i]), (j, i)
            for m in PS.METHODS:
                assert PS.bits((r[0], r[1]) for r in rows if r[3] == m) == int(rec[m][j, i]), (j, i, m)
            assert res.occupied(j, i) == {(r[0], r[1]) for r in rows if r[2]}


# 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("j", [1, 11, 15], ids=lambda j: "%s-%s-%s-%s" % PS.SETTINGS[j])
def test_sweep_equals_the_per_setting_path(swept, j):
    """A board configured with the setting (use_hough=2: HoughCircles on every non-uniform square), every square in the
    check set of every slot, reports the sweep's raw and smoothed occupancy."""
    _, res, _ = swept
    lo, hi, p1, p2 = PS.SETTINGS[j]
    q = _pipeline(run=False, use_hough=2, min_radius_ratio=lo, max_radius_ratio=hi, hough_param1=p1, hough_param2=p2)
    q.reset_state()
    q.set_check_squares(0, [set(ALL)] * N)
    q.run(0, N)
    out = q.results(0, N)
    for i in range(N):
        assert (out[i].raw_occupied, out[i].stable_occupied) == (int(res.raw_occupied[j, i]), int(res.stable_occupied[j, i])), i
    assert any(out[i].raw_occupied != out[i].stable_occupied for i in range(N))
    q.close()


# 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("j", [0, 15], ids=lambda j: "%s-%s-%s-%s" % PS.SETTINGS[j])
def test_piece_detail_equals_detect_piece(swept, j):
    from ref_logic import detect_piece
    p, res, _ = swept
    sq = PS.stream_squares()
    seen = set()
    for i in (0, 9):
        got = p.piece_detail(i, **PS.hough_kw(PS.SETTINGS[j]))
        assert list(got) == PS.ROI_POS
        for pos in PS.ROI_POS:
            want = detect_piece(sq[i][pos], hough=PS.hough_kw(PS.SETTINGS[j]))[0]
            assert got[pos] == want, (i, pos, got[pos], want)
            seen.add(want["method"])
        assert PS.bits(pos for pos, r in got.items() if r["has_piece"]) == int(res.raw_occupied[j, i])
    assert seen >= ({None, "hough"} if j == 0 else {None, "tower_top", "center_diff"})


# 4 ------------------------------------------------------------------------------------------------------------------
def test_invariance(swept):
    p, res, _ = swept
    exp = PS.expected_bits()
    for chunk in (1, 5, 16):
        r = p.piece_sweep(0, N, settings=SETTINGS, expected=exp, chunk_frames=chunk)
        assert r.info["chunk_frames"] == min(chunk, N)
        assert _same(r.records, res.records) and r.summary.tobytes() == res.summary.tobytes(), chunk
    quiet = p.piece_sweep(0, N, settings=SETTINGS, expected=exp, records=False, chunk_frames=5)
    assert quiet.records is None and quiet.summary.tobytes() == res.summary.tobytes()
    order = list(range(len(SETTINGS)))
    random.Random(5).shuffle(order)
    sh = p.piece_sweep(0, N, settings=[SETTINGS[j] for j in order], expected=exp)
    assert _same(sh.records, res.records[order]) and sh.summary.tobytes() == res.summary[order].tobytes()
    dup = p.piece_sweep(0, N, settings=[SETTINGS[7], SETTINGS[12], SETTINGS[7], SETTINGS[0], SETTINGS[7]], expected=exp)
    pick = [7, 12, 7, 0, 7]
    assert _same(dup.records, res.records[pick]) and dup.summary.tobytes() == res.summary[pick].tobytes()
    one = p.piece_sweep(0, N, settings=[SETTINGS[11]], expected=exp)
    assert _same(one.records, res.records[[11]])
    # the product form of the settings, and a later start: the history begins with the call's first frame
    prod = p.piece_sweep(0, N, [.20, .25], [.55], param1s=(100,), param2s=(25, 30))
    assert _same(prod.records[[0, 2, 3]], res.records[[0, 1, 2]])
    late = p.piece_sweep(6, N - 6, settings=SETTINGS[:3])
    assert np.array_equal(late.raw_occupied, res.raw_occupied[:3, 6:]) and np.array_equal(late.stable_occupied[:, 0], late.raw_occupied[:, 0])
    assert not late.summary["frames_exact"].any()  # no `expected`


# 5 ------------------------------------------------------------------------------------------------------------------
def test_the_board_is_untouched(swept):
    """Results, noise results, statistics and HoughCircles records are byte for byte what they were, the model planes too;
    the reference planes and the temporal state have no getter: a run after a sweep equals the same run without it (its
    visual_changes are judged against the reference planes, its smoothed occupancy against the history)."""
    p, _, before = swept
    assert _snapshot(p) == before
    a, b = _pipeline(run=False), _pipeline(run=False)
    for q in (a, b):
        q.run(0, 1)
        q.calibrate_changes(0)
        q.run(1, 5)
    planes = {pos: a.model(pos) for pos in ALL}
    ra = a.piece_sweep(0, 6, settings=SETTINGS)
    assert all(np.array_equal(planes[pos][k], a.model(pos)[k]) for pos in ALL for k in (0, 1))
    for q in (a, b):
        q.run(6, N - 6)
    assert _snapshot(a) == _snapshot(b)
    assert any(r.changed for r in a.results(1, N - 1))  # the calibrated stage is live in the runs compared
    assert _same(ra.records, swept[1].records[:, :6])
    a.close()
    b.close()


# 6 ------------------------------------------------------------------------------------------------------------------
GEOMETRY_SETTINGS = (0, 5, 11, 12, 15)


def test_an_attached_board_with_irregular_squares(gpu_ctx):
    """SmartGridExtractor squares of 76..80 px: the integer radii differ from square to square"""
    grid = (tuple(S.CALIB_GRID_X), tuple(S.CALIB_GRID_Y))
    sets = tuple(PS.SETTINGS[j] for j in GEOMETRY_SETTINGS)
    n = 6
    p = _pipeline(run=False)
    b = p.add_board(PTS, grid_lines=grid)
    p.run(0, n)
    sizes = {(b._cfg.rois[i].w, b._cfg.rois[i].h) for i in range(64)}
    assert len(sizes) > 1 and len({int(min(w, h) * 0.34) for w, h in sizes}) > 1
    got = b.piece_sweep(0, n, settings=list(sets), expected=PS.expected_bits(n))
    PS.assert_records_equal(got.records, PS.yardstick_records(n=n, grid=grid, settings=sets), "attached board, irregular grid")
    assert not got.summary["overflow"].any()
    base = p.piece_sweep(0, n, settings=list(sets), expected=PS.expected_bits(n))
    assert not _same(base.records, got.records)  # the other grid does see other squares
    b.close()
    p.close()


def test_squares_of_100_px(gpu_ctx):
    sets = tuple(PS.SETTINGS[j] for j in GEOMETRY_SETTINGS)
    n = 6
    p = _pipeline(run=False, display_size=(1280, 900), use_hough=False)
    p.run(0, n)
    assert {(p._cfg.rois[i].w, p._cfg.rois[i].h) for i in range(64)} == {(100, 100)}
    got = p.piece_sweep(0, n, settings=list(sets))
    PS.assert_records_equal(got.records, PS.yardstick_records(n=n, display_size=(1280, 900), settings=sets), "100 x 100 squares")
    assert not got.summary["overflow"].any() and got.summary["n_hough"].any()
    p.close()


def test_radius_ratios_that_truncate_to_zero(gpu_ctx):
    """The first trackbar positions: int(min_dim * 0.01) is 0, and HoughCircles reads maxRadius = 0 as "the square's larger
    side", so the radius span (and its histogram) is the widest of all settings, next to settings with narrow ones."""
    sets = ((.01, .01, 100, 25), (.30, .01, 100, 25), (.50, .012, 100, 10), (.20, .55, 100, 25), (.45, .30, 100, 25))
    n = 4
    p = _pipeline(n=n)
    got = p.piece_sweep(0, n, settings=list(sets), expected=PS.expected_bits(n))
    PS.assert_records_equal(got.records, PS.yardstick_records(n=n, settings=sets), "open maximum radius")
    assert not got.summary["overflow"].any() and got.summary["n_hough"][:3].any()
    p.close()


# 7 ------------------------------------------------------------------------------------------------------------------
def test_sweep_on_raw_nv12_frames(gpu_ctx):
    """enhance=False with NV12 input (the warped ring comes from k_warp_yuv) sweeps to what the same pipeline fed the
    converted BGR frames gives."""
    import ref64_yuv as Y
    from chessboard_vision_amd.board_detection import yuv_to_bgr
    from chessboard_vision_amd.stream import BoardPipeline
    n = 6
    src = _pipeline(n=n, run=False)
    raw = [Y.from_bgr(src.download(0, i), "nv12") for i in range(n)]
    src.close()
    out = {}
    for fmt in ("bgr", "nv12"):
        p = BoardPipeline(W, H, n)
        p.configure(PTS, chunk=4, lanes=2, enhance=False)
        if fmt == "nv12":
            p.set_input_format("nv12")
        for i in range(n):
            p.upload(i, raw[i] if fmt == "nv12" else yuv_to_bgr(raw[i], "nv12"), fmt=fmt)
        p.run(0, n)
        out[fmt] = p.piece_sweep(0, n, settings=SETTINGS, expected=PS.expected_bits(n))
        p.close()
    assert _same(out["nv12"].records, out["bgr"].records) and out["nv12"].summary.tobytes() == out["bgr"].summary.tobytes()
    assert out["bgr"].summary["n_hough"].any() and out["bgr"].summary["frames_exact"].any()


# 8 ------------------------------------------------------------------------------------------------------------------
def test_errors_change_nothing(swept):
    _, res, _ = swept
    p = _pipeline(run=False)
    p.run(0, 8)
    before = _snapshot(p, 8)
    lib = p.ctx.lib
    good = (1.2, 100, 25, .20, .55)

    def rc(slot0, count, settings, chunk=0, ns=None):
        sets = np.zeros(max(len(settings), 1), Nat.record_dtype(Nat.HoughParams))
        for i, s in enumerate(settings):
            sets[i] = s
        rec = np.zeros((max(len(settings), 1), max(count, 1)), Nat.record_dtype(Nat.PieceSweepRecord))
        summ = np.zeros(max(len(settings), 1), Nat.record_dtype(Nat.PieceSweepSummary))
        return lib.cbv_pipeline_piece_sweep(p.h_, slot0, count, Nat.ptr(sets), len(settings) if ns is None else ns, None, chunk, Nat.ptr(rec),
                                            Nat.ptr(summ), None)

    nan, inf = float("nan"), float("inf")
    cases = [("a slot never run", STATE, (4, 8, [good])), ("no frames", ARG, (0, 0, [good])), ("count beyond the ring", ARG, (0, N + 1, [good])),
             ("a negative slot", ARG, (-1, 4, [good])), ("slots outside the ring", ARG, (8, 8, [good])),
             ("a negative ratio", ARG, (0, 8, [good, (1.2, 100, 25, -.2, .55)])), ("a NaN ratio", ARG, (0, 8, [(1.2, 100, 25, .2, nan)])),
             ("an infinite ratio", ARG, (0, 8, [(1.2, 100, 25, inf, .55)])), ("param1 = 0", ARG, (0, 8, [(1.2, 0, 25, .2, .55)])),
             ("param1 < 0", ARG, (0, 8, [(1.2, -100, 25, .2, .55)])), ("param2 = 0", ARG, (0, 8, [good, (1.2, 100, 0, .2, .55)])),
             ("param2 = NaN", ARG, (0, 8, [(1.2, 100, nan, .2, .55)])), ("dp = 0", ARG, (0, 8, [(0, 100, 25, .2, .55)])),
             ("dp < 0", ARG, (0, 8, [(-1.2, 100, 25, .2, .55)])), ("dp = 17", UNSUPPORTED, (0, 8, [(17, 100, 25, .2, .55)])),
             ("a ratio above 1", UNSUPPORTED, (0, 8, [good, (1.2, 100, 25, .2, 1.5)])), ("chunk_frames above the limit", ARG, (0, 8, [good], Nat.SWEEP_MAX_CHUNK + 1))]
    for what, code, args in cases:
        assert rc(*args) == code, what
        assert lib.cbv_last_error(p.ctx.h)
    assert rc(0, 8, [good], ns=0) == ARG and rc(0, 8, [good], ns=Nat.PIECE_SWEEP_MAX_SETTINGS + 1) == ARG
    assert lib.cbv_pipeline_piece_sweep(p.h_, 0, 8, None, 1, None, 0, None, None, None) == ARG
    assert lib.cbv_pipeline_piece_sweep(None, 0, 8, None, 1, None, 0, None, None, None) == ARG
    out = (Nat.PieceResult * 64)()
    prm = Nat.HoughParams(*good)
    assert lib.cbv_pipeline_piece_detail(p.h_, 9, prm, out) == STATE and lib.cbv_pipeline_piece_detail(p.h_, 0, prm, None) == ARG
    assert lib.cbv_pipeline_piece_detail(p.h_, 0, Nat.HoughParams(1.2, 100, 0, .2, .55), out) == ARG
    with pytest.raises(RuntimeError):
        p.piece_sweep(4, 8, settings=SETTINGS)
    valid = p.piece_sweep(0, 8, settings=SETTINGS)
    assert _same(valid.records, res.records[:, :8])
    assert _snapshot(p, 8) == before
    from chessboard_vision_amd.stream import BoardPipeline
    fresh = BoardPipeline(W, H, 4)
    sets = np.zeros(1, Nat.record_dtype(Nat.HoughParams))
    sets[0] = good
    summ = np.zeros(1, Nat.record_dtype(Nat.PieceSweepSummary))
    assert lib.cbv_pipeline_piece_sweep(fresh.h_, 0, 1, Nat.ptr(sets), 1, None, 0, None, Nat.ptr(summ), None) == STATE  # not configured
    fresh.close()
    p.close()


# 9 ------------------------------------------------------------------------------------------------------------------
def _counts(ctx, fn):
    ctx.profile_reset()
    ctx.profile_enable(-1)
    try:
        fn()
        return {k: ctx.profile_read(kid)[1] for k, kid in Nat.K_ALL.items() if ctx.profile_read(kid)[1]}
    finally:
        ctx.profile_enable(-2)
        ctx.profile_reset()


def test_off_means_off(gpu_ctx):
    """A pipeline that never sweeps launches what tests/test_gpu_session_chain.py pins for the raw chain (12 frames, chunk 4,
    one lane); a sweep launches no kernel that has a profile id, and the runs behind it launch what they did before."""
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, N)
    p.configure(PTS, chunk=4, lanes=1, enhance=False)
    p.synth(0, N, scene=PS.native_scene(), frames_per_ply=PS.FRAMES_PER_PLY)

    def run():
        p.run(0, N)
        p.results(0, N)
    run()
    off = _counts(gpu_ctx, run)
    assert off == {"WARP": 3, "SQUARES": 3, "SCAN": 1, "HOUGH": 3}, off
    assert _counts(gpu_ctx, lambda: p.piece_sweep(0, N, settings=SETTINGS)) == {}
    assert _counts(gpu_ctx, run) == off
    p.close()
