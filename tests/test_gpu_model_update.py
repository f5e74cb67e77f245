"""Per-frame background model update of the pipeline (cbv_pipeline_set_model_update, k_model_scan) against the reference's
ChangeDetector driven call for call (tests/model_update_ref.py).  Tolerance 0: result dicts equal, model planes equal
bit for bit.  tests/test_model_update_host.py shows on the CPU that the stream used here separates the modes."""
import numpy as np
import pytest

from chessboard_vision_amd import synth as S
import model_update_ref as R

pytestmark = pytest.mark.gpu

W, H, N = R.W, R.H, R.N_FRAMES
PTS = S.scaled_corners(W, H)
ALL = [(f, r) for f in range(8) for r in range(8)]
SPLIT = (1, 2, 3, 7, 5, 10)  # crosses the inline scan of runs of <= 2 frames and the pinned mirror of runs of <= 4
assert sum(SPLIT) == N


def _pipeline(params, chunk=4, lanes=2, **kw):
    """A pipeline holding the yardstick stream, calibrated on frame 0, temporal state reset; model update not set."""
    from chessboard_vision_amd.stream import BoardPipeline
    z, iv, _ = params
    p = BoardPipeline(W, H, N)
    p.configure(PTS, profile={}, chunk=chunk, lanes=lanes, z_threshold=z, initial_variance=iv, **kw)
    p.synth(0, N, scene="normal", frames_per_ply=R.FRAMES_PER_PLY)
    _calibrate(p, p)
    return p


def _calibrate(p, board, slot=0):
    p.run(slot, 1)
    board.calibrate_changes(slot)
    board.reset_state()


def _run_split(p, split=(N,)):
    s = 0
    for c in split:  # nothing is read in between: the runs overlap
        p.run(s, c)
        s += c


def _planes(b):
    return {pos: b.model(pos) for pos in ALL}


def _snapshot(b, n=N):
    return bytes(b.results(0, n)), [bytes(b.square_stats(i)) for i in range(n)], _planes(b)


def _same_planes(a, b):
    return all(np.array_equal(a[pos][0], b[pos][0]) and np.array_equal(a[pos][1], b[pos][1]) for pos in ALL)


def _assert_snapshots_equal(a, b, what):
    assert a[0] == b[0], "%s: frame results differ" % (what,)
    assert a[1] == b[1], "%s: square statistics differ" % (what,)
    assert _same_planes(a[2], b[2]), "%s: model planes differ" % (what,)


def _assert_matches_yardstick(b, dicts, ref, res=None, what=""):
    res = res if res is not None else b.results(0, N)
    for i in range(N):
        got = b.changes_detailed(res[i], i)
        assert got == dicts[i], (what, i, got, dicts[i])
    for pos in ALL:
        mean, var = b.model(pos)
        assert mean.dtype == var.dtype == ref.means[pos].dtype == np.float32
        assert np.array_equal(mean, ref.means[pos]), (what, pos, "mean")
        assert np.array_equal(var, ref.variances[pos]), (what, pos, "variance")


@pytest.mark.parametrize("params", [R.PARAMS_A, R.PARAMS_B], ids=["z2.55_iv600_a0.1", "z1.45_iv50_a0.37"])
@pytest.mark.parametrize("mode", ["every", "unchanged"])
def test_modes_equal_the_reference_class(gpu_ctx, oracle, mode, params):
    """Every frame's detect_changes_detailed dict and, after the run, mean and variance of all 64 squares: chunk = 4, two
    lanes, one run of 28 frames."""
    dicts, ref = R.run_mode(mode, params)
    p = _pipeline(params)
    p.set_model_update(mode, params[2])
    _run_split(p)
    _assert_matches_yardstick(p, dicts, ref, what=(mode, params))
    p.close()


def test_class_api_and_pipeline_agree(gpu_ctx, oracle):
    """ChangeDetector (the class API: detect_changes_detailed, then update_all_references -> k_squares_ema) fed the
    pipeline's own warped boards gives the pipeline's dicts and planes in mode "every"."""
    from chessboard_vision_amd.change_detector import ChangeDetector
    from chessboard_vision_amd.grid_extractor import GridExtractor
    params = R.PARAMS_A
    p = _pipeline(params)
    p.set_model_update("every", params[2])
    _run_split(p)
    res = p.results(0, N)
    cd = ChangeDetector()
    cd.z_threshold, cd.initial_variance, cd.alpha = params
    for i in range(N):
        sq = GridExtractor().split_board(p.download(2, i))
        if i == 0:
            cd.calibrate(sq)
        assert cd.detect_changes_detailed(sq) == p.changes_detailed(res[i], i), i
        cd.update_all_references(sq)
    for pos in ALL:
        mean, var = p.model(pos)
        assert np.array_equal(mean, cd.means[pos]) and np.array_equal(var, cd.variances[pos]), pos
    p.close()


@pytest.mark.parametrize("mode,chunks", [("every", (1, 4, 64)), ("unchanged", (4,))])
def test_run_split_invariance(gpu_ctx, mode, chunks):
    """28 frames as one run, and as overlapping runs of 1, 2, 3, 7, 5 and 10 frames, with several chunk sizes: identical
    result records, square statistics and model planes."""
    params = R.PARAMS_B
    one = _pipeline(params)
    one.set_model_update(mode, params[2])
    _run_split(one)
    want = _snapshot(one)
    one.close()
    assert any(want[0][i * 64 + 32:i * 64 + 40] != bytes(8) for i in range(N))  # some frame reports a change
    for chunk in chunks:
        p = _pipeline(params, chunk=chunk)
        p.set_model_update(mode, params[2])
        _run_split(p, SPLIT)
        _assert_snapshots_equal(_snapshot(p), want, (mode, "chunk", chunk))
        p.close()


def _profiled_counts(ctx, p, split):
    from chessboard_vision_amd import _native as Nat
    ctx.profile_reset()
    ctx.profile_enable(-1)
    try:
        _run_split(p, split)
        p.results(0, N)
        return [ctx.profile_read(kid)[1] for kid in range(Nat.K["MODEL_SCAN"] + 1)]
    finally:
        ctx.profile_enable(-2)
        ctx.profile_reset()


def test_off_means_off(gpu_ctx):
    """set_model_update("frozen") and a pipeline that never heard of the feature: the same results and statistics, no launch
    of the new kernel and the same launches of every other one.  every -> frozen between two runs freezes the model."""
    from chessboard_vision_amd import _native as Nat
    params = R.PARAMS_A
    plain, frozen = _pipeline(params), _pipeline(params)
    frozen.set_model_update("frozen")
    c_plain = _profiled_counts(gpu_ctx, plain, SPLIT)
    c_frozen = _profiled_counts(gpu_ctx, frozen, SPLIT)
    assert c_frozen == c_plain and c_plain[Nat.K["MODEL_SCAN"]] == 0 and c_plain[Nat.K["SQUARES"]] > 0, (c_plain, c_frozen)
    _assert_snapshots_equal(_snapshot(frozen), _snapshot(plain), "frozen against untouched")
    # the frozen model is the calibration: mean = the calibration frame's squares, variance = initial_variance
    assert all(np.all(plain.model(pos)[1] == np.float32(params[1])) for pos in ALL)
    plain.close()
    frozen.close()

    p = _pipeline(params)
    p.set_model_update("every", params[2])
    c_every = _profiled_counts(gpu_ctx, p, (14,))
    assert c_every[Nat.K["MODEL_SCAN"]] == 1
    before = _planes(p)
    assert any(np.any(before[pos][1] != np.float32(params[1])) for pos in ALL)  # the model did move
    p.set_model_update("frozen")
    p.run(14, 14)
    assert _same_planes(before, _planes(p))
    # and the frozen run is judged against the model the first run left behind
    dicts = R.run_mode("every", params)[0]
    ref = R.new_ref(params)
    sq = R.stream_squares()
    ref.calibrate(sq[0])
    for i in range(14):
        R.step(ref, "every", sq[i])
    res = p.results(0, N)
    for i in range(14):
        assert p.changes_detailed(res[i], i) == dicts[i], i
    for i in range(14, N):
        assert p.changes_detailed(res[i], i) == R.step(ref, "frozen", sq[i]), i
    p.close()


def test_piece_detector_side_does_not_move(gpu_ctx):
    """raw / stable occupancy, visual_changes, processed and the NoiseHandler outputs do not read the model: equal in all
    modes, every frame.  `circular` is detect_piece on the current square, reported for the squares in `changed` only
    (k_scan packs it with the change classes), so it is compared where both modes report the square, and is a subset of
    `changed` in every mode; its value against the reference is part of the dicts of test_modes_equal_the_reference_class."""
    params = R.PARAMS_B
    out = {}
    for mode in R.MODES:
        p = _pipeline(params)
        p.set_model_update(mode, params[2])
        _run_split(p, SPLIT)
        out[mode] = (p.results(0, N), [(st.name, sorted(d.items(), key=str)) for st, d in p.noise_results(0, N)])
        p.close()
    base, base_noise = out["frozen"]
    differs = False
    for mode in ("every", "unchanged"):
        res, noise = out[mode]
        assert noise == base_noise, mode
        for i in range(N):
            for field in ("raw_occupied", "stable_occupied", "visual_changes", "processed"):
                assert getattr(res[i], field) == getattr(base[i], field), (mode, i, field)
            both = res[i].changed & base[i].changed
            assert res[i].circular & both == base[i].circular & both, (mode, i)
            assert res[i].circular & ~res[i].changed == 0 and base[i].circular & ~base[i].changed == 0, (mode, i)
            differs |= res[i].changed != base[i].changed
    assert differs  # the ChangeDetector side did move


def test_calibrate_restarts_the_model_and_uncalibrated_boards_do_nothing(gpu_ctx, oracle):
    from chessboard_vision_amd.stream import BoardPipeline
    params = R.PARAMS_A
    # modes set before any calibration: nothing to update, `changed` stays zero, the run succeeds
    p = BoardPipeline(W, H, N)
    p.configure(PTS, profile={}, chunk=4, lanes=2, z_threshold=params[0], initial_variance=params[1])
    p.synth(0, N, scene="normal", frames_per_ply=R.FRAMES_PER_PLY)
    for mode in ("every", "unchanged"):
        p.set_model_update(mode, params[2])
        _run_split(p, SPLIT)
        res = p.results(0, N)
        assert all(r.changed == 0 and r.parcial == 0 and r.total == 0 for r in res), mode
        with pytest.raises(RuntimeError):
            p.model((0, 0))
    # calibrate on frame 0 with the mode already set, run 0..11, calibrate again on frame 12, run 12..27
    for mode in ("every", "unchanged"):
        dicts, ref = R.run_mode(mode, params, calibrate_at=(0, 12))
        p.set_model_update(mode, params[2])
        _calibrate(p, p, 0)
        p.run(0, 12)
        p.run(12, 1)
        p.calibrate_changes(12)
        p.run(12, N - 12)
        _assert_matches_yardstick(p, dicts, ref, what=("recalibrated", mode))
    p.close()


def test_irregular_and_large_squares(gpu_ctx, oracle):
    """grid_lines squares (sides 76-80 px, up to 6400 px: register-resident path, 8 px a lane) in mode "unchanged"; and
    100 x 100 px squares (display_size (1280, 900): 10000 px > MS_PPL * 1024 = 8192), which force the path of
    k_model_scan that leaves the model in memory, in both modes."""
    params = R.PARAMS_B
    grid = (tuple(S.CALIB_GRID_X), tuple(S.CALIB_GRID_Y))
    dicts, ref = R.run_mode("unchanged", params, grid=grid)
    p = _pipeline(params, grid_lines=grid)
    sides = {(p._cfg.rois[i].w, p._cfg.rois[i].h) for i in range(64)}
    assert len(sides) > 1 and max(w * h for w, h in sides) <= 8192
    p.set_model_update("unchanged", params[2])
    _run_split(p, SPLIT)
    _assert_matches_yardstick(p, dicts, ref, what="grid_lines")
    p.close()
    assert any(d for d in dicts)

    big = (1280, 900)
    for mode in ("unchanged", "every"):
        dicts, ref = R.run_mode(mode, params, use_hough=False, display_size=big)
        p = _pipeline(params, display_size=big, use_hough=False)
        assert p._cfg.rois[0].w * p._cfg.rois[0].h == 10000
        p.set_model_update(mode, params[2])
        _run_split(p, SPLIT)
        _assert_matches_yardstick(p, dicts, ref, what=("100 px squares", mode))
        p.close()
        assert any(d for d in dicts)


def test_two_boards_with_different_modes(gpu_ctx):
    """Two boards on one pipeline, one "every" and one "frozen", then the roles swapped: each equals a single-board
    pipeline in that mode on the same frames."""
    params = R.PARAMS_A
    z, iv, alpha = params
    single = {}
    for mode in ("every", "frozen"):
        p = _pipeline(params)
        p.set_model_update(mode, alpha)
        _run_split(p, SPLIT)
        single[mode] = _snapshot(p)
        p.close()
    assert single["every"][0] != single["frozen"][0]
    for modes in (("every", "frozen"), ("frozen", "every")):
        p = _pipeline(params)
        b = p.add_board(PTS, z_threshold=z, initial_variance=iv)
        _calibrate(p, b)
        p.reset_state()
        for board, mode in zip((p, b), modes):
            board.set_model_update(mode, alpha)
        _run_split(p, SPLIT)
        for board, mode in zip((p, b), modes):
            _assert_snapshots_equal(_snapshot(board), single[mode], (modes, mode))
        b.close()
        p.close()


def test_bad_arguments_are_rejected_and_change_nothing(gpu_ctx):
    params = R.PARAMS_A
    dicts, ref = R.run_mode("every", params)
    p = _pipeline(params)
    p.set_model_update("every", params[2])
    lib = p.ctx.lib
    for mode, alpha in ((3, 0.1), (1, -0.1), (2, 1.5)):
        assert lib.cbv_pipeline_set_model_update(p.h_, mode, alpha) == -1  # CBV_ERR_ARG
    with pytest.raises(ValueError):
        p.set_model_update("sometimes")
    _run_split(p)
    _assert_matches_yardstick(p, dicts, ref, what="after the rejected calls")
    p.close()
