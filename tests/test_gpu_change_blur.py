"""The ChangeDetector stage's own blur kernel in the pipeline (cbv_pipeline_set_change_blur, k_change_blur_stats) against the
reference's ChangeDetector with `blur_kernel = k` driven call for call (tests/change_blur_ref.py).  640x480, 28 frames,
profile={}, calibration on frame 0 and temporal state reset as tests/test_gpu_model_update.py has it.  Tolerance 0: result
dicts equal, planes equal bit for bit.  tests/test_change_blur_host.py shows on the CPU that the yardstick separates the
kernels used here."""
import numpy as np
import pytest

from chessboard_vision_amd import synth as S
import change_blur_ref as B
import model_update_ref as R

pytestmark = pytest.mark.gpu

W, H, N = R.W, R.H, R.N_FRAMES
PTS = S.scaled_corners(W, H)
ALL = [(f, r) for f in range(8) for r in range(8)]
SPLIT = (1, 2, 3, 7, 5, 10)  # crosses the inline scan of runs of <= 2 frames and the pinned mirror of runs of <= 4
assert sum(SPLIT) == N
UNSUPPORTED = -5


def _pipeline(params, k=None, chunk=4, lanes=2, **kw):
    """A pipeline holding the yardstick stream with ChangeDetector.blur_kernel = k (None: never mentioned), calibrated on
    frame 0, temporal state reset; model update not set."""
    from chessboard_vision_amd.stream import BoardPipeline
    z, iv, _ = params
    p = BoardPipeline(W, H, N)
    if k is not None:
        kw["blur_kernel"] = k
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
    return {pos: b.model(pos) for pos in _positions(b)}


def _positions(b):
    return [(c, 7 - r) for (r, c) in b.rois_rc]


def _snapshot(b, n=N):
    return bytes(b.results(0, n)), [bytes(b.square_stats(i)) for i in range(n)], _planes(b)


def _same_planes(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[pos][0], b[pos][0]) and np.array_equal(a[pos][1], b[pos][1]) for pos in a)


def _assert_snapshots_equal(a, b, what):
    assert a[0] == b[0], "%s: frame results differ" % (what,)
    assert a[1] == b[1], "%s: square statistics differ" % (what,)
    assert _same_planes(a[2], b[2]), "%s: model planes differ" % (what,)


def _assert_matches_yardstick(b, dicts, ref, what="", frames=range(N)):
    res = b.results(0, N)
    for i in frames:
        got = b.changes_detailed(res[i], i)
        assert got == dicts[i], (what, i, got, dicts[i])
    for pos in ALL:
        mean, var = b.model(pos)
        assert mean.dtype == var.dtype == ref.means[pos].dtype == np.float32
        assert np.array_equal(mean, ref.means[pos]), (what, pos, "mean")
        assert np.array_equal(var, ref.variances[pos]), (what, pos, "variance")


def _assert_calibration_planes(p, oracle, k, iv, what):
    """model() right after calibrate_changes(0) = the oracle's preprocess of the warped board's squares."""
    from chessboard_vision_amd.grid_extractor import GridExtractor, SmartGridExtractor
    ge = GridExtractor()
    if getattr(p, "_grid", None) is not None:
        ge = SmartGridExtractor()
        ge.grid_lines_x, ge.grid_lines_y = list(p._grid[0]), list(p._grid[1])
    sq = ge.split_board(p.download(2, 0))
    assert len(sq) == len(p.rois_rc)
    for pos in _positions(p):
        mean, var = p.model(pos)
        want = oracle.square_preprocess(sq[pos], k)
        assert mean.shape == want.shape and np.array_equal(mean, want.astype(np.float32)), (what, k, pos)
        assert np.all(var == np.float32(iv)), (what, k, pos)


# 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 7, 13, 15, 31])
def test_planes_equal_the_oracle_preprocess(gpu_ctx, oracle, k):
    p = _pipeline(B.PARAMS_B, k)
    assert p.change_blur == k
    _assert_calibration_planes(p, oracle, k, B.PARAMS_B[1], "80 px squares")
    p.close()


def test_planes_of_irregular_and_large_squares(gpu_ctx, oracle):
    """grid_lines squares (sides 76-80) and 100 x 100 squares (display_size (1280, 900)), k = 31."""
    grid = (tuple(S.CALIB_GRID_X), tuple(S.CALIB_GRID_Y))
    p = _pipeline(B.PARAMS_B, 31, grid_lines=grid)
    p._grid = grid
    assert len({(p._cfg.rois[i].w, p._cfg.rois[i].h) for i in range(64)}) > 1
    _assert_calibration_planes(p, oracle, 31, B.PARAMS_B[1], "grid_lines")
    p.close()
    p = _pipeline(B.PARAMS_B, 31, display_size=(1280, 900), use_hough=False)
    assert p._cfg.rois[0].w * p._cfg.rois[0].h == 10000
    _assert_calibration_planes(p, oracle, 31, B.PARAMS_B[1], "100 px squares")
    p.close()


# 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,params,k", [(m, prm, k) for m, prm, ks in B.CASES for k in ks],
                         ids=lambda v: str(v).replace(" ", ""))
def test_dicts_and_planes_equal_the_reference_class(gpu_ctx, oracle, mode, params, k):
    """Every frame's detect_changes_detailed dict and, after the run, mean and variance of all 64 squares: chunk = 4, two
    lanes, one run of 28 frames.  Fails without the feature: the host tests show that k = 5 gives other dicts and planes."""
    dicts, ref = B.run_blur(mode, params, k)
    p = _pipeline(params, k)
    p.set_model_update(mode, params[2])
    _run_split(p)
    _assert_matches_yardstick(p, dicts, ref, what=(mode, params, k))
    p.close()


# 3 ------------------------------------------------------------------------------------------------------------------
def test_run_split_invariance(gpu_ctx):
    params = B.PARAMS_B
    one = _pipeline(params, 13)
    one.set_model_update("unchanged", params[2])
    _run_split(one)
    want = _snapshot(one)
    one.close()
    assert any(want[0][i * 64 + 32:i * 64 + 40] != bytes(8) for i in range(N))  # some frame reports a change
    for chunk in (1, 4, 64):
        p = _pipeline(params, 13, chunk=chunk)
        p.set_model_update("unchanged", params[2])
        _run_split(p, SPLIT)
        _assert_snapshots_equal(_snapshot(p), want, ("chunk", chunk))
        p.close()


# 4 ------------------------------------------------------------------------------------------------------------------
def test_kernel_changed_between_runs_keeps_the_model(gpu_ctx, oracle):
    params, s = B.PARAMS_B, B.SWITCH_AT
    dicts, ref = B.run_blur("every", params, B.SWITCH_FROM, switch=(s, B.SWITCH_TO))
    p = _pipeline(params)
    p.set_model_update("every", params[2])
    p.run(0, s)
    p.set_change_blur(B.SWITCH_TO)
    assert p.change_blur == B.SWITCH_TO
    with pytest.raises(RuntimeError):
        p.calibrate_changes(3)  # slot 3 was last run with k = 5
    p.run(s, N - s)
    _assert_matches_yardstick(p, dicts, ref, what="switched")
    p.run(3, 1)
    p.calibrate_changes(3)
    p.close()


# 5 ------------------------------------------------------------------------------------------------------------------
def _profiled_counts(ctx, p, split):
    from chessboard_vision_amd import _native as Nat
    ctx.profile_reset()
    ctx.profile_enable(-1)
    try:
        _run_split(p, split)
        p.results(0, N)
        return [ctx.profile_read(kid)[1] for kid in range(Nat.K_CHANGE_BLUR + 1)]
    finally:
        ctx.profile_enable(-2)
        ctx.profile_reset()


def test_off_means_off(gpu_ctx):
    from chessboard_vision_amd import _native as Nat
    params = B.PARAMS_SHIPPED
    plain, set5, cfg5 = _pipeline(params), _pipeline(params), _pipeline(params, 4 | 1)
    set5.set_change_blur(5)
    counts = [_profiled_counts(gpu_ctx, q, SPLIT) for q in (plain, set5, cfg5)]
    assert counts[0] == counts[1] == counts[2], counts
    assert counts[0][Nat.K_CHANGE_BLUR] == 0 and counts[0][Nat.K["SQUARES"]] > 0, counts[0]
    want = _snapshot(plain)
    _assert_snapshots_equal(_snapshot(set5), want, "set_change_blur(5) against untouched")
    _assert_snapshots_equal(_snapshot(cfg5), want, "configure(blur_kernel=5) against untouched")
    for q in (plain, set5, cfg5):
        q.close()
    p = _pipeline(params, 13)
    c13 = _profiled_counts(gpu_ctx, p, SPLIT)
    assert c13[Nat.K_CHANGE_BLUR] == c13[Nat.K["SQUARES"]] > 0, c13
    assert c13[:Nat.K_CHANGE_BLUR] == counts[0][:Nat.K_CHANGE_BLUR], (c13, counts[0])
    p.close()


# 6 ------------------------------------------------------------------------------------------------------------------
def test_piece_detector_side_does_not_move(gpu_ctx):
    params = B.PARAMS_B
    out = {}
    for k in (5, 13):
        p = _pipeline(params, k)
        p.set_model_update("unchanged", params[2])
        _run_split(p, SPLIT)
        out[k] = (p.results(0, N), [(st.name, sorted(d.items(), key=str)) for st, d in p.noise_results(0, N)],
                  [bytes(p.hough(i)) for i in range(N)])
        p.close()
    (base, base_noise, base_hough), (res, noise, hough) = out[5], out[13]
    assert noise == base_noise and hough == base_hough
    differs = False
    for i in range(N):
        for field in ("raw_occupied", "stable_occupied", "visual_changes", "processed"):
            assert getattr(res[i], field) == getattr(base[i], field), (i, field)
        both = res[i].changed & base[i].changed
        assert res[i].circular & both == base[i].circular & both, i
        differs |= res[i].changed != base[i].changed
    assert differs  # the ChangeDetector side did move


# 7 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["frozen", "every"])
def test_two_boards_with_different_kernels(gpu_ctx, mode):
    """Boards with k = 5 and k = 13 on one pipeline, then swapped: each equals a single-board pipeline with that kernel on
    the same frames (the multi-board launches of k_change_blur_stats and k_model_scan)."""
    params = B.PARAMS_B
    z, iv, alpha = params
    single = {}
    for k in (5, 13):
        p = _pipeline(params, k)
        p.set_model_update(mode, alpha)
        _run_split(p, SPLIT)
        single[k] = _snapshot(p)
        p.close()
    assert single[5][1] != single[13][1]
    for ks in ((5, 13), (13, 5)):
        p = _pipeline(params, ks[0])
        b = p.add_board(PTS, z_threshold=z, initial_variance=iv, blur_kernel=ks[1])
        assert (p.change_blur, b.change_blur) == ks
        _calibrate(p, b)
        p.reset_state()
        for board in (p, b):
            board.set_model_update(mode, alpha)
        _run_split(p, SPLIT)
        for board, k in zip((p, b), ks):
            _assert_snapshots_equal(_snapshot(board), single[k], (mode, ks, k))
        b.close()
        p.close()


def test_two_boards_on_raw_nv12_frames(gpu_ctx):
    """enhance=False with NV12 input: k_warp_yuv feeds the new kernel.  Boards with k = 13 and k = 5 equal the same pipeline
    fed the converted BGR frames."""
    import ref64_yuv as Y
    from chessboard_vision_amd.board_detection import yuv_to_bgr
    from chessboard_vision_amd.stream import BoardPipeline
    z, iv, alpha = B.PARAMS_B
    n = 12
    src = BoardPipeline(W, H, n)
    src.synth(0, n, scene="normal", frames_per_ply=4)
    raw = [Y.from_bgr(src.download(0, i), "nv12") for i in range(n)]
    src.close()
    bgr = [yuv_to_bgr(f, "nv12") for f in raw]
    snaps = {}
    for fmt in ("bgr", "nv12"):
        p = BoardPipeline(W, H, n)
        p.configure(PTS, chunk=4, lanes=2, enhance=False, z_threshold=z, initial_variance=iv, blur_kernel=13)
        b = p.add_board(PTS, z_threshold=z, initial_variance=iv, blur_kernel=5)
        if fmt == "nv12":
            p.set_input_format("nv12")
        for i in range(n):
            p.upload(i, raw[i] if fmt == "nv12" else bgr[i], fmt=fmt)
        p.run(0, 1)
        for board in (p, b):
            board.calibrate_changes(0)
            board.reset_state()
            board.set_model_update("every", alpha)
        p.run(0, 5)
        p.run(5, n - 5)
        snaps[fmt] = [_snapshot(board, n) for board in (p, b)]
        b.close()
        p.close()
    for k, got, want in zip((13, 5), snaps["nv12"], snaps["bgr"]):
        _assert_snapshots_equal(got, want, ("raw NV12 against converted BGR, k", k))
    assert snaps["bgr"][0][1] != snaps["bgr"][1][1]  # the two kernels do give different statistics here


# 8 ------------------------------------------------------------------------------------------------------------------
def test_class_api_and_pipeline_agree(gpu_ctx, oracle):
    """ChangeDetector (the class API, k_squares_preprocess) with blur_kernel = 13 fed the pipeline's own warped boards gives
    the pipeline's dicts and planes in mode "every"."""
    from chessboard_vision_amd.change_detector import ChangeDetector
    from chessboard_vision_amd.grid_extractor import GridExtractor
    params = R.PARAMS_A
    p = _pipeline(params, 13)
    p.set_model_update("every", params[2])
    _run_split(p)
    res = p.results(0, N)
    cd = ChangeDetector()
    cd.z_threshold, cd.initial_variance, cd.alpha = params
    cd.blur_kernel = 13
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


# 9 ------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_rejected_and_change_nothing(gpu_ctx, oracle):
    params = B.PARAMS_B
    dicts, ref = B.run_blur("every", params, 13)
    p = _pipeline(params, 13)
    p.set_model_update("every", params[2])
    lib = p.ctx.lib
    for k in (33, 255):
        assert lib.cbv_pipeline_set_change_blur(p.h_, k) == UNSUPPORTED
        with pytest.raises(RuntimeError):
            p.set_change_blur(k)
        assert p.change_blur == 13
    assert lib.cbv_pipeline_set_change_blur(None, 13) == -1  # CBV_ERR_ARG
    _run_split(p)
    _assert_matches_yardstick(p, dicts, ref, what="after the rejected calls")
    p.close()


def test_no_kernel_is_too_large_for_tiny_squares(gpu_ctx, oracle):
    """REFLECT_101 folds as often as it takes (d_reflect101, and the oracle's reflect101 the same), so a radius beyond the
    square's side is no error: 3 x 3 squares under k = 31 (radius 15) equal the oracle like any others."""
    p = _pipeline(B.PARAMS_B, 31, display_size=(124, 124), use_hough=False)
    assert {(p._cfg.rois[i].w, p._cfg.rois[i].h) for i in range(64)} == {(3, 3)}
    _assert_calibration_planes(p, oracle, 31, B.PARAMS_B[1], "3 px squares")
    p.close()


@pytest.mark.parametrize("given,k", [(0, 1), (-3, 1), (12, 13)])
def test_kernel_values_are_normalised(gpu_ctx, oracle, given, k):
    p = _pipeline(B.PARAMS_B)
    p.set_change_blur(given)
    assert p.change_blur == k
    _calibrate(p, p)
    _assert_calibration_planes(p, oracle, k, B.PARAMS_B[1], ("set_change_blur", given))
    p.close()


# 10 -----------------------------------------------------------------------------------------------------------------
def test_hand_pattern_of_every_frame(gpu_ctx, oracle):
    params = B.PARAMS_B
    dicts, ref = B.run_blur("unchanged", params, 13)
    p = _pipeline(params, 13)
    p.set_model_update("unchanged", params[2])
    _run_split(p)
    res = p.results(0, N)
    seen = set()
    for i in range(N):
        want = ref.classify_hand_pattern(dicts[i])
        assert p.hand_pattern(res[i]) == want, (i, want)
        seen.add((want["is_hand"], want["is_move"]))
    assert len(seen) > 1, seen
    p.close()
