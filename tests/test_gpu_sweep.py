"""The ChangeDetector sensitivity sweep on the device (cbv_pipeline_sweep, cbv_pipeline_change_hist; k_change_hist and
k_sweep_eval) against the yardsticks of tests/sweep_ref.py: the oracle's difference histograms, the reference class driven
setting by setting, the host twin, and the product's own per-setting path.  640x480, 28 frames, profile={}, calibration on
frame 0, set up as tests/test_gpu_change_blur.py does.  Tolerance 0.  tests/test_sweep_host.py shows on the CPU that the
settings used here reach every case."""
import random

import numpy as np
import pytest

from chessboard_vision_amd import _native as Nat
from chessboard_vision_amd import synth as S
import change_blur_ref as B
import sweep_ref as SR
from test_gpu_change_blur import H, N, PTS, W, _assert_snapshots_equal, _pipeline, _run_split, _snapshot

pytestmark = pytest.mark.gpu

ARG, STATE, UNSUPPORTED = -1, -4, -5
GRID = list(SR.GRID)
REC_FIELDS = ("changed", "parcial", "total", "z_max", "n_changed", "n_total", "flags", "lifted")


def _same_records(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _reduce(rec):
    """cbv_sweep_summary of every setting from its records ([S, F])"""
    out = np.zeros(rec.shape[0], Nat.record_dtype(Nat.SweepSummary))
    out["frames_changed"] = (rec["n_changed"] > 0).sum(axis=1)
    out["frames_hand"] = ((rec["flags"] & 1) != 0).sum(axis=1)
    out["frames_move"] = ((rec["flags"] & 2) != 0).sum(axis=1)
    out["frames_lifted"] = (rec["lifted"] >= 0).sum(axis=1)
    out["squares_reported"] = rec["n_changed"].astype(np.int64).sum(axis=1)
    out["z_max"] = rec["z_max"].max(axis=1)
    return out


@pytest.fixture(scope="module")
def swept(gpu_ctx):
    """A pipeline calibrated with settings of its own (PARAMS_B, k = 5) holding the 28 processed frames, its snapshot, and
    ONE sweep of the 100-setting grid over all of them."""
    p = _pipeline(B.PARAMS_B)
    _run_split(p)
    before = _snapshot(p)
    res = p.sensitivity_sweep(0, 0, N, settings=GRID)
    yield p, res, before
    p.close()


# 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", SR.GRID_K)
def test_change_hist_equals_the_oracle_histogram(swept, k):
    p, _, _ = swept
    want, n_px = SR.oracle_hists(k)
    for f in (0, 9, 27):
        got = p.change_hist(0, f, k)
        assert got.dtype == np.uint16 and got.shape == (64, 256)
        assert np.array_equal(got.sum(axis=1), n_px), (k, f)
        assert np.array_equal(got, want[f]), (k, f)
    first = p.change_hist(0, 0, k)
    assert np.array_equal(first[:, 0], n_px) and not first[:, 1:].any()
    assert want[9][:, 1:].any() and want[27][:, 1:].any()


def test_change_hist_of_irregular_and_large_squares(gpu_ctx):
    """grid_lines squares (sides 76-80) and 100 x 100 squares (display_size (1280, 900)), k = 31."""
    grid = (tuple(S.CALIB_GRID_X), tuple(S.CALIB_GRID_Y))
    for kw, okw in ((dict(grid_lines=grid), dict(grid=grid)),
                    (dict(display_size=(1280, 900), use_hough=False), dict(display_size=(1280, 900)))):
        p = _pipeline(B.PARAMS_B, 31, **kw)
        _run_split(p)
        sizes = {(p._cfg.rois[i].w, p._cfg.rois[i].h) for i in range(64)}
        assert len(sizes) > 1 if "grid_lines" in kw else sizes == {(100, 100)}
        want, n_px = SR.oracle_hists(31, **okw)
        for f in (9, 27):
            got = p.change_hist(0, f, 31)
            assert np.array_equal(got.sum(axis=1), n_px) and np.array_equal(got, want[f]), (sorted(kw), f)
        p.close()


# 2 ------------------------------------------------------------------------------------------------------------------
def test_one_sweep_of_the_grid_equals_the_yardsticks(swept):
    _, res, _ = swept
    rec = res.records
    assert rec.shape == (len(GRID), N) and res.info["kernels_distinct"] == len(SR.GRID_K)
    for s in SR.CLASS_SETTINGS:  # the reference class, frame by frame
        dicts = SR.class_dicts(s)
        j = GRID.index(s)
        for i in range(N):
            SR.assert_record_matches_dict(rec[j, i], dicts[i], (s, i))
            assert res.pattern(j, i)["move_candidates"] == (set(dicts[i]) if len(dicts[i]) <= 2 and not res.is_hand[j, i] else set())
    for k in SR.GRID_K:  # the host twin on the oracle's histograms, every record of the grid
        idx = [j for j, s in enumerate(GRID) if s[2] == k]
        want = SR.eval_host(*SR.oracle_hists(k), [GRID[j] for j in idx])
        for name in REC_FIELDS:
            assert np.array_equal(rec[name][idx], want[name]), (k, name)
    assert res.summary.tobytes() == _reduce(rec).tobytes()
    assert (res.summary["frames_changed"] > 0).any() and (res.summary["frames_hand"] > 0).any() and (res.summary["frames_lifted"] > 0).any()


# 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", [(2.5, 100, 5), (1.45, 50, 13)], ids=str)
def test_sweep_equals_the_per_setting_path(swept, setting):
    """A pipeline configured with the setting, calibrated on frame 0 and run (k_squares_pre5_stats for k = 5,
    k_change_blur_stats otherwise) reports what the sweep's record says, and its z statistics are the device histogram's."""
    p, res, _ = swept
    z, iv, k = setting
    q = _pipeline((z, iv, 0.1), k)
    _run_split(q)
    out = q.results(0, N)
    j = GRID.index(setting)
    reported = 0
    for i in range(N):
        assert (out[i].changed, out[i].parcial, out[i].total) == tuple(int(res.records[name][j, i]) for name in ("changed", "parcial", "total")), i
        reported += bin(out[i].changed).count("1")
    assert reported > 0
    for i in (0, 9, 20, 27):
        hist = p.change_hist(0, i, k)
        want = SR.numpy_eval(hist[None], np.array([d.sum() for d in hist], np.int32), z, iv)
        st = q.square_stats(i)
        assert [s.z_count for s in st] == list(want["z_count"][0]), i
        assert [np.float32(s.z_max) for s in st] == list(want["z_sq"][0]), i
    q.close()


# 4 ------------------------------------------------------------------------------------------------------------------
def test_invariance(swept):
    p, res, _ = swept
    assert res.info["chunk_frames"] == Nat.SWEEP_DEFAULT_CHUNK
    for chunk in (1, 5):
        r = p.sensitivity_sweep(0, 0, N, settings=GRID, chunk_frames=chunk)
        assert r.info["chunk_frames"] == chunk
        assert _same_records(r.records, res.records) and r.summary.tobytes() == res.summary.tobytes(), chunk
    a, b = p.sensitivity_sweep(0, 0, 10, settings=GRID), p.sensitivity_sweep(0, 10, N - 10, settings=GRID)
    assert _same_records(np.concatenate([a.records, b.records], axis=1), res.records)
    assert a.summary.tobytes() == _reduce(res.records[:, :10]).tobytes() and b.summary.tobytes() == _reduce(res.records[:, 10:]).tobytes()
    quiet = p.sensitivity_sweep(0, 0, N, settings=GRID, records=False)
    assert quiet.records is None and quiet.summary.tobytes() == res.summary.tobytes()
    order = list(range(len(GRID)))
    random.Random(5).shuffle(order)
    sh = p.sensitivity_sweep(0, 0, N, settings=[GRID[j] for j in order])
    assert _same_records(sh.records, res.records[order]) and sh.summary.tobytes() == res.summary[order].tobytes()
    dup = p.sensitivity_sweep(0, 0, N, settings=[GRID[7], GRID[42], GRID[7], GRID[7]])
    assert _same_records(dup.records, res.records[[7, 42, 7, 7]]) and dup.summary.tobytes() == res.summary[[7, 42, 7, 7]].tobytes()
    prod = p.sensitivity_sweep(0, 0, N, z_thresholds=SR.GRID_Z, initial_variances=SR.GRID_IV, blur_kernels=SR.GRID_K)
    assert _same_records(prod.records, res.records)
    # the kernel is normalised as set_change_blur does it: 0 -> 1, 12 -> 13
    norm = p.sensitivity_sweep(0, 0, N, settings=[(1.45, 50, 0), (2.55, 600, 12)])
    assert _same_records(norm.records, res.records[[GRID.index((1.45, 50, 1)), GRID.index((2.55, 600, 13))]])


# 5 ------------------------------------------------------------------------------------------------------------------
def test_the_board_is_untouched(swept):
    p, _, before = swept
    _assert_snapshots_equal(_snapshot(p), before, "a board calibrated with other settings, after the sweeps")
    assert p.change_blur == 5
    # an uncalibrated board: results and statistics (it has no model)
    from chessboard_vision_amd.stream import BoardPipeline
    u = BoardPipeline(W, H, N)
    u.configure(PTS, profile={}, chunk=4, lanes=2)
    u.synth(0, N, scene="normal", frames_per_ply=8)
    u.run(0, N)
    snap = (bytes(u.results(0, N)), [bytes(u.square_stats(i)) for i in range(N)])
    r = u.sensitivity_sweep(0, 0, N, settings=GRID)
    assert (bytes(u.results(0, N)), [bytes(u.square_stats(i)) for i in range(N)]) == snap
    with pytest.raises(RuntimeError):
        u.model((0, 0))  # still not calibrated
    u.close()
    # a run enqueued after a sweep equals the same run on a pipeline that never swept
    a, b = _pipeline(B.PARAMS_B, 13), _pipeline(B.PARAMS_B, 13)
    for q in (a, b):
        q.set_model_update("unchanged", B.PARAMS_B[2])
        q.run(0, 12)
    ra = a.sensitivity_sweep(0, 0, 12, settings=GRID)
    for q in (a, b):
        q.run(12, N - 12)
    _assert_snapshots_equal(_snapshot(a), _snapshot(b), "runs around a sweep")
    assert _same_records(ra.records, r.records[:, :12])
    a.close()
    b.close()


# 6 ------------------------------------------------------------------------------------------------------------------
def test_an_attached_board_sweeps_like_a_pipeline_of_its_own(gpu_ctx):
    from chessboard_vision_amd.stream import BoardPipeline
    quad = PTS + np.float32([7, -5])
    z, iv, _ = B.PARAMS_B
    p = _pipeline(B.PARAMS_B, 13)
    b = p.add_board(quad, z_threshold=z, initial_variance=iv, blur_kernel=5, use_hough=False)
    _run_split(p)
    own = BoardPipeline(W, H, N)
    own.configure(quad, profile={}, chunk=4, lanes=2, use_hough=False)
    own.synth(0, N, scene="normal", frames_per_ply=8)
    own.run(0, N)
    got, want = b.sensitivity_sweep(0, 0, N, settings=GRID), own.sensitivity_sweep(0, 0, N, settings=GRID)
    assert _same_records(got.records, want.records) and got.summary.tobytes() == want.summary.tobytes()
    assert (want.summary["frames_changed"] > 0).any()
    base = p.sensitivity_sweep(0, 0, N, settings=GRID)
    assert not _same_records(base.records, got.records)  # the shifted quad does see other squares
    assert np.array_equal(b.change_hist(0, 9, 13), own.change_hist(0, 9, 13))
    own.close()
    b.close()
    p.close()


def test_sweep_on_raw_nv12_frames(gpu_ctx):
    """enhance=False with NV12 input (the warped ring comes from k_warp_yuv) sweeps to what the same pipeline fed the
    converted BGR frames gives."""
    import ref64_yuv as Y
    from chessboard_vision_amd.board_detection import yuv_to_bgr
    from chessboard_vision_amd.stream import BoardPipeline
    n = 12
    src = BoardPipeline(W, H, n)
    src.synth(0, n, scene="normal", frames_per_ply=4)
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
        out[fmt] = p.sensitivity_sweep(0, 1, n - 1, settings=GRID)
        p.close()
    assert _same_records(out["nv12"].records, out["bgr"].records) and out["nv12"].summary.tobytes() == out["bgr"].summary.tobytes()
    assert (out["bgr"].summary["frames_changed"] > 0).any()


# 7 ------------------------------------------------------------------------------------------------------------------
def test_errors_change_nothing(swept):
    _, res, _ = swept
    p = _pipeline(B.PARAMS_B, 13)
    p.run(0, 10)
    before = _snapshot(p, 10)
    lib = p.ctx.lib

    def rc(calib, slot0, count, settings, chunk=0, ns=None):
        sets = np.zeros(max(len(settings), 1), Nat.record_dtype(Nat.SweepSetting))
        for i, s in enumerate(settings):
            sets[i] = s
        rec = np.zeros((max(len(settings), 1), max(count, 1)), Nat.record_dtype(Nat.SweepRecord))
        return lib.cbv_pipeline_sweep(p.h_, calib, slot0, count, Nat.ptr(sets), len(settings) if ns is None else ns, chunk, Nat.ptr(rec), None, None)

    good = [(2.55, 600, 13)]
    cases = [("a frame slot that was never run", STATE, (0, 5, 10, good)), ("a calibration slot that was never run", STATE, (20, 0, 10, good)),
             ("iv = 0", ARG, (0, 0, 10, [(2.55, 0.0, 13)])), ("iv < 0", ARG, (0, 0, 10, good + [(2.55, -600.0, 13)])),
             ("iv = NaN", ARG, (0, 0, 10, [(2.55, float("nan"), 13)])), ("iv = inf", ARG, (0, 0, 10, [(2.55, float("inf"), 13)])),
             ("k = 33", UNSUPPORTED, (0, 0, 10, good + [(2.55, 600, 33)])), ("no frames", ARG, (0, 0, 0, good)),
             ("slots outside the ring", ARG, (0, 20, 10, good)), ("a negative slot", ARG, (-1, 0, 10, good)),
             ("chunk_frames above the limit", ARG, (0, 0, 10, good, Nat.SWEEP_MAX_CHUNK + 1))]
    for what, code, args in cases:
        assert rc(*args) == code, what
        assert lib.cbv_last_error(p.ctx.h)
    assert rc(0, 0, 10, good, ns=0) == ARG and rc(0, 0, 10, good, ns=Nat.SWEEP_MAX_SETTINGS + 1) == ARG
    assert lib.cbv_pipeline_sweep(p.h_, 0, 0, 10, None, 1, 0, None, None, None) == ARG
    assert lib.cbv_pipeline_sweep(None, 0, 0, 10, None, 1, 0, None, None, None) == ARG
    out = np.zeros((64, 256), np.uint16)
    assert lib.cbv_pipeline_change_hist(p.h_, 0, 15, 13, Nat.ptr(out)) == STATE
    assert lib.cbv_pipeline_change_hist(p.h_, 0, 5, 33, Nat.ptr(out)) == UNSUPPORTED
    assert lib.cbv_pipeline_change_hist(p.h_, 0, 5, 13, None) == ARG and not out.any()
    with pytest.raises(RuntimeError):
        p.sensitivity_sweep(0, 5, 10, settings=good)
    valid = p.sensitivity_sweep(0, 0, 10, settings=GRID)
    assert _same_records(valid.records, res.records[:, :10])
    _assert_snapshots_equal(_snapshot(p, 10), before, "after the rejected calls")
    from chessboard_vision_amd.stream import BoardPipeline
    fresh = BoardPipeline(W, H, 4)
    sets = np.zeros(1, Nat.record_dtype(Nat.SweepSetting))
    sets[0] = good[0]
    assert lib.cbv_pipeline_sweep(fresh.h_, 0, 0, 1, Nat.ptr(sets), 1, 0, None, None, None) == STATE  # not configured
    fresh.close()
    p.close()
