"""The profile-only pipeline mode (configure(enhance="profile"), k_warp_profile in the run) and the colour profile sweep
(cbv_pipeline_color_sweep) against the yardstick of tests/color_sweep_ref.py: the oracle's apply_color_profile ->
warp_image -> split_board and the restated reference class, the recorded run of the reference's own classes, and the
product's own per-profile path.  640x480, 8 frames, two palettes, eleven profiles.  Tolerance 0."""
import functools
import random

import numpy as np
import pytest

from chessboard_vision_amd import _native as Nat
from chessboard_vision_amd import synth as S
import color_sweep_ref as CS
import piece_sweep_ref as PS
import refrun

pytestmark = pytest.mark.gpu

ARG, STATE, UNSUPPORTED = -1, -4, -5
W, H, N = CS.W, CS.H, CS.N_FRAMES
PTS = S.scaled_corners(W, H)
ALL = [(f, r) for f in range(8) for r in range(8)]
PROFS = [CS.PROFILES[name] for name in CS.NAMES]
GRID = (tuple(S.CALIB_GRID_X), tuple(S.CALIB_GRID_Y))
_same = PS.same_records


def _pipeline(palette="low", enhance=False, profile=None, n=N, chunk=4, lanes=2, run=False, **kw):
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, n)
    p.configure(PTS, profile=profile, chunk=chunk, lanes=lanes, enhance=enhance, **kw)
    p.synth(0, n, scene=CS.native_scene(palette), frames_per_ply=CS.FRAMES_PER_PLY)
    if run:
        p.run(0, n)
    return p


def _words(res):
    return [(r.raw_occupied, r.stable_occupied, r.visual_changes, r.processed, r.changed, r.parcial, r.total, r.circular) for r in res]


def _snapshot(b, n=N):
    return (bytes(b.results(0, n)), [bytes(b.square_stats(i)) for i in range(n)], [bytes(b.hough(i)) for i in range(n)],
            [b.download(2, i).tobytes() for i in range(n)], [(st.name, sorted(d.items(), key=str)) for st, d in b.noise_results(0, n)])


@functools.lru_cache(maxsize=None)
def _session_words(name, grid=None):
    """(raw, stable, visual, processed) roi bitsets of every frame: RefPieceDetector driven as the pipeline drives it
    (use_delta=True, nothing checked) on the oracle's chain under the profile"""
    from ref_logic import RefPieceDetector
    det = RefPieceDetector(hough=PS.hough_kw(CS.HOUGH))
    out = []
    for sq in CS.stream_squares("low", name, N, grid):
        res, vis = det.detect_all_pieces(sq, use_delta=True)
        out.append((PS.bits(p for p, r in det.cached_results.items() if r["has_piece"]), PS.bits(p for p, r in res.items() if r["has_piece"]),
                    PS.bits(vis), PS.bits(det.last_processed)) + (0, 0, 0, 0))
    return out


# 1 --- the pipeline mode -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CS.PIPELINE_PROFILES)
def test_profile_mode_equals_the_oracle_chain(gpu_ctx, name):
    """download(2, slot) = warp_image(apply_color_profile(frame)) and the eight result words = the reference logic on the
    oracle's chain; chunk 1 / 4 / 8 (a chunk of 8 takes the four-frames-per-thread form), lanes 1 / 2, one run and split runs"""
    want = _session_words(name)
    p = _pipeline(enhance="profile", profile=CS.PROFILES[name])
    for chunk, lanes, split in ((1, 1, (8,)), (4, 2, (8,)), (8, 1, (8,)), (4, 1, (3, 5)), (1, 2, (1, 2, 5)), (8, 2, (8,))):
        p.configure(PTS, profile=CS.PROFILES[name], chunk=chunk, lanes=lanes, enhance="profile")
        s0 = 0
        for cnt in split:
            p.run(s0, cnt)
            s0 += cnt
        got = _words(p.results(0, N))
        assert got == want, (name, chunk, lanes, split, [i for i in range(N) if got[i] != want[i]])
        for i in range(N):
            assert np.array_equal(p.download(2, i), CS.warped("low", name, i)), (name, chunk, lanes, split, i)
    # rotated: the warped board is the oracle's, rotated
    p.configure(PTS, profile=CS.PROFILES[name], chunk=8, lanes=1, enhance="profile", rot180=True)
    p.run(0, N)
    for i in (0, 7):
        assert np.array_equal(p.download(2, i), CS.warped("low", name, i, True)), (name, "rot180", i)
    p.close()


@pytest.mark.parametrize("chunk", [4, 8])
def test_an_attached_board_with_irregular_squares_equals_a_pipeline_of_its_own(gpu_ctx, chunk):
    """SmartGridExtractor squares of 76..80 px on a board attached to a profile-mode pipeline (the multi-board warp), against
    the reference logic on the oracle's chain and against a pipeline configured with that grid"""
    name = "radical"
    p = _pipeline(enhance="profile", profile=CS.PROFILES[name], chunk=chunk)
    b = p.add_board(PTS, grid_lines=GRID)
    p.run(0, N)
    own = _pipeline(enhance="profile", profile=CS.PROFILES[name], chunk=chunk, grid_lines=GRID, run=True)
    assert len({(b._cfg.rois[i].w, b._cfg.rois[i].h) for i in range(64)}) > 1
    assert _words(b.results(0, N)) == _words(own.results(0, N)) == _session_words(name, GRID)
    assert _words(p.results(0, N)) == _session_words(name)
    for i in range(N):
        assert np.array_equal(b.download(2, i), CS.warped("low", name, i)) and np.array_equal(p.download(2, i), CS.warped("low", name, i))
        assert bytes(b.square_stats(i)) == bytes(own.square_stats(i))
    for q in (b, p, own):
        q.close()


def test_nv12_fed_equals_bgr_fed(gpu_ctx):
    """with a YUV input format the mode converts into the BGR ring (no raw mode): same boards and results as the same
    pipeline fed the frames yuv_to_bgr converted"""
    import ref64_yuv as Y
    from chessboard_vision_amd.board_detection import yuv_to_bgr
    raw = [Y.from_bgr(np.array(CS.frame("low", i)), "nv12") for i in range(N)]
    out = {}
    for fmt in ("bgr", "nv12"):
        p = _pipeline(enhance="profile", profile=CS.PROFILES["shipped"])
        if fmt == "nv12":
            p.set_input_format("nv12")
        for i in range(N):
            p.upload(i, raw[i] if fmt == "nv12" else yuv_to_bgr(raw[i], "nv12"), fmt=fmt)
        p.run(0, N)
        out[fmt] = _snapshot(p) + (p.color_sweep(0, N, PROFS[:4]).records.tobytes(),)
        assert np.array_equal(p.download(0, 3), yuv_to_bgr(raw[3], "nv12"))
        p.close()
    assert out["nv12"] == out["bgr"]
    plain = _pipeline(enhance=False, run=True)
    assert out["bgr"][3] != [plain.download(2, i).tobytes() for i in range(N)]  # the profile did act
    plain.close()


def test_a_disabled_profile_is_the_session_chain(gpu_ctx):
    want = None
    for enhance, profile in ((False, None), ("profile", None), ("profile", {})):
        p = _pipeline(enhance=enhance, profile=profile, run=True)
        snap = _snapshot(p)
        want = want or snap
        assert snap == want, (enhance, profile)
        p.close()


def test_mode_errors(gpu_ctx):
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, 2)
    for kw in (dict(keep_enhanced=True), dict(enhance_region=True)):
        with pytest.raises(RuntimeError, match=r"code -1\b"):
            p.configure(PTS, profile=CS.SHIPPED, enhance="profile", **kw)
    with pytest.raises(RuntimeError, match=r"code -1\b"):
        p.configure(PTS, profile=dict(CS.SHIPPED, contrast=float("inf")), enhance="profile")
    p.configure(PTS, profile=CS.SHIPPED, enhance="profile")
    p.synth(0, 2, scene=CS.native_scene("low"))
    p.run(0, 2)
    with pytest.raises(RuntimeError, match=r"code -4\b"):
        p.download(1, 0)
    assert p.download(2, 0).any()
    p.close()


# 2 --- one sweep of every profile ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(CS.PALETTES))
def swept(request, gpu_ctx):
    """A session-chain pipeline that has run, its snapshot, and ONE sweep of the eleven profiles over the 8 frames"""
    p = _pipeline(request.param, enhance=False, run=True)
    before = _snapshot(p)
    res = p.color_sweep(0, N, PROFS, expected=CS.expected_bits())
    yield request.param, p, res, before
    p.close()


def test_one_sweep_equals_the_yardstick(swept):
    palette, p, res, _ = swept
    Y = CS.yardstick_records(palette)
    rec = res.records
    assert rec.shape == (len(PROFS), N) and res.info["chunk_frames"] == N and res.info["chunk_profiles"] == len(PROFS)
    assert res.profiles == PROFS
    PS.assert_records_equal(rec, Y, "device against the reference class")
    exp = CS.expected_bits()
    want = PS.reduce_records(rec, exp, [[r["_radii"] for r in row] for row in Y])
    for name in PS.SUM_FIELDS:
        assert np.array_equal(res.summary[name], want[name]), name
    assert res.summary.tobytes() == want.tobytes()
    assert not res.summary["overflow"].any() and not rec["flags"].any()
    at = CS.NAMES.index
    for j, name in enumerate(CS.NAMES):
        assert (int(res.summary["missed"][j]), int(res.summary["false_pos"][j]), int(res.summary["frames_exact"][j])) == CS.summary_of(Y[j], exp), name
    if palette == "lilac":
        assert res.summary["missed"][at("sat3")] < res.summary["missed"][at("none")] and res.best() in (at("sat3"), at("radical_lilac"))
    else:
        assert res.best() == at("none") and not _same(rec[at("none"):at("none") + 1], rec[at("neutral"):at("neutral") + 1])
        # the recorded run of the reference's own classes
        fx = refrun.load_json("ref_color_profiles.json")
        for run in fx["runs"]:
            j = at(run["profile_name"])
            for i, rows in enumerate(run["frames"]):
                assert PS.bits((r[0], r[1]) for r in rows if r[2]) == int(rec["stable_occupied"][j, i]), (j, i)
                for m in PS.METHODS:
                    assert PS.bits((r[0], r[1]) for r in rows if r[3] == m) == int(rec[m][j, i]), (j, i, m)
                assert res.occupied(j, i) == {(r[0], r[1]) for r in rows if r[2]}
    # the entry without a profile = the PieceDetector sweep of the board's own setting on the frames the pipeline has run
    lo, hi, p1, p2 = CS.HOUGH
    base = p.piece_sweep(0, N, settings=[(lo, hi, p1, p2)], expected=exp)
    assert _same(base.records, rec[at("none"):at("none") + 1]) and base.summary.tobytes() == res.summary[at("none"):at("none") + 1].tobytes()


@pytest.mark.parametrize("name", CS.PIPELINE_PROFILES)
def test_sweep_equals_the_per_profile_path(swept, name):
    """A board configured with the profile (enhance="profile", use_hough=2: HoughCircles on every non-uniform square), every
    square in the check set of every slot, reports the sweep's raw and smoothed occupancy."""
    palette, _, res, _ = swept
    j = CS.NAMES.index(name)
    q = _pipeline(palette, enhance="profile", profile=CS.PROFILES[name], use_hough=2)
    q.reset_state()
    q.set_check_squares(0, [set(ALL)] * N)
    q.run(0, N)
    out = q.results(0, N)
    for i in range(N):
        assert (out[i].raw_occupied, out[i].stable_occupied) == (int(res.raw_occupied[j, i]), int(res.stable_occupied[j, i])), i
    # ... and the PieceDetector sweep of the board's own setting on that pipeline's slots is the profile's row
    lo, hi, p1, p2 = CS.HOUGH
    own = q.piece_sweep(0, N, settings=[(lo, hi, p1, p2)], expected=CS.expected_bits())
    assert _same(own.records, res.records[j:j + 1]) and own.summary.tobytes() == res.summary[j:j + 1].tobytes()
    q.close()


# 3 --- invariance --------------------------------------------------------------------------------------------------------
def test_chunks_order_duplicates_and_slot0(swept):
    palette, p, res, _ = swept
    exp = CS.expected_bits()
    for chunk in (1, 5, 16):
        got = p.color_sweep(0, N, PROFS, expected=exp, chunk_frames=chunk)
        assert got.info["chunk_frames"] == min(chunk, N)
        assert _same(got.records, res.records) and got.summary.tobytes() == res.summary.tobytes(), chunk
    # shuffled, with duplicates, enough of them for several chunks of profiles
    order = list(range(len(PROFS))) * 6
    random.Random(7).shuffle(order)
    got = p.color_sweep(0, N, [PROFS[j] for j in order], expected=exp)
    assert got.info["chunk_profiles"] < len(order)
    assert _same(got.records, res.records[order]) and got.summary.tobytes() == res.summary[order].tobytes()
    only = p.color_sweep(0, N, PROFS, expected=exp, records=False)
    assert only.records is None and only.summary.tobytes() == res.summary.tobytes()
    with pytest.raises(RuntimeError):
        only.occupied(0, 0)
    # a later slot0: the history starts there
    late = p.color_sweep(3, N - 3, PROFS[:4], expected=exp[3:])
    assert np.array_equal(late.raw_occupied, res.raw_occupied[:4, 3:]) and np.array_equal(late.hough, res.hough[:4, 3:])
    assert np.array_equal(late.stable_occupied[:, 4], res.stable_occupied[:4, 7])  # five frames on, the histories hold the same frames


def test_the_pipelines_mode_does_not_matter(swept):
    """the sweep reads the frames as uploaded: enhance=True (whose runs never write the frame ring), "profile" and a
    pipeline that never ran give the records of the session-chain pipeline"""
    palette, _, res, _ = swept
    exp = CS.expected_bits()
    for enhance, profile, run in ((True, CS.SHIPPED, True), ("profile", CS.PROFILES["radical"], True), (False, None, False)):
        q = _pipeline(palette, enhance=enhance, profile=profile, run=run)
        got = q.color_sweep(0, N, PROFS, expected=exp)
        assert _same(got.records, res.records) and got.summary.tobytes() == res.summary.tobytes(), (enhance, run)
        q.close()


def test_an_attached_board_sweeps_with_its_own_grid(gpu_ctx):
    names = ("none", "shipped", "sat3")
    p = _pipeline(enhance=False)
    b = p.add_board(PTS, grid_lines=GRID)
    got = b.color_sweep(0, 6, [CS.PROFILES[n_] for n_ in names])
    want = [[PS.record_of(*fr) for fr in CS.run_profile("low", n_, 6, GRID)] for n_ in names]
    PS.assert_records_equal(got.records, want, "attached board, irregular grid")
    b.close()
    p.close()


# 4 --- no side effects ---------------------------------------------------------------------------------------------------
def test_the_board_is_as_it_was(swept):
    _, p, res, before = swept
    assert _snapshot(p) == before
    p.run(0, N)  # a later run continues from the state the first run left, not from anything the sweep touched
    q = _pipeline(swept[0], enhance=False, run=True)
    q.run(0, N)
    assert _snapshot(p) == _snapshot(q)
    q.close()


def test_errors_change_nothing(gpu_ctx):
    p = _pipeline(enhance=False)
    p.run(0, N)
    before = _snapshot(p)
    lib = p.ctx.lib

    def rc(slot0, count, profiles, chunk=0, np_=None, summary=True):
        profs = (Nat.ColorProfile * max(len(profiles), 1))(*[Nat.ColorProfile.from_dict(d) for d in profiles])
        summ = np.zeros(max(len(profiles), 1), Nat.record_dtype(Nat.PieceSweepSummary))
        return lib.cbv_pipeline_color_sweep(p.h_, slot0, count, profs, len(profiles) if np_ is None else np_, None, chunk, None,
                                            Nat.ptr(summ) if summary else None, None)

    good = CS.SHIPPED
    cases = [("no frames", ARG, (0, 0, [good])), ("count beyond the ring", ARG, (0, N + 1, [good])), ("a negative slot", ARG, (-1, 4, [good])),
             ("slots outside the ring", ARG, (N, 1, [good])), ("a NaN field", ARG, (0, N, [good, dict(good, sat_scale=float("nan"))])),
             ("an infinite field", ARG, (0, N, [dict(good, brightness=float("inf"))])),
             ("chunk_frames above the limit", ARG, (0, N, [good], Nat.SWEEP_MAX_CHUNK + 1)), ("a negative chunk", ARG, (0, N, [good], -1)),
             ("no profiles", ARG, (0, N, [good], 0, 0)), ("too many profiles", ARG, (0, N, [good], 0, Nat.COLOR_SWEEP_MAX_PROFILES + 1)),
             ("no summary", ARG, (0, N, [good], 0, None, False))]
    for what, code, args in cases:
        assert rc(*args) == code, what
        assert lib.cbv_last_error(p.ctx.h)
    assert lib.cbv_pipeline_color_sweep(p.h_, 0, N, None, 1, None, 0, None, None, None) == ARG
    assert lib.cbv_pipeline_color_sweep(None, 0, N, None, 1, None, 0, None, None, None) == ARG
    assert rc(0, N, [good, None]) == 0
    assert _snapshot(p) == before
    p.close()
    from chessboard_vision_amd.stream import BoardPipeline
    fresh = BoardPipeline(W, H, 4)
    profs = (Nat.ColorProfile * 1)(Nat.ColorProfile.from_dict(good))
    summ = np.zeros(1, Nat.record_dtype(Nat.PieceSweepSummary))
    assert lib.cbv_pipeline_color_sweep(fresh.h_, 0, 1, profs, 1, None, 0, None, Nat.ptr(summ), None) == STATE  # not configured
    # raw mode: the frames are NV12, there is no BGR ring to read
    fresh.configure(PTS, enhance=False)
    fresh.set_input_format("nv12")
    assert lib.cbv_pipeline_color_sweep(fresh.h_, 0, 1, profs, 1, None, 0, None, Nat.ptr(summ), None) == UNSUPPORTED
    fresh.close()


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
    """A pipeline that uses neither the mode nor the sweep launches what the session chain always did (8 frames, chunk 4,
    one lane: two chunks); the mode with a disabled profile launches the same; with a profile the warp's launches are
    k_warp_profile's, counted under the warp's id (the enumeration of profile ids is closed), and nothing else changes; the
    runs behind a sweep launch what they did before."""
    def make(enhance, profile=None):
        p = _pipeline(enhance=enhance, profile=profile, lanes=1)

        def run():
            p.run(0, N)
            p.results(0, N)
        run()
        return p, run
    p, run = make(False)
    off = _counts(gpu_ctx, run)
    assert off == {"WARP": 2, "SQUARES": 2, "SCAN": 1, "HOUGH": 2}, off
    for enhance, profile in (("profile", None), ("profile", CS.SHIPPED)):
        q, qrun = make(enhance, profile)
        assert _counts(gpu_ctx, qrun) == off, (enhance, profile)
        q.close()
    sweep = _counts(gpu_ctx, lambda: p.color_sweep(0, N, PROFS, chunk_frames=4))
    assert sweep == {"WARP": 2, "SQUARES": 2}, sweep  # two chunks of frames; the sweep's two own kernels have no id
    assert _counts(gpu_ctx, run) == off
    p.close()
