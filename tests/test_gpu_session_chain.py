"""The reference's session chain in the device-resident pipeline: BoardPipeline.configure(enhance=False) =
warp -> [rotate 180] -> split -> detect on the camera frame as it is (GameSession.on_frame, calibrate_sensitivity.py), and
the warp that samples NV12 / YUYV frames directly (k_warp_yuv) when such a pipeline is fed raw frames.

Yardsticks: the recorded reference run tests/golden/ref_piece_sequence.json; tests/ref_logic.py and
tests/model_update_ref.py (pinned to the reference by tests/test_reference_runs.py) on the oracle's warp of oracle frames;
for the fused warp, an enhance=False pipeline fed the frames board_detection.yuv_to_bgr converted.  Tolerance 0 everywhere."""
import functools

import numpy as np
import pytest

import model_update_ref as MR
import ref64_yuv as Y
import refrun as R
from chessboard_vision_amd import synth as S
from helpers import oracle_frame, random_frame

pytestmark = pytest.mark.gpu

FMTS = ("nv12", "yuyv")
ALL = [(f, r) for f in range(8) for r in range(8)]


def _kids():
    """profiling id of every kernel by name"""
    from chessboard_vision_amd import _native as N
    return N.K_ALL


def _words(res):
    return [(r.raw_occupied, r.stable_occupied, r.visual_changes, r.processed, r.changed, r.parcial, r.total, r.circular) for r in res]


def _grid_lines(kind):
    return (S.CALIB_GRID_X, S.CALIB_GRID_Y) if kind.startswith("smart") else None


def _extractor(kind):
    from chessboard_vision_amd.grid_extractor import GridExtractor, SmartGridExtractor
    if not kind.startswith("smart"):
        return GridExtractor()
    ge = SmartGridExtractor()
    ge.grid_lines_x, ge.grid_lines_y = list(S.CALIB_GRID_X), list(S.CALIB_GRID_Y)
    return ge


def _roi_bits(positions, rois_rc):
    """{(file, rank)} -> the pipeline's bitset (bit = roi index)"""
    roi_of = {(c, 7 - r): i for i, (r, c) in enumerate(rois_rc)}
    m = 0
    for pos in positions:
        m |= 1 << roi_of[tuple(pos)]
    return m


# ------------------------------------------------------------------------------------------------------------------
# 1. the reference's own run
# ------------------------------------------------------------------------------------------------------------------
def test_recorded_reference_run_frames_0_to_16(gpu_ctx):
    """Frames 0..16 of ref_piece_sequence.json (PieceDetector driven like GameSession.on_frame: use_delta=True, default
    smoothing; frames 17..25 use keyword arguments the pipeline has no counterpart for): warped board, visual changes,
    stable occupancy and the raw has_piece of every result row, 17 of the 26 recorded frames."""
    from chessboard_vision_amd.stream import BoardPipeline, bits_to_positions
    fx = R.load_json("ref_piece_sequence.json")
    w, h = fx["size"]
    n = 17
    frames = fx["frames"][:n]
    assert all(rec["kwargs"] == {"use_delta": True} for rec in frames) and fx["frames"][n]["kwargs"] != {"use_delta": True}
    assert fx["script"]["update_references_after"] == 13
    p = BoardPipeline(w, h, n)
    p.configure(S.scaled_corners(w, h), grid_lines=_grid_lines(fx["grid"]), enhance=False, chunk=5, lanes=2,
                min_radius_ratio=fx["settings"]["min_radius_ratio"], max_radius_ratio=fx["settings"]["max_radius_ratio"])
    p.synth(0, n, stream_id=fx["stream_id"], scene=fx["scene"], frames_per_ply=fx["script"]["frames_per_ply"])
    p.set_check_squares(0, [None if rec["to_check_bits"] is None else R.unbits(rec["to_check_bits"]) for rec in frames])
    p.run(0, 14)
    p.update_references(13)
    p.run(14, 3)
    res = p.results(0, n)
    for rec in frames:
        i = rec["i"]
        assert R.sha(p.download(2, i)) == rec["warped_sha256"], ("warped", i)
        assert R.bits(bits_to_positions(res[i].visual_changes, p.rois_rc)) == rec["visual_bits"], ("visual", i)
        assert R.bits(p.occupied(res[i], stable=True)) == rec["occupied_bits"], ("stable", i)
        # The rows: has_piece is the smoothed value (piece_detector.py:425-431), the other fields are the raw detection's,
        # whose method is set exactly when it found a piece; the same set is what the detector cached.
        assert R.bits((row[0], row[1]) for row in rec["results"] if row[2]) == rec["occupied_bits"], ("rows, stable", i)
        raw_rows = R.bits((row[0], row[1]) for row in rec["results"] if row[3] is not None)
        assert raw_rows == rec["state"]["cached_has_bits"], ("fixture", i)
        assert R.bits(p.occupied(res[i], stable=False)) == raw_rows, ("raw", i)
    p.close()


# ------------------------------------------------------------------------------------------------------------------
# 2. long streams against the restated reference logic
# ------------------------------------------------------------------------------------------------------------------
W2, H2, N2 = 1920, 1080, 96
# (scene, grid, rot180, use_hough)
LONG = [("normal", "linear", False, 1), ("dim", "smart", True, 1), ("normal", "smart", True, 0), ("dim", "linear", False, 0)]


@functools.lru_cache(maxsize=None)
def _reference_words(scene, grid, rot180, use_hough):
    """(raw, stable, visual, processed) of every frame: RefPieceDetector on oracle.warp_image of the oracle's frames"""
    from oracle import cbv_oracle as O
    from ref_logic import RefPieceDetector
    det, ge = RefPieceDetector(hough={} if use_hough else None), _extractor(grid)
    pts = S.scaled_corners(W2, H2)
    out = []
    for i in range(N2):
        warped = O.warp_image(oracle_frame(W2, H2, scene, stream_id=4, frame_idx=i, frames_per_ply=6), pts)[0]
        if rot180:
            warped = O.rotate180(warped)
        res, vis = det.detect_all_pieces(ge.split_board(warped), use_delta=True)
        out.append(({p for p, r in det.cached_results.items() if r["has_piece"]}, {p for p, r in res.items() if r["has_piece"]},
                    set(vis), set(det.last_processed)))
    return out


@pytest.mark.parametrize("scene,grid,rot180,use_hough", LONG, ids=lambda v: str(v))
def test_long_stream_equals_reference_logic(gpu_ctx, oracle, scene, grid, rot180, use_hough):
    """96 frames of 1080p; chunk in {1, 5, 64} x lanes in {1, 2, 4}, one run and runs of 1..7 frames: all eight result
    words of every frame (the four ChangeDetector words are zero: nothing was calibrated)."""
    from chessboard_vision_amd.stream import BoardPipeline
    ref = _reference_words(scene, grid, rot180, use_hough)
    p = BoardPipeline(W2, H2, N2)
    p.synth(0, N2, stream_id=4, scene=scene, frames_per_ply=6)
    want = None
    for chunk in (1, 5, 64):
        for lanes in (1, 2, 4):
            p.configure(S.scaled_corners(W2, H2), grid_lines=_grid_lines(grid), rot180=rot180, use_hough=bool(use_hough),
                        chunk=chunk, lanes=lanes, enhance=False)
            if want is None:
                want = [tuple(_roi_bits(s, p.rois_rc) for s in row) + (0, 0, 0, 0) for row in ref]
                assert len({w_[0] for w_ in want}) > 4 and any(w_[2] for w_ in want[1:])  # pieces move, changes are seen
            p.run(0, N2)
            got = _words(p.results(0, N2))
            bad = [i for i in range(N2) if got[i] != want[i]]
            assert not bad, ("one run", chunk, lanes, bad[:5], got[bad[0]], want[bad[0]])
            if (chunk, lanes) in ((1, 4), (5, 2), (64, 1), (5, 4)):
                p.reset_state()
                s0 = k = 0
                while s0 < N2:  # runs of 1, 2, .. 7, 1, 2, .. frames, nothing read in between
                    c = min(1 + k % 7, N2 - s0)
                    p.run(s0, c)
                    s0, k = s0 + c, k + 1
                assert _words(p.results(0, N2)) == want, ("runs of 1..7", chunk, lanes)
    p.close()


# ------------------------------------------------------------------------------------------------------------------
# 3. the ChangeDetector stage
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _raw_squares():
    """the yardstick stream of tests/model_update_ref.py without enhancement: synth -> warp -> split"""
    from oracle import cbv_oracle as O
    from chessboard_vision_amd.grid_extractor import GridExtractor
    pts = S.scaled_corners(MR.W, MR.H)
    return [GridExtractor().split_board(O.warp_image(oracle_frame(MR.W, MR.H, "normal", frame_idx=i, frames_per_ply=MR.FRAMES_PER_PLY), pts)[0])
            for i in range(MR.N_FRAMES)]


@pytest.mark.parametrize("params", [MR.PARAMS_A, MR.PARAMS_B], ids=["z2.55_iv600_a0.1", "z1.45_iv50_a0.37"])
@pytest.mark.parametrize("mode", MR.MODES)
def test_change_detector_stage_and_model_update(gpu_ctx, oracle, mode, params):
    """calibrate_changes on frame 0, then the three model-update modes: every frame's detect_changes_detailed dict and the
    mean and variance planes of all 64 squares after the stream, bit for bit."""
    from chessboard_vision_amd.stream import BoardPipeline
    sq, n = _raw_squares(), MR.N_FRAMES
    ref = MR.new_ref(params)
    ref.calibrate(sq[0])
    dicts = [MR.step(ref, mode, s) for s in sq]
    assert sum(1 for d in dicts if d) >= 4  # the stream does report changes
    p = BoardPipeline(MR.W, MR.H, n)
    p.configure(S.scaled_corners(MR.W, MR.H), chunk=4, lanes=2, z_threshold=params[0], initial_variance=params[1], enhance=False)
    p.synth(0, n, scene="normal", frames_per_ply=MR.FRAMES_PER_PLY)
    p.run(0, 1)
    p.calibrate_changes(0)
    p.reset_state()
    p.set_model_update(mode, params[2])
    for s0, c in ((0, 1), (1, 2), (3, 3), (6, 7), (13, 5), (18, 10)):
        p.run(s0, c)
    res = p.results(0, n)
    for i in range(n):
        got = p.changes_detailed(res[i], i)
        assert got == dicts[i], (mode, i, got, dicts[i])
    for pos in ALL:
        mean, var = p.model(pos)
        assert mean.dtype == var.dtype == ref.means[pos].dtype == np.float32
        assert np.array_equal(mean, ref.means[pos]) and np.array_equal(var, ref.variances[pos]), (mode, pos)
    p.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. the warp straight from NV12 / YUYV
# ------------------------------------------------------------------------------------------------------------------
def _raw_frames(fmt, w, h, n, content, seed=0):
    """n raw frames; `content`: "game" (a scripted game's frames), "smooth", "noise" (uniform bytes: Y < 16, Y > 235 and
    chroma that saturates every channel), "two" (every byte 0 or 255)"""
    shape = (h * 3 // 2, w) if fmt == "nv12" else (h, w, 2)
    rng = np.random.default_rng(seed)
    if content == "noise":
        return [rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(n)]
    if content == "two":
        return [(rng.integers(0, 2, shape, dtype=np.uint8) * 255).astype(np.uint8) for _ in range(n)]
    if content == "smooth":
        base = [Y.from_bgr(random_frame(w, h, seed + k), fmt) for k in range(3)]
        return [np.roll(base[i % 3], 7 * (i // 3), axis=1 if fmt == "nv12" else 0).copy() for i in range(n)]
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(w, h, n)
    p.synth(0, n, scene="normal", frames_per_ply=2)
    out = [Y.from_bgr(p.download(0, i), fmt) for i in range(n)]
    p.close()
    return out


def _everything(p, n, hough):
    """every observable of the boards of a pipeline after its runs"""
    out = []
    for b in [p] + list(p._boards):
        out.append([bytes(b.results(0, n)), repr(b.noise_results(0, n))] + [bytes(b.square_stats(i)) for i in range(n)]
                   + ([bytes(b.hough(i)) for i in range(n)] if hough else []) + [b.download(2, i).tobytes() for i in range(n)])
    return out


def _quads(w, h):
    pts = S.scaled_corners(w, h)
    return {"inside": pts,
            "partly_outside": pts + np.float32([0.42 * w, -0.3 * h]),   # the right and top parts of the quad leave the frame
            "partly_outside_lb": pts + np.float32([-0.42 * w, 0.3 * h]),  # ... and the left and bottom parts
            "mirrored": pts[[1, 0, 3, 2]].copy()}


# boards attached next to board 0: different sizes (S = min(display_size) - margin), geometry and rotation
ATTACHED = [dict(display_size=(800, 600), margin=100, rot180=True), dict(display_size=(640, 480), margin=80),
            dict(display_size=(1280, 420), margin=100, rot180=True), dict(display_size=(1280, 720), margin=100)]


def _make(w, h, n, quad, rot180, hough, boards, chunk=0):
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(w, h, n)
    p.configure(quad, rot180=rot180, use_hough=hough, chunk=chunk, lanes=2, enhance=False)
    for k in range(boards):
        p.add_board(quad + np.float32(3 * (k + 1)), use_hough=hough, **ATTACHED[k])
    return p


def _runs(p, n):
    p.run(0, n - 1)  # groups of four frames per thread, the last one short
    p.run(n - 1, 1)  # one frame per thread


def _strided_nv12(frame, h):
    """(y, uv) views whose rows are further apart than their length, the planes in separate buffers"""
    w = frame.shape[1]
    ybuf, cbuf = np.full((h, w + 24), 0xA5, np.uint8), np.full((h // 2, w + 10), 0x5A, np.uint8)
    ybuf[:, 3:3 + w], cbuf[:, 8:8 + w] = frame[:h], frame[h:]
    return ybuf[:, 3:3 + w], cbuf[:, 8:8 + w]


def _check_fused(gpu_ctx, fmt, w, h, n, content, quad, rot180, boards, seed=0):
    from chessboard_vision_amd.board_detection import yuv_to_bgr
    hough = content in ("game", "smooth")  # (noise and two-level squares can overflow HoughCircles' candidate lists)
    raw = _raw_frames(fmt, w, h, n, content, seed)
    bgr = [yuv_to_bgr(f, fmt) for f in raw]
    ref = _make(w, h, n, quad, rot180, hough, boards)
    for i in range(n):
        ref.upload(i, bgr[i])
    _runs(ref, n)
    want = _everything(ref, n, hough)
    ref.close()
    p = _make(w, h, n, quad, rot180, hough, boards)
    p.set_input_format(fmt)
    ring = p.host_ring()
    for i in range(n):
        ring[i] = raw[i]
    gpu_ctx.profile_reset()
    gpu_ctx.profile_enable(-1)
    try:
        p.submit(0, n - 1)
        p.submit(n - 1, 1)
        _runs(p, n)
        got = _everything(p, n, hough)
        counts = {k: gpu_ctx.profile_read(kid)[1] for k, kid in _kids().items()}
    finally:
        gpu_ctx.profile_enable(-2)
        gpu_ctx.profile_reset()
    assert counts["WARP_YUV"] == 2 and counts["WARP"] == 0 and counts["INGEST"] == 0, counts
    what = (fmt, w, h, content, rot180, boards)
    for b, (g_, w_) in enumerate(zip(got, want)):
        for i in range(n):
            assert g_[-n + i] == w_[-n + i], what + ("board", b, "warped frame", i)
        assert g_ == w_, what + ("board", b)
    for i in (0, n - 1):
        assert np.array_equal(p.download(0, i), bgr[i]), what + ("download(0)", i)
    # the synchronous path: the slots overwritten, then the same frames through upload(fmt=...), strided planes included
    for b in [p] + list(p._boards):
        b.reset_state()
    for i in range(n):
        p.upload(i, np.zeros_like(raw[i]), fmt=fmt)
    for i in range(n):
        p.upload(i, _strided_nv12(raw[i], h) if fmt == "nv12" and i % 2 else raw[i], fmt=fmt)
    _runs(p, n)
    assert _everything(p, n, hough) == want, what + ("upload",)
    p.close()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", [(640, 480), (322, 242)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("content", ["game", "smooth", "noise", "two"])
def test_fused_yuv_warp_equals_convert_then_warp(gpu_ctx, fmt, size, content):
    """widths = 0 and 2 mod 4; a quad inside the frame, two partly outside it (right / top, left / bottom) and a mirrored
    one; both rotations"""
    w, h = size
    for k, (name, quad) in enumerate(_quads(w, h).items()):
        _check_fused(gpu_ctx, fmt, w, h, 10, content, quad, rot180=bool(k % 2) ^ (content == "noise"), boards=0, seed=k)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("boards", [1, 4])
def test_fused_yuv_warp_with_attached_boards(gpu_ctx, fmt, boards):
    for w, h in ((640, 480), (322, 242)):
        quads = _quads(w, h)
        _check_fused(gpu_ctx, fmt, w, h, 10, "game", quads["inside"], rot180=False, boards=boards)
        _check_fused(gpu_ctx, fmt, w, h, 10, "noise", quads["partly_outside"], rot180=True, boards=boards, seed=5)


def test_fused_yuv_warp_4k(gpu_ctx):
    w, h = 3840, 2160
    _check_fused(gpu_ctx, "nv12", w, h, 9, "smooth", _quads(w, h)["inside"], rot180=True, boards=1, seed=11)


# ------------------------------------------------------------------------------------------------------------------
# 5. off means off
# ------------------------------------------------------------------------------------------------------------------
ENHANCEMENT = ("COLOR_LAB_HIST", "CLAHE_LUT", "CLAHE_APPLY", "BILATERAL", "SHARPEN", "NORM_LUT", "NORMALIZE", "RESET")
# Launches per kernel of the run below on a default pipeline, counted on the commit before this feature (the same
# script, the same library entry points): what "nothing moves with the feature off" means for launches.
PARENT_COUNTS = {"COLOR_LAB_HIST": 3, "CLAHE_LUT": 3, "CLAHE_APPLY": 3, "BILATERAL": 3, "SHARPEN": 3, "NORM_LUT": 3, "WARP": 3,
                 "SQUARES": 3, "SCAN": 1, "HOUGH": 3}


def _counted(ctx, p, n, submit=False):
    """launches per kernel of one run of n frames (+ the submit in front of it) after a warm-up run"""
    p.run(0, n)
    p.results(0, n)
    ctx.profile_reset()
    ctx.profile_enable(-1)
    try:
        if submit:
            p.submit(0, n)
        p.run(0, n)
        p.results(0, n)
        return {k: ctx.profile_read(kid)[1] for k, kid in _kids().items() if ctx.profile_read(kid)[1]}
    finally:
        ctx.profile_enable(-2)
        ctx.profile_reset()


def test_off_means_off(gpu_ctx):
    from chessboard_vision_amd.stream import BoardPipeline
    w, h, n = 640, 480, 12
    pts = S.scaled_corners(w, h)

    def make(frames=n, **kw):
        p = BoardPipeline(w, h, frames)
        p.configure(pts, profile=S.SHIPPED_PROFILE, chunk=4, lanes=1, **kw)
        return p

    p = make()
    p.synth(0, n, scene="normal", frames_per_ply=2)
    default = _counted(gpu_ctx, p, n)
    p.close()
    assert default == PARENT_COUNTS, default
    p = make(enhance=False)
    p.synth(0, n, scene="normal", frames_per_ply=2)
    off = _counted(gpu_ctx, p, n)
    p.close()
    assert not any(k in off for k in ENHANCEMENT + ("WARP_YUV", "INGEST")), off
    assert off == {k: v for k, v in default.items() if k not in ENHANCEMENT}, (off, default)
    for fmt in FMTS:
        p = make(enhance=False)
        p.set_input_format(fmt)
        p.host_ring()[:] = 128
        p.submit(0, n)
        raw = _counted(gpu_ctx, p, n, submit=True)
        p.close()
        assert "INGEST" not in raw and "WARP" not in raw and raw.pop("WARP_YUV") == off["WARP"], (fmt, raw)
        assert raw == {k: v for k, v in off.items() if k != "WARP"}, (fmt, raw, off)
    # one frame: the same number of launches whatever the number of boards
    totals = {}
    for boards in (0, 3):  # 1 and 4 boards
        for kw in (dict(), dict(enhance=False)):
            p = make(frames=2, **kw)
            for k in range(boards):
                p.add_board(pts + np.float32(2 * (k + 1)), **ATTACHED[k])
            p.synth(0, 2, scene="normal", frames_per_ply=2)
            totals[(boards, bool(kw))] = sum(_counted(gpu_ctx, p, 1).values())
            p.close()
    assert totals[(0, False)] == totals[(3, False)] and totals[(0, True)] == totals[(3, True)] < totals[(0, False)], totals


# ------------------------------------------------------------------------------------------------------------------
# 6. errors
# ------------------------------------------------------------------------------------------------------------------
def test_errors_name_their_cause(gpu_ctx):
    from chessboard_vision_amd.stream import BoardPipeline
    w, h = 640, 480
    pts = S.scaled_corners(w, h)
    p = BoardPipeline(w, h, 2)
    with pytest.raises(Exception, match="keep_enhanced"):
        p.configure(pts, enhance=False, keep_enhanced=True)
    with pytest.raises(Exception, match="enhance_region"):
        p.configure(pts, enhance=False, enhance_region=True)
    p.configure(pts, enhance=False)
    p.synth(0, 2)
    p.run(0, 2)
    with pytest.raises(Exception, match="without enhancement"):
        p.download(1, 0)
    assert p.download(0, 0).shape == (h, w, 3) and p.download(2, 0).shape == (620, 620, 3)
    for fmt in FMTS:
        p.set_input_format(fmt)
        with pytest.raises(Exception, match="raw mode"):
            p.synth(0, 2)
        with pytest.raises(Exception, match="raw mode"):
            p.upload(0, np.zeros((h, w, 3), np.uint8))
        other = "yuyv" if fmt == "nv12" else "nv12"
        with pytest.raises(Exception, match="raw mode"):
            p.upload(0, np.zeros((h * 3 // 2, w) if other == "nv12" else (h, w, 2), np.uint8), fmt=other)
        with pytest.raises(Exception, match="no raw frame"):
            p.run(0, 1)
        p.upload(0, np.full((h * 3 // 2, w) if fmt == "nv12" else (h, w, 2), 128, np.uint8), fmt=fmt)
        p.run(0, 1)
        assert np.all(p.download(0, 0) == p.download(0, 0)[0, 0]) and p.results(0, 1)[0].processed
    # back to BGR: everything as before
    p.set_input_format("bgr")
    p.synth(0, 2)
    p.run(0, 2)
    # and with enhancement on, a YUV format is converted as it always was: no raw mode
    p.configure(pts)
    p.set_input_format("nv12")
    p.synth(0, 2)
    p.upload(0, np.zeros((h, w, 3), np.uint8))
    p.close()
