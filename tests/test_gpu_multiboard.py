"""Several boards per camera frame (cbv_pipeline_add_board): every attached board computes exactly what a pipeline of its
own computes on the same frames, its state stays its own, it matches the CPU oracle chain, and boards add no launches."""
import ctypes as C

import numpy as np
import pytest

from chessboard_vision_amd import synth as S
from helpers import oracle_scene

pytestmark = pytest.mark.gpu

W, H = 1920, 1080
RUNS = (1, 2, 37, 56)  # 96 frames: one- and two-frame runs (inline scan), long runs over the lanes
N_FRAMES = sum(RUNS)

QUAD_A = S.scaled_corners(W // 2, H)                       # left half, linear grid
QUAD_B = QUAD_A + np.float32([W // 2, 0])                   # right half, smart grid, rot180
QUAD_C = np.float32([[800, 300], [1130, 340], [770, 640], [1100, 690]])  # small, tilted, across the seam

BOARDS = [
    dict(points=QUAD_A),
    dict(points=QUAD_B, grid_lines=(S.CALIB_GRID_X, S.CALIB_GRID_Y), rot180=True),
    dict(points=QUAD_C, display_size=(400, 400), margin=80, use_hough=2, min_radius_ratio=0.15, max_radius_ratio=0.45,
         hough_param2=22, change_threshold=20, history_size=4),
]


def _render(oracle, quad, k):
    from chessboard_vision_amd.board_detection import get_perspective_transform
    Hinv = get_perspective_transform(np.float32(quad), S.BOARD_UNIT_QUAD)
    board = S.board_array(S.position_for_frame(k, 8))
    return oracle.synth_frame(S.frame_seed(7, k), W, H, Hinv, board, oracle_scene("normal"))


@pytest.fixture(scope="module")
def frames(oracle):
    out = []
    for k in range(N_FRAMES):
        a, b = _render(oracle, QUAD_A, k), _render(oracle, QUAD_B, k + 3)
        f = a.copy()
        f[:, W // 2:] = b[:, W // 2:]
        out.append(f)
    return out


def _enh_kw(keep_enhanced, region, lanes):
    return dict(profile=S.SHIPPED_PROFILE, chunk=16, lanes=lanes, keep_enhanced=keep_enhanced, enhance_region=region)


def _board_kw(spec):
    kw = dict(spec)
    kw.pop("points")
    return kw


def _single(frames, enh, spec):
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, N_FRAMES)
    p.configure(spec["points"], **enh, **_board_kw(spec))
    for k, f in enumerate(frames):
        p.upload(k, f)
    return p


def _multi(frames, enh):
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, N_FRAMES)
    p.configure(BOARDS[0]["points"], **enh, **_board_kw(BOARDS[0]))
    for k, f in enumerate(frames):
        p.upload(k, f)
    return p, [p] + [p.add_board(spec["points"], **_board_kw(spec)) for spec in BOARDS[1:]]


def _drive(runner, mid=None):
    s0 = 0
    for n in RUNS:
        runner.run(s0, n)
        s0 += n
        if mid is not None and s0 == RUNS[0] + RUNS[1] + RUNS[2]:
            mid(s0)


def _same(a, b, spec, what):
    r_a, r_b = a.results(0, N_FRAMES), b.results(0, N_FRAMES)
    assert bytes(r_a) == bytes(r_b), what + ": results"
    assert a.noise_results(0, N_FRAMES) == b.noise_results(0, N_FRAMES), what + ": noise_results"
    for k in range(N_FRAMES):
        assert np.array_equal(a.download(2, k), b.download(2, k)), "%s: warped board of slot %d" % (what, k)
        assert bytes(a.square_stats(k)) == bytes(b.square_stats(k)), "%s: square_stats of slot %d" % (what, k)
        if spec.get("use_hough", True):
            assert bytes(a.hough(k)) == bytes(b.hough(k)), "%s: hough of slot %d" % (what, k)


@pytest.mark.parametrize("keep_enhanced,region,lanes", [(False, True, 2), (True, False, 3), (False, False, 2)])
def test_boards_equal_their_single_pipelines(gpu_ctx, frames, keep_enhanced, region, lanes):
    enh = _enh_kw(keep_enhanced, region, lanes)
    p, boards = _multi(frames, enh)
    _drive(p)
    for i, spec in enumerate(BOARDS):
        single = _single(frames, enh, spec)
        _drive(single)
        _same(boards[i], single, spec, "board %d" % i)
        single.close()
    p.close()


def test_board_state_is_isolated(gpu_ctx, frames):
    enh = _enh_kw(False, True, 2)
    p, boards = _multi(frames, enh)
    checks = [{(0, 0), (3, 4), (7, 7)}] * 20

    def poke(target):
        def mid(s):
            target.update_references(s - 1, reset_noise=True)
            target.calibrate_changes(s - 2)
            target.set_check_squares(s, checks)
        return mid

    _drive(p, mid=poke(boards[2]))
    for i, spec in enumerate(BOARDS):
        single = _single(frames, enh, spec)
        _drive(single, mid=poke(single) if i == 2 else None)
        _same(boards[i], single, spec, "board %d" % i)
        single.close()
    # the calls took effect on board C: a background model (z statistics) and forced squares from slot 40 on
    s = RUNS[0] + RUNS[1] + RUNS[2]
    assert any(st.z_max > 0 for st in boards[2].square_stats(s + 3)), "board C has no background model"
    a1 = {i for i, (r, c) in enumerate(boards[2].rois_rc) if (c, 7 - r) in checks[0]}
    assert all((boards[2].results(s, 1)[0].processed >> i) & 1 for i in a1)
    assert not any(st.z_max > 0 for st in boards[1].square_stats(s + 3)), "board B was calibrated too"
    p.close()


def test_two_boards_match_the_oracle_chain(gpu_ctx, oracle):
    from chessboard_vision_amd.grid_extractor import GridExtractor
    from chessboard_vision_amd.stream import BoardPipeline, bits_to_positions
    from helpers import oracle_frame
    from ref_logic import RefPieceDetector
    w, h, n = 640, 480, 6
    pts0 = S.scaled_corners(w, h)
    pts1 = pts0 + np.float32([[6, -4], [-5, 3], [4, 5], [-3, -6]])
    frames = [oracle_frame(w, h, "dim", frame_idx=k, frames_per_ply=2) for k in range(n)]
    p = BoardPipeline(w, h, n)
    p.configure(pts0, profile=S.SHIPPED_PROFILE, chunk=4, lanes=2)
    b1 = p.add_board(pts1)
    for k, f in enumerate(frames):
        p.upload(k, f)
    p.run(0, 2)
    p.run(2, 4)
    for board, pts in ((p, pts0), (b1, pts1)):
        det, ge = RefPieceDetector(hough={}), GridExtractor()
        res = board.results(0, n)
        for k, f in enumerate(frames):
            warped, _, _ = oracle.warp_image(oracle.process_pipeline(f, S.SHIPPED_PROFILE), pts)
            assert np.array_equal(board.download(2, k), warped), "warped board of frame %d" % k
            ref, vis = det.detect_all_pieces(ge.split_board(warped))
            assert bits_to_positions(res[k].stable_occupied, board.rois_rc) == {q for q, r in ref.items() if r["has_piece"]}
            assert bits_to_positions(res[k].raw_occupied, board.rois_rc) == {q for q, r in det.cached_results.items() if r["has_piece"]}
            assert bits_to_positions(res[k].visual_changes, board.rois_rc) == set(vis)
    p.close()


@pytest.mark.parametrize("attached", [0, 1], ids=["1board", "2boards"])
def test_warp_short_last_group_and_taps_outside(gpu_ctx, oracle, attached):
    """the warp with the folded normalize where the runs above do not take it: a quad whose right and top parts leave the
    322 x 242 frame, in one run of 11 frames in one chunk (groups of four frames per thread, the last one of three, the byte
    map from the table) and then in a run of 2 frames (one frame per thread, the byte map worked out from [min, max]), with
    one board (k_warp) and with two (k_warp_mb; the second smaller and rotated), against the oracle's chain"""
    from chessboard_vision_amd.stream import BoardPipeline
    from helpers import oracle_frame
    w, h, n = 322, 242, 13
    quad = S.scaled_corners(w, h) + np.float32([0.42 * w, -0.3 * h])
    assert (quad[:, 0] > w).any() and (quad[:, 1] < 0).any()
    frames = [oracle_frame(w, h, "dim", frame_idx=k, frames_per_ply=2) for k in range(n)]
    p = BoardPipeline(w, h, n)
    p.configure(quad, profile=S.SHIPPED_PROFILE, chunk=11, lanes=1)
    boards = [(p, quad, dict(), False)]
    if attached:
        size = dict(display_size=(800, 600), margin=100)
        boards.append((p.add_board(quad + np.float32(3), rot180=True, **size), quad + np.float32(3), size, True))
    for k, f in enumerate(frames):
        p.upload(k, f)
    p.run(0, 11)
    p.run(11, 2)
    for k, f in enumerate(frames):
        enh = oracle.process_pipeline(f, S.SHIPPED_PROFILE)
        for b, pts, size, rot in boards:
            want = oracle.warp_image(enh, pts, **size)[0]
            assert np.array_equal(b.download(2, k), oracle.rotate180(want) if rot else want), (attached, b is p, k)
    p.close()


def _launches(ctx, n_boards):
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.stream import BoardPipeline
    w, h = 640, 480
    pts = S.scaled_corners(w, h)
    p = BoardPipeline(w, h, 4)
    p.configure(pts, profile=S.SHIPPED_PROFILE)
    for k in range(1, n_boards):
        p.add_board(pts + np.float32(2 * k))
    p.synth(0, 2)
    p.run(0, 1)  # warm-up (first-use launches of the scratch buffers)
    p.results(0, 1)
    ctx.profile_reset()
    ctx.profile_enable(-1)
    try:
        p.run(1, 1)
        p.results(1, 1)
        counts = {}
        for kid in range(16):
            n = ctx.profile_read(kid)[1]
            if n:
                counts[kid] = n
    finally:
        ctx.profile_enable(-2)
        ctx.profile_reset()
    p.close()
    return counts


def test_boards_add_no_launches(gpu_ctx):
    one, four = _launches(gpu_ctx, 1), _launches(gpu_ctx, 4)
    assert one and one == four


def test_error_paths_are_loud(gpu_ctx, frames):
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, 4)
    p.configure(QUAD_A, profile=S.SHIPPED_PROFILE, chunk=2)
    for k in range(4):
        p.upload(k, frames[k])
    extra = [p.add_board(QUAD_A + np.float32(k)) for k in range(1, N.MAX_BOARDS)]
    with pytest.raises(RuntimeError, match=r"code -1\)"):
        p.add_board(QUAD_B)
    for b in extra[1:]:
        b.close()
    b1 = extra[0]
    p.run(0, 2)
    before = [bytes(p.results(0, 2)), bytes(b1.results(0, 2))]
    # a bad ROI: refused, the parent and its board as they were
    cfg = N.BoardConfig()
    C.memmove(C.byref(cfg), C.byref(b1._cfg), C.sizeof(cfg))
    cfg.rois[5].x0 = cfg.board_size
    hdl = C.c_void_p()
    assert p.ctx.lib.cbv_pipeline_add_board(p.h_, C.byref(cfg), C.byref(hdl)) == -1 and not hdl
    p.reset_state()
    b1.reset_state()
    p.run(0, 2)
    assert [bytes(p.results(0, 2)), bytes(b1.results(0, 2))] == before
    # configure of a parent with boards, run / upload / frame downloads on a board handle
    with pytest.raises(RuntimeError, match=r"code -4\)"):
        p.configure(QUAD_A)
    assert p.ctx.lib.cbv_pipeline_run(b1.h_, 0, 1) == -4
    f = np.ascontiguousarray(frames[0])
    assert p.ctx.lib.cbv_pipeline_upload(b1.h_, 0, N.ptr(f), f.strides[0]) == -4
    with pytest.raises(RuntimeError, match=r"code -4\)"):
        b1.download(0, 0)
    # detach, run again: the remaining boards go on unchanged
    b2 = p.add_board(QUAD_B, rot180=True)
    p.reset_state()
    b1.reset_state()
    p.run(0, 2)
    assert [bytes(p.results(0, 2)), bytes(b1.results(0, 2))] == before
    b2.close()
    p.reset_state()
    b1.reset_state()
    p.run(2, 2)
    p.run(0, 2)
    single = BoardPipeline(W, H, 4)
    single.configure(QUAD_A + np.float32(1), profile=S.SHIPPED_PROFILE, chunk=2)
    for k in range(4):
        single.upload(k, frames[k])
    single.run(2, 2)
    single.run(0, 2)
    assert bytes(b1.results(0, 4)) == bytes(single.results(0, 4))
    p.close()
    assert b1.h_ is None  # freed with its parent
    b1.close()            # and closing it again is harmless
    single.close()
