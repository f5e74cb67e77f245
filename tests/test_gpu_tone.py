"""Piece colour per square on the device (k_piece_tone; include/cbv.h "piece colour per square"): the tone sums against the
numpy restatement (tests/tone_ref.py), exactly; the pipeline's tone stage against the restatement on the warped boards it
downloads, bit for bit, and against the synthetic scene's true colours; the device session's tie-break against
cbv_session_walk_tones driven one frame per run; and a pipeline that never enabled tones launching nothing for them."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tone_ref as TR
from chessboard_vision_amd import _native as N
from chessboard_vision_amd import chess_rules as chess
from chessboard_vision_amd import synth as S
from chessboard_vision_amd._squares import _image_of
from chessboard_vision_amd.grid_extractor import GridExtractor, SmartGridExtractor

pytestmark = pytest.mark.gpu

W, H = 640, 480
CALIBRATED = (S.CALIB_GRID_X, S.CALIB_GRID_Y)
STATE = -4


def linear_rois():
    return [(x0, y0, w, h) for (_, _, x0, y0, w, h) in GridExtractor().roi_table(620, 620)]


def calibrated_rois():
    ge = SmartGridExtractor()
    ge.grid_lines_x, ge.grid_lines_y = list(S.CALIB_GRID_X), list(S.CALIB_GRID_Y)
    return [(x0, y0, w, h) for (_, _, x0, y0, w, h) in ge.roi_table(620, 620)]


def device_sums(ctx, board, rois):
    img = _image_of(board)
    assert img is not None
    r = (N.Roi * len(rois))()
    for i, (x0, y0, w, h) in enumerate(rois):
        r[i].x0, r[i].y0, r[i].w, r[i].h = x0, y0, w, h
    out = (N.ToneSums * len(rois))()
    ctx.check(ctx.lib.cbv_tone_sums_image(ctx.h, img, r, len(rois), out))
    return np.frombuffer(out, np.uint32).reshape(-1, 4).copy()


# ---- the kernel on one board ----

def test_sums_of_random_boards_are_exact(gpu_ctx):
    rng = np.random.default_rng(21)
    board = rng.integers(0, 256, (620, 620, 3), dtype=np.uint8)
    lin, cal = linear_rois(), calibrated_rois()
    assert {(w, h) for _, _, w, h in lin} == {(77, 77)} and {w for _, _, w, _ in cal} == {76, 77, 78, 79}
    for rois in (lin, cal, [lin[i] for i in (0, 7, 9, 27, 28, 36, 56, 62, 63)]):
        assert np.array_equal(device_sums(gpu_ctx, board, rois), TR.tone_sums(board, rois))
    # all-255 bytes: the largest sums a 77 x 77 square can have
    full = np.full((620, 620, 3), 255, np.uint8)
    assert np.array_equal(device_sums(gpu_ctx, full, lin), TR.tone_sums(full, lin))


def test_sums_of_small_odd_and_largest_squares(gpu_ctx):
    rng = np.random.default_rng(22)
    board = rng.integers(0, 256, (200, 260, 3), dtype=np.uint8)
    # 1 x 1 and 3 x 5: radius 0, the centre pixel; 4 x 4: radius 1; 128 x 128: the largest square, radius 32 (65 rows of 65)
    rois = [(0, 0, 1, 1), (259, 199, 1, 1), (5, 7, 3, 5), (20, 3, 5, 3), (30, 30, 4, 4), (40, 40, 2, 2), (60, 50, 128, 128), (132, 72, 128, 128),
            (1, 60, 9, 127)]
    want = TR.tone_sums(board, rois)
    assert want[0].tolist() == board[0, 0].tolist() + [1] and want[2].tolist() == board[7 + 2, 5 + 1].tolist() + [1]
    assert want[6][3] == int(TR.disc_mask(128, 128).sum()) > 3000
    assert np.array_equal(device_sums(gpu_ctx, board, rois), want)
    white = np.full((128, 128, 3), 255, np.uint8)
    assert np.array_equal(device_sums(gpu_ctx, white, [(0, 0, 128, 128)]), TR.tone_sums(white, [(0, 0, 128, 128)]))


def test_sums_of_a_strided_host_image(gpu_ctx):
    rng = np.random.default_rng(23)
    parent = rng.integers(0, 256, (640, 700, 3), dtype=np.uint8)
    view = parent[11:631, 37:657]
    assert view.strides[0] == 2100 and not view.flags.c_contiguous
    rois = calibrated_rois()
    assert np.array_equal(device_sums(gpu_ctx, view, rois), TR.tone_sums(view, rois))
    # ROIs outside the image, larger than the largest square, or a gray image are refused
    img = _image_of(view)
    r = (N.Roi * 1)()
    out = (N.ToneSums * 1)()
    for bad in ((600, 0, 21, 10), (0, 0, 129, 10), (-1, 0, 5, 5), (0, 0, 0, 5)):
        r[0].x0, r[0].y0, r[0].w, r[0].h = bad
        assert gpu_ctx.lib.cbv_tone_sums_image(gpu_ctx.h, img, r, 1, out) == -1
    r[0].x0, r[0].y0, r[0].w, r[0].h = 0, 0, 8, 8
    assert gpu_ctx.lib.cbv_tone_sums_image(gpu_ctx.h, _image_of(np.zeros((16, 16), np.uint8)), r, 1, out) == -1


def test_piece_tone_class_api(gpu_ctx):
    from chessboard_vision_amd.piece_tone import PieceTone
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, 2)
    p.configure(S.scaled_corners(W, H), grid_lines=CALIBRATED, enhance=False)
    p.synth(0, 2, scene="normal", frames_per_ply=1)
    p.run(0, 2)
    ge = SmartGridExtractor()
    ge.grid_lines_x, ge.grid_lines_y = list(S.CALIB_GRID_X), list(S.CALIB_GRID_Y)
    pt = PieceTone()
    rep = pt.calibrate(ge.split_board(p.download(2, 0)), None)
    assert rep["misclassified"] == [] and rep["undecided"] == [] and rep["samples"] == [[8, 8], [8, 8]]
    got = pt.classify(ge.split_board(p.download(2, 1)))
    pos = S.position_after(1)
    assert {k: got[k] for k in pos} == {k: ("w" if ch.isupper() else "b") for k, ch in pos.items()}
    # squares that are arrays of their own (no common image) give the same answer
    loose = {k: np.ascontiguousarray(v) for k, v in ge.split_board(p.download(2, 1)).items()}
    assert pt.classify(loose) == got
    p.close()


# ---- the pipeline's stage ----

NF, FPP = 34, 2


def _pipeline(scene, fmt=None, boards=False):
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, NF)
    pts = S.scaled_corners(W, H)
    p.configure(pts, grid_lines=CALIBRATED, enhance=False, chunk=16, lanes=2)
    if boards:  # a second board seen from the other side, turned back by rot180
        p.add_board(pts[::-1].copy(), grid_lines=CALIBRATED, rot180=True)
    if fmt:
        import ref64_yuv as Y
        q = BoardPipeline(W, H, NF)
        q.synth(0, NF, scene=scene, frames_per_ply=FPP)
        p.set_input_format(fmt)
        for i in range(NF):
            p.upload(i, Y.from_bgr(q.download(0, i), fmt), fmt=fmt)
        q.close()
    else:
        p.synth(0, NF, scene=scene, frames_per_ply=FPP)
    return p


def _check_board(b, rois):
    """calibrate on slot 0, run, and hold sums, model and records to the restatement on the downloaded boards"""
    rep = b.calibrate_tones(0)
    assert rep["misclassified"] == [] and rep["undecided"] == [] and rep["samples"] == [[8, 8], [8, 8]]
    warped0 = b.download(2, 0)
    centroid, want_rep = TR.calibrate(TR.tone_sums(warped0, rois), S.board_array(S.position_after(0)))
    m = b.tone_model
    assert [[[m.centroid[k][q][c] for c in range(3)] for q in range(2)] for k in range(2)] == centroid and m.margin == 0.125
    assert rep["D"] == want_rep["D"]
    return centroid


def _check_tones(b, rois, centroid):
    got = b.tones(0, NF)
    res = b.results(0, NF)
    for t in range(NF):
        sums = TR.tone_sums(b.download(2, t), rois)
        assert np.array_equal(np.frombuffer(b.tone_sums(t), np.uint32).reshape(64, 4), sums), t
        assert (got[t].white, got[t].black) == TR.classify(centroid, 0.125, sums), t
        pos = S.position_after(t // FPP)
        occ = sum(1 << ((7 - r) * 8 + f) for f, r in pos)
        assert (got[t].white & occ, got[t].black & occ) == TR.true_tones(pos), t       # every piece decided, none wrong
        colours = b.piece_colours(res[t], got[t])
        assert all(colours[k] == ("w" if pos[k].isupper() else "b") for k in colours if k in pos)
    return bytes(got)


@pytest.mark.parametrize("scene,fmt", [("normal", None), ("dim", None), ("normal", "nv12")])
def test_pipeline_tones_equal_the_restatement_and_the_scene(gpu_ctx, scene, fmt):
    p = _pipeline(scene, fmt)
    rois = calibrated_rois()
    with pytest.raises(RuntimeError):
        p.tones(0, 1)                                   # CBV_ERR_STATE while tones are off
    p.run(0, NF)
    centroid = _check_board(p, rois)
    p.run(0, NF)
    one = _check_tones(p, rois, centroid)
    # runs split as (0, 5) then (5, 29) give the same bytes (off and on again first: the records start from zero)
    model = p.tone_model
    p.set_tones(None)
    p.set_tones(model)
    assert bytes(p.tones(0, NF)) == bytes(16 * NF)
    p.run(0, 5)
    p.run(5, 29)
    assert bytes(p.tones(0, NF)) == one
    # off again: the records are refused, and an uncalibrated model is
    p.set_tones(None)
    with pytest.raises(RuntimeError):
        p.tones(0, 1)
    with pytest.raises(RuntimeError):
        p.set_tones(N.ToneModel())
    p.close()


def test_verify_position(gpu_ctx):
    """the position check the reference planned and never built: stable occupancy and tones of a slot against a FEN"""
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, 60)
    p.configure(S.scaled_corners(W, H), enhance=False, chunk=16, lanes=2)
    p.synth(0, 60, scene="normal", frames_per_ply=30)
    p.run(0, 1)
    p.calibrate_tones(0)
    p.reset_state()
    p.run(0, 60)
    assert p.verify_position(0) == {"ok": True, "missing": [], "extra": [], "wrong_colour": [], "undecided": []}
    v = p.verify_position(59)                              # one move on: e2e4
    assert not v["ok"] and v["missing"] == [(4, 1)] and v["extra"] == [(4, 3)] and not v["wrong_colour"] and not v["undecided"]
    assert p.verify_position(59, fen="rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq - 0 1")["ok"]
    swapped = p.verify_position(0, fen="RNBQKBNR/PPPPPPPP/8/8/8/8/pppppppp/rnbqkbnr w - - 0 1")
    assert len(swapped["wrong_colour"]) == 32 and not swapped["missing"] and not swapped["extra"] and not swapped["ok"]
    p.close()


def test_two_boards_one_with_tones(gpu_ctx):
    rois = calibrated_rois()
    plain = _pipeline("normal", boards=True)              # no tones anywhere: what the detectors give, and the model
    plain.run(0, NF)
    want0, want1 = bytes(plain.results(0, NF)), bytes(plain._boards[0].results(0, NF))
    centroid = _check_board(plain._boards[0], rois)
    model = plain._boards[0].tone_model
    plain.close()
    p = _pipeline("normal", boards=True)
    b1 = p._boards[0]                                     # the rot180 board gets the tones, board 0 none
    b1.set_tones(model)
    p.run(0, NF)
    _check_tones(b1, rois, centroid)
    with pytest.raises(RuntimeError):
        p.tones(0, 1)
    # neither board's detector results moved
    assert bytes(p.results(0, NF)) == want0 and bytes(b1.results(0, NF)) == want1
    p.close()


def test_tones_need_the_64_squares(gpu_ctx):
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, 2)
    p.configure(S.scaled_corners(W, H), enhance=False)
    cfg = p._cfg
    cfg.n_rois = 9
    p.ctx.check(p.ctx.lib.cbv_pipeline_configure(p.h_, cfg))
    m = N.ToneModel()
    m.calibrated = 1
    assert p.ctx.lib.cbv_pipeline_set_tones(p.h_, m) == STATE
    assert p.ctx.lib.cbv_pipeline_tone_sums(p.h_, 0, (N.ToneSums * 64)()) == STATE
    p.close()


# ---- off means off ----

def _launches(ctx, p):
    ctx.profile_reset()
    ctx.profile_enable(-1)
    try:
        p.run(0, NF)
        ctx.synchronize()
        p.results(0, NF)
        return {kid: ctx.profile_read(kid)[1] for kid in range(N.K_TONE + 1)}
    finally:
        ctx.profile_enable(-2)
        ctx.profile_reset()


def test_a_pipeline_without_tones_launches_nothing_new(gpu_ctx):
    p = _pipeline("normal")
    off = _launches(gpu_ctx, p)
    assert off[N.K_TONE] == 0 and off[N.K["SQUARES"]] == 3
    p.calibrate_tones(0)
    on = _launches(gpu_ctx, p)
    assert on[N.K_TONE] == 3                              # one bracket (two launches) per chunk of 16
    assert {k: v for k, v in on.items() if k != N.K_TONE} == {k: v for k, v in off.items() if k != N.K_TONE}
    p.set_tones(None)
    assert _launches(gpu_ctx, p) == off
    p.close()


# ---- the device session ----

FPP_S, NFR, COOLDOWN = 30, 270, 10


def _session_pipeline():
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, NFR)
    p.configure(S.scaled_corners(W, H), enhance=False, chunk=16, lanes=2)
    p.synth(0, NFR, scene="normal", frames_per_ply=FPP_S)
    return p


@functools.lru_cache(maxsize=None)
def _model_bytes():
    p = _session_pipeline()
    p.run(0, 1)
    rep = p.calibrate_tones(0)
    assert rep["misclassified"] == [] and rep["undecided"] == []
    out = bytes(p.tone_model)
    p.close()
    return out


def _model():
    return N.ToneModel.from_buffer_copy(_model_bytes())


def _noise_bytes(b, s0, n):
    out = (N.NoiseResult * n)()
    b.ctx.check(b.ctx.lib.cbv_pipeline_noise_results(b.h_, s0, n, out))
    return out


def _observe(p, ses):
    moves = [(f, m.uci(), s) for f, m, s in ses.moves()]
    return dict(moves=moves, fen=ses.fen(), stable=ses.stable_count, res=bytes(p.results(0, NFR)), noise=bytes(_noise_bytes(p, 0, NFR)),
                tones=bytes(p.tones(0, NFR)) if getattr(p, "tone_model", None) is not None else None)


@functools.lru_cache(maxsize=None)
def _oracle(rule):
    """one frame per run, the walk on the host: cbv_session_walk_tones"""
    lib = N.load()
    chess._L()
    p = _session_pipeline()
    p.set_tones(_model())
    cfg = N.SessionConfig(N.SESSION_RULES[rule], 20, COOLDOWN, 30, 4, 1, 0, 0, 1)
    st = N.SessionState()
    assert lib.cbv_session_state_init(st, None) == 0
    moves = []
    for t in range(NFR):
        c = st.c + 1
        mask = None if c % 30 == 0 else {(i & 7, 7 - (i >> 3)) for i in range(64) if (st.smart_mask >> i) & 1}
        p.set_check_squares(t, [mask])
        p.run(t, 1)
        mv, acc, used = N.SessionMove(), C.c_int(), C.c_int()
        assert lib.cbv_session_walk_tones(cfg, st, p.results(t, 1), _noise_bytes(p, t, 1), 1, None, 0, C.byref(used), None, p.tones(t, 1), mv,
                                          C.byref(acc)) == 1
        if acc.value:
            moves.append((mv.frame, chess.Move._from_code(mv.move).uci(), lib.cbv_game_status_name(mv.status).decode()))
            p.update_references(t, reset_noise=True)
    buf = C.create_string_buffer(128)
    lib.cbv_session_state_fen(st, buf, 128)
    out = dict(moves=moves, fen=buf.value.decode(), stable=st.stable_count, res=bytes(p.results(0, NFR)), noise=bytes(_noise_bytes(p, 0, NFR)),
               tones=bytes(p.tones(0, NFR)))
    p.close()
    return out


def _device(rule, split, tones):
    p = _session_pipeline()
    if tones:
        p.set_tones(_model())
    ses = p.session_begin(rule=rule, cooldown_frames=COOLDOWN, tones=tones)
    t, i = 0, 0
    while t < NFR:
        c = min(split[i % len(split)], NFR - t)
        p.run(t, c)
        t, i = t + c, i + 1
    out = _observe(p, ses)
    assert ses.state().c == NFR
    if tones:  # the stage cannot be switched off under the session that reads it
        assert p.ctx.lib.cbv_pipeline_set_tones(p.h_, None) == STATE
    ses.end()
    p.close()
    return out


@pytest.mark.parametrize("split", [(NFR,), (100, 170), (1,)], ids=["270", "100+170", "1x270"])
def test_session_with_tones_equals_the_host_walk(gpu_ctx, split):
    want = _oracle("session")
    got = _device("session", split, True)
    assert got["moves"] == want["moves"] and got["fen"] == want["fen"] and got["stable"] == want["stable"]
    assert got["res"] == want["res"] and got["noise"] == want["noise"] and got["tones"] == want["tones"]
    script = ["".join(S.SCRIPT[p][0]) for p in range(8)]
    assert [m[1] for m in got["moves"]] == script and "b5a4" in script


def test_session_without_tones_stops_at_the_bishop_retreat(gpu_ctx):
    got = _device("session", (NFR,), False)
    assert [m[1] for m in got["moves"]] == ["".join(S.SCRIPT[p][0]) for p in range(6)]
    # a session that asks for tones on a board whose tones are off is refused
    p = _session_pipeline()
    with pytest.raises(RuntimeError):
        p.session_begin(rule="session", cooldown_frames=COOLDOWN, tones=True)
    p.close()


def test_game_state_rule_is_unchanged_by_tones(gpu_ctx):
    a, b = _device("game_state", (NFR,), True), _device("game_state", (100, 170), False)
    for k in ("moves", "fen", "stable", "res", "noise"):
        assert a[k] == b[k], k
    assert len(a["moves"]) == 8
