"""Piece colour per square and the tie-break of the move rules, host side (include/cbv.h "piece colour per square",
include/cbv_chess.h "tie-break"): classification and calibration against the numpy restatement (tests/tone_ref.py), bit
for bit; the tie-break in GameState.process_occupancy_change, GameSession._infer_move and the session walk.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tone_ref as TR
from chessboard_vision_amd import _native as N
from chessboard_vision_amd import chess_rules as chess
from chessboard_vision_amd import synth as S
from chessboard_vision_amd.game_state import GameState, StableMoveTracker

ARG = -1


def roi_bits(squares):
    b = 0
    for f, r in squares:
        b |= 1 << ((7 - r) * 8 + f)
    return b


def sums_array(rows):
    out = (N.ToneSums * len(rows))()
    for i, r in enumerate(rows):
        out[i].sum[0], out[i].sum[1], out[i].sum[2], out[i].cnt = int(r[0]), int(r[1]), int(r[2]), int(r[3])
    return out


def model_of(centroid, margin):
    m = N.ToneModel()
    for k in range(2):
        for p in range(2):
            for c in range(3):
                m.centroid[k][p][c] = centroid[k][p][c]
    m.margin, m.calibrated = margin, 1
    return m


def native_classify(model, rows):
    w, b = C.c_uint64(), C.c_uint64()
    assert N.load().cbv_tone_classify_host(model, sums_array(rows), len(rows), C.byref(w), C.byref(b)) == 0
    return w.value, b.value


def random_sums(rng, n=64, cnt=1201):
    """plausible sums: a mean per channel anywhere in 0..255, not a whole number"""
    return np.concatenate([rng.integers(0, 255 * cnt + 1, (n, 3)), np.full((n, 1), cnt)], axis=1).astype(np.uint32)


# ---- classify and calibrate ----

def test_classify_equals_the_restatement_on_random_sums():
    rng = np.random.default_rng(11)
    for trial in range(40):
        centroid = rng.uniform(0, 255, (2, 2, 3)).tolist()
        margin = [0.125, 0.0, 0.3, 0.49][trial % 4]
        rows = random_sums(rng, cnt=int(rng.integers(1, 3000)))
        rows[int(rng.integers(64)), 3] = 0           # a square without pixels is undecided
        assert native_classify(model_of(centroid, margin), rows) == TR.classify(centroid, margin, rows), trial


def test_dead_zone_boundaries_belong_to_the_decided_side():
    # light squares: cW = (200, 200, 200), cB = (40, 40, 40): D = 76800, T = 19200 at margin 0.125; on the axis f = (v, v, v)
    # gives dB - dW = 960 v - 115200, so v = 140 sits exactly on white's boundary and v = 100 on black's; all values exact
    centroid = [[[200.0] * 3, [40.0] * 3], [[200.0] * 3, [40.0] * 3]]
    cnt = 1201
    rows = np.array([[v * cnt] * 3 + [cnt] for v in (140, 139, 101, 100, 120, 200, 40, 255, 0)], np.uint32)
    want = ["w", None, None, "b", None, "w", "b", "w", "b"]
    assert [TR.classify_one(centroid, 0.125, i, r) for i, r in enumerate(rows)] == want
    w, b = native_classify(model_of(centroid, 0.125), rows)
    assert [("w" if (w >> i) & 1 else "b" if (b >> i) & 1 else None) for i in range(len(rows))] == want
    # margin 0: no dead zone, the midpoint itself (v = 120) is white (dB - dW = 0 >= 0), and nothing is undecided
    assert native_classify(model_of(centroid, 0.0), rows) == TR.classify(centroid, 0.0, rows)
    w0, b0 = native_classify(model_of(centroid, 0.0), rows)
    assert (w0 >> 4) & 1 and (w0 | b0) == (1 << len(rows)) - 1
    # an uncalibrated model is refused
    m = model_of(centroid, 0.125)
    m.calibrated = 0
    assert N.load().cbv_tone_classify_host(m, sums_array(rows), len(rows), C.byref(C.c_uint64()), C.byref(C.c_uint64())) == ARG


def native_calibrate(rows, position, margin=0.125):
    model, rep = N.ToneModel(), N.ToneReport()
    pos = np.ascontiguousarray(position, np.uint8)
    rc = N.load().cbv_tone_calibrate_host(sums_array(rows), N.ptr(pos), margin, model, rep)
    return rc, model, rep


def test_calibrate_equals_the_restatement():
    rng = np.random.default_rng(12)
    for trial in range(20):
        position = S.board_array(S.position_after(trial % 17))
        rows = random_sums(rng, cnt=int(rng.integers(1, 3000)))
        margin = [0.125, 0.0, 0.4][trial % 3]
        rc, model, rep = native_calibrate(rows, position, margin)
        centroid, want = TR.calibrate(rows, position, margin)
        assert rc == 0 and model.calibrated == 1 and model.margin == margin
        assert [[[model.centroid[k][p][c] for c in range(3)] for p in range(2)] for k in range(2)] == centroid, trial
        assert [[rep.samples[k][p] for p in range(2)] for k in range(2)] == want["samples"]
        assert [rep.D[0], rep.D[1]] == want["D"]
        # random sums do not separate: the report says which calibration squares the model gets wrong, it does not hide them
        assert (rep.misclassified, rep.undecided) == (want["misclassified"], want["undecided"])
        assert rep.misclassified | rep.undecided


def test_calibrate_on_separable_sums_is_clean_and_refuses_degenerate_input():
    position = S.board_array(S.position_after(0))
    rng = np.random.default_rng(13)
    cnt = 1201
    rows = np.zeros((64, 4), np.uint32)
    for i in range(64):
        base = {0: 120, 1: 235, 2: 25}[int(position[i])] + (10 if TR.square_colour(i) else 0)
        rows[i] = [(base + int(rng.integers(-5, 6))) * cnt + int(rng.integers(cnt)) for _ in range(3)] + [cnt]
    rc, model, rep = native_calibrate(rows, position)
    assert rc == 0 and rep.misclassified == 0 and rep.undecided == 0
    w, b = native_classify(model, rows)
    occ = sum(1 << i for i in range(64) if position[i])
    assert (w & occ, b & occ) == TR.true_tones(S.position_after(0))
    # an empty class: no black piece on the board
    only_white = np.where(position == 2, 0, position)
    assert native_calibrate(rows, only_white)[0] == ARG and TR.calibrate(rows, only_white) is None
    # D == 0: white and black pieces with the same sums
    same = rows.copy()
    same[:, :3] = 100 * cnt
    assert native_calibrate(same, position)[0] == ARG and TR.calibrate(same, position) is None
    # margin outside [0, 0.5), a byte that is no colour
    assert native_calibrate(rows, position, 0.5)[0] == ARG and native_calibrate(rows, position, -0.1)[0] == ARG
    bad = position.copy()
    bad[0] = 3
    assert native_calibrate(rows, bad)[0] == ARG


# ---- the tie-break ----

TWO_VICTIMS = "4k3/8/8/2p1p3/3P4/8/8/4K3 w - - 0 1"


def test_ambiguous_capture_is_resolved_by_the_tones():
    def play(tones):
        g = GameState()
        g.set_fen(TWO_VICTIMS)
        vision = g.get_board_occupancy() - {(3, 3)}   # d4 vanished
        mv, status = g.process_occupancy_change(vision, tones)
        return (mv.uci() if mv else None), status, g.get_fen()
    c5, e5 = (2, 4), (4, 4)
    uci, status, fen = play(({c5}, {e5}))             # c5 looks white now: the pawn went there
    assert (uci, status) == ("d4c5", "capture_confirmed") and fen.startswith("4k3/8/8/2P1p3/8/8/8/4K3 b")
    assert play(({e5}, {c5}))[:2] == ("d4e5", "capture_confirmed")
    for tones in (None, (set(), set()), ({c5, e5}, set()), (set(), {c5, e5}), ({c5, e5}, {c5, e5})):
        assert play(tones) == (None, "ambiguous_capture", TWO_VICTIMS), tones
    # the same through StableMoveTracker on rule "game_state"
    g = GameState()
    g.set_fen(TWO_VICTIMS)
    tr = StableMoveTracker(g, rule="game_state")
    tr.STABILITY_REQUIRED = 2
    clock = tr.use_frame_clock(cooldown_frames=0)
    vision = g.get_board_occupancy() - {(3, 3)}
    got = []
    for _ in range(3):
        clock.tick()
        got.append(tr.process(vision, tones=({c5}, {e5})))
    assert [m.uci() if m else None for m in got][:2] == [None, "d4c5"] and tr.last_status == "capture_confirmed"


def _transitions():
    """(fen before, vision occupancy word in square numbering) of the scripted game's plies, plus random words."""
    lib = chess._L()
    b = chess.Board()
    out = []
    for p in range(16):
        out.append((b.fen(), lib.cbv_roi_bits_to_squares(roi_bits(S.position_after(p + 1).keys()))))
        b.push(chess.Move.from_uci("".join(S.SCRIPT[p][0])))
    rng = np.random.default_rng(14)
    fens = [f for f, _ in out] + [TWO_VICTIMS]
    for k in range(400):
        fen = fens[k % len(fens)]
        bb = chess.Board()
        bb.set_fen(fen)
        occ = bb.occupancy_bits()
        word = occ
        for _ in range(int(rng.integers(1, 4))):      # drop or add a few squares: mostly one-piece changes
            word ^= 1 << int(rng.integers(64))
        out.append((fen, word))
    out.append((TWO_VICTIMS, chess.Board().occupancy_bits()))
    return out


def test_tones_only_ever_break_ties():
    lib = chess._L()
    rng = np.random.default_rng(15)
    resolved = 0
    for fen, vision in _transitions():
        for trial in range(4):
            tw, tb = (int(rng.integers(0, 1 << 63)) << 1 | int(rng.integers(2)) for _ in range(2))
            if trial == 0:
                tw = tb = 0
            plain, toned = chess.Board(), chess.Board()
            plain.set_fen(fen), toned.set_fen(fen)
            c0, c1 = C.c_uint16(), C.c_uint16()
            n0 = lib.cbv_game_infer_move(plain._h, vision, C.byref(c0))
            n1 = lib.cbv_game_infer_move_tones(toned._h, vision, tw, tb, C.byref(c1))
            assert n0 == n1                             # the count is the one before the filter
            if n0 <= 1:
                assert c0.value == c1.value
            else:
                assert c0.value == chess.MOVE_NONE
                resolved += c1.value != chess.MOVE_NONE
            s0 = lib.cbv_game_process_occupancy(plain._h, vision, C.byref(c0))
            s1 = lib.cbv_game_process_occupancy_tones(toned._h, vision, tw, tb, C.byref(c1))
            if lib.cbv_game_status_name(s0) != b"ambiguous_capture":
                assert (s0, c0.value, plain.fen()) == (s1, c1.value, toned.fen())
            else:
                assert lib.cbv_game_status_name(s1) in (b"ambiguous_capture", b"capture_confirmed")
    assert resolved > 0   # (the random words did reach the tie-break)


# ---- the session walk ----

HOLD, GAP, COOLDOWN = 30, 3, 10


def script_frames(first, last, tones=True):
    """per frame (stable_occupied, visual_changes, tone white, tone black): positions first..last of the script held HOLD
    frames each, GAP frames of a hand between them; the tones are the true colours of the position"""
    frames = []
    burst = roi_bits({(f, 3) for f in range(6)})
    for p in range(first, last + 1):
        pos = S.position_after(p)
        occ = roi_bits(pos.keys())
        w, b = TR.true_tones(pos) if tones else (0, 0)
        if p > first:
            frames += [(occ ^ roi_bits({(f, r) for f in range(2, 6) for r in (3, 4)}), burst, 0, 0)] * GAP
        frames += [(occ, 0, w, b)] * HOLD
    return frames


def walk(frames, fen=None, tone=1, give_tones=True, entry="tones", rule="session"):
    """the walk called again behind every accepted move, the NoiseHandler restarted there as the device's rounds do"""
    from chessboard_vision_amd.noise_handler import NoiseHandler, NoiseState
    lib = N.load()
    cfg = N.SessionConfig(N.SESSION_RULES[rule], 20, COOLDOWN, 30, 4, 1, 0, 0, tone)
    st = N.SessionState()
    assert lib.cbv_session_state_init(st, fen.encode() if fen else None) == 0
    n = len(frames)
    res, ton = (N.FrameResult * n)(), (N.ToneResult * n)()
    for t, (occ, changes, w, b) in enumerate(frames):
        res[t].stable_occupied, res[t].visual_changes, ton[t].white, ton[t].black = occ, changes, w, b
    moves, records, t0 = [], b"", 0
    while t0 < n:
        noise = NoiseHandler()
        rec = (N.NoiseResult * (n - t0))()
        for k in range(n - t0):
            state, _ = noise.process({(i & 7, 7 - (i >> 3)) for i in range(64) if (frames[t0 + k][1] >> i) & 1})
            rec[k].state = {NoiseState.IDLE: 0, NoiseState.NOISE_ACTIVE: 1, NoiseState.MOVE_PENDING: 2}[state]
        mv, acc, used_ev = N.SessionMove(), C.c_int(), C.c_int()
        sub = (N.FrameResult * (n - t0)).from_buffer(res, C.sizeof(N.FrameResult) * t0)
        tsub = (N.ToneResult * (n - t0)).from_buffer(ton, C.sizeof(N.ToneResult) * t0) if give_tones else None
        if entry == "tones":
            used = lib.cbv_session_walk_tones(cfg, st, sub, rec, n - t0, None, 0, C.byref(used_ev), None, tsub, mv, C.byref(acc))
        else:
            used = lib.cbv_session_walk_events(cfg, st, sub, rec, n - t0, None, 0, C.byref(used_ev), None, mv, C.byref(acc))
        assert 0 < used <= n - t0
        if acc.value:
            moves.append((mv.frame, chess.Move._from_code(mv.move).uci(), mv.candidates))
            records += bytes(mv)
        t0 += used
    return moves, st, records


def test_walk_plies_1_to_9_accepts_eight_with_tones_and_six_without():
    frames = script_frames(0, 9)
    moves, st, _ = walk(frames)
    script = ["".join(S.SCRIPT[p][0]) for p in range(8)]
    assert [m[1] for m in moves] == script and moves[6][1] == "b5a4"
    assert moves[6][2] == 3 and [m[2] for m in moves[:6]] == [1] * 6   # `candidates` keeps the count before the filter
    # ply 9, castling: e1g1, e1f1, h1g1 and h1f1 all end on squares that look white, tones cannot choose
    assert st.n_moves == 8 and st.last_candidates == 4 and st.rejected_valid == 1
    assert st.rejected == roi_bits(S.position_after(9).keys())
    plain, st0, _ = walk(frames, tone=0)
    assert [m[1] for m in plain] == script[:6] and st0.last_candidates == 3
    assert [m[0] for m in moves[:6]] == [m[0] for m in plain]


def fen_after(plies):
    b = chess.Board()
    for p in range(plies):
        b.push(chess.Move.from_uci("".join(S.SCRIPT[p][0])))
    return b.fen()


def test_walk_plies_11_to_15_from_the_position_after_ply_10():
    fen = fen_after(10)
    frames = script_frames(10, 15)
    moves, st, _ = walk(frames, fen=fen)
    assert [m[1] for m in moves] == ["".join(S.SCRIPT[p][0]) for p in range(10, 15)]
    assert moves[2][1] == "a4b3" and moves[2][2] == 2   # Bb3 or Bxb5
    buf = C.create_string_buffer(128)
    N.load().cbv_session_state_fen(st, buf, 128)
    assert buf.value.decode() == fen_after(15)
    plain, _, _ = walk(frames, fen=fen, tone=0)
    assert [m[1] for m in plain] == ["f1e1", "b7b5"]


@pytest.mark.parametrize("rule", ["session", "game_state"])
def test_tone_off_is_the_plain_walk_byte_for_byte(rule):
    frames = script_frames(0, 9)
    want_moves, want_st, want_rec = walk(frames, tone=0, entry="events", rule=rule)
    for tone, give in ((0, True), (1, False), (0, False)):
        moves, st, rec = walk(frames, tone=tone, give_tones=give, rule=rule)
        assert moves == want_moves and bytes(st) == bytes(want_st) and rec == want_rec, (tone, give)
    # a tone flag that is neither 0 nor 1 is refused like every other bad field
    cfg = N.SessionConfig(0, 20, COOLDOWN, 30, 4, 1, 0, 0, 2)
    st = N.SessionState()
    N.load().cbv_session_state_init(st, None)
    res = (N.FrameResult * 1)()
    assert N.load().cbv_session_walk_tones(cfg, st, res, None, 1, None, 0, C.byref(C.c_int()), None, None, N.SessionMove(), C.byref(C.c_int())) == ARG


# ---- the synthetic scene, rendered and warped by the CPU oracle ----

@pytest.mark.parametrize("scene", ["normal", "dim"])
def test_scene_positions_classify_cleanly(scene):
    """The 17 positions of the scripted game at 640 x 480 on the calibrated grid: calibrate on position 0, classify all
    with the restatement; no occupied square undecided, none wrong (the scene's pieces have 0.42 of a square as radius,
    the disc a quarter)."""
    from chessboard_vision_amd.grid_extractor import SmartGridExtractor
    from helpers import oracle_frame
    from oracle import cbv_oracle as O
    w, h = 640, 480
    ge = SmartGridExtractor()
    ge.grid_lines_x, ge.grid_lines_y = list(S.CALIB_GRID_X), list(S.CALIB_GRID_Y)
    rois = [(x0, y0, rw, rh) for (_, _, x0, y0, rw, rh) in ge.roi_table(620, 620)]
    assert len(rois) == 64
    model = None
    for p in range(17):
        frame = oracle_frame(w, h, scene, frame_idx=p, frames_per_ply=1)
        warped, _, _ = O.warp_image(frame, S.scaled_corners(w, h))
        sums = TR.tone_sums(warped, rois)
        pos = S.position_after(p)
        if p == 0:
            model, rep = TR.calibrate(sums, S.board_array(pos))
            assert rep["misclassified"] == 0 and rep["undecided"] == 0 and min(rep["D"]) > 0
            rc, native, nrep = native_calibrate(sums, S.board_array(pos))
            assert rc == 0 and [[[native.centroid[k][q][c] for c in range(3)] for q in range(2)] for k in range(2)] == model
        white, black = TR.classify(model, 0.125, sums)
        occ = roi_bits(pos.keys())
        assert (white & occ, black & occ) == TR.true_tones(pos), (scene, p)
        assert native_classify(model_of(model, 0.125), sums) == (white, black)


# ---- kernel ids, settings file ----

def test_kernel_id_of_the_tone_kernel():
    lib = N.load()
    assert N.K_TONE == N.K_CHANGE_BLUR + 5 == 24   # CBV_K_COUNT + 5
    assert lib.cbv_kernel_name(N.K_TONE) == b"k_piece_tone"
    assert lib.cbv_kernel_name(N.K_TONE - 1) == b"" and lib.cbv_kernel_name(N.K_TONE + 1) == b""
    assert "TONE" not in N.K_EVERY and N.K_TONE not in N.K_EVERY.values()


def test_tone_model_round_trips_through_its_settings_file(tmp_path):
    from chessboard_vision_amd.stream import load_tones, save_tones
    rng = np.random.default_rng(16)
    m = model_of(rng.uniform(0, 255, (2, 2, 3)).tolist(), 0.2)
    save_tones(str(tmp_path / "tone_model.json"), m)
    back = load_tones(str(tmp_path / "tone_model.json"))
    assert bytes(back) == bytes(m)


def test_position_array_forms():
    from chessboard_vision_amd.piece_tone import position_array
    start = S.board_array(S.position_after(0))
    assert np.array_equal(position_array(None), start) and np.array_equal(position_array(S.position_after(0)), start)
    assert np.array_equal(position_array(fen_after(10)), S.board_array(S.position_after(10)))
    assert np.array_equal(position_array(start), start)
    with pytest.raises(ValueError):
        position_array(np.zeros(63, np.uint8))
