"""The game session's walk on host buffers (cbv_session_walk, include/cbv.h): the same core the device kernel runs
(csrc/session_core.h, csrc/chess_core.h), against a Python loop over GameState + StableMoveTracker on a frame clock +
NoiseHandler, called again and again across the moves, for both rules.  No GPU."""
import ctypes as C

import pytest

from chessboard_vision_amd import _native as N
from chessboard_vision_amd import chess_rules as chess
from chessboard_vision_amd import synth as S
from chessboard_vision_amd.game_state import FrameClock, GameState, StableMoveTracker
from chessboard_vision_amd.noise_handler import NoiseHandler, NoiseState

HOLD, GAP, COOLDOWN = 30, 3, 10


def roi_bits(squares):
    """{(file, rank)} -> ROI-numbered bits (8 * row + col, row 0 = rank 8)."""
    b = 0
    for f, r in squares:
        b |= 1 << ((7 - r) * 8 + f)
    return b


def squares_of(bits):
    return {(i & 7, 7 - (i >> 3)) for i in range(64) if (bits >> i) & 1}


def script_stream(plies=16):
    """[(stable_occupied, visual_changes)] per frame: each position of synth.SCRIPT held HOLD frames, GAP frames of a hand
    between them (an occupancy far from any position and a 6-square visual_changes burst)."""
    frames = []
    burst = roi_bits({(f, 3) for f in range(6)})
    for p in range(plies + 1):
        occ = roi_bits(S.position_after(p).keys())
        if p:
            hand = occ ^ roi_bits({(f, r) for f in range(2, 6) for r in (3, 4)})  # eight squares differ
            frames += [(hand, burst)] * GAP
        frames += [(occ, 0)] * HOLD
    return frames


def python_session(frames, rule, fen=None, stability=20, cooldown=COOLDOWN, max_diff=4):
    """The reference's per-frame order (game_session.py:157-225) with the host classes."""
    game = GameState()
    if fen:
        game.set_fen(fen)
    noise = NoiseHandler()
    tracker = StableMoveTracker(game, after_move=noise.reset, rule=rule)
    tracker.STABILITY_REQUIRED = stability
    clock = tracker.use_frame_clock(cooldown_frames=cooldown)
    assert isinstance(clock, FrameClock)
    assert max_diff == 4  # the host class has the reference's literal
    moves = []
    for t, (occ, changes) in enumerate(frames):
        clock.tick()
        state, _ = noise.process(squares_of(changes))
        mv = tracker.process(squares_of(occ), noise_active=state == NoiseState.NOISE_ACTIVE)
        if mv is not None:
            moves.append((t, mv.uci(), tracker.last_status if rule == "game_state" else "move_confirmed"))
    return moves, game.get_fen(), tracker.stable_count


def native_session(frames, rule, fen=None, stability=20, cooldown=COOLDOWN, max_diff=4):
    """cbv_session_walk called again behind every accepted move, with NoiseHandler records of a handler that is reset
    there (what the device's resume rounds do)."""
    lib = N.load()
    chess._L()
    cfg = N.SessionConfig(N.SESSION_RULES[rule], stability, cooldown, 30, max_diff, 1)
    st = N.SessionState()
    assert lib.cbv_session_state_init(st, fen.encode() if fen else None) == 0
    n = len(frames)
    res = (N.FrameResult * n)()
    for t, (occ, changes) in enumerate(frames):
        res[t].stable_occupied, res[t].visual_changes = occ, changes
    moves, t0 = [], 0
    while t0 < n:
        noise = NoiseHandler()
        rec = (N.NoiseResult * (n - t0))()
        for k in range(n - t0):
            state, _ = noise.process(squares_of(frames[t0 + k][1]))
            rec[k].state = {NoiseState.IDLE: 0, NoiseState.NOISE_ACTIVE: 1, NoiseState.MOVE_PENDING: 2}[state]
        mv, acc = N.SessionMove(), C.c_int()
        sub = (N.FrameResult * (n - t0)).from_buffer(res, C.sizeof(N.FrameResult) * t0)
        used = lib.cbv_session_walk(cfg, st, sub, rec, n - t0, mv, C.byref(acc))
        assert 0 < used <= n - t0
        if acc.value:
            assert mv.frame == t0 + used - 1 == st.c - 1
            moves.append((mv.frame, chess.Move._from_code(mv.move).uci(), lib.cbv_game_status_name(mv.status).decode()))
        t0 += used
    buf = C.create_string_buffer(128)
    lib.cbv_session_state_fen(st, buf, 128)
    return moves, buf.value.decode(), st


@pytest.mark.parametrize("rule", ["session", "game_state"])
def test_walk_matches_the_host_classes_over_the_script(rule):
    frames = script_stream()
    want_moves, want_fen, want_stable = python_session(frames, rule)
    moves, fen, st = native_session(frames, rule)
    assert moves == want_moves
    assert fen == want_fen
    assert st.stable_count == want_stable
    assert st.c == len(frames) and st.n_moves == len(moves)


def test_infer_move_rule_stops_at_the_ambiguous_bishop_retreat():
    """GameSession._infer_move recognises plies 1-6 of the script; at ply 7 (b5a4) the bishop could also have captured
    on a6 or c6, which vision sees occupied: three candidates, no move, and the board stays behind."""
    moves, fen, st = native_session(script_stream(), "session")
    script = ["".join(S.SCRIPT[p][0]) for p in range(6)]
    assert [m[1] for m in moves[:6]] == script and len(moves) == 6
    # a stream that ends in the ply-7 position: the walk's last rule call is the ambiguous one, and it records the count
    moves7, fen7, st7 = native_session(script_stream(7), "session")
    assert moves7 == moves and fen7 == fen
    assert st7.last_candidates == 3 and st7.rejected_valid == 1 and st7.rejected == roi_bits(S.position_after(7).keys())
    # ... the same count as the rules give when asked directly
    b = chess.Board()
    for u in script:
        b.push(chess.Move.from_uci(u))
    code = C.c_uint16()
    vision = chess._L().cbv_roi_bits_to_squares(roi_bits(S.position_after(7).keys()))
    assert chess._L().cbv_game_infer_move(b._h, vision, C.byref(code)) == 3
    assert fen == b.fen()


def test_process_occupancy_rule_plays_the_whole_script():
    moves, fen, st = native_session(script_stream(), "game_state")
    assert len(moves) == 16 and st.n_moves == 16
    assert [m[1] for m in moves] == ["".join(S.SCRIPT[p][0]) for p in range(16)]
    assert moves[8][2] == "castling_confirmed"
    # each move is accepted on the 20th frame of its position: stability counts from the first frame behind the hand
    assert [m[0] for m in moves] == [HOLD + (HOLD + GAP) * p + GAP + 19 for p in range(16)]


MID_FEN = "r1bqkbnr/1ppp1ppp/p1n5/1B2p3/4P3/5N2/PPPP1PPP/RNBQK2R w KQkq - 0 4"  # the script after six plies


@pytest.mark.parametrize("rule", ["session", "game_state"])
def test_begin_from_a_mid_game_fen(rule):
    occ0 = roi_bits(S.position_after(6).keys())
    if rule == "game_state":  # e1g1: castling, two squares each way
        uci, occ1 = "e1g1", roi_bits(S.position_after(6).keys() - {(4, 0), (7, 0)} | {(6, 0), (5, 0)})
    else:  # (_infer_move sees four candidates in a castling: e1g1, e1f1, h1g1, h1f1)
        uci, occ1 = "d2d3", roi_bits(S.position_after(6).keys() - {(3, 1)} | {(3, 2)})
    frames = [(occ0, 0)] * 3 + [(occ1, 0)] * 4
    want = python_session(frames, rule, fen=MID_FEN, stability=3, cooldown=0)
    moves, fen, st = native_session(frames, rule, fen=MID_FEN, stability=3, cooldown=0)
    assert (moves, fen, st.stable_count) == want
    assert [m[1] for m in moves] == [uci] and moves[0][0] == 5
    assert N.load().cbv_session_state_init(N.SessionState(), b"not a fen") != 0


def test_max_diff_cooldown_and_noise_gating():
    start = roi_bits(S.position_after(0).keys())
    e4 = roi_bits(S.position_after(1).keys())
    e5 = roi_bits(S.position_after(2).keys())
    # max_diff: an occupancy five squares away never becomes stable
    far = start ^ roi_bits({(0, 3), (1, 3), (2, 3), (3, 3), (4, 3)})
    moves, _, st = native_session([(far, 0)] * 6, "session", stability=2, cooldown=0)
    assert moves == [] and st.stable_count == 0 and st.stable_occupancy == 0
    # ... and with max_diff = 5 it does (and is rejected: no legal move explains it)
    moves, _, st = native_session([(far, 0)] * 6, "session", stability=2, cooldown=0, max_diff=5)
    assert moves == [] and st.stable_count == 6 and st.rejected_valid == 1 and st.rejected == far
    # cooldown: the second move waits until more than `cooldown` frames have passed since the first
    frames = [(e4, 0)] * 2 + [(e5, 0)] * 8
    for cooldown, second in ((0, 3), (4, 6)):
        want = python_session(frames, "session", stability=2, cooldown=cooldown)
        moves, fen, st = native_session(frames, "session", stability=2, cooldown=cooldown)
        assert (moves, fen, st.stable_count) == want
        assert [(m[0], m[1]) for m in moves] == [(1, "e2e4"), (second, "e7e5")]
    # noise: while NoiseHandler reports NOISE_ACTIVE (a 4-square burst, then its 5-frame cool-down) no move is looked for
    burst = roi_bits({(0, 3), (1, 3), (2, 3), (3, 3)})
    frames = [(e4, burst)] + [(e4, 0)] * 7
    want = python_session(frames, "game_state", stability=2, cooldown=0)
    moves, fen, st = native_session(frames, "game_state", stability=2, cooldown=0)
    assert (moves, fen, st.stable_count) == want
    assert [(m[0], m[1]) for m in moves] == [(5, "e2e4")]
