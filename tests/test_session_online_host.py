"""The online game session on host buffers (cbv_session_walk_events, include/cbv.h): board events between frames, the
turn gate and the radar, on the same core the device kernels run (csrc/session_core.h), against a plain Python
restatement of LichessSession (on_move_detected, _sync_moves, LichessClient.is_my_turn) + GameSession._process_stable_move
+ _update_radar_ui over the host classes GameState, StableMoveTracker and chess_rules.  No GPU."""
import ctypes as C

import pytest

from chessboard_vision_amd import _native as N
from chessboard_vision_amd import chess_rules as chess
from chessboard_vision_amd.game_state import GameState, StableMoveTracker
from chessboard_vision_amd.noise_handler import NoiseHandler, NoiseState


def roi_bits(squares):
    b = 0
    for f, r in squares:
        b |= 1 << ((7 - r) * 8 + f)
    return b


def squares_of(bits):
    return {(i & 7, 7 - (i >> 3)) for i in range(64) if (bits >> i) & 1}


def occ_after(moves_str, fen=None):
    """ROI-numbered occupancy of the position after the UCI moves."""
    g = GameState()
    if fen:
        g.set_fen(fen)
    for u in moves_str.split():
        g.board.push_uci(u)
    return roi_bits(g.get_board_occupancy())


def is_my_turn(player, moves_str):
    """LichessClient.is_my_turn (lichess_client.py:193-204)"""
    count = len(moves_str.split()) if moves_str else 0
    return count % 2 == 0 if player == "white" else count % 2 == 1


class OnlineLogic:
    """LichessSession's side of a frame on the host classes: `event` is _sync_moves under the lock, `frame` is
    _update_radar_ui followed by _process_stable_move with LichessSession.on_move_detected as the hook (make_move taken as
    sent).  The native `rejected` memo is invisible except in n_ignored (rule calls turned down, not frames), so a refusal
    is listed once per memo: the memo holds the last occupancy the rule turned down or found no move for, and an event or
    a push clears it."""

    def __init__(self, player, stability, cooldown, fen=None, after_move=None):
        self.player, self.game = player, GameState()
        if fen:
            self.game.set_fen(fen)
            self.waiting = (self.game.get_turn_name() == "white") != (player == "white")
        else:
            self.waiting = not is_my_turn(player, "")
        self.memo, self.t, self.occ, self.ignored, self.moves = None, 0, None, [], []
        self.tracker = StableMoveTracker(self.game, on_move_detected=self.on_move_detected, after_move=after_move, rule="session")
        self.tracker.STABILITY_REQUIRED = stability
        self.clock = self.tracker.use_frame_clock(cooldown_frames=cooldown)
        infer = self.tracker.infer_move

        def watched(vision):
            move, n = infer(vision)
            if move is None and self.occ != self.game.get_board_occupancy():
                self.memo = self.occ
            return move, n

        self.tracker.infer_move = watched

    def on_move_detected(self, move):
        if self.waiting:
            if self.memo != self.occ:
                self.ignored.append((self.t, move.uci()))
                self.memo = self.occ
            return False
        self.waiting = True
        return True

    def event(self, moves_str):
        self.game.sync_moves(moves_str)
        self.waiting = not is_my_turn(self.player, moves_str)
        self.memo = None

    def frame(self, occupied, noise_active):
        """One frame from its occupied squares {(file, rank)}: (radar record, accepted move or None)."""
        self.t, self.occ = self.clock.tick() - 1, set(occupied)
        lifted, dests = self.game.radar(occupied)
        mv = self.tracker.process(occupied, noise_active=noise_active)
        if mv is not None:
            self.moves.append((self.t, mv.uci()))
            self.memo = None
        return (lifted, sorted(set(dests))), mv  # the record is the union: the reference lists a promotion square four times


def python_online(frames, events, player, stability, cooldown, fen=None):
    """frames: [(stable_occupied, visual_changes)], events: [(at_frame, moves_str)] applied between two frames as the
    stream thread does under the lock.  Returns everything the native state must agree with."""
    noise = NoiseHandler()
    s = OnlineLogic(player, stability, cooldown, fen, after_move=noise.reset)
    radar = []
    for t, (occ, changes) in enumerate(frames):
        for at, moves_str in events:
            if at == t:
                s.event(moves_str)
        state, _ = noise.process(squares_of(changes))
        radar.append(s.frame(squares_of(occ), state == NoiseState.NOISE_ACTIVE)[0])
    return dict(moves=s.moves, fen=s.game.get_fen(), stable=s.tracker.stable_count, waiting=s.waiting, ignored=s.ignored, radar=radar)


def make_events(events, player, online=True):
    out = (N.SessionEvent * max(1, len(events)))()
    for k, (at, moves_str) in enumerate(events):
        out[k].at_frame = at
        assert N.load().cbv_session_pos_from_moves(moves_str.encode(), out[k].pos, None) == 0
        out[k].waiting_for_opponent = 0 if (not online or is_my_turn(player, moves_str)) else 1
    return out


def native_online(frames, events, player, stability, cooldown, fen=None, radar_on=True, rule="session", online=True):
    """cbv_session_walk_events called again behind every accepted move with the events that are still to come, and with
    the NoiseHandler records of a handler that is reset there (what the device's resume rounds do)."""
    lib = N.load()
    chess._L()
    cfg = N.SessionConfig(N.SESSION_RULES[rule], stability, cooldown, 30, 4, 1, N.SESSION_ONLINE[player] if online else 0, 1 if radar_on else 0)
    st = N.SessionState()
    assert lib.cbv_session_state_init_cfg(st, cfg, fen.encode() if fen else None) == 0
    n = len(frames)
    res = (N.FrameResult * n)()
    for t, (occ, changes) in enumerate(frames):
        res[t].stable_occupied, res[t].visual_changes = occ, changes
    ev = make_events(events, player, online)
    rad = (N.SessionRadar * n)()
    moves, t0, e0 = [], 0, 0
    while t0 < n:
        noise = NoiseHandler()
        rec = (N.NoiseResult * (n - t0))()
        for k in range(n - t0):
            state, _ = noise.process(squares_of(frames[t0 + k][1]))
            rec[k].state = {NoiseState.IDLE: 0, NoiseState.NOISE_ACTIVE: 1, NoiseState.MOVE_PENDING: 2}[state]
        mv, acc, used_ev = N.SessionMove(), C.c_int(), C.c_int()
        sub = (N.FrameResult * (n - t0)).from_buffer(res, C.sizeof(N.FrameResult) * t0)
        rsub = (N.SessionRadar * (n - t0)).from_buffer(rad, C.sizeof(N.SessionRadar) * t0)
        esub = (N.SessionEvent * max(1, len(events) - e0)).from_buffer(ev, C.sizeof(N.SessionEvent) * e0) if e0 < len(events) else None
        used = lib.cbv_session_walk_events(cfg, st, sub, rec, n - t0, esub, len(events) - e0, C.byref(used_ev), rsub, mv, C.byref(acc))
        assert 0 < used <= n - t0, used
        if acc.value:
            assert mv.frame == t0 + used - 1 == st.c - 1
            moves.append((mv.frame, chess.Move._from_code(mv.move).uci()))
        t0, e0 = t0 + used, e0 + used_ev.value
    buf = C.create_string_buffer(128)
    lib.cbv_session_state_fen(st, buf, 128)
    radar = [(squares_of(1 << r.lifted).pop() if r.lifted >= 0 else None, sorted(squares_of(r.destinations))) for r in rad]
    return dict(moves=moves, fen=buf.value.decode(), stable=st.stable_count, waiting=bool(st.waiting_for_opponent), radar=radar, st=st)


def both(frames, events, player, stability, cooldown, fen=None):
    want = python_online(frames, events, player, stability, cooldown, fen)
    got = native_online(frames, events, player, stability, cooldown, fen)
    st = got.pop("st")
    ignored = want.pop("ignored")
    assert got == want
    assert st.n_ignored == len(ignored)
    if ignored:
        assert (st.ignored_frame, chess.Move._from_code(st.ignored_move).uci()) == ignored[-1]
    else:
        assert st.ignored_frame == -1 and st.ignored_move == chess.MOVE_NONE
    assert st.c == len(frames) and st.n_moves == len(got["moves"])
    return got, ignored, st


START, E4, E4E5, E4E5NF3 = occ_after(""), occ_after("e2e4"), occ_after("e2e4 e7e5"), occ_after("e2e4 e7e5 g1f3")


@pytest.mark.parametrize("stability,cooldown", [(2, 0), (3, 0), (2, 4), (3, 2)])
def test_a_opponent_event_before_the_pieces_are_moved(stability, cooldown):
    """White plays e2e4; black's reply arrives over the network while the board still shows the e4 position; then the
    pieces follow and vision equals expected: no move is found for black and nothing is ignored."""
    frames = [(START, 0)] * 3 + [(E4, 0)] * 8 + [(E4E5, 0)] * 6 + [(E4E5NF3, 0)] * 8
    events = [(3 + 5, "e2e4 e7e5")]
    got, ignored, st = both(frames, events, "white", stability, cooldown)
    assert [m[1] for m in got["moves"]] == ["e2e4", "g1f3"] and ignored == [] and got["waiting"]
    assert got["moves"][0][0] == 3 + stability - 1


@pytest.mark.parametrize("stability,cooldown", [(2, 0), (3, 0), (2, 4), (3, 2)])
def test_b_pieces_moved_before_the_event(stability, cooldown):
    """The opponent's piece is moved on the board before the network says so: the rule finds e7e5 while waiting, the gate
    turns it down once (the memo covers the identical frames behind it), stable_count keeps counting, and after the event
    the board matches and play goes on."""
    frames = [(START, 0)] * 2 + [(E4, 0)] * 6 + [(E4E5, 0)] * 9 + [(E4E5NF3, 0)] * 8
    events = [(2 + 6 + 7, "e2e4 e7e5")]
    got, ignored, st = both(frames, events, "white", stability, cooldown)
    assert [m[1] for m in got["moves"]] == ["e2e4", "g1f3"]
    assert [u for _, u in ignored] == ["e7e5"] and st.n_ignored == 1
    assert ignored[0][0] >= 8 + stability - 1
    # stopped just behind the refusal: no push, no refresh, and stable_count has not been reset
    k = ignored[0][0] + 1
    cut = native_online(frames[:k], [], "white", stability, cooldown)
    assert cut["st"].stable_count == k - 8 and cut["st"].n_moves == 1 and cut["st"].rejected_valid == 1 and cut["st"].rejected == E4E5
    assert cut["st"].expected == E4 and cut["waiting"]


def test_c_a_second_move_seen_while_waiting_is_ignored():
    # own move accepted, then the next moves on the board are seen before any event: turned down, the board stays.  The
    # second occupancy (white's knight has moved too) still reads as e7e5 on the board that waits: a new occupancy, so a
    # new rule call and a second refusal.
    frames = [(E4, 0)] * 4 + [(E4E5, 0)] * 5 + [(E4E5NF3, 0)] * 5
    got, ignored, st = both(frames, [], "white", 2, 0)
    assert got["moves"] == [(1, "e2e4")] and ignored == [(5, "e7e5"), (10, "e7e5")] and got["waiting"]
    # a second OWN move: the event's move list has three tokens of which one is not a move, so the board is two plies on
    # (white to move) while is_my_turn counts three: the session waits, and white's g1f3 is found and turned down
    frames = [(E4, 0)] * 4 + [(E4E5, 0)] * 4 + [(E4E5NF3, 0)] * 5
    got, ignored, st = both(frames, [(5, "e2e4 e7e5 e9e9")], "white", 2, 0)
    assert got["moves"] == [(1, "e2e4")] and [u for _, u in ignored] == ["g1f3"] and got["waiting"]
    assert got["fen"].split()[1] == "w"


def test_d_an_event_clears_a_standing_rejected_memo():
    # black's session: white's e2e4 (and black's own e7e5) stand on the board before the network reports e2e4.  The rule
    # finds e2e4, the gate turns it down and remembers the occupancy; the event changes the board under the same
    # occupancy, so the memo must go: e7e5 is found and accepted.
    frames = [(E4E5, 0)] * 12
    got, ignored, st = both(frames, [(6, "e2e4")], "black", 2, 0)
    assert ignored == [(1, "e2e4")] and got["moves"] == [(6, "e7e5")]
    # without the event the memo stands and nothing more happens
    got, ignored, st = both(frames, [], "black", 2, 0)
    assert ignored == [(1, "e2e4")] and got["moves"] == [] and st.rejected_valid == 1
    # a memo left by "no move found": white played e2e4 and, too early, g1f3; once black's reply has come in over the
    # network, the same occupancy is g1f3 (and black's pieces yet to be moved)
    early = occ_after("e2e4") ^ roi_bits({(6, 0), (5, 2)})
    frames = [(E4, 0)] * 3 + [(early, 0)] * 10
    got, ignored, st = both(frames, [(8, "e2e4 e7e5")], "white", 2, 0)
    assert ignored == [] and got["moves"] == [(1, "e2e4"), (8, "g1f3")]


RADAR_CASES = [
    # fen, squares taken off the expected occupancy, lifted, destinations
    (None, {(4, 1)}, (4, 1), {(4, 2), (4, 3)}),                                  # e2: e3, e4
    (None, {(6, 0)}, (6, 0), {(5, 2), (7, 2)}),                                  # g1: f3, h3
    (None, {(4, 6)}, None, set()),                                               # e7 is the opponent's
    (None, {(4, 1), (3, 1)}, None, set()),                                       # two squares lifted
    (None, set(), None, set()),
    ("r3k2r/8/8/8/8/8/8/R3K2R w KQkq - 0 1", {(4, 0)}, (4, 0), {(3, 0), (5, 0), (3, 1), (4, 1), (5, 1), (6, 0), (2, 0)}),  # castling
    ("8/P6k/8/8/8/8/8/K7 w - - 0 1", {(0, 6)}, (0, 6), {(0, 7)}),                # the four promotions share a8
    ("r3k2r/8/8/8/8/8/8/R3K2R b KQkq - 0 1", {(4, 7)}, (4, 7), {(3, 7), (5, 7), (3, 6), (4, 6), (5, 6), (6, 7), (2, 7)}),
    ("4k3/8/8/8/8/8/4r3/4K3 w - - 0 1", {(4, 0)}, (4, 0), {(4, 1), (3, 0), (5, 0)}),  # a king in check: only the legal squares
]


def test_e_radar():
    for fen, off, lifted, dests in RADAR_CASES:
        base = occ_after("", fen)
        occ = base & ~roi_bits(off)
        frames = [(base, 0), (occ, 0), (occ, 0), (base, 0)]
        got, _, _ = both(frames, [], "white", 3, 0, fen=fen)
        assert got["radar"][0] == (None, []) and got["radar"][3] == (None, [])
        assert got["radar"][1] == got["radar"][2] == (lifted, sorted(dests)), (fen, off)
    # the radar follows the board in force at the frame: before the event e7 is the opponent's, from the event's frame on e2 is
    occ = E4 & ~roi_bits({(4, 6)})
    got, _, _ = both([(START, 0)] * 2 + [(occ, 0)] * 4, [(4, "e2e4")], "black", 3, 0)
    assert [r[0] for r in got["radar"]] == [None, None, None, None, (4, 6), (4, 6)]
    assert got["radar"][5][1] == [(4, 4), (4, 5)]
    # radar off: the records stay empty, the rest is the same
    a = native_online([(START & ~roi_bits({(4, 1)}), 0)] * 3, [], "white", 3, 0, radar_on=False)
    assert a["radar"] == [(None, [])] * 3


def test_f_argument_errors():
    lib = N.load()
    ARG, UNSUPPORTED = -1, -5
    # the occupancy rule together with online
    cfg = N.SessionConfig(N.SESSION_RULES["game_state"], 2, 0, 30, 4, 1, 1, 0)
    st = N.SessionState()
    assert lib.cbv_session_state_init_cfg(st, cfg, None) == ARG
    assert lib.cbv_session_state_init(st, None) == 0
    res, mv, acc, used = (N.FrameResult * 4)(), N.SessionMove(), C.c_int(), C.c_int()
    for r in res:
        r.stable_occupied = START
    assert lib.cbv_session_walk_events(cfg, st, res, None, 4, None, 0, C.byref(used), None, mv, C.byref(acc)) == ARG
    for bad in (dict(online=3), dict(online=-1), dict(radar=2)):
        cfg = N.SessionConfig(0, 2, 0, 30, 4, 1, bad.get("online", 0), bad.get("radar", 0))
        assert lib.cbv_session_state_init_cfg(st, cfg, None) == ARG
    cfg = N.SessionConfig(0, 2, 0, 30, 4, 1, 1, 0)
    assert lib.cbv_session_state_init_cfg(st, cfg, None) == 0 and st.waiting_for_opponent == 0
    assert lib.cbv_session_walk_events(cfg, st, res, None, 2, None, 0, C.byref(used), None, mv, C.byref(acc)) == 2 and st.c == 2
    before = bytes(st)
    # at_frame in the past
    ev = make_events([(1, "e2e4")], "white")
    assert lib.cbv_session_walk_events(cfg, st, res, None, 2, ev, 1, C.byref(used), None, mv, C.byref(acc)) == ARG
    # out of order
    ev = make_events([(3, "e2e4"), (2, "e2e4 e7e5")], "white")
    assert lib.cbv_session_walk_events(cfg, st, res, None, 2, ev, 2, C.byref(used), None, mv, C.byref(acc)) == ARG
    # more than the queue holds
    ev = make_events([(2 + k, "e2e4") for k in range(N.SESSION_EVENTS + 1)], "white")
    assert lib.cbv_session_walk_events(cfg, st, res, None, 2, ev, N.SESSION_EVENTS + 1, C.byref(used), None, mv, C.byref(acc)) == UNSUPPORTED
    assert bytes(st) == before  # nothing has changed
    # ... and a full queue is fine; the events behind the frames consumed stay with the caller
    assert lib.cbv_session_walk_events(cfg, st, res, None, 2, ev, N.SESSION_EVENTS, C.byref(used), None, mv, C.byref(acc)) == 2
    assert used.value == 2 and st.c == 4
    # black's session waits from the start; a session from a FEN takes it from the side to move
    cfg = N.SessionConfig(0, 2, 0, 30, 4, 1, 2, 0)
    assert lib.cbv_session_state_init_cfg(st, cfg, None) == 0 and st.waiting_for_opponent == 1
    assert lib.cbv_session_state_init_cfg(st, cfg, b"rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq - 0 1") == 0 and st.waiting_for_opponent == 0


def test_pos_from_moves_replays_like_sync_moves():
    lib = N.load()
    for moves in ("", "e2e4", "e2e4 e7e5 g1f3 b8c6 f1b5 a7a6", "e2e4 zzzz e7e5 e2e4 0000 g1f3", "e2e4 e7e5 g1f3 b8c6 f1c4 f8c5 e1g1",
                  "e2e4 e7e5 g1f3 b8c6 f1c4 f8c5 e1h1 g8f6", "a2a4 b7b5 a4b5 a7a6 b5a6 c8b7 a6b7 b8c6 b7a8q", "a2a4 b7b5 a4b5 a7a6 b5a6 c8b7 a6b7 b8c6 b7a8"):
        g = GameState()
        g.sync_moves(moves.replace("e1h1", "e1g1"))  # (python-chess reads king-takes-rook as castling; the host class does not)
        pos, n = N.SessionPos(), C.c_int()
        assert lib.cbv_session_pos_from_moves(moves.encode(), pos, C.byref(n)) == 0
        st = N.SessionState()
        C.memmove(C.byref(st), C.byref(pos), C.sizeof(pos))
        buf = C.create_string_buffer(128)
        lib.cbv_session_state_fen(st, buf, 128)
        assert buf.value.decode() == g.get_fen(), moves
        assert n.value == len(g.board.move_stack)
    assert lib.cbv_session_pos_from_moves(None, None, None) == -1


def test_offline_sessions_are_what_they_were():
    """online = 0, radar = 0, no events: cbv_session_walk_events is cbv_session_walk, and the new state fields stay at rest."""
    from test_session_host import native_session, script_stream
    frames = script_stream(8)
    moves, fen, st = native_session(frames, "session")
    got = native_online(frames, [], "white", 20, 10, radar_on=False, online=False)
    assert got["moves"] == [(f, u) for f, u, _ in moves] and got["fen"] == fen
    new = ("waiting_for_opponent", "ignored_move", "ignored_frame", "n_ignored")
    for name, _ in N.SessionState._fields_:
        assert getattr(got["st"], name)[:] == getattr(st, name)[:] if name == "sq" else getattr(got["st"], name) == getattr(st, name), name
    assert [getattr(st, k) for k in new] == [0, chess.MOVE_NONE, -1, 0]
