"""The online game session on the device (session_begin(online=..., radar=True), Session.sync_moves; include/cbv.h,
cbv_pipeline_session_sync) against one-frame runs driven from the host: set_check_squares for the frame, run(slot, 1),
then LichessSession's logic on the host classes (tests/test_session_online_host.py, OnlineLogic) with the board events
applied between two runs, the turn gate in the host session and the radar on the host GameState.  The device session must
reproduce every result word, every NoiseHandler record, the moves with their frames, the final FEN, stable_count,
waiting_for_opponent, the ignored move and its count, and every radar record, bit for bit, whatever the run lengths and
wherever in a run the events fall.

Scene of tests/test_gpu_session.py: 640x480, no enhancement, the scripted game at 30 frames per ply, 6 plies (210 frames),
cooldown 10.  stability_required is 8, so that a ply is recognised about 10 frames behind its boundary and an opponent's
event 12 frames behind the boundary finds the move already turned down (case b); 5 frames before the boundary is case a."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chessboard_vision_amd import _native as N
from chessboard_vision_amd import synth as S
from chessboard_vision_amd.game_state import smart_scan_squares
from test_gpu_session import COOLDOWN, FPP, _assert_same, _make, _noise_bytes, _observe, _oracle, _session
from test_session_online_host import OnlineLogic

pytestmark = pytest.mark.gpu

PLIES, STABILITY = 6, 8
NFR = (PLIES + 1) * FPP
UCI = ["".join(S.SCRIPT[p][0]) for p in range(PLIES)]


def moves_str(plies):
    return " ".join(UCI[:plies])


class _HostOnline:
    """GameSession.on_frame's back half as LichessSession runs it, for one board, one frame per run."""

    def __init__(self, board, player, events):
        self.b, self.events = board, events
        self.s = OnlineLogic(player, STABILITY, COOLDOWN)
        self.radar = []

    def before(self, slot, t):
        for at, ms in self.events:
            if at == t:  # the stream thread got the lock between two frames
                self.s.event(ms)
        c = self.s.clock.frame + 1
        self.b.set_check_squares(slot, [None if c % 30 == 0 else smart_scan_squares(self.s.game)])

    def after(self, slot):
        res = self.b.results(slot, 1)[0]
        noise = _noise_bytes(self.b, slot, 1)[0]
        rec, mv = self.s.frame(self.b.occupied(res), noise.state == 1)
        self.radar.append(rec)
        if mv is not None:
            self.b.update_references(slot, reset_noise=True)


def _summary(obs, per_board):
    keys = ("moves", "fen", "stable", "waiting", "ignored", "radar")
    return dict(obs=obs, **{k: {b: v[k] for b, v in per_board.items()} for k in keys})


def _oracle_online(p, n, specs):
    """specs: {board index: (player, [(at_frame, moves_str)])}"""
    boards = [p] + list(p._boards)
    hosts = {k: _HostOnline(boards[k], *spec) for k, spec in specs.items()}
    for t in range(n):
        for h in hosts.values():
            h.before(t, t)
        p.run(t, 1)
        for h in hosts.values():
            h.after(t)
    return _summary(_observe(p, n), {k: dict(moves=h.s.moves, fen=h.s.game.get_fen(), stable=h.s.tracker.stable_count, waiting=h.s.waiting,
                                             ignored=(len(h.s.ignored), h.s.ignored[-1] if h.s.ignored else None), radar=h.radar)
                                     for k, h in hosts.items()})


def _device_online(p, n, split, specs, late=False):
    """Without `late` every event waits in the board's queue from the start.  With it the events of a run are delivered
    just before that run, in their order (the queue takes them in non-decreasing at_frame order only), and one whose
    frame is the run's first frame goes with at_frame=None."""
    boards = [p] + list(p._boards)
    ses = {k: boards[k].session_begin(rule="session", cooldown_frames=COOLDOWN, stability_required=STABILITY, online=player, radar=True)
           for k, (player, _) in specs.items()}
    if not late:
        for k, (_, events) in specs.items():
            for at, ms in events:
                ses[k].sync_moves(ms, at_frame=at)
    t, i = 0, 0
    while t < n:
        c = min(split[i % len(split)], n - t)
        if late:
            for k, (_, events) in specs.items():
                for at, ms in events:
                    if t <= at < t + c:
                        ses[k].sync_moves(ms, at_frame=None if at == t else at)
        p.run(t, c)
        t, i = t + c, i + 1
    per = {}
    for k, s_ in ses.items():
        cnt, last = s_.ignored
        per[k] = dict(moves=[(f, m.uci()) for f, m, _ in s_.moves()], fen=s_.fen(), stable=s_.stable_count, waiting=s_.waiting_for_opponent,
                      ignored=(cnt, (last[0], last[1].uci()) if last else None), radar=s_.radar(0, n))
        assert s_.state().c == n
    out = _summary(_observe(p, n), per)
    for s_ in ses.values():
        s_.end()
    return out


def _assert_online_same(got, want, what):
    for key in ("waiting", "ignored"):
        assert got[key] == want[key], (what, key)
    for k in want["radar"]:
        bad = [t for t, (g, w) in enumerate(zip(got["radar"][k], want["radar"][k])) if g != w]
        assert not bad and len(got["radar"][k]) == len(want["radar"][k]), "%s: board %d: radar frames %s differ, e.g. %s != %s" % (
            what, k, bad[:8], got["radar"][k][bad[0]], want["radar"][k][bad[0]])
    _assert_same(got, want, what)


def _white_events(t5):
    """Black's plies for white's session: e7e5 five frames before its pieces move (case a), b8c6 twelve frames behind
    (case b: the move has been seen and turned down), a resync of the same list on the very frame white's f1b5 is accepted
    (a board event on the frame of an accepted move), a7a6 twelve frames behind."""
    ev = [(2 * FPP - 5, moves_str(2)), (4 * FPP + 12, moves_str(4)), (6 * FPP + 12, moves_str(6))]
    if t5 is not None:
        ev.insert(2, (t5, moves_str(4)))
    return ev


@functools.lru_cache(maxsize=None)
def _white_reference(rot180):
    p = _make(NFR, rot180)
    first = _oracle_online(p, NFR, {0: ("white", _white_events(None))})
    p.close()
    t5 = [f for f, u in first["moves"][0] if u == UCI[4]]
    assert len(t5) == 1, first["moves"]
    events = _white_events(t5[0])
    p = _make(NFR, rot180)
    want = _oracle_online(p, NFR, {0: ("white", events)})
    p.close()
    return events, want


def _check_the_oracle_exercises_the_feature(want, events):
    assert [u for _, u in want["moves"][0]] == [UCI[0], UCI[2], UCI[4]], want["moves"]   # white's plies only
    assert want["ignored"][0][0] == 2 and want["ignored"][0][1][1] == UCI[5]               # b8c6 and a7a6 were turned down
    assert want["ignored"][0][1][0] < events[-1][0]
    assert want["waiting"][0] is False
    lifted = [r for r in want["radar"][0] if r[0] is not None]
    assert lifted and all(r[1] for r in lifted), "no frame of the scene shows a lifted piece: the radar is not exercised"


SPLITS = [(NFR,), (1, 7, 64), (2 * FPP - 5, 4 * FPP + 12 - (2 * FPP - 5) + 1, NFR)]  # the last: events on a run's first / last frame, in its middle


def test_white_session_with_black_over_the_network(gpu_ctx):
    events, want = _white_reference(False)
    _check_the_oracle_exercises_the_feature(want, events)
    firsts = [events[0][0]]
    lasts = [events[1][0]]
    assert SPLITS[2][0] == firsts[0] and SPLITS[2][0] + SPLITS[2][1] - 1 == lasts[0] and lasts[0] + 1 < events[2][0] < events[3][0] < NFR - 1
    p = _make(NFR)
    for split in SPLITS:
        for late in ((False, True) if split == SPLITS[2] else (False,)):
            p.reset_state()
            got = _device_online(p, NFR, split, {0: ("white", events)}, late=late)
            _assert_online_same(got, want, "split %s late %s" % (split, late))
    p.close()


def test_rot180(gpu_ctx):
    events, want = _white_reference(True)
    _check_the_oracle_exercises_the_feature(want, events)
    p = _make(NFR, True)
    got = _device_online(p, NFR, (64,), {0: ("white", events)})
    p.close()
    _assert_online_same(got, want, "rot180")


def test_an_attached_board_plays_black_with_its_own_events(gpu_ctx):
    n = 5 * FPP
    white = [(2 * FPP - 5, moves_str(2)), (4 * FPP + 12, moves_str(4))]
    black = [(FPP + 12, moves_str(1)), (3 * FPP - 5, moves_str(3))]  # e2e4 behind its pieces (turned down first), g1f3 ahead of them
    specs = {0: ("white", white), 1: ("black", black)}
    p = _make(n, boards=1)
    want = _oracle_online(p, n, specs)
    p.close()
    assert [u for _, u in want["moves"][0]] == [UCI[0], UCI[2]] and [u for _, u in want["moves"][1]] == [UCI[1], UCI[3]], want["moves"]
    assert want["ignored"][1][0] >= 1 and want["ignored"][1][1][1] == UCI[0] and want["ignored"][0][0] == 1
    p = _make(n, boards=1)
    got = _device_online(p, n, (64, 9), specs)
    p.close()
    _assert_online_same(got, want, "two boards")


def test_offline_session_is_what_it_was(gpu_ctx):
    """A guard, not the proof: a session begun without online, radar or events gives the observations of the host oracle
    of tests/test_gpu_session.py, byte for byte; the new state fields stay at rest and the new calls say why they fail."""
    n = 96
    p = _make(n)
    want = _oracle(p, n, "session")
    p.close()
    assert len(want["moves"][0]) >= 2
    p = _make(n)
    got = _session(p, n, "session", (7, 64))
    _assert_same(got, want, "offline")
    s = p.session_begin(cooldown_frames=COOLDOWN)
    st = s.state()
    assert (st.waiting_for_opponent, st.ignored_move, st.ignored_frame, st.n_ignored) == (0, 0xFFFF, -1, 0)
    with pytest.raises(RuntimeError, match="radar = 1"):
        s.radar(0, 1)
    s.end()
    with pytest.raises(RuntimeError, match="online needs"):
        p.session_begin(rule="game_state", online="white")
    with pytest.raises(ValueError):
        p.session_begin(online="green")
    s = p.session_begin(online="black", cooldown_frames=COOLDOWN)
    assert s.waiting_for_opponent and s.ignored == (0, None)
    p.run(0, 4)
    with pytest.raises(RuntimeError, match="next frame 4"):
        s.sync_moves("e2e4", at_frame=3)
    s.sync_moves("e2e4", at_frame=9)
    with pytest.raises(RuntimeError, match="last queued event"):
        s.sync_moves("e2e4 e7e5", at_frame=8)
    for k in range(N.SESSION_EVENTS - 1):
        s.sync_moves("e2e4", at_frame=9)
    with pytest.raises(RuntimeError, match="queue is full"):
        s.sync_moves("e2e4", at_frame=9)
    p.run(4, 8)
    assert not s.waiting_for_opponent and s.fen().split()[1] == "b" and s.state().c == 12
    s.end()
    p.close()
