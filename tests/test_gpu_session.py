"""The game session on the device (BoardPipeline.session_begin; include/cbv.h, cbv_pipeline_session_begin) against the
pipeline as it was, driven one frame per run from the host: set_check_squares for the frame, run(slot, 1), the Python
session logic (GameState + StableMoveTracker on a frame clock + smart_scan_squares), update_references(slot,
reset_noise=True) on a move.  The session must reproduce every result word, every NoiseHandler record, the moves with
their frames, the final FEN and stable_count, bit for bit, whatever the run lengths.

Scene: 640x480, the scripted game at 30 frames per ply, 8 plies (270 frames), cooldown 10 frames, no enhancement.  The
detector reads the "normal" scene's positions exactly, so the oracle accepts a move 20 frames into every ply.  The case
with enhancement runs the full chain with an empty colour profile, the one the "normal" scene is lit for (synth.SCENES):
the reference's shipped profile is calibrated for an under-exposed camera and on this scene makes the detector see pieces
on 16 empty squares, more than max_diff, so no move would ever be looked for."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chessboard_vision_amd import _native as N
from chessboard_vision_amd import chess_rules as chess
from chessboard_vision_amd import synth as S
from chessboard_vision_amd.game_state import GameState, StableMoveTracker, smart_scan_squares

pytestmark = pytest.mark.gpu

W, H, FPP, NFR, COOLDOWN = 640, 480, 30, 270, 10
CALIBRATED = (S.CALIB_GRID_X, S.CALIB_GRID_Y)


def _noise_bytes(b, s0, n):
    out = (N.NoiseResult * n)()
    b.ctx.check(b.ctx.lib.cbv_pipeline_noise_results(b.h_, s0, n, out))
    return out


def _make(n, rot180=False, grid=None, enhance=False, boards=0, fmt=None):
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, n)
    pts = S.scaled_corners(W, H)
    kw = dict(profile={}) if enhance else {}
    p.configure(pts, grid_lines=grid, rot180=rot180, enhance=enhance, chunk=16, lanes=2, **kw)
    for k in range(boards):
        p.add_board(pts + np.float32(2 * (k + 1)), rot180=rot180)
    # a camera that looks at the board from the other side sees it turned: rot180 turns it back
    src = pts[::-1].copy() if rot180 else pts
    if fmt:
        import ref64_yuv as Y
        q = BoardPipeline(W, H, n)
        q.synth(0, n, scene="normal", frames_per_ply=FPP, points=src)
        p.set_input_format(fmt)
        for i in range(n):
            p.upload(i, Y.from_bgr(q.download(0, i), fmt), fmt=fmt)
        q.close()
    else:
        p.synth(0, n, scene="normal", frames_per_ply=FPP, points=src)
    return p


class _HostSession:
    """GameSession.on_frame's back half with the host classes, one per board."""

    def __init__(self, board, rule, fen=None, stale=False):
        self.b, self.game, self.stale = board, GameState(), stale
        if fen:
            self.game.set_fen(fen)
        self.tracker = StableMoveTracker(self.game, rule=rule)
        self.clock = self.tracker.use_frame_clock(cooldown_frames=COOLDOWN)
        self.frame0 = None
        self.moves = []
        self.mask0 = smart_scan_squares(self.game)

    def before(self, slot):
        c = self.clock.frame + 1
        mask = self.mask0 if self.stale else smart_scan_squares(self.game)
        self.b.set_check_squares(slot, [None if c % 30 == 0 else mask])

    def after(self, slot):
        self.clock.tick()
        res = self.b.results(slot, 1)[0]
        noise = _noise_bytes(self.b, slot, 1)[0]
        mv = self.tracker.process(self.b.occupied(res), noise_active=noise.state == 1)
        if mv is not None:
            status = self.tracker.last_status if self.tracker.rule == "game_state" else "move_confirmed"
            self.moves.append((self.clock.frame - 1, mv.uci(), status))
            self.b.update_references(slot, reset_noise=True)


def _observe(p, n):
    return [(bytes(b.results(0, n)), bytes(_noise_bytes(b, 0, n))) for b in [p] + list(p._boards)]


def _oracle(p, n, rule, stale=False, begin=None):
    """`begin`: {board index: (first frame, fen)}; default every board from frame 0 and the start position"""
    boards = [p] + list(p._boards)
    begin = begin or {k: (0, None) for k in range(len(boards))}
    hosts = {}
    for t in range(n):
        for k, (t0, fen) in begin.items():
            if t == t0:
                hosts[k] = _HostSession(boards[k], rule, fen, stale)
        for h in hosts.values():
            h.before(t)
        p.run(t, 1)
        for h in hosts.values():
            h.after(t)
    return dict(obs=_observe(p, n), moves={k: h.moves for k, h in hosts.items()}, fen={k: h.game.get_fen() for k, h in hosts.items()},
                stable={k: h.tracker.stable_count for k, h in hosts.items()})


def _session(p, n, rule, split, begin=None):
    boards = [p] + list(p._boards)
    begin = begin or {k: (0, None) for k in range(len(boards))}
    cuts = sorted({t0 for t0, _ in begin.values()} - {0})
    ses, t, i = {}, 0, 0
    while t < n:
        for k, (t0, fen) in begin.items():
            if t == t0:
                ses[k] = boards[k].session_begin(rule=rule, fen=fen, cooldown_frames=COOLDOWN)
        c = min(split[i % len(split)], n - t, *[x - t for x in cuts if x > t])
        p.run(t, c)
        t, i = t + c, i + 1
    out = dict(obs=_observe(p, n), moves={k: [(f, m.uci(), s) for f, m, s in s_.moves()] for k, s_ in ses.items()},
               fen={k: s_.fen() for k, s_ in ses.items()}, stable={k: s_.stable_count for k, s_ in ses.items()})
    for k, s_ in ses.items():
        assert s_.board.fen() == out["fen"][k] and s_.state().c == n - begin[k][0]
        s_.end()
    return out


def _assert_same(got, want, what):
    assert got["moves"] == want["moves"], what
    assert got["fen"] == want["fen"] and got["stable"] == want["stable"], what
    for k, (g, w) in enumerate(zip(got["obs"], want["obs"])):
        if g != w:
            gr, wr = np.frombuffer(g[0], np.uint64).reshape(-1, 8), np.frombuffer(w[0], np.uint64).reshape(-1, 8)
            bad = np.nonzero((gr != wr).any(axis=1))[0]
            gn, wn = np.frombuffer(g[1], np.uint8).reshape(-1, 16), np.frombuffer(w[1], np.uint8).reshape(-1, 16)
            badn = np.nonzero((gn != wn).any(axis=1))[0]
            raise AssertionError("%s: board %d differs: result frames %s, noise frames %s" % (what, k, bad[:8].tolist(), badn[:8].tolist()))


@functools.lru_cache(maxsize=None)
def _reference(rule, rot180, calibrated):
    p = _make(NFR, rot180, CALIBRATED if calibrated else None)
    want = _oracle(p, NFR, rule)
    p.close()
    return want


CASES = [("session", False, False, ((1,), (7,), (64,), (NFR,), (5, 1, 33, 2, 90))), ("game_state", False, True, ((64,), (NFR,))),
         ("session", True, True, ((NFR,),)), ("game_state", True, False, ((7,), (64,)))]


@pytest.mark.parametrize("rule,rot180,calibrated,splits", CASES)
def test_session_equals_one_frame_runs_driven_from_the_host(gpu_ctx, rule, rot180, calibrated, splits):
    want = _reference(rule, rot180, calibrated)
    # the oracle must exercise the feature: moves, two of them inside one run (the resume path twice), and check sets that
    # matter behind a move
    moves = want["moves"][0]
    assert len(moves) >= 4, moves
    if not rot180 and not calibrated:
        p = _make(NFR)
        stale = _oracle(p, NFR, rule, stale=True)
        p.close()
        a = np.frombuffer(want["obs"][0][0], np.uint64).reshape(-1, 8)[:, 3]
        b = np.frombuffer(stale["obs"][0][0], np.uint64).reshape(-1, 8)[:, 3]
        first = moves[0][0]
        assert (a[first + 1:] != b[first + 1:]).any(), "stale check sets give the same `processed` words: the scene does not test the feedback"
    p = _make(NFR, rot180, CALIBRATED if calibrated else None)
    for split in splits:
        if split == (NFR,):
            assert len([m for m in moves if m[0] < NFR]) >= 2  # one run holds at least two accepted moves
        p.reset_state()
        got = _session(p, NFR, rule, split)
        _assert_same(got, want, "split %s" % (split,))
    p.close()


def test_two_boards_with_sessions_at_different_plies(gpu_ctx):
    n = 150
    g = GameState()
    for ply in range(2):
        g.board.push(chess.Move.from_uci("".join(S.SCRIPT[ply][0])))
    begin = {0: (0, None), 1: (2 * FPP, g.get_fen())}
    p = _make(n, boards=1)
    want = _oracle(p, n, "game_state", begin=begin)
    p.close()
    assert len(want["moves"][0]) >= 4 and len(want["moves"][1]) >= 2 and want["fen"][0] == want["fen"][1]
    assert [m[0] for m in want["moves"][1]] != [m[0] for m in want["moves"][0][2:]]  # frames count from each session's begin
    p = _make(n, boards=1)
    got = _session(p, n, "game_state", (64,), begin=begin)
    p.close()
    _assert_same(got, want, "two boards")


@pytest.mark.parametrize("kw", [dict(enhance=True), dict(fmt="nv12")], ids=["enhanced", "nv12-raw"])
def test_session_with_enhancement_and_in_raw_mode(gpu_ctx, kw):
    n = 96
    p = _make(n, **kw)
    want = _oracle(p, n, "session")
    p.close()
    assert len(want["moves"][0]) >= 2, want["moves"]
    p = _make(n, **kw)
    got = _session(p, n, "session", (n,))
    p.close()
    _assert_same(got, want, str(kw))


FENS = [chess.STARTING_FEN,
        "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1",  # Kiwipete
        "rnbqkbnr/ppp1p1pp/8/3pPp2/8/8/PPPP1PPP/RNBQKBNR w KQkq f6 0 3",            # en passant
        "8/2p5/3p4/KP5r/1R3p1k/8/4P1P1/8 w - - 0 1",                               # pins, en passant under a pin
        "n1n5/PPPk4/8/8/8/8/4Kppp/5N1N b - - 0 1",                                 # promotions
        "r3k2r/Pppp1ppp/1b3nbN/nP6/BBP1P3/q4N2/Pp1P2PP/R2Q1RK1 w kq - 0 1",       # castling rights, check
        "r3k2r/8/8/8/8/8/8/R3K2R b Kq - 0 1"]


@pytest.mark.parametrize("fen", FENS)
def test_device_generator_equals_the_host_generator(gpu_ctx, fen):
    lib = gpu_ctx.lib
    b = chess.Board()
    b.set_fen(fen)
    want = (C.c_uint16 * 256)()
    nw = chess._L().cbv_board_legal_moves(b._h, want, 256)
    got, ng = (C.c_uint16 * 256)(), C.c_int()
    gpu_ctx.check(lib.cbv_session_device_legal_moves(gpu_ctx.h, fen.encode(), got, 256, C.byref(ng)))
    assert ng.value == nw > 0 and list(got[:nw]) == list(want[:nw])


# launches per kernel of a 12-frame run, chunk = 4, one lane, as tests/test_gpu_session_chain.py records them for the
# commit this feature was added on
PARENT_COUNTS = {"COLOR_LAB_HIST": 3, "CLAHE_LUT": 3, "CLAHE_APPLY": 3, "BILATERAL": 3, "SHARPEN": 3, "NORM_LUT": 3, "WARP": 3,
                 "SQUARES": 3, "SCAN": 1, "HOUGH": 3}
ENHANCEMENT = ("COLOR_LAB_HIST", "CLAHE_LUT", "CLAHE_APPLY", "BILATERAL", "SHARPEN", "NORM_LUT")


def _counted(ctx, p, n):
    p.run(0, n)
    p.results(0, n)
    ctx.profile_reset()
    ctx.profile_enable(-1)
    try:
        p.run(0, n)
        p.results(0, n)
        return {k: ctx.profile_read(kid)[1] for k, kid in N.K_ALL.items() if ctx.profile_read(kid)[1]}
    finally:
        ctx.profile_enable(-2)
        ctx.profile_reset()


def test_off_means_off_and_errors(gpu_ctx):
    from chessboard_vision_amd.stream import BoardPipeline
    n = 12
    pts = S.scaled_corners(W, H)
    p = BoardPipeline(W, H, n)
    with pytest.raises(RuntimeError, match="not configured"):
        p.session_begin()
    p.configure(pts, profile=S.SHIPPED_PROFILE, chunk=4, lanes=1)
    p.synth(0, n, scene="normal", frames_per_ply=2)
    assert _counted(gpu_ctx, p, n) == PARENT_COUNTS
    p.configure(pts, enhance=False, chunk=4, lanes=1)
    off = _counted(gpu_ctx, p, n)
    assert off == {k: v for k, v in PARENT_COUNTS.items() if k not in ENHANCEMENT}
    with pytest.raises(RuntimeError, match="not a FEN"):
        p.session_begin(fen="8/8 w")
    with pytest.raises(RuntimeError, match="bad configuration"):
        p.session_begin(stability_required=0)
    with pytest.raises(RuntimeError, match="bad configuration"):  # frame counts near INT_MAX would wrap the round count
        p.session_begin(stability_required=2 ** 31 - 1)
    with pytest.raises(RuntimeError, match="bad configuration"):
        p.session_begin(cooldown_frames=2 ** 31 - 1)
    s = p.session_begin(cooldown_frames=COOLDOWN)
    with pytest.raises(RuntimeError, match="game session with smart_scan"):
        p.set_check_squares(0, [set()])
    on = _counted(gpu_ctx, p, n)  # 1 + ceil(12 / 20) rounds of the scan stage, nothing else changes
    assert on == dict(off, SCAN=2), on
    p.update_references(0)  # stays legal during a session
    s.end()
    p.set_check_squares(0, [set()])
    assert _counted(gpu_ctx, p, n) == off  # ... and the session is gone without a trace in the launches
    s = p.session_begin(smart_scan=False)
    p.set_check_squares(0, [set()])  # the check sets stay the caller's
    s.end()
    p.close()


@functools.lru_cache(maxsize=None)
def _short_runs(boards, session_on):
    """12 frames at 5 frames per ply in runs of 1, 3 and 8 frames (at most 4: the fused pack + NoiseHandler launch; more:
    the separate ones) -> board 0's results, noise records and square statistics, and the moves of the session on board
    `session_on` (None: no session)."""
    from chessboard_vision_amd.stream import BoardPipeline
    n = 12
    pts = S.scaled_corners(W, H)
    p = BoardPipeline(W, H, n)
    p.configure(pts, enhance=False, chunk=16, lanes=2)
    for k in range(boards):
        p.add_board(pts + np.float32(2 * (k + 1)))
    p.synth(0, n, scene="normal", frames_per_ply=5, points=pts)
    all_boards = [p] + list(p._boards)
    ses = all_boards[session_on].session_begin(stability_required=2, cooldown_frames=1) if session_on is not None else None
    t = 0
    for c in (1, 3, 8):
        p.run(t, c)
        t += c
    out = dict(results=bytes(p.results(0, n)), noise=bytes(_noise_bytes(p, 0, n)), stats=[bytes(p.square_stats(s)) for s in range(n)],
               moves=[m.uci() for _, m, _ in ses.moves()] if ses else [])
    p.close()
    return out


def test_board_without_session_beside_one_with_a_session_in_short_runs(gpu_ctx):
    """A board without a session in a pipeline where another board runs one is scanned by itself, behind the table-driven
    HoughCircles passes of both boards: in runs of 1, 3 and 8 frames it gives what the same board gives in a pipeline
    of its own."""
    got, want = _short_runs(1, 1), _short_runs(0, None)
    assert got["moves"], "the session accepted no move: the case tests nothing"
    assert got["results"] == want["results"] and any(want["results"])
    assert got["noise"] == want["noise"]
    assert got["stats"] == want["stats"]
