"""The scripted game through the device session with rule="session" (GameSession._infer_move), without and with piece
tones.  Without them the session stops for good at ply 7: the bishop's retreat b5a4 could also have been a capture on a6
or c6, which vision still sees occupied, so _infer_move has three candidates.  With tones the destination squares of the
two captures still look black, the side not to move, and the retreat is the one candidate left; the game goes on until
castling (ply 9), whose four candidates all end on squares of the mover's colour and stay ambiguous, as in the reference.

    python examples/session_tones.py            # needs the built library and a gfx950 GPU
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chessboard_vision_amd import synth as S  # noqa: E402
from chessboard_vision_amd.stream import BoardPipeline  # noqa: E402

W, H, FRAMES_PER_PLY, PLIES = 1280, 720, 30, 10
N = FRAMES_PER_PLY * PLIES


def play(tones):
    pipe = BoardPipeline(W, H, N)
    pipe.configure(S.scaled_corners(W, H), grid_lines=(S.CALIB_GRID_X, S.CALIB_GRID_Y), enhance=False)
    pipe.synth(0, N, scene="normal", frames_per_ply=FRAMES_PER_PLY)
    if tones:
        pipe.run(0, 1)                       # slot 0 shows the start position: calibrate on it, then check it
        report = pipe.calibrate_tones(0)
        pipe.reset_state()
        print("  calibration: D = %.0f (light squares), %.0f (dark); misclassified %s, undecided %s"
              % (report["D"][0], report["D"][1], report["misclassified"], report["undecided"]))
    ses = pipe.session_begin(rule="session", cooldown_frames=10, tones=tones)
    pipe.run(0, N)
    if tones:
        print("  start position confirmed by vision:", pipe.verify_position(0)["ok"])
    moves = ses.moves()
    st = ses.state()
    print("  %d moves: %s" % (len(moves), " ".join(m.uci() for _, m, _ in moves)))
    print("  last rule call saw %d candidates; FEN %s" % (st.last_candidates, ses.fen()))
    ses.end()
    pipe.close()
    return [m.uci() for _, m, _ in moves]


print("rule='session' without tones")
plain = play(False)
print("rule='session' with tones")
toned = play(True)
assert plain == toned[:len(plain)] and len(plain) == 6 and len(toned) == 8 and toned[6] == "b5a4"
