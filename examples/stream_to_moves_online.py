"""Online play with the game session on the device: the scripted game as white, black's plies delivered the way
LichessSession._sync_moves delivers them (the game's whole move list, between two frames), the turn gate in front of the
board and the radar per frame.  The network client is not here: `opponent` stands for the stream thread.

    python examples/stream_to_moves_online.py [--frames 224] [--run 64] [--delay 12]

`--delay`: frames between black's pieces moving on the board and the move list arriving; negative = the list comes first.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chessboard_vision_amd import synth as S  # noqa: E402
from chessboard_vision_amd.stream import BoardPipeline  # noqa: E402

FPP = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=224)
    ap.add_argument("--run", type=int, default=64)
    ap.add_argument("--delay", type=int, default=12)
    a = ap.parse_args()
    w, h = 1280, 720
    p = BoardPipeline(w, h, a.run)
    p.configure(S.scaled_corners(w, h), enhance=False)
    ses = p.session_begin(rule="session", fps=30, cooldown_frames=10, stability_required=8, online="white", radar=True)
    # what the stream thread would hand over: (session frame, the game's moves so far) for each of black's plies
    uci = ["".join(S.SCRIPT[k][0]) for k in range(len(S.SCRIPT))]
    opponent = [(ply * FPP + a.delay, " ".join(uci[:ply])) for ply in range(2, len(uci) + 1, 2)]
    for f0 in range(0, a.frames, a.run):
        c = min(a.run, a.frames - f0)
        while opponent and opponent[0][0] < f0 + c:  # events of this batch wait in the board's queue: no run is cut short
            at, moves = opponent.pop(0)
            ses.sync_moves(moves, at_frame=max(at, f0))
        p.synth(0, c, frame0=f0, scene="normal", frames_per_ply=FPP)  # stands for the camera's frames of this batch
        p.run(0, c)
        for frame, move, _ in ses.moves():
            print("frame %4d  sent %s" % (frame, move.uci()))
        last = None
        for k, (lifted, dests) in enumerate(ses.radar(0, c)):
            if lifted != last and lifted is not None:
                print("frame %4d  lifted %s -> %s" % (f0 + k, "abcdefgh"[lifted[0]] + str(lifted[1] + 1),
                                                      " ".join("abcdefgh"[f] + str(r + 1) for f, r in dests)))
            last = lifted
    n, ignored = ses.ignored
    print("%s  waiting for the opponent: %s  moves turned down: %d%s" % (
        ses.fen(), ses.waiting_for_opponent, n, "  (last: frame %d %s)" % (ignored[0], ignored[1].uci()) if ignored else ""))
    ses.end()
    p.close()


if __name__ == "__main__":
    main()
