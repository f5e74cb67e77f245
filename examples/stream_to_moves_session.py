"""Frames in, moves out, with the game session on the device: the whole of GameSession.on_frame (warp, detection, smart
scan, stable-move detection, the move rule, reference refresh) runs per frame on the GPU inside batched runs, and the
host reads back a short list of moves and a FEN.

    python examples/stream_to_moves_session.py [--frames 256] [--run 64] [--rule game_state]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chessboard_vision_amd import synth as S  # noqa: E402
from chessboard_vision_amd.stream import BoardPipeline  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--run", type=int, default=64)
    ap.add_argument("--rule", default="game_state", choices=["session", "game_state"])
    a = ap.parse_args()
    w, h = 1280, 720
    p = BoardPipeline(w, h, a.run)
    p.configure(S.scaled_corners(w, h), enhance=False)
    ses = p.session_begin(rule=a.rule, fps=30, cooldown_frames=10)
    for f0 in range(0, a.frames, a.run):
        c = min(a.run, a.frames - f0)
        p.synth(0, c, frame0=f0, scene="normal", frames_per_ply=32)  # stands for the camera's frames of this batch
        p.run(0, c)
        for frame, move, status in ses.moves():
            print("frame %4d  %s  %s" % (frame, move.uci(), status))
    print(ses.fen())
    ses.end()
    p.close()


if __name__ == "__main__":
    main()
