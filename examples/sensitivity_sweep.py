"""Finding ChangeDetector settings on a recorded clip: one device pass over frames already in the pipeline answers every
trackbar position of calibrate_sensitivity.py (51 x 80 x 8 settings), where the tool has one person watching the board.

A synthetic clip on the chain the tool runs (`enhance=False`): frame 0 calibrates, the frames before the first ply are
quiet, then the scripted plies follow.  A usable setting reports nothing on the quiet frames; among those, the settings
that see the most move frames (two squares, no hand) behind them come first, and the first is saved in the tool's file.

    python examples/sensitivity_sweep.py [--frames 192] [--frames-per-ply 32] [--out sensitivity_settings.json]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chessboard_vision_amd import synth as S  # noqa: E402
from chessboard_vision_amd.stream import BoardPipeline, save_sensitivity_settings, sensitivity_trackbar_grid  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=192)
    ap.add_argument("--frames-per-ply", type=int, default=32)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=0.20, help="written to the file as it is: the tool never updates its model")
    ap.add_argument("--out", default="sensitivity_settings.json")
    a = ap.parse_args()
    w, h = 1280, 720
    quiet_end = a.frames_per_ply  # the first ply is played at this frame
    p = BoardPipeline(w, h, a.frames)
    p.configure(S.scaled_corners(w, h), enhance=False)
    p.synth(0, a.frames, scene="normal", frames_per_ply=a.frames_per_ply)  # stands for the recorded clip
    p.run(0, a.frames)
    z, iv, k = sensitivity_trackbar_grid()
    quiet = p.sensitivity_sweep(0, 1, quiet_end - 1, z, iv, k, records=False)
    rest = p.sensitivity_sweep(0, quiet_end, a.frames - quiet_end, z, iv, k, records=False)
    info = rest.info
    print("%d settings x %d frames: planes %.2f ms, histograms %.2f ms, evaluation %.2f ms on the GPU"
          % (len(rest.settings), a.frames - quiet_end, info["planes_ms"], info["hist_ms"], info["eval_ms"]))
    silent = np.flatnonzero(quiet.summary["frames_changed"] == 0)
    print("%d of %d settings report nothing on the %d quiet frames" % (len(silent), len(quiet.settings), quiet_end - 1))
    if not len(silent):
        return
    s = rest.summary[silent]
    order = silent[np.lexsort((s["frames_hand"], -s["frames_move"].astype(np.int64)))]
    print("%6s %5s %3s %12s %12s %14s %8s" % ("z", "iv", "k", "move frames", "hand frames", "lifted frames", "z_max"))
    for j in order[:a.top]:
        st, sm = rest.settings[j], rest.summary[j]
        print("%6.2f %5d %3d %12d %12d %14d %8.2f" % (st["z_threshold"], st["initial_variance"], st["blur_kernel"], sm["frames_move"],
                                                      sm["frames_hand"], sm["frames_lifted"], sm["z_max"]))
    best = rest.settings[order[0]]
    save_sensitivity_settings(a.out, float(best["z_threshold"]), float(best["initial_variance"]), int(best["blur_kernel"]), a.alpha)
    print("saved z_threshold %.2f, initial_variance %d, blur_kernel %d to %s" % (best["z_threshold"], best["initial_variance"], best["blur_kernel"], a.out))
    p.close()


if __name__ == "__main__":
    main()
