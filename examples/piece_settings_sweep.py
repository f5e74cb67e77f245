"""Finding PieceDetector settings on a recorded clip: one device pass over frames already in the pipeline answers every
position of the MinRadius% and MaxRadius% trackbars of calibrate_piece_detector.py (50 x 70 settings), where the tool has
one person moving sliders until the window shows "Pecas: 32/32".

A synthetic clip on the chain the tool runs (`enhance=False`) with the scripted game as the expected occupancy.  The best
setting has the most frames whose smoothed occupancy is exactly the expected one, then the fewest missed plus false
pieces; it is saved in the tool's file, which PieceDetector reads at construction, with the report the tool's 's' key writes.

    python examples/piece_settings_sweep.py [--frames 16] [--frames-per-ply 4] [--step 5] [--out piece_detector_settings.json]

`--step 5` takes every fifth trackbar position (10 x 14 settings); `--step 1` is the tool's whole grid.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chessboard_vision_amd import synth as S  # noqa: E402
from chessboard_vision_amd.stream import BoardPipeline, piece_stats_text, piece_trackbar_grid, save_piece_settings  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--frames-per-ply", type=int, default=4)
    ap.add_argument("--step", type=int, default=5, help="every n-th position of the two radius trackbars")
    ap.add_argument("--param1", type=float, default=100)
    ap.add_argument("--param2", type=float, default=25)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--out", default="piece_detector_settings.json")
    a = ap.parse_args()
    w, h = 1280, 720
    p = BoardPipeline(w, h, a.frames)
    p.configure(S.scaled_corners(w, h), enhance=False)
    p.synth(0, a.frames, scene="normal", frames_per_ply=a.frames_per_ply)  # stands for the recorded clip
    p.run(0, a.frames)
    expected = [set(S.position_for_frame(i, a.frames_per_ply).keys()) for i in range(a.frames)]
    lo, hi = piece_trackbar_grid()
    lo, hi = lo[a.step - 1::a.step], hi[a.step - 1::a.step]
    res = p.piece_sweep(0, a.frames, lo, hi, param1s=(a.param1,), param2s=(a.param2,), expected=expected, records=False)
    print("%d settings x %d frames: HoughCircles %.1f ms, decision and smoothing %.2f ms on the GPU"
          % (len(res.settings), a.frames, res.info["hough_ms"], res.info["eval_ms"]))
    sm = res.summary
    order = np.lexsort((sm["missed"].astype(np.int64) + sm["false_pos"], -sm["frames_exact"].astype(np.int64)))
    print("%5s %5s %13s %7s %6s %7s %10s %12s %9s" % ("min%", "max%", "exact frames", "missed", "false", "hough", "tower_top", "center_diff", "radius"))
    for j in order[:a.top]:
        st, s = res.settings[j], sm[j]
        print("%5d %5d %13d %7d %6d %7d %10d %12d %4d..%-4d" % (round(st["min_radius_ratio"] * 100), round(st["max_radius_ratio"] * 100), s["frames_exact"],
                                                              s["missed"], s["false_pos"], s["n_hough"], s["n_tower_top"], s["n_center_diff"], s["r_min"], s["r_max"]))
    best = res.settings[res.best()]
    assert res.best() == order[0]
    save_piece_settings(a.out, float(best["min_radius_ratio"]), float(best["max_radius_ratio"]), hough_param1=int(a.param1), hough_param2=int(a.param2))
    print("saved min_radius %d, max_radius %d to %s" % (round(best["min_radius_ratio"] * 100), round(best["max_radius_ratio"] * 100), a.out))
    detail = p.piece_detail(a.frames - 1, float(best["min_radius_ratio"]), float(best["max_radius_ratio"]), a.param1, a.param2)
    # the tool's report takes (col, row) with row 0 = rank 8
    print(piece_stats_text({(f, 7 - r): d for (f, r), d in detail.items()}, p.board_size // 8), end="")
    p.close()


if __name__ == "__main__":
    main()
