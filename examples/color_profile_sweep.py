"""Finding a colour profile on a recorded clip: one round of coordinate descent over the five scalar trackbars of
calibrate_colors.py (hue_shift, sat_scale, val_scale, contrast, brightness), each axis judged in ONE device pass over frames
already in the pipeline, where the tool has one person moving sliders and looking at the grayscale view.

A synthetic clip with lilac-like pieces, which the PieceDetector misses on the frames as they are, and the scripted game as
the expected occupancy.  Along each axis the best position has the most frames whose smoothed occupancy is exactly the
expected one, then the fewest missed plus false pieces; it replaces that axis' value before the next axis is swept.  The
result is saved as the tool saves it (color_profile.json, which ImageEnhancer reads) and the pipeline is reconfigured with
`enhance="profile"`, the mode the sweep judges profiles for.

    python examples/color_profile_sweep.py [--frames 16] [--frames-per-ply 4] [--step 10] [--out color_profile.json]
                                           [--format bgr|nv12|yuyv]

`--step 10` takes every tenth trackbar position; `--step 1` is every position of the tool.
`--format nv12` (or yuyv) feeds camera-native frames to a pipeline configured with `enhance="profile", raw=True`: the raw
ring is the only frame store, the sweep runs on that very pipeline, and the profile found is applied with `set_profile`,
which keeps the pipeline's state.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chessboard_vision_amd import _native as N  # noqa: E402
from chessboard_vision_amd import synth as S  # noqa: E402
from chessboard_vision_amd.stream import (BoardPipeline, color_axis_profiles, color_full_profile, color_trackbar_axes, load_color_profile,  # noqa: E402
                                          save_color_profile)

LILAC = dict(bg_lo=60, bg_span=31, light=(190, 200, 210), dark=(90, 110, 135), white=(215, 175, 205), black=(120, 100, 125), noise=3, radius=0.36)


def camera_frame(bgr, fmt):
    """a camera-native frame of a BGR picture: BT.601 limited range, the chroma of each block's (pair's) first sample"""
    b, g, r = (bgr[..., i].astype(np.float32) for i in range(3))
    to8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)  # noqa: E731
    y, u, v = to8(16 + .257 * r + .504 * g + .098 * b), to8(128 - .148 * r - .291 * g + .439 * b), to8(128 + .439 * r - .368 * g - .071 * b)
    h, w = y.shape
    if fmt == "nv12":
        out = np.empty((h * 3 // 2, w), np.uint8)
        out[:h], out[h:, 0::2], out[h:, 1::2] = y, u[::2, ::2], v[::2, ::2]
        return out
    out = np.empty((h, w, 2), np.uint8)
    out[..., 0], out[:, 0::2, 1], out[:, 1::2, 1] = y, u[:, ::2], v[:, ::2]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--frames-per-ply", type=int, default=4)
    ap.add_argument("--step", type=int, default=10, help="every n-th position of each trackbar")
    ap.add_argument("--out", default="color_profile.json")
    ap.add_argument("--format", default="bgr", choices=("bgr", "nv12", "yuyv"), help="the format of the frames the pipeline is fed")
    a = ap.parse_args()
    w, h = 1280, 720
    pts = S.scaled_corners(w, h)
    p = BoardPipeline(w, h, a.frames)
    raw = a.format != "bgr"
    if raw:  # the clip as a camera delivers it: no BGR frame is kept on the device, the sweep reads the raw ring
        clip = BoardPipeline(w, h, a.frames)
        clip.configure(pts, enhance=False)
        clip.synth(0, a.frames, scene=N.Scene.from_dict(LILAC), frames_per_ply=a.frames_per_ply)
        p.configure(pts, enhance="profile", raw=True, profile=None)  # no profile yet: the plain raw warp
        p.set_input_format(a.format)
        for i in range(a.frames):
            p.upload(i, camera_frame(clip.download(0, i), a.format), fmt=a.format)
        clip.close()
    else:
        p.configure(pts, enhance=False)
        p.synth(0, a.frames, scene=N.Scene.from_dict(LILAC), frames_per_ply=a.frames_per_ply)  # stands for the recorded clip
    expected = [set(S.position_for_frame(i, a.frames_per_ply).keys()) for i in range(a.frames)]
    axes = color_trackbar_axes()
    profile = color_full_profile(None)  # the neutral profile
    base = p.color_sweep(0, a.frames, [None, profile], expected=expected, records=False).summary
    print("no profile: %d exact frames, %d missed, %d false" % (base["frames_exact"][0], base["missed"][0], base["false_pos"][0]))
    for axis in ("hue_shift", "sat_scale", "val_scale", "contrast", "brightness"):
        values = axes[axis][::a.step]
        res = p.color_sweep(0, a.frames, color_axis_profiles(profile, axis, values), expected=expected, records=False)
        j = res.best()
        profile = res.profiles[j]
        s = res.summary[j]
        print("%-10s %4d positions in %.1f ms on the GPU -> %-6g: %d exact frames, %d missed, %d false"
              % (axis, len(values), sum(res.info[k] for k in ("warp_ms", "squares_ms", "hough_ms", "eval_ms")), profile[axis], s["frames_exact"],
                 s["missed"], s["false_pos"]))
    save_color_profile(a.out, profile)
    print("saved %s" % a.out)
    # the pipeline with the profile found: the same chain, now per frame
    if raw:
        p.set_profile(load_color_profile(a.out))
    else:
        p.configure(pts, enhance="profile", profile=load_color_profile(a.out))
    p.run(0, a.frames)
    out = p.results(0, a.frames)
    roi_of = {(c, 7 - r): i for i, (r, c) in enumerate(p.rois_rc)}
    exact = sum(out[i].stable_occupied == sum(1 << roi_of[pos] for pos in expected[i]) for i in range(a.frames))
    print(('set_profile on the raw-frame pipeline' if raw else 'configure(enhance="profile")') + ': %d of %d frames exact in the live mode (changed squares only are looked at again)' % (exact, a.frames))
    p.close()


if __name__ == "__main__":
    main()
