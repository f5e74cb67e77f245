"""Records what the REFERENCE'S OWN classes return under the colour profile sweep's definition (include/cbv.h,
cbv_pipeline_color_sweep) on the yardstick stream of tests/color_sweep_ref.py (palette "low"):

  ref_color_profiles.json   for 4 of the profiles and the first 6 frames: ImageEnhancer with .profile set to the profile,
                            apply_color_profile(frame) -> board_detection.warp_image -> GridExtractor.split_board -> a
                            fresh PieceDetector (radii and Hough parameters of the yardstick's board) driven with
                            detect_all_pieces(squares, use_smoothing=True, squares_to_check=<all 64>) frame by frame;
                            result rows as tests/refrun.py::result_rows, and the sha256 of every warped board.
                            "tool_equals_enhancer": calibrate_colors.ColorCalibrator.apply_color_adjustments, called
                            unbound with the profile's eight values (defaults for missing keys), returned exactly
                            ImageEnhancer.apply_color_profile's bytes on those frames (null: the tool's module could not
                            be imported under the shim).

Runs only where the reference tree is present (it never travels), with `cv2` bound to tests/golden/cv2_oracle_shim.py
under the caveat of tests/golden/README.md: the reference's numpy arithmetic and control flow are pinned exactly, the
OpenCV-side pixel numbers are the oracle's own.

Run:  python tests/golden/make_color_profile_run.py
"""
import contextlib
import hashlib
import io
import json
import os
import shutil
import sys
import tempfile

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

from tests.golden import cv2_oracle_shim as shim  # noqa: E402

try:
    import cv2 as _cv2_real
    CV2_KIND = "opencv-python " + _cv2_real.__version__
except ImportError:
    sys.modules["cv2"] = shim.as_module()
    CV2_KIND = "oracle shim (tests/golden/cv2_oracle_shim.py): OpenCV-side numbers are the oracle's own"

# the reference reads color_profile.json / piece_detector_settings.json from the cwd at construction
_SCRATCH = tempfile.mkdtemp(prefix="cbv_ref_")
for _f in ("color_profile.json", "piece_detector_settings.json"):
    shutil.copy(os.path.join(REF, _f), _SCRATCH)
os.chdir(_SCRATCH)
with contextlib.redirect_stdout(io.StringIO()):
    import board_detection
    import frame_enhancer
    import grid_extractor
    import piece_detector
    try:
        import calibrate_colors
        TOOL_ERROR = None
    except Exception as e:  # the tool's module needs more of cv2 than the shim has
        calibrate_colors, TOOL_ERROR = None, "%s: %s" % (type(e).__name__, e)

import color_sweep_ref as CS  # noqa: E402
import refrun  # noqa: E402
from chessboard_vision_amd import synth as S  # noqa: E402

TOOL_DEFAULTS = dict(hue_shift=0, sat_scale=1.0, val_scale=1.0, contrast=1.0, brightness=0, radical_mode=0, target_hue=0, hue_window=20)


def main():
    pts = S.scaled_corners(CS.W, CS.H)
    lo, hi, p1, p2 = CS.HOUGH
    runs, tool_equal = [], (True if calibrate_colors else None)
    for name in CS.FIXTURE_PROFILES:
        prof = CS.PROFILES[name]
        with contextlib.redirect_stdout(io.StringIO()):
            enh = frame_enhancer.ImageEnhancer()
            det = piece_detector.PieceDetector()
        assert type(enh).__name__ == "ImageEnhancerPython"
        enh.profile = dict(prof)
        det.min_radius_ratio, det.max_radius_ratio, det.hough_param1, det.hough_param2 = lo, hi, p1, p2
        ge = grid_extractor.GridExtractor()
        frames, shas = [], []
        for i in range(CS.FIXTURE_FRAMES):
            f = np.array(CS.frame("low", i))
            col = enh.apply_color_profile(f)
            if calibrate_colors:
                kw = dict(TOOL_DEFAULTS, **prof)
                tool = calibrate_colors.ColorCalibrator.apply_color_adjustments(None, f, *[kw[k] for k in TOOL_DEFAULTS])
                tool_equal = tool_equal and bool(np.array_equal(tool, col))
            warped = board_detection.warp_image(col, pts)[0]
            shas.append(hashlib.sha256(np.ascontiguousarray(warped).tobytes()).hexdigest())
            sq = ge.split_board(warped)
            results, _ = det.detect_all_pieces(sq, use_smoothing=True, squares_to_check=set(sq.keys()))
            frames.append(refrun.result_rows(results))
        runs.append({"profile_name": name, "profile": prof, "warped_sha256": shas, "frames": frames})
    data = {"cv2": CV2_KIND, "size": [CS.W, CS.H], "frames_per_ply": CS.FRAMES_PER_PLY, "palette": {k: list(v) if isinstance(v, tuple) else v for k, v in CS.PALETTES["low"].items()},
            "hough": list(CS.HOUGH), "call": "detect_all_pieces(squares, use_smoothing=True, squares_to_check=<all 64>)",
            "tool_equals_enhancer": tool_equal, "tool_import_error": TOOL_ERROR, "runs": runs}
    with open(os.path.join(OUT, "ref_color_profiles.json"), "w") as f:
        json.dump(data, f, separators=(",", ":"))
    print("wrote ref_color_profiles.json:", os.path.getsize(os.path.join(OUT, "ref_color_profiles.json")), "bytes; tool == enhancer:", tool_equal, TOOL_ERROR)


if __name__ == "__main__":
    try:
        main()
    finally:
        shutil.rmtree(_SCRATCH, ignore_errors=True)
