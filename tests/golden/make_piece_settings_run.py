"""Records what the REFERENCE'S OWN PieceDetector returns under the settings sweep's definition (include/cbv.h,
cbv_pipeline_piece_sweep) on the yardstick stream of tests/piece_sweep_ref.py:

  ref_piece_settings.json   for 4 of the 18 settings and the first 6 frames: a fresh PieceDetector with
                            min_radius_ratio / max_radius_ratio / hough_param1 / hough_param2 set as
                            calibrate_piece_detector.py and piece_detector.py:229-230 (getattr) read them, driven with
                            detect_all_pieces(squares, use_smoothing=True, squares_to_check=<all 64>) frame by frame;
                            result rows as tests/refrun.py::result_rows

Runs only where the reference tree is present (it never travels), with `cv2` bound to tests/golden/cv2_oracle_shim.py
under the caveat of tests/golden/README.md: the reference's numpy arithmetic and control flow are pinned exactly, the
OpenCV-side pixel numbers are the oracle's own.

Run:  python tests/golden/make_piece_settings_run.py
"""
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile

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

# the reference reads piece_detector_settings.json from the cwd at construction (piece_detector.py:54)
_SCRATCH = tempfile.mkdtemp(prefix="cbv_ref_")
shutil.copy(os.path.join(REF, "piece_detector_settings.json"), _SCRATCH)
os.chdir(_SCRATCH)
with contextlib.redirect_stdout(io.StringIO()):
    import piece_detector

import piece_sweep_ref as PS  # noqa: E402
import refrun  # noqa: E402


def main():
    squares = PS.stream_squares()[:PS.FIXTURE_FRAMES]
    runs = []
    for j in PS.FIXTURE_SETTINGS:
        lo, hi, p1, p2 = PS.SETTINGS[j]
        with contextlib.redirect_stdout(io.StringIO()):
            det = piece_detector.PieceDetector()
        det.min_radius_ratio, det.max_radius_ratio, det.hough_param1, det.hough_param2 = lo, hi, p1, p2
        frames = []
        for sq in squares:
            results, _ = det.detect_all_pieces(sq, use_smoothing=True, squares_to_check=set(sq.keys()))
            frames.append(refrun.result_rows(results))
        runs.append({"setting_index": j, "setting": [lo, hi, p1, p2], "frames": frames})
    data = {"cv2": CV2_KIND, "size": [PS.W, PS.H], "frames_per_ply": PS.FRAMES_PER_PLY, "palette": {k: list(v) if isinstance(v, tuple) else v for k, v in PS.PALETTE.items()},
            "call": "detect_all_pieces(squares, use_smoothing=True, squares_to_check=<all 64>)", "runs": runs}
    with open(os.path.join(OUT, "ref_piece_settings.json"), "w") as f:
        json.dump(data, f, separators=(",", ":"))
    print("wrote ref_piece_settings.json:", os.path.getsize(os.path.join(OUT, "ref_piece_settings.json")), "bytes")


if __name__ == "__main__":
    try:
        main()
    finally:
        shutil.rmtree(_SCRATCH, ignore_errors=True)
