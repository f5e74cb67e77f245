"""The yardstick of the pipeline's ChangeDetector blur kernel (cbv_pipeline_set_change_blur): ref_logic.RefChangeDetector
with `blur_kernel = k` (it preprocesses with O.square_preprocess(img, blur_kernel | 1) and is pinned to the reference by
tests/golden/ref_change_sequence.json), driven over model_update_ref's stream with its `new_ref` and `step`.  Nothing here
touches the code under test."""
import functools

import model_update_ref as R

PARAMS_SHIPPED = (2.55, 600, 0.13)  # the reference's sensitivity_settings.json (with blur_kernel 13)
PARAMS_B = R.PARAMS_B               # (1.45, 50, 0.37)
# (mode, parameters, kernels) the GPU tests compare against this yardstick
CASES = (("frozen", PARAMS_SHIPPED, (1, 13)), ("every", PARAMS_B, (3, 13, 31)), ("unchanged", PARAMS_B, (3, 13, 31)))
SWITCH_AT, SWITCH_FROM, SWITCH_TO = 14, 5, 13


@functools.lru_cache(maxsize=None)
def run_blur(mode, params, k, switch=None, grid=None, use_hough=True, display_size=(1280, 720)):
    """Every frame's detect_changes_detailed dict and the detector after the stream, calibrated on frame 0 with kernel `k`.
    `switch` = (frame, kernel): blur_kernel is set to `kernel` before that frame is processed; the model is kept."""
    sq = R.stream_squares(grid=grid, display_size=display_size)
    ref = R.new_ref(params, {} if use_hough else None)
    ref.blur_kernel = k
    ref.calibrate(sq[0])
    dicts = []
    for i in range(len(sq)):
        if switch is not None and i == switch[0]:
            ref.blur_kernel = switch[1]
        dicts.append(R.step(ref, mode, sq[i]))
    return dicts, ref


def keysets(dicts):
    return [frozenset(d) for d in dicts]


def same_planes(a, b):
    import numpy as np
    return all(np.array_equal(a.means[p], b.means[p]) and np.array_equal(a.variances[p], b.variances[p]) for p in a.means)
