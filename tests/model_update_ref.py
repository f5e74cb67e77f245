"""The yardstick of the pipeline's model-update modes (cbv_pipeline_set_model_update): the reference's ChangeDetector,
restated in ref_logic.RefChangeDetector and pinned to the reference by tests/golden/ref_change_sequence.json, driven call
for call as include/cbv.h defines the three modes, on the oracle chain's squares of a synthetic stream.  Nothing here
touches the code under test."""
import functools

from chessboard_vision_amd import synth as S
from helpers import oracle_frame

W, H = 640, 480
N_FRAMES, FRAMES_PER_PLY = 28, 8
# (z_threshold, initial_variance, alpha): the first reaches LEVE, PARCIAL and empty dicts, the second TOTAL and the
# np.maximum(new_var, 10.0) clamp (tests/test_model_update_host.py asserts both)
PARAMS_A = (2.55, 600, 0.1)
PARAMS_B = (1.45, 50, 0.37)
MODES = ("frozen", "every", "unchanged")


@functools.lru_cache(maxsize=None)
def stream_squares(n=N_FRAMES, frames_per_ply=FRAMES_PER_PLY, grid=None, display_size=(1280, 720)):
    """Per frame the {(file, rank): BGR square} dict of the oracle chain: synth -> process_pipeline -> warp -> split.
    `grid`: None = GridExtractor, else (grid_lines_x, grid_lines_y) tuples for SmartGridExtractor."""
    from oracle import cbv_oracle as O
    from chessboard_vision_amd.grid_extractor import GridExtractor, SmartGridExtractor
    pts = S.scaled_corners(W, H)
    out = []
    for i in range(n):
        f = oracle_frame(W, H, "normal", frame_idx=i, frames_per_ply=frames_per_ply)
        warped, _, _ = O.warp_image(O.process_pipeline(f, {}), pts, display_size=display_size)
        if grid is None:
            ge = GridExtractor()
        else:
            ge = SmartGridExtractor()
            ge.grid_lines_x, ge.grid_lines_y = list(grid[0]), list(grid[1])
        out.append(ge.split_board(warped))
    return out


def step(ref, mode, squares):
    """One frame in a mode: detect_changes_detailed against the model as it is, then the mode's update."""
    detailed = ref.detect_changes_detailed(squares)
    if mode == "every":
        ref.clear_focus()
        ref.update_all_references(squares)
    elif mode == "unchanged":
        keep = set(squares) - set(detailed)
        if keep:  # an empty focus set means "all squares" in the reference: a frame that reports every square updates none
            ref.set_focus_squares(keep)
            ref.update_all_references(squares)
            ref.clear_focus()
    else:
        assert mode == "frozen"
    return detailed


def new_ref(params, hough={}):
    from ref_logic import RefChangeDetector
    ref = RefChangeDetector(hough=hough)
    ref.z_threshold, ref.initial_variance, ref.alpha = params
    return ref


@functools.lru_cache(maxsize=None)
def run_mode(mode, params, calibrate_at=(0,), grid=None, use_hough=True, display_size=(1280, 720)):
    """The yardstick's result dict of every frame and its detector after the stream.  `calibrate_at`: frames whose
    squares calibrate the model BEFORE the frame is processed (as `run(i, 1); calibrate_changes(i)` then a run from i)."""
    sq = stream_squares(grid=grid, display_size=display_size)
    ref = new_ref(params, {} if use_hough else None)
    dicts = []
    for i in range(len(sq)):
        if i in calibrate_at:
            ref.calibrate(sq[i])
        dicts.append(step(ref, mode, sq[i]))
    return dicts, ref
