"""The yardstick of the colour profile sweep (cbv_pipeline_color_sweep) and of the profile-only pipeline mode
(configure(enhance="profile")): two 640x480 streams of 8 frames (the low-contrast palette of piece_sweep_ref and a
lilac-like one), eleven colour profiles, and the chain the header defines, from the oracle and the restated reference class
alone: O.apply_color_profile -> O.warp_image -> split_board -> a fresh ref_logic.RefPieceDetector per profile with
detect_all_pieces(squares, use_smoothing=True, squares_to_check=<all 64>) on the frames in order.  The reference's own
classes pin it (tests/golden/ref_color_profiles.json).  Nothing here touches the code under test."""
import functools

from chessboard_vision_amd import synth as S

import piece_sweep_ref as PS

W, H = PS.W, PS.H
N_FRAMES, FRAMES_PER_PLY = 8, 4
HOUGH = (.20, .55, 100, 25)  # the board's setting: DETECTOR_DEFAULTS of stream.py
PALETTES = {
    "low": PS.PALETTE,
    "lilac": dict(PS.PALETTE, white=(215, 175, 205), black=(120, 100, 125)),
}
SHIPPED = {"hue_shift": -86, "sat_scale": 0.91, "val_scale": 2.46, "contrast": 1.48, "brightness": -30, "radical_mode": 0, "target_hue": 0,
           "hue_window": 26}
# name -> profile dict (None = no profile); "shipped" .. "fractional" are the six of tests/golden/make_reference_runs.py
PROFILES = {
    "none": None,
    "neutral": {"hue_shift": 0, "sat_scale": 1.0, "val_scale": 1.0, "contrast": 1.0, "brightness": 0},
    "shipped": SHIPPED,
    "radical": {"hue_shift": 17, "sat_scale": 1.3, "val_scale": 0.8, "contrast": 0.9, "brightness": 12, "radical_mode": 1, "target_hue": 30,
                "hue_window": 26},
    "radical_wrap": {"radical_mode": 1, "target_hue": 175, "hue_window": 12, "hue_shift": 95},
    "partial_negative": {"hue_shift": -200},
    "clipping": {"hue_shift": 179.5, "sat_scale": 3.7, "val_scale": 0.31, "contrast": 2.2, "brightness": -140},
    "fractional": {"hue_shift": 0.5, "sat_scale": 0.999, "val_scale": 1.001, "contrast": 1.0, "brightness": 0.49},
    "sat3": {"sat_scale": 3.0},
    "val06": {"val_scale": 0.6},
    "radical_lilac": {"radical_mode": 1, "target_hue": 150, "hue_window": 20, "sat_scale": 1.5},
}
NAMES = tuple(PROFILES)
FIXTURE_PROFILES = ("neutral", "shipped", "radical", "sat3")  # recorded from the reference's own classes (first 6 frames, palette "low")
FIXTURE_FRAMES = 6
PIPELINE_PROFILES = ("shipped", "radical", "sat3")  # the three the pipeline-mode and per-setting tests run
# test_gpu_stages.py's `fractional`: a hue shift below -180, a brightness that drives convertScaleAbs negative
STAGES_FRACTIONAL = {"hue_shift": -200.5, "sat_scale": 0.33, "val_scale": 1.01, "contrast": 2.5, "brightness": -140.25}


def oracle_scene(palette):
    from oracle import cbv_oracle as O
    pal = PALETTES[palette]
    sc = O.Scene()
    sc.bg_lo, sc.bg_span, sc.noise, sc.radius = pal["bg_lo"], pal["bg_span"], pal["noise"], pal["radius"]
    for k in ("light", "dark", "white", "black"):
        for i in range(3):
            getattr(sc, k)[i] = pal[k][i]
    return sc


def native_scene(palette):
    from chessboard_vision_amd import _native as N
    return N.Scene.from_dict(PALETTES[palette])


@functools.lru_cache(maxsize=None)
def frame(palette, i):
    from oracle import cbv_oracle as O
    Hinv = O.get_perspective_transform(S.scaled_corners(W, H), S.BOARD_UNIT_QUAD)
    board = S.board_array(S.position_for_frame(i, FRAMES_PER_PLY))
    f = O.synth_frame(S.frame_seed(0, i), W, H, Hinv, board, oracle_scene(palette))
    f.setflags(write=False)
    return f


def profiled(img, name):
    """ImageEnhancer(profile).apply_color_profile(img): the frame itself without a profile (frame_enhancer.py:57-58)"""
    from oracle import cbv_oracle as O
    prof = PROFILES[name] if isinstance(name, str) else name
    return O.apply_color_profile(img, prof) if prof else img


def extractor(grid=None):
    from chessboard_vision_amd.grid_extractor import GridExtractor, SmartGridExtractor
    if grid is None:
        return GridExtractor()
    ge = SmartGridExtractor()
    ge.grid_lines_x, ge.grid_lines_y = list(grid[0]), list(grid[1])
    return ge


@functools.lru_cache(maxsize=None)
def warped(palette, name, i, rot180=False):
    """the warped board of frame i under profile `name`: warp_image(apply_color_profile(frame)) (+ rotate 180)"""
    from oracle import cbv_oracle as O
    w = O.warp_image(profiled(frame(palette, i), name), S.scaled_corners(W, H))[0]
    w = w[::-1, ::-1].copy() if rot180 else w
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def stream_squares(palette, name, n=N_FRAMES, grid=None):
    ge = extractor(grid)
    return [ge.split_board(warped(palette, name, i)) for i in range(n)]


@functools.lru_cache(maxsize=None)
def run_profile(palette, name, n=N_FRAMES, grid=None):
    """The definition: per frame (results, raw) of a fresh RefPieceDetector on the profile's squares, as PS.run_setting"""
    from ref_logic import RefPieceDetector
    det = RefPieceDetector(hough=PS.hough_kw(HOUGH))
    out = []
    for sq in stream_squares(palette, name, n, grid):
        res, _ = det.detect_all_pieces(sq, use_smoothing=True, squares_to_check=set(sq.keys()))
        assert det.last_processed == set(sq.keys())
        out.append((res, {pos: dict(r) for pos, r in det.cached_results.items()}))
    return out


@functools.lru_cache(maxsize=None)
def yardstick_records(palette, names=NAMES, n=N_FRAMES):
    """[profile][frame] record dicts (PS.record_of)"""
    return [[PS.record_of(*fr) for fr in run_profile(palette, name, n)] for name in names]


def expected_bits(n=N_FRAMES):
    return PS.expected_bits(n, FRAMES_PER_PLY)


def summary_of(rows, expected):
    """(missed, false_pos, frames_exact) of one profile's records"""
    pop = lambda v: bin(v).count("1")  # noqa: E731
    return (sum(pop(e & ~r["stable_occupied"]) for r, e in zip(rows, expected)), sum(pop(r["stable_occupied"] & ~e) for r, e in zip(rows, expected)),
            sum(r["stable_occupied"] == e for r, e in zip(rows, expected)))
