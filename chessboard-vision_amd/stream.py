"""Device-resident batched path: enhance -> warp -> 64-square detect over
frames that stay in HBM (the composed chain of SURVEY.md §3 D).

One BoardPipeline = one camera stream on one GPU: an input frame ring, the
per-square temporal state of PieceDetector.detect_all_pieces
(reference squares, cached raw results, 5-frame history) and the result ring.
Streams are independent, so N GPUs run N pipelines with no exchange.
"""
import ctypes as C
import json

import numpy as np

from . import _native as N
from . import synth as S
from .board_detection import get_perspective_transform, undistort_points
from .develop import Develop, develop_tables, load_develop, save_develop  # noqa: F401  (Develop and its JSON belong to this module's surface)
from .grid_extractor import GridExtractor, SmartGridExtractor


def bits_to_positions(bits, rois_rc):
    """u64 bitset over roi indices -> {(file, rank)} (a1 = (0,0), row 0 = rank 8)."""
    return {(c, 7 - r) for i, (r, c) in enumerate(rois_rc) if (bits >> i) & 1}


# The detector settings of a board and their defaults: the keywords of BoardPipeline.configure and BoardPipeline.add_board
DETECTOR_DEFAULTS = dict(history_size=5, min_presence=0.6, change_threshold=25, z_threshold=2.5, initial_variance=100,
                         use_hough=True, min_radius_ratio=0.20, max_radius_ratio=0.55, hough_param1=100, hough_param2=25)
_D = DETECTOR_DEFAULTS


def load_sensitivity_settings(path="sensitivity_settings.json"):
    """The ChangeDetector settings calibrate_sensitivity.py saves: {"z_threshold", "initial_variance", "blur_kernel",
    "alpha"}; the tool's other keys are left out.  z_threshold, initial_variance and blur_kernel are keywords of
    `configure` / `add_board`, alpha goes to `set_model_update`.  (The reference's ChangeDetector never reads the file
    itself: only the tool writes and reloads it.)"""
    with open(path) as f:
        data = json.load(f)
    return {"z_threshold": float(data["z_threshold"]), "initial_variance": float(data["initial_variance"]),
            "blur_kernel": int(data["blur_kernel"]), "alpha": float(data["alpha"])}


# calibrate_sensitivity.py:31-39, the file's keys and the values the tool starts from
SENSITIVITY_FILE_DEFAULTS = {"sensitivity": 25, "blur_kernel": 5, "stable_frames": 10, "z_threshold": 2.0, "alpha": 0.20,
                             "initial_variance": 100, "use_gaussian": True}


def save_sensitivity_settings(path, z_threshold, initial_variance, blur_kernel, alpha, **other):
    """Write the file calibrate_sensitivity.py saves (:56-59: json, indent 2) with these ChangeDetector settings.  An
    existing file keeps every key that is not given here; a new one starts from the tool's defaults (:31-39), as the tool's
    own load-then-save does.  `other`: further keys of the file (sensitivity, stable_frames, use_gaussian, ...).
    `load_sensitivity_settings(path)` returns what was written."""
    data = dict(SENSITIVITY_FILE_DEFAULTS)
    try:
        with open(path) as f:
            data.update(json.load(f))
    except FileNotFoundError:
        pass
    iv = float(initial_variance)
    data.update(other)
    data.update(z_threshold=float(z_threshold), initial_variance=int(iv) if iv == int(iv) else iv, blur_kernel=int(blur_kernel),
                alpha=float(alpha))
    with open(path, "w") as f:
        json.dump(data, f, indent=2)
    return data


def sensitivity_trackbar_grid():
    """(z_thresholds, initial_variances, blur_kernels): every value the trackbars of calibrate_sensitivity.py can produce
    (:91-98 the ranges, :116-126 and :139 the formulas), duplicates removed, in trackbar order: 51, 80 and 8 values."""
    def uniq(values):
        return list(dict.fromkeys(values))
    z = uniq(max(0.5, min(3.0, 3.0 - s / 20.0)) for s in range(51))
    iv = uniq(max(10, t * 10) for t in range(81))
    k = uniq(max(1, b) | 1 for b in range(16))
    return z, iv, k


def piece_trackbar_grid():
    """(min_radius_ratios, max_radius_ratios): every value the MinRadius% (0..50) and MaxRadius% (0..70) trackbars of
    calibrate_piece_detector.py can produce (:118-121 the ranges, :135 `max(1, v)`, :113-114 `/ 100`), duplicates removed,
    in trackbar order: 50 and 70 values."""
    def uniq(values):
        return list(dict.fromkeys(values))
    return uniq(max(1, v) / 100 for v in range(51)), uniq(max(1, v) / 100 for v in range(71))


# calibrate_piece_detector.py:36-45, the file's keys and the values the tool starts from
PIECE_FILE_DEFAULTS = {"min_radius": 20, "max_radius": 55, "hough_param1": 100, "hough_param2": 30, "small_min": 12, "small_max": 25,
                       "knight_aspect_max": 250, "center_diff_thresh": 40}


def save_piece_settings(path, min_radius_ratio, max_radius_ratio, **other):
    """Write the piece_detector_settings.json that calibrate_piece_detector.py saves (:61-66: json, indent 2) and
    PieceDetector reads at construction (piece_detector.py:52-68): `min_radius` and `max_radius` are integer percent of the
    square; `other` (hough_param1, hough_param2, small_min, ...) passes through.  An existing file keeps every key that is
    not given here; a new one starts from the tool's defaults (:36-45).  Returns what was written."""
    data = dict(PIECE_FILE_DEFAULTS)
    try:
        with open(path) as f:
            data.update(json.load(f))
    except FileNotFoundError:
        pass
    data.update(other)
    data.update(min_radius=int(round(min_radius_ratio * 100)), max_radius=int(round(max_radius_ratio * 100)))
    with open(path, "w") as f:
        json.dump(data, f, indent=2)
    return data


def piece_stats_text(results, sq_size):
    """The report DetectorCalibrator.export_stats writes to piece_stats.txt (calibrate_piece_detector.py:72-107), as a
    string: `results` = {(col, row): detect_piece dict} as the tool passes it (`piece_detail`'s dict works: its keys are
    (file, rank), which the tool's report labels the same way)."""
    area_square = sq_size ** 2
    out = [f"=== ESTATISTICAS DE PECAS ({len(results)} casas analisadas) ===\n", f"Square Size: {sq_size}px\n",
           f"{'CASA':<6} {'STATUS':<10} {'METODO':<15} {'RAIO':<8} {'AREA%':<8} {'BG%':<8} {'CONF'}\n", "-" * 80 + "\n"]
    count = 0
    for (col, row), info in results.items():
        if info["has_piece"]:
            count += 1
            coord = f"{chr(ord('a') + col)}{8 - row}"
            radius = info.get("radius", 0)
            method = info.get("method", "N/A")
            conf = info.get("confidence", 0.0)
            pct_area = (np.pi * (radius ** 2) / area_square) * 100
            pct_bg = 100 - pct_area
            out.append(f"{coord:<6} {'PECA':<10} {method:<15} {radius:<8} {pct_area:<8.1f} {pct_bg:<8.1f} {conf:.2%}\n")
    out.append("-" * 80 + "\n")
    out.append(f"Total de pecas detectadas: {count}\n")
    return "".join(out)


class PieceSweepResult:
    """What `piece_sweep` returns.  `settings`: [S] structured array (dp, param1, param2, min_radius_ratio,
    max_radius_ratio as given).  With records: `raw_occupied`, `stable_occupied`, `hough`, `tower_top`, `center_diff`,
    `symmetry` (uint64 square sets, bit i = roi i), `n_raw`, `n_stable`, `r_min`, `r_max`, `flags` as [S, F] arrays.
    `summary`: [S] structured array (frames, frames_exact, missed, false_pos, n_hough, n_tower_top, n_center_diff,
    n_symmetry, r_min, r_max, n_r, overflow, r_sum).  `info`: dict of the GPU times (ms) of the two kernels, the number of
    distinct param1 values and the chunk."""

    def __init__(self, settings, records, summary, info, rois_rc):
        self.settings, self.records, self.summary, self.info, self._rois_rc = settings, records, summary, info, rois_rc
        if records is not None:
            for name in records.dtype.names:
                setattr(self, name, records[name])

    def occupied(self, s, i, stable=True):
        """{(file, rank)} of setting s on frame i."""
        if self.records is None:
            raise RuntimeError("the sweep was made with records=False")
        return bits_to_positions(int((self.stable_occupied if stable else self.raw_occupied)[s, i]), self._rois_rc)

    def best(self):
        """Index of the best setting: most frames_exact, then fewest missed + false_pos, then the first."""
        sm = self.summary
        return min(range(len(sm)), key=lambda j: (-int(sm["frames_exact"][j]), int(sm["missed"][j]) + int(sm["false_pos"][j]), j))


class ColorSweepResult(PieceSweepResult):
    """What `color_sweep` returns.  `profiles`: the dicts as given (`None` / `{}` = disabled).  With records: the fields of
    PieceSweepResult as [P, F] arrays.  `summary`: [P] structured array as PieceSweepResult's.  `info`: dict of the GPU
    times (ms) of the four stages (warp, squares, hough, eval) and the chunk sizes.  `occupied(p, i)` and `best()` as
    PieceSweepResult's."""

    def __init__(self, profiles, records, summary, info, rois_rc):
        PieceSweepResult.__init__(self, profiles, records, summary, info, rois_rc)
        self.profiles = profiles


# calibrate_colors.py:194-203, the keys of color_profile.json in the tool's order
COLOR_PROFILE_KEYS = ("hue_shift", "sat_scale", "val_scale", "contrast", "brightness", "radical_mode", "target_hue", "hue_window")


def color_trackbar_axes():
    """{key: [values]}: every value each trackbar of calibrate_colors.py can produce, in trackbar order (:23-42 the
    ranges, :137-145 the formulas): hue_shift pos - 180 for 0..360, sat_scale / val_scale / contrast pos / 100.0 for
    0..300, brightness pos - 100 for 0..200, radical_mode 0 / 1, target_hue 0..179, hue_window 0..50."""
    scale = [pos / 100.0 for pos in range(301)]
    return {"hue_shift": [pos - 180 for pos in range(361)], "sat_scale": list(scale), "val_scale": list(scale), "contrast": list(scale),
            "brightness": [pos - 100 for pos in range(201)], "radical_mode": [0, 1], "target_hue": list(range(180)),
            "hue_window": list(range(51))}


def color_full_profile(profile):
    """The eight keys of `profile` with ImageEnhancer.apply_color_profile's defaults (frame_enhancer.py:61-68) for the
    missing ones: an ENABLED profile, also for `None` / `{}`."""
    d = dict(hue_shift=0, sat_scale=1.0, val_scale=1.0, contrast=1.0, brightness=0, radical_mode=0, target_hue=0, hue_window=20)
    d.update({k: v for k, v in (profile or {}).items() if k in COLOR_PROFILE_KEYS})
    return d


def color_axis_profiles(base, axis, values=None):
    """The profiles along one trackbar: `base` (missing keys take the defaults) with `axis` set to each of `values`
    (default: every position of that trackbar, `color_trackbar_axes`)."""
    if axis not in COLOR_PROFILE_KEYS:
        raise ValueError("colour profile axis %r: expected one of %s" % (axis, ", ".join(COLOR_PROFILE_KEYS)))
    if values is None:
        values = color_trackbar_axes()[axis]
    return [dict(color_full_profile(base), **{axis: v}) for v in values]


def save_color_profile(path, profile):
    """Write the color_profile.json calibrate_colors.py saves (:194-204, :54-57: the eight keys, json, indent 4), which
    ImageEnhancer.load_profile reads from the working directory.  Missing keys take the defaults.  Returns what was
    written."""
    full = color_full_profile(profile)
    data = {k: full[k] for k in COLOR_PROFILE_KEYS}
    with open(path, "w") as f:
        json.dump(data, f, indent=4)
    return data


def load_color_profile(path="color_profile.json"):
    """The profile dict of a color_profile.json, as ImageEnhancer.load_profile returns it."""
    with open(path) as f:
        return json.load(f)


class Lens:
    """The camera's lens as cv2.calibrateCamera describes it: the camera matrix (fx, fy, cx, cy) and OpenCV's first five
    distortion coefficients (k1, k2, p1, p2, k3), include/cbv.h's cbv_lens.  The warp corrects the distortion in its gather
    (`BoardPipeline.configure(lens=...)`, `set_lens`, `board_detection.warp_image(lens=...)`): one interpolation per pixel,
    for every frame format.  Estimating the coefficients is cv2's business; this class consumes them."""
    FIELDS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")

    def __init__(self, fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.k1, self.k2, self.p1, self.p2, self.k3 = float(k1), float(k2), float(p1), float(p2), float(k3)

    @classmethod
    def from_opencv(cls, camera_matrix, dist_coeffs):
        """From the 3 x 3 camera_matrix and the dist_coeffs (4 or 5 of them: k1, k2, p1, p2[, k3]) of cv2.calibrateCamera.
        Longer vectors are taken when everything beyond the fifth coefficient is zero; the rational, thin-prism and tilt
        terms are not modelled (ValueError)."""
        K = np.asarray(camera_matrix, dtype=np.float64).reshape(3, 3)
        d = np.asarray(dist_coeffs, dtype=np.float64).reshape(-1)
        if d.size < 4:
            raise ValueError("dist_coeffs: 4 or 5 coefficients (k1, k2, p1, p2[, k3]), got %d" % d.size)
        if np.any(d[5:] != 0):
            raise ValueError("dist_coeffs beyond k3 are not zero: the rational and thin-prism terms are not modelled")
        return cls(K[0, 0], K[1, 1], K[0, 2], K[1, 2], d[0], d[1], d[2], d[3], d[4] if d.size > 4 else 0.0)

    def scaled(self, from_size, to_size):
        """The same lens for frames of another resolution: from_size, to_size = (w, h).  fx, cx scale with the width and
        fy, cy with the height; the coefficients act on normalised coordinates and stay."""
        sx, sy = float(to_size[0]) / float(from_size[0]), float(to_size[1]) / float(from_size[1])
        return Lens(self.fx * sx, self.fy * sy, self.cx * sx, self.cy * sy, self.k1, self.k2, self.p1, self.p2, self.k3)

    @property
    def camera_matrix(self):
        return np.array([[self.fx, 0.0, self.cx], [0.0, self.fy, self.cy], [0.0, 0.0, 1.0]])

    @property
    def dist_coeffs(self):
        return np.array([self.k1, self.k2, self.p1, self.p2, self.k3])

    def struct(self):
        """The cbv_lens of this lens, enabled."""
        return N.LensStruct(1, 0, *(getattr(self, k) for k in self.FIELDS))

    def __eq__(self, other):
        return isinstance(other, Lens) and all(getattr(self, k) == getattr(other, k) for k in self.FIELDS)

    def __repr__(self):
        return "Lens(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.FIELDS)


def lens_struct(lens):
    """The cbv_lens of a Lens; None is the disabled one."""
    return lens.struct() if lens is not None else N.LensStruct()


def save_tones(path, model):
    """Write a ToneModel as tone_model.json beside the other settings files: {"centroid": [light, dark][white, black][b, g, r],
    "margin"}.  The doubles round-trip exactly (repr)."""
    d = {"centroid": [[[float(model.centroid[k][p][c]) for c in range(3)] for p in range(2)] for k in range(2)], "margin": float(model.margin)}
    with open(path, "w") as f:
        json.dump(d, f, indent=2)
    return d


def load_tones(path="tone_model.json"):
    """The ToneModel save_tones wrote."""
    with open(path) as f:
        d = json.load(f)
    m = N.ToneModel()
    for k in range(2):
        for p in range(2):
            for c in range(3):
                m.centroid[k][p][c] = float(d["centroid"][k][p][c])
    m.margin = float(d.get("margin", 0.125))
    m.calibrated = 1
    return m


def save_lens(path, lens, image_size=None):
    """Write a lens as JSON: camera_matrix (3 x 3), dist_coeffs (5) and, when given, image_size = [w, h], the resolution
    the calibration was made at (`Lens.scaled` takes it from there to another).  Returns what was written."""
    data = {"camera_matrix": lens.camera_matrix.tolist(), "dist_coeffs": lens.dist_coeffs.tolist()}
    if image_size is not None:
        data["image_size"] = [int(image_size[0]), int(image_size[1])]
    with open(path, "w") as f:
        json.dump(data, f, indent=4)
    return data


def load_lens(path, with_size=False):
    """The Lens of a JSON file with camera_matrix and dist_coeffs (`save_lens`, or the two arrays cv2.calibrateCamera
    returned, dumped as lists).  with_size=True: (lens, image_size or None)."""
    with open(path) as f:
        data = json.load(f)
    lens = Lens.from_opencv(data["camera_matrix"], data["dist_coeffs"])
    size = tuple(int(v) for v in data["image_size"]) if data.get("image_size") is not None else None
    return (lens, size) if with_size else lens


class SweepResult:
    """What `sensitivity_sweep` returns.  `settings`: [S] structured array (z_threshold, initial_variance, blur_kernel as
    given).  With records: `changed`, `parcial`, `total` (uint64 square sets, bit i = roi i), `z_max`, `n_changed`,
    `n_total`, `is_hand`, `is_move`, `lifted` (roi or -1) as [S, F] arrays.  `summary`: [S] structured array
    (frames_changed, frames_hand, frames_move, frames_lifted, squares_reported, z_max).  `info`: dict of the GPU times (ms) of
    the three stages, the number of distinct blur kernels and the chunk."""

    def __init__(self, settings, records, summary, info, rois_rc):
        self.settings, self.records, self.summary, self.info, self._rois_rc = settings, records, summary, info, rois_rc
        if records is not None:
            for name in ("changed", "parcial", "total", "z_max", "n_changed", "n_total", "lifted"):
                setattr(self, name, records[name])
            self.is_hand = (records["flags"] & N.SWEEP_HAND) != 0
            self.is_move = (records["flags"] & N.SWEEP_MOVE) != 0

    def pattern(self, s, i):
        """ChangeDetector.classify_hand_pattern's dict for setting s on frame i, positions as (file, rank)."""
        if self.records is None:
            raise RuntimeError("the sweep was made with records=False")
        return classify_hand_bits(int(self.changed[s, i]), int(self.total[s, i]), self._rois_rc)


def classify_hand_bits(changed, total, rois_rc):
    """ChangeDetector.classify_hand_pattern (change_detector.py:169-201) from the `changed` and `total` bitsets of one
    frame (bit i = roi i, `rois_rc` as bits_to_positions takes it)."""
    n = bin(changed).count("1")
    if bin(total).count("1") >= 2 or n >= 4 or n > 2:
        return {"is_hand": True, "is_move": False, "move_candidates": set()}
    return {"is_hand": False, "is_move": n == 2, "move_candidates": bits_to_positions(changed, rois_rc)}


def _fill_board(cfg, points, grid_lines, rot180, display_size, margin, history_size, min_presence, change_threshold,
                z_threshold, initial_variance, use_hough, min_radius_ratio, max_radius_ratio, hough_param1, hough_param2, lens=None):
    """The per-board fields of a PipelineConfig or BoardConfig: geometry, square table and detector settings.  With a
    `lens` the points are positions in the frame as delivered: they are undistorted first, and the matrix is the
    ideal-coordinate one."""
    S_ = min(display_size) - margin
    if lens is not None:
        points = undistort_points(points, lens)
    M = get_perspective_transform(np.float32(points), np.float32([[0, 0], [S_, 0], [0, S_], [S_, S_]]))
    for i in range(9):
        cfg.M[i] = float(M.reshape(9)[i])
    cfg.board_size, cfg.rot180 = S_, 1 if rot180 else 0
    if grid_lines is not None:
        ge = SmartGridExtractor()
        ge.grid_lines_x, ge.grid_lines_y = list(grid_lines[0]), list(grid_lines[1])
    else:
        ge = GridExtractor()
    table = ge.roi_table(S_, S_)
    cfg.n_rois = len(table)
    rois_rc = []
    for i, (r, c, x0, y0, w, h) in enumerate(table):
        cfg.rois[i].x0, cfg.rois[i].y0, cfg.rois[i].w, cfg.rois[i].h = x0, y0, w, h
        rois_rc.append((r, c))
    cfg.history_size, cfg.min_presence, cfg.change_threshold = history_size, min_presence, change_threshold
    cfg.z_threshold, cfg.initial_variance = z_threshold, initial_variance
    cfg.use_hough = int(use_hough)  # 2 = evaluate HoughCircles on every non-uniform square (inspection)
    cfg.hough = N.HoughParams(1.2, float(hough_param1), float(hough_param2), float(min_radius_ratio), float(max_radius_ratio))
    return S_, M, rois_rc


class _BoardMethods:
    """The per-board calls, shared by BoardPipeline (board 0) and the boards attached to it (Board): the handle `h_`
    names one board, whose temporal state, results and warped frames they read or change."""

    def set_check_squares(self, slot0, sets, count=None):
        """`squares_to_check` of detect_all_pieces per frame: a list of {(file, rank)} sets for the slots slot0.. —
        those squares are evaluated afresh even when unchanged and cached.  `sets=None` clears `count` slots
        (default: all from slot0)."""
        if sets is None:
            n = self.max_frames - slot0 if count is None else count
            self.ctx.check(self.ctx.lib.cbv_pipeline_set_check_squares(self.h_, slot0, n, None))
            return
        roi_of = {(c, 7 - r): i for i, (r, c) in enumerate(self.rois_rc)}
        masks = np.zeros(len(sets), np.uint64)
        for k, st in enumerate(sets):
            m = 0
            for pos in (st or ()):
                if pos in roi_of:
                    m |= 1 << roi_of[pos]
            masks[k] = m
        self.ctx.check(self.ctx.lib.cbv_pipeline_set_check_squares(self.h_, slot0, len(sets), N.ptr(masks)))

    def update_references(self, slot, reset_noise=False):
        """PieceDetector.update_references with the squares of a processed slot (and NoiseHandler.reset() when
        `reset_noise`): what the session does right after it accepted a move (game_session.py:219-223)."""
        self.ctx.check(self.ctx.lib.cbv_pipeline_update_references(self.h_, slot, 1 if reset_noise else 0))

    def reset_state(self):
        self.ctx.check(self.ctx.lib.cbv_pipeline_reset_state(self.h_))

    def calibrate_changes(self, slot):
        """ChangeDetector.calibrate from an already processed slot: later runs also classify
        every square's change (LEVE / PARCIAL / TOTAL) against that background model."""
        self.ctx.check(self.ctx.lib.cbv_pipeline_calibrate(self.h_, slot))

    def set_model_update(self, mode="frozen", alpha=0.1):
        """What happens to the ChangeDetector model after each frame of the runs enqueued from now on: "frozen" (default)
        nothing, "every" ChangeDetector.update_all_references on all squares, "unchanged" the same on the squares the
        frame did not report only (include/cbv.h, cbv_pipeline_set_model_update).  `alpha` is ChangeDetector.alpha."""
        if not isinstance(mode, int):
            if str(mode).lower() not in N.MODEL_MODES:
                raise ValueError("model update mode %r: expected one of %s" % (mode, ", ".join(sorted(N.MODEL_MODES))))
            mode = N.MODEL_MODES[str(mode).lower()]
        self.ctx.check(self.ctx.lib.cbv_pipeline_set_model_update(self.h_, mode, float(alpha)))

    def set_change_blur(self, blur_kernel):
        """ChangeDetector.blur_kernel of this board for the runs enqueued from now on (default 5): values below 1 count as
        1, then `| 1`, at most 31.  The model is kept; `calibrate_changes` of a slot last run with another kernel raises
        until the slot is run again (include/cbv.h, cbv_pipeline_set_change_blur)."""
        self.ctx.check(self.ctx.lib.cbv_pipeline_set_change_blur(self.h_, int(blur_kernel)))
        self._change_blur = max(int(blur_kernel), 1) | 1

    def set_profile(self, profile):
        """The colour profile of this board (the pipeline's own board or an attached one) for the runs enqueued from now
        on: a dict with the keys of color_profile.json, `None` / `{}` = none.  Only on a pipeline configured with
        `enhance="profile"`; every board starts with the profile `configure` was given.  Detector, model, noise and
        session state are kept (include/cbv.h, cbv_pipeline_set_profile)."""
        self.ctx.check(self.ctx.lib.cbv_pipeline_set_profile(self.h_, N.ColorProfile.from_dict(profile)))

    @property
    def change_blur(self):
        """The blur kernel the ChangeDetector stage of this board runs with."""
        return getattr(self, "_change_blur", 5)

    def hand_pattern(self, result):
        """ChangeDetector.classify_hand_pattern of one frame's cbv_frame_result: what calibrate_sensitivity.py:156-162
        computes right after detect_changes_detailed."""
        return classify_hand_bits(result.changed, result.total, self.rois_rc)

    def sensitivity_sweep(self, calib_slot, slot0, count, z_thresholds=None, initial_variances=None, blur_kernels=None,
                          settings=None, records=True, chunk_frames=0):
        """What calibrate_sensitivity.py's loop reports for many trackbar positions at once (include/cbv.h,
        cbv_pipeline_sweep): every setting on the processed slots slot0 .. slot0 + count - 1, judged against a model
        calibrated on `calib_slot` and never updated, exactly as a board configured with that setting would report it.
        Settings: itertools.product(z_thresholds, initial_variances, blur_kernels), or `settings` = [(z_threshold, initial_variance, blur_kernel)].  The board itself is not touched.  `records=False`
        returns the per-setting summary only.  Returns a SweepResult."""
        import itertools
        if settings is None:
            if z_thresholds is None or initial_variances is None or blur_kernels is None:
                raise ValueError("sensitivity_sweep: give z_thresholds, initial_variances and blur_kernels, or settings")
            settings = list(itertools.product(z_thresholds, initial_variances, blur_kernels))
        sets = np.zeros(len(settings), N.record_dtype(N.SweepSetting))
        for i, (z, iv, k) in enumerate(settings):
            sets[i] = (z, iv, k)
        rec = np.zeros((len(sets), count), N.record_dtype(N.SweepRecord)) if records else None
        summ = np.zeros(len(sets), N.record_dtype(N.SweepSummary))
        info = N.SweepInfo()
        self.ctx.check(self.ctx.lib.cbv_pipeline_sweep(self.h_, calib_slot, slot0, count, N.ptr(sets), len(sets), chunk_frames,
                                                       N.ptr(rec) if records else None, N.ptr(summ), info))
        return SweepResult(sets, rec, summ, {name: getattr(info, name) for name, _ in N.SweepInfo._fields_}, self.rois_rc)

    def piece_sweep(self, slot0, count, min_radius_ratios=None, max_radius_ratios=None, param1s=(100,), param2s=(25,),
                    expected=None, records=True, chunk_frames=16, settings=None):
        """What calibrate_piece_detector.py shows for many positions of its radius and Hough trackbars at once
        (include/cbv.h, cbv_pipeline_piece_sweep): every setting on the processed slots slot0 .. slot0 + count - 1, as a
        fresh PieceDetector with that setting reports them when every square is checked on every frame (raw and smoothed
        occupancy, methods, radii).  Settings: itertools.product(min_radius_ratios, max_radius_ratios, param1s, param2s), or
        `settings` = [(min_radius_ratio, max_radius_ratio, param1, param2)].  `expected`: per frame a {(file, rank)} set or a
        roi bitset, for the summary's frames_exact / missed / false_pos.  The board itself is not touched.  `records=False`
        returns the per-setting summary only.  Returns a PieceSweepResult."""
        import itertools
        if settings is None:
            if min_radius_ratios is None or max_radius_ratios is None:
                raise ValueError("piece_sweep: give min_radius_ratios and max_radius_ratios, or settings")
            settings = list(itertools.product(min_radius_ratios, max_radius_ratios, param1s, param2s))
        sets = np.zeros(len(settings), N.record_dtype(N.HoughParams))
        for i, (lo, hi, p1, p2) in enumerate(settings):
            sets[i] = (1.2, p1, p2, lo, hi)
        exp = None
        if expected is not None:
            if len(expected) != count:
                raise ValueError("piece_sweep: `expected` needs one entry per frame")
            roi_of = {(c, 7 - r): i for i, (r, c) in enumerate(self.rois_rc)}
            exp = np.array([e if isinstance(e, (int, np.integer)) else sum(1 << roi_of[pos] for pos in e) for e in expected], np.uint64)
        rec = np.zeros((len(sets), count), N.record_dtype(N.PieceSweepRecord)) if records else None
        summ = np.zeros(len(sets), N.record_dtype(N.PieceSweepSummary))
        info = N.PieceSweepInfo()
        self.ctx.check(self.ctx.lib.cbv_pipeline_piece_sweep(self.h_, slot0, count, N.ptr(sets), len(sets), N.ptr(exp) if exp is not None else None,
                                                             chunk_frames, N.ptr(rec) if records else None, N.ptr(summ), info))
        return PieceSweepResult(sets, rec, summ, {name: getattr(info, name) for name, _ in N.PieceSweepInfo._fields_}, self.rois_rc)

    def color_sweep(self, slot0, count, profiles, expected=None, chunk_frames=0, records=True):
        """What calibrate_colors.py's trackbars do to the PieceDetector, for many positions at once (include/cbv.h,
        cbv_pipeline_color_sweep): every profile on the frames in the slots slot0 .. slot0 + count - 1 (as uploaded; they
        need not have been run), as a board configured with `enhance="profile"`, that profile and every square checked
        reports them: apply_color_profile -> warp -> split -> a fresh PieceDetector with this board's radii and Hough
        settings.  `profiles`: dicts with the keys of color_profile.json (missing keys take ImageEnhancer's defaults),
        `None` / `{}` = the frame as it is.  `expected`: per frame a {(file, rank)} set or a roi bitset, for the summary's
        frames_exact / missed / false_pos.  The board itself is not touched.  `records=False` returns the per-profile
        summary only.  Returns a ColorSweepResult."""
        profiles = list(profiles)
        profs = (N.ColorProfile * len(profiles))(*[N.ColorProfile.from_dict(d) for d in profiles])
        exp = None
        if expected is not None:
            if len(expected) != count:
                raise ValueError("color_sweep: `expected` needs one entry per frame")
            roi_of = {(c, 7 - r): i for i, (r, c) in enumerate(self.rois_rc)}
            exp = np.array([e if isinstance(e, (int, np.integer)) else sum(1 << roi_of[pos] for pos in e) for e in expected], np.uint64)
        rec = np.zeros((len(profiles), count), N.record_dtype(N.PieceSweepRecord)) if records else None
        summ = np.zeros(len(profiles), N.record_dtype(N.PieceSweepSummary))
        info = N.ColorSweepInfo()
        self.ctx.check(self.ctx.lib.cbv_pipeline_color_sweep(self.h_, slot0, count, profs, len(profiles), N.ptr(exp) if exp is not None else None,
                                                             chunk_frames, N.ptr(rec) if records else None, N.ptr(summ), info))
        return ColorSweepResult(profiles, rec, summ, {name: getattr(info, name) for name, _ in N.ColorSweepInfo._fields_}, self.rois_rc)

    def piece_detail(self, slot, min_radius_ratio=_D["min_radius_ratio"], max_radius_ratio=_D["max_radius_ratio"],
                     param1=_D["hough_param1"], param2=_D["hough_param2"]):
        """{(file, rank): dict} shaped like detect_all_pieces' results, for one setting on one processed slot: detect_piece
        of every square (has_piece is the raw value), by the sweep's own kernel (cbv_pipeline_piece_detail)."""
        out = (N.PieceResult * len(self.rois_rc))()
        prm = N.HoughParams(1.2, float(param1), float(param2), float(min_radius_ratio), float(max_radius_ratio))
        self.ctx.check(self.ctx.lib.cbv_pipeline_piece_detail(self.h_, slot, prm, out))
        res = {}
        for i, (r, c) in enumerate(self.rois_rc):
            o = out[i]
            has = bool(o.has_piece)
            res[(c, 7 - r)] = {"has_piece": has, "confidence": o.confidence, "center": (o.cx, o.cy) if has else None,
                               "radius": o.radius if has else None, "method": N.METHOD_NAMES[o.method],
                               "center_border_diff": o.center_border_diff,
                               "is_ellipse": False, "axes": None}
        return res

    def change_hist(self, calib_slot, slot, blur_kernel):
        """[n_rois, 256] uint16: per square the histogram of |gray - calibration gray| of a processed slot against
        `calib_slot` under ChangeDetector.blur_kernel = `blur_kernel`, the sufficient statistic of the sweep."""
        out = np.zeros((len(self.rois_rc), 256), np.uint16)
        self.ctx.check(self.ctx.lib.cbv_pipeline_change_hist(self.h_, calib_slot, slot, int(blur_kernel), N.ptr(out)))
        return out

    def change_radar(self, pattern, game):
        """The radar of calibrate_sensitivity.py:173-189 on a classify_hand_pattern dict (`hand_pattern`,
        `SweepResult.pattern`) and a GameState: with exactly one move candidate, no hand, and a piece of the side to move
        on that square, (lifted (file, rank), [(file, rank) of that piece's legal destinations, in move order]); else
        (None, []).  Host code."""
        from . import chess_rules as chess
        candidates = pattern.get("move_candidates", set())
        if len(candidates) != 1 or pattern.get("is_hand"):
            return None, []
        lifted = next(iter(candidates))
        sq = chess.square(*lifted)
        piece = game.board.piece_at(sq)
        if not piece or piece.color != game.board.turn:
            return None, []
        return lifted, [(chess.square_file(m.to_square), chess.square_rank(m.to_square)) for m in game.board.legal_moves if m.from_square == sq]

    def model(self, pos):
        """(mean, variance) float32 planes of the square at (file, rank) after every run enqueued so far:
        ChangeDetector.means[pos], .variances[pos]."""
        roi = {(c, 7 - r): i for i, (r, c) in enumerate(self.rois_rc)}[tuple(pos)]
        w, h = self._cfg.rois[roi].w, self._cfg.rois[roi].h
        planes = []
        for which in (0, 1):
            out = np.empty((h, w), np.float32)
            self.ctx.check(self.ctx.lib.cbv_pipeline_model(self.h_, which, roi, N.ptr(out)))
            planes.append(out)
        return planes[0], planes[1]

    def hough(self, slot):
        """HoughCircles outcome of every square of a processed slot (index = roi)."""
        out = (N.HoughResult * N.MAX_SQUARES)()
        self.ctx.check(self.ctx.lib.cbv_pipeline_hough(self.h_, slot, out))
        return out

    def changes_detailed(self, result, slot):
        """The dict ChangeDetector.detect_changes_detailed returns (change_detector.py:105-167) for one frame."""
        st = self.square_stats(slot)
        out = {}
        for i, (r, c) in enumerate(self.rois_rc):
            if not (result.changed >> i) & 1:
                continue
            pct = (st[i].z_count / st[i].n) * 100
            inten = "TOTAL" if (result.total >> i) & 1 else ("PARCIAL" if (result.parcial >> i) & 1 else "LEVE")
            out[(c, 7 - r)] = {"z_score": float(st[i].z_max), "pct_changed": pct, "intensity": inten,
                               "is_circular": bool((result.circular >> i) & 1), "center_ratio": 1.0}
        return out

    def results(self, slot0, count):
        out = (N.FrameResult * count)()
        self.ctx.check(self.ctx.lib.cbv_pipeline_results(self.h_, slot0, count, out))
        return out

    def noise_results(self, slot0, count):
        """NoiseHandler.process outputs of the frames, as (NoiseState, data) tuples (game_session.py:165)."""
        from .noise_handler import decode_device_result
        out = (N.NoiseResult * count)()
        self.ctx.check(self.ctx.lib.cbv_pipeline_noise_results(self.h_, slot0, count, out))
        idx2pos = [(c, 7 - r) for (r, c) in self.rois_rc]
        return [decode_device_result(r, idx2pos) for r in out]

    def download(self, which, slot):
        shape = (self.h, self.w, 3) if which in (0, 1) else (self.board_size, self.board_size, 3)
        out = np.empty(shape, np.uint8)
        self.ctx.check(self.ctx.lib.cbv_pipeline_download(self.h_, which, slot, N.ptr(out)))
        return out

    def square_stats(self, slot):
        out = (N.SqStats * len(self.rois_rc))()
        self.ctx.check(self.ctx.lib.cbv_pipeline_square_stats(self.h_, slot, out))
        return out

    def occupied(self, result, stable=True):
        return bits_to_positions(result.stable_occupied if stable else result.raw_occupied, self.rois_rc)

    # ---- piece colour per square (include/cbv.h, "piece colour per square") ----

    def tone_sums(self, slot):
        """cbv_tone_sums of the 64 squares of a processed slot (index = roi), with tones on or off."""
        out = (N.ToneSums * N.MAX_SQUARES)()
        self.ctx.check(self.ctx.lib.cbv_pipeline_tone_sums(self.h_, slot, out))
        return out

    def set_tones(self, model):
        """Turn the board's tone stage on with a calibrated ToneModel, or off with None: with it on every processed frame
        leaves its tone record (`tones`), and a session begun with tones=True breaks the rules' ties with it."""
        self.ctx.check(self.ctx.lib.cbv_pipeline_set_tones(self.h_, model))
        self.tone_model = model

    def calibrate_tones(self, slot, position=None, margin=0.125):
        """Calibrate the tones on a processed slot that shows a known position and turn the stage on.  `position`: 64 bytes
        in synth.board_array's convention (0 empty, 1 white, 2 black, ROI order), a FEN, or None = the board of the session
        running on this board, else the start position.  Returns the report: {"samples", "D", "misclassified",
        "undecided"}, the last two as lists of (file, rank) squares the new model does not classify cleanly."""
        from .piece_tone import position_array, report_dict
        if position is None:
            ses = getattr(self, "_session", None)
            position = ses.fen() if ses is not None and ses._open else None
        pos = position_array(position)
        model, rep = N.ToneModel(), N.ToneReport()
        self.ctx.check(self.ctx.lib.cbv_tone_calibrate_host(self.tone_sums(slot), N.ptr(pos), float(margin), model, rep))
        self.set_tones(model)
        return report_dict(rep)

    def tones(self, slot0, count):
        """cbv_tone_result of processed slots: .white / .black, bit = roi, all 64 squares whatever their occupancy."""
        out = (N.ToneResult * count)()
        self.ctx.check(self.ctx.lib.cbv_pipeline_tones(self.h_, slot0, count, out))
        return out

    def piece_colours(self, result, tone):
        """{(file, rank): "w" | "b" | None} for the stably occupied squares of a frame (its FrameResult and ToneResult)."""
        out = {}
        for i, (r, c) in enumerate(self.rois_rc):
            if (result.stable_occupied >> i) & 1:
                w, b = (tone.white >> i) & 1, (tone.black >> i) & 1
                out[(c, 7 - r)] = "w" if w and not b else "b" if b and not w else None
        return out

    def verify_position(self, slot, fen=None):
        """The slot's stable occupancy and tones against a position (None = the start position): {"ok", "missing" (expected,
        not seen), "extra" (seen, not expected), "wrong_colour", "undecided"}, lists of (file, rank).  The reference's
        unbuilt initial-position check ("Confirmar posição inicial com visão")."""
        from .piece_tone import position_array
        pos = position_array(fen)
        seen = self.piece_colours(self.results(slot, 1)[0], self.tones(slot, 1)[0])
        want = {(i & 7, 7 - (i >> 3)): "w" if pos[i] == 1 else "b" for i in range(64) if pos[i]}
        both = sorted(set(seen) & set(want))
        rep = {"missing": sorted(set(want) - set(seen)), "extra": sorted(set(seen) - set(want)),
               "wrong_colour": [s for s in both if seen[s] is not None and seen[s] != want[s]],
               "undecided": [s for s in both if seen[s] is None]}
        rep["ok"] = not any(rep.values())
        return rep

    def session_begin(self, rule="session", fps=30, fen=None, online=None, radar=False, tones=False, **cfg):
        """Start a game session on this board (include/cbv.h, cbv_pipeline_session_begin): from now on every frame of
        every `run` also goes through the back half of GameSession.on_frame on the device (smart-scan check sets, stable
        move detection, the move rule, and after an accepted move update_references + NoiseHandler.reset()), whatever the
        run length.  `rule`: "session" = GameSession._infer_move, "game_state" = GameState.process_occupancy_change.
        Keywords: stability_required (20), cooldown_frames (round(MOVE_COOLDOWN * fps)), scan_period (30), max_diff (4),
        smart_scan (True).  `online` "white" / "black": the session of LichessSession for that player (rule "session"
        only) — moves found while it is the opponent's turn are turned down, and the opponent's moves arrive through
        Session.sync_moves.  `radar`: every frame leaves the lifted piece and its destinations (Session.radar).
        `tones`: the rule breaks ties with the board's piece tones (calibrate_tones / set_tones first).
        Returns a Session."""
        from .game_state import StableMoveTracker
        if rule not in N.SESSION_RULES:
            raise ValueError("rule %r: expected one of %s" % (rule, ", ".join(sorted(N.SESSION_RULES))))
        d = dict(stability_required=StableMoveTracker.STABILITY_REQUIRED, cooldown_frames=int(round(StableMoveTracker.MOVE_COOLDOWN * fps)),
                 scan_period=30, max_diff=4, smart_scan=True)
        unknown = set(cfg) - set(d)
        if unknown:
            raise TypeError("session_begin: unknown keyword(s) %s" % ", ".join(sorted(unknown)))
        d.update(cfg)
        if online not in N.SESSION_ONLINE:
            raise ValueError("online %r: expected 'white', 'black' or None" % (online,))
        c = N.SessionConfig(N.SESSION_RULES[rule], int(d["stability_required"]), int(d["cooldown_frames"]), int(d["scan_period"]),
                            int(d["max_diff"]), 1 if d["smart_scan"] else 0, N.SESSION_ONLINE[online], 1 if radar else 0, 1 if tones else 0)
        self.ctx.check(self.ctx.lib.cbv_pipeline_session_begin(self.h_, c, fen.encode() if fen is not None else None))
        self._session = Session(self, c)
        return self._session


class Session:
    """A game session running on a board (`session_begin`).  The host reads back moves and the position; the frames never
    leave the device."""

    def __init__(self, board, config):
        self._b, self.config = board, config
        self.ctx = board.ctx
        self._open = True

    def state(self):
        """cbv_session_state after every run enqueued so far."""
        st = N.SessionState()
        self.ctx.check(self.ctx.lib.cbv_pipeline_session_state(self._b.h_, st))
        return st

    def moves(self):
        """The moves accepted since the previous call: [(frame since session_begin, chess_rules.Move, status string)]."""
        from . import chess_rules as chess
        out = (N.SessionMove * N.SESSION_RING)()
        n = C.c_int()
        self.ctx.check(self.ctx.lib.cbv_pipeline_session_moves(self._b.h_, out, N.SESSION_RING, C.byref(n)))
        lib = chess._L()
        return [(out[i].frame, chess.Move._from_code(out[i].move), lib.cbv_game_status_name(out[i].status).decode()) for i in range(n.value)]

    def fen(self):
        st = self.state()
        buf = C.create_string_buffer(128)
        self.ctx.lib.cbv_session_state_fen(st, buf, 128)
        return buf.value.decode()

    @property
    def board(self):
        """A chess_rules.Board at the session's position (its move stack starts here)."""
        from . import chess_rules as chess
        b = chess.Board()
        b.set_fen(self.fen())
        return b

    @property
    def stable_count(self):
        return self.state().stable_count

    def sync_moves(self, moves_str, at_frame=None):
        """LichessSession._sync_moves (lichess_session.py:89-117) in front of session frame `at_frame` (None = the next frame
        to be enqueued): the board becomes the start position plus the legal tokens of `moves_str`, and
        waiting_for_opponent follows from the number of tokens and the player's colour as LichessClient.is_my_turn has it
        (an offline session is never waiting).  Does not wait for the runs in flight."""
        pos = N.SessionPos()
        self.ctx.check(self.ctx.lib.cbv_session_pos_from_moves((moves_str or "").encode(), pos, None))
        count = len((moves_str or "").split())
        mine = {0: True, 1: count % 2 == 0, 2: count % 2 == 1}[self.config.online]
        if at_frame is None:
            nxt = C.c_int()
            self.ctx.check(self.ctx.lib.cbv_pipeline_session_frames(self._b.h_, C.byref(nxt)))
            at_frame = nxt.value
        self.ctx.check(self.ctx.lib.cbv_pipeline_session_sync(self._b.h_, int(at_frame), pos, 0 if mine else 1))

    def radar(self, slot0, n):
        """GameSession._update_radar_ui per frame of processed slots: [(lifted (file, rank) or None, [(file, rank), ...])],
        a1 = (0, 0), the destinations in square order (the reference lists them in move order).  Needs
        session_begin(radar=True)."""
        out = (N.SessionRadar * n)()
        self.ctx.check(self.ctx.lib.cbv_pipeline_session_radar(self._b.h_, slot0, n, out))
        pos = [(c, 7 - r) for (r, c) in self._b.rois_rc]
        return [(pos[r.lifted] if r.lifted >= 0 else None, sorted(bits_to_positions(r.destinations, self._b.rois_rc))) for r in out]

    @property
    def waiting_for_opponent(self):
        return bool(self.state().waiting_for_opponent)

    @property
    def ignored(self):
        """(moves turned down so far, the last of them as (frame, chess_rules.Move) or None).  A move is counted once, on
        the frame the rule found it, not on the identical frames behind it."""
        from . import chess_rules as chess
        st = self.state()
        return st.n_ignored, ((st.ignored_frame, chess.Move._from_code(st.ignored_move)) if st.n_ignored else None)

    def end(self):
        if self._open and self._b.h_:
            self.ctx.check(self.ctx.lib.cbv_pipeline_session_end(self._b.h_))
        self._open = False


_NO_PROFILE = object()  # add_board(profile=...) not given: the board keeps the pipeline's configured profile


class BoardPipeline(_BoardMethods):
    def __init__(self, w, h, max_frames, ctx=None):
        self.ctx = ctx or N.context()
        self.w, self.h, self.max_frames = w, h, max_frames
        hdl = C.c_void_p()
        self.ctx.check(self.ctx.lib.cbv_pipeline_create(self.ctx.h, w, h, max_frames, C.byref(hdl)))
        self.h_ = hdl
        self.rois_rc = []
        self.board_size = 0
        self._boards = []
        self.input_format = "bgr"
        self.develop = None
        self.lens = None

    def set_lens(self, lens):
        """The camera's lens (a `Lens`; None turns it off), shared by every board of the pipeline: every warp goes through
        it from the next run on (include/cbv.h, cbv_pipeline_set_lens).  The boards' matrices stay as they are: with a lens
        they are expected in ideal coordinates, which `configure(points, lens=...)` and `add_board` see to."""
        self.ctx.check(self.ctx.lib.cbv_pipeline_set_lens(self.h_, lens_struct(lens)))
        self.lens = lens

    def close(self):
        if self.h_:
            for b in list(self._boards):  # the library frees them with the pipeline: their handles die here
                b.h_ = None
            self._boards.clear()
            self.ctx.lib.cbv_pipeline_destroy(self.h_)
            self.h_ = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def configure(self, points, profile=None, grid_lines=None, rot180=False, chunk=0, lanes=0, keep_enhanced=False,
                  clahe_clip_limit=3.0, tile_grid_size=(8, 8), sharpen_kernel=None, display_size=(1280, 720), margin=100,
                  history_size=_D["history_size"], min_presence=_D["min_presence"], change_threshold=_D["change_threshold"],
                  z_threshold=_D["z_threshold"], initial_variance=_D["initial_variance"], use_hough=_D["use_hough"],
                  min_radius_ratio=_D["min_radius_ratio"], max_radius_ratio=_D["max_radius_ratio"],
                  hough_param1=_D["hough_param1"], hough_param2=_D["hough_param2"], enhance_region=False, enhance=True,
                  blur_kernel=5, raw=False, lens=None):
        """`lens` (a `Lens`, or None for a pinhole camera): the camera's lens distortion is corrected inside the warp of
        every board of this pipeline (`set_lens`), and `points` are the corners as clicked in the frame as delivered.
        `use_hough` and the radii mirror PieceDetector's attributes (piece_detector.py:33-35,222-230);
        pass min_radius / 100 and max_radius / 100 of piece_detector_settings.json as the application does.
        `enhance_region` (only without keep_enhanced): enhance the part of each frame the warp samples first and the rest
        only when normalize's global min / max could depend on it; every output stays identical (include/cbv.h).
        `enhance=True` (default) reproduces the composed chain process_pipeline -> warp -> split -> detect.
        `enhance="profile"` runs apply_color_profile -> warp -> rotate -> split -> detect: of the enhancement only the
        colour `profile`, applied inside the warp at nearly the cost of `enhance=False`; the CLAHE and sharpen settings are
        ignored, `keep_enhanced` and `enhance_region` are errors, a `None` / `{}` profile is `enhance=False`'s warp, and
        YUV frames are converted into the BGR ring as with `enhance=True`, unless `raw=True`: then a YUV or Bayer
        `set_input_format` makes the raw ring the frames, as with `enhance=False`, and the warp converts its taps and
        applies the profile to them (`raw=True` with any other `enhance` is a ValueError; with BGR frames it changes
        nothing).  `color_sweep` judges profiles for this mode, on either kind of ring; `set_profile` gives a board a
        profile of its own.
        `enhance=False` reproduces what GameSession.on_frame (game_session.py:123-161) and calibrate_sensitivity.py:142-157
        run: the warp samples the camera frame as it is, then rotate, split and detect; `profile` (used by `enhance=True`
        and `enhance="profile"` only), the CLAHE and sharpen settings are ignored, `keep_enhanced` and `enhance_region` are errors, and with a YUV `set_input_format` the warp
        reads the raw frames directly (raw mode: `upload` takes that format only, `synth` is an error, `download(0, slot)`
        converts the slot).
        `blur_kernel`: ChangeDetector.blur_kernel (`set_change_blur`)."""
        cfg = N.PipelineConfig()
        e = cfg.enhance
        e.profile = N.ColorProfile.from_dict(profile)
        e.clahe_clip_limit = clahe_clip_limit
        e.tiles_x, e.tiles_y = tile_grid_size
        e.bilateral_d, e.sigma_color, e.sigma_space = 9, 75.0, 75.0
        k = np.asarray(sharpen_kernel if sharpen_kernel is not None else [[-1, -1, -1], [-1, 9, -1], [-1, -1, -1]],
                       dtype=np.float32).reshape(9)
        for i in range(9):
            e.sharpen_kernel[i] = float(k[i])
        S_, M, rois_rc = _fill_board(cfg, points, grid_lines, rot180, display_size, margin, history_size, min_presence,
                                     change_threshold, z_threshold, initial_variance, use_hough, min_radius_ratio,
                                     max_radius_ratio, hough_param1, hough_param2, lens=lens)
        cfg.chunk, cfg.lanes, cfg.keep_enhanced = chunk, lanes, 1 if keep_enhanced else 0
        cfg.enhance_region = 1 if enhance_region else 0
        if isinstance(enhance, str) and enhance != "profile":
            raise ValueError("enhance %r: expected True, False or \"profile\"" % (enhance,))
        if raw and enhance != "profile":
            raise ValueError("raw=True goes with enhance=\"profile\" (enhance=False samples raw frames as it is), got enhance=%r" % (enhance,))
        cfg.skip_enhance = (N.SKIP_ENHANCE_PROFILE_RAW if raw else N.SKIP_ENHANCE_PROFILE) if enhance == "profile" else (0 if enhance else 1)
        if lens is not None or getattr(self, "lens", None) is not None:  # (a caller without a lens makes the calls it always made)
            self.set_lens(lens)
        self.ctx.check(self.ctx.lib.cbv_pipeline_configure(self.h_, cfg))
        self.rois_rc = rois_rc
        self.board_size = S_
        self.matrix = M
        self._cfg = cfg
        self.set_change_blur(blur_kernel)

    def add_board(self, points, grid_lines=None, rot180=False, display_size=(1280, 720), margin=100, blur_kernel=5, profile=_NO_PROFILE,
                  **detector):
        """Attach another board seen by the same camera (include/cbv.h, cbv_pipeline_add_board): it shares this
        pipeline's frames and enhancement, and has its own geometry, detector settings (the detector keywords of
        `configure`: history_size, min_presence, change_threshold, z_threshold, initial_variance, use_hough,
        min_radius_ratio, max_radius_ratio, hough_param1, hough_param2), `blur_kernel` (`set_change_blur`), colour
        `profile` (`set_profile`; not given: the pipeline's configured one) and temporal state.  `run` processes every
        attached board.  Returns a Board with the per-board methods of this class."""
        b = Board(self, points, grid_lines, rot180, display_size, margin, **detector)
        b.set_change_blur(blur_kernel)
        if profile is not _NO_PROFILE:
            b.set_profile(profile)
        return b

    def frames_ptr(self):
        return self.ctx.lib.cbv_pipeline_frames_dev(self.h_)

    def upload(self, slot, frame, fmt="bgr", colorspace="bt601"):
        """One frame into a slot, synchronous.  `fmt` "nv12" / "nv21" (one [h * 3 // 2, w] array or a (y, chroma) pair of
        possibly strided views), "yuv420p" / "yv12" (one contiguous [h * 3 // 2, w] array or the three planes in memory
        order, (y, u, v) / (y, v, u)) and "yuyv" / "yvyu" / "uyvy" ([h, w, 2]) are converted to BGR on the GPU (include/cbv.h,
        cbv_pipeline_upload_raw; "i420" is not a name, the format is "yuv420p"), and so are the 8-bit Bayer mosaics
        "bayer_rggb" / "bayer_bggr" / "bayer_grbg" / "bayer_gbrg" (one [h, w] array, named by the top-left 2 x 2 block:
        cv2's COLOR_BayerBG2BGR is "bayer_rggb") and those of more bits, "...16" (one uint16 [h, w] array), "...10p" and "...12p"
        (MIPI-packed rows, uint8 [h, w * 5 // 4] / [h, w * 3 // 2]), which go through the pipeline's tables (`set_develop`) when
        the format is the pipeline's own and through their format's default otherwise; in raw mode (`configure(enhance=False)` or `(enhance="profile", raw=True)` with a YUV or Bayer
        `set_input_format`) the frame is stored as it is.  `colorspace`: of a YUV frame (`set_input_format`); a raw-mode
        ring takes frames of its own format and colour space only."""
        N.colorspace_bits(colorspace, fmt)
        if isinstance(fmt, str) and fmt.lower() == "mjpeg":  # one baseline JPEG stream (bytes or a uint8 array), decoded on the GPU
            a = np.frombuffer(frame, np.uint8) if isinstance(frame, (bytes, bytearray, memoryview)) else np.ascontiguousarray(frame, dtype=np.uint8).reshape(-1)
            self.ctx.check(self.ctx.lib.cbv_pipeline_upload_jpeg(self.h_, slot, N.ptr(a), a.size))
            return
        if N.format_id(fmt) == N.FMT_BGR:
            f = N.as_bgr(frame)
            assert f.shape[:2] == (self.h, self.w)
            self.ctx.check(self.ctx.lib.cbv_pipeline_upload(self.h_, slot, N.ptr(f), f.strides[0]))
            return
        raw, w, h, keep = N.raw_frame(frame, fmt, colorspace)
        if (h, w) != (self.h, self.w):
            raise ValueError("a %dx%d %s frame does not fit the pipeline's %dx%d frames" % (w, h, fmt, self.w, self.h))
        self.ctx.check(self.ctx.lib.cbv_pipeline_upload_raw(self.h_, slot, raw))

    def set_develop(self, develop):
        """The per-colour tables of the pipeline's Bayer input format (include/cbv.h, cbv_pipeline_set_bayer_tables): a
        `Develop`, a uint8 [3, 2^bits] array (rows B, G, R), or None for the format's default (the neutral table of a
        "...16" / "...10p" / "...12p" format, no table for an 8-bit mosaic).  They apply wherever the ring's mosaics become
        BGR: `submit`, raw mode's warp, `upload` in the pipeline's format, `download(0, slot)` in raw mode, `color_sweep`.
        Call between runs; detector, model and session state are kept.  RuntimeError when the input format is not Bayer."""
        # (another input format: the library refuses the call whatever the tables are, so none are built)
        tables, bits = develop_tables(develop, N.format_id(self.input_format)) if N.is_bayer(self.input_format) else (None, 0)
        self.ctx.check(self.ctx.lib.cbv_pipeline_set_bayer_tables(self.h_, N.ptr(tables) if tables is not None else None, bits))
        self.develop = develop

    def set_input_format(self, fmt, slot_bytes=None, planes=False, colorspace="bt601", develop=None):
        """Format of the frames the capture side writes into `host_ring()`: "bgr" (default), "nv12", "nv21", "yuv420p"
        (cv2's I420; "i420" itself is an unknown format), "yv12", "yuyv", "yvyu", "uyvy", or an 8-bit Bayer mosaic
        "bayer_rggb", "bayer_bggr", "bayer_grbg" or "bayer_gbrg" (w and h even and at least 4), or one of those four with
        "16" (10 to 16 bits in a little-endian 16-bit container), "10p" or "12p" (MIPI RAW10 / RAW12 packed rows; "10p": w a
        multiple of 4) behind it.  `develop` (a `Develop`, a uint8 [3, 2^bits] array, or None for the format's default) gives
        a Bayer format its per-colour tables: black and white level, white balance, tone curve (`set_develop`; every format
        change resets them to the default).  Raw frames cross PCIe as
        they are and are converted to BGR on the GPU behind their copy.  The ring is freed here and
        allocated again by the next `host_ring()`: an array that call returned earlier must not be touched any more.
        "mjpeg": a slot holds one baseline JPEG stream (a Motion-JPEG frame) of up to `slot_bytes` bytes (default w * h / 2,
        rounded up to 256), its length goes into `jpeg_lengths()`, and `submit` copies only the used bytes and decodes them on
        the GPU into the BGR frames (include/cbv.h, CBV_FMT_MJPEG).  `planes` (False, True = "444", "444", "422", "420" or
        "gray": the largest chroma sampling the streams may have) makes "mjpeg" a raw format: on a pipeline configured with
        `enhance=False` or `enhance="profile", raw=True` the decode stops at the planes, no BGR frame is written, and the warp
        samples the planes with the same bytes as a result (include/cbv.h, cbv_pipeline_set_jpeg_planes).
        `colorspace` of a YUV format: "bt601" (default; cv2's BT.601 limited range: a UVC webcam's YUYV), "bt601-full" (JFIF:
        phone cameras, full-range UVC modes), "bt709" (decoded video at 720p and above) or "bt709-full" (capture cards in
        PC range).  It is stored with the ring's format (`input_colorspace`) and honoured wherever the ring's frames are
        converted: `submit`, raw mode, `color_sweep`, attached boards, `set_lens`.  ValueError for an unknown name, and
        for another colour space than "bt601" with a format that is not YUV."""
        bits = N.colorspace_bits(colorspace, fmt)
        if isinstance(fmt, str) and fmt.lower() == "mjpeg":
            self.ctx.check(self.ctx.lib.cbv_pipeline_set_jpeg_planes(self.h_, N.jpeg_planes_id(planes)))
            if slot_bytes is not None:
                self.ctx.check(self.ctx.lib.cbv_pipeline_set_jpeg_slot_bytes(self.h_, int(slot_bytes)))
            self.ctx.check(self.ctx.lib.cbv_pipeline_set_input_format(self.h_, N.FMT_MJPEG))
            self.input_format, self.input_colorspace = "mjpeg", "bt601"
            return
        if slot_bytes is not None:
            raise ValueError("slot_bytes belongs to the \"mjpeg\" format")
        if N.jpeg_planes_id(planes):
            raise ValueError("planes belongs to the \"mjpeg\" format")
        if develop is not None and not N.is_bayer(fmt):
            raise ValueError("develop belongs to the Bayer formats, not to %r" % (fmt,))
        tables = develop_tables(develop, N.format_id(fmt)) if develop is not None else None  # (refused before anything changes)
        self.ctx.check(self.ctx.lib.cbv_pipeline_set_input_format(self.h_, N.format_id(fmt) | bits))
        self.input_format, self.input_colorspace, self.develop = fmt.lower(), colorspace.lower(), None
        if tables is not None:
            self.set_develop(develop)

    def host_ring(self):
        """Pinned host mirror of the frame ring as a numpy array: the capture side writes frames here, `submit` copies
        them to the GPU asynchronously.  [max_frames, h, w, 3] for BGR; [max_frames, h * 3 // 2, w] for the 4:2:0 layouts
        (luma rows, then the chroma rows of NV12 / NV21, or the two chroma planes of yuv420p / yv12 back to back, each
        h // 2 rows of w // 2 bytes); [max_frames, h, w, 2] for YUYV, YVYU and UYVY; [max_frames, h, w] for the Bayer
        mosaics (uint16 for "...16"; uint8 [max_frames, h, w * 5 // 4] for "...10p" and [max_frames, h, w * 3 // 2] for "...12p"); [max_frames, slot_bytes] for "mjpeg" (`set_input_format`)."""
        ptr = self.ctx.lib.cbv_pipeline_host_ring(self.h_)
        if not ptr:
            raise RuntimeError(self.ctx.lib.cbv_last_error(self.ctx.h).decode())
        fs = self.ctx.lib.cbv_pipeline_host_slot_bytes(self.h_)  # slots are 256-byte aligned in both rings
        buf = (C.c_uint8 * (fs * self.max_frames)).from_address(ptr)
        flat = np.frombuffer(buf, dtype=np.uint8)
        w, h = self.w, self.h
        if self.input_format == "mjpeg":
            return flat.reshape(self.max_frames, fs)
        if self.input_format == "bgr":
            shape, strides = (h, w, 3), (w * 3, 3, 1)
        elif self.input_format in N.FORMATS_420:
            shape, strides = (h * 3 // 2, w), (w, 1)
        elif self.input_format in N.BAYER_FORMATS:
            shape, strides = (h, w), (w, 1)
        elif self.input_format in N.BAYER_DEEP_FORMATS:  # [h, w] uint16, or the packed rows as bytes
            fid = N.format_id(self.input_format)
            rb = N.bayer_row_bytes(fid, w)
            if fid & N.BAYER_ENC_MASK == N.BAYER_16:
                ring = np.frombuffer(buf, dtype=np.uint16)
                return np.lib.stride_tricks.as_strided(ring, shape=(self.max_frames, h, w), strides=(fs, rb, 2))
            shape, strides = (h, rb), (rb, 1)
        else:
            shape, strides = (h, w, 2), (w * 2, 2, 1)
        return np.lib.stride_tricks.as_strided(flat, shape=(self.max_frames,) + shape, strides=(fs,) + strides)

    def jpeg_lengths(self):
        """The pinned uint32 [max_frames] array of the streams' lengths in the "mjpeg" host ring; the capture side fills it."""
        ptr = self.ctx.lib.cbv_pipeline_host_jpeg_lengths(self.h_)
        if not ptr:
            raise RuntimeError("the pipeline's input format was never \"mjpeg\"")
        return np.frombuffer((C.c_uint32 * self.max_frames).from_address(ptr), dtype=np.uint32)

    @property
    def jpeg_planes(self):
        """The planes mode of the "mjpeg" format (`set_input_format`): "off", "gray", "420", "422" or "444"."""
        n = self.ctx.lib.cbv_pipeline_jpeg_planes(self.h_)
        if n < 0:
            self.ctx.check(n)
        return {v: k for k, v in N.JPEG_PLANES.items()}[n]

    def jpeg_status(self, slot0, count):
        """The status words of the streams last decoded into the slots (0, or _native.JPEG_BAD_CODE | JPEG_NO_DATA |
        JPEG_RESTART for damaged entropy data, which decodes as far as it goes); waits for the submitted decodes."""
        out = np.zeros(count, np.int32)
        self.ctx.check(self.ctx.lib.cbv_pipeline_jpeg_status(self.h_, slot0, count, N.ptr(out)))
        return out

    def set_jpeg_entropy(self, mode, piece_bytes=0):
        """The entropy path of the "mjpeg" decodes: "auto" (pieces for streams without DRI, restart intervals otherwise; the
        default), "interval", "pieces" or "segments" (the piece path for every stream, restart intervals cut into pieces), and
        the piece size in bytes (0: the library's default, otherwise a multiple of 4).  The frames do not depend on either
        (include/cbv.h).  Call between runs."""
        self.ctx.check(self.ctx.lib.cbv_pipeline_set_jpeg_entropy(self.h_, N.JPEG_ENTROPY[mode], int(piece_bytes)))

    def set_jpeg_depth(self, n):
        """How many frames an "mjpeg" submit decodes per launch through one set of scratch buffers (1 to 64, default 8): device
        memory for throughput (include/cbv.h, cbv_pipeline_set_jpeg_depth).  The frames do not depend on it.  Call between runs."""
        self.ctx.check(self.ctx.lib.cbv_pipeline_set_jpeg_depth(self.h_, int(n)))

    @property
    def jpeg_depth(self):
        n = self.ctx.lib.cbv_pipeline_jpeg_depth(self.h_)
        if n < 0:
            self.ctx.check(n)
        return n

    def jpeg_stats(self, slot0, count):
        """The piece path's figures of the streams last decoded into the slots: a [count, 3] uint32 array of pieces, rounds and
        settled_round0 (zeros for a stream decoded by restart interval); waits for the submitted decodes."""
        out = np.zeros((count, 3), np.uint32)
        self.ctx.check(self.ctx.lib.cbv_pipeline_jpeg_stats(self.h_, slot0, count, N.ptr(out)))
        return out

    def submit(self, slot0, count):
        """Enqueue host ring -> device ring for the slots; run() of those slots waits for the copy."""
        self.ctx.check(self.ctx.lib.cbv_pipeline_submit(self.h_, slot0, count))

    def wait_submitted(self):
        """Block until every submitted copy has left the host ring (runs stay in flight); the ring may be rewritten."""
        self.ctx.check(self.ctx.lib.cbv_pipeline_wait_submitted(self.h_))

    def synth(self, slot0, count, stream_id=0, frame0=0, scene="normal", frames_per_ply=32, points=None):
        """Fill slots with synthetic frames of stream `stream_id`, frame indices
        frame0.. (scripted game, one ply every `frames_per_ply` frames)."""
        pts = points if points is not None else S.scaled_corners(self.w, self.h)
        Hinv = np.ascontiguousarray(get_perspective_transform(pts, S.BOARD_UNIT_QUAD).reshape(9))
        seeds = np.array([S.frame_seed(stream_id, frame0 + i) for i in range(count)], dtype=np.uint64)
        boards = np.concatenate([S.board_array(S.position_for_frame(frame0 + i, frames_per_ply)) for i in range(count)])
        boards = np.ascontiguousarray(boards, dtype=np.uint8)
        sc = N.Scene.from_dict(S.SCENES[scene]) if isinstance(scene, str) else scene
        self.ctx.check(self.ctx.lib.cbv_pipeline_synth(self.h_, slot0, count, N.ptr(seeds), N.ptr(Hinv), N.ptr(boards), sc))

    def run(self, slot0, count):
        """Asynchronous on the context's stream."""
        self.ctx.check(self.ctx.lib.cbv_pipeline_run(self.h_, slot0, count))


class Board(_BoardMethods):
    """A board attached to a BoardPipeline (BoardPipeline.add_board): the per-board methods of BoardPipeline on its own
    state.  It keeps its pipeline alive; `close` detaches it (the pipeline and its other boards go on unchanged)."""

    def __init__(self, pipeline, points, grid_lines=None, rot180=False, display_size=(1280, 720), margin=100, **detector):
        if not pipeline.h_:
            raise RuntimeError("the pipeline is closed")
        self.pipeline, self.ctx = pipeline, pipeline.ctx
        self.w, self.h, self.max_frames = pipeline.w, pipeline.h, pipeline.max_frames
        cfg = N.BoardConfig()
        unknown = set(detector) - set(DETECTOR_DEFAULTS)
        if unknown:
            raise TypeError("add_board: unknown detector keyword(s) %s" % ", ".join(sorted(unknown)))
        # (the points are seen through the pipeline's lens, the camera's)
        self.board_size, self.matrix, self.rois_rc = _fill_board(cfg, points, grid_lines, rot180, display_size, margin,
                                                                 lens=getattr(pipeline, "lens", None), **dict(DETECTOR_DEFAULTS, **detector))
        hdl = C.c_void_p()
        self.ctx.check(self.ctx.lib.cbv_pipeline_add_board(pipeline.h_, cfg, C.byref(hdl)))
        self.h_ = hdl
        self._cfg = cfg
        pipeline._boards.append(self)

    def close(self):
        if self.h_:
            self.ctx.lib.cbv_pipeline_destroy(self.h_)
            self.h_ = None
            self.pipeline._boards.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def jpeg_plane_slot_bytes(w, h, planes):
    """Bytes of one slot of the plane ring of a w x h "mjpeg" pipeline in planes mode `planes` (`set_input_format`): the
    largest plane_elems among the samplings the mode admits, rounded up to 256; 0 for off (include/cbv.h,
    cbv_jpeg_plane_slot_bytes).  Needs no GPU."""
    return int(N.load().cbv_jpeg_plane_slot_bytes(int(w), int(h), N.jpeg_planes_id(planes)))
