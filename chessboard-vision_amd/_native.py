"""ctypes binding of libcbv_hip.so (include/cbv.h).

There is no CPU fallback.  `load()` raises ImportError when the shared library
is missing; `context()` raises ImportError when no gfx950 device can be
opened.  ImportError is what the reference's own plugin selector catches to
fall back to its Python classes (frame_enhancer.py:13-21,
change_detector.py:12-19), so a host without an MI355X keeps working exactly
as it does today with a missing Cython extension.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libcbv_hip.so")

CBV_OK = 0
MAX_SQUARES = 64


class ColorProfile(C.Structure):
    _fields_ = [("hue_shift", C.c_double), ("sat_scale", C.c_double), ("val_scale", C.c_double),
                ("contrast", C.c_double), ("brightness", C.c_double), ("radical_mode", C.c_int32),
                ("target_hue", C.c_double), ("hue_window", C.c_double), ("enabled", C.c_int32)]

    @classmethod
    def from_dict(cls, d):
        """Defaults of ImageEnhancer.apply_color_profile (frame_enhancer.py:61-68);
        a falsy profile is the no-op `{}` case (frame_enhancer.py:57-58)."""
        p = cls()
        p.enabled = 1 if d else 0
        d = d or {}
        p.hue_shift = d.get("hue_shift", 0)
        p.sat_scale = d.get("sat_scale", 1.0)
        p.val_scale = d.get("val_scale", 1.0)
        p.contrast = d.get("contrast", 1.0)
        p.brightness = d.get("brightness", 0)
        p.radical_mode = 1 if d.get("radical_mode", 0) else 0
        p.target_hue = d.get("target_hue", 0)
        p.hue_window = d.get("hue_window", 20)
        return p


class LensStruct(C.Structure):
    """cbv_lens: OpenCV's camera matrix and five distortion coefficients (stream.Lens is the Python face of it)."""
    _fields_ = [("enabled", C.c_int32), ("pad", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("k1", C.c_double), ("k2", C.c_double), ("p1", C.c_double), ("p2", C.c_double), ("k3", C.c_double)]


class EnhanceParams(C.Structure):
    _fields_ = [("profile", ColorProfile), ("clahe_clip_limit", C.c_double), ("tiles_x", C.c_int32),
                ("tiles_y", C.c_int32), ("bilateral_d", C.c_int32), ("sigma_color", C.c_double),
                ("sigma_space", C.c_double), ("sharpen_kernel", C.c_float * 9)]


class Roi(C.Structure):
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32)]


class SquareView(C.Structure):
    _fields_ = [("data", C.c_void_p), ("w", C.c_int32), ("h", C.c_int32), ("stride", C.c_int32), ("cn", C.c_int32)]


class SqStats(C.Structure):
    _fields_ = [("n", C.c_uint32), ("sum", C.c_uint32), ("sumsq", C.c_uint32), ("sad_ref", C.c_uint32),
                ("center_sum", C.c_uint32), ("center_cnt", C.c_uint32), ("border_sum", C.c_uint32),
                ("border_cnt", C.c_uint32), ("ring_sum", C.c_uint32 * 4), ("ring_cnt", C.c_uint32 * 4),
                ("z_count", C.c_uint32), ("z_max", C.c_float)]


class Scene(C.Structure):
    _fields_ = [("bg_lo", C.c_uint8), ("bg_span", C.c_uint8), ("light", C.c_uint8 * 3), ("dark", C.c_uint8 * 3),
                ("white", C.c_uint8 * 3), ("black", C.c_uint8 * 3), ("noise", C.c_uint8), ("pad", C.c_uint8 * 3),
                ("radius", C.c_double)]

    @classmethod
    def from_dict(cls, d):
        s = cls()
        s.bg_lo, s.bg_span, s.noise, s.radius = d["bg_lo"], d["bg_span"], d["noise"], d["radius"]
        for k in ("light", "dark", "white", "black"):
            for i in range(3):
                getattr(s, k)[i] = d[k][i]
        return s


class HoughParams(C.Structure):
    _fields_ = [("dp", C.c_double), ("param1", C.c_double), ("param2", C.c_double), ("min_radius_ratio", C.c_double),
                ("max_radius_ratio", C.c_double)]


HOUGH_KEEP = 6
HOUGH_OVERFLOW, HOUGH_SKIPPED = 1, 2


class HoughResult(C.Structure):
    _fields_ = [("found", C.c_uint8), ("kind", C.c_uint8), ("n_circles", C.c_uint16), ("cx", C.c_float), ("cy", C.c_float),
                ("r", C.c_float), ("votes", C.c_int32), ("n_edges", C.c_uint32), ("n_centres", C.c_uint16),
                ("flags", C.c_uint16), ("circles", (C.c_float * 4) * HOUGH_KEEP)]


class HostImage(C.Structure):
    _fields_ = [("data", C.c_void_p), ("w", C.c_int32), ("h", C.c_int32), ("stride", C.c_int32), ("cn", C.c_int32)]


METHOD_NAMES = (None, "hough", "tower_top", "center_diff", "symmetry")


class PieceResult(C.Structure):
    _fields_ = [("has_piece", C.c_uint8), ("method", C.c_uint8), ("changed", C.c_uint8), ("should_process", C.c_uint8),
                ("evaluated", C.c_uint8), ("pad", C.c_uint8 * 3), ("cx", C.c_int32), ("cy", C.c_int32), ("radius", C.c_int32),
                ("confidence", C.c_double), ("center_border_diff", C.c_double)]


class DetectParams(C.Structure):
    _fields_ = [("change_threshold", C.c_double), ("circle_threshold", C.c_double), ("hough", HoughParams),
                ("has_ref", C.c_uint64), ("cached", C.c_uint64), ("check", C.c_uint64), ("check_given", C.c_int32),
                ("use_delta", C.c_int32)]


class ChangeParams(C.Structure):
    _fields_ = [("z_threshold", C.c_double), ("select", C.c_uint64), ("circle_threshold", C.c_double), ("hough", HoughParams)]


class ChangeResult(C.Structure):
    _fields_ = [("in_result", C.c_uint8), ("intensity", C.c_uint8), ("is_circular", C.c_uint8), ("pad", C.c_uint8),
                ("z_max", C.c_float), ("z_count", C.c_uint32), ("n", C.c_uint32)]


def record_dtype(struct, skip=("pad",)):
    """numpy dtype with the layout of a ctypes Structure (padding fields left out): an array of it is filled by the
    library in place and `.tolist()` turns all records into Python scalars in one call."""
    names = [n for n, _ in struct._fields_ if n not in skip]
    return np.dtype({"names": names, "formats": [np.dtype(dict(struct._fields_)[n]) for n in names],
                     "offsets": [getattr(struct, n).offset for n in names], "itemsize": C.sizeof(struct)})


class PipelineConfig(C.Structure):
    _fields_ = [("enhance", EnhanceParams), ("M", C.c_double * 9), ("board_size", C.c_int32), ("rot180", C.c_int32),
                ("n_rois", C.c_int32), ("rois", Roi * MAX_SQUARES), ("history_size", C.c_int32),
                ("min_presence", C.c_double), ("change_threshold", C.c_double), ("chunk", C.c_int32),
                ("lanes", C.c_int32), ("z_threshold", C.c_double), ("initial_variance", C.c_double), ("keep_enhanced", C.c_int32),
                ("use_hough", C.c_int32), ("hough", HoughParams), ("enhance_region", C.c_int32), ("skip_enhance", C.c_int32)]


class BoardConfig(C.Structure):
    """cbv_board_config: the per-board subset of cbv_pipeline_config (cbv_pipeline_add_board)."""
    _fields_ = [("M", C.c_double * 9), ("board_size", C.c_int32), ("rot180", C.c_int32), ("n_rois", C.c_int32),
                ("rois", Roi * MAX_SQUARES), ("history_size", C.c_int32), ("min_presence", C.c_double),
                ("change_threshold", C.c_double), ("z_threshold", C.c_double), ("initial_variance", C.c_double),
                ("use_hough", C.c_int32), ("hough", HoughParams)]


MAX_BOARDS = 8


class FrameResult(C.Structure):
    _fields_ = [("raw_occupied", C.c_uint64), ("stable_occupied", C.c_uint64), ("visual_changes", C.c_uint64),
                ("processed", C.c_uint64), ("changed", C.c_uint64), ("parcial", C.c_uint64), ("total", C.c_uint64),
                ("circular", C.c_uint64)]


class NoiseResult(C.Structure):
    _fields_ = [("state", C.c_uint8), ("msg", C.c_uint8), ("stable", C.c_uint8), ("lifted", C.c_int8),
                ("count", C.c_uint16), ("blocked", C.c_uint16), ("squares", C.c_uint64)]


class NoiseDevState(C.Structure):
    _fields_ = [("state", C.c_uint32), ("stable_count", C.c_uint32), ("cooldown_count", C.c_uint32),
                ("lifted", C.c_int32), ("pending", C.c_uint64)]


class SessionConfig(C.Structure):
    """cbv_session_config: the game session of a board (include/cbv.h)."""
    _fields_ = [("rule", C.c_int32), ("stability_required", C.c_int32), ("cooldown_frames", C.c_int32),
                ("scan_period", C.c_int32), ("max_diff", C.c_int32), ("smart_scan", C.c_int32),
                ("online", C.c_int32), ("radar", C.c_int32), ("tone", C.c_int32)]


class SessionMove(C.Structure):
    _fields_ = [("frame", C.c_int32), ("move", C.c_uint16), ("status", C.c_uint8), ("candidates", C.c_uint8)]


class SessionState(C.Structure):
    _fields_ = [("sq", C.c_int8 * 64), ("turn", C.c_int32), ("castling", C.c_int32), ("ep", C.c_int32),
                ("halfmove", C.c_int32), ("fullmove", C.c_int32), ("expected", C.c_uint64), ("smart_mask", C.c_uint64),
                ("stable_occupancy", C.c_uint64), ("rejected", C.c_uint64), ("rejected_valid", C.c_int32),
                ("stable_count", C.c_int32), ("c", C.c_int32), ("last_move_c", C.c_int32), ("n_moves", C.c_int32),
                ("last_candidates", C.c_int32), ("waiting_for_opponent", C.c_int32), ("ignored_move", C.c_int32),
                ("ignored_frame", C.c_int32), ("n_ignored", C.c_int32)]


class SessionPos(C.Structure):
    """cbv_session_pos: the board part of a SessionState."""
    _fields_ = [("sq", C.c_int8 * 64), ("turn", C.c_int32), ("castling", C.c_int32), ("ep", C.c_int32),
                ("halfmove", C.c_int32), ("fullmove", C.c_int32)]


class SessionEvent(C.Structure):
    _fields_ = [("at_frame", C.c_int32), ("waiting_for_opponent", C.c_int32), ("pos", SessionPos)]


class SessionRadar(C.Structure):
    _fields_ = [("lifted", C.c_int8), ("destinations", C.c_uint64)]


class ToneSums(C.Structure):
    """cbv_tone_sums: the B, G, R sums and the pixel count of a square's centre disc."""
    _fields_ = [("sum", C.c_uint32 * 3), ("cnt", C.c_uint32)]


class ToneModel(C.Structure):
    """cbv_tone_model: centroid[light, dark][white piece, black piece][b, g, r], the dead zone's margin."""
    _fields_ = [("centroid", ((C.c_double * 3) * 2) * 2), ("margin", C.c_double), ("calibrated", C.c_int32), ("pad", C.c_int32)]


class ToneResult(C.Structure):
    _fields_ = [("white", C.c_uint64), ("black", C.c_uint64)]


class ToneReport(C.Structure):
    _fields_ = [("samples", (C.c_int32 * 2) * 2), ("D", C.c_double * 2), ("misclassified", C.c_uint64), ("undecided", C.c_uint64)]


class SweepSetting(C.Structure):
    """cbv_sweep_setting: one trackbar position of calibrate_sensitivity.py (cbv_pipeline_sweep)."""
    _fields_ = [("z_threshold", C.c_double), ("initial_variance", C.c_double), ("blur_kernel", C.c_int32), ("pad", C.c_int32)]


class SweepRecord(C.Structure):
    _fields_ = [("changed", C.c_uint64), ("parcial", C.c_uint64), ("total", C.c_uint64), ("z_max", C.c_float),
                ("n_changed", C.c_uint8), ("n_total", C.c_uint8), ("flags", C.c_uint8), ("lifted", C.c_int8)]


class SweepSummary(C.Structure):
    _fields_ = [("frames_changed", C.c_uint32), ("frames_hand", C.c_uint32), ("frames_move", C.c_uint32),
                ("frames_lifted", C.c_uint32), ("squares_reported", C.c_uint32), ("z_max", C.c_float)]


class SweepInfo(C.Structure):
    _fields_ = [("planes_ms", C.c_float), ("hist_ms", C.c_float), ("eval_ms", C.c_float), ("kernels_distinct", C.c_int32),
                ("chunk_frames", C.c_int32)]


class PieceSweepRecord(C.Structure):
    """cbv_piece_sweep_record: one (setting, frame) of cbv_pipeline_piece_sweep."""
    _fields_ = [("raw_occupied", C.c_uint64), ("stable_occupied", C.c_uint64), ("hough", C.c_uint64), ("tower_top", C.c_uint64),
                ("center_diff", C.c_uint64), ("symmetry", C.c_uint64), ("r_min", C.c_int16), ("r_max", C.c_int16),
                ("n_raw", C.c_uint8), ("n_stable", C.c_uint8), ("flags", C.c_uint8), ("pad", C.c_uint8)]


class PieceSweepSummary(C.Structure):
    _fields_ = [("frames", C.c_uint32), ("frames_exact", C.c_uint32), ("missed", C.c_uint32), ("false_pos", C.c_uint32),
                ("n_hough", C.c_uint32), ("n_tower_top", C.c_uint32), ("n_center_diff", C.c_uint32), ("n_symmetry", C.c_uint32),
                ("r_min", C.c_int32), ("r_max", C.c_int32), ("n_r", C.c_uint32), ("overflow", C.c_uint32), ("r_sum", C.c_uint64)]


class PieceSweepInfo(C.Structure):
    _fields_ = [("hough_ms", C.c_float), ("eval_ms", C.c_float), ("param1_distinct", C.c_int32), ("chunk_frames", C.c_int32)]


class ColorSweepInfo(C.Structure):
    """cbv_color_sweep_info: GPU time of the four stages of cbv_pipeline_color_sweep and the chunk sizes used."""
    _fields_ = [("warp_ms", C.c_float), ("squares_ms", C.c_float), ("hough_ms", C.c_float), ("eval_ms", C.c_float),
                ("chunk_frames", C.c_int32), ("chunk_profiles", C.c_int32)]


COLOR_SWEEP_MAX_PROFILES = 65536
SKIP_ENHANCE_PROFILE = 2  # cbv_pipeline_config::skip_enhance: the colour profile only (CBV_SKIP_ENHANCE_PROFILE)
SKIP_ENHANCE_PROFILE_RAW = 3  # ... and camera-native frames are sampled as they are (CBV_SKIP_ENHANCE_PROFILE_RAW)


class PieceChoice(C.Structure):
    """What k_piece_sweep_hough leaves per (setting, frame, square); cbv_piece_sweep_eval_host reads arrays of it."""
    _fields_ = [("kind", C.c_uint8), ("flags", C.c_uint8), ("r", C.c_int16), ("cx", C.c_int16), ("cy", C.c_int16)]


PIECE_SWEEP_OVERFLOW, PIECE_SWEEP_MAX_SETTINGS = 1, 65536
SWEEP_HAND, SWEEP_MOVE = 1, 2
SWEEP_MAX_SETTINGS, SWEEP_MAX_CHUNK, SWEEP_DEFAULT_CHUNK = 65536, 64, 16

SESSION_RULES = {"session": 0, "game_state": 1}
SESSION_RING = 1024
SESSION_ONLINE = {None: 0, "white": 1, "black": 2}
SESSION_EVENTS = 64


class RawFrame(C.Structure):
    """cbv_raw_frame: one camera-native frame in host memory (stride2 / plane2: the three-plane formats only)."""
    _fields_ = [("fmt", C.c_int32), ("stride0", C.c_int32), ("stride1", C.c_int32), ("stride2", C.c_int32), ("plane0", C.c_void_p),
                ("plane1", C.c_void_p), ("plane2", C.c_void_p)]


# The ids are bit fields (include/cbv.h): low nibble 1 = 4:2:0, 2 = packed 4:2:2; 0x10 = V before U; 0x20 = planar chroma
# (4:2:0) or chroma-first bytes (4:2:2).  The three-plane format is "yuv420p", libav's name: "i420" is NOT a name here.
FMT_BGR, FMT_NV12, FMT_YUYV = 0, 1, 2
FMT_NV21, FMT_YUV420P, FMT_YV12, FMT_YVYU, FMT_UYVY = 0x11, 0x21, 0x31, 0x12, 0x22
FORMATS = {"bgr": FMT_BGR, "nv12": FMT_NV12, "yuyv": FMT_YUYV, "nv21": FMT_NV21, "yuv420p": FMT_YUV420P, "yv12": FMT_YV12,
           "yvyu": FMT_YVYU, "uyvy": FMT_UYVY}
FORMATS_420 = ("nv12", "nv21", "yuv420p", "yv12")      # ring slots [h * 3 // 2, w]
FORMATS_422 = ("yuyv", "yvyu", "uyvy")                 # ring slots [h, w, 2]
# 8-bit Bayer mosaics, named by their top-left 2 x 2 block read row by row (cv2 names its codes by the block at (1, 1):
# "bayer_rggb" is COLOR_BayerBG2BGR).  Low nibble 4 = the family; 0x10 = blue where RGGB has red; 0x20 = rows start with green.
# A table of its own: FORMATS stays the BGR and YUV formats.
FMT_BAYER_RGGB, FMT_BAYER_BGGR, FMT_BAYER_GRBG, FMT_BAYER_GBRG = 0x04, 0x14, 0x24, 0x34
BAYER_FORMATS = {"bayer_rggb": FMT_BAYER_RGGB, "bayer_bggr": FMT_BAYER_BGGR, "bayer_grbg": FMT_BAYER_GRBG,
                 "bayer_gbrg": FMT_BAYER_GBRG}                 # ring slots [h, w]
# Sample encodings of more than 8 bits (include/cbv.h, "developed mosaics"): a field OR-ed onto a layout's id, a suffix on its
# name.  "16": a little-endian 16-bit container holding 10, 12, 14 or 16 bits (V4L2 SRGGB10 / 12 / 14 / 16, libav
# bayer_rggb16le); "10p" / "12p": MIPI RAW10 / RAW12 packed rows (V4L2 SRGGB10P / SRGGB12P).  A table of its own again:
# BAYER_FORMATS stays the 8-bit mosaics.
BAYER_16, BAYER_10P, BAYER_12P, BAYER_ENC_MASK = 0x1000, 0x2000, 0x3000, 0xF000
BAYER_ENCODINGS = {"16": BAYER_16, "10p": BAYER_10P, "12p": BAYER_12P}
BAYER_DEEP_FORMATS = {name + suffix: fid | enc for name, fid in BAYER_FORMATS.items() for suffix, enc in BAYER_ENCODINGS.items()}
BAYER_TABLE_BITS = {0: (8,), BAYER_16: (10, 12, 14, 16), BAYER_10P: (10,), BAYER_12P: (12,)}  # the bits an encoding's tables may have
BAYER_DEFAULT_BITS = {0: 0, BAYER_16: 16, BAYER_10P: 10, BAYER_12P: 12}                       # ... and its default table's (0: none)


def bayer_row_bytes(fmt_id, w):
    """Bytes of a row of w samples of a Bayer id."""
    enc = fmt_id & BAYER_ENC_MASK
    return {0: w, BAYER_16: 2 * w, BAYER_10P: w // 4 * 5, BAYER_12P: w // 2 * 3}[enc]


def is_bayer(fmt):
    """`fmt` names a Bayer mosaic of any encoding."""
    return isinstance(fmt, str) and (fmt.lower() in BAYER_FORMATS or fmt.lower() in BAYER_DEEP_FORMATS)


def neutral_tables(bits):
    """The neutral tables of `bits` bits, uint8 [3, 2^bits]: v * 255 / M rounded half up, M = 2^bits - 1, for every colour."""
    m = (1 << bits) - 1
    v = np.arange(m + 1, dtype=np.int64)
    return np.repeat(((510 * v + m) // (2 * m)).astype(np.uint8)[None], 3, axis=0)

# The colour space of a YUV frame travels in its format id (include/cbv.h): CBV_CS_* bits OR-ed onto a YUV id.  "bt601" is
# cv2.cvtColor's BT.601 limited range, the default and all there was; "bt601-full" is JFIF (phone cameras, full-range UVC
# modes), "bt709" decoded video at 720p and above, "bt709-full" capture cards in PC range.
CS_FULL, CS_BT709, CS_MASK = 0x400, 0x800, 0xC00
COLORSPACES = {"bt601": 0, "bt601-full": CS_FULL, "bt709": CS_BT709, "bt709-full": CS_BT709 | CS_FULL}


def colorspace_bits(colorspace, fmt):
    """CBV_CS_* bits of a colour space name for frames of format `fmt` (a name).  ValueError for an unknown name and for a
    colour space other than "bt601" with a format that is not YUV (BGR, Bayer, Motion-JPEG)."""
    try:
        bits = COLORSPACES[colorspace.lower()]
    except (KeyError, AttributeError):
        raise ValueError("unknown colour space %r (expected one of %s)" % (colorspace, ", ".join(COLORSPACES)))
    name = fmt.lower() if isinstance(fmt, str) else fmt
    if bits and (name == "bgr" or name not in FORMATS):
        raise ValueError("colour space %r goes with the YUV formats (%s), not with %r" % (colorspace, ", ".join(k for k in FORMATS if k != "bgr"), fmt))
    return bits


# cbv_pipeline_set_jpeg_planes: the largest sampling a slot of the plane ring holds (gray < 4:2:0 < 4:2:2 < 4:4:4)
JPEG_PLANES = {"off": 0, "gray": 1, "420": 2, "422": 3, "444": 4}


def jpeg_planes_id(planes):
    """False / None -> off, True -> "444", or one of the names of JPEG_PLANES."""
    if planes is None or planes is False:
        return 0
    if planes is True:
        return JPEG_PLANES["444"]
    if isinstance(planes, str) and planes.lower() in JPEG_PLANES:
        return JPEG_PLANES[planes.lower()]
    raise ValueError("planes %r: False, True (= \"444\"), \"444\", \"422\", \"420\" or \"gray\"" % (planes,))


FMT_MJPEG = 0x08  # one JPEG stream per frame: jpeg_to_bgr, BoardPipeline.set_input_format("mjpeg"); has no raw_frame() layout
JPEG_BAD_CODE, JPEG_NO_DATA, JPEG_RESTART = 1, 2, 4


class JpegInfo(C.Structure):
    _fields_ = [("w", C.c_int32), ("h", C.c_int32), ("components", C.c_int32), ("hs", C.c_int32), ("vs", C.c_int32),
                ("restart_interval", C.c_int32), ("intervals", C.c_int32), ("std_tables", C.c_int32),
                ("entropy_offset", C.c_uint32), ("entropy_length", C.c_uint32), ("plane_elems", C.c_uint32),
                ("blocks_w", C.c_int32 * 3), ("blocks_h", C.c_int32 * 3)]


JPEG_ENTROPY = {"auto": 0, "interval": 1, "pieces": 2, "segments": 4}  # CBV_JPEG_ENTROPY_* (3 is no mode)


class JpegDecodeStats(C.Structure):
    _fields_ = [("pieces", C.c_uint32), ("rounds", C.c_uint32), ("settled_round0", C.c_uint32)]


KERNEL_IDS = ["COLOR_LAB_HIST", "CLAHE_LUT", "CLAHE_APPLY", "BILATERAL", "SHARPEN", "NORM_LUT", "NORMALIZE", "WARP",
              "SQUARES", "GRAY_BLUR", "OTSU", "THRESHOLD", "SCAN", "SYNTH", "RESET", "HOUGH", "INGEST"]
K = {name: i for i, name in enumerate(KERNEL_IDS)}
# Kernels outside the default path (they launch only when a feature is switched on) follow the list above in the
# library's id space (CBV_K_* of include/cbv.h) and are named in K only.
K["MODEL_SCAN"] = len(KERNEL_IDS)
# ... and k_warp_yuv (pipelines without enhancement on raw frames) follows those, under a name of its own
K_WARP_YUV = K["MODEL_SCAN"] + 1
# ... and k_change_blur_stats (boards whose ChangeDetector has a blur kernel of its own, set_change_blur) follows that
K_CHANGE_BLUR = K_WARP_YUV + 1
K_ALL = dict(K, WARP_YUV=K_WARP_YUV, CHANGE_BLUR=K_CHANGE_BLUR)  # every id by name (K itself stays as tests/test_model_update_host.py pins it)
# ... and the kernels of developed mosaics (k_ingest_deep, the warp kernels of k_warp_deep.hip and k_warp_lens_deep.hip) follow
# one id further on: tests/test_change_blur_host.py pins that K_CHANGE_BLUR is K_ALL's last id and that the id behind it has
# no name, so that id stays empty and K_ALL stays as it is.  K_EVERY is every id by name.
K_INGEST_BAYER_DEEP, K_WARP_BAYER_DEEP = K_CHANGE_BLUR + 2, K_CHANGE_BLUR + 3
K_EVERY = dict(K_ALL, INGEST_BAYER_DEEP=K_INGEST_BAYER_DEEP, WARP_BAYER_DEEP=K_WARP_BAYER_DEEP)
# ... and k_piece_tone (piece colour per square: set_tones, tone_sums_image) two ids further on, under a name of its own: the
# id behind K_WARP_BAYER_DEEP stays without a name (tests/test_bayer_deep_host.py pins that), and K_EVERY stays as it is
K_TONE = K_WARP_BAYER_DEEP + 2

MODEL_FROZEN, MODEL_EVERY, MODEL_UNCHANGED = 0, 1, 2
MODEL_MODES = {"frozen": MODEL_FROZEN, "every": MODEL_EVERY, "unchanged": MODEL_UNCHANGED}

_lib = None


def load():
    """dlopen libcbv_hip.so and declare prototypes.  ImportError if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("chessboard_vision_amd: %s not built (run `python -m chessboard_vision_amd.build`); "
                          "there is no CPU fallback" % LIB_PATH)
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # e.g. ROCm runtime missing
        raise ImportError("chessboard_vision_amd: cannot load %s: %s" % (LIB_PATH, e))
    vp, i32, dbl, u8p = C.c_void_p, C.c_int, C.c_double, C.c_void_p
    P = C.POINTER
    proto = {
        "cbv_device_count": (i32, []),
        "cbv_ctx_create": (i32, [i32, P(vp)]),
        "cbv_ctx_destroy": (None, [vp]),
        "cbv_last_error": (C.c_char_p, [vp]),
        "cbv_ctx_set_stream": (i32, [vp, vp]),
        "cbv_ctx_synchronize": (i32, [vp]),
        "cbv_device_name": (C.c_char_p, [vp]),
        "cbv_profile_enable": (i32, [vp, i32]),
        "cbv_profile_read": (i32, [vp, i32, P(dbl), P(C.c_longlong)]),
        "cbv_profile_reset": (i32, [vp]),
        "cbv_kernel_name": (C.c_char_p, [i32]),
        "cbv_apply_color_profile": (i32, [vp, u8p, i32, i32, i32, P(ColorProfile), u8p, i32]),
        "cbv_correct_lighting": (i32, [vp, u8p, i32, i32, i32, dbl, i32, i32, u8p, i32]),
        "cbv_clahe_apply": (i32, [vp, u8p, i32, i32, i32, dbl, i32, i32, u8p, i32]),
        "cbv_reduce_noise": (i32, [vp, u8p, i32, i32, i32, i32, dbl, dbl, u8p, i32]),
        "cbv_sharpen": (i32, [vp, u8p, i32, i32, i32, vp, u8p, i32]),
        "cbv_normalize_intensity": (i32, [vp, u8p, i32, i32, i32, u8p, i32]),
        "cbv_prepare_analysis": (i32, [vp, u8p, i32, i32, i32, u8p, i32, u8p, i32, P(i32)]),
        "cbv_process_pipeline": (i32, [vp, u8p, i32, i32, i32, P(EnhanceParams), u8p, i32]),
        "cbv_get_perspective_transform": (i32, [vp, vp, vp]),
        "cbv_warp_perspective": (i32, [vp, u8p, i32, i32, i32, vp, i32, i32, i32, u8p, i32]),
        "cbv_warp_color_profile": (i32, [vp, u8p, i32, i32, i32, P(ColorProfile), vp, i32, i32, i32, u8p, i32]),
        "cbv_squares_create": (i32, [vp, P(vp)]),
        "cbv_squares_destroy": (None, [vp]),
        "cbv_squares_load": (i32, [vp, P(SquareView), i32, i32]),
        "cbv_squares_load_dev": (i32, [vp, vp, i32, i32, i32, i32, P(Roi), i32, i32]),
        "cbv_squares_calibrate": (i32, [vp, dbl, vp]),
        "cbv_squares_ema": (i32, [vp, dbl, vp]),
        "cbv_squares_set_ref": (i32, [vp, vp]),
        "cbv_squares_stats": (i32, [vp, i32, i32, dbl, P(SqStats)]),
        "cbv_board_corners_from_edges": (i32, [u8p, i32, i32, i32, C.POINTER(C.c_int32), C.POINTER(i32)]),
        "cbv_largest_contour_polygon": (i32, [u8p, i32, i32, i32, dbl, C.POINTER(C.c_int32), i32, C.POINTER(dbl), C.POINTER(i32)]),
        "cbv_find_chessboard_corners": (i32, [vp, u8p, i32, i32, i32, C.POINTER(C.c_int32), u8p, i32]),
        "cbv_canny": (i32, [vp, u8p, i32, i32, i32, i32, dbl, dbl, u8p, i32]),
        "cbv_gaussian_blur": (i32, [vp, u8p, i32, i32, i32, i32, i32, dbl, u8p, i32, P(C.c_int32)]),
        "cbv_gaussian_q8": (i32, [i32, dbl, P(C.c_int32)]),
        "cbv_dilate_rect": (i32, [vp, u8p, i32, i32, i32, i32, u8p, i32]),
        "cbv_external_contours": (i32, [u8p, i32, i32, i32, P(C.c_int32), i32, P(C.c_int32), P(dbl), P(dbl), i32, P(i32), P(i32)]),
        "cbv_approx_poly_closed": (i32, [P(C.c_int32), i32, dbl, P(C.c_int32), i32]),
        "cbv_squares_hough": (i32, [vp, P(HoughParams), P(HoughResult)]),
        "cbv_squares_load_image": (i32, [vp, P(HostImage), P(Roi), i32, i32]),
        "cbv_squares_set_ref_mask": (i32, [vp, C.c_uint64]),
        "cbv_decide_piece": (i32, [P(SqStats), P(HoughResult), i32, i32, dbl, P(PieceResult)]),
        "cbv_np_std_below_15": (i32, [vp, i32, P(C.c_double)]),
        "cbv_squares_detect_all": (i32, [vp, P(HostImage), P(Roi), i32, P(DetectParams), vp]),
        "cbv_squares_detect_changes": (i32, [vp, P(HostImage), P(Roi), i32, i32, P(ChangeParams), vp]),
        "cbv_debug_poison": (i32, [vp, i32]),
        "cbv_debug_bilateral_offsets": (i32, [i32, dbl, dbl]),
        "cbv_debug_bilateral_centre_is_one": (i32, [i32, dbl, dbl]),
        "cbv_debug_reduce_noise_batch": (i32, [vp, u8p, i32, i32, i32, i32, dbl, dbl, u8p]),
        "cbv_squares_get": (i32, [vp, i32, i32, vp]),
        "cbv_squares_set": (i32, [vp, i32, i32, vp]),
        "cbv_squares_geometry": (i32, [vp, i32, P(i32), P(i32)]),
        "cbv_pipeline_create": (i32, [vp, i32, i32, i32, P(vp)]),
        "cbv_pipeline_destroy": (None, [vp]),
        "cbv_pipeline_configure": (i32, [vp, P(PipelineConfig)]),
        "cbv_pipeline_frames_dev": (vp, [vp]),
        "cbv_pipeline_upload": (i32, [vp, i32, u8p, i32]),
        "cbv_pipeline_synth": (i32, [vp, i32, i32, vp, vp, vp, P(Scene)]),
        "cbv_pipeline_reset_state": (i32, [vp]),
        "cbv_pipeline_calibrate": (i32, [vp, i32]),
        "cbv_pipeline_run": (i32, [vp, i32, i32]),
        "cbv_pipeline_results": (i32, [vp, i32, i32, P(FrameResult)]),
        "cbv_pipeline_download": (i32, [vp, i32, i32, u8p]),
        "cbv_pipeline_noise_results": (i32, [vp, i32, i32, P(NoiseResult)]),
        "cbv_noise_run": (i32, [vp, vp, i32, P(NoiseDevState), P(NoiseResult)]),
        "cbv_pipeline_host_ring": (C.c_void_p, [vp]),
        "cbv_pipeline_submit": (i32, [vp, i32, i32]),
        "cbv_pipeline_wait_submitted": (i32, [vp]),
        "cbv_pipeline_update_references": (i32, [vp, i32, i32]),
        "cbv_pipeline_set_check_squares": (i32, [vp, i32, i32, vp]),
        "cbv_pipeline_square_stats": (i32, [vp, i32, P(SqStats)]),
        "cbv_pipeline_hough": (i32, [vp, i32, P(HoughResult)]),
        "cbv_pipeline_add_board": (i32, [vp, P(BoardConfig), P(vp)]),
        "cbv_yuv_to_bgr": (i32, [vp, P(RawFrame), i32, i32, u8p, i32]),
        "cbv_bayer_to_bgr": (i32, [vp, P(RawFrame), i32, i32, u8p, i32, u8p, i32]),
        "cbv_pipeline_set_bayer_tables": (i32, [vp, u8p, i32]),
        "cbv_pipeline_upload_raw": (i32, [vp, i32, P(RawFrame)]),
        "cbv_pipeline_set_input_format": (i32, [vp, i32]),
        "cbv_pipeline_host_slot_bytes": (C.c_size_t, [vp]),
        "cbv_pipeline_set_model_update": (i32, [vp, i32, dbl]),
        "cbv_pipeline_set_change_blur": (i32, [vp, i32]),
        "cbv_pipeline_set_profile": (i32, [vp, P(ColorProfile)]),
        "cbv_warp_color_profile_raw": (i32, [vp, P(RawFrame), i32, i32, P(ColorProfile), vp, i32, i32, i32, u8p, i32]),
        "cbv_pipeline_model": (i32, [vp, i32, i32, vp]),
        "cbv_pipeline_sweep": (i32, [vp, i32, i32, i32, vp, i32, i32, vp, vp, P(SweepInfo)]),
        "cbv_pipeline_change_hist": (i32, [vp, i32, i32, i32, vp]),
        "cbv_sweep_eval_host": (i32, [vp, vp, i32, vp, i32, vp]),
        "cbv_pipeline_piece_sweep": (i32, [vp, i32, i32, vp, i32, vp, i32, vp, vp, P(PieceSweepInfo)]),
        "cbv_pipeline_piece_detail": (i32, [vp, i32, P(HoughParams), vp]),
        "cbv_pipeline_color_sweep": (i32, [vp, i32, i32, vp, i32, vp, i32, vp, vp, P(ColorSweepInfo)]),
        "cbv_piece_sweep_eval_host": (i32, [vp, vp, vp, i32, i32, vp, i32, vp, vp, vp]),
        "cbv_pipeline_session_begin": (i32, [vp, P(SessionConfig), C.c_char_p]),
        "cbv_pipeline_session_end": (i32, [vp]),
        "cbv_pipeline_session_moves": (i32, [vp, P(SessionMove), i32, P(i32)]),
        "cbv_pipeline_session_state": (i32, [vp, P(SessionState)]),
        "cbv_session_walk": (i32, [P(SessionConfig), P(SessionState), P(FrameResult), P(NoiseResult), i32, P(SessionMove), P(i32)]),
        "cbv_session_state_init": (i32, [P(SessionState), C.c_char_p]),
        "cbv_session_state_fen": (i32, [P(SessionState), C.c_char_p, i32]),
        "cbv_session_pos_from_moves": (i32, [C.c_char_p, P(SessionPos), P(i32)]),
        "cbv_pipeline_session_sync": (i32, [vp, i32, P(SessionPos), i32]),
        "cbv_pipeline_session_frames": (i32, [vp, P(i32)]),
        "cbv_pipeline_session_radar": (i32, [vp, i32, i32, P(SessionRadar)]),
        "cbv_session_walk_events": (i32, [P(SessionConfig), P(SessionState), P(FrameResult), P(NoiseResult), i32, P(SessionEvent), i32,
                                          P(i32), P(SessionRadar), P(SessionMove), P(i32)]),
        "cbv_session_state_init_cfg": (i32, [P(SessionState), P(SessionConfig), C.c_char_p]),
        "cbv_session_device_legal_moves": (i32, [vp, C.c_char_p, P(C.c_uint16), i32, P(i32)]),
        "cbv_session_generator_time": (i32, [vp, C.c_char_p, i32, P(dbl)]),
        "cbv_jpeg_probe": (i32, [vp, C.c_size_t, P(JpegInfo)]),
        "cbv_jpeg_decode_host": (i32, [vp, C.c_size_t, u8p, i32, vp, vp, P(C.c_int32)]),
        "cbv_jpeg_decode": (i32, [vp, vp, C.c_size_t, u8p, i32, vp, vp, P(C.c_int32)]),
        "cbv_pipeline_host_jpeg_lengths": (C.c_void_p, [vp]),
        "cbv_pipeline_set_jpeg_slot_bytes": (i32, [vp, C.c_size_t]),
        "cbv_pipeline_upload_jpeg": (i32, [vp, i32, vp, C.c_size_t]),
        "cbv_pipeline_jpeg_status": (i32, [vp, i32, i32, vp]),
        "cbv_jpeg_decode_host_ex": (i32, [vp, C.c_size_t, u8p, i32, vp, vp, P(C.c_int32), i32, C.c_uint32, P(JpegDecodeStats)]),
        "cbv_jpeg_decode_ex": (i32, [vp, vp, C.c_size_t, u8p, i32, vp, vp, P(C.c_int32), i32, C.c_uint32, P(JpegDecodeStats)]),
        "cbv_pipeline_set_jpeg_entropy": (i32, [vp, i32, C.c_uint32]),
        "cbv_pipeline_jpeg_stats": (i32, [vp, i32, i32, vp]),
        "cbv_pipeline_set_jpeg_depth": (i32, [vp, i32]),
        "cbv_pipeline_jpeg_depth": (i32, [vp]),
        "cbv_pipeline_set_jpeg_planes": (i32, [vp, i32]),
        "cbv_pipeline_jpeg_planes": (i32, [vp]),
        "cbv_jpeg_plane_slot_bytes": (C.c_size_t, [i32, i32, i32]),
        "cbv_warp_jpeg": (i32, [vp, vp, C.c_size_t, P(ColorProfile), vp, i32, i32, i32, u8p, i32, P(C.c_int32)]),
        "cbv_lens_distort_points": (i32, [P(LensStruct), vp, i32, vp]),
        "cbv_lens_undistort_points": (i32, [P(LensStruct), vp, i32, vp]),
        "cbv_lens_warp_coords": (i32, [P(LensStruct), vp, i32, i32, vp]),
        "cbv_lens_warp_footprint": (i32, [P(LensStruct), vp, i32, i32, i32, i32, vp]),
        "cbv_warp_lens": (i32, [vp, P(RawFrame), i32, i32, P(ColorProfile), P(LensStruct), vp, i32, i32, i32, u8p, i32]),
        "cbv_warp_jpeg_lens": (i32, [vp, vp, C.c_size_t, P(ColorProfile), P(LensStruct), vp, i32, i32, i32, u8p, i32, P(C.c_int32)]),
        "cbv_pipeline_set_lens": (i32, [vp, P(LensStruct)]),
        "cbv_tone_sums_image": (i32, [vp, P(HostImage), P(Roi), i32, P(ToneSums)]),
        "cbv_tone_calibrate_host": (i32, [P(ToneSums), vp, dbl, P(ToneModel), P(ToneReport)]),
        "cbv_tone_classify_host": (i32, [P(ToneModel), P(ToneSums), i32, P(C.c_uint64), P(C.c_uint64)]),
        "cbv_pipeline_set_tones": (i32, [vp, P(ToneModel)]),
        "cbv_pipeline_tone_sums": (i32, [vp, i32, P(ToneSums)]),
        "cbv_pipeline_tones": (i32, [vp, i32, i32, P(ToneResult)]),
        "cbv_session_walk_tones": (i32, [P(SessionConfig), P(SessionState), P(FrameResult), P(NoiseResult), i32, P(SessionEvent), i32,
                                         P(i32), P(SessionRadar), P(ToneResult), P(SessionMove), P(i32)]),
    }
    for name, (res, args) in proto.items():
        fn = getattr(lib, name)  # AttributeError here means the .so is stale
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


EXPORTS = None  # filled lazily by tests from include/cbv.h


class Context:
    """One cbv_ctx (one GPU)."""

    def __init__(self, device_id=0):
        lib = load()
        h = C.c_void_p()
        rc = lib.cbv_ctx_create(device_id, C.byref(h))
        if rc != CBV_OK:
            msg = lib.cbv_last_error(None).decode()
            # no device / wrong device: surface as ImportError so the reference's
            # selector falls back (see module docstring)
            raise ImportError("chessboard_vision_amd: cannot open GPU %d: %s" % (device_id, msg))
        self.h = h
        self.lib = lib
        self.device_id = device_id

    def check(self, rc):
        if rc != CBV_OK:
            raise RuntimeError("libcbv_hip: %s (code %d)" % (self.lib.cbv_last_error(self.h).decode(), rc))

    @property
    def name(self):
        return self.lib.cbv_device_name(self.h).decode()

    def set_stream(self, stream_ptr):
        self.check(self.lib.cbv_ctx_set_stream(self.h, C.c_void_p(stream_ptr)))

    def synchronize(self):
        self.check(self.lib.cbv_ctx_synchronize(self.h))

    def profile_enable(self, kid):
        self.check(self.lib.cbv_profile_enable(self.h, kid))

    def profile_reset(self):
        self.check(self.lib.cbv_profile_reset(self.h))

    def profile_read(self, kid):
        ms, n = C.c_double(), C.c_longlong()
        self.check(self.lib.cbv_profile_read(self.h, kid, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def close(self):
        if self.h:
            self.lib.cbv_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}


def context(device_id=None):
    """Process-wide context per device.  Device defaults to $CBV_DEVICE or
    $LOCAL_RANK (one process per GPU) or 0."""
    if device_id is None:
        device_id = int(os.environ.get("CBV_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    if device_id not in _default_ctx:
        _default_ctx[device_id] = Context(device_id)
    return _default_ctx[device_id]


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def as_bgr(frame):
    """uint8 HxWx3 array with contiguous pixels (row stride free)."""
    a = np.asarray(frame)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("expected a uint8 HxWx3 BGR frame, got %s %s" % (a.dtype, a.shape))
    if a.strides[2] != 1 or a.strides[1] != 3 or a.strides[0] < a.shape[1] * 3:
        a = np.ascontiguousarray(a)
    return a


def format_id(fmt):
    """CBV_FMT_* of "bgr" | "nv12" | "nv21" | "yuv420p" | "yv12" | "yuyv" | "yvyu" | "uyvy" | "bayer_rggb" | "bayer_bggr" |
    "bayer_grbg" | "bayer_gbrg", or one of those four with "16", "10p" or "12p" behind it (BAYER_DEEP_FORMATS).  The three-plane 4:2:0 format goes by libav's name, "yuv420p" (cv2's COLOR_YUV2BGR_I420 /
    _IYUV); "i420" is an unknown format and raises ValueError.  A Bayer layout goes by its top-left 2 x 2 block read row by
    row (libav's bayer_rggb8, V4L2's SRGGB8); cv2 names the block at (1, 1), so "bayer_rggb" is COLOR_BayerBG2BGR."""
    try:
        name = fmt.lower()
        return FORMATS[name] if name in FORMATS else BAYER_FORMATS[name] if name in BAYER_FORMATS else BAYER_DEEP_FORMATS[name]
    except (KeyError, AttributeError):
        raise ValueError("unknown frame format %r (expected one of %s)" % (fmt, ", ".join(list(FORMATS) + list(BAYER_FORMATS) + list(BAYER_DEEP_FORMATS))))


def _rows(a, what):
    """uint8 2-D array whose rows are contiguous bytes (row stride free)."""
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError("expected uint8 rows for %s, got %s %s" % (what, a.dtype, a.shape))
    if a.strides[1] != 1 or a.strides[0] < a.shape[1]:
        a = np.ascontiguousarray(a)
    return a


def raw_frame(frame, fmt, colorspace="bt601"):
    """(RawFrame, w, h, arrays the struct points into) of a camera-native frame.  Row strides are free unless stated.
    "nv12" / "nv21": one [h * 3 // 2, w] array or a (y [h, w], chroma [h // 2, w] or [h // 2, w // 2, 2]) pair.
    "yuv420p" / "yv12": one [h * 3 // 2, w] array, cv2's single-matrix layout with the planes back to back (a strided one is
    made contiguous first), or a triple of planes in the format's memory order, (y, u, v) for yuv420p and (y, v, u) for
    yv12, of shapes [h, w], [h // 2, w // 2], [h // 2, w // 2].  ("i420" is not a name: see format_id.)
    "yuyv" / "yvyu" / "uyvy": [h, w, 2].  "bgr": [h, w, 3].
    "bayer_rggb" / "bayer_bggr" / "bayer_grbg" / "bayer_gbrg": one [h, w] array, w and h even and at least 4; a view whose
    rows are contiguous is taken as it is, whatever its row stride.  With "16" behind the name: one uint16 [h, w] array; with
    "10p": one uint8 [h, w * 5 // 4] array of MIPI RAW10 rows (w a multiple of 4); with "12p": one uint8 [h, w * 3 // 2] array
    of MIPI RAW12 rows; the row stride is free again (V4L2's bytesperline padding).
    ValueError for other shapes and dtypes, an odd w, and an odd h of a 4:2:0 format.
    `colorspace` (COLORSPACES; YUV formats only) goes into the struct's format id: ValueError for an unknown name, and for
    another colour space than "bt601" with a format that is not YUV."""
    bits = colorspace_bits(colorspace, fmt)
    r, w, h, keep = _raw_frame(frame, fmt)
    r.fmt |= bits
    return r, w, h, keep


def _raw_frame(frame, fmt):
    """raw_frame in colour space "bt601"."""
    f = format_id(fmt)
    name = fmt.upper()
    if f & 15 == FMT_BAYER_RGGB and f & BAYER_ENC_MASK:
        enc = f & BAYER_ENC_MASK
        a = np.asarray(frame) if not isinstance(frame, (tuple, list)) else None
        item = 2 if enc == BAYER_16 else 1
        if a is None or a.dtype != (np.uint16 if enc == BAYER_16 else np.uint8) or a.ndim != 2:
            raise ValueError("expected one %s 2-D %s mosaic, got %s" % ("uint16" if enc == BAYER_16 else "uint8", name, _describe(frame)))
        if a.strides[1] != item or a.strides[0] < a.shape[1] * item:
            a = np.ascontiguousarray(a)
        group, samples = {BAYER_16: (1, 1), BAYER_10P: (5, 4), BAYER_12P: (3, 2)}[enc]
        if a.shape[1] % group:
            raise ValueError("a %s row is a multiple of %d bytes, got %s" % (name, group, a.shape))
        w, h = a.shape[1] // group * samples, a.shape[0]
        if h % 2 or w % 2 or min(w, h) < 4:
            raise ValueError("a %s frame has an even width and height of at least 4, got %dx%d" % (name, w, h))
        r = RawFrame()
        r.fmt, r.stride0, r.plane0 = f, a.strides[0], a.ctypes.data
        return r, w, h, (a,)
    if f & 15 == FMT_BAYER_RGGB:
        a = np.asarray(frame) if not isinstance(frame, (tuple, list)) else None
        if a is None or a.dtype != np.uint8 or a.ndim != 2:
            raise ValueError("expected one uint8 HxW %s mosaic, got %s" % (name, _describe(frame)))
        if a.shape[0] % 2 or a.shape[1] % 2 or min(a.shape) < 4:
            raise ValueError("a %s frame has an even width and height of at least 4, got %s" % (name, a.shape))
        a = _rows(a, "the %s frame" % name)
        r = RawFrame()
        r.fmt, r.stride0, r.plane0 = f, a.strides[0], a.ctypes.data
        return r, a.shape[1], a.shape[0], (a,)
    odd_ok = f in (FMT_NV12, FMT_YUYV)   # these two leave odd sizes to the library's own check (a RuntimeError), as they always did
    r = RawFrame()
    r.fmt = f
    if f == FMT_BGR:
        a = as_bgr(frame)
        r.stride0, r.plane0 = a.strides[0], a.ctypes.data
        return r, a.shape[1], a.shape[0], (a,)
    if f & 15 == FMT_YUYV:
        a = np.asarray(frame) if not isinstance(frame, (tuple, list)) else None
        if a is None or a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 2:
            raise ValueError("expected a uint8 HxWx2 %s frame, got %s" % (name, _describe(frame)))
        if not odd_ok and a.shape[1] % 2:
            raise ValueError("a %s frame has an even width, got %s" % (name, a.shape))
        if a.strides[2] != 1 or a.strides[1] != 2 or a.strides[0] < a.shape[1] * 2:
            a = np.ascontiguousarray(a)
        r.stride0, r.plane0 = a.strides[0], a.ctypes.data
        return r, a.shape[1], a.shape[0], (a,)
    planar = bool(f & 0x20)
    if isinstance(frame, (tuple, list)) and planar:
        if len(frame) != 3:
            raise ValueError("a %s frame is one array or three planes, got %d" % (name, len(frame)))
        y, c1, c2 = (_rows(p, "a %s plane" % name) for p in frame)
        h, w = y.shape
        if h % 2 or w % 2 or c1.shape != (h // 2, w // 2) or c2.shape != c1.shape:
            raise ValueError("%s planes do not fit: luma %s, chroma %s and %s" % (name, y.shape, c1.shape, c2.shape))
        r.stride0, r.plane0, r.stride1, r.plane1, r.stride2, r.plane2 = (y.strides[0], y.ctypes.data, c1.strides[0], c1.ctypes.data,
                                                                         c2.strides[0], c2.ctypes.data)
        return r, w, h, (y, c1, c2)
    if isinstance(frame, (tuple, list)):
        if len(frame) != 2:
            raise ValueError("a %s frame is one array or a (luma, chroma) pair, got %d planes" % (name, len(frame)))
        y, uv = frame
        uv = np.asarray(uv)
        if uv.ndim == 3 and uv.shape[2] == 2 and uv.strides[2] == 1 and uv.strides[1] == 2:  # [h/2, w/2, 2] view of the chroma rows
            uv = np.lib.stride_tricks.as_strided(uv, shape=(uv.shape[0], uv.shape[1] * 2), strides=(uv.strides[0], 1))
        elif uv.ndim == 3 and uv.shape[2] == 2:
            uv = np.ascontiguousarray(uv).reshape(uv.shape[0], uv.shape[1] * 2)
        y, uv = _rows(y, "the luma plane"), _rows(uv, "the chroma plane")
        if y.shape[0] % 2 or uv.shape != (y.shape[0] // 2, y.shape[1]) or (not odd_ok and y.shape[1] % 2):
            raise ValueError("%s planes do not fit: luma %s, chroma %s" % (name, y.shape, uv.shape))
    else:
        a = _rows(frame, "the %s frame" % name)
        if a.shape[0] % 3:
            raise ValueError("the [h * 3 // 2, w] array of a %s frame has a multiple of 3 rows, got %s" % (name, a.shape))
        h = a.shape[0] // 3 * 2
        if not odd_ok and (h % 2 or a.shape[1] % 2):
            raise ValueError("a %s frame has an even width and height, got %s" % (name, a.shape))
        if planar:
            w = a.shape[1]
            if a.strides[0] != w:  # the chroma planes are rows of w // 2 bytes back to back: only a contiguous array holds them
                a = np.ascontiguousarray(a)
            y = a[:h]
            c1 = np.ndarray((h // 2, w // 2), np.uint8, a, offset=h * w)
            c2 = np.ndarray((h // 2, w // 2), np.uint8, a, offset=h * w + (h // 2) * (w // 2))
            r.stride0, r.plane0, r.stride1, r.plane1, r.stride2, r.plane2 = w, y.ctypes.data, w // 2, c1.ctypes.data, w // 2, c2.ctypes.data
            return r, w, h, (a, y, c1, c2)
        y, uv = a[:h], a[h:]
    r.stride0, r.plane0, r.stride1, r.plane1 = y.strides[0], y.ctypes.data, uv.strides[0], uv.ctypes.data
    return r, y.shape[1], y.shape[0], (y, uv)


def _describe(frame):
    if isinstance(frame, (tuple, list)):
        return "%d planes" % len(frame)
    a = np.asarray(frame)
    return "%s %s" % (a.dtype, a.shape)
