"""The yardstick of the raw-frame profile warp (cbv_warp_color_profile_raw, CBV_SKIP_ENHANCE_PROFILE_RAW): the oracle's
warp_perspective of the oracle's apply_color_profile of the converted frame, the conversion being the int64 definition of
ref64_yuv / ref64_yuv_layouts and the integer demosaic of ref64_bayer; and the inputs: camera-native frames made from a BGR
frame by ref64_yuv's forward transform, ref64_yuv_layouts' byte shuffles and ref64_bayer's mosaic sampler.  Nothing here
touches the code under test."""
import numpy as np

import ref64_bayer as RB
import ref64_yuv as RY
import ref64_yuv_layouts as RL

YUV_FORMATS = RL.FAMILY_420 + RL.FAMILY_422
FORMATS = YUV_FORMATS + RB.FORMATS


def to_bgr(raw, fmt):
    """the definition's BGR frame of a raw frame ([h * 3 // 2, w], [h, w, 2] or a [h, w] mosaic)"""
    return RB.to_bgr_int(raw, fmt) if fmt in RB.FORMATS else RL.to_bgr(raw, fmt)


def from_bgr(bgr, fmt):
    """a raw frame of a BGR picture (even w and h): an INPUT, never an expected value"""
    if fmt in RB.FORMATS:
        return RB.mosaic(bgr, fmt)
    base = "nv12" if fmt in RL.FAMILY_420 else "yuyv"
    return RL.relayout(RY.from_bgr(bgr, base), base, fmt)


def noise(w, h, fmt, seed):
    """white noise in the layout of `fmt`"""
    rng = np.random.default_rng(seed * 1009 + w * 31 + h)
    shape = (h, w) if fmt in RB.FORMATS else (h * 3 // 2, w) if fmt in RL.FAMILY_420 else (h, w, 2)
    return rng.integers(0, 256, shape, dtype=np.uint8)


def size_of(raw, fmt):
    """(w, h) of a raw frame"""
    raw = np.asarray(raw)
    return (raw.shape[1], raw.shape[0] // 3 * 2) if fmt in RL.FAMILY_420 else (raw.shape[1], raw.shape[0])


def yardstick(oracle, bgr, profile, M, dsize, rot180=False):
    """warp_perspective(apply_color_profile(bgr)) (+ rotate 180) of an already converted frame; no profile: the frame itself"""
    col = oracle.apply_color_profile(np.ascontiguousarray(bgr), profile) if profile else np.ascontiguousarray(bgr)
    out = oracle.warp_perspective(col, M, dsize)
    return oracle.rotate180(out) if rot180 else out


def quads(w, h):
    """source corners TL, TR, BL, BR"""
    return {"inside": [[w * .2, h * .1], [w * .85, h * .15], [w * .1, h * .9], [w * .95, h * .8]],
            "partly_outside": [[-w * .1, -h * .1], [w * 1.1, h * .05], [w * .02, h * 1.1], [w * .9, h * .95]],
            "mirrored": [[w * .9, h * .1], [w * .1, h * .1], [w * .9, h * .9], [w * .1, h * .9]],
            "outside": [[w + 40, h + 30], [w + 140, h + 35], [w + 45, h + 120], [w + 150, h + 130]]}


def source_coords(M, dsize):
    """float64 source coordinates (x [dh, dw], y [dh, dw]) of every destination pixel under the forward matrix M"""
    dw, dh = dsize
    Minv = np.linalg.inv(np.asarray(M, np.float64))
    yy, xx = np.mgrid[0:dh, 0:dw].astype(np.float64)
    W = Minv[2, 0] * xx + Minv[2, 1] * yy + Minv[2, 2]
    return (Minv[0, 0] * xx + Minv[0, 1] * yy + Minv[0, 2]) / W, (Minv[1, 0] * xx + Minv[1, 1] * yy + Minv[1, 2]) / W
