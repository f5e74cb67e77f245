"""The four colour spaces of a YUV frame (include/cbv.h, CBV_CS_*) restated from the definition for the tests: the table
of constants, the conversion in numpy int64 (the product's arithmetic) and in float64 with the exact coefficients, the
per-layout splitters, and float64 forward transforms that prepare test INPUTS (never an expected value).  Row 0 is
cv2's BT.601 limited range with its three-decimal constants (ref64_yuv); rows 1 to 3 are round(c * 2^20) of the exact
fractions.  Imports neither the product nor the oracle."""
from fractions import Fraction

import numpy as np

import ref64_yuv as R
import ref64_yuv_layouts as L

SHIFT = 20
NAMES = ("bt601", "bt601-full", "bt709", "bt709-full")
NEW = NAMES[1:]
LAYOUTS = L.FAMILY_420 + L.FAMILY_422
CS_FULL, CS_BT709, CS_MASK = 0x400, 0x800, 0xC00
BITS = {"bt601": 0, "bt601-full": CS_FULL, "bt709": CS_BT709, "bt709-full": CS_BT709 | CS_FULL}
# name: (yoff, CY, CUB, CUG, CVG, CVR), as the issue's table states them
TABLE = {
    "bt601": (16, 1220542, 2116026, -409993, -852492, 1673527),
    "bt601-full": (0, 1048576, 1858077, -360853, -748826, 1470104),
    "bt709": (16, 1220945, 2215014, -223607, -558796, 1879825),
    "bt709-full": (0, 1048576, 1945738, -196424, -490864, 1651297),
}
KR_KB = {"bt601-full": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000)),
         "bt709-full": (Fraction(2126, 10000), Fraction(722, 10000))}


def full_range(cs):
    return cs.endswith("-full")


def exact(cs):
    """(yoff, c_y, c_ub, c_ug, c_vg, c_vr) of rows 1 to 3 as exact fractions"""
    kr, kb = KR_KB[cs]
    kg = 1 - kr - kb
    cy, s = (Fraction(1), Fraction(1)) if full_range(cs) else (Fraction(255, 219), Fraction(255, 224))
    return (0 if full_range(cs) else 16, cy, 2 * (1 - kb) * s, -2 * kb * (1 - kb) * s / kg, -2 * kr * (1 - kr) * s / kg, 2 * (1 - kr) * s)


def yuv_to_bgr_int(Y, U, V, cs, with_extremes=False):
    """(Y, U, V) byte arrays of one shape -> uint8 [..., 3] BGR, every step in int64: clamp, then shift.  with_extremes: also
    the largest magnitude any intermediate sum reached."""
    yoff, CY, CUB, CUG, CVG, CVR = TABLE[cs]
    y = np.maximum(0, np.asarray(Y, np.int64) - yoff) * CY
    u, v = np.asarray(U, np.int64) - 128, np.asarray(V, np.int64) - 128
    half = 1 << (SHIFT - 1)
    sums = (y + half + CUB * u, y + half + CVG * v + CUG * u, y + half + CVR * v)
    out = np.stack([np.clip(s, 0, (256 << SHIFT) - 1) >> SHIFT for s in sums], axis=-1).astype(np.uint8)
    if with_extremes:
        parts = (y, half + CUB * u, CVG * v, half + CVG * v, half + CVG * v + CUG * u, half + CVR * v)
        return out, max(int(np.abs(t).max()) for t in sums + parts)
    return out


def yuv_to_bgr_float(Y, U, V, cs):
    """The exact coefficients in float64, rounded to nearest (half to even), saturated (rows 1 to 3)."""
    yoff, cy, cub, cug, cvg, cvr = (float(c) for c in exact(cs))
    y = cy * np.maximum(0, np.asarray(Y, np.float64) - yoff)
    u, v = np.asarray(U, np.float64) - 128, np.asarray(V, np.float64) - 128
    bgr = np.stack([y + cub * u, y + cvg * v + cug * u, y + cvr * v], axis=-1)
    return np.clip(np.rint(bgr), 0, 255).astype(np.uint8)


def split(frame, fmt):
    """per-pixel (Y, U, V) planes [h, w] of a frame of any of the seven layouts"""
    return L.split(frame, fmt)


def to_bgr(frame, fmt, cs):
    return yuv_to_bgr_int(*split(frame, fmt), cs)


# --- input preparation --------------------------------------------------------------------------------------------
def _forward(bgr, cs):
    """float64 forward transform of the colour space's Kr / Kb and range: BGR [h, w, 3] -> Y, U, V float planes"""
    if cs == "bt601":
        return R._forward(bgr)
    kr, kb = (float(k) for k in KR_KB[cs])
    b, g, r = (np.asarray(bgr, np.float64)[..., i] for i in range(3))
    y = kr * r + (1 - kr - kb) * g + kb * b
    pb, pr = (b - y) / (2 * (1 - kb)), (r - y) / (2 * (1 - kr))
    if full_range(cs):
        return y, 128 + pb, 128 + pr
    return 16 + y * 219 / 255, 128 + pb * 224 / 255, 128 + pr * 224 / 255


def from_bgr(bgr, fmt, cs):
    """A plausible frame of layout `fmt` in colour space `cs` of a BGR image (even w and h): chroma averaged over the 2 x 2
    block (4:2:0) or the pair (4:2:2)"""
    y, u, v = _forward(bgr, cs)
    h, w = y.shape
    family = L.SIBLING.get(fmt, fmt)
    if family == "nv12":
        avg = lambda c: c.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))
        out = np.empty((h * 3 // 2, w), np.uint8)
        out[:h] = R._bytes(y)
        out[h:] = np.stack([R._bytes(avg(u)), R._bytes(avg(v))], axis=-1).reshape(h // 2, w)
    else:
        avg = lambda c: c.reshape(h, w // 2, 2).mean(axis=2)
        out = np.empty((h, w, 2), np.uint8)
        out[..., 0] = R._bytes(y)
        out[:, 0::2, 1] = R._bytes(avg(u))
        out[:, 1::2, 1] = R._bytes(avg(v))
    return L.relayout(out, family, fmt)


def noise(w, h, fmt, seed):
    """a frame of layout `fmt` of uniformly random bytes"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h * 3 // 2, w) if fmt in L.FAMILY_420 else (h, w, 2), dtype=np.uint8)
