"""cv2.cvtColor's COLOR_YUV2BGR_NV12 / COLOR_YUV2BGR_YUY2 on 8-bit data, restated from the definition: BT.601, limited
range, fixed point with 20 fraction bits in numpy int64, no chroma interpolation; the float64 form of the same
coefficients; and a BGR -> YUV generator that prepares test INPUTS (never an expected value).  Imports neither the
product nor the oracle."""
import numpy as np

SHIFT = 20
CY, CUB, CUG, CVG, CVR = 1220542, 2116026, -409993, -852492, 1673527   # round(c * 2^20) of 1.164, 2.018, 0.391, 0.813, 1.596


def yuv_to_bgr_int(Y, U, V, with_extremes=False):
    """(Y, U, V) byte arrays of one shape -> uint8 [..., 3] BGR, every step in int64.  with_extremes: also the largest
    magnitude any intermediate sum reached."""
    y = np.maximum(0, np.asarray(Y, np.int64) - 16) * CY + (1 << (SHIFT - 1))
    u, v = np.asarray(U, np.int64) - 128, np.asarray(V, np.int64) - 128
    sums = (y + CUB * u, y + CVG * v + CUG * u, y + CVR * v)
    out = np.stack([np.clip(s >> SHIFT, 0, 255) for s in sums], axis=-1).astype(np.uint8)   # >> on int64: arithmetic
    if with_extremes:
        return out, max(int(np.abs(t).max()) for t in sums + (y, CUB * u, CVG * v, CUG * u, CVG * v + CUG * u, CVR * v))
    return out


def yuv_to_bgr_float(Y, U, V):
    """The published BT.601 coefficients in float64, rounded to nearest (half to even), saturated."""
    y = 1.164 * np.maximum(0, np.asarray(Y, np.float64) - 16)
    u, v = np.asarray(U, np.float64) - 128, np.asarray(V, np.float64) - 128
    bgr = np.stack([y + 2.018 * u, y - 0.813 * v - 0.391 * u, y + 1.596 * v], axis=-1)
    return np.clip(np.rint(bgr), 0, 255).astype(np.uint8)


def split_nv12(frame):
    """[h * 3 // 2, w] -> per-pixel (Y, U, V) planes [h, w]: a pixel takes the U, V of its 2x2 block."""
    frame = np.asarray(frame)
    h = frame.shape[0] // 3 * 2
    w = frame.shape[1]
    assert frame.shape[0] * 2 == h * 3 and h % 2 == 0 and w % 2 == 0
    uv = frame[h:].reshape(h // 2, w // 2, 2)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
    return frame[:h], up(uv[..., 0]), up(uv[..., 1])


def split_yuyv(frame):
    """[h, w, 2] (Y0 U Y1 V) -> per-pixel (Y, U, V) planes [h, w]: a pixel takes the U, V of its horizontal pair."""
    frame = np.asarray(frame)
    assert frame.ndim == 3 and frame.shape[2] == 2 and frame.shape[1] % 2 == 0
    c = frame[..., 1]
    return frame[..., 0], np.repeat(c[:, 0::2], 2, axis=1), np.repeat(c[:, 1::2], 2, axis=1)


def nv12_to_bgr(frame):
    return yuv_to_bgr_int(*split_nv12(frame))


def yuyv_to_bgr(frame):
    return yuv_to_bgr_int(*split_yuyv(frame))


def to_bgr(frame, fmt):
    return {"nv12": nv12_to_bgr, "yuyv": yuyv_to_bgr}[fmt](frame)


# --- input preparation --------------------------------------------------------------------------------------------
def _forward(bgr):
    """float64 BT.601 forward transform, limited range: BGR [h, w, 3] -> Y, U, V float planes."""
    b, g, r = (np.asarray(bgr, np.float64)[..., i] for i in range(3))
    y = 16 + 0.257 * r + 0.504 * g + 0.098 * b
    u = 128 - 0.148 * r - 0.291 * g + 0.439 * b
    v = 128 + 0.439 * r - 0.368 * g - 0.071 * b
    return y, u, v


def _bytes(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def bgr_to_nv12(bgr):
    """A plausible NV12 frame [h * 3 // 2, w] of a BGR image (even w, h): chroma averaged over 2x2 blocks."""
    y, u, v = _forward(bgr)
    h, w = y.shape
    avg = lambda c: c.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))
    out = np.empty((h * 3 // 2, w), np.uint8)
    out[:h] = _bytes(y)
    out[h:] = np.stack([_bytes(avg(u)), _bytes(avg(v))], axis=-1).reshape(h // 2, w)
    return out


def bgr_to_yuyv(bgr):
    """A plausible YUYV frame [h, w, 2] of a BGR image (even w): chroma averaged over horizontal pairs."""
    y, u, v = _forward(bgr)
    h, w = y.shape
    avg = lambda c: c.reshape(h, w // 2, 2).mean(axis=2)
    out = np.empty((h, w, 2), np.uint8)
    out[..., 0] = _bytes(y)
    out[:, 0::2, 1] = _bytes(avg(u))
    out[:, 1::2, 1] = _bytes(avg(v))
    return out


def from_bgr(bgr, fmt):
    return {"nv12": bgr_to_nv12, "yuyv": bgr_to_yuyv}[fmt](bgr)


def cube_nv12():
    """One 4096 x 4096 NV12 frame that holds every (Y, U, V) triple exactly once: chroma block (by, bx) has
    U = bx % 256, V = by % 256, and its four pixels have Y = 4 * (bx // 256 + 8 * (by // 256)) + {0, 1, 2, 3}."""
    n = 4096
    by, bx = np.mgrid[:n // 2, :n // 2]
    base = 4 * (bx // 256 + 8 * (by // 256))
    out = np.empty((n * 3 // 2, n), np.uint8)
    out[0:n:2, 0::2], out[0:n:2, 1::2], out[1:n:2, 0::2], out[1:n:2, 1::2] = base, base + 1, base + 2, base + 3
    out[n:, 0::2], out[n:, 1::2] = bx % 256, by % 256
    return out


def cube_yuyv(part, parts=4):
    """Frame `part` of `parts` 4096-wide YUYV frames that together hold every (Y, U, V) triple exactly once: pair (row,
    px) has U = px % 256, V = row % 256, and its two pixels have Y = 2 * (px // 256 + 8 * (row // 256)) + {0, 1}."""
    n = 4096
    rows = n // parts
    row, px = np.mgrid[part * rows:(part + 1) * rows, :n // 2]
    base = 2 * (px // 256 + 8 * (row // 256))
    out = np.empty((rows, n, 2), np.uint8)
    out[:, 0::2, 0], out[:, 1::2, 0] = base, base + 1
    out[:, 0::2, 1], out[:, 1::2, 1] = px % 256, row % 256
    return out
