"""The layouts beside NV12 and YUYV (NV21, yuv420p, YV12, YVYU, UYVY: include/cbv.h) for the tests: where each pixel's Y,
U and V lie, restated from the layout table, and byte shuffles that turn the NV12 / YUYV frames of ref64_yuv's generators
into inputs of the other layouts.  The arithmetic is ref64_yuv.yuv_to_bgr_int and nothing else.  Imports neither the
product nor the oracle."""
import numpy as np

from ref64_yuv import yuv_to_bgr_int

FAMILY_420 = ("nv12", "nv21", "yuv420p", "yv12")   # one [h * 3 // 2, w] array
FAMILY_422 = ("yuyv", "yvyu", "uyvy")              # one [h, w, 2] array
NEW = ("nv21", "yuv420p", "yv12", "yvyu", "uyvy")
SIBLING = {"nv21": "nv12", "yuv420p": "nv12", "yv12": "nv12", "yvyu": "yuyv", "uyvy": "yuyv"}


def _chroma_420(frame, fmt):
    """(h, w, U [h/2, w/2], V [h/2, w/2]) of a [h * 3 // 2, w] frame"""
    frame = np.asarray(frame)
    w = frame.shape[1]
    h = frame.shape[0] // 3 * 2
    assert frame.ndim == 2 and frame.shape[0] * 2 == h * 3 and h % 2 == 0 and w % 2 == 0, frame.shape
    if fmt in ("nv12", "nv21"):
        pairs = frame[h:].reshape(h // 2, w // 2, 2)
        first, second = pairs[..., 0], pairs[..., 1]
    else:   # two planes of h/2 rows of w/2 bytes, back to back behind the luma rows
        planes = np.ascontiguousarray(frame[h:]).reshape(2, h // 2, w // 2)
        first, second = planes[0], planes[1]
    u, v = (first, second) if fmt in ("nv12", "yuv420p") else (second, first)
    return h, w, u, v


def split(frame, fmt):
    """per-pixel (Y, U, V) planes [h, w] of a frame of any layout: a pixel takes the U, V of its 2x2 block (4:2:0) or of
    its horizontal pair (4:2:2)"""
    frame = np.asarray(frame)
    if fmt in FAMILY_420:
        h, w, u, v = _chroma_420(frame, fmt)
        up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
        return frame[:h], up(u), up(v)
    assert fmt in FAMILY_422 and frame.ndim == 3 and frame.shape[2] == 2 and frame.shape[1] % 2 == 0, (fmt, frame.shape)
    yb, cb = (1, 0) if fmt == "uyvy" else (0, 1)          # UYVY: U Y0 V Y1, the others Y0 c Y1 c
    first, second = frame[:, 0::2, cb], frame[:, 1::2, cb]
    u, v = (second, first) if fmt == "yvyu" else (first, second)
    return frame[..., yb], np.repeat(u, 2, axis=1), np.repeat(v, 2, axis=1)


def to_bgr(frame, fmt):
    return yuv_to_bgr_int(*split(frame, fmt))


def relayout(src, src_fmt, fmt):
    """The frame `src` (NV12 [h * 3 // 2, w] or YUYV [h, w, 2]) with the same samples in layout `fmt` of the same family:
    bytes are moved, none is computed."""
    src = np.asarray(src)
    assert SIBLING.get(fmt, fmt) == src_fmt and src_fmt in ("nv12", "yuyv"), (src_fmt, fmt)
    if fmt == src_fmt:
        return src.copy()
    out = np.empty_like(src)
    if src_fmt == "nv12":
        w = src.shape[1]
        h = src.shape[0] // 3 * 2
        out[:h] = src[:h]
        uv = src[h:].reshape(h // 2, w // 2, 2)
        if fmt == "nv21":
            out[h:] = uv[..., ::-1].reshape(h // 2, w)
        else:
            first, second = (uv[..., 0], uv[..., 1]) if fmt == "yuv420p" else (uv[..., 1], uv[..., 0])
            out[h:] = np.concatenate([first.ravel(), second.ravel()]).reshape(h // 2, w)
        return out
    y, u, v = src[..., 0], src[:, 0::2, 1], src[:, 1::2, 1]
    if fmt == "yvyu":
        out[..., 0], out[:, 0::2, 1], out[:, 1::2, 1] = y, v, u
    else:   # uyvy
        out[..., 1], out[:, 0::2, 0], out[:, 1::2, 0] = y, u, v
    return out


def planes(frame, fmt):
    """the planes of a 4:2:0 frame in memory order as separate contiguous arrays: (y, chroma) or (y, c1, c2)"""
    frame = np.asarray(frame)
    w = frame.shape[1]
    h = frame.shape[0] // 3 * 2
    if fmt in ("nv12", "nv21"):
        return frame[:h].copy(), frame[h:].copy()
    c = np.ascontiguousarray(frame[h:]).reshape(2, h // 2, w // 2)
    return frame[:h].copy(), c[0].copy(), c[1].copy()
