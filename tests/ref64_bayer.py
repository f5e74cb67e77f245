"""The bilinear demosaic of an 8-bit Bayer mosaic (include/cbv.h, CBV_FMT_BAYER_*), restated twice, and the sampler that
makes a mosaic from a BGR frame.  Imports neither the product nor the oracle.

`to_bgr` is the float64 meaning: per colour, the mean of the nearest samples of that colour, rounded half up.  It is a
masked convolution of the mosaic: the colour's samples are kept, everything else is zero, and the sum over the 3 x 3
neighbourhood with the bilinear kernel is divided by the kernel's weight over the samples present.  For the layouts of a
Bayer mosaic that is the kernel / 4 of the issue: red and blue take [[1,2,1],[2,4,2],[1,2,1]] / 4, green takes
[[0,1,0],[1,4,1],[0,1,0]] / 4, each over its own samples only, and in the interior the weights present always sum to 4.
`to_bgr_int` is the integer restatement with the shifts of the definition.  Both fill the frame's edge by the clamp on
indices: out(x, y) = D(clamp(x, 1, w - 2), clamp(y, 1, h - 2))."""
import numpy as np

FORMATS = ("bayer_rggb", "bayer_bggr", "bayer_grbg", "bayer_gbrg")
IDS = {"bayer_rggb": 0x04, "bayer_bggr": 0x14, "bayer_grbg": 0x24, "bayer_gbrg": 0x34}
# the top-left 2 x 2 block, rows 0 and 1, as channel indices of a BGR pixel (B = 0, G = 1, R = 2)
BLOCK = {"bayer_rggb": ((2, 1), (1, 0)), "bayer_bggr": ((0, 1), (1, 2)), "bayer_grbg": ((1, 2), (0, 1)), "bayer_gbrg": ((1, 0), (2, 1))}

K_RB = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], np.float64) / 4
K_G = np.array([[0, 1, 0], [1, 4, 1], [0, 1, 0]], np.float64) / 4


def channel_map(fmt, h, w):
    """[h, w] array: which BGR channel the site carries"""
    blk = np.array(BLOCK[fmt])
    yy, xx = np.mgrid[0:h, 0:w]
    return blk[yy & 1, xx & 1]


def mosaic(bgr, fmt):
    """keep each pixel's one colour"""
    bgr = np.asarray(bgr)
    h, w = bgr.shape[:2]
    return np.take_along_axis(bgr, channel_map(fmt, h, w)[:, :, None], axis=2)[:, :, 0].copy()


def _check(raw):
    raw = np.asarray(raw)
    assert raw.dtype == np.uint8 and raw.ndim == 2
    h, w = raw.shape
    assert h >= 4 and w >= 4 and h % 2 == 0 and w % 2 == 0, raw.shape
    return raw, h, w


def _clamp_fill(inner):
    """[h - 2, w - 2, 3] interior results -> [h, w, 3] with the edge rule restated on indices"""
    hh, ww = inner.shape[0] + 2, inner.shape[1] + 2
    ys = np.clip(np.arange(hh), 1, hh - 2) - 1
    xs = np.clip(np.arange(ww), 1, ww - 2) - 1
    return inner[ys][:, xs]


def _conv3(a, k):
    """valid 3 x 3 correlation of a float64 [h, w] array: [h - 2, w - 2] (the kernels are symmetric)"""
    h, w = a.shape
    out = np.zeros((h - 2, w - 2), np.float64)
    for dy in range(3):
        for dx in range(3):
            if k[dy, dx] != 0.0:
                out += k[dy, dx] * a[dy:dy + h - 2, dx:dx + w - 2]
    return out


def to_bgr(raw, fmt):
    """float64 meaning: the mean of the nearest samples of each colour, floor(mean + 0.5)"""
    raw, h, w = _check(raw)
    cm = channel_map(fmt, h, w)
    inner = np.zeros((h - 2, w - 2, 3), np.float64)
    for c in range(3):
        mask = (cm == c).astype(np.float64)
        k = K_G if c == 1 else K_RB
        inner[:, :, c] = _conv3(raw.astype(np.float64) * mask, k)
        # the weights over the samples present: 4 x kernel / 4 sums to 1 everywhere in the interior of a Bayer mosaic
        assert np.array_equal(_conv3(mask, k), np.ones((h - 2, w - 2)))
    return _clamp_fill(np.floor(inner + 0.5).astype(np.uint8))


def to_bgr_int(raw, fmt):
    """the integer definition, site by site in vector form, with the shifts as include/cbv.h writes them"""
    raw, h, w = _check(raw)
    p = raw.astype(np.int64)
    c = p[1:-1, 1:-1]
    l, r, u, d = p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1]
    cross = (l + r + u + d + 2) >> 2
    diag = (p[:-2, :-2] + p[:-2, 2:] + p[2:, :-2] + p[2:, 2:] + 2) >> 2
    hp, vp = (l + r + 1) >> 1, (u + d + 1) >> 1
    cm = channel_map(fmt, h, w)
    own = cm[1:-1, 1:-1]                      # the site's own colour
    rowc = cm[1:-1, :-2]                      # at a green site: the colour of the samples in this row
    inner = np.zeros((h - 2, w - 2, 3), np.int64)
    for ch in (0, 2):
        other = 2 - ch
        inner[:, :, ch] = np.where(own == ch, c, np.where(own == other, diag, np.where(rowc == ch, hp, vp)))
    inner[:, :, 1] = np.where(own == 1, c, cross)
    assert inner.min() >= 0 and inner.max() <= 255
    return _clamp_fill(inner.astype(np.uint8))


# the shapes (w, h) the GPU tests convert, and the inputs for each
SHAPES = [(4, 4), (4, 6), (6, 4), (6, 6), (10, 6), (322, 6), (8, 4), (64, 48), (320, 240)]


def inputs(w, h, seed=0):
    """name -> [h, w] uint8 mosaic: white noise, all 0, all 255, 0/255 checkers of period 1 and 2"""
    rng = np.random.default_rng(seed * 7919 + w * 31 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    return {"noise": rng.integers(0, 256, (h, w), dtype=np.uint8),
            "zeros": np.zeros((h, w), np.uint8),
            "ones": np.full((h, w), 255, np.uint8),
            "checker1": (((xx + yy) & 1) * 255).astype(np.uint8),
            "checker2": ((((xx >> 1) + (yy >> 1)) & 1) * 255).astype(np.uint8)}
