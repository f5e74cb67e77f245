"""Developed mosaics (include/cbv.h: Bayer samples of 10 to 16 bits in a 16-bit container, MIPI RAW10 / RAW12 packed rows, and
per-colour tables in front of the 8-bit demosaic), restated.  Imports neither the product nor the oracle.

    m8(x, y) = T[c(x, y)][min(s(x, y), 2^bits - 1)],   BGR = ref64_bayer.to_bgr(m8)   (to_bgr_int is the second restatement)

`unpack` / `pack` are the table of encodings written out byte by byte, `develop` is the definition above with its clamp,
`neutral` the float64 meaning of the default table, and `develop_tables` the formula of stream.Develop."""
import numpy as np

import ref64_bayer as RB

LAYOUTS = RB.FORMATS
ENCODINGS = ("16", "10p", "12p")
FIELD = {"8": 0, "16": 0x1000, "10p": 0x2000, "12p": 0x3000}
# name -> (layout name, encoding)
FORMATS = {lay + enc: (lay, enc) for lay in LAYOUTS for enc in ENCODINGS}
IDS = {lay + enc: RB.IDS[lay] | FIELD[enc] for lay in LAYOUTS for enc in ENCODINGS}
BITS = {"8": (8,), "16": (10, 12, 14, 16), "10p": (10,), "12p": (12,)}     # the bits an encoding's tables may have
DEFAULT_BITS = {"16": 16, "10p": 10, "12p": 12}
SAMPLE_BITS = {"8": 8, "16": 16, "10p": 10, "12p": 12}                      # the bits an encoding can hold


def row_bytes(enc, w):
    return {"8": w, "16": 2 * w, "10p": 5 * w // 4, "12p": 3 * w // 2}[enc]


def pack(samples, enc):
    """[h, w] integer samples -> the rows as a camera delivers them: uint16 [h, w] for "16", uint8 [h, row bytes] otherwise"""
    s = np.asarray(samples).astype(np.int64)
    h, w = s.shape
    assert s.min() >= 0 and s.max() < (1 << SAMPLE_BITS[enc])
    if enc == "8":
        return s.astype(np.uint8)
    if enc == "16":
        return s.astype("<u2")
    out = np.zeros((h, row_bytes(enc, w)), np.uint8)
    if enc == "10p":
        assert w % 4 == 0
        for i in range(4):                                   # byte i of a group: the high eight bits of sample i
            out[:, i::5] = s[:, i::4] >> 2
        out[:, 4::5] = sum((s[:, i::4] & 3) << (2 * i) for i in range(4))   # byte 4: the low two bits, sample 0 lowest
        return out
    assert enc == "12p" and w % 2 == 0
    out[:, 0::3] = s[:, 0::2] >> 4
    out[:, 1::3] = s[:, 1::2] >> 4
    out[:, 2::3] = (s[:, 0::2] & 15) | ((s[:, 1::2] & 15) << 4)             # the even sample's low nibble lowest
    return out


def unpack(raw, enc):
    """the rows of `pack` -> [h, w] int64 samples, sample by sample as include/cbv.h's table writes them"""
    raw = np.asarray(raw)
    if enc == "8":
        assert raw.dtype == np.uint8
        return raw.astype(np.int64)
    if enc == "16":
        assert raw.dtype.itemsize == 2
        b = raw.astype("<u2").view(np.uint8).reshape(raw.shape[0], -1).astype(np.int64)
        return b[:, 0::2] | (b[:, 1::2] << 8)
    assert raw.dtype == np.uint8
    B = raw.astype(np.int64)
    h = B.shape[0]
    if enc == "10p":
        assert B.shape[1] % 5 == 0
        w = B.shape[1] // 5 * 4
        out = np.zeros((h, w), np.int64)
        for x in range(w):
            g, i = x >> 2, x & 3
            out[:, x] = (B[:, 5 * g + i] << 2) | ((B[:, 5 * g + 4] >> (2 * i)) & 3)
        return out
    assert enc == "12p" and B.shape[1] % 3 == 0
    w = B.shape[1] // 3 * 2
    out = np.zeros((h, w), np.int64)
    for x in range(w):
        g = x >> 1
        out[:, x] = (B[:, 3 * g + 1] << 4) | (B[:, 3 * g + 2] >> 4) if x & 1 else (B[:, 3 * g] << 4) | (B[:, 3 * g + 2] & 15)
    return out


def develop(samples, layout, tables, bits):
    """[h, w] samples -> the uint8 mosaic m8: the site's colour's table at min(sample, 2^bits - 1)"""
    s = np.asarray(samples).astype(np.int64)
    t = np.asarray(tables)
    assert t.shape == (3, 1 << bits) and t.dtype == np.uint8
    idx = np.minimum(s, (1 << bits) - 1)
    return t[RB.channel_map(layout, *s.shape), idx]


def expected(raw, fmt, tables, bits):
    """the BGR frame of the rows `raw` of format `fmt` (a name of FORMATS, or an 8-bit layout with tables)"""
    layout, enc = FORMATS[fmt] if fmt in FORMATS else (fmt, "8")
    return RB.to_bgr(develop(unpack(raw, enc), layout, tables, bits), layout)


def expected_int(raw, fmt, tables, bits):
    layout, enc = FORMATS[fmt] if fmt in FORMATS else (fmt, "8")
    return RB.to_bgr_int(develop(unpack(raw, enc), layout, tables, bits), layout)


def neutral(bits):
    """float64: v * 255 / M rounded half up, for every colour; uint8 [3, 2^bits]"""
    m = (1 << bits) - 1
    v = np.arange(m + 1, dtype=np.float64)
    return np.repeat(np.floor(v * 255.0 / m + 0.5).astype(np.uint8)[None], 3, axis=0)


def develop_tables(bits, black_level=0, white_level=None, gains=(1, 1, 1), gamma=1.0):
    """stream.Develop's formula, value by value in Python floats (float64): rows B, G, R"""
    white = (1 << bits) - 1 if white_level is None else white_level
    r, g, b = gains
    out = np.zeros((3, 1 << bits), np.uint8)
    for row, gain in enumerate((b, g, r)):
        for v in range(1 << bits):
            x = min(max((v - black_level) / (white - black_level), 0.0), 1.0)
            x = min(x * gain, 1.0)
            out[row, v] = int(np.floor(255.0 * np.float64(x) ** (1.0 / gamma) + 0.5))
    return out


def random_tables(bits, seed):
    """three DIFFERENT random byte tables: a site that takes another colour's table shows at once"""
    return np.random.default_rng(1000 * bits + seed).integers(0, 256, (3, 1 << bits), dtype=np.uint8)


# the shapes (w, h) the GPU tests convert; "10p" takes those with w % 4 == 0
SHAPES = [(4, 4), (8, 4), (6, 4), (6, 6), (12, 6), (324, 6), (64, 48), (320, 240)]


def inputs(w, h, sample_bits, seed=0):
    """name -> [h, w] samples below 2^sample_bits: full-range noise, all zero, all maximum, 0 / maximum checkers of period 1, 2"""
    rng = np.random.default_rng(seed * 7919 + w * 31 + h + sample_bits)
    top = (1 << sample_bits) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    return {"noise": rng.integers(0, top + 1, (h, w), dtype=np.int64),
            "zeros": np.zeros((h, w), np.int64),
            "ones": np.full((h, w), top, np.int64),
            "checker1": ((xx + yy) & 1) * top,
            "checker2": (((xx >> 1) + (yy >> 1)) & 1) * top}
