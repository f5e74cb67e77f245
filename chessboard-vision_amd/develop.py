"""Developing a Bayer mosaic: the per-colour tables in front of the demosaic (include/cbv.h, "developed mosaics").

Black level, white level, white-balance gains and a tone curve are each a function of one sample of one colour, so together
they are one lookup table per colour from a raw sample to a byte.  `Develop` builds the tables in numpy, in float64, and
hands them to the library as data: the library evaluates no power function.  `stream.BoardPipeline.set_input_format`,
`set_develop` and `board_detection.bayer_to_bgr` take a `Develop`, a uint8 [3, 2^bits] array (rows B, G, R), or None for
the format's default."""
import json

import numpy as np


class Develop:
    """Tables for samples of `bits` bits (8 for the 8-bit mosaics, 10 for "...10p", 12 for "...12p", 10 / 12 / 14 / 16 for
    "...16"): for sample v of colour c, in float64,
        x = clip((v - black_level) / (white_level - black_level), 0, 1);  x = min(x * gain_c, 1);
        byte = floor(255 * x ** (1 / gamma) + 0.5).
    `white_level` defaults to 2^bits - 1; `gains` are (r, g, b); `gamma` 1.0 leaves the data linear (2.2 is close to sRGB).
    Black level and gains come from the camera: the sensor's data sheet or V4L2_CID / GenICam BlackLevel, and the camera's
    white-balance ratios or a gray card (gain_c = green mean / colour mean)."""

    FIELDS = ("bits", "black_level", "white_level", "gains", "gamma")

    def __init__(self, bits, black_level=0, white_level=None, gains=(1, 1, 1), gamma=1.0):
        bits = int(bits)
        if bits not in (8, 10, 12, 14, 16):
            raise ValueError("bits %r: expected 8, 10, 12, 14 or 16" % (bits,))
        white_level = (1 << bits) - 1 if white_level is None else white_level
        gains = tuple(float(g) for g in gains)
        if len(gains) != 3 or not all(np.isfinite(g) and g >= 0 for g in gains):
            raise ValueError("gains %r: three finite values (r, g, b), none negative" % (gains,))
        if not (np.isfinite(black_level) and np.isfinite(white_level) and white_level > black_level):
            raise ValueError("white_level %r must lie above black_level %r" % (white_level, black_level))
        if not (np.isfinite(gamma) and gamma > 0):
            raise ValueError("gamma %r: a positive number" % (gamma,))
        self.bits, self.black_level, self.white_level, self.gains, self.gamma = bits, float(black_level), float(white_level), gains, float(gamma)

    def tables(self):
        """uint8 [3, 2^bits], rows in B, G, R order (the BGR channel index)."""
        v = np.arange(1 << self.bits, dtype=np.float64)
        x = np.clip((v - self.black_level) / (self.white_level - self.black_level), 0.0, 1.0)
        r, g, b = self.gains
        out = np.empty((3, v.size), np.uint8)
        for row, gain in enumerate((b, g, r)):
            xc = np.minimum(x * gain, 1.0)
            out[row] = np.floor(255.0 * xc ** (1.0 / self.gamma) + 0.5).astype(np.uint8)
        return out

    def to_dict(self):
        return {"bits": self.bits, "black_level": self.black_level, "white_level": self.white_level, "gains": list(self.gains), "gamma": self.gamma}

    def __eq__(self, other):
        return isinstance(other, Develop) and self.to_dict() == other.to_dict()

    def __repr__(self):
        return "Develop(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.FIELDS)


def develop_tables(develop, fmt_id):
    """(uint8 [3, 2^bits] contiguous array, bits) of a Develop or an array for the Bayer id `fmt_id`, or (None, 0) for None
    (the format's default).  ValueError for an array of another shape or dtype, and for bits that do not go with the encoding."""
    from . import _native as N
    if develop is None:
        return None, 0
    t = develop.tables() if isinstance(develop, Develop) else np.asarray(develop)
    if t.dtype != np.uint8 or t.ndim != 2 or t.shape[0] != 3 or t.shape[1] not in (1 << 8, 1 << 10, 1 << 12, 1 << 14, 1 << 16):
        raise ValueError("tables are a uint8 [3, 2^bits] array (rows B, G, R), got %s %s" % (t.dtype, t.shape))
    bits = t.shape[1].bit_length() - 1
    allowed = N.BAYER_TABLE_BITS[fmt_id & N.BAYER_ENC_MASK]
    if bits not in allowed:
        raise ValueError("tables of %d bits do not go with this format (%s)" % (bits, " / ".join(str(b) for b in allowed)))
    return np.ascontiguousarray(t), bits


def save_develop(path, develop):
    """Write a Develop as JSON (bits, black_level, white_level, gains = [r, g, b], gamma).  Returns what was written."""
    data = develop.to_dict()
    with open(path, "w") as f:
        json.dump(data, f, indent=4)
    return data


def load_develop(path):
    """The Develop of a JSON file written by `save_develop` (white_level, gains and gamma may be missing: their defaults)."""
    with open(path) as f:
        data = json.load(f)
    return Develop(data["bits"], data.get("black_level", 0), data.get("white_level"), tuple(data.get("gains", (1, 1, 1))), data.get("gamma", 1.0))
