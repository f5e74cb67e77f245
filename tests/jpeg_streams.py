"""The JPEG streams the host-twin tests (test_jpeg_host.py) and the GPU tests (test_gpu_jpeg.py) share, built by
tests/ref_jpeg.py's encoders, and their reference decodes, computed once per process."""
import functools

import numpy as np

import ref_jpeg as R

SHAPES = [(1, 1), (8, 8), (17, 23), (33, 50), (9, 40), (40, 9)]  # (w, h): partial MCUs on both axes, odd chroma widths
SAMPLINGS = ("444", "422", "420", "gray")


def scene(w, h, seed=0):
    """a picture with edges, gradients and some noise, so that every frequency and both chroma planes carry something"""
    rs = np.random.RandomState(seed + 7 * w + h)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 5 + y * 2) % 256, (x * y) % 256, 255 - (x * 3 + y * 7) % 256], -1).astype(np.int64)
    img[(x // 4 + y // 4) % 2 == 0] //= 3
    img += rs.randint(-20, 21, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def shape_stream(w, h, sampling):
    return R.encode_image(scene(w, h), quality=90, sampling=sampling)


# restart markers.  64 x 48 has 48 MCUs at most (4:4:4), so the case with more than 64 intervals is 96 x 56 (84 MCUs).
RESTART_CASES = {
    "dri-1-mcu": (64, 48, "420", 1),        # 12 intervals
    "dri-mcu-row": (64, 48, "420", 4),      # an MCU row: 3 intervals
    "dri-wraps": (64, 48, "444", 4),        # 12 intervals: the numbering passes 7
    "dri-two-waves": (96, 56, "444", 1),    # 84 intervals: more than one wave of lanes
    "dri-last-short": (64, 48, "422", 5),   # 24 MCUs in intervals of 5: the last one is short
}


@functools.lru_cache(maxsize=None)
def restart_stream(name):
    w, h, sampling, dri = RESTART_CASES[name]
    return R.encode_image(scene(w, h, 3), quality=75, sampling=sampling, dri=dri)


# ---------------------------------------------------------------------------------------------------------------------
# streams from the coefficient encoder
# ---------------------------------------------------------------------------------------------------------------------
# sixteen symbols with code lengths 1..16: every length is used, the last code has 16 bits
LONG_DC = ([1] * 16, [0, 11, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14, 15])
LONG_AC = ([1] * 16, [0x01, 0x02, 0x03, 0x04, 0x11, 0x12, 0x21, 0x31, 0x00, 0x72, 0x05, 0x41, 0x13, 0xD1, 0xF0, 0x0A])


def _long_code_blocks():
    b = np.zeros((4, 64), np.int64)
    zz = R.ZIGZAG
    # block 0: DC size 11, AC size 10, then zeros up to coefficient 63 (three ZRL and a run of 13): no EOB
    b[0, 0] = 2047
    b[0, zz[1]] = 1023
    b[0, zz[63]] = 1
    # block 1: DC difference -2047 (size 11), all AC zero
    # block 2: one of every (run, size) symbol of the table, a ZRL chain in the middle
    for k, v in ((1, 1), (2, 2), (3, 5), (4, 9), (6, 1), (8, 3), (11, 1), (15, -1), (16, 17), (21, 1), (23, 4), (47, -3)):
        b[2, zz[k]] = v
    b[2, 0] = 5
    # block 3: all zero (DC difference -5)
    return b


@functools.lru_cache(maxsize=None)
def special_stream(name):
    q1, q255 = np.ones(64, np.int64), np.full(64, 255, np.int64)
    if name == "long-codes-gray":  # 16 x 16 gray: four blocks, tables with 16-bit codes, quantiser 1
        blocks = _long_code_blocks().reshape(2, 2, 64)
        return R.encode_coefs([blocks], 16, 16, "gray", {0: q1}, huff={(0, 0): LONG_DC, (1, 0): LONG_AC}, tq=[0], tsel=[(0, 0)])
    if name == "long-codes-420":   # 16 x 16 4:2:0: one MCU, luma with the long tables, chroma with the standard ones
        blocks = _long_code_blocks()
        c = np.zeros((1, 1, 64), np.int64)
        c[0, 0, 0], c[0, 0, 1], c[0, 0, 8] = -30, 12, -7
        return R.encode_coefs([blocks.reshape(2, 2, 64), c, -c], 16, 16, "420", {0: q1, 1: q1},
                              huff={(0, 0): LONG_DC, (1, 0): LONG_AC, (0, 1): R.STD_DC_CHR, (1, 1): R.STD_AC_CHR})
    rs = np.random.RandomState(11)

    def sparse(bh, bw, amp):
        a = np.zeros((bh, bw, 64), np.int64)
        a[..., 0] = rs.randint(-amp, amp + 1, (bh, bw))
        for _ in range(3):
            k = rs.randint(1, 64, (bh, bw))
            np.put_along_axis(a, k[..., None], rs.randint(-amp // 4, amp // 4 + 1, (bh, bw, 1)), axis=-1)
        return a

    if name.startswith("q1-q255"):  # 17 x 23 4:2:0 (2 x 2 MCUs): quantisers 1 (id 0) and 255 (id 2), two DQT ids
        coefs = [sparse(4, 4, 600), sparse(2, 2, 3), sparse(2, 2, 3)]
        kw = {}
        if name == "q1-q255-split-dht":
            kw = dict(split_dht=True)
        elif name == "q1-q255-no-dht":
            kw = dict(omit_dht=True)
        elif name == "q1-q255-segments":
            kw = dict(fill=2, extra=[(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"), (0xE1, b"Exif\x00\x00" + bytes(range(40))),
                                     (0xFE, b"a comment with \xff\xd8 inside"), (0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x01")])
        return R.encode_coefs(coefs, 17, 23, "420", {0: q1, 2: q255}, tq=[0, 2, 2], **kw)
    if name == "zero-blocks-422":  # 40 x 9 4:2:2: every coefficient zero
        return R.encode_coefs([np.zeros((2, 6, 64), np.int64), np.zeros((2, 3, 64), np.int64), np.zeros((2, 3, 64), np.int64)], 40, 9, "422",
                              {0: q1, 1: q255})
    raise KeyError(name)


SPECIAL = ("long-codes-gray", "long-codes-420", "q1-q255", "q1-q255-split-dht", "q1-q255-no-dht", "q1-q255-segments", "zero-blocks-422")


def entropy_of(data):
    h = R.parse(data)
    return bytes(data)[h["ent_off"]:]


# ---------------------------------------------------------------------------------------------------------------------
# four fixed damaged streams, made from one good one: 64 x 48 4:2:2, 24 MCUs in 12 intervals of 2
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def damage_base():
    return R.encode_image(scene(64, 48, 5), quality=90, sampling="422", dri=2)


def _markers(d):
    off = R.parse(d)["ent_off"]
    return [i for i in range(off, len(d) - 1) if d[i] == 0xFF and 0xD0 <= d[i + 1] <= 0xD7]


@functools.lru_cache(maxsize=None)
def damaged_stream(name):
    d = bytearray(damage_base())
    m = _markers(d)
    assert len(m) == 11
    if name == "truncated":          # cut inside interval 7
        return bytes(d[:(m[6] + m[7]) // 2])
    if name == "bad-code":           # interval 3 starts with sixteen 1 bits: no DC code
        assert m[3] - m[2] > 6
        d[m[2] + 2:m[2] + 6] = b"\xff\x00\xff\x00"
        return bytes(d)
    if name == "missing-restart":    # marker 5 is gone
        del d[m[5]:m[5] + 2]
        return bytes(d)
    if name == "wrong-restart-number":
        d[m[5] + 1] = 0xD0 + ((5 + 3) & 7)
        return bytes(d)
    raise KeyError(name)


DAMAGED = {"truncated": R.NO_DATA | R.RESTART, "bad-code": R.BAD_CODE, "missing-restart": R.RESTART, "wrong-restart-number": R.RESTART}


@functools.lru_cache(maxsize=None)
def frame_1080p():
    """(picture, stream): 1920 x 1080 4:2:2 at quality 90, a restart interval of one MCU row (68 intervals)"""
    rs = np.random.RandomState(5)
    y, x = np.mgrid[0:1080, 0:1920]
    img = np.stack([(x // 3 + y // 5) % 256, (x * y // 512) % 256, 255 - (x // 2 + y) % 256], -1).astype(np.uint8)
    img[::7, ::5] = rs.randint(0, 256, img[::7, ::5].shape)
    img.setflags(write=False)
    return img, R.encode_image(img, quality=90, sampling="422", dri=120)


def all_valid():
    """(name, stream) of every undamaged stream above"""
    out = [("%dx%d-%s" % (w, h, s), shape_stream(w, h, s)) for (w, h) in SHAPES for s in SAMPLINGS]
    out += [(n, restart_stream(n)) for n in RESTART_CASES]
    out += [(n, special_stream(n)) for n in SPECIAL]
    return out


@functools.lru_cache(maxsize=None)
def _ref_cached(data):
    return R.decode(data)


def ref(data):
    """tests/ref_jpeg.py's decode of a stream, computed once; the arrays are read-only"""
    r = _ref_cached(bytes(data))
    for k in ("bgr", "coef", "planes"):
        r[k].setflags(write=False)
    return r
