"""Streams without restart markers for the piece path of the JPEG decode (tests/test_jpeg_pieces_host.py and
tests/test_gpu_jpeg_pieces.py): each puts one feature of the entropy data across a piece boundary at piece_bytes = 4, and
checks that it does with a symbol trace of its own.  All are one-component streams from ref_jpeg.encode_coefs, n blocks in
a row, so one pair of tables decodes them."""
import functools

import numpy as np

import jpeg_streams as S
import ref_jpeg as R

PIECE = 4
Q1 = np.ones(64, np.int64)
ZZ = R.ZIGZAG
# every symbol of the standard AC table with an 8-bit code: nothing shorter to fall back into step with
FLAT_AC = ([0] * 7 + [162] + [0] * 8, list(R.STD_AC_LUM[1]))


def gray(blocks, huff=None):
    blocks = np.asarray(blocks, np.int64)
    n = blocks.shape[0]
    return R.encode_coefs([blocks.reshape(1, n, 64)], 8 * n, 8, "gray", {0: Q1}, huff=huff, tq=[0], tsel=[(0, 0)])


def trace(data):
    """the symbols of a one-component stream without DRI, up to the data's end: dicts with kind ("dc" | "ac"), rs (the
    symbol), k (the zig-zag index before it), a / c / b = the raw bit offsets in the entropy data of its first bit, of
    the first bit behind its code and of the first bit behind its value bits"""
    h = R.parse(data)
    assert len(h["comps"]) == 1 and not h["dri"]
    ent = bytes(data)[h["ent_off"]:]
    raw_of, bits, i = [], [], 0
    while i < len(ent):
        b = ent[i]
        if b == 0xFF and not (i + 1 < len(ent) and ent[i + 1] == 0):
            break
        raw_of.append(i)
        bits.append(format(b, "08b"))
        i += 2 if b == 0xFF else 1
    raw_of.append(i)
    s = "".join(bits)

    def raw(p):  # the raw offset of bit p (p = len(s): where the data ends)
        return raw_of[p // 8] * 8 + p % 8

    dc, ac = h["huff"][(0, h["comps"][0]["td"])], h["huff"][(1, h["comps"][0]["ta"])]
    out, p, k = [], 0, 0
    nblocks = h["comps"][0]["bw"] * h["comps"][0]["bh"]
    blk = 0
    while blk < nblocks:
        tab = dc if k == 0 else ac
        for l in range(1, 17):
            if p + l <= len(s) and (l, int(s[p:p + l], 2)) in tab:
                break
        else:
            break
        rs = tab[(l, int(s[p:p + l], 2))]
        size = rs if k == 0 else rs & 15
        if p + l + size > len(s):
            break
        out.append(dict(kind="dc" if k == 0 else "ac", rs=rs, k=k, blk=blk, a=raw(p), c=raw(p + l), b=raw(p + l + size)))
        p += l + size
        if k == 0:
            k = 1
        elif size == 0:
            k = 64 if rs != 0xF0 else k + 16
        else:
            k += (rs >> 4) + 1
        if k >= 64:
            k, blk = 0, blk + 1
    return out


def cut_inside(lo, hi):
    """is a piece boundary strictly inside the raw bit span [lo, hi)?"""
    first = (lo // (8 * PIECE) + 1) * 8 * PIECE
    return lo < first < hi


def _noise_blocks(seed, n=12, amp=900):
    rs = np.random.RandomState(seed)
    b = np.zeros((n, 64), np.int64)
    b[:, 0] = rs.randint(-amp, amp + 1, n)
    for i in range(n):
        k = rs.randint(1, 64, 6)
        b[i, ZZ[k]] = rs.randint(-amp, amp + 1, 6)
    return b


def _search(make, ok, what, dc_sizes=11, ac_sizes=11):
    """the first shim (the size of block 0's DC difference and of its first AC coefficient) for which the stream has the property"""
    for s0 in range(0, dc_sizes):
        for s1 in range(0, ac_sizes):
            d = make((1 << s0) - 1, (1 << s1) - 1)
            if ok(d):
                return d
    raise AssertionError("no shim puts %s on a piece boundary" % what)


@functools.lru_cache(maxsize=None)
def boundary_case(name):
    ent = S.entropy_of
    if name == "ff00-straddles":  # FF as the last byte of a piece, its 00 the first of the next
        for seed in range(200):
            d = gray(_noise_blocks(seed))
            e = ent(d)
            if any(e[i] == 0xFF and e[i + 1] == 0 and (i + 1) % PIECE == 0 for i in range(len(e) - 3)):
                return d
        raise AssertionError("no stream with a stuffed pair across a boundary")
    long_tabs = {(0, 0): S.LONG_DC, (1, 0): S.LONG_AC}
    if name == "inside-16-bit-code":  # symbol 0x0A of LONG_AC: sixteen bits of code
        def make(v0, v1):
            b = np.zeros((4, 64), np.int64)
            b[0, 0], b[0, ZZ[1]] = v0, v1
            b[1, ZZ[1]], b[2, ZZ[1]], b[3, ZZ[1]] = 1023, -1023, 600
            return gray(b, long_tabs)
        return _search(make, lambda d: any(t["kind"] == "ac" and t["rs"] == 0x0A and cut_inside(t["a"], t["c"]) for t in trace(d)), name, 16, 6)
    if name == "inside-15-bit-value":  # DC differences of size 15 (LONG_DC has every size)
        def make(v0, v1):
            b = np.zeros((4, 64), np.int64)
            b[0, 0], b[0, ZZ[1]] = v0, v1
            b[1, 0], b[2, 0], b[3, 0] = 20000, -12000, 9000
            return gray(b, long_tabs)
        return _search(make, lambda d: any(t["kind"] == "dc" and t["rs"] == 15 and cut_inside(t["c"], t["b"]) for t in trace(d)), name, 16, 6)
    if name == "zrl-chain":  # three ZRL in a row, a boundary behind the first and before the last
        def make(v0, v1):
            b = np.zeros((3, 64), np.int64)
            b[0, 0], b[0, ZZ[1]] = v0, v1
            b[1, ZZ[63]] = 1
            b[2, ZZ[50]] = -2
            return gray(b)

        def ok(d):
            t = trace(d)
            for i in range(len(t) - 2):
                if all(x["kind"] == "ac" and x["rs"] == 0xF0 for x in t[i:i + 3]) and cut_inside(t[i]["b"] - 1, t[i + 2]["a"] + 1):
                    return True
            return False
        return _search(make, ok, name)
    if name == "no-eob-ends-on-boundary":  # coefficient 63 is set: the block ends at k = 64 without EOB, exactly on a boundary
        def make(v0, v1):
            b = np.zeros((4, 64), np.int64)
            b[0, 0], b[0, ZZ[1]] = v0, v1
            b[1, ZZ[62]], b[1, ZZ[63]] = 3, -1
            b[2, 0], b[2, ZZ[5]] = 40, 7
            b[3, ZZ[63]] = 2
            return gray(b)

        def ok(d):
            t = trace(d)
            return any(x["blk"] in (1, 3) and x["k"] + (x["rs"] >> 4) == 63 and x["b"] % (8 * PIECE) == 0 for x in t if x["kind"] == "ac")
        return _search(make, ok, name)
    base = gray(_noise_blocks(3, n=16))
    off = R.parse(base)["ent_off"]
    e = ent(base)
    assert len(e) > 12 * PIECE
    if name == "ends-in-first-piece":  # EOI after two bytes of data, the rest of the scan behind it
        return base[:off + 2] + b"\xff\xd9" + base[off + 2:]
    if name == "stray-eoi-in-the-middle":  # the data ends in a middle piece
        m = off + (len(e) // (2 * PIECE)) * PIECE + 1
        assert base[m - 1] != 0xFF
        return base[:m] + b"\xff\xd9" + base[m:]
    if name == "ends-in-last-piece":  # no EOI at all: the stream is cut inside its last blocks
        return base[:len(base) - 2 - PIECE - 1]
    if name == "bad-code-in-the-middle":  # 48 one bits where symbols were: no code; the scan's valid bytes go on behind them
        m = off + (len(e) // (2 * PIECE)) * PIECE + 2
        assert base[m - 1] != 0xFF
        return base[:m] + b"\xff\x00" * 6 + base[m + 12:]
    if name == "flat-8-bit-ac":  # every AC code has 8 bits: a lane out of step has no short code to fall back into step with
        return R.encode_image(S.scene(64, 48, 9), quality=92, sampling="gray", huff={(0, 0): R.STD_DC_LUM, (1, 0): FLAT_AC}, tsel=[(0, 0)])
    raise KeyError(name)


BOUNDARY = ("ff00-straddles", "inside-16-bit-code", "inside-15-bit-value", "zrl-chain", "no-eob-ends-on-boundary", "ends-in-first-piece",
            "stray-eoi-in-the-middle", "ends-in-last-piece", "bad-code-in-the-middle")
SLOW = "flat-8-bit-ac"


def no_dri_picture(w, h, sampling, seed=0, quality=90):
    return R.encode_image(S.scene(w, h, seed), quality=quality, sampling=sampling)
