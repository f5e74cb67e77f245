"""Baseline JPEG as include/cbv.h defines it (CBV_FMT_MJPEG), restated in numpy: the reference the host twin and the kernels
are held to, byte for byte.  No Pillow, no library code.  The entropy decode is a plain Python loop over bit strings, the IDCT
is vectorised over blocks in int64 and asserts that no intermediate leaves int32, the upsampling works on edge-padded planes.

Also here: an entropy ENCODER from coefficients (standard tables or tables the test gives, any of the accepted samplings,
DRI, extra segments, fill bytes, no DHT) and encode_image (float FDCT, IJG quality scaling), so that tests can build streams
that no library writes."""
import numpy as np

BAD_CODE, NO_DATA, RESTART = 1, 2, 4

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])

# T.81 Annex K.3: (bits[16], vals)
_DC_VALS = list(range(12))
STD_DC_LUM = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], _DC_VALS)
STD_DC_CHR = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], _DC_VALS)
STD_AC_LUM = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa])
STD_AC_CHR = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa])
STD_HUFF = {(0, 0): STD_DC_LUM, (0, 1): STD_DC_CHR, (1, 0): STD_AC_LUM, (1, 1): STD_AC_CHR}

# T.81 Annex K.1 / K.2 (row-major), scaled by quality as the IJG code does
Q_LUM = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                  18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
                  100, 103, 99])
Q_CHR = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                 + [99] * 32)

SAMPLINGS = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "gray": (1, 1)}


def quality_tables(quality):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [np.clip((t * s + 50) // 100, 1, 255).astype(np.int64) for t in (Q_LUM, Q_CHR)]


# --------------------------------------------------------------------------------------------------------------------
# header
# --------------------------------------------------------------------------------------------------------------------
def huff_codes(bits, vals):
    """{(length, code): symbol} of a canonical table"""
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out[(l, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return out


def parse(data):
    d = bytes(data)
    assert d[:2] == b"\xff\xd8"
    h = dict(q={}, huff={}, dri=0, any_dht=False)
    i = 2
    while True:
        assert d[i] == 0xFF
        while d[i] == 0xFF:
            i += 1
        m = d[i]
        i += 1
        L = d[i] * 256 + d[i + 1]
        s = d[i + 2:i + L]
        i += L
        if m == 0xC0:
            assert s[0] == 8
            h["h"], h["w"], nc = s[1] * 256 + s[2], s[3] * 256 + s[4], s[5]
            h["comps"] = [dict(id=s[6 + 3 * c], hs=s[7 + 3 * c] >> 4, vs=s[7 + 3 * c] & 15, tq=s[8 + 3 * c]) for c in range(nc)]
        elif m == 0xDB:
            p = 0
            while p < len(s):
                assert s[p] >> 4 == 0
                q = np.zeros(64, np.int64)
                q[ZIGZAG] = np.frombuffer(s[p + 1:p + 65], np.uint8)
                h["q"][s[p] & 15] = q
                p += 65
        elif m == 0xC4:
            p = 0
            while p < len(s):
                bits = list(s[p + 1:p + 17])
                n = sum(bits)
                h["huff"][(s[p] >> 4, s[p] & 15)] = huff_codes(bits, list(s[p + 17:p + 17 + n]))
                h["any_dht"] = True
                p += 17 + n
        elif m == 0xDD:
            h["dri"] = s[0] * 256 + s[1]
        elif m == 0xDA:
            assert s[0] == len(h["comps"])
            for c, comp in enumerate(h["comps"]):
                assert s[1 + 2 * c] == comp["id"]
                comp["td"], comp["ta"] = s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15
            break
        else:
            assert m not in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF), "not baseline"
    if not h["any_dht"]:
        h["huff"] = {k: huff_codes(*v) for k, v in STD_HUFF.items()}
    if len(h["comps"]) == 1:
        h["comps"][0]["hs"] = h["comps"][0]["vs"] = 1
    h["hmax"], h["vmax"] = h["comps"][0]["hs"], h["comps"][0]["vs"]
    h["mcux"] = -(-h["w"] // (8 * h["hmax"]))
    h["mcuy"] = -(-h["h"] // (8 * h["vmax"]))
    for comp in h["comps"]:
        comp["bw"], comp["bh"] = h["mcux"] * comp["hs"], h["mcuy"] * comp["vs"]
        comp["cw"] = -(-h["w"] * comp["hs"] // h["hmax"])
        comp["ch"] = -(-h["h"] * comp["vs"] // h["vmax"])
    nmcu = h["mcux"] * h["mcuy"]
    h["nint"] = -(-nmcu // h["dri"]) if h["dri"] else 1
    h["ent_off"] = i
    return h


# --------------------------------------------------------------------------------------------------------------------
# entropy decode
# --------------------------------------------------------------------------------------------------------------------
class _Bits:
    """the bits of one interval: FF 00 is FF, FF and anything else (or the end) ends the data, zero bits follow"""

    def __init__(self, seg):
        out, i = [], 0
        while i < len(seg):
            b = seg[i]
            i += 1
            if b == 0xFF:
                if i < len(seg) and seg[i] == 0:
                    i += 1
                else:
                    break
            out.append(b)
        self.s = "".join(format(b, "08b") for b in out)
        self.real = len(self.s)
        self.pos = 0

    def take(self, n):
        s = self.s[self.pos:self.pos + n]
        self.pos += n
        return int(s + "0" * (n - len(s)), 2) if n else 0

    def symbol(self, codes):
        for l in range(1, 17):
            s = self.s[self.pos:self.pos + l]
            key = (l, int(s + "0" * (l - len(s)), 2))
            if key in codes:
                self.pos += l
                return codes[key]
        return -1

    def extend(self, s):
        v = self.take(s)
        return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def _wrap16(v):
    return ((v + 32768) & 0xFFFF) - 32768


def _block(b, dc, ac, pred, out):
    s = b.symbol(dc)
    if s < 0 or s > 15:
        return pred, BAD_CODE
    if s:
        pred += b.extend(s)
    out[0] = _wrap16(pred)
    k = 1
    while k < 64:
        rs = b.symbol(ac)
        if rs < 0:
            return pred, BAD_CODE
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r != 15:
                break
            k += 16
            continue
        k += r
        if k > 63:
            return pred, BAD_CODE
        out[ZIGZAG[k]] = b.extend(s)
        k += 1
    return pred, 0


def decode_coefs(data, h):
    """[component] int16 [bh, bw, 64] (natural order) and the status word"""
    d = bytes(data)
    coefs = [np.zeros((c["bh"], c["bw"], 64), np.int16) for c in h["comps"]]
    st = 0
    e = len(d)
    marks = []
    if h["dri"]:
        hits = [i for i in range(h["ent_off"], e - 1) if d[i] == 0xFF and 0xD0 <= d[i + 1] <= 0xD7]
        if len(hits) != h["nint"] - 1:
            st |= RESTART
        marks = hits[:h["nint"] - 1]
        if any((d[p + 1] & 7) != (k & 7) for k, p in enumerate(marks)):
            st |= RESTART
    nmcu = h["mcux"] * h["mcuy"]
    for iv in range(h["nint"]):
        if iv > len(marks):
            seg = b""
        else:
            a = h["ent_off"] if iv == 0 else marks[iv - 1] + 2
            seg = d[a:(marks[iv] if iv < len(marks) else e)]
        b = _Bits(seg)
        m0 = iv * h["dri"] if h["dri"] else 0
        m1 = min(m0 + h["dri"], nmcu) if h["dri"] else nmcu
        pred = [0] * len(h["comps"])
        bad = 0
        for m in range(m0, m1):
            my, mx = divmod(m, h["mcux"])
            for c, comp in enumerate(h["comps"]):
                for by in range(comp["vs"]):
                    for bx in range(comp["hs"]):
                        out = np.zeros(64, np.int64)
                        pred[c], bad = _block(b, h["huff"][(0, comp["td"])], h["huff"][(1, comp["ta"])], pred[c], out)
                        coefs[c][my * comp["vs"] + by, mx * comp["hs"] + bx] = out.astype(np.int16)  # (what a bad block got so far stays)
                        if bad:
                            break
                    if bad:
                        break
                if bad:
                    break
            if bad:
                break
        st |= bad
        if b.pos > b.real:
            st |= NO_DATA
    return coefs, st


# --------------------------------------------------------------------------------------------------------------------
# IDCT, upsampling, colour
# --------------------------------------------------------------------------------------------------------------------
def _i32(x):
    assert x.size == 0 or (x.min() >= -2 ** 31 and x.max() <= 2 ** 31 - 1), "an intermediate leaves int32"
    return x


def _pass(v, shift):
    """jidctint's 8-point pass along the last axis of int64 v"""
    i = [v[..., k] for k in range(8)]
    z1 = _i32(_i32(i[2] + i[6]) * 4433)
    t2 = _i32(z1 + _i32(i[6] * -15137))
    t3 = _i32(z1 + _i32(i[2] * 6270))
    t0 = _i32(_i32(i[0] + i[4]) << 13)
    t1 = _i32(_i32(i[0] - i[4]) << 13)
    t10, t13, t11, t12 = _i32(t0 + t3), _i32(t0 - t3), _i32(t1 + t2), _i32(t1 - t2)
    a0, a1, a2, a3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = _i32(a0 + a3), _i32(a1 + a2), _i32(a0 + a2), _i32(a1 + a3)
    z5 = _i32(_i32(z3 + z4) * 9633)
    a0, a1, a2, a3 = _i32(a0 * 2446), _i32(a1 * 16819), _i32(a2 * 25172), _i32(a3 * 12299)
    z1, z2, z3, z4 = _i32(z1 * -7373), _i32(z2 * -20995), _i32(z3 * -16069), _i32(z4 * -3196)
    z3, z4 = _i32(z3 + z5), _i32(z4 + z5)
    a0 = _i32(_i32(a0 + z1) + z3)
    a1 = _i32(_i32(a1 + z2) + z4)
    a2 = _i32(_i32(a2 + z2) + z3)
    a3 = _i32(_i32(a3 + z1) + z4)
    r = 1 << (shift - 1)
    outs = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return np.stack([_i32(_i32(o) + r) >> shift for o in outs], axis=-1)


def idct_plane(coef, q):
    """int16 [bh, bw, 64] and q[64] (natural order) -> uint8 [bh * 8, bw * 8]"""
    bh, bw, _ = coef.shape
    v = _i32(coef.astype(np.int64) * q.astype(np.int64)).reshape(bh, bw, 8, 8)
    v = _pass(v.swapaxes(-1, -2), 11).swapaxes(-1, -2)  # columns
    v = _pass(v, 18)                                    # rows
    v = np.clip(v + 128, 0, 255).astype(np.uint8)
    return v.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def upsample_h2v1(p):
    """p: the component at its true size [ch, cw] -> [ch, 2 cw]"""
    p = p.astype(np.int64)
    e = np.pad(p, ((0, 0), (1, 1)), mode="edge")
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    out[:, 0::2] = (3 * p + e[:, :-2] + 1) >> 2
    out[:, 1::2] = (3 * p + e[:, 2:] + 2) >> 2
    return out


def upsample_h2v2(p):
    """[ch, cw] -> [2 ch, 2 cw]"""
    p = p.astype(np.int64)
    ev = np.pad(p, ((1, 1), (0, 0)), mode="edge")
    s = np.empty((2 * p.shape[0], p.shape[1]), np.int64)
    s[0::2] = 3 * p + ev[:-2]   # even output rows: the row above is nearer
    s[1::2] = 3 * p + ev[2:]
    e = np.pad(s, ((0, 0), (1, 1)), mode="edge")
    out = np.empty((s.shape[0], 2 * s.shape[1]), np.int64)
    out[:, 0::2] = (3 * s + e[:, :-2] + 8) >> 4
    out[:, 1::2] = (3 * s + e[:, 2:] + 7) >> 4
    return out


def _F(c):
    return int(c * 65536 + 0.5)


def ycc_to_bgr(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((_F(1.402) * cr + 32768) >> 16)
    b = y + ((_F(1.772) * cb + 32768) >> 16)
    g = y + ((-_F(0.34414) * cb - _F(0.71414) * cr + 32768) >> 16)
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def decode(data):
    """dict: bgr [h, w, 3], coef (int16, the components' [bh, bw, 64] arrays flattened back to back), planes (uint8, the padded
    planes back to back), status, header"""
    h = parse(data)
    coefs, st = decode_coefs(data, h)
    planes = [idct_plane(c, h["q"][comp["tq"]]) for c, comp in zip(coefs, h["comps"])]
    W, H = h["w"], h["h"]
    if len(planes) == 1:
        y = planes[0][:H, :W]
        bgr = np.stack([y, y, y], axis=-1)
    else:
        full = [planes[0][:H, :W]]
        for p, comp in zip(planes[1:], h["comps"][1:]):
            t = p[:comp["ch"], :comp["cw"]]
            if h["hmax"] == 2 and comp["cw"] <= 2:  # libjpeg-turbo filters only components more than 2 wide: these are replicated
                t = np.repeat(np.repeat(t, 2, axis=1), h["vmax"], axis=0)
            elif (h["hmax"], h["vmax"]) == (2, 1):
                t = upsample_h2v1(t)
            elif (h["hmax"], h["vmax"]) == (2, 2):
                t = upsample_h2v2(t)
            else:
                assert (h["hmax"], h["vmax"]) == (1, 1)
            full.append(t[:H, :W])
        bgr = ycc_to_bgr(*full)
    return dict(bgr=bgr, coef=np.concatenate([c.reshape(-1) for c in coefs]), planes=np.concatenate([p.reshape(-1) for p in planes]),
                status=st, header=h)


# --------------------------------------------------------------------------------------------------------------------
# encoder
# --------------------------------------------------------------------------------------------------------------------
def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def dht_payload(tables):
    """tables: {(class, id): (bits, vals)} -> one DHT payload holding all of them"""
    out = b""
    for (tc, th), (bits, vals) in sorted(tables.items()):
        out += bytes([tc << 4 | th]) + bytes(bits) + bytes(vals)
    return out


class _Writer:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _size(v):
    return int(abs(int(v))).bit_length()


def _put_value(wr, v, s):
    v = int(v)
    wr.put(v if v >= 0 else v + (1 << s) - 1, s)


def _encode_block(wr, blk, pred, dc, ac):
    """blk: 64 coefficients in natural order"""
    diff = int(blk[0]) - pred
    s = _size(diff)
    wr.put(*dc[s])
    if s:
        _put_value(wr, diff, s)
    zz = blk[ZIGZAG]
    prev = 0
    last = 0
    for k in np.flatnonzero(zz[1:]) + 1:
        k = int(k)
        run = k - prev - 1
        while run > 15:
            wr.put(*ac[0xF0])
            run -= 16
        s = _size(zz[k])
        wr.put(*ac[run << 4 | s])
        _put_value(wr, zz[k], s)
        prev = last = k
    if last < 63:
        wr.put(*ac[0x00])
    return int(blk[0])


def encode_coefs(coefs, w, h, sampling, qtabs, huff=None, dri=0, tq=None, tsel=None, omit_dht=False, split_dht=False, extra=(), fill=0,
                 rst_numbers=None):
    """A baseline stream from coefficients.  coefs: per component an integer array [bh, bw, 64] in natural order, whole
    MCUs.  sampling: "444" | "422" | "420" | "gray".  qtabs: {id: 64 values, natural order}; tq: the components' table ids
    (default 0, 1, 1).  huff: {(class, id): (bits, vals)}, default the standard tables; tsel: the components' (dc id, ac id)
    (default (0, 0), (1, 1), (1, 1)).  omit_dht: write no DHT (the tables must be the standard ones).  split_dht: one DHT
    segment per table instead of one for all.  extra: segments (marker, payload) written behind SOI.  fill: 0xFF bytes put
    before every marker of the header.  rst_numbers: the numbers written into the restart markers (default 0, 1, ... mod 8)."""
    nc = len(coefs)
    hs, vs = SAMPLINGS[sampling]
    huff = dict(STD_HUFF) if huff is None else huff
    tq = tq or [0, 1, 1][:nc]
    tsel = tsel or [(0, 0), (1, 1), (1, 1)][:nc]
    enc = {}
    for key, (bits, vals) in huff.items():
        enc[key] = {sym: (code, l) for (l, code), sym in huff_codes(bits, vals).items()}
    F = b"\xff" * fill
    out = bytearray(b"\xff\xd8")
    for m, payload in extra:
        out += F + _seg(m, payload)
    for i in sorted(set(tq)):
        q = np.asarray(qtabs[i])
        out += F + _seg(0xDB, bytes([i]) + bytes(int(v) for v in q[ZIGZAG]))
    comps = [(c + 1, (hs, vs) if c == 0 else (1, 1), tq[c]) for c in range(nc)]
    out += F + _seg(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([nc]) +
                    b"".join(bytes([cid, sh << 4 | sv, t]) for cid, (sh, sv), t in comps))
    if not omit_dht:
        used = {(0, d) for d, _ in tsel} | {(1, a) for _, a in tsel}
        tabs = {k: v for k, v in huff.items() if k in used}
        if split_dht:
            for k, v in sorted(tabs.items()):
                out += F + _seg(0xC4, dht_payload({k: v}))
        else:
            out += F + _seg(0xC4, dht_payload(tabs))
    if dri:
        out += F + _seg(0xDD, dri.to_bytes(2, "big"))
    out += F + _seg(0xDA, bytes([nc]) + b"".join(bytes([c + 1, tsel[c][0] << 4 | tsel[c][1]]) for c in range(nc)) + bytes([0, 63, 0]))
    mcuy, mcux = coefs[0].shape[0] // (vs if nc > 1 else 1), coefs[0].shape[1] // (hs if nc > 1 else 1)
    assert mcux == -(-w // (8 * (hs if nc > 1 else 1))) and mcuy == -(-h // (8 * (vs if nc > 1 else 1))), "coefficients are not whole MCUs of the size"
    wr = _Writer()
    pred = [0] * nc
    nmcu = mcux * mcuy
    nrst = 0
    for m in range(nmcu):
        if dri and m and m % dri == 0:
            wr.flush()
            out += wr.out
            wr = _Writer()
            out += bytes([0xFF, 0xD0 + ((rst_numbers[nrst] if rst_numbers else nrst) & 7)])
            nrst += 1
            pred = [0] * nc
        my, mx = divmod(m, mcux)
        for c in range(nc):
            ch, cv = ((hs, vs) if c == 0 else (1, 1)) if nc > 1 else (1, 1)
            for by in range(cv):
                for bx in range(ch):
                    pred[c] = _encode_block(wr, np.asarray(coefs[c][my * cv + by, mx * ch + bx]).astype(np.int64), pred[c],
                                            enc[(0, tsel[c][0])], enc[(1, tsel[c][1])])
    wr.flush()
    out += wr.out
    out += b"\xff\xd9"
    return bytes(out)


def _fdct_matrix():
    k = np.arange(8)
    C = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * 0.5
    C[0] *= 1 / np.sqrt(2)
    return C


def encode_image(bgr, quality=90, sampling="420", dri=0, **kw):
    """A baseline stream of a uint8 [h, w, 3] BGR image: JFIF colour conversion and float FDCT, box-filter chroma downsampling,
    IJG quality scaling, the standard Huffman tables.  Further arguments go to encode_coefs."""
    bgr = np.asarray(bgr)
    H, W = bgr.shape[:2]
    b, g, r = (bgr[..., i].astype(np.float64) for i in range(3))
    y = 0.299 * r + 0.587 * g + 0.114 * b
    if sampling == "gray":
        planes, facs = [y], [(1, 1)]
    else:
        cb = -0.168736 * r - 0.331264 * g + 0.5 * b + 128
        cr = 0.5 * r - 0.418688 * g - 0.081312 * b + 128
        planes, facs = [y, cb, cr], [(1, 1), SAMPLINGS[sampling], SAMPLINGS[sampling]]
    hs, vs = SAMPLINGS[sampling]
    mw, mh = 8 * hs, 8 * vs
    PW, PH = -(-W // mw) * mw, -(-H // mh) * mh
    ql, qc = quality_tables(quality)
    C = _fdct_matrix()
    coefs = []
    for i, (p, (fh, fv)) in enumerate(zip(planes, facs)):
        p = np.pad(p, ((0, PH - H), (0, PW - W)), mode="edge")
        if fh > 1 or fv > 1:
            p = p.reshape(PH // fv, fv, PW // fh, fh).mean(axis=(1, 3))
        bh, bw = p.shape[0] // 8, p.shape[1] // 8
        blocks = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128.0
        f = C @ blocks @ C.T
        q = (ql if i == 0 else qc).reshape(8, 8)
        coefs.append(np.rint(f / q).astype(np.int64).reshape(bh, bw, 64))
    return encode_coefs(coefs, W, H, sampling, {0: ql, 1: qc}, dri=dri, **kw)
