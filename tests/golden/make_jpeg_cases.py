"""Pillow-encoded JPEG streams with Pillow's own decode of each (libjpeg-turbo with libjpeg's defaults: JDCT_ISLOW, fancy
upsampling; what cv2.imdecode calls), recorded into jpeg_cases.npz.  Needs Pillow; the tests that read the file do not.

    python tests/golden/make_jpeg_cases.py

matrix() is the full 504-case matrix (tests/test_jpeg_host.py decodes all of it live where Pillow is installed); every
fourth case of it is recorded, plus a standard-table file with its DHT segments stripped, which Pillow decodes to the same
bytes as the full file."""
import io
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "jpeg_cases.npz")

SIZES = [(1, 1), (3, 4), (4, 3), (8, 8), (9, 40), (16, 16), (17, 23), (33, 50)]  # (w, h)
CONTENTS = ("noise", "smooth", "saturated")
SAMPLINGS = ("444", "422", "420", "gray")


def content(kind, w, h, seed):
    rs = np.random.RandomState(seed)
    if kind == "noise":
        return rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "smooth":
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([(x * 7 + y * 3) % 256, (x * 2 + y * 5 + 40) % 256, (x + y) * 4 % 256], -1).astype(np.uint8)
    return (rs.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)


def matrix():
    """(name, w, h, content, sampling, quality, save options)"""
    out = []
    for w, h in SIZES:
        for kind in CONTENTS:
            for samp in SAMPLINGS:
                for q in (30, 90, 100):
                    out.append(("%dx%d-%s-%s-q%d" % (w, h, kind, samp, q), w, h, kind, samp, q, {}))
                if samp != "gray":
                    out.append(("%dx%d-%s-%s-q90-opt" % (w, h, kind, samp), w, h, kind, samp, 90, dict(optimize=True)))
                    out.append(("%dx%d-%s-%s-q90-rstmcu" % (w, h, kind, samp), w, h, kind, samp, 90, dict(restart_marker_blocks=1)))
                    out.append(("%dx%d-%s-%s-q90-rstrow" % (w, h, kind, samp), w, h, kind, samp, 90, dict(restart_marker_rows=1)))
    return out


def pillow_encode(case, index):
    """(stream bytes, Pillow's decode as BGR [h, w, 3])"""
    from PIL import Image
    name, w, h, kind, samp, q, opts = case
    img = content(kind, w, h, index)
    im = Image.fromarray(img[..., 0]) if samp == "gray" else Image.fromarray(np.ascontiguousarray(img[..., ::-1]))
    kw = dict(opts)
    if samp != "gray":
        kw["subsampling"] = {"444": 0, "422": 1, "420": 2}[samp]
    b = io.BytesIO()
    im.save(b, "JPEG", quality=q, **kw)
    data = b.getvalue()
    return data, pillow_decode(data)


def pillow_decode(data):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1])


def strip_dht(data):
    """the stream without its DHT segments"""
    d = bytes(data)
    out = bytearray(d[:2])
    i = 2
    while True:
        m, L = d[i + 1], d[i + 2] * 256 + d[i + 3]
        if m != 0xC4:
            out += d[i:i + 2 + L]
        i += 2 + L
        if m == 0xDA:
            return bytes(out + d[i:])


def main():
    cases = matrix()
    assert len(cases) == 504, len(cases)
    rec = {}
    names = []
    for i, case in enumerate(cases):
        if i % 4:
            continue
        data, bgr = pillow_encode(case, i)
        names.append(case[0])
        rec["data_%d" % (len(names) - 1)] = np.frombuffer(data, np.uint8)
        rec["bgr_%d" % (len(names) - 1)] = bgr
    # a standard-table (non-optimised) file without its DHT segments
    i = [c[0] for c in cases].index("33x50-noise-422-q90")
    data, bgr = pillow_encode(cases[i], i)
    stripped = strip_dht(data)
    assert b"\xff\xc4" not in stripped[:stripped.index(b"\xff\xda")]
    assert np.array_equal(pillow_decode(stripped), bgr), "Pillow decodes the DHT-stripped file differently"
    names.append("33x50-noise-422-q90-nodht")
    rec["data_%d" % (len(names) - 1)] = np.frombuffer(stripped, np.uint8)
    rec["bgr_%d" % (len(names) - 1)] = bgr
    np.savez_compressed(OUT, names=np.array(names), **rec)
    print(len(names), "cases,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
