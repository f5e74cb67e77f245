"""The frame plan without a GPU (chessboard-vision_amd/csrc/frame_plan.h; DESIGN.md, "Where the frames live"): a stand-alone
program (tools/frame_plan_host.cpp), built with the host compiler under AddressSanitizer and UBSan, prints the plan of
every cell, four configuration kinds x {bgr, nv12, yuyv, bayer_rggb, mjpeg with planes off / gray / 4:2:0 / 4:2:2 / 4:4:4},
and the expected values are written out here: from the table of who reads what, from cbv_jpeg_probe's plane_elems for the
plane ring's slots (as tests/test_jpeg_planes_host.py does) and from include/cbv.h's rule for the decode scratch: depth
frames of 3 samples per pixel of the frame padded to 16 x 16 MCUs, ceil(w / 8) x ceil(h / 8) possible restart intervals, at
most ceil(slot bytes / S) pieces a frame and with segments one more per possible interval, 9 words a piece (10 with
segments) and with segments 3 words per possible interval and one more.  Nothing here calls the library's own sizing."""
import os
import shutil
import subprocess

import pytest

import test_jpeg_planes_host as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, S1, P, PR = range(4)
BGR, NV12, YUYV, RGGB, MJPEG = 0, 1, 2, 4, 8                       # include/cbv.h, CBV_FMT_*
PLANES = {0: None, 1: "gray", 2: "420", 3: "422", 4: "444"}        # CBV_JPEG_PLANES_*
AUTO, INTERVAL, PIECES, SEGMENTS = 0, 1, 2, 4                      # CBV_JPEG_ENTROPY_*
SIZES = [(16, 1), (1920, 1080)]  # at 16 x 1 a 4:2:0 slot is larger than a 4:2:2 one


def r256(n):
    return (n + 255) // 256 * 256


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("frame_plan") / "frame_plan_host"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "chessboard-vision_amd", "csrc"), os.path.join(ROOT, "tools", "frame_plan_host.cpp"),
                        "-o", str(out)], capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler has no sanitizer runtime: %s" % r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    return str(out)


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout.splitlines()


def expected(kind, fmt, planes, w, h, slot_bytes, entropy, piece_bytes, depth):
    mjpeg = fmt == MJPEG
    raw_kind, y, j1 = kind in (S1, PR), fmt in (NV12, YUYV, RGGB), mjpeg and planes != 0
    e = {}
    e["source"] = (2 if j1 else 1) if raw_kind and (y or j1) else 0               # BGR ring, raw ring, plane ring
    e["bgr"] = int(not ((kind == PR and y) or (raw_kind and j1)))                 # S1 keeps an idle one beside the raw ring
    e["slot"] = (slot_bytes or r256((w * h + 1) // 2)) if mjpeg else r256({BGR: w * h * 3, NV12: w * h * 3 // 2, YUYV: w * h * 2, RGGB: w * h}[fmt])
    e["pmode"] = planes if mjpeg else 0                                           # in all four kinds: idle under E and P
    e["pslot"] = r256(max(TP._plane_elems(w, h, s) for s in TP.ADMITS[PLANES[planes]])) if j1 else 0
    S = 0 if entropy == INTERVAL else piece_bytes or 64
    seg = int(entropy == SEGMENTS)
    e["S"], e["seg"] = S, seg
    maxint = -(-w // 8) * -(-h // 8)
    cap = (-(-e["slot"] // S) + (maxint if seg else 0)) if S and mjpeg else 0
    e["depth"] = depth if mjpeg else 0
    e["own"] = int(mjpeg and not (raw_kind and j1))                               # there the decode writes the plane ring
    e["elems"] = 3 * (-(-w // 16) * 16) * (-(-h // 16) * 16) if mjpeg else 0
    e["maxint"] = maxint if mjpeg else 0
    e["cap"] = cap
    e["pwords"] = cap * (10 if seg else 9)
    e["swords"] = 3 * maxint + 1 if seg and mjpeg else 0
    return e


SETTINGS = [(0, AUTO, 0, 8), (0, INTERVAL, 0, 8), (0, PIECES, 32, 1), (0, SEGMENTS, 0, 3), (100096, SEGMENTS, 4, 64), (1 << 30, AUTO, 4, 8)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("settings", SETTINGS, ids=lambda s: "slot%d-entropy%d-piece%d-depth%d" % s)
def test_every_cell(exe, size, settings):
    w, h = size
    lines = run(exe, w, h, *settings)
    cells = [(k, f, p) for k in (E, S1, P, PR) for f in (BGR, NV12, YUYV, RGGB, MJPEG) for p in range(5) if f == MJPEG or p in (0, 4)]
    assert len(cells) == 4 * 13 and len(lines) == len(cells)
    for (k, f, p), line in zip(cells, lines):
        word = line.split()
        assert [int(x) for x in word[:3]] == [k, f, p], line
        got = {a.split("=")[0]: int(a.split("=")[1]) for a in word[3:]}
        assert got == expected(k, f, p, w, h, *settings), (line, expected(k, f, p, w, h, *settings))


def test_the_table_in_words(exe):
    """a few cells spelled out, so that a slip in expected() above cannot hide one in the header"""
    got = {tuple(int(x) for x in l.split()[:3]): l for l in run(exe, 1920, 1080, 0, AUTO, 0, 8)}
    assert "source=0 bgr=1 slot=6220800 " in got[(E, BGR, 0)]
    assert "source=1 bgr=1 slot=3110400 " in got[(S1, NV12, 0)] and "source=1 bgr=0 slot=3110400 " in got[(PR, NV12, 0)]
    assert "source=0 bgr=1 slot=2073600 " in got[(P, RGGB, 0)] and "source=0 bgr=1 slot=4147200 " in got[(E, YUYV, 0)]
    assert "source=0 bgr=1 slot=1036800 pmode=0 pslot=0 S=64 seg=0 depth=8 own=1 elems=6266880 maxint=32400 cap=16200 pwords=145800 swords=0" in got[(S1, MJPEG, 0)]
    assert "source=2 bgr=0 slot=1036800 pmode=4 pslot=6220800 " in got[(S1, MJPEG, 4)] and " own=0 " in got[(PR, MJPEG, 4)]
    assert "source=0 bgr=1 slot=1036800 pmode=2 pslot=3133440 " in got[(E, MJPEG, 2)] and " own=1 " in got[(P, MJPEG, 2)]
    small = {tuple(int(x) for x in l.split()[:3]): l for l in run(exe, 16, 1, 0, AUTO, 0, 8)}
    assert " pslot=512 " in small[(S1, MJPEG, 3)] and " pslot=512 " in small[(S1, MJPEG, 2)] and " pslot=256 " in small[(S1, MJPEG, 1)]


def test_the_entropy_settings_that_are_refused(exe):
    """what cbv_jpeg_decode_host_ex refuses (tests/test_jpeg_segments_host.py: modes 3 and 5, pieces of 2, 6 and 2^25 bytes)"""
    pairs = [(0, 0), (1, 0), (2, 0), (4, 0), (2, 4), (4, 1 << 24), (1, 12), (3, 0), (5, 0), (-1, 0), (4, 2), (2, 6), (4, (1 << 24) + 4), (0, 1 << 25), (0, 3)]
    lines = run(exe, "--piece-size", *[x for p in pairs for x in p])
    assert len(lines) == len(pairs)
    for (mode, bytes_), line in zip(pairs, lines):
        if mode not in (0, 1, 2, 4):
            assert line == "%d %d refused -1 entropy mode %d" % (mode, bytes_, mode)
        elif bytes_ and (bytes_ < 4 or bytes_ % 4 or bytes_ > 1 << 24):
            assert line == "%d %d refused -1 pieces of %d bytes (a multiple of 4, from 4 to 2^24, or 0 for the default)" % (mode, bytes_, bytes_)
        else:
            assert line == "%d %d S=%d seg=%d" % (mode, bytes_, 0 if mode == 1 else bytes_ or 64, mode == 4)
    # ... and the plan of every cell refuses them too, whatever the format
    for mode, bytes_ in ((3, 0), (4, 6)):
        for line in run(exe, 16, 1, 0, mode, bytes_, 8):
            assert " refused -1 " in line, line
