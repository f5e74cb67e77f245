"""The 8-bit Bayer formats, the parts that need no GPU: the two restatements of the definition against each other and
against hand-written values, the identities between the layouts, the format ids against gcc, N.raw_frame's shapes and
refusals, and the argument checks of the entry points."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ref64_bayer as RB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = RB.SHAPES + [(1920, 1080)]


@pytest.mark.parametrize("fmt", RB.FORMATS)
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_two_restatements_agree(fmt, size):
    """float64 mean of the nearest samples, rounded half up == the integer sums and shifts"""
    w, h = size
    yy, xx = np.mgrid[0:h, 0:w]
    frames = dict(RB.inputs(w, h))
    frames["ramp"] = ((xx * 5 + yy * 3) & 255).astype(np.uint8)
    frames["two_level"] = (np.random.default_rng(w + h).integers(0, 2, (h, w)) * 255).astype(np.uint8)
    for name, f in frames.items():
        a, b = RB.to_bgr(f, fmt), RB.to_bgr_int(f, fmt)
        assert a.shape == (h, w, 3) and a.dtype == np.uint8
        assert np.array_equal(a, b), (fmt, name)


# one 4 x 4 mosaic; per layout the four interior results (sites (1,1), (2,1), (1,2), (2,2)) as B, G, R, worked out by hand
# from include/cbv.h.  At (1,1): centre 100, cross 125, diagonal 61, row pair 129, column pair 121; at (2,1): 251, 54, 147,
# 82, 26; at (1,2): 41, 112, 85, 99, 125; at (2,2): 18, 156, 79, 148, 164.
HAND = np.array([[12, 200, 33, 90], [7, 100, 251, 64], [180, 41, 18, 255], [5, 150, 77, 0]], np.uint8)
HAND_BGR = {
    "bayer_rggb": ((100, 125, 61), (82, 251, 26), (125, 41, 99), (79, 156, 18)),      # B site, G in a blue row, G in a red row, R site
    "bayer_bggr": ((61, 125, 100), (26, 251, 82), (99, 41, 125), (18, 156, 79)),
    "bayer_grbg": ((129, 100, 121), (251, 54, 147), (85, 112, 41), (164, 18, 148)),   # G in a blue row, B site, R site, G in a red row
    "bayer_gbrg": ((121, 100, 129), (147, 54, 251), (41, 112, 85), (148, 18, 164)),
}


@pytest.mark.parametrize("fmt", RB.FORMATS)
def test_hand_written_4x4(fmt):
    a, b, c, d = HAND_BGR[fmt]
    want = np.array([[a, a, b, b], [a, a, b, b], [c, c, d, d], [c, c, d, d]], np.uint8)   # the edge copies its neighbour
    assert np.array_equal(RB.to_bgr(HAND, fmt), want)
    assert np.array_equal(RB.to_bgr_int(HAND, fmt), want)


def test_block_table_is_the_names():
    letters = "BGR"
    for fmt in RB.FORMATS:
        (a, b), (c, d) = RB.BLOCK[fmt]
        assert (letters[a] + letters[b] + letters[c] + letters[d]).lower() == fmt[-4:]
        m = RB.mosaic(np.dstack([np.full((4, 4), v, np.uint8) for v in (10, 20, 30)]), fmt)     # B = 10, G = 20, R = 30
        assert [int(m[0, 0]), int(m[0, 1]), int(m[1, 0]), int(m[1, 1])] == [(10, 20, 30)[i] for i in (a, b, c, d)]


@pytest.mark.parametrize("fmt", RB.FORMATS)
def test_constant_colour_survives(fmt):
    for w, h in [(4, 4), (6, 8), (10, 6)]:
        for colour in [(0, 0, 0), (255, 255, 255), (13, 200, 77), (255, 0, 128)]:
            bgr = np.empty((h, w, 3), np.uint8)
            bgr[:] = colour
            assert np.array_equal(RB.to_bgr(RB.mosaic(bgr, fmt), fmt), bgr)


def test_swap_identities():
    rng = np.random.default_rng(5)
    for w, h in [(4, 4), (8, 6), (64, 48)]:
        f = rng.integers(0, 256, (h, w), dtype=np.uint8)
        assert np.array_equal(RB.to_bgr(f, "bayer_rggb"), RB.to_bgr(f, "bayer_bggr")[:, :, ::-1])
        assert np.array_equal(RB.to_bgr(f, "bayer_grbg"), RB.to_bgr(f, "bayer_gbrg")[:, :, ::-1])
    # grbg of a frame is rggb of the frame shifted by one column, in the interior
    big = rng.integers(0, 256, (12, 18), dtype=np.uint8)
    a = RB.to_bgr(big[:, 1:17], "bayer_grbg")       # columns 1 .. 16 of `big`: its column 1 is a G of a G R row when big is RGGB
    b = RB.to_bgr(big[:, 0:16], "bayer_rggb")
    assert np.array_equal(a[1:-1, 1:-2], b[1:-1, 2:-1])
    a = RB.to_bgr(big[:, 1:17], "bayer_gbrg")
    b = RB.to_bgr(big[:, 0:16], "bayer_bggr")
    assert np.array_equal(a[1:-1, 1:-2], b[1:-1, 2:-1])


def test_header_ids_against_gcc(tmp_path):
    from chessboard_vision_amd import _native as N
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include "cbv.h"', 'int main(void) {']
    for py in RB.FORMATS:
        lines.append('printf("%s %%d\\n", CBV_FMT_%s);' % (py, py.upper()))
    lines += ["return 0;", "}"]
    src = tmp_path / "bayer_ids.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "bayer_ids"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = {k: int(v) for k, v in (l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    assert got == RB.IDS == N.BAYER_FORMATS
    for py, i in RB.IDS.items():
        assert i & 15 == 4
        assert bool(i & 0x10) == (py in ("bayer_bggr", "bayer_gbrg")) and bool(i & 0x20) == (py in ("bayer_grbg", "bayer_gbrg"))
        assert N.format_id(py) == N.format_id(py.upper()) == i
    assert (N.FMT_BAYER_RGGB, N.FMT_BAYER_BGGR, N.FMT_BAYER_GRBG, N.FMT_BAYER_GBRG) == (0x04, 0x14, 0x24, 0x34)


def test_formats_table_keeps_its_eight_entries():
    from chessboard_vision_amd import _native as N
    assert set(N.FORMATS) == {"bgr", "nv12", "yuyv", "nv21", "yuv420p", "yv12", "yvyu", "uyvy"}
    assert not set(N.FORMATS) & set(N.BAYER_FORMATS) and not set(N.FORMATS.values()) & set(N.BAYER_FORMATS.values())
    for bad in (0x04, 4, None, "bayer", "bayer_rgbg", "rggb", "bayer_rggb8"):
        with pytest.raises(ValueError):
            N.format_id(bad)


def _addr(a):
    return a.__array_interface__["data"][0]


def test_raw_frame_accepts_and_refuses():
    from chessboard_vision_amd import _native as N
    big = np.zeros((12, 19), np.uint8)
    for fmt in RB.FORMATS:
        r, w, h, keep = N.raw_frame(big[:8, :10], fmt)                   # a view: kept in place, its stride kept
        assert (r.fmt, w, h, r.stride0, r.plane0) == (RB.IDS[fmt], 10, 8, 19, _addr(big)) and not r.plane1 and not r.plane2
        r, w, h, keep = N.raw_frame(big[2:6, 3:7], fmt.upper())
        assert (w, h, r.stride0, r.plane0) == (4, 4, 19, _addr(big) + 2 * 19 + 3)
        r, w, h, keep = N.raw_frame(big[:4, 0:16:2], fmt)                # bytes of a row not adjacent: copied
        assert (w, h, r.stride0) == (8, 4, 8) and not _addr(big) <= r.plane0 < _addr(big) + big.size
        r, w, h, keep = N.raw_frame(np.zeros((6, 4), np.uint8), fmt)
        assert (w, h, r.stride0) == (4, 6, 4)
    u8 = lambda *s: np.zeros(s, np.uint8)
    bad = [(u8(6, 7), "7"), (u8(5, 8), "5"), (u8(2, 8), "(2, 8)"), (u8(8, 2), "(8, 2)"),      # odd, below 4
           (u8(6, 8, 1), "(6, 8, 1)"), (u8(6, 8, 3), "(6, 8, 3)"),                           # rank 3
           (np.zeros((6, 8), np.uint16), "uint16"), (np.zeros((6, 8), np.float32), "float32"),
           ((u8(6, 8),), "1 planes"), ((u8(6, 8), u8(3, 8)), "2 planes")]
    for fmt in RB.FORMATS:
        for frame, text in bad:
            with pytest.raises(ValueError) as e:
                N.raw_frame(frame, fmt)
            assert text in str(e.value), (fmt, text, str(e.value))


def test_python_entry_points_without_a_device():
    from chessboard_vision_amd.board_detection import bayer_to_bgr, yuv_to_bgr
    from chessboard_vision_amd.stream import BoardPipeline
    with pytest.raises(ValueError) as e:
        yuv_to_bgr(np.zeros((4, 4), np.uint8), "bayer_rggb")
    assert "bayer_to_bgr" in str(e.value)
    for fmt in ("nv12", "bgr", "bayer", 4):
        with pytest.raises(ValueError):
            bayer_to_bgr(np.zeros((6, 4), np.uint8), fmt)
    with pytest.raises(ValueError):
        bayer_to_bgr(np.zeros((5, 4), np.uint8), "bayer_grbg")
    from chessboard_vision_amd import _native as N
    for f in (N.format_id, N.raw_frame, bayer_to_bgr, BoardPipeline.upload, BoardPipeline.set_input_format):
        assert "bayer_rggb" in f.__doc__, f.__name__
    assert "bayer_to_bgr" in yuv_to_bgr.__doc__ and "[max_frames, h, w]" in BoardPipeline.host_ring.__doc__


def test_null_handles_are_refused_with_the_functions_name():
    from chessboard_vision_amd import _native as N
    lib = N.load()
    out = np.zeros((4, 4, 3), np.uint8)
    for fmt in RB.FORMATS:
        raw = N.raw_frame(np.zeros((4, 4), np.uint8), fmt)[0]
        assert lib.cbv_yuv_to_bgr(None, raw, 4, 4, N.ptr(out), 12) == -1
        assert b"cbv_yuv_to_bgr" in lib.cbv_last_error(None)
        assert lib.cbv_pipeline_set_input_format(None, RB.IDS[fmt]) == -1
        assert b"cbv_pipeline_set_input_format" in lib.cbv_last_error(None)
        assert lib.cbv_pipeline_upload_raw(None, 0, raw) == -1
        assert b"cbv_pipeline_upload_raw" in lib.cbv_last_error(None)
