"""The colour spaces of a YUV frame without a GPU (include/cbv.h, CBV_CS_*; tests/ref64_yuv_cs.py): the integers of the
table against the exact fractions, the int form against the float64 form over all 2^24 triples, the 32-bit bound, row 0
against ref64_yuv, the refusals the Python layer makes before the library is called, the constants of cbv.h against
_native.py, and the frame plan, which does not depend on the colour space."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ref64_yuv as R
import ref64_yuv_cs as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the triples on which the int form and the float64 form differ (by 1, in one channel): the exact ties of the fractions
DIFFER = {"bt601-full": 8940, "bt709": 1315, "bt709-full": 0}


def _cube_planes():
    """every (Y, U, V) triple once, as 256 slabs of one Y each"""
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for y in range(256):
        yield np.full_like(u, y), u, v


@pytest.mark.parametrize("cs", RC.NEW)
def test_the_integers_are_the_rounded_fractions(cs):
    yoff, *coef = RC.exact(cs)
    want = (yoff,) + tuple(int(round(c * (1 << RC.SHIFT))) for c in coef)   # Fraction.__round__: half to even; no tie occurs
    assert all((c * (1 << RC.SHIFT)).denominator != 2 for c in coef)
    assert RC.TABLE[cs] == want, (cs, want)


@pytest.mark.parametrize("cs", RC.NEW)
def test_int_and_float_forms_over_all_triples_and_the_32_bit_bound(cs):
    differ, worst, most = 0, 0, 0
    for Y, U, V in _cube_planes():
        got, ext = RC.yuv_to_bgr_int(Y, U, V, cs, with_extremes=True)
        d = np.abs(got.astype(np.int16) - RC.yuv_to_bgr_float(Y, U, V, cs))
        worst = max(worst, int(d.max()))
        assert int((d.sum(axis=-1) > 1).sum()) == 0   # one channel at a time
        differ += int(d.any(axis=-1).sum())
        most = max(most, ext)
    assert worst <= 1 and differ == DIFFER[cs], (cs, worst, differ)
    assert most < 2 ** 31 and most <= 575851935, (cs, most)
    if cs == "bt709":
        assert most == 573636921   # the largest any sum reaches over the triples, BT.709 limited's B


def test_the_bound_of_the_table():
    """the largest magnitude a sum could reach, from the constants alone: BT.709 limited, B"""
    bounds = {cs: (255 - t[0]) * t[1] + (1 << 19) + 128 * max(t[2], -(t[3] + t[4]), t[5]) for cs, t in RC.TABLE.items()}
    assert max(bounds.values()) == bounds["bt709"] == 575851935 < 2 ** 31


def test_row_0_is_ref64_yuv():
    assert RC.TABLE["bt601"][1:] == (R.CY, R.CUB, R.CUG, R.CVG, R.CVR)
    rng = np.random.default_rng(5)
    Y, U, V = (rng.integers(0, 256, (64, 4096), dtype=np.uint8) for _ in range(3))
    assert np.array_equal(RC.yuv_to_bgr_int(Y, U, V, "bt601"), R.yuv_to_bgr_int(Y, U, V))
    for Yc, Uc, Vc in list(_cube_planes())[::17]:
        assert np.array_equal(RC.yuv_to_bgr_int(Yc, Uc, Vc, "bt601"), R.yuv_to_bgr_int(Yc, Uc, Vc))


@pytest.mark.parametrize("fmt", RC.LAYOUTS)
def test_generators_and_splitters_round_trip(fmt):
    """from_bgr -> to_bgr comes back near a smooth image in every colour space (inputs only: a sanity check of the helper)"""
    yy, xx = np.mgrid[:16, :24]
    bgr = np.stack([40 + 6 * xx, 60 + 8 * yy, 200 - 5 * xx], axis=-1).astype(np.uint8)
    for cs in RC.NAMES:
        back = RC.to_bgr(RC.from_bgr(bgr, fmt, cs), fmt, cs)
        assert np.abs(back.astype(int) - bgr).max() <= 12, (fmt, cs)


def test_python_refusals_before_the_library_is_called():
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.board_detection import warp_perspective_profiled, yuv_to_bgr
    nv12 = np.zeros((6, 4), np.uint8)
    with pytest.raises(ValueError, match="unknown colour space"):
        yuv_to_bgr(nv12, "nv12", colorspace="bt2020")
    with pytest.raises(ValueError, match="unknown colour space"):
        N.colorspace_bits(None, "nv12")
    for fmt in ("bgr", "bayer_rggb", "mjpeg"):
        with pytest.raises(ValueError, match="YUV formats"):
            N.colorspace_bits("bt709", fmt)
        assert N.colorspace_bits("bt601", fmt) == 0
    with pytest.raises(ValueError, match="YUV formats"):
        warp_perspective_profiled(np.zeros((4, 4), np.uint8), np.eye(3), (4, 4), None, fmt="bayer_rggb", colorspace="bt709-full")
    with pytest.raises(ValueError, match="YUV formats"):
        warp_perspective_profiled(np.zeros((4, 4, 3), np.uint8), np.eye(3), (4, 4), None, colorspace="bt601-full")
    with pytest.raises(ValueError, match="YUV formats"):
        warp_perspective_profiled(b"", np.eye(3), (4, 4), None, fmt="mjpeg", colorspace="bt709")
    for cs in RC.NAMES:
        for fmt in RC.LAYOUTS:
            assert N.colorspace_bits(cs, fmt) == RC.BITS[cs]
    r, w, h, keep = N.raw_frame(nv12, "nv12", "bt709-full")
    assert (r.fmt, w, h) == (N.FMT_NV12 | 0xC00, 4, 4)
    assert N.raw_frame(nv12, "nv12")[0].fmt == N.FMT_NV12


def test_the_header_and_the_python_constants_agree():
    from chessboard_vision_amd import _native as N
    text = open(os.path.join(ROOT, "include", "cbv.h")).read()
    got = {k: int(v, 16) for k, v in re.findall(r"#define\s+(CBV_CS_\w+)\s+(0x[0-9a-fA-F]+)", text)}
    assert got == {"CBV_CS_FULL": 0x400, "CBV_CS_BT709": 0x800, "CBV_CS_MASK": 0xC00}
    assert (N.CS_FULL, N.CS_BT709, N.CS_MASK) == (got["CBV_CS_FULL"], got["CBV_CS_BT709"], got["CBV_CS_MASK"])
    assert N.COLORSPACES == RC.BITS and tuple(N.COLORSPACES) == RC.NAMES
    assert all(b & ~N.CS_MASK == 0 for b in N.COLORSPACES.values())
    assert all(f & N.CS_MASK == 0 for f in list(N.FORMATS.values()) + list(N.BAYER_FORMATS.values()) + [N.FMT_MJPEG])


def test_the_table_of_the_kernels_is_the_table():
    """cbv_yuv.h's rows, read as text: (cy, cub, cug, cvg, cvr, yoff) of rows 1 to 3; row 0 names the enum of colour space 0"""
    text = open(os.path.join(ROOT, "chessboard-vision_amd", "csrc", "cbv_yuv.h")).read()
    body = text[text.index("kYuvCs[4]"):]
    rows = re.findall(r"\{(-?\d+), (-?\d+), (-?\d+), (-?\d+), (-?\d+), (\d+)\}", body)
    assert [tuple(int(x) for x in r) for r in rows] == [RC.TABLE[cs][1:] + RC.TABLE[cs][:1] for cs in RC.NEW]
    assert "{YUV_CY, YUV_CUB, YUV_CUG, YUV_CVG, YUV_CVR, 16}" in body


def test_the_frame_plan_does_not_depend_on_the_colour_space(tmp_path):
    """tools/frame_plan_host.cpp with a colour space as its seventh argument prints the lines it prints without one"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "frame_plan_host")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "chessboard-vision_amd", "csrc"),
                        os.path.join(ROOT, "tools", "frame_plan_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for size in ((16, 2), (1920, 1080)):
        args = [str(a) for a in size + (0, 0, 0, 8)]
        plain = subprocess.run([exe] + args, capture_output=True, text=True, check=True).stdout
        assert len(plain.splitlines()) == 52
        for cs in (1, 2, 3):
            assert subprocess.run([exe] + args + [str(cs)], capture_output=True, text=True, check=True).stdout == plain, (size, cs)
