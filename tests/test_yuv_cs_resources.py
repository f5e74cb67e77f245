"""Every kernel of the units that hold the runtime-matrix YUV forms (colour spaces 1 to 3: k_ingest_cs.hip, k_warp_cs.hip,
k_warp_lens_cs.hip) as the compiler reports it, with the build's own flags.  Per YUV layout the kernels know (six: YV12 is
launched as yuv420p):
  k_ingest_cs.hip      12 = 6 layouts x {dword path, byte path}
  k_warp_cs.hip        48 = 6 layouts x {k_warp_one, k_warp_boards} x {WarpRawCs, WarpRawProfileCs}
                            x {one frame a thread, the many-frames form}
  k_warp_lens_cs.hip   24 = 6 layouts x k_warp_lens x {WarpRawCs, WarpRawProfileCs} x {one frame a thread, the many-frames form}
The many-frames forms: four frames without a profile, planar 4:2:0 two (its four-frame form needs 65 VGPRs once the constants
are the launch's); with a profile what the siblings take (four, planar 4:2:0 two; two with a lens).  None uses scratch; the
forms without a profile stay at or under 64 VGPRs (8 waves per SIMD, as k_warp.hip's) and use no LDS; the profile forms stage
the 7 680 B of the profile's tables and nothing else, and their one-frame forms stay at or under 64 VGPRs like their siblings'.
No device is needed; the files are compiled for the device only and nothing is written."""
import re

import pytest

import warp_kernels as W
from chessboard_vision_amd import _native as N
from chessboard_vision_amd import build as B

YUV = {k: v for k, v in N.FORMATS.items() if k not in ("bgr", "yv12")}
PLANAR = N.FMT_YUV420P
UNITS = ("k_ingest_cs.hip", "k_warp_cs.hip", "k_warp_lens_cs.hip")


def _remarks(unit):
    """(kernel, format id, second template number) -> figures of k_ingest_cs.hip; (kernel template, source, format id, frames
    per thread) -> figures of the warp units"""
    if unit != "k_ingest_cs.hip":
        return W.instances(unit)
    return {_ingest_instance(n): v for n, v in W.remarks(unit).items()}


def _ingest_instance(mangled):
    """(kernel, format id, second template number) of _Z<len><name>ILi<fmt>ELi<n>EE..."""
    m = re.match(r"_Z(\d+)", mangled)
    name, rest = mangled[m.end():m.end() + int(m.group(1))], mangled[m.end() + int(m.group(1)):]
    a = re.match(r"ILi(\d+)ELi(\d+)E", rest)
    return name, int(a.group(1)), int(a.group(2))


def _many(fmt, profile, lens=False):
    if profile:
        return 2 if lens or fmt == PLANAR else 4
    return 2 if fmt == PLANAR else 4


def test_the_units_are_in_the_build():
    assert all(u in B.SOURCES for u in UNITS) and "cbv_yuv.h" in B.HEADERS and "warp_gather.h" in B.HEADERS and "warp_lens.h" in B.HEADERS


def test_the_exact_kernel_lists():
    want = sorted(("k_ingest_cs", f, px) for f in YUV.values() for px in (2, 4))
    assert sorted(_remarks("k_ingest_cs.hip")) == want and len(want) == 12
    want = sorted((k, s, f, fpt) for f in YUV.values() for k in ("k_warp_one", "k_warp_boards") for s in ("WarpRawCs", "WarpRawProfileCs")
                  for fpt in (1, _many(f, "Profile" in s)))
    assert sorted(_remarks("k_warp_cs.hip")) == want and len(want) == 48
    want = sorted(("k_warp_lens", s, f, fpt) for f in YUV.values() for s in ("WarpRawCs", "WarpRawProfileCs") for fpt in (1, _many(f, "Profile" in s, lens=True)))
    assert sorted(_remarks("k_warp_lens_cs.hip")) == want and len(want) == 24


@pytest.mark.parametrize("unit", UNITS)
def test_no_scratch_registers_and_lds(unit):
    for key, v in _remarks(unit).items():
        name, f, n = key[-3:]  # (a warp kernel: its source)
        profile = "rofile" in name
        assert v["ScratchSize"] == 0, (name, f, n, v)
        assert v["LDS Size"] == (7680 if profile else 0), (name, f, n, v)
        if not profile or n == 1:
            assert v["VGPRs"] <= 64, (name, f, n, v)
