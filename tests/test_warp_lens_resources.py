"""Every kernel of the lens units (k_warp_lens.hip, k_warp_lens_profile.hip) as the compiler reports it, with the build's own
flags: the one kernel template k_warp_lens<Src, FPT> yields exactly one one-frame and one many-frames form per source the
pipeline can run (both byte-map forms of WarpBgr, WarpProfile, WarpRaw and WarpRawProfile of the six YUV and four Bayer
layouts, WarpJpeg, WarpJpegProfile), and none of them uses scratch.  The VGPR counts are not held to 64 here: DESIGN.md
section 6r records them and says which forms lie above it.  No device is needed; the files are compiled for the device only
and nothing is written."""
import pytest

import warp_kernels as W
from chessboard_vision_amd import build as B

RAW_FORMATS = (0x01, 0x11, 0x21, 0x02, 0x12, 0x22, 0x04, 0x14, 0x24, 0x34)  # NV12 NV21 YUV420P YUYV YVYU UYVY and the four mosaics (YV12 runs as YUV420P)
UNITS = {
    "k_warp_lens.hip": {(("WarpBgr", False), 4), (("WarpBgr", True), 4), ("WarpProfile", 4), ("WarpJpeg", 4)} | {(("WarpRaw", f), 4) for f in RAW_FORMATS},
    "k_warp_lens_profile.hip": {("WarpJpegProfile", 2)} | {(("WarpRawProfile", f), 2) for f in RAW_FORMATS},
}


_remarks = W.remarks


def _forms(unit):
    """{(source, frames per thread)} of the unit's kernels, which are all k_warp_lens<Src, FPT>"""
    forms = set()
    for name, src, arg, fpt in W.instances(unit):
        assert name == "k_warp_lens", name
        forms.add((src if arg is None else (src, arg), fpt))
    return forms


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_the_unit_yields_the_expected_lens_kernels(unit):
    want = UNITS[unit] | {(src, 1) for src, _ in UNITS[unit]}
    assert _forms(unit) == want and len(_remarks(unit)) == len(want)
    assert len(want) == (28 if unit == "k_warp_lens.hip" else 22)
    assert unit in B.SOURCES


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_no_lens_kernel_uses_scratch(unit):
    for name, v in _remarks(unit).items():
        assert v["ScratchSize"] == 0, (name, v)
        print(name, "VGPRs", v["VGPRs"], "occupancy", v.get("Occupancy"))
