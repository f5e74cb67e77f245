"""Every kernel of the lens units (k_warp_lens.hip, k_warp_lens_profile.hip) as the compiler reports it, with the build's own
flags: the one kernel template k_warp_lens<Src, FPT> yields exactly one one-frame and one many-frames form per source the
pipeline can run (both byte-map forms of WarpBgr, WarpProfile, WarpRaw and WarpRawProfile of the six YUV and four Bayer
layouts, WarpJpeg, WarpJpegProfile), and none of them uses scratch.  The VGPR counts are not held to 64 here: DESIGN.md
section 6r records them and says which forms lie above it.  No device is needed; the files are compiled for the device only
and nothing is written."""
import functools
import os
import re
import subprocess

import pytest

from chessboard_vision_amd import build as B

RAW_FORMATS = (0x01, 0x11, 0x21, 0x02, 0x12, 0x22, 0x04, 0x14, 0x24, 0x34)  # NV12 NV21 YUV420P YUYV YVYU UYVY and the four mosaics (YV12 runs as YUV420P)
UNITS = {
    "k_warp_lens.hip": {("7WarpBgrILb0EE", 4), ("7WarpBgrILb1EE", 4), ("11WarpProfile", 4), ("8WarpJpeg", 4)} | {("7WarpRawILi%dEE" % f, 4) for f in RAW_FORMATS},
    "k_warp_lens_profile.hip": {("15WarpJpegProfile", 2)} | {("14WarpRawProfileILi%dEE" % f, 2) for f in RAW_FORMATS},
}


@functools.lru_cache(maxsize=None)
def _remarks(unit):
    src = os.path.join(B.CSRC, unit)
    cmd = [B._hipcc(), *B.FLAGS, "--cuda-device-only", "-S", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for fn, body in re.findall(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", r.stderr, re.S):
        out[fn] = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", body)}
    return out


def _forms(unit):
    """{(mangled source type, frames per thread)} of the unit's kernels, which are all k_warp_lens<Src, FPT>"""
    forms = set()
    for name in _remarks(unit):
        m = re.match(r"_Z11k_warp_lensI(.+?)Li(\d+)EEvT_", name)
        assert m, name
        forms.add((m.group(1), int(m.group(2))))
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
