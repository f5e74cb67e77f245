"""The Bayer kernels' registers as the compiler reports them, with the build's own flags: every Bayer instantiation of
k_ingest, k_warp_bayer and k_warp_bayer_mb runs without scratch, and the warp forms stay at or under 64 VGPRs, the line
DESIGN.md section 4 gives for running beside the squares and HoughCircles kernels at 8 waves per SIMD.
No device is needed; the files are compiled for the device only and nothing is written."""
import functools
import os
import re
import subprocess

import pytest

from chessboard_vision_amd import build as B

IDS = (0x04, 0x14, 0x24, 0x34)


@functools.lru_cache(maxsize=None)
def _remarks(name):
    src = os.path.join(B.CSRC, name)
    cmd = [B._hipcc(), *B.FLAGS, "--cuda-device-only", "-S", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for fn, body in re.findall(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", r.stderr, re.S):
        out[fn] = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", body)}
    return out


def _instances(remarks, kernel, second):
    """mangled name -> figures of kernel<id, second> for the four Bayer ids"""
    found = {}
    for i in IDS:
        for s in second:
            tag = "%d%sILi%dELi%dEE" % (len(kernel), kernel, i, s)
            hits = [n for n in remarks if tag in n]
            assert len(hits) == 1, (tag, sorted(remarks))
            found[hits[0]] = remarks[hits[0]]
    return found


def test_ingest_runs_without_scratch():
    k = _instances(_remarks("k_ingest.hip"), "k_ingest", (4, 2))
    assert len(k) == 8
    for name, v in k.items():
        assert v["ScratchSize"] == 0, (name, v)


@pytest.mark.parametrize("kernel", ["k_warp_bayer", "k_warp_bayer_mb"])
def test_warp_stays_under_64_registers_without_scratch(kernel):
    k = _instances(_remarks("k_warp.hip"), kernel, (4, 1))
    assert len(k) == 8
    for name, v in k.items():
        assert v["ScratchSize"] == 0 and v["VGPRs"] <= 64, (name, v)
