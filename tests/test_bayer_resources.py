"""The Bayer kernels' registers as the compiler reports them, with the build's own flags: every Bayer instantiation of
k_ingest and of the warp of a mosaic (k_warp_one and k_warp_boards of WarpRaw, k_warp.hip) runs without scratch, and the warp
forms stay at or under 64 VGPRs, the line DESIGN.md section 4 gives for running beside the squares and HoughCircles kernels at 8 waves per SIMD.
No device is needed; the files are compiled for the device only and nothing is written."""
import pytest

import warp_kernels as W

IDS = W.BAYER_IDS
_remarks = W.remarks


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


# (the ids are the kernels' names before the warp had one kernel template per launch shape)
@pytest.mark.parametrize("kernel", [pytest.param("k_warp_one", id="k_warp_bayer"), pytest.param("k_warp_boards", id="k_warp_bayer_mb")])
def test_warp_stays_under_64_registers_without_scratch(kernel):
    warp = {W.instance(n): v for n, v in _remarks("k_warp.hip").items() if "k_synth" not in n}
    k = {key: v for key, v in warp.items() if key[:2] == (kernel, "WarpRaw") and key[2] in IDS}
    assert sorted(key[2:] for key in k) == sorted((i, s) for i in IDS for s in (4, 1))
    assert len(k) == 8
    for name, v in k.items():
        assert v["ScratchSize"] == 0 and v["VGPRs"] <= 64, (name, v)
