"""The kernels of developed mosaics (k_ingest_deep.hip, k_warp_deep.hip, k_warp_lens_deep.hip) as the compiler reports them, with
the build's own flags: the units hold exactly the kernels their headers name, and every one runs without scratch.  The VGPR
counts are printed, not bounded: DESIGN.md section 6v records them beside the 8-bit kernels' (tests/test_bayer_resources.py).
No device is needed; the files are compiled for the device only and nothing is written."""
import re

import pytest

import warp_kernels as W


def test_ingest_deep_is_four_kernels_without_scratch():
    k = W.remarks("k_ingest_deep.hip")
    forms = sorted(re.search(r"13k_ingest_deepILi(\d)ELb([01])EE", n).groups() for n in k)
    assert forms == [("2", "0"), ("2", "1"), ("4", "0"), ("4", "1")], sorted(k)
    for name, v in k.items():
        print(name, v)
        assert v["ScratchSize"] == 0, (name, v)


@pytest.mark.parametrize("unit,templates", [("k_warp_deep.hip", ("k_warp_one", "k_warp_boards")), ("k_warp_lens_deep.hip", ("k_warp_lens",))])
def test_warp_deep_kernels_run_without_scratch(unit, templates):
    k = W.instances(unit)
    want = sorted((t, src, lds, fpt) for t in templates for src in ("WarpDeep", "WarpDeepProfile") for lds in (False, True) for fpt in (1, 2))
    assert sorted(k) == want, sorted(k)
    for key, v in sorted(k.items()):
        print(key, v)
        assert v["ScratchSize"] == 0, (key, v)


def test_the_units_of_the_default_path_hold_no_deep_kernel():
    for unit in ("k_ingest.hip", "k_warp.hip", "k_warp_raw_profile.hip", "k_warp_lens.hip", "k_warp_lens_profile.hip"):
        assert not [n for n in W.remarks(unit) if "Deep" in n or "deep" in n], unit
