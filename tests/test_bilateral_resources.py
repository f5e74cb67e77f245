"""The batched d = 9 bilateral (k_bilateral<4, 768, PAIRS>) stays under 96 registers without scratch only because an
empty asm statement and a sched_barrier per half step keep hipcc from looking every weight of the tile up before it
accumulates (168 VGPRs and 1.8 KB of scratch otherwise).  That is scheduler behaviour, so the figures the compiler
reports are checked here with the build's own flags: a compiler update cannot quietly ship a spilling kernel.
No device is needed; the file is compiled for the device only and nothing is written."""
import os
import re
import subprocess

import pytest

from chessboard_vision_amd import build as B


def _remarks(extra, flags):
    src = os.path.join(B.CSRC, "k_bilateral.hip")
    cmd = [B._hipcc(), *extra, *flags, "--cuda-device-only", "-S", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for name, body in re.findall(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", r.stderr, re.S):
        out[name] = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", body)}
    return out


# the form a build selects and its documented figures: (extra flags, instantiation, LDS bytes)
FORMS = {"default": ([], "ILi4ELi768ELb1ELi0E", 61184), "BL_NT1024": (["-DBL_NT1024"], "ILi4ELi1024ELb1ELi5E", 69888)}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_batched_d9_form_fits_96_registers_without_scratch(form):
    extra, inst, lds = FORMS[form]
    # the build's A/B switches come in through the environment (build.py's FLAGS); the forms are checked without them
    flags = [f for f in B.FLAGS if f not in ("-DBL_NT1024", "-DBL_NO_CAP", "-DBL_NO_PAIRS")]
    k = _remarks(extra, flags)
    assert k and all(v["ScratchSize"] == 0 for v in k.values()), {n: v["ScratchSize"] for n, v in k.items()}
    (pairs,) = [v for n, v in k.items() if inst in n]
    assert pairs["VGPRs"] <= 96 and pairs["Occupancy"] >= 5 and pairs["LDS Size"] == lds, pairs
