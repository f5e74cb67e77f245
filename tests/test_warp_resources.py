"""Every kernel of k_warp.hip as the compiler reports it, with the build's own flags: the one gather (warp_gather) yields
exactly the 52 warp kernels (8 k_warp / k_warp_mb, 4 k_warp_profile / k_warp_profile_mb, 24 k_warp_yuv / k_warp_yuv_mb,
16 k_warp_bayer / k_warp_bayer_mb) beside k_synth, none of them uses scratch, and each stays at or under 64 VGPRs, the
line DESIGN.md section 4 gives for running at 8 waves per SIMD.
No device is needed; the file is compiled for the device only and nothing is written."""
import functools
import os
import re
import subprocess

from chessboard_vision_amd import build as B

# kernel -> instantiations: formats (or byte-map forms) x frames per thread
EXPECTED = {"k_warp": 4, "k_warp_mb": 4, "k_warp_profile": 2, "k_warp_profile_mb": 2, "k_warp_yuv": 12, "k_warp_yuv_mb": 12,
            "k_warp_bayer": 8, "k_warp_bayer_mb": 8}


@functools.lru_cache(maxsize=None)
def _remarks():
    src = os.path.join(B.CSRC, "k_warp.hip")
    cmd = [B._hipcc(), *B.FLAGS, "--cuda-device-only", "-S", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for fn, body in re.findall(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", r.stderr, re.S):
        out[fn] = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", body)}
    return out


def _kernel(mangled):
    """the template's name of _Z<len><name>I...; the plain name of an extern "C"-like symbol"""
    m = re.match(r"_Z(\d+)", mangled)
    return mangled[m.end():m.end() + int(m.group(1))] if m else mangled


def test_the_file_yields_the_52_warp_kernels_and_k_synth():
    count = {}
    for name in _remarks():
        count[_kernel(name)] = count.get(_kernel(name), 0) + 1
    assert count.pop("k_synth", 0) == 1, sorted(_remarks())
    assert count == EXPECTED and sum(count.values()) == 52, count


def test_every_kernel_runs_without_scratch_at_64_registers_or_fewer():
    rem = _remarks()
    assert len(rem) == 53
    for name, v in rem.items():
        assert v["ScratchSize"] == 0, (name, v)
        assert v["VGPRs"] <= 64, (name, v)
