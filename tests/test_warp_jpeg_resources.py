"""Every kernel of k_warp_jpeg.hip as the compiler reports it, with the build's own flags: k_warp_jpeg, k_warp_jpeg_mb,
k_warp_jpeg_profile and k_warp_jpeg_profile_mb, each with one frame per thread and with its many-frames form (four frames a
thread for the plain kernels, two for the profile kernels); none uses scratch, the profile kernels stage the 7 680 B of the
profile's tables and nothing else, the plain kernels use no LDS (warp_gather gives their kind none), and each stays at or
under the VGPR count written down here when the form was chosen, so that a regression shows.
No device is needed; the file is compiled for the device only and nothing is written."""
import functools
import os
import re
import subprocess

from chessboard_vision_amd import build as B

# (kernel, frames per thread) -> (VGPRs, LDS bytes)
WANT = {
    ("k_warp_jpeg", 1): (44, 0), ("k_warp_jpeg_mb", 1): (44, 0),
    ("k_warp_jpeg", 4): (83, 0), ("k_warp_jpeg_mb", 4): (83, 0),
    ("k_warp_jpeg_profile", 1): (70, 7680), ("k_warp_jpeg_profile_mb", 1): (70, 7680),
    ("k_warp_jpeg_profile", 2): (93, 7680), ("k_warp_jpeg_profile_mb", 2): (93, 7680),
}


@functools.lru_cache(maxsize=None)
def _remarks():
    src = os.path.join(B.CSRC, "k_warp_jpeg.hip")
    cmd = [B._hipcc(), *B.FLAGS, "--cuda-device-only", "-S", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for fn, body in re.findall(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", r.stderr, re.S):
        out[fn] = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", body)}
    return out


def _instance(mangled):
    """(kernel, frames per thread) of _Z<len><name>ILi<fpt>EE..."""
    m = re.match(r"_Z(\d+)", mangled)
    name = mangled[m.end():m.end() + int(m.group(1))]
    a = re.match(r"ILi(\d+)E", mangled[m.end() + int(m.group(1)):])
    return name, int(a.group(1))


def test_the_file_is_in_the_build():
    assert "k_warp_jpeg.hip" in B.SOURCES and "warp_gather.h" in B.HEADERS and "jpeg_core.h" in B.HEADERS


def test_the_file_yields_the_expected_instantiations():
    got = sorted(_instance(n) for n in _remarks())
    assert got == sorted(WANT) and len(got) == 8


def test_no_scratch_the_lds_and_the_committed_registers():
    rem = {_instance(n): v for n, v in _remarks().items()}
    for key, (most, lds) in WANT.items():
        v = rem[key]
        assert v["ScratchSize"] == 0, (key, v)
        assert v["LDS Size"] == lds, (key, v)
        assert v["VGPRs"] <= most, (key, v)
    assert WANT[("k_warp_jpeg", 1)][0] <= 64  # the one-frame plain form keeps 8 waves per SIMD
