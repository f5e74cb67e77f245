"""The host pieces of the lens model under AddressSanitizer and UBSan: a stand-alone program (tools/lens_fuzz_host.cpp) that
includes csrc/lens_core.h, the body the kernels and the library's host functions run, built and run here on the CPU.
Nothing loaded into Python runs under a sanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lens_core_is_clean_under_sanitizers_on_extreme_inputs(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "lens_fuzz_host"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "chessboard-vision_amd", "csrc"),
                        os.path.join(ROOT, "tools", "lens_fuzz_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler has no sanitizer runtime: %s" % r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe), "400"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "400 rounds" in r.stdout
