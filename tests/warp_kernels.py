"""What the resource tests of the warp units share: a unit's kernels as the compiler reports them, with the build's own flags,
and the reading of a warp kernel's mangled name.  The warp has three kernel templates, one per launch shape (warp_gather.h,
warp_lens.h): k_warp_one<Src, FPT>, k_warp_boards<Src, FPT> and k_warp_lens<Src, FPT>; the source is a type, so a kernel is
named by (template, source, the source's template argument, frames per thread).  No device is needed; a unit is compiled for
the device only and nothing is written."""
import functools
import os
import re
import subprocess

from chessboard_vision_amd import build as B

TEMPLATES = ("k_warp_one", "k_warp_boards", "k_warp_lens")
BAYER_IDS = (0x04, 0x14, 0x24, 0x34)


@functools.lru_cache(maxsize=None)
def remarks(unit):
    """mangled kernel name -> {figure: value} of -Rpass-analysis=kernel-resource-usage for one file of csrc"""
    cmd = [B._hipcc(), *B.FLAGS, "--cuda-device-only", "-S", os.path.join(B.CSRC, unit), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for fn, body in re.findall(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", r.stderr, re.S):
        out[fn] = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", body)}
    return out


def instance(mangled):
    """(template, source, argument, frames per thread) of _Z<len><template>I<len><source>[IL<i|b><argument>EE]Li<fpt>EE...: the
    argument is the format id of a raw source, the CALC of WarpBgr, None of a source that is no template"""
    m = re.match(r"_Z(\d+)", mangled)
    name, rest = mangled[m.end():m.end() + int(m.group(1))], mangled[m.end() + int(m.group(1)):]
    assert name in TEMPLATES, mangled
    a = re.match(r"I(\d+)", rest)
    src, rest = rest[a.end():a.end() + int(a.group(1))], rest[a.end() + int(a.group(1)):]
    b = re.match(r"(?:IL([ib])(\d+)EE)?Li(\d+)EEvT_", rest)
    assert b, mangled
    arg = None if b.group(1) is None else bool(int(b.group(2))) if b.group(1) == "b" else int(b.group(2))
    return name, src, arg, int(b.group(3))


def instances(unit):
    """(template, source, argument, frames per thread) -> figures, for a unit that holds warp kernels only"""
    out = {instance(n): v for n, v in remarks(unit).items()}
    assert len(out) == len(remarks(unit))
    return out
