"""Every kernel of k_warp.hip as the compiler reports it, with the build's own flags: the one gather (warp_gather) yields
exactly the 52 warp kernels (k_warp_one and k_warp_boards of: WarpBgr 4 each, WarpProfile 2 each, WarpRaw of the YUV layouts 12
each, WarpRaw of the mosaics 8 each) beside k_synth, none of them uses scratch, and each stays at or under 64 VGPRs, the
line DESIGN.md section 4 gives for running at 8 waves per SIMD.
No device is needed; the file is compiled for the device only and nothing is written."""
import warp_kernels as W

# (kernel template, source) -> instantiations: formats (or byte-map forms) x frames per thread
EXPECTED = {("k_warp_one", "WarpBgr"): 4, ("k_warp_boards", "WarpBgr"): 4, ("k_warp_one", "WarpProfile"): 2, ("k_warp_boards", "WarpProfile"): 2,
            ("k_warp_one", "WarpRaw yuv"): 12, ("k_warp_boards", "WarpRaw yuv"): 12, ("k_warp_one", "WarpRaw bayer"): 8, ("k_warp_boards", "WarpRaw bayer"): 8}


def _remarks():
    return W.remarks("k_warp.hip")


def _kernel(mangled):
    """(template, source) of a warp kernel, the raw source split into its YUV and Bayer formats; the plain name of k_synth"""
    if "k_synth" in mangled:
        return "k_synth"
    name, src, arg, fpt = W.instance(mangled)
    assert fpt in (1, 4), mangled
    if src == "WarpRaw":
        src += " bayer" if arg in W.BAYER_IDS else " yuv"
    return name, src


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
