"""Every kernel of k_warp_jpeg.hip as the compiler reports it, with the build's own flags: k_warp_one and k_warp_boards of
WarpJpeg and of WarpJpegProfile, each with one frame per thread and with its many-frames form (four frames a thread for the
plain source, two for the source with a profile); none uses scratch, the profile kernels stage the 7 680 B of the
profile's tables and nothing else, the plain kernels use no LDS (warp_gather gives their kind none), and each stays at or
under the VGPR count written down here when the form was chosen, so that a regression shows.
No device is needed; the file is compiled for the device only and nothing is written."""
import warp_kernels as W
from chessboard_vision_amd import build as B

# (kernel template, source, frames per thread) -> (VGPRs, LDS bytes)
WANT = {
    ("k_warp_one", "WarpJpeg", 1): (44, 0), ("k_warp_boards", "WarpJpeg", 1): (44, 0),
    ("k_warp_one", "WarpJpeg", 4): (83, 0), ("k_warp_boards", "WarpJpeg", 4): (83, 0),
    ("k_warp_one", "WarpJpegProfile", 1): (70, 7680), ("k_warp_boards", "WarpJpegProfile", 1): (70, 7680),
    ("k_warp_one", "WarpJpegProfile", 2): (93, 7680), ("k_warp_boards", "WarpJpegProfile", 2): (93, 7680),
}


def _instances():
    """(kernel template, source, frames per thread) -> figures; neither source is a template"""
    out = {}
    for (name, src, arg, fpt), v in W.instances("k_warp_jpeg.hip").items():
        assert arg is None, (name, src, arg)
        out[(name, src, fpt)] = v
    return out


def test_the_file_is_in_the_build():
    assert "k_warp_jpeg.hip" in B.SOURCES and "warp_gather.h" in B.HEADERS and "jpeg_core.h" in B.HEADERS


def test_the_file_yields_the_expected_instantiations():
    got = sorted(_instances())
    assert got == sorted(WANT) and len(got) == 8


def test_no_scratch_the_lds_and_the_committed_registers():
    rem = _instances()
    for key, (most, lds) in WANT.items():
        v = rem[key]
        assert v["ScratchSize"] == 0, (key, v)
        assert v["LDS Size"] == lds, (key, v)
        assert v["VGPRs"] <= most, (key, v)
    assert WANT[("k_warp_one", "WarpJpeg", 1)][0] <= 64  # the one-frame plain form keeps 8 waves per SIMD
