"""Every kernel of k_warp_raw_profile.hip as the compiler reports it, with the build's own flags: per raw format the warp
knows one k_warp_one and one k_warp_boards of WarpRawProfile with one frame per thread and one each with the family's
many-frames form (four frames a thread; planar 4:2:0 two); none uses scratch, each stages the 7 680 B of the profile's tables
and nothing else, and each stays at or under the VGPR count written down here when the form was chosen, so that a
regression shows.  The one-frame forms are at or under 64, the line DESIGN.md section 4 gives for 8 waves per SIMD; the
many-frames forms are above it on purpose: they were the fastest inside the run.
No device is needed; the file is compiled for the device only and nothing is written."""
import warp_kernels as W
from chessboard_vision_amd import _native as N
from chessboard_vision_amd import build as B

FMT = dict(N.FORMATS, **N.BAYER_FORMATS)
# (format, frames per thread) -> VGPRs of WarpRawProfile in (k_warp_one, k_warp_boards); YV12 is launched as yuv420p
VGPRS = {
    ("nv12", 1): (58, 52), ("nv21", 1): (58, 52), ("yuv420p", 1): (62, 56),
    ("yuyv", 1): (46, 46), ("yvyu", 1): (46, 46), ("uyvy", 1): (44, 44),
    ("nv12", 4): (79, 79), ("nv21", 4): (79, 79), ("yuv420p", 2): (77, 77),
    ("yuyv", 4): (71, 71), ("yvyu", 4): (71, 71), ("uyvy", 4): (70, 70),
    ("bayer_rggb", 1): (57, 55), ("bayer_bggr", 1): (57, 55), ("bayer_grbg", 1): (55, 53), ("bayer_gbrg", 1): (55, 53),
    ("bayer_rggb", 4): (72, 72), ("bayer_bggr", 4): (72, 72), ("bayer_grbg", 4): (72, 72), ("bayer_gbrg", 4): (72, 72),
}
KERNELS = ("k_warp_one", "k_warp_boards")


def _instances():
    return W.instances("k_warp_raw_profile.hip")


def test_the_file_is_in_the_build():
    assert "k_warp_raw_profile.hip" in B.SOURCES and "warp_gather.h" in B.HEADERS


def test_the_file_yields_the_expected_instantiations():
    got = sorted(_instances())
    want = sorted((k, "WarpRawProfile", FMT[f], fpt) for (f, fpt) in VGPRS for k in KERNELS)
    assert got == want and len(got) == 40
    assert "yv12" not in {f for f, _ in VGPRS} and set(f for f, _ in VGPRS) == set(FMT) - {"bgr", "yv12"}


def test_no_scratch_the_tables_lds_and_the_committed_registers():
    rem = _instances()
    for (f, fpt), counts in VGPRS.items():
        for k, most in zip(KERNELS, counts):
            v = rem[(k, "WarpRawProfile", FMT[f], fpt)]
            assert v["ScratchSize"] == 0, (k, f, fpt, v)
            assert v["LDS Size"] == 7680, (k, f, fpt, v)
            assert v["VGPRs"] <= most and (fpt > 1 or most <= 64), (k, f, fpt, v)
