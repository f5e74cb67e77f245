"""cbv_yuv_to_bgr in the colour spaces beside cv2's BT.601 limited range (include/cbv.h, CBV_CS_*; k_ingest_cs.hip): bit
exact against the int64 restatement of tests/ref64_yuv_cs.py, the only source of expected values here.  The cube (every
(Y, U, V) triple once) guards saturation and sign handling; small frames of all seven layouts take both load paths of
k_ingest_cs and their tails."""
import numpy as np
import pytest

import ref64_yuv as R
import ref64_yuv_cs as RC
import ref64_yuv_layouts as L

pytestmark = pytest.mark.gpu

WIDTHS, HEIGHTS = (6, 16, 18, 34), (2, 6)   # 16: the dword path; 6, 18, 34: the byte path (w % 4 = 2)


@pytest.fixture(scope="module")
def cube():
    f = R.cube_nv12()
    f.setflags(write=False)
    return f, L.split(f, "nv12")


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d bytes differ, first at %s: got %d, want %d"
                             % (what, len(bad), want.size, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.mark.parametrize("cs", RC.NEW)
def test_whole_cube(gpu_ctx, cube, cs):
    """one 4096 x 4096 NV12 frame holds every (Y, U, V) triple once"""
    from chessboard_vision_amd.board_detection import yuv_to_bgr
    f, yuv = cube
    _same(yuv_to_bgr(f, "nv12", colorspace=cs), RC.yuv_to_bgr_int(*yuv, cs), "NV12 cube, %s" % cs)


def _views(frame, fmt, pad, rng):
    """the planes of `frame` as views of larger buffers of other bytes, `pad` more bytes a row, at an offset of pad // 2 + 1"""
    def view(plane):
        big = rng.integers(0, 256, (plane.shape[0] + 2, plane.shape[1] + pad) + plane.shape[2:], dtype=np.uint8)
        o = pad // 2 + 1
        big[1:-1, o:o + plane.shape[1]] = plane
        return big[1:-1, o:o + plane.shape[1]]
    if fmt in L.FAMILY_422:
        return view(frame)
    return tuple(view(p) for p in L.planes(frame, fmt))


@pytest.mark.parametrize("fmt", RC.LAYOUTS)
@pytest.mark.parametrize("cs", RC.NEW)
def test_every_layout_both_load_paths_tight_and_strided(gpu_ctx, fmt, cs):
    """uniformly random bytes (Y below the offset, chroma that saturates every channel); tight frames, planes with a row stride
    that is a multiple of 4 (they travel as they lie: the device strides differ from the width) and planes with an odd stride
    at an odd address (packed on the way); the staging buffer is poisoned first, so a read outside the rows shows"""
    from chessboard_vision_amd.board_detection import yuv_to_bgr
    rng = np.random.default_rng(RC.LAYOUTS.index(fmt) * 7 + RC.NEW.index(cs))
    gpu_ctx.check(gpu_ctx.lib.cbv_debug_poison(gpu_ctx.h, 1))
    try:
        for w in WIDTHS:
            for h in HEIGHTS:
                f = RC.noise(w, h, fmt, 100 * w + h)
                want = RC.to_bgr(f, fmt, cs)
                got = yuv_to_bgr(f, fmt, colorspace=cs)
                assert got.shape == (h, w, 3) and got.dtype == np.uint8
                _same(got, want, "%s %s %dx%d tight" % (fmt, cs, w, h))
                for pad in (4, 7):
                    _same(yuv_to_bgr(_views(f, fmt, pad, rng), fmt, colorspace=cs), want, "%s %s %dx%d pad %d" % (fmt, cs, w, h, pad))
    finally:
        gpu_ctx.check(gpu_ctx.lib.cbv_debug_poison(gpu_ctx.h, 0))


@pytest.mark.parametrize("fmt", RC.LAYOUTS)
def test_the_default_is_untouched(gpu_ctx, fmt):
    """colorspace="bt601" is the call without the keyword, byte for byte, and the int64 definition of ref64_yuv"""
    from chessboard_vision_amd.board_detection import yuv_to_bgr
    for w, h in ((16, 6), (34, 2)):
        f = RC.noise(w, h, fmt, 3)
        plain = yuv_to_bgr(f, fmt)
        assert np.array_equal(yuv_to_bgr(f, fmt, colorspace="bt601"), plain)
        assert np.array_equal(plain, L.to_bgr(f, fmt)) and np.array_equal(plain, RC.to_bgr(f, fmt, "bt601"))
        assert not np.array_equal(plain, yuv_to_bgr(f, fmt, colorspace="bt709"))


def test_the_library_refuses_a_colour_space_on_bayer_mjpeg_and_bgr(gpu_ctx):
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.stream import BoardPipeline
    a = np.zeros((8, 8), np.uint8)
    out = np.full((8, 8, 3), 0x5A, np.uint8)
    for fmt, name in ((N.FMT_BAYER_RGGB, "BAYER_RGGB"), (N.FMT_BAYER_GBRG, "BAYER_GBRG")):
        for bits in (N.CS_FULL, N.CS_BT709, N.CS_MASK):
            r = N.RawFrame()
            r.fmt, r.stride0, r.plane0 = fmt | bits, 8, a.ctypes.data
            with pytest.raises(RuntimeError, match="colour-space bits.*%s" % name):
                gpu_ctx.check(gpu_ctx.lib.cbv_yuv_to_bgr(gpu_ctx.h, r, 8, 8, N.ptr(out), 24))
            assert (out == 0x5A).all()
    p = BoardPipeline(16, 8, 2)
    try:
        for fmt, name in ((N.FMT_MJPEG, "MJPEG"), (N.FMT_BGR, "BGR"), (N.FMT_BAYER_BGGR, "BAYER_BGGR")):
            with pytest.raises(RuntimeError, match="colour-space bits.*%s" % name):
                p.ctx.check(p.ctx.lib.cbv_pipeline_set_input_format(p.h_, fmt | N.CS_BT709))
        r = N.RawFrame()
        bgr = np.zeros((8, 16, 3), np.uint8)
        r.fmt, r.stride0, r.plane0 = N.FMT_BGR | N.CS_FULL, 48, bgr.ctypes.data
        with pytest.raises(RuntimeError, match="colour-space bits.*BGR"):
            p.ctx.check(p.ctx.lib.cbv_pipeline_upload_raw(p.h_, 0, r))
        assert p.ctx.lib.cbv_pipeline_set_input_format(p.h_, N.FMT_NV12 | N.CS_MASK) == 0
        assert p.ctx.lib.cbv_pipeline_set_input_format(p.h_, N.FMT_NV12 | 0x100) == -1   # (a bit outside the mask: an unknown format)
        # the Python layer refuses before the library is called
        with pytest.raises(ValueError, match="YUV formats"):
            p.set_input_format("bayer_rggb", colorspace="bt709")
        with pytest.raises(ValueError, match="YUV formats"):
            p.set_input_format("mjpeg", colorspace="bt601-full")
        with pytest.raises(ValueError, match="unknown colour space"):
            p.set_input_format("nv12", colorspace="rec709")
        p.set_input_format("yuyv", colorspace="BT709-full")
        assert (p.input_format, p.input_colorspace) == ("yuyv", "bt709-full")
        p.set_input_format("nv12")
        assert (p.input_format, p.input_colorspace) == ("nv12", "bt601")
    finally:
        p.close()
