"""cbv_warp_jpeg (k_warp_jpeg / k_warp_jpeg_profile; board_detection.warp_perspective_profiled(fmt="mjpeg")) against two
yardsticks: tests/raw_profile_ref.py's, the oracle's warp_perspective(apply_color_profile(bgr)) with bgr = tests/ref_jpeg.py's
decode of the stream, and the product's own stages composed, jpeg_to_bgr then warp_perspective_profiled on BGR.  Streams of
all four samplings from 1 x 1 (chroma replicated up to 4 wide, filtered from 5; heights 1 to 3 clamp the 4:2:0 row
neighbour) to partial MCUs on both axes, and one 640 x 480 synthetic frame; destinations that are no multiple of the
workgroup tile and one of many tiles; quads inside, partly outside, mirrored and entirely outside; both rotations; no
profile, the shipped one and a radical one; the four fixed damaged streams.  Tolerance 0."""
import functools

import numpy as np
import pytest

import color_sweep_ref as CS
import jpeg_streams as JS
import raw_profile_ref as RP
import ref_jpeg as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (6, 3), (17, 23), (9, 40), (40, 9), (33, 50)]
DESTS = ((33, 21), (620, 620))
PROFILES = {"none": None, "shipped": CS.SHIPPED, "radical": CS.PROFILES["radical"]}
ARG, UNSUPPORTED = -1, -5


def _matrix(quad, dw, dh):
    from chessboard_vision_amd.board_detection import get_perspective_transform
    return get_perspective_transform(np.float32(quad), np.float32([[0, 0], [dw, 0], [0, dh], [dw, dh]]))


def _check(oracle, data, bgr, what, profiles=("none", "shipped", "radical")):
    """every destination, quad, rotation and profile of one stream whose reference decode is `bgr`"""
    from chessboard_vision_amd.board_detection import jpeg_to_bgr, warp_perspective_profiled
    h, w = bgr.shape[:2]
    own = jpeg_to_bgr(data)
    assert np.array_equal(own, bgr), what  # (the decode itself: held elsewhere, needed for what follows)
    for dest in DESTS:
        for qname, quad in RP.quads(w, h).items():
            M = _matrix(quad, *dest)
            for name in profiles:
                prof = PROFILES[name]
                want = RP.yardstick(oracle, bgr, prof, M, dest)
                for rot in (False, True):
                    got = warp_perspective_profiled(data, M, dest, prof, rot180=rot, fmt="mjpeg")
                    ref = oracle.rotate180(want) if rot else want
                    assert np.array_equal(got, ref), (what, dest, qname, rot, name, int((got != ref).sum()))
                    if qname == "outside":
                        assert not got.any()  # BORDER_CONSTANT 0, not the profile of black
                    assert np.array_equal(got, warp_perspective_profiled(own, M, dest, prof, rot180=rot)), (what, dest, qname, rot, name)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("sampling", JS.SAMPLINGS)
def test_equals_the_yardstick_and_the_composed_stages(gpu_ctx, oracle, sampling, shape):
    data = JS.shape_stream(shape[0], shape[1], sampling)
    _check(oracle, data, JS.ref(data)["bgr"], (sampling, shape))


@functools.lru_cache(maxsize=None)
def _synth_streams():
    f = np.array(CS.frame("lilac", 0))
    assert f.shape == (480, 640, 3)
    return {s: R.encode_image(f, quality=90, sampling=s, dri=0 if s != "422" else 40) for s in JS.SAMPLINGS}


@pytest.mark.parametrize("sampling", JS.SAMPLINGS)
def test_a_640_x_480_synthetic_frame(gpu_ctx, oracle, sampling):
    from chessboard_vision_amd.board_detection import jpeg_decode
    data = _synth_streams()[sampling]
    twin = jpeg_decode(data, host=True)
    assert twin[3] == 0
    _check(oracle, data, twin[0], ("synth", sampling), profiles=("none", "shipped") if sampling != "420" else ("none", "shipped", "radical"))


@pytest.mark.parametrize("name", sorted(JS.DAMAGED))
def test_a_damaged_stream_changes_values_and_nothing_else(gpu_ctx, name):
    """the four FIXED damaged streams: the host twin decodes each without fault, the warp's output is that of the composed
    stages and its status word is the twin's"""
    from chessboard_vision_amd.board_detection import jpeg_decode, jpeg_to_bgr, warp_jpeg, warp_perspective_profiled
    data = JS.damaged_stream(name)
    twin = jpeg_decode(data, host=True)
    assert twin[3] & JS.DAMAGED[name] == JS.DAMAGED[name]
    own = jpeg_to_bgr(data)
    assert np.array_equal(own, twin[0])
    h, w = own.shape[:2]
    for dest in DESTS:
        for qname, quad in RP.quads(w, h).items():
            M = _matrix(quad, *dest)
            for prof in (None, CS.SHIPPED):
                for rot in (False, True):
                    got, st = warp_jpeg(data, M, dest, prof, rot180=rot)
                    assert st == twin[3], (name, st)
                    assert np.array_equal(got, warp_perspective_profiled(own, M, dest, prof, rot180=rot)), (name, dest, qname, rot)


def test_an_empty_profile_is_the_plain_warp(gpu_ctx):
    from chessboard_vision_amd.board_detection import jpeg_to_bgr, warp_image, warp_image_profiled, warp_perspective, warp_perspective_profiled
    data = JS.shape_stream(33, 50, "420")
    own = jpeg_to_bgr(data)
    for quad in RP.quads(33, 50).values():
        M = _matrix(quad, 33, 21)
        for prof in (None, {}):
            for rot in (False, True):
                got = warp_perspective_profiled(data, M, (33, 21), prof, rot180=rot, fmt="mjpeg")
                assert np.array_equal(got, warp_perspective(own, M, (33, 21), rot180=rot))
    pts = RP.quads(33, 50)["inside"]
    a = warp_image_profiled(np.frombuffer(data, np.uint8), pts, CS.SHIPPED, display_size=(200, 150), margin=20, fmt="mjpeg")
    b = warp_image_profiled(own, pts, CS.SHIPPED, display_size=(200, 150), margin=20)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] == 130
    assert np.array_equal(warp_image_profiled(data, pts, None, display_size=(200, 150), margin=20, fmt="mjpeg")[0],
                          warp_image(own, pts, display_size=(200, 150), margin=20)[0])


def test_refusals_leave_out_untouched(gpu_ctx):
    import ctypes as C
    from chessboard_vision_amd import _native as N
    lib, ctx = gpu_ctx.lib, gpu_ctx
    good = np.frombuffer(JS.shape_stream(33, 50, "422"), np.uint8)
    M = np.eye(3)
    prof = N.ColorProfile.from_dict(CS.SHIPPED)
    nan = N.ColorProfile.from_dict(dict(CS.SHIPPED, val_scale=float("nan")))
    out = np.full((21, 33, 3), 0x5A, np.uint8)
    st = C.c_int32(77)

    def call(data=good, n=None, profile=prof, m=M, dw=33, dh=21, o=out, ostride=99, status=st):
        return lib.cbv_warp_jpeg(ctx.h, N.ptr(data) if data is not None else None, (data.size if data is not None else 0) if n is None else n, profile,
                                 N.ptr(m) if m is not None else None, dw, dh, 0, N.ptr(o) if o is not None else None, ostride,
                                 C.byref(status) if status is not None else None)

    assert call() == 0 and not (out == 0x5A).all() and st.value == 0
    out[:] = 0x5A
    prog = good.copy()
    prog[bytes(prog).index(b"\xff\xc0") + 1] = 0xC2
    cases = [("no stream", dict(data=None), ARG), ("not a JPEG stream", dict(data=np.zeros(64, np.uint8)), ARG),
             ("a header cut off", dict(n=30), ARG), ("a progressive stream", dict(data=prog), UNSUPPORTED),
             ("a non-finite profile", dict(profile=nan), ARG), ("no profile", dict(profile=None), ARG), ("no matrix", dict(m=None), ARG),
             ("a short output stride", dict(ostride=98), ARG), ("an empty destination", dict(dw=0), ARG),
             ("a destination too large", dict(dh=8193), ARG), ("no status", dict(status=None), ARG)]
    for what, kw, code in cases:
        assert call(**kw) == code, what
        assert (out == 0x5A).all(), what
    assert call(o=None) == ARG
