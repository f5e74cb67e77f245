"""Baseline JPEG on the GPU: cbv_jpeg_decode equals tests/ref_jpeg.py (the numpy restatement of include/cbv.h's definition)
at coefficient, plane and BGR level, tolerance 0.  No random garbage runs here: the four damaged streams are fixed, and the
host twin has passed them (and a few thousand seeded ones, under sanitizers) in tests/test_jpeg_host.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import jpeg_streams as S  # noqa: E402
import ref_jpeg as R  # noqa: E402

pytestmark = pytest.mark.gpu


def gpu(data):
    from chessboard_vision_amd.board_detection import jpeg_decode
    return jpeg_decode(data)


def assert_same(got, ref, what):
    bgr, coef, planes, st = got
    print("%s: coefficients differing %d, plane samples %d, BGR bytes %d, status %d / %d" % (
        what, np.count_nonzero(coef != ref["coef"]), np.count_nonzero(planes != ref["planes"]), np.count_nonzero(bgr != ref["bgr"]), st,
        ref["status"]))
    assert np.array_equal(coef, ref["coef"]), what
    assert np.array_equal(planes, ref["planes"]), what
    assert np.array_equal(bgr, ref["bgr"]), what
    assert st == ref["status"], what


@pytest.mark.parametrize("sampling", S.SAMPLINGS)
@pytest.mark.parametrize("w,h", S.SHAPES)
def test_shapes(gpu_ctx, w, h, sampling):
    d = S.shape_stream(w, h, sampling)
    assert_same(gpu(d), S.ref(d), "%dx%d %s" % (w, h, sampling))


@pytest.mark.parametrize("name", sorted(S.RESTART_CASES))
def test_restart_markers(gpu_ctx, name):
    d = S.restart_stream(name)
    ref = S.ref(d)
    assert ref["status"] == 0 and ref["header"]["nint"] > 1
    assert_same(gpu(d), ref, name)


@pytest.mark.parametrize("name", S.SPECIAL)
def test_streams_from_the_coefficient_encoder(gpu_ctx, name):
    d = S.special_stream(name)
    ref = S.ref(d)
    assert ref["status"] == 0
    assert_same(gpu(d), ref, name)


def test_recorded_pillow_decodes(gpu_ctx):
    z = np.load(os.path.join(HERE, "golden", "jpeg_cases.npz"))
    names = [str(n) for n in z["names"]]
    bad = []
    for i, n in enumerate(names):
        bgr, _, _, st = gpu(z["data_%d" % i].tobytes())
        if st != 0 or not np.array_equal(bgr, z["bgr_%d" % i]):
            bad.append(n)
    print("recorded Pillow decodes: %d of %d differ" % (len(bad), len(names)))
    assert not bad, bad[:8]


def test_jpeg_to_bgr_is_the_decode(gpu_ctx):
    from chessboard_vision_amd.board_detection import jpeg_to_bgr
    d = S.shape_stream(33, 50, "420")
    assert np.array_equal(jpeg_to_bgr(d), S.ref(d)["bgr"])
    assert np.array_equal(jpeg_to_bgr(np.frombuffer(d, np.uint8)), S.ref(d)["bgr"])
    with pytest.raises(ValueError):
        jpeg_to_bgr(b"\xff\xd8\xff\xd9")


def test_damaged_streams_stay_in_bounds_and_a_valid_frame_follows(gpu_ctx):
    """each fixed damaged stream gives the twin's bytes and status, leaves the guard bytes behind every output alone, and the
    valid frame decoded afterwards is correct"""
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.board_detection import jpeg_decode, jpeg_probe
    lib = gpu_ctx.lib
    good = S.damage_base()
    for name in sorted(S.DAMAGED):
        d = np.frombuffer(S.damaged_stream(name), np.uint8)
        info = jpeg_probe(d)
        w, h, n = info["w"], info["h"], info["plane_elems"]
        G = 4096
        bgr = np.full(h * w * 3 + G, 0xA5, np.uint8)
        coef = np.full(n + G, 0x5A5A, np.int16)
        planes = np.full(n + G, 0xA5, np.uint8)
        st = C.c_int32(-1)
        gpu_ctx.check(lib.cbv_jpeg_decode(gpu_ctx.h, N.ptr(d), d.size, N.ptr(bgr), w * 3, N.ptr(coef), N.ptr(planes), C.byref(st)))
        tw = jpeg_decode(d, host=True)
        ref = S.ref(d.tobytes())
        print("%s: status %d (twin %d, reference %d)" % (name, st.value, tw[3], ref["status"]))
        assert st.value == tw[3] == ref["status"] and st.value & S.DAMAGED[name] == S.DAMAGED[name]
        assert np.array_equal(coef[:n], tw[1]) and np.array_equal(planes[:n], tw[2]) and np.array_equal(bgr[:h * w * 3].reshape(h, w, 3), tw[0])
        assert np.array_equal(tw[0], ref["bgr"])
        assert (bgr[h * w * 3:] == 0xA5).all() and (coef[n:] == 0x5A5A).all() and (planes[n:] == 0xA5).all(), "guard bytes were written"
        assert_same(gpu(good), S.ref(good), "the valid frame after " + name)


def test_strided_output_and_stage_outputs_are_optional(gpu_ctx):
    from chessboard_vision_amd import _native as N
    d = np.frombuffer(S.shape_stream(17, 23, "422"), np.uint8)
    out = np.full((23, 64), 0xA5, np.uint8)
    st = C.c_int32(-1)
    gpu_ctx.check(gpu_ctx.lib.cbv_jpeg_decode(gpu_ctx.h, N.ptr(d), d.size, N.ptr(out), 64, None, None, C.byref(st)))
    assert st.value == 0
    assert np.array_equal(out[:, :51].reshape(23, 17, 3), S.ref(d.tobytes())["bgr"]) and (out[:, 51:] == 0xA5).all()
    assert gpu_ctx.lib.cbv_jpeg_decode(gpu_ctx.h, N.ptr(d), d.size, N.ptr(out), 50, None, None, C.byref(st)) == -1


def test_one_1080p_frame_equals_the_twin(gpu_ctx):
    """1920 x 1080 4:2:2, restart interval of one MCU row: 68 lanes of entropy decode, 48600 blocks; GPU = host twin, byte for byte"""
    from chessboard_vision_amd.board_detection import jpeg_decode
    img, d = S.frame_1080p()
    g = jpeg_decode(d)
    t = jpeg_decode(d, host=True)
    print("1080p: %d bytes of stream, status %d / %d" % (len(d), g[3], t[3]))
    assert g[3] == t[3] == 0
    assert np.array_equal(g[1], t[1]) and np.array_equal(g[2], t[2]) and np.array_equal(g[0], t[0])
    # ... and it is the picture: unrelated bytes are 85 apart on average, quality 90 costs a few levels
    assert np.abs(g[0].astype(int) - img).mean() < 20
