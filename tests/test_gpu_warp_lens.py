"""cbv_warp_lens / cbv_warp_jpeg_lens (k_warp_lens.hip, k_warp_lens_profile.hip) against tests/ref_lens.py, the numpy
restatement of the definition in include/cbv.h, on the converted frame, byte for byte.  The conversions are the product's own
stage calls, which are pinned elsewhere: yuv_to_bgr, bayer_to_bgr, jpeg_to_bgr, cbv_apply_color_profile.  96 x 64 noise
frames, a 100 x 72 destination (two 64-wide blocks, the second partial; no multiple of the profile kernels' 16 rows), one
homography inside the frame and one with about a third of the board outside, both rotations, with and without a profile.
And a geometry check that shares nothing with ref_lens's blend: a ramp frame, whose warped bytes ARE the sampled position."""
import functools

import numpy as np
import pytest

import color_sweep_ref as CS
import raw_profile_ref as RP
import ref_jpeg as RJ
import ref_lens as R

pytestmark = pytest.mark.gpu

W, H, DEST = 96, 64, (100, 72)
# the barrel and pincushion coefficients of ref_lens on a 96 x 64 frame
LENS_96 = {"barrel": (75.0, 75.0, 48.0, 32.0) + R.BARREL[4:], "pincushion": (75.0, 75.0, 48.0, 32.0) + R.PINCUSHION[4:]}
QUADS = {"inside": RP.quads(W, H)["inside"], "third_outside": [[-30, 6], [70, -4], [-25, 58], [80, 60]]}  # ideal coordinates
FULL = ["bgr", "nv12", "yuv420p", "yuyv", "bayer_rggb", "bayer_gbrg", "mjpeg420", "mjpeg422"]
ONCE = ["nv21", "yv12", "yvyu", "uyvy", "bayer_bggr", "bayer_grbg", "mjpeg444", "mjpeggray"]


def _lens(t):
    from chessboard_vision_amd.stream import Lens
    return Lens(*t)


@functools.lru_cache(maxsize=None)
def _frame(fmt):
    """(what the entry point takes, its fmt argument, the BGR frame the product's own conversion makes of it)"""
    from chessboard_vision_amd.board_detection import bayer_to_bgr, jpeg_to_bgr, yuv_to_bgr
    if fmt == "bgr":
        f = np.random.default_rng(11).integers(0, 256, (H, W, 3), dtype=np.uint8)
        return f, "bgr", f
    if fmt.startswith("mjpeg"):
        f = np.random.default_rng(12).integers(0, 256, (H, W, 3), dtype=np.uint8)
        data = RJ.encode_image(f, quality=90, sampling=fmt[5:])
        return data, "mjpeg", jpeg_to_bgr(data)
    raw = RP.noise(W, H, fmt, 5)
    return raw, fmt, (bayer_to_bgr(raw, fmt) if fmt.startswith("bayer") else yuv_to_bgr(raw, fmt))


def _profiled(gpu_ctx, bgr, prof):
    from chessboard_vision_amd import _native as N
    if not prof:
        return bgr
    out = np.empty_like(bgr)
    gpu_ctx.check(gpu_ctx.lib.cbv_apply_color_profile(gpu_ctx.h, N.ptr(bgr), bgr.shape[1], bgr.shape[0], bgr.strides[0], N.ColorProfile.from_dict(prof),
                                                      N.ptr(out), out.strides[0]))
    return out


def _check(gpu_ctx, fmt, lens_name, profiles, quads, rots):
    from chessboard_vision_amd.board_detection import warp_lens
    img, f, bgr = _frame(fmt)
    t = LENS_96[lens_name]
    for prof in profiles:
        src = _profiled(gpu_ctx, bgr, prof)
        for qname in quads:
            M = R.homography(QUADS[qname], [(0, 0), (DEST[0], 0), (0, DEST[1]), DEST])
            for rot in rots:
                got = warp_lens(img, M, DEST, _lens(t), prof, rot180=rot, fmt=f)
                want = R.warp(src, t, M, DEST[0], DEST[1], rot)
                assert np.array_equal(got, want), (fmt, lens_name, bool(prof), qname, rot, int((got != want).sum()))
                outside = (~want.any(2)).mean()  # (white noise: a pixel sampled inside the frame is not black)
                assert (0.1 < outside < 0.6) if qname == "third_outside" else outside < 0.01, (qname, outside)  # the case is what its name says


@pytest.mark.parametrize("lens_name", sorted(LENS_96))
@pytest.mark.parametrize("fmt", FULL)
def test_equals_the_definition_on_the_converted_frame(gpu_ctx, fmt, lens_name):
    _check(gpu_ctx, fmt, lens_name, (None, CS.SHIPPED), ("inside", "third_outside"), (False, True))


@pytest.mark.parametrize("fmt", ONCE)
def test_the_remaining_layouts_once_each(gpu_ctx, fmt):
    _check(gpu_ctx, fmt, "barrel", (None,), ("third_outside",), (False,))


def test_a_disabled_lens_is_the_lens_free_call(gpu_ctx):
    from chessboard_vision_amd.board_detection import warp_lens, warp_perspective_profiled
    M = R.homography(QUADS["third_outside"], [(0, 0), (DEST[0], 0), (0, DEST[1]), DEST])
    for fmt in ("bgr", "nv12", "bayer_rggb", "mjpeg420"):
        img, f, _ = _frame(fmt)
        for prof in (None, CS.SHIPPED):
            assert np.array_equal(warp_lens(img, M, DEST, None, prof, fmt=f), warp_perspective_profiled(img, M, DEST, prof, fmt=f)), (fmt, bool(prof))


def test_refusals_leave_out_untouched(gpu_ctx):
    from chessboard_vision_amd import _native as N
    f = np.ascontiguousarray(_frame("bgr")[0])
    raw = N.raw_frame(f, "bgr")[0]
    out = np.full((DEST[1], DEST[0], 3), 0x5A, np.uint8)
    M = np.eye(3)
    for field, bad in (("fx", 0.0), ("fy", -2.0), ("k2", float("nan")), ("cx", float("inf"))):
        s = _lens(LENS_96["barrel"]).struct()
        setattr(s, field, bad)
        assert gpu_ctx.lib.cbv_warp_lens(gpu_ctx.h, raw, W, H, None, s, N.ptr(M), DEST[0], DEST[1], 0, N.ptr(out), out.strides[0]) == -1, field
        assert (out == 0x5A).all()
    good = _lens(LENS_96["barrel"]).struct()
    assert gpu_ctx.lib.cbv_warp_lens(gpu_ctx.h, raw, W, H, None, good, None, DEST[0], DEST[1], 0, N.ptr(out), out.strides[0]) == -1
    assert gpu_ctx.lib.cbv_warp_lens(gpu_ctx.h, raw, W, H, None, good, N.ptr(M), DEST[0], DEST[1], 0, N.ptr(out), 10) == -1
    assert (out == 0x5A).all()
    assert gpu_ctx.lib.cbv_warp_lens(gpu_ctx.h, raw, W, H, None, good, N.ptr(M), DEST[0], DEST[1], 0, N.ptr(out), out.strides[0]) == 0


# ---------------------------------------------------------------------------
# the geometry, independent of ref_lens's blend
# ---------------------------------------------------------------------------
GW, GH = 256, 192
CLICKED = np.array([(40, 30), (215, 25), (30, 170), (225, 165)], np.float64)  # in the frame as delivered


@pytest.mark.parametrize("S", [100, 72])
@pytest.mark.parametrize("lens_name", ["barrel", "pincushion"])
def test_a_ramp_frame_comes_out_as_the_position_it_was_sampled_at(gpu_ctx, lens_name, S):
    """B = x, G = y: the blend of a linear ramp is exact before its final rounding (at most 0.5 off) and the position is
    quantised to 1/32 px (at most 1/64 off), so every destination pixel must satisfy |B - u'| <= 0.5 + 1/64 and the same
    for G against v', with (u', v') the float64 position from the formula below.  Every tap of every pixel lies inside the
    frame with these inputs (sx 29..223, sy 22..171), so no pixel is left out."""
    from chessboard_vision_amd.board_detection import undistort_points, warp_lens, warp_perspective
    t = R.BARREL if lens_name == "barrel" else R.PINCUSHION
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = t
    frame = np.zeros((GH, GW, 3), np.uint8)
    frame[..., 0] = np.arange(GW)[None, :]
    frame[..., 1] = np.arange(GH)[:, None]
    corners = np.array([(0, 0), (S, 0), (0, S), (S, S)], np.float64)
    M = R.homography(undistort_points(CLICKED, _lens(t)), corners)
    Minv = np.linalg.inv(M)

    def position(dx, dy):  # the three lines: homography, normalise, Brown-Conrady
        q = Minv @ np.stack([dx, dy, np.ones_like(dx)])
        x, y = (q[0] / q[2] - cx) / fx, (q[1] / q[2] - cy) / fy
        r2 = x * x + y * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        return ((x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)) * fx + cx, (y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y) * fy + cy)

    # the clicked points come out at the board's corners
    cu, cv = position(corners[:, 0], corners[:, 1])
    assert np.abs(cu - CLICKED[:, 0]).max() <= 1e-6 and np.abs(cv - CLICKED[:, 1]).max() <= 1e-6
    dx, dy = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64))
    u, v = position(dx.ravel(), dy.ravel())
    u, v = u.reshape(S, S), v.reshape(S, S)
    bound = 0.5 + 1.0 / 64
    got = warp_lens(frame, M, (S, S), _lens(t))
    eb, eg = np.abs(got[..., 0] - u), np.abs(got[..., 1] - v)
    print("ramp %s S=%d: max |B - u'| %.4f, max |G - v'| %.4f (bound %.4f)" % (lens_name, S, eb.max(), eg.max(), bound))
    assert eb.max() <= bound and eg.max() <= bound and not got[..., 2].any()
    rot = warp_lens(frame, M, (S, S), _lens(t), rot180=True)
    assert np.array_equal(rot, got[::-1, ::-1])
    # the lens-free warp of the same frame and matrix is off by many pixels
    free = warp_perspective(frame, M, (S, S))
    worst = max(np.abs(free[..., 0] - u).max(), np.abs(free[..., 1] - v).max())
    print("lens-free: off by up to %.2f px" % worst)
    assert worst > bound
