"""The host side of the lens model (include/cbv.h, cbv_lens), no GPU: the coordinates of the warp through a lens against
the numpy restatement (ref_lens) bit for bit, the inverse for the clicked corners, the footprint, the refusals, and the
Python face (stream.Lens, load_lens / save_lens)."""
import ctypes as C
import json

import numpy as np
import pytest

import ref_lens as R
from chessboard_vision_amd import _native as N
from chessboard_vision_amd import board_detection as BD
from chessboard_vision_amd import stream as ST

W, H = 256, 192
LENSES = {"barrel": R.BARREL, "pincushion": R.PINCUSHION}
CORNERS = [(40, 30), (215, 25), (30, 170), (225, 165)]  # as clicked in the delivered frame: TL, TR, BL, BR


def _lens(t):
    return ST.Lens(*t)


def _ideal_matrix(t, S, corners=CORNERS):
    """board <- ideal frame, float64, from corners clicked in the delivered frame"""
    u, v = R.undistort(t, [c[0] for c in corners], [c[1] for c in corners])
    return R.homography(np.stack([u, v], 1), [(0, 0), (S, 0), (0, S), (S, S)])


def _coords(t, Minv, dw, dh):
    out = np.empty((dh, dw, 2), np.int32)
    Minv = np.ascontiguousarray(Minv, dtype=np.float64)
    assert N.load().cbv_lens_warp_coords(_lens(t).struct(), N.ptr(Minv), dw, dh, N.ptr(out)) == 0
    return out[..., 0].astype(np.int64), out[..., 1].astype(np.int64)


@pytest.mark.parametrize("S", [100, 72])  # two 64-wide blocks; a partial second block
@pytest.mark.parametrize("name", sorted(LENSES))
@pytest.mark.parametrize("corners", ["inside", "partly_outside"])
def test_warp_coords_equal_the_definition_bit_for_bit(name, S, corners):
    t = LENSES[name]
    if corners == "inside":
        M = _ideal_matrix(t, S)
    else:  # ideal-coordinate corners that put about a third of the board left of and above the frame
        M = R.homography([(-70, 20), (150, -30), (-60, 150), (170, 175)], [(0, 0), (S, 0), (0, S), (S, S)])
    Minv = R.invert3x3(M)
    X, Y = _coords(t, Minv, S, S)
    Xr, Yr = R.coords(t, Minv, S, S)
    assert np.array_equal(X, Xr) and np.array_equal(Y, Yr)
    sx, sy = X >> 5, Y >> 5
    out = (sx < -1) | (sx >= W) | (sy < -1) | (sy >= H)
    assert out.any() == (corners == "partly_outside")  # the case does what its name says


def test_warp_coords_of_degenerate_maps_follow_the_definition():
    # W = 0 everywhere: Wi = 0, u = v = 0, a finite position; W = 0 with an infinite lens term: not a number -> the lowest int32
    X, Y = _coords(R.BARREL, np.zeros(9), 8, 8)
    Xr, Yr = R.coords(R.BARREL, np.zeros(9), 8, 8)
    assert np.array_equal(X, Xr) and np.array_equal(Y, Yr)
    huge = np.array([1e300, 0, 1e300, 0, 1e300, -1e300, 0, 0, 1.0])  # x * x overflows: inf - inf appears in the model
    X, Y = _coords(R.BARREL, huge, 8, 8)
    Xr, Yr = R.coords(R.BARREL, huge, 8, 8)
    assert np.array_equal(X, Xr) and np.array_equal(Y, Yr)
    assert np.all((X >> 5 < -1) | (X >> 5 > 32767) | (Y >> 5 < -1) | (Y >> 5 > 32767))


@pytest.mark.parametrize("name,t,size", [("barrel", R.BARREL, (W, H)), ("pincushion", R.PINCUSHION, (W, H)), ("barrel_1080p", R.BARREL_1080P, (1920, 1080))])
def test_distort_of_undistort_returns_the_point(name, t, size):
    """40 rounds leave at most 5e-13 px with these lenses (the same iteration in numpy); 20 rounds leave 6e-8: the bound
    of 1e-9 px tells them apart with three orders of margin."""
    xs, ys = np.meshgrid(np.arange(0, size[0], 7.0), np.arange(0, size[1], 7.0))
    p = np.stack([xs.ravel(), ys.ravel()], 1)
    back = BD.distort_points(BD.undistort_points(p, _lens(t)), _lens(t))
    assert np.abs(back - p).max() <= 1e-9
    # the library's iteration is the definition's, to the bit, and the forward model too
    u, v = R.undistort(t, p[:, 0], p[:, 1])
    assert np.array_equal(BD.undistort_points(p, _lens(t)), np.stack([u, v], 1))
    ud, vd = R.distort(t, p[:, 0], p[:, 1])
    assert np.array_equal(BD.distort_points(p, _lens(t)), np.stack([ud, vd], 1))
    if size == (W, H):  # what the bound is for: half the rounds miss it
        u20, v20 = R.undistort(t, p[:, 0], p[:, 1], rounds=20)
        ud20, vd20 = R.distort(t, u20, v20)
        if name == "barrel":
            assert max(np.abs(ud20 - p[:, 0]).max(), np.abs(vd20 - p[:, 1]).max()) > 1e-9


def _footprint(t, Minv, S):
    r = (C.c_int32 * 4)()
    Minv = np.ascontiguousarray(Minv, dtype=np.float64)
    rc = N.load().cbv_lens_warp_footprint(_lens(t).struct() if t else None, N.ptr(Minv), S, S, W, H, r)
    assert rc in (0, 1)
    return tuple(r) if rc else None


@pytest.mark.parametrize("name", sorted(LENSES))
def test_footprint_bounds_every_tap_within_its_margin(name):
    t, S = LENSES[name], 100
    Minv = R.invert3x3(_ideal_matrix(t, S))
    X, Y = R.coords(t, Minv, S, S)
    sx, sy = X >> 5, Y >> 5
    x0, y0, x1, y1 = _footprint(t, Minv, S)
    assert x0 <= sx.min() and sx.max() + 1 < x1 and y0 <= sy.min() and sy.max() + 1 < y1
    assert x0 >= sx.min() - 6 and x1 <= sx.max() + 8 and y0 >= sy.min() - 6 and y1 <= sy.max() + 8  # and is no looser than its margin
    # no lens: the projective footprint of the same matrix
    assert _footprint(None, Minv, S) is not None


def test_refusals():
    lib = N.load()
    p = np.zeros((1, 2))
    for field, bad in [("fx", 0.0), ("fy", -1.0), ("fx", float("nan")), ("cx", float("inf")), ("k1", float("nan")), ("p2", float("-inf")), ("k3", float("nan"))]:
        s = _lens(R.BARREL).struct()
        setattr(s, field, bad)
        out = np.full((1, 2), 7.0)
        assert lib.cbv_lens_undistort_points(s, N.ptr(p), 1, N.ptr(out)) == -1, (field, bad)
        assert lib.cbv_lens_distort_points(s, N.ptr(p), 1, N.ptr(out)) == -1
        xy = np.full((2, 2, 2), 7, np.int32)
        assert lib.cbv_lens_warp_coords(s, N.ptr(np.eye(3)), 2, 2, N.ptr(xy)) == -1
        assert np.all(out == 7.0) and np.all(xy == 7)  # nothing written
    assert lib.cbv_lens_undistort_points(None, N.ptr(p), 1, N.ptr(p)) == -1
    with pytest.raises(ValueError):
        BD.undistort_points(p, ST.Lens(0, 1, 0, 0))


def test_lens_from_opencv_scaled_and_files(tmp_path):
    K = [[1400.0, 0, 960.0], [0, 1390.0, 540.0], [0, 0, 1]]
    l5 = ST.Lens.from_opencv(K, [[-0.28, 0.09, 0.001, -0.0005, -0.012]])
    assert (l5.fx, l5.fy, l5.cx, l5.cy, l5.k1, l5.k2, l5.p1, l5.p2, l5.k3) == (1400.0, 1390.0, 960.0, 540.0, -0.28, 0.09, 0.001, -0.0005, -0.012)
    l4 = ST.Lens.from_opencv(np.array(K), [-0.28, 0.09, 0.001, -0.0005])
    assert l4.k3 == 0.0 and l4.p2 == -0.0005
    assert ST.Lens.from_opencv(K, [-0.28, 0.09, 0.001, -0.0005, -0.012, 0, 0, 0]) == l5
    with pytest.raises(ValueError):
        ST.Lens.from_opencv(K, [-0.28, 0.09, 0.001, -0.0005, -0.012, 0.01, 0, 0])
    with pytest.raises(ValueError):
        ST.Lens.from_opencv(K, [-0.28, 0.09, 0.001])
    half = l5.scaled((1920, 1080), (960, 540))
    assert (half.fx, half.fy, half.cx, half.cy) == (700.0, 695.0, 480.0, 270.0) and half.dist_coeffs.tolist() == l5.dist_coeffs.tolist()
    # a scaled lens maps scaled points to scaled points
    p = np.array([[100.0, 50.0], [1800.0, 1000.0]])
    assert np.abs(BD.undistort_points(p / 2, half) - BD.undistort_points(p, l5) / 2).max() < 1e-9
    path = tmp_path / "lens.json"
    wrote = ST.save_lens(str(path), l5, image_size=(1920, 1080))
    assert set(wrote) == {"camera_matrix", "dist_coeffs", "image_size"} and json.load(open(path)) == wrote
    assert ST.load_lens(str(path)) == l5 and ST.load_lens(str(path), with_size=True) == (l5, (1920, 1080))
    ST.save_lens(str(path), l4)
    assert ST.load_lens(str(path), with_size=True) == (l4, None)
    s = l5.struct()
    assert s.enabled == 1 and s.k3 == -0.012 and C.sizeof(N.LensStruct) == 80
