"""The detector-side definitions of tests/ref64.py (GaussianBlur k = 1..31, Canny) on the CPU: properties the definitions
must have by themselves, and the CPU oracle under the same checkers and inputs as test_gpu_ref64_detectors.py runs on the HIP
kernels.  The oracle's Canny and blur were written from the same reading of OpenCV as the kernels; here they have to meet a
second statement of the definition that shares none of their code."""
import ctypes as C

import numpy as np
import pytest

import ref64 as R
import ref64_checks as K


# ------------------------------------------------------------------ the definitions themselves


def test_fixed_point_sectors_equal_real_angle_sectors():
    """Every (|dx|, |dy|) an 8-bit Sobel can give (0..1020 each): the integer sector test of Canny, tan 22.5 degrees as
    13573 / 2^15 and tan 67.5 degrees = tan 22.5 degrees + 2, restated here, picks the sector of the real angle.  The one
    pair left out is (0, 0): a zero gradient has no angle, and with M = 0 it is no candidate under any threshold >= 0."""
    ax, ay = np.meshgrid(np.arange(1021, dtype=np.int64), np.arange(1021, dtype=np.int64), indexing="ij")
    horizontal = (ay << 15) < ax * 13573
    vertical = (ay << 15) > ax * 13573 + (ax << 16)
    fixed = np.where(horizontal, 0, np.where(vertical, 1, 2))
    real = R.canny_sector(ax, ay)
    differ = fixed != real
    differ[0, 0] = False
    assert int(differ.sum()) == 0 and differ.size == 1021 * 1021
    t = np.abs(ay[1:, 1:] / ax[1:, 1:] - np.tan(np.radians(22.5)))
    assert 1e-7 < t.min() < 1e-6  # the nearest ratio is far from the boundary in float64 terms


@pytest.mark.parametrize("k", K.BLUR_KS)
def test_gaussian_q8_coefficients(k):
    q, c = R.gaussian_q8(k), R.gaussian_kernel(k)
    assert len(q) == len(c) == k and abs(c.sum() - 1) < 1e-15 and np.array_equal(c, c[::-1])
    assert np.array_equal(q, q[::-1]) and int(q.sum()) == 256
    e = q - 256.0 * c
    assert (np.abs(e) < 1).all(), e
    assert (np.abs(np.cumsum(e)) <= 0.5).all(), np.cumsum(e)  # error diffusion; a wrong sigma breaks this
    if k <= 7:
        assert not e.any()
        assert K.gaussian_e1(k) == 0.0
    else:
        sigma = 0.3 * ((k - 1) / 2 - 1) + 0.8
        x = np.arange(k) - k // 2
        assert np.allclose(c[k // 2 + 1] / c[k // 2], np.exp(-1 / (2 * sigma * sigma)), rtol=1e-14)
        assert np.allclose(c, np.exp(-x * x / (2 * sigma * sigma)) / np.exp(-x * x / (2 * sigma * sigma)).sum(), rtol=1e-14)


def test_five_by_five_is_the_k5_case():
    """gaussian_blur_5x5* (used by check_blur and check_prepare_analysis) against the binomial kernel written out."""
    for (w, h, content) in K.shapes_and_contents():
        g = R.bgr2gray_q15(K.frame(content, w, h))
        f = g.astype(np.float64)
        b = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
        p = R._pad101(f, 2, 2)
        tmp = sum(b[j] * p[:, j:j + w] for j in range(5))
        want = sum(b[i] * tmp[i:i + h] for i in range(5))
        assert np.array_equal(R.gaussian_blur_5x5(g), want) and np.array_equal(R.gaussian_blur(g, 5), want)
        assert np.array_equal(R.gaussian_blur_5x5_u8(g), np.floor(want + 0.5).astype(np.uint8))


def test_reflection_repeats_beyond_the_array():
    g = np.array([[10, 20, 30]], np.uint8)
    # radius 15 on a length-3 axis: positions -15..17 fold with period 4 onto 0 1 2 1
    idx = R.reflect101_index(np.arange(-15, 18), 3)
    assert list(idx[:8]) == [1, 2, 1, 0, 1, 2, 1, 0] and idx[15] == 0
    c = R.gaussian_kernel(31)
    want = [float((c * g[0, R.reflect101_index(np.arange(x - 15, x + 16), 3)]).sum()) for x in range(3)]
    assert np.allclose(R.gaussian_blur(g, 31)[0], want, rtol=0, atol=1e-12)


def test_sobel_and_canny_known_answers():
    """A vertical step of height a: dx = 4a on the two columns beside it, dy = 0; OpenCV's tie rule keeps the left column."""
    g = np.full((6, 8), 50, np.uint8)
    g[:, 4:] = 90
    dx, dy = R.sobel3(g)
    assert not dy.any() and (dx[:, 3:5] == 160).all() and not dx[:, :3].any() and not dx[:, 5:].any()
    strict, loose, conv = R.canny_sets(g, 50, 150)
    assert not strict.any() and loose[:, 3:5].all() and loose.sum() == 12
    assert conv[:, 3].all() and conv.sum() == 6
    assert not R.canny_sets(g, 50, 160)[2].any()                      # M > high is strict
    assert not R.canny_sets(g, 160, 200)[2].any() and R.canny_sets(g, 159.9, 10)[2].sum() == 6


# ------------------------------------------------------------------ the oracle under both checkers


@pytest.mark.parametrize("k", K.BLUR_KS)
def test_oracle_coefficients_and_blur(oracle, k):
    coef = (C.c_int * 64)()
    oracle.lib().orc_gaussian_kernel_q8(k, coef)
    assert list(coef[:k]) == list(R.gaussian_q8(k))
    for key, img in K.blur_squares().items():
        out = oracle.square_preprocess(img, k)
        if img.ndim == 3:
            gray = R.bgr2gray_q15(img)
            K.check_gray(gray, img)
        else:
            gray = img
            assert np.array_equal(oracle.gaussian_blur(img, k), out)
        K.check_gaussian(out, gray, k)


@pytest.mark.parametrize("h,w,content,t", K.canny_cases(), ids=str)
def test_oracle_canny(oracle, h, w, content, t):
    gray = K.canny_input(content, h, w)
    K.check_canny(oracle.canny(gray, *t), gray, *t, tie_cap=K.canny_tie_cap(content, h, w))


@pytest.mark.parametrize("end", ["left", "right"])
def test_oracle_canny_tile_crossing_curve(oracle, end):
    gray = K.hysteresis_curve(end)
    K.check_hysteresis_curve(oracle.canny(gray, *K.CURVE_THRESHOLDS), end)


def test_oracle_canny_magnitude_equal_to_a_threshold(oracle):
    K.check_threshold_step(oracle.canny)


@pytest.mark.parametrize("param1", [100, 60])
def test_oracle_hough_edge_map(oracle, param1):
    from test_gpu_stages import _hough_squares
    n = 0
    for g in _hough_squares(oracle):
        _, edges = oracle.hough_circles(g, 1.2, min(g.shape) // 3, param1, 25, int(min(g.shape) * 0.2), int(min(g.shape) * 0.55),
                                        return_edges=True)
        n += K.check_canny(edges, g, param1 / 2, param1)["edges"]
    assert n > 1000


def test_oracle_hough_edge_map_magnitude_equal_to_low(oracle):
    """param1 = 80: low = 40 is the magnitude of the weak stretch of threshold_step(), which must stay out."""
    g = K.threshold_step()
    assert R.canny_sets(g, 40, 80)[2].sum() < R.canny_sets(g, 38, 80)[2].sum()
    _, edges = oracle.hough_circles(g, 1.2, 13, 80, 25, 8, 22, return_edges=True)
    K.check_canny(edges, g, 40, 80)
