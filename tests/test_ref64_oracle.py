"""The CPU oracle against tests/ref64.py, the float64 restatement written from each operation's definition.

Every GPU test compares a kernel with the oracle bit for bit, so a convention both of them got wrong (window shape,
border mode, tile centre, correlation vs convolution, ...) would pass there.  Here the oracle has to land inside a
derived envelope around the definition (tests/ref64_checks.py), at the shapes, inputs and parameters the GPU suite
sweeps.  test_gpu_ref64.py runs the same checks on the HIP kernels' output."""
import numpy as np
import pytest

import ref64 as R
import ref64_checks as K

from ref64_checks import CLAHE_SWEEP, GPU_BILATERAL_SWEEP, quad_matrix, random_kernels, random_quad_case, shapes_and_contents


# ------------------------------------------------------------------ point operations


@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (1.37, -20.3), (-0.71, 12.9), (2.53, -140.2), (0.93, 12.1)])
def test_convert_scale_abs(oracle, alpha, beta):
    x = np.arange(256, dtype=np.uint8).reshape(16, 16)
    # float32 alpha, beta and one fused multiply-add: error below 4 u * (255 |alpha| + |beta|)
    eps = 4 * K.U32 * (255 * abs(alpha) + abs(beta))
    K.check_rounded(oracle.convert_scale_abs(x, alpha, beta), R.convert_scale_abs(x, alpha, beta), eps, "convertScaleAbs")


def test_bgr2hsv_whole_cube(oracle):
    cube = np.arange(1 << 24, dtype=np.uint32)
    for part in np.array_split(cube, 8):
        img = np.stack([part & 255, (part >> 8) & 255, part >> 16], axis=-1).astype(np.uint8).reshape(-1, 4096, 3)
        K.check_bgr2hsv(oracle.bgr2hsv(img), img)


def test_hsv2bgr_sampled_triples(oracle):
    h, s, v = np.meshgrid(np.arange(180), np.arange(0, 256, 3), np.arange(0, 256, 3), indexing="ij")
    hsv = np.stack([h, s, v], axis=-1).astype(np.uint8).reshape(180, -1, 3)
    K.check_hsv2bgr(oracle.hsv2bgr(hsv), hsv)


@pytest.mark.parametrize("direction", ["bgr2lab", "lab2bgr"])
def test_lab_whole_cube(oracle, direction):
    cube = np.arange(1 << 24, dtype=np.uint32)
    fn, ref = (oracle.bgr2lab, R.bgr2lab) if direction == "bgr2lab" else (oracle.lab2bgr, R.lab2bgr)
    worst = np.zeros(3)
    over = 0
    for part in np.array_split(cube, 16):
        img = np.stack([part & 255, (part >> 8) & 255, part >> 16], axis=-1).astype(np.uint8).reshape(-1, 1024, 3)
        d = np.abs(fn(img).astype(np.float64) - ref(img))
        worst = np.maximum(worst, d.reshape(-1, 3).max(axis=0))
        over += int((d > 1).sum())
    assert (worst <= K.LAB_MAX).all(), (direction, worst)
    assert over / (3 << 24) <= K.LAB_SHARE_OVER_1, (direction, over / (3 << 24))


@pytest.mark.parametrize("w,h,content", shapes_and_contents())
def test_profile_neutral_is_hsv_round_trip(oracle, w, h, content):
    img = K.frame(content, w, h)
    neutral = {"contrast": 1.0, "brightness": 0, "sat_scale": 1.0, "val_scale": 1.0, "hue_shift": 0}
    K.check_profile_neutral(oracle.apply_color_profile(K.view(img), neutral), img)


@pytest.mark.parametrize("w,h,content", shapes_and_contents())
def test_gray_blur_otsu(oracle, w, h, content):
    img = K.frame(content, w, h)
    gray, binary, t = oracle.prepare_analysis(K.view(img))
    K.check_prepare_analysis(gray, binary, t, img)
    K.check_blur(oracle.gaussian_blur(gray, 5), gray)


def test_otsu_threshold_maximises_variance(oracle):
    rng = np.random.default_rng(5)
    for _ in range(50):
        hist = rng.integers(0, 50, 256) * (rng.random(256) < rng.uniform(0.05, 1))
        hist[rng.integers(0, 256, 2)] += 1
        t = oracle.otsu_from_hist(hist)
        _, var = R.otsu_threshold(hist)
        assert var[t] >= var.max() * (1 - 1e-12), (t, int(np.argmax(var)))


@pytest.mark.parametrize("w,h,content", shapes_and_contents())
def test_normalize(oracle, w, h, content):
    img = K.frame(content, w, h)
    K.check_normalize(oracle.normalize_minmax(K.view(img)), img)


def test_normalize_channels_with_different_ranges(oracle):
    img = K.smooth(120, 90, 3)
    img[..., 0] = img[..., 0] // 4 + 60                  # blue spans about 64 levels, red the whole range
    img[..., 1] = img[..., 1] // 2
    K.check_normalize(oracle.normalize_minmax(img), img)
    flat = np.full((9, 11, 3), 200, np.uint8)
    assert not oracle.normalize_minmax(flat).any()
    K.check_normalize(oracle.normalize_minmax(flat), flat)


# ------------------------------------------------------------------ neighbourhood operations


@pytest.mark.parametrize("w,h,content", shapes_and_contents())
def test_bilateral_reference_parameters(oracle, w, h, content):
    img = K.frame(content, w, h)
    K.check_bilateral(oracle.bilateral(K.view(img), 9, 75.0, 75.0), img, 9, 75.0, 75.0)


@pytest.mark.parametrize("d,sc,ss", GPU_BILATERAL_SWEEP)
@pytest.mark.parametrize("w,h,content", [(131, 97, "noise"), (35, 33, "edges"), (3, 5, "smooth"), (1, 7, "noise")])
def test_bilateral_sweep(oracle, d, sc, ss, w, h, content):
    img = K.frame(content, w, h)
    K.check_bilateral(oracle.bilateral(K.view(img), d, sc, ss), img, d, sc, ss)


@pytest.mark.parametrize("w,h,content", shapes_and_contents())
def test_filter2d(oracle, w, h, content):
    img = K.frame(content, w, h)
    K.check_filter2d(oracle.filter3x3(K.view(img)), img, oracle.SHARPEN_KERNEL)
    for k in random_kernels(w * 31 + h, 2):
        K.check_filter2d(oracle.filter3x3(K.view(img), k), img, k)


@pytest.mark.parametrize("clip,tiles", CLAHE_SWEEP)
@pytest.mark.parametrize("w,h,content", [(96, 72, "smooth"), (160, 120, "noise"), (37, 29, "smooth"), (7, 5, "noise"),
                                         (13, 1, "smooth"), (1, 11, "noise"), (63, 9, "edges"), (64, 64, "const")])
def test_clahe(oracle, clip, tiles, w, h, content):
    gray = R.bgr2gray_q15(K.frame(content, w, h))
    out, luts = oracle.clahe(K.view(gray), clip, tiles, return_lut=True)
    K.check_clahe(out, gray, clip, tiles, luts=luts)


@pytest.mark.parametrize("clip,tiles", CLAHE_SWEEP)
@pytest.mark.parametrize("w,h", [(160, 120), (37, 29), (16, 12), (7, 5)])
def test_correct_lighting_composite(oracle, clip, tiles, w, h):
    img = K.lighting_frame(w, h, w + h, tiles)
    K.check_correct_lighting(oracle.correct_lighting(img, clip, tiles), img, clip, tiles)


@pytest.mark.parametrize("seed", range(12))
def test_warp_random_quads(oracle, seed):
    img, M, dsize = random_quad_case(seed)
    K.check_warp(oracle.warp_perspective(K.view(img), M, dsize), img, M, dsize)


def test_warp_board_quad(oracle):
    from chessboard_vision_amd import synth as S
    img = K.smooth(640, 480, 4)
    pts = np.float64(S.scaled_corners(640, 480))
    M = quad_matrix(pts, np.float64([[0, 0], [620, 0], [0, 620], [620, 620]]))
    K.check_warp(oracle.warp_perspective(img, M, (620, 620)), img, M, (620, 620))


# ------------------------------------------------------------------ one 1080p frame through every stage


def test_1080p_frame(oracle):
    img = K.smooth(1920, 1080, 11)
    K.check_bilateral(oracle.bilateral(img), img)
    K.check_filter2d(oracle.filter3x3(img), img, oracle.SHARPEN_KERNEL)
    K.check_normalize(oracle.normalize_minmax(img), img)
    gray, binary, t = oracle.prepare_analysis(img)
    K.check_prepare_analysis(gray, binary, t, img)
    out, luts = oracle.clahe(gray, 3.0, (8, 8), return_lut=True)
    K.check_clahe(out, gray, 3.0, (8, 8), luts=luts)
