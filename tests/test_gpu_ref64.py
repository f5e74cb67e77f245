"""The HIP kernels against tests/ref64.py directly: the same inputs and envelope checks as test_ref64_oracle.py, with
the expected values computed on the host from each operation's definition and never from the oracle.  The library
has no stand-alone Lab or HSV call, so the colour conversions are reached through the neutral colour profile (an HSV
round trip) and through correct_lighting (Lab -> CLAHE(L) -> BGR) on inputs whose bound can be derived.  The colour profile
away from the neutral setting (its byte map, its hue, saturation and value maps, the radical window) is held to
ref64_checks.check_profile, one admissible value per pixel: cbv_apply_color_profile, the warp's own copy of the table
consumer, and the context's table cache."""
import ctypes as C
import os

import numpy as np
import pytest

import ref64 as R
import ref64_checks as K
from ref64_checks import CLAHE_SWEEP, GPU_BILATERAL_SWEEP, quad_matrix, random_kernels, random_quad_case, shapes_and_contents

pytestmark = pytest.mark.gpu

NEUTRAL = {"contrast": 1.0, "brightness": 0, "sat_scale": 1.0, "val_scale": 1.0, "hue_shift": 0}


@pytest.fixture(scope="module")
def enh(gpu_ctx, tmp_path_factory):
    from chessboard_vision_amd.frame_enhancer import ImageEnhancer
    cwd = os.getcwd()
    os.chdir(tmp_path_factory.mktemp("noprofile"))  # no color_profile.json in cwd
    try:
        e = ImageEnhancer()
    finally:
        os.chdir(cwd)
    assert e.profile == {}
    return e


def reduce_noise(ctx, img, d, sc, ss):
    h, w = img.shape[:2]
    out = np.empty((h, w, 3), np.uint8)
    ctx.check(ctx.lib.cbv_reduce_noise(ctx.h, img.ctypes.data, w, h, img.strides[0], d, sc, ss, out.ctypes.data, out.strides[0]))
    return out


def prepare_analysis(ctx, img):
    h, w = img.shape[:2]
    gray = np.empty((h, w), np.uint8)
    binary = np.empty((h, w), np.uint8)
    t = C.c_int(-1)
    ctx.check(ctx.lib.cbv_prepare_analysis(ctx.h, img.ctypes.data, w, h, img.strides[0], gray.ctypes.data, w,
                                           binary.ctypes.data, w, C.byref(t)))
    return gray, binary, t.value


@pytest.mark.parametrize("w,h,content", shapes_and_contents())
def test_reduce_noise_reference_parameters(enh, w, h, content):
    img = K.frame(content, w, h)
    K.check_bilateral(enh.reduce_noise(K.view(img)), img, 9, 75.0, 75.0)


@pytest.mark.parametrize("d,sc,ss", GPU_BILATERAL_SWEEP)
@pytest.mark.parametrize("w,h,content", [(131, 97, "noise"), (35, 33, "edges"), (3, 5, "smooth"), (1, 7, "noise")])
def test_reduce_noise_sweep(gpu_ctx, d, sc, ss, w, h, content):
    img = K.frame(content, w, h)
    K.check_bilateral(reduce_noise(gpu_ctx, K.view(img), d, sc, ss), img, d, sc, ss)


@pytest.mark.parametrize("w,h,content", shapes_and_contents())
def test_sharpen(enh, w, h, content):
    img = K.frame(content, w, h)
    old = enh.sharpen_kernel
    try:
        K.check_filter2d(enh.sharpen(K.view(img)), img, old)
        for k in random_kernels(w * 31 + h, 2):
            enh.sharpen_kernel = k
            K.check_filter2d(enh.sharpen(K.view(img)), img, k)
    finally:
        enh.sharpen_kernel = old


@pytest.mark.parametrize("w,h,content", shapes_and_contents())
def test_normalize(enh, w, h, content):
    img = K.frame(content, w, h)
    K.check_normalize(enh.normalize_intensity(K.view(img)), img)


def test_normalize_channels_with_different_ranges(enh):
    img = K.smooth(120, 90, 3)
    img[..., 0] = img[..., 0] // 4 + 60
    img[..., 1] = img[..., 1] // 2
    K.check_normalize(enh.normalize_intensity(img), img)
    flat = np.full((9, 11, 3), 200, np.uint8)
    K.check_normalize(enh.normalize_intensity(flat), flat)


@pytest.mark.parametrize("w,h,content", shapes_and_contents())
def test_prepare_analysis(gpu_ctx, enh, w, h, content):
    img = K.frame(content, w, h)
    gray, binary, t = prepare_analysis(gpu_ctx, K.view(img))
    K.check_prepare_analysis(gray, binary, t, img)
    g2, b2 = enh.prepare_analysis(K.view(img))
    assert np.array_equal(g2, gray) and np.array_equal(b2, binary)


@pytest.mark.parametrize("clip,tiles", CLAHE_SWEEP)
@pytest.mark.parametrize("w,h,content", [(96, 72, "smooth"), (160, 120, "noise"), (37, 29, "smooth"), (7, 5, "noise"),
                                         (13, 1, "smooth"), (1, 11, "noise"), (63, 9, "edges"), (64, 64, "const")])
def test_clahe_apply(enh, clip, tiles, w, h, content):
    gray = R.bgr2gray_q15(K.frame(content, w, h))
    enh.clahe.setClipLimit(clip)
    enh.clahe.setTilesGridSize(tiles)
    try:
        K.check_clahe(enh.clahe.apply(K.view(gray)), gray, clip, tiles)
    finally:
        enh.clahe.setClipLimit(3.0)
        enh.clahe.setTilesGridSize((8, 8))


@pytest.mark.parametrize("clip,tiles", CLAHE_SWEEP)
@pytest.mark.parametrize("w,h", [(160, 120), (37, 29), (16, 12), (7, 5)])
def test_correct_lighting_composite(gpu_ctx, clip, tiles, w, h):
    from chessboard_vision_amd.frame_enhancer import ImageEnhancer
    e = ImageEnhancer(clahe_clip_limit=clip, tile_grid_size=tiles)
    img = K.lighting_frame(w, h, w + h, tiles)
    K.check_correct_lighting(e.correct_lighting(img), img, clip, tiles)


@pytest.mark.parametrize("w,h,content", shapes_and_contents())
def test_profile_neutral_is_hsv_round_trip(enh, w, h, content):
    img = K.frame(content, w, h)
    enh.profile = NEUTRAL
    try:
        K.check_profile_neutral(enh.apply_color_profile(K.view(img)), img)
    finally:
        enh.profile = {}


def test_profile_neutral_sampled_cube(enh):
    """Every third level of each channel: the BGR -> HSV -> BGR round trip over 86^3 colours in one frame."""
    v = np.arange(0, 256, 3, dtype=np.uint8)
    b, g, r = np.meshgrid(v, v, v, indexing="ij")
    img = np.stack([b, g, r], axis=-1).reshape(86 * 86, 86, 3)
    enh.profile = NEUTRAL
    try:
        K.check_profile_neutral(enh.apply_color_profile(img), img)
    finally:
        enh.profile = {}


# ------------------------------------------------------------------ the colour profile beyond the neutral setting


@pytest.fixture
def profiled(enh):
    """apply(img, profile): cbv_apply_color_profile through ImageEnhancer.apply_color_profile."""
    def apply(img, profile):
        enh.profile = profile
        try:
            return enh.apply_color_profile(img)
        finally:
            enh.profile = {}
    return apply


def warp_identity(rot180):
    """apply(img, profile): k_warp_profile at integer positions, where the 1/32-pixel blend is exact: the warp's own copy of
    the table consumer and nothing else.  With rot180 the output is turned back, so the checks compare against the reference
    reversed."""
    from chessboard_vision_amd.board_detection import warp_perspective_profiled

    def apply(img, profile):
        out = warp_perspective_profiled(img, np.eye(3), (img.shape[1], img.shape[0]), profile, rot180=rot180)
        return out[::-1, ::-1] if rot180 else out
    return apply


@pytest.mark.parametrize("name,offset", K.profile_cube_cases())
def test_profile_on_cube(profiled, name, offset):
    """86^2 x 86 pixels, one launch per cube (and one of 256 pixels for the byte map)."""
    s = K.check_profile_cube(profiled, name, offset)
    print("profile %s cube %d: max %.4f, over 1 LSB %.4f, ties %d" % (name, offset, s["max"], s["over1"], s["ties"]))


@pytest.mark.parametrize("name", list(K.PROFILE_CASES))
def test_profile_on_small_frames(profiled, name):
    K.check_profile_frames(profiled, name)


WARP_PROFILES = ("shipped", "radical_wrap", "clipping", "neg_contrast")


@pytest.mark.parametrize("rot180", [False, True])
@pytest.mark.parametrize("name", WARP_PROFILES)
def test_warp_profile_table_consumer(gpu_ctx, name, rot180):
    """warp_perspective_profiled with the identity matrix against the definition directly, not against
    cbv_apply_color_profile: the cube with offset 0 as an 860 x 740 frame (its first 344 colours once more fill the last
    row) and the 37 x 29 frame as a strided view."""
    apply = warp_identity(rot180)
    profile = K.PROFILE_CASES[name]
    byte_map = K.observed_byte_map(apply, profile)

    def as_frame(a):
        flat = a.reshape(-1, 3)
        return np.concatenate([flat, flat[:860 * 740 - len(flat)]]).reshape(740, 860, 3)

    cube = as_frame(K.color_cube(0))
    K.check_profile(apply(cube, profile), cube, profile, byte_map, ref=as_frame(K.cube_reference(name, 0, byte_map.tobytes())),
                    tie_cap=K.PROFILE_TIE_CAP, what="warp profile %s rot180=%d, cube" % (name, rot180))
    img = K.frame("noise", 37, 29)
    K.check_profile(apply(K.view(img), profile), img, profile, byte_map, what="warp profile %s rot180=%d, 37x29" % (name, rot180))


@pytest.mark.parametrize("a,b", [("shipped", "radical_wrap"), ("radical_wrap", dict(K.PROFILE_CASES["radical_wrap"], hue_window=13)),
                                 ("neg_contrast", {"contrast": -0.71, "brightness": 13.9})])
def test_profile_table_cache(profiled, a, b):
    """The context keeps the tables of the last profile and compares the next one with it: A, B, A on one context, B a
    different profile or A with one field changed.  Each output is held to its own profile, and the two of A are equal."""
    pa, pb = K.PROFILE_CASES[a], (K.PROFILE_CASES[b] if isinstance(b, str) else b)
    img = K.frame("noise", 37, 29)
    maps = [K.observed_byte_map(profiled, p) for p in (pa, pb, pa)]
    outs = [profiled(K.view(img), p) for p in (pa, pb, pa)]                 # back to back: nothing else sets a profile between
    for p, byte_map, out in zip((pa, pb, pa), maps, outs):
        K.check_profile(out, img, p, byte_map, what="profile after another profile")
    assert np.array_equal(outs[0], outs[2])
    assert not np.array_equal(outs[0], outs[1]), "the two profiles do not differ on this frame: the case says nothing"


@pytest.mark.parametrize("seed", range(12))
def test_warp_random_quads(gpu_ctx, seed):
    from chessboard_vision_amd.board_detection import warp_perspective
    img, M, dsize = random_quad_case(seed)
    K.check_warp(warp_perspective(K.view(img), M, dsize), img, M, dsize)


def test_warp_board_quad(gpu_ctx):
    from chessboard_vision_amd import synth as S
    from chessboard_vision_amd.board_detection import warp_perspective
    img = K.smooth(640, 480, 4)
    M = quad_matrix(np.float64(S.scaled_corners(640, 480)), np.float64([[0, 0], [620, 0], [0, 620], [620, 620]]))
    K.check_warp(warp_perspective(img, M, (620, 620)), img, M, (620, 620))


def test_1080p_frame(gpu_ctx, enh):
    img = K.smooth(1920, 1080, 11)
    K.check_bilateral_bands(enh.reduce_noise(img), img)
    K.check_filter2d(enh.sharpen(img), img, enh.sharpen_kernel)
    K.check_normalize(enh.normalize_intensity(img), img)
    gray, binary, t = prepare_analysis(gpu_ctx, img)
    K.check_prepare_analysis(gray, binary, t, img)
    K.check_clahe(enh.clahe.apply(gray), gray, 3.0, (8, 8))


def test_4k_bilateral_normalize_warp(gpu_ctx, enh):
    from chessboard_vision_amd.board_detection import warp_perspective
    w, h = 3840, 2160
    img = K.smooth(w, h, 12)
    img[h // 3:h // 2, w // 5:w // 3] = K.noise(w // 3 - w // 5, h // 2 - h // 3, 5)   # a noisy patch: large colour distances
    K.check_bilateral_bands(enh.reduce_noise(img), img)
    K.check_normalize(enh.normalize_intensity(img), img)
    src = np.float64([[310.5, 220.25], [3560.0, 140.0], [120.0, 2050.75], [3700.25, 2110.0]])
    M = quad_matrix(src, np.float64([[0, 0], [1900, 0], [0, 1060], [1900, 1060]]))
    K.check_warp(warp_perspective(img, M, (1920, 1080)), img, M, (1920, 1080))
