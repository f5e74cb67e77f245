"""The batched d = 9 bilateral (k_bilateral<4, 768, PAIRS>) shares, inside a lane, the tap weights that connect two of
the lane's own eight outputs (a 4-pixel strip on two adjacent rows): the weight between pixels of one row is looked up
by the right-hand one and reused by the left-hand one, the weight between a pixel of the lower row and one of the
upper row is looked up by the lower one and reused by the upper one.  A wrong partner index, a weight taken from the
wrong row of the pair or a stale register shows as a wrong output byte, so every case compares with the oracle
bit for bit.

cbv_reduce_noise launches one frame; the 768-lane form is taken when the frame has at least 2 x CUs tiles of
128 x 48 pixels (bilateral_nt in k_bilateral.hip), so the frames here are very wide or very tall instead of many."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TW, TH = 128, 48            # tile of the 768-lane form


@pytest.fixture(scope="module")
def min_tiles(gpu_ctx):
    """bilateral_nt's threshold: 2 x the compute units of the context's device.  The count is asked of the HIP runtime
    that the library itself is linked to (a symbol looked up through the library's handle resolves in its dependencies):
    another copy of the runtime loaded by name, such as the one a Python package bundles, may see no device at all."""
    import ctypes
    lib = gpu_ctx.lib
    cus = ctypes.c_int(0)
    assert lib.hipDeviceGetAttribute(ctypes.byref(cus), 63, gpu_ctx.device_id) == 0    # hipDeviceAttributeMultiprocessorCount
    assert cus.value > 0
    return 2 * cus.value


def _tiles(h, w):
    return ((w + TW - 1) // TW) * ((h + TH - 1) // TH)


def _noise(h, w, seed):
    """White noise: every weight of a pixel's disc is distinct, a swapped or stale one cannot hide."""
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _steps(h, w, seed):
    """Two colours 20 apart per channel plus +-1 of noise, in blocks of 3 x 5 pixels: weights near 1 and near 0 side by
    side inside every 4 x 2 strip pair."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    two = (((yy // 3) + (xx // 5)) & 1).astype(np.uint8)
    f = np.where(two[..., None] == 1, np.uint8(200), np.uint8(40)) + rng.integers(0, 3, (h, w, 3), dtype=np.uint8)
    return np.ascontiguousarray(f.astype(np.uint8))


# (h, w): all select the 768-lane form on a 256-CU device (checked in the test against the device's own count)
SHAPES = [
    (2, 65536),       # one row pair: the two own rows meet REFLECT_101 rows above and below
    (2, 65537),       # width 1 mod 4: a one-pixel strip at the right edge and a row stride that is no multiple of 4
    (24576, 5),       # narrower than the 9 x 9 disc: REFLECT_101 on both sides at once, 512 tiles one above the other
    (12288, 129),     # one pixel wider than a tile
    (49, 32646),      # tile height + 1, width 2 mod 4
    (47, 65539),      # tile height - 1 (the last row pair's lower row is outside the frame), width 3 mod 4
    (97, 21764),      # 2 x tile height + 1: tiles above each other, stride a multiple of 4
]


@pytest.mark.parametrize("content", ["noise", "steps"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_batched_bilateral_with_shared_weights_equals_oracle(gpu_ctx, oracle, min_tiles, shape, content):
    h, w = shape
    assert _tiles(h, w) >= min_tiles, "the frame must select the 768-lane form"
    f = _noise(h, w, h + w) if content == "noise" else _steps(h, w, h + w)
    out = np.empty_like(f)
    gpu_ctx.check(gpu_ctx.lib.cbv_reduce_noise(gpu_ctx.h, f.ctypes.data, w, h, f.strides[0], 9, 75.0, 75.0, out.ctypes.data, out.strides[0]))
    want = oracle.bilateral(f, 9, 75, 75)
    assert np.array_equal(out, want), (shape, content, int((out != want).sum()))


def test_strided_input_and_other_sigmas(gpu_ctx, oracle, min_tiles):
    """A view into a wider buffer (odd byte offset and stride) and narrow sigmas, where most weights are exactly 0."""
    h, w = 50, 32645
    assert _tiles(h, w) >= min_tiles
    big = _noise(h, w + 5, 7)
    big[h // 3:2 * h // 3, w // 4:w // 2] //= 3
    f = big[:, 2:2 + w]
    for sc, ss in ((75.0, 75.0), (10.0, 3.0)):
        out = np.empty((h, w, 3), np.uint8)
        gpu_ctx.check(gpu_ctx.lib.cbv_reduce_noise(gpu_ctx.h, f.ctypes.data, w, h, f.strides[0], 9, sc, ss, out.ctypes.data, out.strides[0]))
        want = oracle.bilateral(np.ascontiguousarray(f), 9, sc, ss)
        assert np.array_equal(out, want), (sc, ss, int((out != want).sum()))
