"""The batched d = 9 bilateral (k_bilateral<4, NT, PAIRS>) is straight-line code for the whole tile: every tile row carries
its table offsets as compile-time constants, the taps are looked up half a pixel step ahead of their FMAs and the row
is read in pixel pairs.  A wrong row constant, a disc extent off by one, a weight taken from the wrong step of the
software pipeline or a pixel pair loaded for the wrong row shows as a wrong output byte, so every case compares with
the oracle bit for bit.

The shapes sit around a tile height of 64, that of the 1024-lane build (BL_NT1024=1), and hold for the default 768-lane
build (tile height 48) as they are: there they are further positions of the frame's last rows inside a tile.
bilateral_nt chooses the batched form by the count of 128 x 48 tiles (at least 2 x CUs) in both builds, so the frames
are wide or tall ones like those of test_gpu_bilateral_pairs.py."""
import numpy as np
import pytest

from test_gpu_bilateral_pairs import _noise, _steps, _tiles, min_tiles  # noqa: F401  (min_tiles is a fixture)

pytestmark = pytest.mark.gpu

# (h, w): all select the batched form on a 256-CU device (checked in the test against the device's own count)
SHAPES = [
    (2, 65536),       # one row pair: REFLECT_101 rows above and below meet the far rows
    (63, 65539),      # tile height - 1 (the last row pair's lower row is outside the frame), width 3 mod 4
    (65, 32646),      # tile height + 1: a second tile row one pixel high, width 2 mod 4
    (129, 21764),     # 2 x tile height + 1
    (24576, 5),       # narrower than the 9 x 9 disc: REFLECT_101 on both sides at once, tiles one above the other
    (12288, 129),     # one pixel wider than a tile
]


@pytest.mark.parametrize("content", ["noise", "steps"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_batched_bilateral_on_64_row_tiles_equals_oracle(gpu_ctx, oracle, min_tiles, shape, content):
    h, w = shape
    assert _tiles(h, w) >= min_tiles, "the frame must select the batched form"
    f = _noise(h, w, h + w) if content == "noise" else _steps(h, w, h + w)
    out = np.empty_like(f)
    gpu_ctx.check(gpu_ctx.lib.cbv_reduce_noise(gpu_ctx.h, f.ctypes.data, w, h, f.strides[0], 9, 75.0, 75.0, out.ctypes.data, out.strides[0]))
    want = oracle.bilateral(f, 9, 75, 75)
    assert np.array_equal(out, want), (shape, content, int((out != want).sum()))


def test_strided_input_and_other_sigmas(gpu_ctx, oracle, min_tiles):
    """A view into a wider buffer (odd byte offset and stride) and narrow sigmas, where most weights are exactly 0."""
    h, w = 66, 32645
    assert _tiles(h, w) >= min_tiles
    big = _noise(h, w + 4, 11)
    big[h // 3:2 * h // 3, w // 4:w // 2] //= 3
    f = big[:, 1:1 + w]
    assert (f.ctypes.data - big.ctypes.data) % 2 == 1 and f.strides[0] % 2 == 1
    for sc, ss in ((75.0, 75.0), (10.0, 3.0)):
        out = np.empty((h, w, 3), np.uint8)
        gpu_ctx.check(gpu_ctx.lib.cbv_reduce_noise(gpu_ctx.h, f.ctypes.data, w, h, f.strides[0], 9, sc, ss, out.ctypes.data, out.strides[0]))
        want = oracle.bilateral(np.ascontiguousarray(f), 9, sc, ss)
        assert np.array_equal(out, want), (sc, ss, int((out != want).sum()))
