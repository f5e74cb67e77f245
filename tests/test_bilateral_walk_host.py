"""The batched d = 9 bilateral takes the weight of tap (0, 0) as the constant 1.0f instead of looking it up: the pixel
against itself has colour distance 0, so the entry is space weight 1 x colour weight 1.  launch_bilateral refuses a
table whose entry is anything else (bilateral_centre_mismatch in k_bilateral.hip); this is the same check on the
host-built table, for wide, narrow and lopsided sigmas.  No device is needed.

The tile queue per XCD of DESIGN.md section 4 (round 6, "not built") would put its range rule's test here; there is no
such rule yet, and nothing in this file tests one."""
import pytest

from chessboard_vision_amd import _native as N


@pytest.mark.parametrize("radius", [1, 2, 3, 4])
@pytest.mark.parametrize("sigmas", [(75.0, 75.0), (10.0, 10.0), (150.0, 3.0)])
def test_centre_entry_of_the_folded_table_is_exactly_one(radius, sigmas):
    assert N.load().cbv_debug_bilateral_centre_is_one(2 * radius + 1, *sigmas) == 1


def test_unsupported_radius_is_reported():
    assert N.load().cbv_debug_bilateral_centre_is_one(11, 75.0, 75.0) == -1
