"""k_bilateral.hip carries the table offset of every tap of the batched d = 9 form as a compile-time constant
(bl_class_off: a class is a distinct dx^2 + dy^2, numbered by first occurrence in raster tap order, offset = class x 768)
in place of the tap_off table cbv_tables.cpp builds.  launch_bilateral compares the two before it selects that form;
this is the same comparison, on the host, for every supported radius.  No device is needed."""
import pytest

from chessboard_vision_amd import _native as N


@pytest.mark.parametrize("radius", [1, 2, 3, 4])
@pytest.mark.parametrize("sigmas", [(75.0, 75.0), (10.0, 3.0)])
def test_compile_time_offsets_equal_the_table(radius, sigmas):
    assert N.load().cbv_debug_bilateral_offsets(2 * radius + 1, *sigmas) == 0


def test_unsupported_radius_is_reported():
    assert N.load().cbv_debug_bilateral_offsets(11, 75.0, 75.0) == -1
