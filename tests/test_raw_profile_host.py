"""The raw-frame profile mode (CBV_SKIP_ENHANCE_PROFILE_RAW, BoardPipeline.configure(enhance="profile", raw=True)) as far as
it shows without a GPU: the constant and its mirror, the Python keyword, the size of cbv_pipeline_config, and the yardstick
of the GPU tests itself (tests/raw_profile_ref.py), which is shown not to be trivial."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import color_sweep_ref as CS
import raw_profile_ref as RP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_constant_is_3_and_mirrored():
    from chessboard_vision_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "cbv.h")).read()
    assert re.search(r"^#define CBV_SKIP_ENHANCE_PROFILE_RAW 3\b", hdr, re.M)
    assert re.search(r"^#define CBV_SKIP_ENHANCE_PROFILE 2\b", hdr, re.M)
    assert N.SKIP_ENHANCE_PROFILE_RAW == 3 and N.SKIP_ENHANCE_PROFILE == 2


def test_the_new_entry_points_are_bound():
    from chessboard_vision_amd import _native as N
    lib = N.load()
    assert lib.cbv_pipeline_set_profile.argtypes and lib.cbv_warp_color_profile_raw.argtypes
    # null handles are refused before anything is touched
    assert lib.cbv_pipeline_set_profile(None, N.ColorProfile.from_dict(CS.SHIPPED)) == -1
    assert lib.cbv_warp_color_profile_raw(None, None, 4, 4, None, None, 4, 4, 0, None, 12) == -1


def test_configure_maps_raw_to_skip_enhance_3():
    """BoardPipeline.configure: enhance="profile" with raw=True -> 3, without -> 2; raw=True with any other `enhance` is a
    ValueError (checked on the value the method writes, without a device)"""
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd import synth as S
    from chessboard_vision_amd.stream import BoardPipeline

    class Lib:
        cfg = None

        def cbv_pipeline_configure(self, h, cfg):
            self.cfg = cfg
            return 0

        def cbv_pipeline_set_change_blur(self, h, k):
            return 0

    class Ctx:
        lib = Lib()

        def check(self, rc):
            assert rc == 0

    p = BoardPipeline.__new__(BoardPipeline)
    p.ctx, p.h_ = Ctx(), None
    pts = S.scaled_corners(640, 480)
    for kw, want in ((dict(enhance="profile", raw=True), 3), (dict(enhance="profile", raw=False), 2), (dict(enhance="profile"), 2),
                     (dict(enhance=True), 0), (dict(enhance=False), 1)):
        p.configure(pts, profile=CS.SHIPPED, **kw)
        assert p.ctx.lib.cfg.skip_enhance == want, kw
        assert p.ctx.lib.cfg.enhance.profile.enabled == 1 and p.ctx.lib.cfg.enhance.profile.val_scale == 2.46
    assert N.SKIP_ENHANCE_PROFILE_RAW == 3
    p.ctx.lib.cfg = None
    for enhance in (True, False, "profiles"):
        with pytest.raises(ValueError):
            p.configure(pts, profile=CS.SHIPPED, enhance=enhance, raw=True)
        assert p.ctx.lib.cfg is None  # nothing reached the library


def test_the_config_struct_keeps_its_size(tmp_path):
    """cbv_pipeline_config is what it was: 1360 bytes, skip_enhance its last field, against gcc"""
    from chessboard_vision_amd import _native as N
    assert C.sizeof(N.PipelineConfig) == 1360 and N.PipelineConfig.skip_enhance.offset == 1356
    assert N.PipelineConfig._fields_[-1][0] == "skip_enhance"
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    src = tmp_path / "f.c"
    src.write_text("\n".join(['#include <stddef.h>', '#include <stdio.h>', '#include "cbv.h"', 'int main(void) {',
                              'printf("%zu %zu %d\\n", sizeof(cbv_pipeline_config), offsetof(cbv_pipeline_config, skip_enhance), CBV_SKIP_ENHANCE_PROFILE_RAW);',
                              'return 0;', '}']))
    exe = tmp_path / "f"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["1360", "1356", "3"]


@pytest.mark.parametrize("fmt", ["nv12", "yuyv", "bayer_grbg"])
def test_the_yardstick_is_not_trivial(oracle, fmt):
    """warp(apply_color_profile(to_bgr(raw))) with the shipped profile on a quad partly outside a 38 x 30 frame: (a) is not the
    plain raw warp, (b) is not the profile applied after the warp, (c) is 0 beyond one pixel outside the frame, although the
    shipped profile sends black to something else, so a kernel that converted its border taps would fail (c)"""
    w, h, dest = 38, 30, (33, 21)
    raw = RP.noise(w, h, fmt, 5)
    bgr = RP.to_bgr(raw, fmt)
    assert bgr.shape == (h, w, 3) and bgr.dtype == np.uint8
    M = oracle.get_perspective_transform(np.float32(RP.quads(w, h)["partly_outside"]), np.float32([[0, 0], [dest[0], 0], [0, dest[1]], [dest[0], dest[1]]]))
    want = RP.yardstick(oracle, bgr, CS.SHIPPED, M, dest)
    plain = RP.yardstick(oracle, bgr, None, M, dest)
    assert not np.array_equal(want, plain)  # (a)
    after = oracle.apply_color_profile(plain, CS.SHIPPED)
    assert not np.array_equal(want, after)  # (b)
    # (c): the taps of a pixel whose source position lies more than a pixel (and the 1/32 px of the coordinates' grid) outside
    # the frame are all outside it
    sx, sy = RP.source_coords(M, dest)
    far = (sx < -1.1) | (sx > w + .1) | (sy < -1.1) | (sy > h + .1)
    assert far.sum() >= 8 and not far.all()
    assert not want[far].any()
    black = oracle.apply_color_profile(np.zeros((2, 2, 3), np.uint8), CS.SHIPPED)
    assert black.any()          # |0 * 1.48 - 30| = 30 and what the HSV stage makes of it: not black
    assert after[far].any()     # which is what a conversion of the border's zeros shows there
