"""The colour profile sweep and the profile-only pipeline mode without a GPU: the yardstick (tests/color_sweep_ref.py) meets
the conditions it is meant to, reproduces what the reference's own classes recorded (tests/golden/ref_color_profiles.json),
and the host-side pieces: the profile file, the trackbar axes, the ctypes mirrors and the new value of skip_enhance.
Tolerance 0 everywhere."""
import ctypes as C
import hashlib
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import color_sweep_ref as CS
import refrun

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# 1 ------------------------------------------------------------------------------------------------------------------
def test_the_yardstick_meets_its_conditions():
    """Conditions on the yardstick alone (it calls nothing under test).  The figures of these streams, (missed, false_pos,
    frames_exact) over 8 frames: palette "low": none (2, 2, 6), neutral (3, 2, 5), shipped (128, 0, 0), radical (87, 2, 0),
    clipping (164, 2, 0), val06 (192, 0, 0), sat3 (2, 2, 6); palette "lilac": none (128, 0, 0), sat3 and radical_lilac (66, 2, 0)."""
    exp = CS.expected_bits()
    Y = {pal: CS.yardstick_records(pal) for pal in CS.PALETTES}
    summ = {pal: [CS.summary_of(rows, exp) for rows in Y[pal]] for pal in CS.PALETTES}
    at = CS.NAMES.index
    assert len(CS.NAMES) >= 10 and len(set(summ["low"])) >= 4, summ["low"]
    assert min(s[0] for s in summ["lilac"]) < summ["lilac"][at("none")][0], summ["lilac"]
    assert summ["lilac"][at("sat3")][0] < summ["lilac"][at("none")][0]
    strip = lambda rows: [{k: v for k, v in r.items() if k != "_radii"} for r in rows]  # noqa: E731
    assert strip(Y["low"][at("neutral")]) != strip(Y["low"][at("none")])  # the 8-bit HSV round trip is not the identity
    behind_a_ply = [i for i in range(CS.N_FRAMES) if i >= CS.FRAMES_PER_PLY]
    assert any(Y["low"][j][i]["raw_occupied"] != Y["low"][j][i]["stable_occupied"] for j in range(len(CS.NAMES)) for i in behind_a_ply)
    assert summ["low"][at("none")] == (2, 2, 6) and summ["low"][at("val06")] == (192, 0, 0) and summ["low"][at("shipped")][0] == 128


def test_yardstick_reproduces_the_reference_classes_run():
    """tests/golden/ref_color_profiles.json: ImageEnhancer.apply_color_profile -> warp_image -> split_board -> PieceDetector
    of the reference itself under 4 of the profiles, first 6 frames; and the calibration tool's own adjustment function
    returned the enhancer's bytes on those frames"""
    fx = refrun.load_json("ref_color_profiles.json")
    assert fx["size"] == [CS.W, CS.H] and fx["frames_per_ply"] == CS.FRAMES_PER_PLY and fx["hough"] == list(CS.HOUGH)
    assert {k: tuple(v) if isinstance(v, list) else v for k, v in fx["palette"].items()} == CS.PALETTES["low"]
    assert [run["profile_name"] for run in fx["runs"]] == list(CS.FIXTURE_PROFILES)
    assert fx["tool_equals_enhancer"] is True
    for run in fx["runs"]:
        name = run["profile_name"]
        assert run["profile"] == CS.PROFILES[name] and len(run["frames"]) == CS.FIXTURE_FRAMES
        mine = CS.run_profile("low", name)
        for i, rows in enumerate(run["frames"]):
            assert hashlib.sha256(np.ascontiguousarray(CS.warped("low", name, i)).tobytes()).hexdigest() == run["warped_sha256"][i], (name, i)
            assert json.loads(json.dumps(refrun.result_rows(mine[i][0]))) == rows, (name, i)


# 2 ------------------------------------------------------------------------------------------------------------------
def test_color_profile_file_round_trip(tmp_path, monkeypatch):
    from chessboard_vision_amd import stream
    path = tmp_path / "color_profile.json"
    data = stream.save_color_profile(str(path), CS.SHIPPED)
    assert data == CS.SHIPPED and list(data) == list(stream.COLOR_PROFILE_KEYS)
    assert stream.load_color_profile(str(path)) == CS.SHIPPED
    # the tool's eight keys in its order (calibrate_colors.py:194-203), json with indent = 4 (:57)
    assert list(json.loads(path.read_text())) == ["hue_shift", "sat_scale", "val_scale", "contrast", "brightness", "radical_mode", "target_hue",
                                                  "hue_window"]
    assert path.read_text() == json.dumps(CS.SHIPPED, indent=4) and path.read_text().startswith('{\n    "hue_shift": -86,')
    # missing keys take ImageEnhancer's defaults; keys that are not the tool's are left out
    part = stream.save_color_profile(str(path), {"sat_scale": 3.0, "camera": "left"})
    assert part == {"hue_shift": 0, "sat_scale": 3.0, "val_scale": 1.0, "contrast": 1.0, "brightness": 0, "radical_mode": 0, "target_hue": 0,
                    "hue_window": 20}
    assert stream.save_color_profile(str(path), None) == dict(part, sat_scale=1.0)
    # ... and the product's ImageEnhancer reads the file from the working directory as the reference's does
    stream.save_color_profile(str(path), CS.PROFILES["radical"])
    monkeypatch.chdir(tmp_path)
    from chessboard_vision_amd.frame_enhancer import ImageEnhancerHIP
    enh = ImageEnhancerHIP.__new__(ImageEnhancerHIP)
    assert ImageEnhancerHIP.load_profile(enh) == CS.PROFILES["radical"]


def test_color_trackbar_axes_and_axis_profiles():
    from chessboard_vision_amd import stream
    ax = stream.color_trackbar_axes()
    assert list(ax) == list(stream.COLOR_PROFILE_KEYS)
    assert ax["hue_shift"] == list(range(-180, 181))                      # "Hue Shift" 0..360, pos - 180
    for k in ("sat_scale", "val_scale", "contrast"):                      # 0..300, pos / 100.0
        assert ax[k] == [pos / 100.0 for pos in range(301)] and ax[k][0] == 0.0 and ax[k][-1] == 3.0 and ax[k][91] == 0.91
    assert ax["brightness"] == list(range(-100, 101))                     # "Brightness" 0..200, pos - 100
    assert ax["radical_mode"] == [0, 1] and ax["target_hue"] == list(range(180)) and ax["hue_window"] == list(range(51))
    assert [len(ax[k]) for k in ax] == [361, 301, 301, 301, 201, 2, 180, 51]
    profs = stream.color_axis_profiles({"val_scale": 2.0}, "sat_scale")
    assert len(profs) == 301 and all(set(p) == set(stream.COLOR_PROFILE_KEYS) and p["val_scale"] == 2.0 for p in profs)
    assert [p["sat_scale"] for p in profs] == ax["sat_scale"] and profs[100] == stream.color_full_profile({"val_scale": 2.0})
    assert [p["brightness"] for p in stream.color_axis_profiles(None, "brightness", [-5, 5])] == [-5, 5]
    with pytest.raises(ValueError):
        stream.color_axis_profiles({}, "gamma")


# 3 ------------------------------------------------------------------------------------------------------------------
def test_ctypes_mirrors_and_the_profile_only_value(tmp_path):
    """sizes and every field's offset against what gcc lays out for include/cbv.h, compiled as C99; skip_enhance = 2 is a
    value of its own and cbv_pipeline_config did not grow"""
    from chessboard_vision_amd import _native as N
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    pairs = [("cbv_color_sweep_info", N.ColorSweepInfo), ("cbv_color_profile", N.ColorProfile), ("cbv_pipeline_config", N.PipelineConfig)]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "cbv.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('printf("limits %d %d\\n", CBV_COLOR_SWEEP_MAX_PROFILES, CBV_SKIP_ENHANCE_PROFILE);')
    lines += ["return 0;", "}"]
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(l.split(None, 1) for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, cls in pairs:
        assert int(got[cname]) == C.sizeof(cls), (cname, got[cname], C.sizeof(cls))
        for fname, _ in cls._fields_:
            assert int(got["%s.%s" % (cname, fname)]) == getattr(cls, fname).offset, (cname, fname)
    assert C.sizeof(N.ColorSweepInfo) == 24
    assert got["limits"].split() == [str(N.COLOR_SWEEP_MAX_PROFILES), str(N.SKIP_ENHANCE_PROFILE)] == ["65536", "2"]
    assert N.SKIP_ENHANCE_PROFILE not in (0, 1) and N.PipelineConfig._fields_[-1][0] == "skip_enhance"
    # the struct is what it was before the mode existed: skip_enhance is its last field, 4 bytes, and nothing follows it
    assert N.PipelineConfig.skip_enhance.offset + 4 + 7 >= C.sizeof(N.PipelineConfig) and N.PipelineConfig.skip_enhance.size == 4
    hdr = open(os.path.join(ROOT, "include", "cbv.h")).read()
    for sym in ("cbv_pipeline_color_sweep", "cbv_warp_color_profile"):
        assert re.search(r"^CBV_API\s+int\s+%s\s*\(" % sym, hdr, flags=re.M) and hasattr(N.load(), sym)


def test_configure_maps_enhance_to_skip_enhance():
    """BoardPipeline.configure's `enhance`: True -> 0, False -> 1, "profile" -> 2, any other string is an error (checked on
    the value the method writes, without a device)"""
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.stream import BoardPipeline

    class Lib:
        def cbv_pipeline_configure(self, h, cfg):
            self.cfg = cfg
            return 0

        def cbv_pipeline_set_change_blur(self, h, k):
            return 0

    class Ctx:
        lib = Lib()

        def check(self, rc):
            assert rc == 0

    from chessboard_vision_amd import synth as S
    p = BoardPipeline.__new__(BoardPipeline)
    p.ctx, p.h_ = Ctx(), None
    for enhance, want in ((True, 0), (False, 1), ("profile", N.SKIP_ENHANCE_PROFILE)):
        p.configure(S.scaled_corners(640, 480), profile=CS.SHIPPED, enhance=enhance)
        assert p.ctx.lib.cfg.skip_enhance == want and p.ctx.lib.cfg.enhance.profile.enabled == 1
        assert p.ctx.lib.cfg.enhance.profile.val_scale == 2.46
    with pytest.raises(ValueError):
        p.configure(S.scaled_corners(640, 480), enhance="profiles")
