"""The ChangeDetector sensitivity sweep without a GPU: the yardsticks reach every case, cbv_sweep_eval_host (the host twin of
k_sweep_eval) on the oracle's difference histograms equals the reference class setting by setting and the float32 numpy
evaluation on the whole grid, and the host-side helpers of stream.py (trackbar grid, settings file, change radar).
Tolerance 0 everywhere."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import sweep_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# 1 ------------------------------------------------------------------------------------------------------------------
def test_the_class_settings_reach_every_case():
    """From the yardstick side alone (the reference class's dicts): what the settings of test 2 and of the GPU tests
    reach between them."""
    seen = set()
    for s in SR.CLASS_SETTINGS:
        for d in SR.class_dicts(s):
            kinds = [v["intensity"] for v in d.values()]
            seen.update(kinds)
            seen.add("size %d" % len(d) if len(d) < 4 else "four or more")
            if len(d) == 64:
                seen.add("all 64")
            if kinds.count("TOTAL") >= 2 and len(d) <= 2:
                seen.add("hand by two TOTALs alone")
    assert seen >= {"LEVE", "PARCIAL", "TOTAL", "size 0", "size 1", "size 2", "size 3", "four or more", "all 64",
                    "hand by two TOTALs alone"}, seen


# 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", SR.CLASS_SETTINGS, ids=lambda s: "z%s-iv%s-k%s" % s)
def test_host_twin_equals_the_reference_class(setting):
    hist, n_px = SR.oracle_hists(setting[2])
    rec = SR.eval_host(hist, n_px, [setting])[0]
    dicts = SR.class_dicts(setting)
    assert len(dicts) == SR.N_FRAMES == len(rec)
    for i in range(SR.N_FRAMES):
        SR.assert_record_matches_dict(rec[i], dicts[i], (setting, i))


# 3 ------------------------------------------------------------------------------------------------------------------
def test_host_twin_equals_the_numpy_evaluation_on_the_grid(oracle):
    checked = 0
    for k in SR.GRID_K:
        hist, n_px = SR.oracle_hists(k)
        assert np.array_equal(hist.sum(axis=-1), np.broadcast_to(n_px, hist.shape[:2]))
        sets = [s for s in SR.GRID if s[2] == k]
        rec = SR.eval_host(hist, n_px, sets)
        for j, (z, iv, _) in enumerate(sets):
            want = SR.numpy_eval(hist, n_px, z, iv)
            for name in ("changed", "parcial", "total", "z_max"):
                assert np.array_equal(rec[name][j], want[name]), (z, iv, k, name)
            for f in range(SR.N_FRAMES):
                n, nt, flags, lifted = SR.derived(rec["changed"][j, f], rec["total"][j, f])
                assert (rec["n_changed"][j, f], rec["n_total"][j, f], rec["flags"][j, f], rec["lifted"][j, f]) == (n, nt, flags, lifted)
            checked += 1
    assert checked == len(SR.GRID) == 100
    # ... and that evaluation is O.square_stats with a constant variance plane, on a sample
    import model_update_ref as R
    sq = R.stream_squares()
    for (z, iv, k), f, roi in (((1.45, 50, 1), 9, 12), ((2.55, 600, 13), 27, 52), ((0.5, 10, 31), 20, 33), ((3.0, 800, 5), 14, 28)):
        pos = SR.ROI_POS[roi]
        g = oracle.square_preprocess(sq[f][pos], k)
        mean = oracle.square_preprocess(sq[0][pos], k).astype(np.float32)
        st = oracle.square_stats(g, mean=mean, var=np.full(g.shape, iv, np.float32), z_thresh=z)
        hist, n_px = SR.oracle_hists(k)
        want = SR.numpy_eval(hist, n_px, z, iv)
        assert (st.z_count, np.float32(st.z_max)) == (want["z_count"][f, roi], want["z_sq"][f, roi]), (z, iv, k, f, roi)


def test_host_twin_rejects_bad_arguments():
    from chessboard_vision_amd import _native as N
    lib = N.load()
    hist, n_px = SR.oracle_hists(1)
    h, n = np.ascontiguousarray(hist[3]), np.ascontiguousarray(n_px)
    out = np.zeros(1, N.record_dtype(N.SweepRecord))
    for iv in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        s = np.zeros(1, N.record_dtype(N.SweepSetting))
        s[0] = (2.5, iv, 5)
        assert lib.cbv_sweep_eval_host(N.ptr(h), N.ptr(n), 64, N.ptr(s), 1, N.ptr(out)) == -1, iv
    s[0] = (2.5, 100, 5)
    assert lib.cbv_sweep_eval_host(N.ptr(h), N.ptr(n), 65, N.ptr(s), 1, N.ptr(out)) == -1
    assert lib.cbv_sweep_eval_host(None, N.ptr(n), 64, N.ptr(s), 1, N.ptr(out)) == -1
    assert lib.cbv_sweep_eval_host(N.ptr(h), N.ptr(n), 64, N.ptr(s), 0, N.ptr(out)) == -1
    assert lib.cbv_sweep_eval_host(N.ptr(h), N.ptr(n), 64, N.ptr(s), 1, N.ptr(out)) == 0


# 4 ------------------------------------------------------------------------------------------------------------------
def test_trackbar_grid():
    from chessboard_vision_amd.stream import sensitivity_trackbar_grid
    z, iv, k = sensitivity_trackbar_grid()
    assert (len(z), len(iv), len(k)) == (51, 80, 8)
    assert z[0] == 3.0 and z[-1] == 0.5 and z[9] == 3.0 - 9 / 20.0 and all(0.5 <= v <= 3.0 for v in z)
    assert iv == [10 * t for t in range(1, 81)]
    assert k == [1, 3, 5, 7, 9, 11, 13, 15]
    assert len(set(z)) == 51
    # the shipped file's position is on the grid: Sensibilidade 9, Tolerancia 60, Suavizacao 13
    assert 2.55 in z and 600 in iv and 13 in k


def test_settings_file_round_trip(tmp_path):
    from chessboard_vision_amd.stream import load_sensitivity_settings, save_sensitivity_settings
    path = tmp_path / "sensitivity_settings.json"
    save_sensitivity_settings(str(path), 2.55, 600, 13, 0.13)
    want = {"z_threshold": 2.55, "initial_variance": 600.0, "blur_kernel": 13, "alpha": 0.13}
    assert load_sensitivity_settings(str(path)) == want
    data = json.loads(path.read_text())
    assert set(data) == {"sensitivity", "blur_kernel", "stable_frames", "z_threshold", "alpha", "initial_variance", "use_gaussian"}
    assert data["initial_variance"] == 600 and isinstance(data["initial_variance"], int)  # as the tool writes it
    assert path.read_text().startswith("{\n  ")  # indent 2
    # an existing file with foreign keys keeps them, and its own other keys
    path.write_text(json.dumps({"sensitivity": 8, "camera": "left", "z_threshold": 1.0, "nested": {"a": [1, 2]}}))
    save_sensitivity_settings(str(path), 1.45, 50, 31, 0.37, stable_frames=4)
    data = json.loads(path.read_text())
    assert data["camera"] == "left" and data["nested"] == {"a": [1, 2]} and data["sensitivity"] == 8 and data["stable_frames"] == 4
    assert load_sensitivity_settings(str(path)) == {"z_threshold": 1.45, "initial_variance": 50.0, "blur_kernel": 31, "alpha": 0.37}
    # the shipped fixture survives a load / save / load
    shipped = os.path.join(ROOT, "tests", "golden", "sensitivity_settings.json")
    s = load_sensitivity_settings(shipped)
    path.write_text(open(shipped).read())
    save_sensitivity_settings(str(path), **s)
    assert json.loads(path.read_text()) == json.load(open(shipped)) and load_sensitivity_settings(str(path)) == s


def test_change_radar_on_the_start_position():
    from chessboard_vision_amd.game_state import GameState
    from chessboard_vision_amd.stream import _BoardMethods, classify_hand_bits
    radar = _BoardMethods.change_radar
    rois_rc = [(r, c) for r in range(8) for c in range(8)]

    def pattern(*squares, total=()):
        roi = {pos: i for i, pos in enumerate(SR.ROI_POS)}
        return classify_hand_bits(sum(1 << roi[p] for p in squares), sum(1 << roi[p] for p in total), rois_rc)
    game = GameState()
    e2, e7, d2, g1 = (4, 1), (4, 6), (3, 1), (6, 0)
    assert radar(None, pattern(e2), game) == (e2, [(4, 2), (4, 3)])         # e3, e4
    lifted, dests = radar(None, pattern(g1), game)
    assert lifted == g1 and sorted(dests) == [(5, 2), (7, 2)]                # Nf3, Nh3
    assert radar(None, pattern(e7), game) == (None, [])                     # black's pawn, white to move
    assert radar(None, pattern((4, 3)), game) == (None, [])                 # an empty square
    assert radar(None, pattern(e2, d2), game) == (None, [])                 # two candidates: a move, not a lift
    assert radar(None, pattern(e2, d2, e7), game) == (None, [])             # three squares: a hand
    assert radar(None, pattern(e2, d2, total=(e2, d2)), game) == (None, [])  # two TOTALs: a hand
    assert radar(None, {}, game) == (None, [])                              # the tool's empty pattern
    game.board.push_uci("e2e4")
    assert radar(None, pattern(e7), game) == (e7, [(4, 5), (4, 4)])         # now it is black's


# 5 ------------------------------------------------------------------------------------------------------------------
def test_ctypes_mirrors_of_the_new_structs(tmp_path):
    """tests/test_abi.py checks a fixed list of pairs; the sweep's four structs are checked here the same way: sizes and
    every field's offset against what gcc lays out for include/cbv.h."""
    import shutil
    import subprocess
    from chessboard_vision_amd import _native as N
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    pairs = [("cbv_sweep_setting", N.SweepSetting), ("cbv_sweep_record", N.SweepRecord), ("cbv_sweep_summary", N.SweepSummary),
             ("cbv_sweep_info", N.SweepInfo)]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "cbv.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('printf("limits %d %d %d %d %d\\n", CBV_SWEEP_MAX_SETTINGS, CBV_SWEEP_MAX_CHUNK, CBV_SWEEP_DEFAULT_CHUNK, CBV_SWEEP_HAND, CBV_SWEEP_MOVE);')
    lines += ["return 0;", "}"]
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    got = dict(l.split(None, 1) for l in out)
    for cname, cls in pairs:
        assert int(got[cname]) == C.sizeof(cls), (cname, got[cname], C.sizeof(cls))
        for fname, _ in cls._fields_:
            assert int(got["%s.%s" % (cname, fname)]) == getattr(cls, fname).offset, (cname, fname)
    assert C.sizeof(N.SweepRecord) == 32 and C.sizeof(N.SweepSetting) == 24 and C.sizeof(N.SweepSummary) == 24
    assert got["limits"].split() == [str(v) for v in (N.SWEEP_MAX_SETTINGS, N.SWEEP_MAX_CHUNK, N.SWEEP_DEFAULT_CHUNK, N.SWEEP_HAND, N.SWEEP_MOVE)]
    hdr = open(os.path.join(ROOT, "include", "cbv.h")).read()
    for sym in ("cbv_pipeline_sweep", "cbv_pipeline_change_hist", "cbv_sweep_eval_host"):
        assert re.search(r"^CBV_API\s+int\s+%s\s*\(" % sym, hdr, flags=re.M) and hasattr(N.load(), sym)
