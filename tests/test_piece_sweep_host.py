"""The PieceDetector settings sweep without a GPU: the yardstick (tests/piece_sweep_ref.py) reaches the cases it is meant to,
reproduces what the reference's own class recorded (tests/golden/ref_piece_settings.json), cbv_piece_sweep_eval_host (the
host twin of k_piece_sweep_eval) on the oracle's statistics and circle choices equals it record for record, hand-made
statistics take the twin through the branches the scene does not reach, and the host-side helpers of stream.py (trackbar
grid, settings file, statistics report).  Tolerance 0 everywhere."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import piece_sweep_ref as PS
import refrun

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pop(v):
    return bin(int(v)).count("1")


# 1 ------------------------------------------------------------------------------------------------------------------
def test_the_yardstick_reaches_every_case():
    """12 frames, one ply every 4: per (setting, frame) the smoothed occupancy against the scripted position.  The figures
    of this stream: settings 0, 1, 2, 5, 8, 13, 16, 17 are exact on 8 of 12 frames (the two frames behind each ply lag by one
    piece: 1 missed, 1 false); settings 3, 4, 6, 7, 10, 14 miss 24 on every frame; setting 12 (param2 = 1) has 20 false
    pieces on frames 0..9.  This test validates the yardstick, not the product: it calls nothing under test and passes with
    or without the feature; every other test of this file calls the new entry points."""
    exp = PS.expected_bits()
    Y = PS.yardstick_records()
    missed = np.array([[_pop(exp[i] & ~r["stable_occupied"]) for i, r in enumerate(row)] for row in Y])
    false = np.array([[_pop(r["stable_occupied"] & ~exp[i]) for i, r in enumerate(row)] for row in Y])
    exact = (missed == 0) & (false == 0)
    assert [j for j in range(len(Y)) if exact[j].sum() == 8] == [0, 1, 2, 5, 8, 13, 16, 17] and exact.sum(axis=1).max() == 8
    assert [j for j in range(len(Y)) if (missed[j] == 24).all()] == [3, 4, 6, 7, 10, 14] and missed.max() == 24
    assert list(false[12]) == [20] * 10 + [19, 19] and false.max() == 20 and not missed[12].any()
    assert sorted(set(missed.ravel()) | set(false.ravel())) != [0]
    for m in ("hough", "tower_top", "center_diff"):
        assert any(r[m] for row in Y for r in row), m
    assert not any(r["symmetry"] for row in Y for r in row)  # not in this scene: test 3 drives it by hand
    lag = [(j, i) for j, row in enumerate(Y) for i, r in enumerate(row) if r["raw_occupied"] != r["stable_occupied"]]
    assert (0, 4) in lag and (0, 8) in lag  # the frame of a ply: the history still holds the old position
    assert {_pop(r["raw_occupied"]) for row in Y for r in row} >= {8, 32, 52}


# 2 ------------------------------------------------------------------------------------------------------------------
def test_host_twin_equals_the_yardstick(oracle):
    exp = PS.expected_bits()
    Y = PS.yardstick_records()
    stats, ws, hs, ch = PS.oracle_inputs()
    assert (ch["kind"] == 1).any() and (ch["kind"] == 2).any() and (ch["kind"] == 0).any()
    rec, summ = PS.eval_host(stats, ws, hs, ch, exp)
    PS.assert_records_equal(rec, Y, "host twin")
    want = PS.reduce_records(rec, exp, [[r["_radii"] for r in row] for row in Y])
    for name in PS.SUM_FIELDS:
        assert np.array_equal(summ[name], want[name]), name
    assert summ.tobytes() == want.tobytes()
    # without `expected` the three comparisons stay 0 and nothing else changes
    rec2, summ2 = PS.eval_host(stats, ws, hs, ch, None)
    assert PS.same_records(rec2, rec)
    assert not summ2["frames_exact"].any() and not summ2["missed"].any() and not summ2["false_pos"].any()
    assert np.array_equal(summ2["r_sum"], summ["r_sum"]) and np.array_equal(summ2["n_hough"], summ["n_hough"])
    # a walk in two halves restarts the history: frames 0..5 alone equal the first half
    rec3, _ = PS.eval_host(stats[:6], ws, hs, ch[:, :6], exp[:6])
    assert PS.same_records(rec3, rec[:, :6])


# 3 ------------------------------------------------------------------------------------------------------------------
def _stats(n=6400, mean=100, spread=20, center=100, border=100, rings=(100, 100, 100, 100)):
    """hand-made cbv_sq_stats of an 80 x 80 square: half the pixels at mean - spread, half at mean + spread"""
    from chessboard_vision_amd import _native as N
    st = np.zeros(1, N.record_dtype(N.SqStats))
    st["n"] = n
    st["sum"] = n * mean
    st["sumsq"] = n * (mean * mean + spread * spread)
    st["center_cnt"], st["border_cnt"] = 1000, 400
    st["center_sum"], st["border_sum"] = 1000 * center, 400 * border
    st["ring_cnt"][0] = [300, 300, 300, 300]
    st["ring_sum"][0] = [300 * r for r in rings]
    return st


def test_host_twin_on_hand_made_statistics():
    from chessboard_vision_amd import _native as N
    ws = hs = np.full(1, 80, np.int32)
    none = np.zeros((1, 1, 1), N.record_dtype(N.PieceChoice))
    circle = none.copy()
    circle[0, 0, 0] = (1, 0, 27, 41, 39)

    def one(st, ch):
        rec, summ = PS.eval_host(st[None], ws, hs, ch, None)
        return rec[0, 0], summ[0]

    # np.var of ring means (100, 100, 160, 160) = 900 -> 900 / 500 caps at 1 > 0.6: symmetry
    r, s = one(_stats(rings=(100, 100, 160, 160)), none)
    assert (r["raw_occupied"], r["symmetry"], r["center_diff"], r["hough"], r["n_raw"]) == (1, 1, 0, 0, 1) and s["n_symmetry"] == 1
    # (100, 100, 130, 130): var 225 -> 0.45, not above 0.6: nothing
    r, _ = one(_stats(rings=(100, 100, 130, 130)), none)
    assert (r["raw_occupied"], r["symmetry"]) == (0, 0)
    # (100, 100, 134.65.., ...) exactly at the threshold: var / 500 == 0.6 is not above it (rings 100, 100, 100 + d, 100 + d: var = d^2 / 4)
    r, _ = one(_stats(rings=(100, 100, 134, 135)), none)
    assert r["symmetry"] == 0 and 0.5 < np.var([100, 100, 134, 135]) / 500 <= 0.6
    # the centre-versus-corner difference comes before the symmetry, the circle before both
    r, _ = one(_stats(center=150, border=100, rings=(100, 100, 160, 160)), none)
    assert (r["center_diff"], r["symmetry"]) == (1, 0)
    r, _ = one(_stats(center=140, border=100), none)  # 40 is not above 40
    assert r["raw_occupied"] == 0
    r, s = one(_stats(center=150, border=100, rings=(100, 100, 160, 160)), circle)
    assert (r["hough"], r["center_diff"], r["symmetry"], r["r_min"], r["r_max"]) == (1, 0, 0, 27, 27) and (s["n_r"], s["r_sum"]) == (1, 27)
    # std < 15 gates everything, the circle included; std == 15 does not
    r, s = one(_stats(spread=14, center=150, border=100, rings=(100, 100, 160, 160)), circle)
    assert (r["raw_occupied"], r["hough"], r["center_diff"], r["symmetry"], r["r_max"]) == (0, 0, 0, 0, 0) and s["n_r"] == 0
    r, _ = one(_stats(spread=15, center=150, border=100), none)
    assert r["center_diff"] == 1
    # an overflow in the choice travels into the record and the summary
    over = none.copy()
    over[0, 0, 0] = (0, N.HOUGH_OVERFLOW, 0, 0, 0)
    r, s = one(_stats(), over)
    assert r["flags"] == N.PIECE_SWEEP_OVERFLOW and s["overflow"] == 1
    # the history: raw 1 1 0 0 0 1 -> stable 1 1 1 0 0 0 (2/3, 2/4 < 0.6, 2/5, 2/5)
    seq = [1, 1, 0, 0, 0, 1]
    st = np.concatenate([_stats(center=150 if v else 100) for v in seq])[:, None]
    rec, _ = PS.eval_host(st, ws, hs, np.zeros((1, len(seq), 1), none.dtype), None)
    assert list(rec["raw_occupied"][0]) == seq and list(rec["stable_occupied"][0]) == [1, 1, 1, 0, 0, 0]
    # bad arguments
    lib = N.load()
    st1 = _stats()
    args = [N.ptr(st1), N.ptr(ws), N.ptr(hs), 1, 1, N.ptr(none), 1, None, None, N.ptr(np.zeros(1, N.record_dtype(N.PieceSweepSummary)))]
    assert lib.cbv_piece_sweep_eval_host(*args) == 0
    for k, bad in ((0, None), (3, 0), (3, 65), (4, 0), (5, None), (6, 0), (9, None)):
        a = list(args)
        a[k] = bad
        assert lib.cbv_piece_sweep_eval_host(*a) == -1, k


def test_decide_piece_is_the_shared_decision():
    """cbv_decide_piece (the existing entry point) and the sweep's twin give the same answer on the oracle's statistics."""
    from chessboard_vision_amd import _native as N
    lib = N.load()
    stats, ws, hs, ch = PS.oracle_inputs()
    rec, _ = PS.eval_host(stats[:1], ws, hs, ch[:1, :1], None)
    raw = 0
    for roi in range(64):
        st = N.SqStats.from_buffer_copy(stats[0, roi].tobytes())
        c = ch[0, 0, roi]
        hg = N.HoughResult()
        hg.found, hg.kind, hg.cx, hg.cy, hg.r = int(c["kind"] != 0), int(c["kind"]), float(c["cx"]) + 0.5, float(c["cy"]) + 0.25, float(c["r"]) + 0.75
        out = N.PieceResult()
        assert lib.cbv_decide_piece(st, hg, int(ws[roi]), int(hs[roi]), 0.6, out) == 0
        raw |= int(out.has_piece) << roi
        if c["kind"]:
            assert (out.cx, out.cy, out.radius) == (c["cx"], c["cy"], c["r"])  # int(): toward zero
    assert raw == int(rec["raw_occupied"][0, 0]) and _pop(raw) == 32


# 4 ------------------------------------------------------------------------------------------------------------------
def test_ctypes_mirrors_of_the_new_structs(tmp_path):
    """sizes and every field's offset against what gcc lays out for include/cbv.h, compiled as C99"""
    import shutil
    import subprocess
    from chessboard_vision_amd import _native as N
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    pairs = [("cbv_piece_sweep_record", N.PieceSweepRecord), ("cbv_piece_sweep_summary", N.PieceSweepSummary),
             ("cbv_piece_sweep_info", N.PieceSweepInfo), ("cbv_hough_params", N.HoughParams)]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "cbv.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('printf("limits %d %d\\n", CBV_PIECE_SWEEP_MAX_SETTINGS, CBV_PIECE_SWEEP_OVERFLOW);')
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
    assert C.sizeof(N.PieceSweepRecord) == 56 and C.sizeof(N.PieceSweepSummary) == 56 and C.sizeof(N.PieceChoice) == 8
    assert got["limits"].split() == [str(N.PIECE_SWEEP_MAX_SETTINGS), str(N.PIECE_SWEEP_OVERFLOW)]
    hdr = open(os.path.join(ROOT, "include", "cbv.h")).read()
    for sym in ("cbv_pipeline_piece_sweep", "cbv_pipeline_piece_detail", "cbv_piece_sweep_eval_host"):
        assert re.search(r"^CBV_API\s+int\s+%s\s*\(" % sym, hdr, flags=re.M) and hasattr(N.load(), sym)


# 5 ------------------------------------------------------------------------------------------------------------------
def test_yardstick_reproduces_the_reference_class_run():
    """tests/golden/ref_piece_settings.json: the reference's own PieceDetector under 4 of the settings, first 6 frames"""
    fx = refrun.load_json("ref_piece_settings.json")
    assert fx["size"] == [PS.W, PS.H] and fx["frames_per_ply"] == PS.FRAMES_PER_PLY
    assert {k: tuple(v) if isinstance(v, list) else v for k, v in fx["palette"].items()} == PS.PALETTE
    assert [run["setting_index"] for run in fx["runs"]] == list(PS.FIXTURE_SETTINGS)
    methods = set()
    for run in fx["runs"]:
        s = PS.SETTINGS[run["setting_index"]]
        assert run["setting"] == list(s) and len(run["frames"]) == PS.FIXTURE_FRAMES
        mine = PS.run_setting(s)
        for i, rows in enumerate(run["frames"]):
            assert json.loads(json.dumps(refrun.result_rows(mine[i][0]))) == rows, (s, i)
            methods.update(row[3] for row in rows)
    assert methods >= {None, "hough", "center_diff"}


# helpers of stream.py ---------------------------------------------------------------------------------------------------
def test_piece_trackbar_grid():
    from chessboard_vision_amd.stream import piece_trackbar_grid
    lo, hi = piece_trackbar_grid()
    assert (len(lo), len(hi)) == (50, 70)
    assert lo[0] == 0.01 and lo[-1] == 0.5 and hi[-1] == 0.7 and lo[19] == 20 / 100 and hi[54] == 55 / 100
    assert lo == [v / 100 for v in range(1, 51)] and hi == [v / 100 for v in range(1, 71)]


def test_piece_settings_file(tmp_path):
    from chessboard_vision_amd.stream import save_piece_settings
    path = tmp_path / "piece_detector_settings.json"
    data = save_piece_settings(str(path), 0.25, 0.55, hough_param1=100, hough_param2=30)
    assert json.loads(path.read_text()) == data
    assert (data["min_radius"], data["max_radius"], data["hough_param1"], data["hough_param2"]) == (25, 55, 100, 30)
    assert isinstance(data["min_radius"], int) and path.read_text().startswith("{\n  ")
    assert set(data) == {"min_radius", "max_radius", "hough_param1", "hough_param2", "small_min", "small_max", "knight_aspect_max", "center_diff_thresh"}
    # what PieceDetector.load_settings does with it (piece_detector.py:59-62): percent / 100.0
    assert (data["min_radius"] / 100.0, data["max_radius"] / 100.0) == (0.25, 0.55)
    assert save_piece_settings(str(path), 0.29, 0.57)["min_radius"] == 29  # 0.29 * 100 = 28.999...: rounded, not truncated
    path.write_text(json.dumps({"min_radius": 20, "camera": "left", "nested": {"a": [1]}}))
    data = save_piece_settings(str(path), 0.12, 0.3, small_min=9)
    assert data["camera"] == "left" and data["nested"] == {"a": [1]} and (data["min_radius"], data["max_radius"], data["small_min"]) == (12, 30, 9)


def test_piece_stats_text():
    from chessboard_vision_amd.stream import piece_stats_text
    results = {(0, 0): {"has_piece": True, "radius": 27, "method": "hough", "confidence": 0.9},
               (1, 0): {"has_piece": False, "radius": None, "method": None, "confidence": 0.0},
               (4, 6): {"has_piece": True, "radius": 25, "method": "center_diff", "confidence": 0.5125}}
    want = ("=== ESTATISTICAS DE PECAS (3 casas analisadas) ===\n"
            "Square Size: 77px\n"
            "CASA   STATUS     METODO          RAIO     AREA%    BG%      CONF\n" + "-" * 80 + "\n"
            "a8     PECA       hough           27       38.6     61.4     90.00%\n"
            "e2     PECA       center_diff     25       33.1     66.9     51.25%\n" + "-" * 80 + "\n"
            "Total de pecas detectadas: 2\n")
    assert piece_stats_text(results, 77) == want
