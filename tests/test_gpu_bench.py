"""bench.py end to end on the GPU: a plain run times exactly --steps steps and carries the headline only; --dump-outputs
writes what the last timed step computed, identical from run to run with the same arguments; --full still runs the
legs that take runs of their own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench(args, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs_repeat(tmp_path):
    from chessboard_vision_amd import synth as S
    F = 128
    args = ["--frames", str(F), "--steps", "3", "--warmup", "1"]
    a = _bench(args + ["--dump-outputs", str(tmp_path / "a")])
    assert a["steps"] == 3 and a["warmup"] == 1 and a["ms_per_step"] > 0 and a["full"] is False
    assert a["unit"] == "frames/s" and a["higher_is_better"] is True and a["dtype"] == "u8" and a["metric"].startswith("frames/sec")
    assert abs(a["value"] - F / (a["ms_per_step"] * 1e-3)) <= 0.01 * a["value"]
    assert a["occupancy_check"] is True and a["path_roofline"]["frac"] > 0
    for k in ("roofline", "single_frame_ms", "noise_scene", "class_api", "region_limited", "c4_fps", "cpu_baseline", "c1_cpu_ms"):
        assert a[k] is None, k
    assert a["kernels"] == {}
    da = _load(tmp_path / "a")
    assert sum(v.nbytes for v in da.values()) == a["dumped_bytes"] <= 64 * 10 ** 6
    assert all(v.dtype in (np.float32, np.float64) for v in da.values())
    assert da["frame_results"].shape == (F, 8, 64) and da["warped_boards"].shape == (6, 620, 620, 3)
    assert da["square_stats"].shape[:2] == da["hough"].shape[:2] == (F, 64) and da["noise_results"].shape == (F, 70)
    # raw_occupied (plane 0) of every frame holds as many squares as the scripted position has pieces
    assert [int(n) for n in da["frame_results"][:, 0].sum(axis=1)] == [len(S.position_for_frame(i)) for i in range(F)]
    assert da["warped_boards"].max() > 0
    b = _bench(args + ["--dump-outputs", str(tmp_path / "b")])
    db = _load(tmp_path / "b")
    assert sorted(da) == sorted(db)
    for k in da:
        assert np.array_equal(da[k], db[k]), k
    assert b["occupancy_check"] is True
    # two streams on the GPU: one set of arrays per stream, the sample budget shared between them
    c = _bench(["--frames", str(F), "--steps", "1", "--warmup", "0", "--streams", "2", "--dump-outputs", str(tmp_path / "c")])
    dc = _load(tmp_path / "c")
    assert c["occupancy_check"] is True and c["config"]["frames_per_stream"] == F // 2
    for sid in (0, 1):
        assert dc["stream%d_frame_results" % sid].shape == (F // 2, 8, 64)
        assert dc["stream%d_warped_boards" % sid].shape == (3, 620, 620, 3)
    assert not any(k.startswith("frame_results") for k in dc)


@pytest.mark.gpu
def test_full_run_keeps_every_leg():
    r = _bench(["--full", "--frames", "64", "--steps", "2", "--warmup", "1", "--cpu-frames", "2", "--cpu-frames-1t", "1"], timeout=600)
    assert r["full"] is True and r["occupancy_check"] is True and r["steps"] == 2
    assert r["roofline"]["launches"] > 0 and r["roofline"]["avg_launch_ms"] > 0
    assert "k_bilateral" in r["kernels"] and r["single_frame_ms"] > 0
    for k in ("noise_scene", "class_api", "region_limited", "c4_fps", "cpu_baseline", "cpu_baseline_1t", "c1_cpu_ms"):
        assert r[k] is not None, k
