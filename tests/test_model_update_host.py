"""Model-update modes of the pipeline, the part that needs no GPU: the yardstick stream of tests/test_gpu_model_update.py
is worth testing on (the three modes really differ on it, and it reaches every class and the variance clamp), and the
new entry points exist from the library up to the Python classes."""
import itertools

import numpy as np

import model_update_ref as R


def _differing(a, b):
    return sum(1 for x, y in zip(a, b) if x != y)


def _names(d):
    return {"abcdefgh"[f] + str(r + 1) for (f, r) in d}


def test_the_three_modes_differ_on_the_yardstick_stream(oracle):
    """Conditions on the INPUTS of the GPU tests, so that those cannot pass vacuously: on the 28-frame stream the modes'
    result-dict sequences differ pairwise in at least 10 frames with both parameter sets; with (2.55, 600, 0.1) mode
    "every" reports nothing in frames 10-15 and 18-23 where the frozen model still reports e2, e4 (and e5, e7), produces
    LEVE, PARCIAL and empty dicts, and learns a variance below the initial one; with (1.45, 50, 0.37) it reaches TOTAL and
    the np.maximum(new_var, 10.0) clamp."""
    for params in (R.PARAMS_A, R.PARAMS_B):
        seqs = {m: R.run_mode(m, params)[0] for m in R.MODES}
        assert all(len(s) == R.N_FRAMES for s in seqs.values())
        for a, b in itertools.combinations(R.MODES, 2):
            nd = _differing(seqs[a], seqs[b])
            print(params, a, b, "differ in", nd, "frames")
            assert nd >= 10, (params, a, b, nd)

    frozen, every = R.run_mode("frozen", R.PARAMS_A)[0], R.run_mode("every", R.PARAMS_A)[0]
    for i in list(range(10, 16)) + list(range(18, 24)):
        assert every[i] == {}, (i, every[i])
        assert {"e2", "e4"} <= _names(frozen[i]), (i, _names(frozen[i]))
    for i in range(18, 24):
        assert {"e5", "e7"} <= _names(frozen[i]), (i, _names(frozen[i]))
    seen = {v["intensity"] for d in every for v in d.values()}
    assert {"LEVE", "PARCIAL"} <= seen and any(d == {} for d in every), seen
    ref = R.run_mode("every", R.PARAMS_A)[1]
    vmin = min(float(v.min()) for v in ref.variances.values())
    print("smallest variance after 'every', first parameter set:", vmin)
    assert 10.0 <= vmin < R.PARAMS_A[1]

    every_b, ref_b = R.run_mode("every", R.PARAMS_B)
    assert "TOTAL" in {v["intensity"] for d in every_b for v in d.values()}
    assert min(float(v.min()) for v in ref_b.variances.values()) == 10.0
    assert all(v.dtype == np.float32 for v in ref_b.variances.values())


def test_entry_points_exist_from_the_library_to_the_classes():
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.stream import Board, BoardPipeline
    lib = N.load()
    for name in ("cbv_pipeline_set_model_update", "cbv_pipeline_model"):
        assert hasattr(lib, name), "the library does not export %s" % name
        assert getattr(lib, name).argtypes is not None, "no prototype bound for %s" % name
    for cls in (Board, BoardPipeline):
        assert callable(cls.set_model_update) and callable(cls.model)
    assert (N.MODEL_FROZEN, N.MODEL_EVERY, N.MODEL_UNCHANGED) == (0, 1, 2)
    # the new kernel's profiling id follows every existing one
    assert N.K["MODEL_SCAN"] == max(v for k, v in N.K.items() if k != "MODEL_SCAN") + 1
    assert lib.cbv_kernel_name(N.K["MODEL_SCAN"]) == b"k_model_scan"
