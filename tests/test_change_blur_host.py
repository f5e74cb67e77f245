"""ChangeDetector blur kernel of the pipeline, the part that needs no GPU: the yardstick of tests/test_gpu_change_blur.py
separates the kernels it is used with (otherwise those tests would prove nothing), the settings loader reads the file the
reference ships, and the bit-level hand pattern is classify_hand_pattern."""
import itertools
import os

import change_blur_ref as B
from ref_logic import RefChangeDetector

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sensitivity_settings.json")


def test_the_yardstick_separates_the_kernels(oracle):
    """Per configuration the GPU tests use: no two kernels give the same sequence of dicts or the same final mean planes.
    With (1.45, 50, 0.37) "unchanged" even the `changed` key sets differ pairwise, with "every" all but (7, 13), which
    the GPU tests do not pair; with the shipped settings, frozen, the key sets agree and pct_changed / z_score differ."""
    import numpy as np
    for mode, params, ks in B.CASES:
        runs = {k: B.run_blur(mode, params, k) for k in ks + (5,)}  # 5 = what the pipeline did before
        for a, b in itertools.combinations(runs, 2):
            assert runs[a][0] != runs[b][0], (mode, a, b, "dict sequences")
            assert any(not np.array_equal(runs[a][1].means[p], runs[b][1].means[p]) for p in runs[a][1].means), (mode, a, b, "means")
            same_keys = B.keysets(runs[a][0]) == B.keysets(runs[b][0])
            print(mode, params, a, b, "key sets equal:", same_keys)
            if mode == "frozen":
                assert same_keys, (a, b)
            else:
                assert not same_keys, (mode, a, b)
        assert any(d for d in runs[ks[0]][0])


def test_the_switched_stream_is_neither_pure_run(oracle):
    """k = 5 up to frame 13, then 13, model kept, mode "every": frames 0..13 are the k = 5 run's, frames 14..27 differ from
    both the pure k = 5 and the pure k = 13 run."""
    s = B.SWITCH_AT
    sw = B.run_blur("every", B.PARAMS_B, B.SWITCH_FROM, switch=(s, B.SWITCH_TO))[0]
    p5 = B.run_blur("every", B.PARAMS_B, B.SWITCH_FROM)[0]
    p13 = B.run_blur("every", B.PARAMS_B, B.SWITCH_TO)[0]
    assert sw[:s] == p5[:s]
    assert sw[s:] != p5[s:] and sw[s:] != p13[s:]


def test_load_sensitivity_settings_reads_the_shipped_file():
    from chessboard_vision_amd.stream import load_sensitivity_settings
    got = load_sensitivity_settings(GOLDEN)
    assert got == {"z_threshold": 2.55, "initial_variance": 600, "blur_kernel": 13, "alpha": 0.13}
    assert isinstance(got["blur_kernel"], int)


def _bits(dicts_frame, rois_rc):
    roi_of = {(c, 7 - r): i for i, (r, c) in enumerate(rois_rc)}
    changed = sum(1 << roi_of[p] for p in dicts_frame)
    total = sum(1 << roi_of[p] for p, v in dicts_frame.items() if v["intensity"] == "TOTAL")
    return changed, total


def test_hand_pattern_from_bits_is_classify_hand_pattern(oracle):
    from chessboard_vision_amd.stream import classify_hand_bits
    rois_rc = [(r, c) for r in range(8) for c in range(8)]
    ref = RefChangeDetector()
    seen = set()
    for mode, params, ks in B.CASES:
        for k in ks:
            for d in B.run_blur(mode, params, k)[0]:
                want = ref.classify_hand_pattern(d)
                assert classify_hand_bits(*_bits(d, rois_rc), rois_rc) == want, (mode, k, d)
                seen.add((want["is_hand"], want["is_move"]))
    print("patterns on the yardstick runs:", sorted(seen))

    def mk(n, n_total):
        pos = [(f, 0) for f in range(n)]
        return {p: {"intensity": "TOTAL" if i < n_total else "LEVE"} for i, p in enumerate(pos)}
    # 2 TOTAL; 4 squares; 3 squares; exactly 2; 1; 0
    for n, nt, hand, move in ((2, 2, True, False), (4, 0, True, False), (3, 1, True, False), (2, 1, False, True), (2, 0, False, True),
                              (1, 1, False, False), (1, 0, False, False), (0, 0, False, False)):
        d = mk(n, nt)
        got = classify_hand_bits(*_bits(d, rois_rc), rois_rc)
        assert got == ref.classify_hand_pattern(d), (n, nt)
        assert (got["is_hand"], got["is_move"]) == (hand, move), (n, nt, got)
        assert got["move_candidates"] == (set() if hand else set(d)), (n, nt, got)


def test_entry_points_exist_from_the_library_to_the_classes():
    import inspect
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.stream import Board, BoardPipeline
    lib = N.load()
    assert hasattr(lib, "cbv_pipeline_set_change_blur") and lib.cbv_pipeline_set_change_blur.argtypes is not None
    for cls in (Board, BoardPipeline):
        assert callable(cls.set_change_blur) and callable(cls.hand_pattern) and isinstance(cls.change_blur, property)
    assert inspect.signature(BoardPipeline.configure).parameters["blur_kernel"].default == 5
    assert inspect.signature(BoardPipeline.add_board).parameters["blur_kernel"].default == 5
    # the new kernel's profiling id follows every existing one, which keep their numbers
    assert N.K_CHANGE_BLUR == N.K_WARP_YUV + 1 == max(N.K_ALL.values())
    assert lib.cbv_kernel_name(N.K_CHANGE_BLUR) == b"k_change_blur_stats"
    assert lib.cbv_kernel_name(N.K_CHANGE_BLUR + 1) == b""
    # no device: a null board is refused before anything else
    assert lib.cbv_pipeline_set_change_blur(None, 13) == -1
