"""cbv_board_config (include/cbv.h) is plain C99 and its ctypes mirror has gcc's layout; the Python surface of
BoardPipeline.add_board is bound.  No GPU needed."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_board_config_layout_matches_gcc(tmp_path):
    from chessboard_vision_amd import _native as N
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "cbv.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(cbv_board_config));', 'printf("max %d\\n", CBV_MAX_BOARDS);']
    for fname, _ in N.BoardConfig._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(cbv_board_config, %s));' % (fname, fname))
    lines += ["return 0;", "}"]
    src = tmp_path / "board_abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "board_abi"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(N.BoardConfig)
    assert int(got["max"]) == N.MAX_BOARDS == 8
    for fname, _ in N.BoardConfig._fields_:
        assert int(got[fname]) == getattr(N.BoardConfig, fname).offset, fname


def test_add_board_is_bound():
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.stream import Board, BoardPipeline
    lib = N.load()
    assert lib.cbv_pipeline_add_board.argtypes is not None
    per_board = ("results", "noise_results", "occupied", "changes_detailed", "square_stats", "hough", "download",
                 "update_references", "calibrate_changes", "set_check_squares", "reset_state", "close")
    for name in per_board:
        assert callable(getattr(Board, name)) and callable(getattr(BoardPipeline, name)), name
    assert callable(BoardPipeline.add_board)


def test_add_board_takes_configures_detector_defaults():
    """add_board and configure share one table of detector defaults: a board attached with no keywords is configured
    like the pipeline configured with none."""
    import inspect
    from chessboard_vision_amd.stream import DETECTOR_DEFAULTS, BoardPipeline
    sig = inspect.signature(BoardPipeline.configure).parameters
    assert {k: sig[k].default for k in DETECTOR_DEFAULTS} == DETECTOR_DEFAULTS
