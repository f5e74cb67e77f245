"""The session chain of the pipeline (cbv_pipeline_config::skip_enhance, BoardPipeline.configure(enhance=False)) as far
as it shows without a GPU: the C-ABI field, its ctypes mirror, the Python keyword, the new kernel's id."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_holds_skip_enhance_where_the_ctypes_mirror_has_it(tmp_path):
    """include/cbv.h compiled as C99: skip_enhance is the LAST field of cbv_pipeline_config (appended: a config written for
    the struct as it was, zero-initialised, keeps today's behaviour), at the mirror's offset, and the struct has the
    mirror's size."""
    from chessboard_vision_amd import _native as N
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    assert N.PipelineConfig._fields_[-1][0] == "skip_enhance" and N.PipelineConfig._fields_[-2][0] == "enhance_region"
    src = tmp_path / "f.c"
    src.write_text("\n".join([
        '#include <stddef.h>', '#include <stdio.h>', '#include "cbv.h"', 'int main(void) {',
        'cbv_pipeline_config c = {0};',
        'printf("size %zu\\n", sizeof(c));',
        'printf("skip %zu\\n", offsetof(cbv_pipeline_config, skip_enhance));',
        'printf("region %zu\\n", offsetof(cbv_pipeline_config, enhance_region));',
        'printf("width %zu\\n", sizeof(c.skip_enhance));',
        'printf("zero %d\\n", (int)c.skip_enhance);',
        'printf("kid %d %d\\n", CBV_K_WARP_YUV, CBV_K_COUNT);',
        'return 0;', '}']))
    exe = tmp_path / "f"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = {l.split()[0]: l.split()[1:] for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()}
    assert int(got["size"][0]) == C.sizeof(N.PipelineConfig)
    assert int(got["skip"][0]) == N.PipelineConfig.skip_enhance.offset > int(got["region"][0]) == N.PipelineConfig.enhance_region.offset
    assert int(got["width"][0]) == 4 and int(got["zero"][0]) == 0
    assert int(got["kid"][0]) == N.K_WARP_YUV == int(got["kid"][1]) - 1
    # nothing after the field but padding
    assert N.PipelineConfig.skip_enhance.offset + 4 + 7 >= C.sizeof(N.PipelineConfig)


def test_kernel_id_and_name():
    from chessboard_vision_amd import _native as N
    lib = N.load()
    assert lib.cbv_kernel_name(N.K_WARP_YUV) == b"k_warp_yuv"
    # outside the default path, like MODEL_SCAN: not in the list bench.py walks; the ids known so far keep their numbers
    assert "WARP_YUV" not in N.KERNEL_IDS and N.K_WARP_YUV == N.K["MODEL_SCAN"] + 1 == max(N.K.values()) + 1


def test_configure_has_the_enhance_keyword():
    from chessboard_vision_amd.stream import Board, BoardPipeline
    par = inspect.signature(BoardPipeline.configure).parameters
    assert "enhance" in par and par["enhance"].default is True
    doc = BoardPipeline.configure.__doc__
    assert "game_session.py:123-161" in doc and "process_pipeline" in doc
    assert "enhance" not in inspect.signature(Board.__init__).parameters  # a board follows its pipeline


def test_product_still_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "chessboard-vision_amd")
    seen = 0
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "cbv_oracle" not in txt and "from oracle" not in txt and "import oracle" not in txt, f
                seen += 1
    assert seen > 20
