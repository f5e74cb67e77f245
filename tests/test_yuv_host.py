"""Camera-native frames (NV12, YUYV), the parts that need no GPU: the integer definition of the conversion against its
float64 form, the layout of cbv_raw_frame against gcc, the bound entry points and their argument checks."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ref64_yuv as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixed_point_is_within_one_of_float64_over_the_whole_cube():
    """Every (Y, U, V) triple: the int64 restatement of the 20-bit fixed-point definition differs from the float64 form
    by at most 1, in each channel on fewer than 0.1 % of the triples (B 7 168, G 4 385, R 16 384 of 16 777 216; 27 926
    triples = 0.17 % differ in at least one channel), and no intermediate leaves the signed 32-bit range."""
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    differ, triples, worst, extreme = np.zeros(3, np.int64), 0, 0, 0
    for y in range(256):
        Y = np.full_like(u, y)
        fixed, ext = R.yuv_to_bgr_int(Y, u, v, with_extremes=True)
        d = np.abs(fixed.astype(np.int16) - R.yuv_to_bgr_float(Y, u, v).astype(np.int16))
        differ += np.count_nonzero(d, axis=(0, 1))
        triples += int(np.count_nonzero(d.max(axis=-1)))
        worst, extreme = max(worst, int(d.max())), max(extreme, ext)
    print("values that differ (B, G, R): %s of %d each, %d triples in some channel; largest difference %d, largest "
          "intermediate %d" % (differ.tolist(), 1 << 24, triples, worst, extreme))
    assert worst <= 1
    assert (differ < (1 << 24) / 1000).all()
    assert extreme < 2 ** 31 and 5.5e8 < extreme < 5.7e8


def test_gray_axis():
    """U = V = 128: both forms give 0 up to Y = 16 and 255 from Y = 235, equal channels everywhere, and differ at one
    luma value only, Y = 141 (1.164 * 125 = 145.5 exactly: half to even gives 146, the fixed-point constant is a hair
    under 1.164 * 2^20 and gives 145)."""
    Y = np.arange(256)
    c = np.full(256, 128)
    fixed, flt = R.yuv_to_bgr_int(Y, c, c), R.yuv_to_bgr_float(Y, c, c)
    for a in (fixed, flt):
        assert (a[:17] == 0).all() and (a[235:] == 255).all()
        assert (a[..., 0] == a[..., 1]).all() and (a[..., 1] == a[..., 2]).all()
        assert (np.diff(a[..., 0].astype(int)) >= 0).all()
    assert np.flatnonzero((fixed != flt).any(axis=-1)).tolist() == [141]
    assert fixed[141, 0] == 145 and flt[141, 0] == 146


def test_constants_are_the_rounded_bt601_coefficients():
    assert [R.CY, R.CUB, -R.CUG, -R.CVG, R.CVR] == [int(round(c * 2 ** 20)) for c in (1.164, 2.018, 0.391, 0.813, 1.596)]


def test_generators_round_trip_and_cubes_hold_every_triple():
    """The input generators produce frames of the documented layouts; a gray ramp survives BGR -> YUV -> BGR within the
    quantisation of the limited range."""
    g = np.repeat(np.arange(0, 256, 4, dtype=np.uint8)[None, :, None], 4, axis=0).repeat(3, axis=2)   # [4, 64, 3]
    for fmt in ("nv12", "yuyv"):
        raw = R.from_bgr(g, fmt)
        assert raw.shape == ((6, 64) if fmt == "nv12" else (4, 64, 2)) and raw.dtype == np.uint8
        assert np.abs(R.to_bgr(raw, fmt).astype(int) - g).max() <= 2
    Y, U, V = R.split_nv12(R.cube_nv12())
    key = (Y.astype(np.int64) << 16 | U.astype(np.int64) << 8 | V).ravel()
    assert key.size == 1 << 24 and np.unique(key).size == 1 << 24
    keys = []
    for part in range(4):
        Y, U, V = R.split_yuyv(R.cube_yuyv(part))
        keys.append((Y.astype(np.int64) << 16 | U.astype(np.int64) << 8 | V).ravel())
    key = np.concatenate(keys)
    assert key.size == 1 << 24 and np.unique(key).size == 1 << 24


def test_raw_frame_layout_matches_gcc(tmp_path):
    from chessboard_vision_amd import _native as N
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "cbv.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(cbv_raw_frame));',
             'printf("fmts %d%d%d\\n", CBV_FMT_BGR, CBV_FMT_NV12, CBV_FMT_YUYV);', 'printf("kid %d\\n", CBV_K_INGEST);']
    for fname, _ in N.RawFrame._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(cbv_raw_frame, %s));' % (fname, fname))
    lines += ["return 0;", "}"]
    src = tmp_path / "raw_abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "raw_abi"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(N.RawFrame)
    assert got["fmts"] == "%d%d%d" % (N.FMT_BGR, N.FMT_NV12, N.FMT_YUYV) == "012"
    assert int(got["kid"]) == N.K["INGEST"] == len(N.KERNEL_IDS) - 1
    for fname, _ in N.RawFrame._fields_:
        assert int(got[fname]) == getattr(N.RawFrame, fname).offset, fname


def test_entry_points_are_bound():
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.board_detection import yuv_to_bgr
    from chessboard_vision_amd.stream import BoardPipeline
    lib = N.load()
    for name in ("cbv_yuv_to_bgr", "cbv_pipeline_upload_raw", "cbv_pipeline_set_input_format", "cbv_pipeline_host_slot_bytes"):
        assert getattr(lib, name).argtypes is not None, name
    assert lib.cbv_pipeline_host_slot_bytes.restype is C.c_size_t
    assert lib.cbv_kernel_name(N.K["INGEST"]) == b"k_ingest"
    assert callable(yuv_to_bgr) and callable(BoardPipeline.set_input_format)


def test_argument_checks_without_a_device():
    from chessboard_vision_amd import _native as N
    lib = N.load()
    raw = N.RawFrame()
    out = np.zeros((2, 2, 3), np.uint8)
    assert lib.cbv_yuv_to_bgr(None, raw, 2, 2, N.ptr(out), 6) == -1
    assert b"cbv_yuv_to_bgr" in lib.cbv_last_error(None)
    assert lib.cbv_pipeline_set_input_format(None, N.FMT_NV12) == -1
    assert b"cbv_pipeline_set_input_format" in lib.cbv_last_error(None)
    assert lib.cbv_pipeline_upload_raw(None, 0, raw) == -1
    assert lib.cbv_pipeline_host_slot_bytes(None) == 0


def test_raw_frame_views():
    """N.raw_frame: the accepted shapes, strided views taken as they are, everything else refused."""
    from chessboard_vision_amd import _native as N
    big = np.zeros((12, 16), np.uint8)
    r, w, h, keep = N.raw_frame(big[:6, :8], "nv12")                      # one [h * 3 // 2, w] view
    assert (r.fmt, w, h, r.stride0, r.stride1) == (N.FMT_NV12, 8, 4, 16, 16) and r.plane1 - r.plane0 == 4 * 16
    r, w, h, keep = N.raw_frame((big[:4, :8], big[8:10, 4:12]), "NV12")   # a (y, uv) pair
    assert (w, h, r.stride0, r.stride1) == (8, 4, 16, 16) and r.plane1 - r.plane0 == 8 * 16 + 4
    r, w, h, keep = N.raw_frame((big[:4, :8], np.zeros((2, 4, 2), np.uint8)), "nv12")
    assert (w, h, r.stride1) == (8, 4, 8)
    yuyv = np.zeros((4, 10, 2), np.uint8)
    r, w, h, keep = N.raw_frame(yuyv[:, :6], "yuyv")
    assert (r.fmt, w, h, r.stride0) == (N.FMT_YUYV, 6, 4, 20) and not r.plane1
    for bad, fmt in ((np.zeros((5, 8), np.uint8), "nv12"), (np.zeros((4, 8, 3), np.uint8), "yuyv"),
                     ((big[:4, :8], big[:2, :6]), "nv12"), (np.zeros((6, 8), np.float32), "nv12"), (big, "i420")):
        with pytest.raises(ValueError):
            N.raw_frame(bad, fmt)
