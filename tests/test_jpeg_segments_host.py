"""The segments mode of the JPEG entropy decode without a GPU (include/cbv.h, CBV_JPEG_ENTROPY_SEGMENTS): every restart
interval cut into pieces.  cbv_jpeg_decode_host_ex in mode SEGMENTS against the serial twin (by restart interval) at
coefficient, plane, BGR and status level, at piece sizes from 4 bytes up, on undamaged and damaged streams; the figures it
reports against the streams' own bytes; and the same comparison in a stand-alone program under AddressSanitizer and UBSan
over seeded damage of streams with DRI (tools/jpeg_segments_fuzz_host.cpp)."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import jpeg_segment_cases as SC  # noqa: E402
import jpeg_streams as S  # noqa: E402
import ref_jpeg as R  # noqa: E402

LEVELS = ("BGR", "coefficients", "planes")
ZERO = dict(pieces=0, rounds=0, settled_round0=0)


def decode(data, **kw):
    from chessboard_vision_amd.board_detection import jpeg_decode
    return jpeg_decode(data, host=True, **kw)


def check_segments_equal_serial(name, data, sizes=SC.PIECE_BYTES):
    """SEGMENTS at every size = the serial twin, with the figures the stream's own bytes give; returns (serial, stats by size)"""
    from chessboard_vision_amd.board_detection import jpeg_probe
    info = jpeg_probe(data)
    serial = decode(data, entropy="interval", stats=True)
    assert serial[4] == ZERO, name
    out = {}
    for p in sizes:
        got = decode(data, entropy="segments", piece_bytes=p, stats=True)
        for lvl, a, b in zip(LEVELS, got[:3], serial[:3]):
            assert np.array_equal(a, b), "%s, pieces of %d bytes: %d %s differ from the serial twin" % (name, p, np.count_nonzero(a != b), lvl)
        assert got[3] == serial[3], "%s, pieces of %d bytes: status %d, serial %d" % (name, p, got[3], serial[3])
        st = got[4]
        if info["restart_interval"]:
            n = SC.piece_counts(data, p)
            assert len(n) == info["intervals"]
            assert st["pieces"] == sum(n), (name, p, st, sum(n))
            assert 1 <= st["rounds"] <= max(n), (name, p, st, max(n))  # after round r the pieces 0..r of every segment are true
            assert info["intervals"] <= st["settled_round0"] <= st["pieces"], (name, p, st)  # every first piece starts from the true state
        else:
            assert st == decode(data, entropy="pieces", piece_bytes=p, stats=True)[4], (name, p, st)
            assert st["pieces"] == max(1, -(-info["entropy_length"] // p)), (name, p, st)
        out[p] = st
    return serial, out


def test_mode_3_and_mode_5_are_refused_and_4_is_bound():
    from chessboard_vision_amd import _native as N
    lib = N.load()
    assert N.JPEG_ENTROPY["segments"] == 4
    d = np.frombuffer(S.restart_stream("dri-mcu-row"), np.uint8)
    out = np.zeros((48, 64, 3), np.uint8)
    st = C.c_int32(-1)
    ps = N.JpegDecodeStats()
    for mode in (3, 5):
        assert lib.cbv_jpeg_decode_host_ex(N.ptr(d), d.size, N.ptr(out), 192, None, None, C.byref(st), mode, 0, None) == -1, mode
    assert lib.cbv_jpeg_decode_host_ex(N.ptr(d), d.size, N.ptr(out), 192, None, None, C.byref(st), 4, 0, C.byref(ps)) == 0
    assert st.value == 0 and np.array_equal(out, S.ref(d.tobytes())["bgr"])
    assert ps.pieces == sum(SC.piece_counts(d.tobytes(), 64)) and ps.pieces >= 3  # the default piece size
    for pb in (2, 6, 1 << 25):
        assert lib.cbv_jpeg_decode_host_ex(N.ptr(d), d.size, N.ptr(out), 192, None, None, C.byref(st), 4, pb, None) == -1, pb


def test_pieces_mode_still_leaves_a_frame_with_dri_to_the_interval_path():
    d = S.restart_stream("dri-mcu-row")
    assert decode(d, entropy="pieces", piece_bytes=4, stats=True)[4] == ZERO
    assert decode(d, entropy="auto", stats=True)[4] == ZERO
    assert decode(d, entropy="segments", piece_bytes=4, stats=True)[4]["pieces"] > 100


@pytest.mark.parametrize("name", sorted(S.RESTART_CASES))
def test_restart_cases(name):
    d = S.restart_stream(name)
    serial, st = check_segments_equal_serial(name, d)
    assert serial[3] == 0 and np.array_equal(serial[0], S.ref(d)["bgr"])
    if name == "dri-two-waves":
        assert st[4]["pieces"] == 1222 and len(SC.piece_counts(d, 4)) == 84  # more pieces than the kernel's workgroup has lanes


@pytest.mark.parametrize("sampling", SC.LONG)
def test_long_intervals(sampling):
    d = SC.long_stream(sampling)
    serial, st = check_segments_equal_serial("96x56 %s dri 12" % sampling, d)
    assert serial[3] == 0 and np.array_equal(serial[0], S.ref(d)["bgr"])
    n = SC.piece_counts(d, 4)
    if sampling == "422":
        assert len(n) == 4 and sum(n) == 1374 and max(n) == 403
    else:
        assert [b - a for a, b in SC.segments(d)] == [2464, 2261]
    for p, s in st.items():
        print("%s, pieces of %d bytes: %s" % (sampling, p, s))


@pytest.mark.parametrize("name", sorted(S.DAMAGED))
def test_the_recorded_damaged_streams(name):
    d = S.damaged_stream(name)
    serial, _ = check_segments_equal_serial(name, d)
    assert serial[3] & S.DAMAGED[name] == S.DAMAGED[name]


@pytest.mark.parametrize("name,data", S.all_valid(), ids=[n for n, _ in S.all_valid()])
def test_every_valid_stream(name, data):
    serial, _ = check_segments_equal_serial(name, data)
    assert serial[3] == 0


def test_the_recorded_cases():
    z = np.load(os.path.join(HERE, "golden", "jpeg_cases.npz"))
    names = [str(n) for n in z["names"]]
    assert len(names) == 127
    for i, n in enumerate(names):
        data = z["data_%d" % i].tobytes()
        check_segments_equal_serial(n, data)
        assert np.array_equal(decode(data, entropy="segments", piece_bytes=12)[0], z["bgr_%d" % i]), n


@pytest.mark.parametrize("name", SC.DAMAGED)
def test_fixed_damaged_streams(name):
    """the expected status is the interval path's; what each stream must look like is checked on its bytes and on that decode"""
    d = SC.damaged(name)
    good = SC.long_stream("422")
    serial, st = check_segments_equal_serial(name, d)
    seg = SC.segments(d)
    lens = [b - a for a, b in seg]
    coef = serial[1]
    print("%s: status %d, segment bytes %s, at 4 bytes %s" % (name, serial[3], lens, st[4]))
    assert len(seg) == 4
    if name == "adjacent-markers":
        assert lens[1] == 0 and lens[0] > 1000 and serial[3] & R.NO_DATA and not serial[3] & R.RESTART
        assert SC.luma_block(d, coef, 24).any() and SC.luma_block(d, coef, 41).any()  # the intervals behind it decode
    elif name == "extra-marker":
        assert len(SC.markers(d)) == 4 and seg[3][0] < SC.markers(d)[3] < seg[3][1] and serial[3] & R.RESTART
    elif name == "marker-removed":
        assert len(SC.markers(d)) == 2 and lens[3] == 0 and serial[3] & R.RESTART
    elif name.startswith("cut-in"):
        k = {"cut-in-first-interval": 0, "cut-in-middle-interval": 2, "cut-in-last-interval": 3}[name]
        assert serial[3] & R.NO_DATA and bool(serial[3] & R.RESTART) == (k < 3)
        assert len(SC.markers(d)) == k and lens[k] > 100 and all(l == 0 for l in lens[k + 1:])
        assert SC.luma_block(d, coef, 12 * k).any()  # the cut interval decodes as far as its data goes
    elif name == "bad-code-in-middle-interval":
        assert serial[3] == R.BAD_CODE
        gcoef = decode(good, entropy="interval")[1]
        assert np.array_equal(SC.luma_block(d, coef, 12), SC.luma_block(good, gcoef, 12)) and SC.luma_block(d, coef, 12).any()
        for m in (22, 23):  # the blocks behind the bad code inside its interval stay 0, although its own bytes go on
            assert not any(SC.luma_block(d, coef, m, b).any() for b in range(2)), m
        for m in (24, 30, 36, 41):  # the two intervals behind it decode
            assert np.array_equal(SC.luma_block(d, coef, m), SC.luma_block(good, gcoef, m)) and SC.luma_block(good, gcoef, m).any(), m
    elif name == "short-next-to-long":
        assert lens[1] == 2 and SC.piece_counts(d, 4)[1] == 1 and SC.piece_counts(d, 4)[0] > 300
        assert SC.luma_block(d, coef, 24).any()
    assert serial[3] != 0


def test_cut_streams_lose_their_markers_as_the_names_say():
    """a check of the fixtures alone: where each cut stream ends"""
    good = SC.segments(SC.long_stream("422"))
    for name, k in (("cut-in-first-interval", 0), ("cut-in-middle-interval", 2), ("cut-in-last-interval", 3)):
        d = SC.damaged(name)
        assert good[k][0] + 50 < len(d) < good[k][1] - 50, name


# ---------------------------------------------------------------------------------------------------------------------
# segments against the serial twin under sanitizers: a stand-alone program (tools/jpeg_segments_fuzz_host.cpp), on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_segments_equal_the_serial_twin_under_sanitizers_on_seeded_damage(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "jpeg_segments_fuzz_host"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "chessboard-vision_amd", "csrc"), os.path.join(ROOT, "tools", "jpeg_segments_fuzz_host.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler has no sanitizer runtime: %s" % r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    files = []
    for i, d in enumerate(SC.fuzz_streams()):
        p = tmp_path / ("s%d.jpg" % i)
        p.write_bytes(d)
        files.append(str(p))
    fixed = []  # every damaged stream tests/test_gpu_jpeg_segments.py gives the GPU, as it is
    for i, d in enumerate(SC.gpu_damaged_streams()):
        p = tmp_path / ("fixed%d.jpg" % i)
        p.write_bytes(d)
        fixed.append(str(p))
    assert len(fixed) == 12
    r = subprocess.run([str(exe), "600"] + files + ["--fixed"] + fixed, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    print(r.stdout)
    assert "1800 damaged streams" in r.stdout and " 12 fixed streams, 12 of them with a status" in r.stdout and " 0 decodes differ" in r.stdout, r.stdout
