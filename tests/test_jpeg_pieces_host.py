"""The piece path of the JPEG entropy decode without a GPU: cbv_jpeg_decode_host_ex in mode PIECES against the serial twin
(cbv_jpeg_decode_host by restart interval) at coefficient, plane, BGR and status level, at piece sizes from 4 bytes up, on
undamaged and damaged streams; the figures it reports; and the same comparison in a stand-alone program under
AddressSanitizer and UBSan over seeded damage (tools/jpeg_pieces_fuzz_host.cpp)."""
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

import jpeg_piece_cases as PC  # noqa: E402
import jpeg_streams as S  # noqa: E402
import ref_jpeg as R  # noqa: E402

PIECE_BYTES = (4, 8, 12, 64, 128, 4096)
LEVELS = ("BGR", "coefficients", "planes")


def decode(data, **kw):
    from chessboard_vision_amd.board_detection import jpeg_decode
    return jpeg_decode(data, host=True, **kw)


def check_pieces_equal_serial(name, data, sizes=PIECE_BYTES):
    """PIECES at every size = the serial twin; returns the stats by size"""
    from chessboard_vision_amd.board_detection import jpeg_probe
    info = jpeg_probe(data)
    serial = decode(data, entropy="interval", stats=True)
    assert serial[4] == dict(pieces=0, rounds=0, settled_round0=0), name
    out = {}
    for p in sizes:
        got = decode(data, entropy="pieces", piece_bytes=p, stats=True)
        for lvl, a, b in zip(LEVELS, got[:3], serial[:3]):
            assert np.array_equal(a, b), "%s, pieces of %d bytes: %d %s differ from the serial twin" % (name, p, np.count_nonzero(a != b), lvl)
        assert got[3] == serial[3], "%s, pieces of %d bytes: status %d, serial %d" % (name, p, got[3], serial[3])
        st = got[4]
        if info["restart_interval"]:
            assert st == dict(pieces=0, rounds=0, settled_round0=0), (name, p, st)
        else:
            assert st["pieces"] == max(1, -(-info["entropy_length"] // p)), (name, p, st)
            assert 1 <= st["rounds"] <= st["pieces"], (name, p, st)  # a condition of the algorithm: after round r, pieces 0..r are true
            assert 1 <= st["settled_round0"] <= st["pieces"], (name, p, st)  # piece 0 starts from the true state
            if st["pieces"] == 1:
                assert st["rounds"] == 1, (name, p, st)
        out[p] = st
    return out


def test_the_ex_symbols_exist_and_the_plain_calls_are_auto():
    from chessboard_vision_amd import _native as N
    lib = N.load()
    d = np.frombuffer(S.shape_stream(33, 50, "420"), np.uint8)
    out = [np.zeros((50, 33, 3), np.uint8) for _ in range(2)]
    st = C.c_int32(-1)
    ps = N.JpegDecodeStats()
    assert lib.cbv_jpeg_decode_host(N.ptr(d), d.size, N.ptr(out[0]), 99, None, None, C.byref(st)) == 0 and st.value == 0
    assert lib.cbv_jpeg_decode_host_ex(N.ptr(d), d.size, N.ptr(out[1]), 99, None, None, C.byref(st), N.JPEG_ENTROPY["auto"], 0, C.byref(ps)) == 0
    assert st.value == 0 and np.array_equal(out[0], out[1]) and np.array_equal(out[0], S.ref(d.tobytes())["bgr"])
    assert ps.pieces == -(-(d.size - R.parse(d.tobytes())["ent_off"]) // 64) and ps.rounds >= 1  # the default piece size, include/cbv.h
    assert lib.cbv_jpeg_decode_host_ex(N.ptr(d), d.size, N.ptr(out[1]), 99, None, None, C.byref(st), N.JPEG_ENTROPY["auto"], 0, None) == 0
    for mode, pb in ((3, 0), (-1, 0), (2, 2), (2, 6), (0, 1 << 25)):
        assert lib.cbv_jpeg_decode_host_ex(N.ptr(d), d.size, N.ptr(out[1]), 99, None, None, C.byref(st), mode, pb, None) == -1, (mode, pb)


@pytest.mark.parametrize("name,data", S.all_valid(), ids=[n for n, _ in S.all_valid()])
def test_pieces_equal_the_serial_twin(name, data):
    check_pieces_equal_serial(name, data)
    assert decode(data, entropy="pieces", piece_bytes=4)[3] == 0


def test_pieces_equal_the_serial_twin_on_the_recorded_cases():
    z = np.load(os.path.join(HERE, "golden", "jpeg_cases.npz"))
    names = [str(n) for n in z["names"]]
    assert len(names) == 127
    for i, n in enumerate(names):
        data = z["data_%d" % i].tobytes()
        check_pieces_equal_serial(n, data)
        assert np.array_equal(decode(data, entropy="pieces", piece_bytes=12)[0], z["bgr_%d" % i]), n


@pytest.mark.parametrize("name", sorted(S.DAMAGED))
def test_pieces_equal_the_serial_twin_on_the_fixed_damaged_streams(name):
    """these four have DRI and stay on the interval path; without their DRI segment the first restart marker ends the data"""
    d = S.damaged_stream(name)
    check_pieces_equal_serial(name, d)
    i = d.index(b"\xff\xdd\x00\x04")
    nodri = d[:i] + d[i + 6:]
    st = check_pieces_equal_serial(name + " without DRI", nodri)
    assert st[4]["pieces"] > 100
    assert decode(nodri, entropy="pieces", piece_bytes=4)[3] & R.NO_DATA


def test_a_frame_with_dri_stays_on_the_interval_path_in_auto():
    d = S.restart_stream("dri-mcu-row")
    a = decode(d, stats=True)
    b = decode(d, entropy="interval", stats=True)
    assert a[4]["pieces"] == 0 and a[4] == b[4]
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3] == 0


@pytest.mark.parametrize("name", PC.BOUNDARY)
def test_boundary_cases(name):
    """each stream puts its feature on a piece boundary at 4 bytes (tests/jpeg_piece_cases.py checks that it does)"""
    d = PC.boundary_case(name)
    st = check_pieces_equal_serial(name, d)
    assert st[4]["pieces"] >= 3
    got = decode(d, entropy="pieces", piece_bytes=4)
    if name.startswith("ends-in") or name == "stray-eoi-in-the-middle":
        assert got[3] == R.NO_DATA, got[3]
    elif name == "bad-code-in-the-middle":
        assert got[3] == R.BAD_CODE, got[3]
        coef = got[1].reshape(-1, 64)
        assert coef[:4].any() and not coef[12:].any(), "the blocks behind the bad code must stay 0"
        assert len(set(d[-40:-2])) > 8  # ... although the scan's own bytes follow it
    else:
        assert got[3] == 0, got[3]


def test_the_data_ends_where_the_cases_say():
    """a check of the fixtures alone (it calls no library code): the three streams end their data in the piece their names say"""
    n = {}
    for name in ("ends-in-first-piece", "stray-eoi-in-the-middle", "ends-in-last-piece"):
        d = PC.boundary_case(name)
        e = S.entropy_of(d)
        end = next((i for i in range(len(e) - 1) if e[i] == 0xFF and e[i + 1] != 0), len(e))
        n[name] = (end // 4, -(-len(e) // 4))
    assert n["ends-in-first-piece"][0] == 0 and n["ends-in-first-piece"][1] > 10
    assert 2 < n["stray-eoi-in-the-middle"][0] < n["stray-eoi-in-the-middle"][1] - 3
    assert n["ends-in-last-piece"][0] >= n["ends-in-last-piece"][1] - 1


def test_slow_resynchronisation_with_a_flat_ac_table():
    """162 AC symbols with 8-bit codes each: equality holds and rounds stay within the algorithm's bound however slowly the lanes fall into step"""
    d = PC.boundary_case(PC.SLOW)
    h = R.parse(d)
    assert {l for (l, _) in h["huff"][(1, 0)]} == {8} and len(h["huff"][(1, 0)]) == 162
    st = check_pieces_equal_serial(PC.SLOW, d)
    for p, s in st.items():
        print("flat AC table, pieces of %d bytes: %d pieces, %d rounds, %d settled in round 0" % (p, s["pieces"], s["rounds"], s["settled_round0"]))
    assert decode(d, entropy="pieces", piece_bytes=64)[3] == 0


def test_multi_component_frames_with_partial_mcus():
    for w, h, sampling in ((96, 56, "420"), (17, 23, "422"), (40, 9, "444")):
        check_pieces_equal_serial("%dx%d %s" % (w, h, sampling), PC.no_dri_picture(w, h, sampling), sizes=(4, 16, 128))


# ---------------------------------------------------------------------------------------------------------------------
# pieces against the serial twin under sanitizers: a stand-alone program (tools/jpeg_pieces_fuzz_host.cpp), on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_pieces_equal_the_serial_twin_under_sanitizers_on_seeded_damage(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "jpeg_pieces_fuzz_host"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "chessboard-vision_amd", "csrc"), os.path.join(ROOT, "tools", "jpeg_pieces_fuzz_host.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler has no sanitizer runtime: %s" % r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    files = []
    for i, d in enumerate([S.damage_base(), S.restart_stream("dri-wraps"), S.shape_stream(33, 50, "420"), S.shape_stream(17, 23, "gray"),
                           S.special_stream("long-codes-420"), S.special_stream("q1-q255-no-dht")]):
        p = tmp_path / ("s%d.jpg" % i)
        p.write_bytes(d)
        files.append(str(p))
    r = subprocess.run([str(exe), "600"] + files, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "3600 damaged streams" in r.stdout and " 0 decodes differ" in r.stdout, r.stdout
