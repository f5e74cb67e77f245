"""Baseline JPEG without a GPU: tests/ref_jpeg.py (the numpy restatement of include/cbv.h's definition) against recorded and
live Pillow decodes, the library's host twin (cbv_jpeg_decode_host) against ref_jpeg at coefficient, plane and BGR level,
the header probe and its refusals, and the twin under AddressSanitizer and UBSan on seeded damage."""
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
sys.path.insert(0, os.path.join(HERE, "golden"))

import jpeg_streams as S  # noqa: E402
import ref_jpeg as R  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "jpeg_cases.npz"))
    names = [str(n) for n in z["names"]]
    return [(n, z["data_%d" % i].tobytes(), z["bgr_%d" % i]) for i, n in enumerate(names)]


def twin(data):
    from chessboard_vision_amd.board_detection import jpeg_decode
    return jpeg_decode(data, host=True)


def assert_same(got, ref, what):
    bgr, coef, planes, st = got
    assert np.array_equal(coef, ref["coef"]), "%s: %d coefficients differ" % (what, np.count_nonzero(coef != ref["coef"]))
    assert np.array_equal(planes, ref["planes"]), "%s: %d plane samples differ" % (what, np.count_nonzero(planes != ref["planes"]))
    assert np.array_equal(bgr, ref["bgr"]), "%s: %d BGR bytes differ" % (what, np.count_nonzero(bgr != ref["bgr"]))
    assert st == ref["status"], "%s: status %d, reference %d" % (what, st, ref["status"])


def test_ref_equals_every_recorded_pillow_decode(golden):
    assert len(golden) >= 120
    assert any("rstmcu" in n for n, _, _ in golden) and any("rstrow" in n for n, _, _ in golden) and any("opt" in n for n, _, _ in golden)
    for name, data, bgr in golden:
        r = R.decode(data)
        assert r["status"] == 0, name
        assert np.array_equal(r["bgr"], bgr), "%s: %d bytes differ from Pillow's decode" % (name, np.count_nonzero(r["bgr"] != bgr))


def test_twin_equals_every_recorded_pillow_decode(golden):
    for name, data, bgr in golden:
        got = twin(data)
        assert got[3] == 0, name
        assert np.array_equal(got[0], bgr), "%s: %d bytes differ from Pillow's decode" % (name, np.count_nonzero(got[0] != bgr))


def test_recorded_file_without_dht_uses_the_standard_tables(golden):
    from chessboard_vision_amd.board_detection import jpeg_probe
    by = {n: (d, b) for n, d, b in golden}
    d, b = by["33x50-noise-422-q90-nodht"]
    assert b"\xff\xc4" not in d[:d.index(b"\xff\xda")]
    info = jpeg_probe(d)
    assert info["std_tables"] == 1 and (info["w"], info["h"], info["hs"], info["vs"]) == (33, 50, 2, 1)
    assert np.array_equal(twin(d)[0], b)
    assert jpeg_probe(golden[0][1])["std_tables"] == 0  # Pillow writes its tables


def test_ref_equals_live_pillow_on_the_full_matrix():
    pytest.importorskip("PIL")
    import make_jpeg_cases as M
    cases = M.matrix()
    assert len(cases) == 504
    bad = []
    for i, case in enumerate(cases):
        data, bgr = M.pillow_encode(case, i)
        r = R.decode(data)
        if r["status"] != 0 or not np.array_equal(r["bgr"], bgr):
            bad.append(case[0])
    assert not bad, "%d of 504 differ from Pillow: %s" % (len(bad), bad[:8])


@pytest.mark.parametrize("name,data", S.all_valid(), ids=[n for n, _ in S.all_valid()])
def test_twin_equals_ref(name, data):
    ref = S.ref(data)
    assert ref["status"] == 0
    assert_same(twin(data), ref, name)


def test_special_streams_hold_what_they_are_for():
    d = S.special_stream("long-codes-gray")
    assert b"\xff\x00" in S.entropy_of(d)[:-2], "no stuffed FF 00 in the entropy data"
    c = S.ref(d)["coef"].reshape(4, 64)
    assert c[0, 0] == 2047 and c[1, 0] == 0 and c[0, 1] == 1023 and c[0, 63] == 1 and not c[1].any() and not c[3, 1:].any()
    h = R.parse(d)
    assert {l for (l, _) in h["huff"][(1, 0)]} == set(range(1, 17)) and {l for (l, _) in h["huff"][(0, 0)]} == set(range(1, 17))
    h = R.parse(S.special_stream("q1-q255"))
    assert sorted(h["q"]) == [0, 2] and set(h["q"][0]) == {1} and set(h["q"][2]) == {255}
    assert S.special_stream("q1-q255-split-dht").count(b"\xff\xc4") == 4 and S.special_stream("q1-q255").count(b"\xff\xc4") == 1
    assert b"\xff\xc4" not in S.special_stream("q1-q255-no-dht")
    seg = S.special_stream("q1-q255-segments")
    assert seg[2:5] == b"\xff\xff\xff" and b"Exif" in seg and b"a comment" in seg
    for n in ("q1-q255-split-dht", "q1-q255-no-dht", "q1-q255-segments"):  # the same picture whatever the packaging
        assert np.array_equal(S.ref(S.special_stream(n))["bgr"], S.ref(S.special_stream("q1-q255"))["bgr"])
    assert not S.ref(S.special_stream("zero-blocks-422"))["coef"].any()
    assert R.parse(S.restart_stream("dri-wraps"))["nint"] > 8 and R.parse(S.restart_stream("dri-two-waves"))["nint"] > 64


def test_coefficient_round_trip_is_exact():
    rs = np.random.RandomState(3)
    for sampling, (w, h) in (("444", (17, 9)), ("422", (33, 8)), ("420", (20, 40)), ("gray", (9, 17))):
        hs, vs = R.SAMPLINGS[sampling]
        mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
        shapes = [(my * vs, mx * hs)] + ([] if sampling == "gray" else [(my, mx), (my, mx)])
        coefs = []
        for bh, bw in shapes:
            a = rs.randint(-40, 41, (bh, bw, 64)) * (rs.rand(bh, bw, 64) < 0.2)
            a[..., 0] = rs.randint(-1000, 1001, (bh, bw))
            coefs.append(a.astype(np.int64))
        for dri in (0, 1, 3):
            d = R.encode_coefs(coefs, w, h, sampling, {0: np.ones(64, np.int64), 1: np.full(64, 2, np.int64)}, dri=dri)
            want = np.concatenate([c.reshape(-1) for c in coefs])
            r = S.ref(d)
            assert r["status"] == 0 and np.array_equal(r["coef"], want), (sampling, dri)
            got = twin(d)
            assert got[3] == 0 and np.array_equal(got[1], want), (sampling, dri)


@pytest.mark.parametrize("name", sorted(S.DAMAGED))
def test_twin_equals_ref_on_the_fixed_damaged_streams(name):
    d = S.damaged_stream(name)
    ref = S.ref(d)
    assert ref["status"] & S.DAMAGED[name] == S.DAMAGED[name], ref["status"]
    assert_same(twin(d), ref, name)
    # a wrong number costs the status bit only: the intervals are found by position
    assert np.array_equal(ref["bgr"], S.ref(S.damage_base())["bgr"]) == (name == "wrong-restart-number")


# ---------------------------------------------------------------------------------------------------------------------
# the probe
# ---------------------------------------------------------------------------------------------------------------------
def probe_rc(data):
    from chessboard_vision_amd import _native as N
    lib = N.load()
    a = np.frombuffer(bytes(data), np.uint8)
    info = N.JpegInfo()
    rc = lib.cbv_jpeg_probe(N.ptr(a), a.size, C.byref(info))
    return rc, lib.cbv_last_error(None).decode() if rc else "", info


def test_probe_returns_the_fields():
    for name, (w, h, sampling, dri) in S.RESTART_CASES.items():
        d = S.restart_stream(name)
        rc, _, info = probe_rc(d)
        hd = R.parse(d)
        assert rc == 0
        assert (info.w, info.h, info.components) == (w, h, 3)
        assert (info.hs, info.vs) == R.SAMPLINGS[sampling]
        assert info.restart_interval == dri and info.intervals == hd["nint"] and info.std_tables == 0
        assert info.entropy_offset == hd["ent_off"] and info.entropy_offset + info.entropy_length == len(d)
        assert [(info.blocks_w[c], info.blocks_h[c]) for c in range(3)] == [(c["bw"], c["bh"]) for c in hd["comps"]]
        assert info.plane_elems == sum(c["bw"] * c["bh"] * 64 for c in hd["comps"])
    rc, _, info = probe_rc(S.shape_stream(17, 23, "gray"))
    assert rc == 0 and (info.components, info.hs, info.vs, info.intervals, info.restart_interval) == (1, 1, 1, 1, 0)
    assert probe_rc(S.special_stream("q1-q255-no-dht"))[2].std_tables == 1


def _seg(m, payload):
    return bytes([0xFF, m]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def _header(sof_marker=0xC0, precision=8, comps=((1, 0x22, 0), (2, 0x11, 1), (3, 0x11, 1)), dqt=b"\x00" + bytes([1] * 64) + b"\x01" + bytes([1] * 64),
            extra=b"", scan_comps=None, w=16, h=16):
    sof = bytes([precision]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([len(comps)]) + b"".join(bytes(c) for c in comps)
    sc = comps if scan_comps is None else scan_comps
    sos = bytes([len(sc)]) + b"".join(bytes([c[0], 0x00 if i == 0 else 0x11]) for i, c in enumerate(sc)) + bytes([0, 63, 0])
    return b"\xff\xd8" + extra + _seg(0xDB, dqt) + _seg(sof_marker, sof) + _seg(0xDA, sos) + b"\x00\xff\xd9"


REFUSED = {
    "progressive": (_header(sof_marker=0xC2), "progressive"),
    "arithmetic": (_header(sof_marker=0xC9), "arithmetic"),
    "12-bit": (_header(sof_marker=0xC1, precision=12), "12-bit"),
    "12-bit-sof0": (_header(precision=12), "12-bit"),
    "16-bit-dqt": (_header(dqt=b"\x10" + bytes(128)), "16-bit quantisation"),
    "several-scans": (_header(scan_comps=((1, 0x22, 0),)), "several scans"),
    "four-components": (_header(comps=((1, 0x11, 0), (2, 0x11, 0), (3, 0x11, 0), (4, 0x11, 0))), "four components"),
    "adobe-transform-0": (_header(extra=_seg(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x00"), comps=((1, 0x11, 0), (2, 0x11, 1), (3, 0x11, 1))), "Adobe"),
    "sampling-1x2": (_header(comps=((1, 0x12, 0), (2, 0x11, 1), (3, 0x11, 1))), "sampling"),
    "sampling-4x1": (_header(comps=((1, 0x41, 0), (2, 0x11, 1), (3, 0x11, 1))), "sampling"),
    "sampling-chroma-2x1": (_header(comps=((1, 0x22, 0), (2, 0x21, 1), (3, 0x21, 1))), "sampling"),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_probe_refuses_with_the_reason(name):
    data, word = REFUSED[name]
    rc, msg, _ = probe_rc(data)
    assert rc == -5, (rc, msg)
    assert word in msg and "cbv_jpeg_probe" in msg, msg


def test_hand_built_header_is_accepted_when_nothing_is_wrong():
    rc, msg, info = probe_rc(_header())
    assert rc == 0, msg
    assert (info.w, info.h, info.hs, info.vs, info.std_tables) == (16, 16, 2, 2, 1)
    rc, msg, _ = probe_rc(_header(extra=_seg(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x01")))
    assert rc == 0, msg


@pytest.mark.parametrize("name,data", [
    ("no-soi", b"\x00\x01\x02\x03\x04"), ("soi-only", b"\xff\xd8\xff\xd9"), ("cut-in-segment", _header()[:30]), ("no-sos", _header()[:-20]),
    ("segment-length-1", b"\xff\xd8\xff\xe0\x00\x01\x00"), ("no-dqt", _header(dqt=b"")), ("zero-width", _header(w=0)),
    ("sos-before-sof", b"\xff\xd8" + _seg(0xDA, b"\x01\x01\x00\x00\x3f\x00")), ("garbage-between", b"\xff\xd8\x12\x34" + _header()[2:]),
])
def test_malformed_headers_are_argument_errors(name, data):
    rc, msg, _ = probe_rc(data)
    assert rc == -1, (rc, msg)
    assert msg


def test_decode_host_argument_errors():
    from chessboard_vision_amd import _native as N
    lib = N.load()
    d = np.frombuffer(S.shape_stream(8, 8, "444"), np.uint8)
    out = np.zeros((8, 8, 3), np.uint8)
    st = C.c_int32()
    assert lib.cbv_jpeg_decode_host(None, 10, N.ptr(out), 24, None, None, C.byref(st)) == -1
    assert lib.cbv_jpeg_decode_host(N.ptr(d), d.size, N.ptr(out), 23, None, None, C.byref(st)) == -1
    assert b"stride" in lib.cbv_last_error(None)
    assert lib.cbv_jpeg_decode(None, N.ptr(d), d.size, N.ptr(out), 24, None, None, C.byref(st)) == -1
    assert lib.cbv_jpeg_decode_host(N.ptr(d), d.size, N.ptr(out), 24, None, None, C.byref(st)) == 0 and st.value == 0
    assert np.array_equal(out, S.ref(d.tobytes())["bgr"])


# ---------------------------------------------------------------------------------------------------------------------
# the twin under sanitizers: a stand-alone program (tools/jpeg_fuzz_host.cpp), here on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_twin_is_clean_under_sanitizers_on_seeded_damage(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "jpeg_fuzz_host"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "chessboard-vision_amd", "csrc"), os.path.join(ROOT, "tools", "jpeg_fuzz_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
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
    assert "3600 damaged streams" in r.stdout, r.stdout
