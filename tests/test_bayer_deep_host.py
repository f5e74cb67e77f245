"""Developed mosaics without a GPU (include/cbv.h: Bayer samples of 10 to 16 bits, MIPI-packed rows, per-colour tables): the
restated encodings of tests/ref64_bayer_deep.py against themselves and against bytes spelled out by hand, the twelve new format
names, the neutral table and stream.Develop's tables against their float64 meaning, and the frame plan's cells of the new
encodings from the host tool (tools/frame_plan_host.cpp --bayer-deep), with the expected slot bytes written out here."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import ref64_bayer as RB
import ref64_bayer_deep as RD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------
# the encodings
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc", ("8", "16", "10p", "12p"))
def test_unpack_inverts_pack(enc):
    rng = np.random.default_rng(5)
    for w, h in ((4, 4), (8, 6), (12, 4), (324, 6)):
        s = rng.integers(0, 1 << RD.SAMPLE_BITS[enc], (h, w), dtype=np.int64)
        raw = RD.pack(s, enc)
        assert raw.shape == ((h, w) if enc in ("8", "16") else (h, RD.row_bytes(enc, w)))
        assert raw.dtype == (np.uint16 if enc == "16" else np.uint8)
        assert np.array_equal(RD.unpack(raw, enc), s), (enc, w, h)


def test_one_raw10_group_and_one_raw12_pair_by_hand():
    # RAW10: the samples 0x3FF, 0x000, 0x155, 0x2AA; high eight bits each, then the low two bits, sample 0 lowest
    #   0x3FF = 11111111 11   0x000 = 00000000 00   0x155 = 01010101 01   0x2AA = 10101010 10
    #   byte 4 = 10 01 00 11 = 0x93
    s = np.array([[0x3FF, 0x000, 0x155, 0x2AA]])
    assert RD.pack(s, "10p").tolist() == [[0xFF, 0x00, 0x55, 0xAA, 0x93]]
    assert RD.unpack(np.array([[0xFF, 0x00, 0x55, 0xAA, 0x93]], np.uint8), "10p").tolist() == s.tolist()
    # RAW12: the samples 0xABC, 0x123: high eight bits each, then the low nibbles, the even sample's lowest
    s = np.array([[0xABC, 0x123]])
    assert RD.pack(s, "12p").tolist() == [[0xAB, 0x12, 0x3C]]
    assert RD.unpack(np.array([[0xAB, 0x12, 0x3C]], np.uint8), "12p").tolist() == s.tolist()
    # the 16-bit container is little-endian: 0x1234 lies as 34 12
    assert RD.pack(np.array([[0x1234, 0x00FF]]), "16").astype("<u2").tobytes() == bytes([0x34, 0x12, 0xFF, 0x00])


def test_the_index_clamp_is_part_of_develop():
    t = RD.random_tables(10, 1)
    s = np.array([[0, 1023, 1024, 65535], [5, 2000, 1022, 40000], [0, 0, 0, 0], [0, 0, 0, 0]])
    m8 = RD.develop(s, "bayer_rggb", t, 10)
    # rows R G R G / G B G B: 1024, 2000, 40000 and 65535 read entry 1023 of their own colour's table
    assert m8[0, 1] == t[1][1023] and m8[0, 2] == t[2][1023] and m8[0, 3] == t[1][1023] and m8[1, 1] == t[0][1023] and m8[1, 3] == t[0][1023]
    assert m8[0, 0] == t[2][0] and m8[1, 0] == t[1][5] and m8[1, 2] == t[1][1022]


# ------------------------------------------------------------------------------------------------------------------
# the product's names, ids and tables
# ------------------------------------------------------------------------------------------------------------------
def test_format_ids_of_the_twelve_new_names():
    from chessboard_vision_amd import _native as N
    assert len(RD.IDS) == 12
    for name, fid in RD.IDS.items():
        assert N.format_id(name) == N.format_id(name.upper()) == fid, name
    assert RD.IDS["bayer_rggb16"] == 0x1004 and RD.IDS["bayer_bggr10p"] == 0x2014 and RD.IDS["bayer_gbrg12p"] == 0x3034
    for name in RB.FORMATS:                       # the 8-bit ids are what they were
        assert N.format_id(name) == RB.IDS[name]
    for bad in ("bayer_rggb14", "bayer_rggb10", "bayer_rggb12", "bayer_rggb8", "bayer_rggb16le"):
        with pytest.raises(ValueError):
            N.format_id(bad)
    # the kernels of developed mosaics have ids of their own, outside the ids every other test reads
    assert set(N.K_EVERY) - set(N.K_ALL) == {"INGEST_BAYER_DEEP", "WARP_BAYER_DEEP"}
    assert len(set(N.K_EVERY.values())) == len(N.K_EVERY)
    lib = N.load()
    assert lib.cbv_kernel_name(N.K_INGEST_BAYER_DEEP) == b"k_ingest_deep" and lib.cbv_kernel_name(N.K_WARP_BAYER_DEEP) == b"k_warp_deep"
    assert lib.cbv_kernel_name(N.K_WARP_BAYER_DEEP + 1) == b""


def test_raw_frames_of_the_new_names():
    from chessboard_vision_amd import _native as N
    s = np.random.default_rng(2).integers(0, 1024, (6, 8), dtype=np.int64)
    for enc, cols in (("16", 8), ("10p", 10), ("12p", 12)):
        a = RD.pack(s, enc)
        r, w, h, keep = N.raw_frame(a, "bayer_grbg" + enc)
        assert (r.fmt, w, h, r.stride0) == (RD.IDS["bayer_grbg" + enc], 8, 6, a.strides[0]) and a.shape[1] == cols
        parent = np.zeros((8, a.shape[1] + 3), a.dtype)
        view = parent[1:7, 2:2 + a.shape[1]]
        r, w, h, keep = N.raw_frame(view, "bayer_grbg" + enc)
        assert (w, h, r.stride0) == (8, 6, parent.strides[0]) and r.plane0 == view.ctypes.data
    with pytest.raises(ValueError):
        N.raw_frame(np.zeros((6, 8), np.uint8), "bayer_rggb16")       # a container is uint16
    with pytest.raises(ValueError):
        N.raw_frame(np.zeros((6, 9), np.uint8), "bayer_rggb10p")      # a RAW10 row is whole groups of five bytes
    with pytest.raises(ValueError):
        N.raw_frame(np.zeros((6, 8), np.uint8), "bayer_rggb12p")      # a RAW12 row is whole pairs of three bytes
    with pytest.raises(ValueError):
        N.raw_frame(np.zeros((5, 12), np.uint8), "bayer_rggb12p")     # an odd height
    with pytest.raises(ValueError):
        N.colorspace_bits("bt709", "bayer_rggb10p")


@pytest.mark.parametrize("bits", (10, 12, 14, 16))
def test_neutral_table_is_v_255_over_m_rounded_half_up(bits, exe):
    from chessboard_vision_amd import _native as N
    want = RD.neutral(bits)
    assert want[0, 0] == 0 and want[0, -1] == 255 and np.all(np.diff(want[0].astype(int)) >= 0)
    assert np.array_equal(N.neutral_tables(bits), want)
    lines = run(exe, "--bayer-neutral", bits)                         # the library's own (frame_plan.h, bayer_neutral_table)
    assert np.array_equal(np.array(lines[0].split(), dtype=np.int64), want[0])
    got = {int(l.split()[0].split("=")[1]): l for l in lines[1:]}
    assert "known=1" in got[0] and "known=1" in got[3] and "known=0" in got[4]
    assert ("ok=1" in got[1]) and ("ok=1" in got[2]) == (bits == 10) and ("ok=1" in got[3]) == (bits == 12) and "ok=0" in got[0]
    assert "default=0" in got[0] and "default=16" in got[1] and "default=10" in got[2] and "default=12" in got[3]


def test_develop_tables_follow_the_formula():
    from chessboard_vision_amd.stream import Develop
    for bits, kw in ((8, {}), (10, dict(black_level=64, white_level=1000, gains=(1.9, 1.0, 1.5), gamma=2.2)), (12, dict(black_level=256, gains=(2.0, 1.0, 1.25))),
                     (10, dict(gamma=0.5)), (8, dict(black_level=16, white_level=235, gains=(0.5, 1, 4), gamma=2.2))):
        t = Develop(bits, **kw).tables()
        assert t.shape == (3, 1 << bits) and t.dtype == np.uint8
        assert np.array_equal(t, RD.develop_tables(bits, **kw)), (bits, kw)
        assert np.all(np.diff(t.astype(int), axis=1) >= 0), "monotone"
    # gamma 1, no levels, unit gains: the neutral table
    for bits in (8, 10, 12, 14, 16):
        assert np.array_equal(Develop(bits).tables(), RD.neutral(bits))
    # the exactly representable points: black -> 0, white -> 255, whatever the gamma; a gain that saturates
    d = Develop(12, black_level=200, white_level=3000, gains=(2, 1, 4), gamma=2.2).tables()
    assert np.all(d[:, :201] == 0) and np.all(d[:, 3000:] == 255)
    assert d[2, 1600] == 255 and d[2, 1500] < 255          # red, gain 2: saturates at black + (white - black) / 2 (x = 1/2 exactly)
    assert d[0, 900] == 255 and d[0, 850] < 255            # blue, gain 4: at black + (white - black) / 4 (x = 1/4 exactly)
    assert d[1, 2900] < 255                                # green, gain 1: only at white
    lin = Develop(10, black_level=0, white_level=1020, gamma=1.0).tables()
    assert lin[1, 4] == 1 and lin[1, 1] == 0 and lin[1, 510] == 128 and lin[1, 1020] == 255    # v / 4; 127.5 rounds half up
    for bad in (dict(bits=11), dict(bits=10, white_level=5, black_level=5), dict(bits=10, gamma=0), dict(bits=10, gains=(1, 1))):
        with pytest.raises(ValueError):
            Develop(**bad)


def test_develop_json_round_trip(tmp_path):
    from chessboard_vision_amd.stream import Develop, load_develop, save_develop
    d = Develop(12, black_level=240, white_level=4000, gains=(1.8, 1.0, 1.6), gamma=2.2)
    path = str(tmp_path / "develop.json")
    written = save_develop(path, d)
    assert json.load(open(path)) == written == {"bits": 12, "black_level": 240.0, "white_level": 4000.0, "gains": [1.8, 1.0, 1.6], "gamma": 2.2}
    back = load_develop(path)
    assert back == d and np.array_equal(back.tables(), d.tables())
    with open(path, "w") as f:
        json.dump({"bits": 10}, f)
    assert load_develop(path) == Develop(10)


def test_tables_are_checked_against_the_encoding():
    from chessboard_vision_amd.develop import develop_tables
    from chessboard_vision_amd.stream import Develop
    assert develop_tables(None, RD.IDS["bayer_rggb10p"]) == (None, 0)
    t, bits = develop_tables(Develop(10), RD.IDS["bayer_rggb10p"])
    assert bits == 10 and t.shape == (3, 1024)
    for fmt, bad in (("bayer_rggb10p", 12), ("bayer_rggb12p", 10), ("bayer_rggb16", 8)):
        with pytest.raises(ValueError):
            develop_tables(Develop(bad), RD.IDS[fmt])
    with pytest.raises(ValueError):
        develop_tables(Develop(10), RB.IDS["bayer_rggb"])
    with pytest.raises(ValueError):
        develop_tables(np.zeros((3, 2048), np.uint8), RD.IDS["bayer_rggb16"])       # 11 bits anywhere
    with pytest.raises(ValueError):
        develop_tables(np.zeros((3, 1024), np.uint16), RD.IDS["bayer_rggb16"])
    for bits in (10, 12, 14, 16):
        assert develop_tables(RD.random_tables(bits, 0), RD.IDS["bayer_gbrg16"])[1] == bits


def test_new_symbols_are_declared_exported_and_bound():
    from chessboard_vision_amd import _native as N
    lib = N.load()
    header = open(os.path.join(ROOT, "include", "cbv.h")).read()
    for name in ("cbv_bayer_to_bgr", "cbv_pipeline_set_bayer_tables"):
        assert "CBV_API int %s(" % name in header
        assert getattr(lib, name).argtypes is not None
    for macro, value in (("CBV_BAYER_16", 0x1000), ("CBV_BAYER_10P", 0x2000), ("CBV_BAYER_12P", 0x3000), ("CBV_BAYER_ENC_MASK", 0xF000)):
        assert "#define %s " % macro in header and getattr(N, macro[4:]) == value
    # no device: null handles are refused before anything else
    assert lib.cbv_pipeline_set_bayer_tables(None, None, 0) == -1
    assert lib.cbv_bayer_to_bgr(None, None, 4, 4, None, 0, None, 12) == -1


# ------------------------------------------------------------------------------------------------------------------
# the frame plan's cells of the new encodings
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("frame_plan_deep") / "frame_plan_host"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "chessboard-vision_amd", "csrc"), os.path.join(ROOT, "tools", "frame_plan_host.cpp"),
                        "-o", str(out)], capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler has no sanitizer runtime: %s" % r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    return str(out)


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout.splitlines()


E, S1, P, PR = range(4)
# slot bytes by hand.  16 x 4: 16 * 2 * 4 = 128, 16 * 5 / 4 * 4 = 80, 16 * 3 / 2 * 4 = 96, each rounded up to 256.
# 1920 x 1080: 1920 * 2 * 1080 = 4 147 200, 2400 * 1080 = 2 592 000, 2880 * 1080 = 3 110 400, multiples of 256 already.
SLOTS = {(16, 4): {"16": (32, 128, 256), "10p": (20, 80, 256), "12p": (24, 96, 256)},
         (1920, 1080): {"16": (3840, 4147200, 4147200), "10p": (2400, 2592000, 2592000), "12p": (2880, 3110400, 3110400)}}


@pytest.mark.parametrize("size", sorted(SLOTS), ids=lambda s: "%dx%d" % s)
def test_frame_plan_cells_of_the_new_encodings(exe, size):
    w, h = size
    lines = run(exe, "--bayer-deep", w, h)
    cells = [(k, enc, lay) for k in (E, S1, P, PR) for enc in RD.ENCODINGS for lay in RD.LAYOUTS]
    assert len(lines) == len(cells) == 48
    for (k, enc, lay), line in zip(cells, lines):
        word = line.split()
        assert [int(x) for x in word[:2]] == [k, RD.IDS[lay + enc]], line
        got = {a.split("=")[0]: int(a.split("=")[1]) for a in word[2:]}
        row, frame, slot = SLOTS[size][enc]
        raw_kind = k in (S1, PR)
        want = {"bayer": 1, "enc": RD.ENCODINGS.index(enc) + 1, "row": row, "frame": frame, "slot": slot,
                "source": 1 if raw_kind else 0,            # raw mode: the raw ring is the frames
                "bgr": 0 if k == PR else 1,                 # ... and under PROFILE_RAW no BGR ring exists, as for 8-bit Bayer
                "pmode": 0, "depth": 0}
        assert got == want, (line, want)


def test_default_output_of_the_host_tool_is_what_it_was(exe):
    assert len(run(exe, 16, 4, 0, 0, 0, 8)) == 52
