"""The host side of the Motion-JPEG planes mode (include/cbv.h, cbv_pipeline_set_jpeg_planes): the size of a slot of the
plane ring against the header probe, and the ABI of the new entry points.  No GPU.

cbv_jpeg_plane_slot_bytes(w, h, mode) is the largest plane_elems among the samplings the mode admits (gray; 4:2:0 adds
4:2:0; 4:2:2 adds 4:2:2; 4:4:4 adds 4:4:4), rounded up to 256.  The expected value comes from cbv_jpeg_probe on a stream of
that size and sampling: a small stream of tests/ref_jpeg.py's encoder whose SOF0 size fields are rewritten (the probe reads
the header alone)."""
import ctypes as C
import os
import re

import pytest

import jpeg_streams as JS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (16, 1), (1, 16), (17, 23), (640, 480), (1920, 1080)]
ADMITS = {"gray": ("gray",), "420": ("gray", "420"), "422": ("gray", "420", "422"), "444": ("gray", "420", "422", "444")}


def _header_of(w, h, sampling):
    """a stream whose header says w x h in `sampling`"""
    d = bytearray(JS.shape_stream(8, 8, sampling))
    i = d.index(b"\xff\xc0")
    assert d[i + 4] == 8  # the precision byte of SOF0
    d[i + 5:i + 9] = bytes([h >> 8, h & 255, w >> 8, w & 255])
    return bytes(d)


def _plane_elems(w, h, sampling):
    from chessboard_vision_amd.board_detection import jpeg_probe
    info = jpeg_probe(_header_of(w, h, sampling))
    assert (info["w"], info["h"]) == (w, h)
    return info["plane_elems"]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_slot_bytes_is_the_largest_admitted_sampling_rounded_to_256(size):
    from chessboard_vision_amd.stream import jpeg_plane_slot_bytes
    w, h = size
    got = {}
    for mode, admitted in ADMITS.items():
        most = max(_plane_elems(w, h, s) for s in admitted)
        got[mode] = jpeg_plane_slot_bytes(w, h, mode)
        assert got[mode] == (most + 255) // 256 * 256, (size, mode, most)
    assert got["420"] >= got["gray"] and got["422"] >= got["420"] and got["444"] >= got["422"]
    assert jpeg_plane_slot_bytes(w, h, True) == got["444"]


def test_the_largest_is_not_always_the_named_sampling():
    """at 16 x 1 a 4:2:0 frame (one 16 x 16 MCU: 384 samples) needs more than a 4:2:2 frame (one 16 x 8 MCU: 256)"""
    from chessboard_vision_amd.stream import jpeg_plane_slot_bytes
    assert _plane_elems(16, 1, "420") == 384 and _plane_elems(16, 1, "422") == 256
    assert jpeg_plane_slot_bytes(16, 1, "422") == 512


def test_zero_for_off_unknown_modes_and_bad_sizes():
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.stream import jpeg_plane_slot_bytes
    lib = N.load()
    assert jpeg_plane_slot_bytes(640, 480, False) == 0 and jpeg_plane_slot_bytes(640, 480, None) == 0
    for mode in (-1, 5, 99):
        assert lib.cbv_jpeg_plane_slot_bytes(640, 480, mode) == 0
    for w, h in ((0, 480), (640, 0), (-3, 5), (5, -3)):
        for mode in N.JPEG_PLANES.values():
            assert lib.cbv_jpeg_plane_slot_bytes(w, h, mode) == 0
    with pytest.raises(ValueError):
        jpeg_plane_slot_bytes(640, 480, "411")


def test_the_mode_constants():
    txt = open(os.path.join(ROOT, "include", "cbv.h")).read()
    from chessboard_vision_amd import _native as N
    for name, key in (("OFF", "off"), ("GRAY", "gray"), ("420", "420"), ("422", "422"), ("444", "444")):
        m = re.search(r"#define CBV_JPEG_PLANES_%s (\d+)" % name, txt)
        assert m and int(m.group(1)) == N.JPEG_PLANES[key]
    assert N.JPEG_PLANES["off"] == 0


# the C types of the new declarations as ctypes binds them
CTYPES = {"cbv_pipeline*": C.c_void_p, "cbv_ctx*": C.c_void_p, "int": C.c_int, "size_t": C.c_size_t, "const uint8_t*": C.c_void_p,
          "const double*": C.c_void_p, "uint8_t*": C.c_void_p, "int32_t*": C.POINTER(C.c_int32)}
NEW = ("cbv_pipeline_set_jpeg_planes", "cbv_pipeline_jpeg_planes", "cbv_jpeg_plane_slot_bytes", "cbv_warp_jpeg")


def _declaration(name):
    txt = open(os.path.join(ROOT, "include", "cbv.h")).read()
    m = re.search(r"^CBV_API\s+([\w\s\*]+?)\b%s\s*\(([^)]*)\)\s*;" % name, txt, flags=re.M)
    assert m, "%s is not declared in include/cbv.h" % name
    args = []
    for a in m.group(2).split(","):
        a = " ".join(a.split())
        t = re.match(r"(.*?)(\w+)$", a).group(1).strip().replace(" *", "*")
        args.append(t)
    return m.group(1).strip(), args


@pytest.mark.parametrize("name", NEW)
def test_abi_of_the_new_entry_points(name):
    from chessboard_vision_amd import _native as N
    lib = N.load()
    assert hasattr(lib, name), "libcbv_hip.so does not export %s" % name
    ret, args = _declaration(name)
    fn = getattr(lib, name)
    assert fn.restype is CTYPES[ret]
    assert fn.argtypes is not None and len(fn.argtypes) == len(args), (name, args)
    for have, c in zip(fn.argtypes, args):
        if c == "const cbv_color_profile*":
            assert have._type_ is N.ColorProfile
        else:
            assert have is CTYPES[c] or (CTYPES[c] is C.c_int and have is C.c_int32), (name, c, have)


def test_the_declared_shapes():
    assert _declaration("cbv_pipeline_set_jpeg_planes") == ("int", ["cbv_pipeline*", "int"])
    assert _declaration("cbv_pipeline_jpeg_planes") == ("int", ["cbv_pipeline*"])
    assert _declaration("cbv_jpeg_plane_slot_bytes") == ("size_t", ["int", "int", "int"])
    assert _declaration("cbv_warp_jpeg") == ("int", ["cbv_ctx*", "const uint8_t*", "size_t", "const cbv_color_profile*", "const double*", "int", "int", "int",
                                                    "uint8_t*", "int", "int32_t*"])


def test_planes_names():
    from chessboard_vision_amd import _native as N
    assert N.jpeg_planes_id(False) == 0 and N.jpeg_planes_id(None) == 0 and N.jpeg_planes_id(True) == N.JPEG_PLANES["444"]
    assert [N.jpeg_planes_id(k) for k in ("gray", "420", "422", "444")] == [1, 2, 3, 4]
    for bad in ("411", 3, "yes"):
        with pytest.raises(ValueError):
            N.jpeg_planes_id(bad)
