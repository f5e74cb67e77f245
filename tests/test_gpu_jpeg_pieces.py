"""The piece path of the JPEG entropy decode on the GPU (k_jpeg_pieces): jpeg_decode(entropy="pieces") equals the host twin at
coefficient, plane, BGR and status level and reports the twin's figures (both run the same rounds), at piece sizes from 4
bytes up; the pipeline's frames do not depend on the entropy setting.  Every stream here has passed the host twin against
the serial decode in tests/test_jpeg_pieces_host.py; no random garbage runs on the GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import jpeg_piece_cases as PC  # noqa: E402
import jpeg_streams as JS  # noqa: E402
import ref_jpeg as R  # noqa: E402
from chessboard_vision_amd import synth as S  # noqa: E402

pytestmark = pytest.mark.gpu

LEVELS = ("BGR", "coefficients", "planes")


def assert_gpu_equals_twin(data, p, what):
    from chessboard_vision_amd.board_detection import jpeg_decode
    g = jpeg_decode(data, entropy="pieces", piece_bytes=p, stats=True)
    t = jpeg_decode(data, host=True, entropy="pieces", piece_bytes=p, stats=True)
    print("%s, pieces of %d bytes: differing BGR %d, coefficients %d, planes %d; status %d / %d; GPU %s, twin %s" % (
        what, p, *(np.count_nonzero(a != b) for a, b in zip(g[:3], t[:3])), g[3], t[3], g[4], t[4]))
    for lvl, a, b in zip(LEVELS, g[:3], t[:3]):
        assert np.array_equal(a, b), "%s: %s" % (what, lvl)
    assert g[3] == t[3], what
    assert g[4] == t[4], what
    return g


@pytest.mark.parametrize("p", (4, 16, 128))
@pytest.mark.parametrize("sampling", JS.SAMPLINGS)
@pytest.mark.parametrize("w,h", JS.SHAPES)
def test_shapes(gpu_ctx, w, h, sampling, p):
    d = JS.shape_stream(w, h, sampling)
    g = assert_gpu_equals_twin(d, p, "%dx%d %s" % (w, h, sampling))
    assert g[3] == 0 and g[4]["pieces"] == -(-len(JS.entropy_of(d)) // p) and np.array_equal(g[0], JS.ref(d)["bgr"])


@pytest.mark.parametrize("name", JS.SPECIAL)
def test_streams_from_the_coefficient_encoder(gpu_ctx, name):
    d = JS.special_stream(name)
    g = assert_gpu_equals_twin(d, 4, name)
    assert g[3] == 0 and np.array_equal(g[1], JS.ref(d)["coef"])


@pytest.mark.parametrize("name", PC.BOUNDARY + (PC.SLOW,))
def test_boundary_cases(gpu_ctx, name):
    g = assert_gpu_equals_twin(PC.boundary_case(name), 4, name)
    assert 1 <= g[4]["rounds"] <= g[4]["pieces"]


def test_more_pieces_than_lanes_and_a_dc_scan_over_three_components(gpu_ctx):
    d = PC.no_dri_picture(96, 56, "420")
    g = assert_gpu_equals_twin(d, 4, "96x56 4:2:0")
    assert g[4]["pieces"] > 1024 and g[3] == 0  # the workgroup has 1024 lanes: each loops over its pieces
    assert np.array_equal(g[0], JS.ref(d)["bgr"])
    d = PC.no_dri_picture(17, 23, "422")
    for p in (4, 16):
        g = assert_gpu_equals_twin(d, p, "17x23 4:2:2")
        assert np.array_equal(g[1], JS.ref(d)["coef"])


def test_modes_and_sizes_that_are_refused(gpu_ctx):
    from chessboard_vision_amd import _native as N
    d = np.frombuffer(JS.shape_stream(8, 8, "444"), np.uint8)
    out = np.zeros((8, 8, 3), np.uint8)
    st = C.c_int32()
    for mode, pb in ((3, 0), (2, 6), (2, 2)):
        assert gpu_ctx.lib.cbv_jpeg_decode_ex(gpu_ctx.h, N.ptr(d), d.size, N.ptr(out), 24, None, None, C.byref(st), mode, pb, None) == -1
    ps = N.JpegDecodeStats()
    gpu_ctx.check(gpu_ctx.lib.cbv_jpeg_decode_ex(gpu_ctx.h, N.ptr(d), d.size, N.ptr(out), 24, None, None, C.byref(st), 1, 0, C.byref(ps)))
    assert (ps.pieces, ps.rounds, ps.settled_round0) == (0, 0, 0) and np.array_equal(out, JS.ref(d.tobytes())["bgr"])


def _no_dri(d):
    i = d.index(b"\xff\xdd\x00\x04")
    return d[:i] + d[i + 6:]


def test_damaged_streams_stay_in_bounds_and_a_valid_frame_follows(gpu_ctx):
    """the four fixed damaged streams, as they are (DRI: the interval path) and without their DRI segment (the piece path; the
    first restart marker then ends the data), and the damaged boundary cases: the twin's bytes and status, the guard bytes
    behind every output untouched, and a valid frame decoded afterwards is correct"""
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.board_detection import jpeg_decode, jpeg_probe
    lib = gpu_ctx.lib
    good = PC.no_dri_picture(64, 48, "422", 5)
    cases = [(n, JS.damaged_stream(n)) for n in sorted(JS.DAMAGED)] + [(n + " without DRI", _no_dri(JS.damaged_stream(n))) for n in sorted(JS.DAMAGED)]
    cases += [(n, PC.boundary_case(n)) for n in ("ends-in-first-piece", "stray-eoi-in-the-middle", "ends-in-last-piece", "bad-code-in-the-middle")]
    for name, data in cases:
        d = np.frombuffer(data, np.uint8)
        info = jpeg_probe(d)
        w, h, n = info["w"], info["h"], info["plane_elems"]
        G = 4096
        bgr = np.full(h * w * 3 + 2 * G, 0xA5, np.uint8)
        coef = np.full(n + 2 * G, 0x5A5A, np.int16)
        planes = np.full(n + 2 * G, 0xA5, np.uint8)
        st = C.c_int32(-1)
        ps = N.JpegDecodeStats()
        gpu_ctx.check(lib.cbv_jpeg_decode_ex(gpu_ctx.h, N.ptr(d), d.size, N.ptr(bgr[G:]), w * 3, N.ptr(coef[G:]), N.ptr(planes[G:]), C.byref(st),
                                             N.JPEG_ENTROPY["pieces"], 4, C.byref(ps)))
        tw = jpeg_decode(d, host=True, entropy="pieces", piece_bytes=4, stats=True)
        print("%s: status %d (twin %d), %d pieces, %d rounds" % (name, st.value, tw[3], ps.pieces, ps.rounds))
        assert st.value == tw[3] and st.value != 0
        assert (ps.pieces, ps.rounds, ps.settled_round0) == (tw[4]["pieces"], tw[4]["rounds"], tw[4]["settled_round0"])
        assert (ps.pieces == 0) == (info["restart_interval"] != 0)
        assert np.array_equal(coef[G:G + n], tw[1]) and np.array_equal(planes[G:G + n], tw[2])
        assert np.array_equal(bgr[G:G + h * w * 3].reshape(h, w, 3), tw[0])
        for a, size, v in ((bgr, h * w * 3, 0xA5), (coef, n, 0x5A5A), (planes, n, 0xA5)):
            assert (a[:G] == v).all() and (a[G + size:] == v).all(), "guard bytes were written"
        assert_gpu_equals_twin(good, 4, "the valid frame after " + name)


# ---------------------------------------------------------------------------------------------------------------------
# the pipeline (the settings of tests/test_gpu_pipeline_jpeg.py)
# ---------------------------------------------------------------------------------------------------------------------
W, H, N_FRAMES = 640, 480, 16
MIX = [("420", 0), ("422", 0), ("444", 0), ("gray", 0), ("420", 40), ("422", 1), ("444", 80), ("420", 7)]


def game():
    """the 16 streams of tests/test_gpu_pipeline_jpeg.py (mixed sampling, with and without DRI), encoded once for both files"""
    import test_gpu_pipeline_jpeg as TP
    assert (TP.W, TP.H, TP.N_FRAMES, TP.MIX) == (W, H, N_FRAMES, MIX)
    return TP.game()[0]


def fill(ring, lengths, slot, data):
    ring[slot, :len(data)] = np.frombuffer(data, np.uint8)
    lengths[slot] = len(data)


def test_pipeline_frames_do_not_depend_on_the_entropy_setting(gpu_ctx):
    from chessboard_vision_amd.stream import BoardPipeline
    streams = game()
    n = N_FRAMES
    dri = np.array([MIX[i % len(MIX)][1] != 0 for i in range(n)])

    def run(mode, piece_bytes):
        p = BoardPipeline(W, H, n)
        p.configure(S.scaled_corners(W, H), profile=S.SHIPPED_PROFILE, chunk=4, lanes=2, enhance=False)
        p.set_input_format("mjpeg")
        p.set_jpeg_entropy(mode, piece_bytes)
        ring, lengths = p.host_ring(), p.jpeg_lengths()
        for i in range(n):
            fill(ring, lengths, i, streams[i])
        p.submit(0, 10)  # a whole chunk of 8 and a part of one: both kinds of frame in every launch
        p.submit(10, 6)
        p.run(0, 10)
        p.run(10, 6)
        out = [p.download(0, i).tobytes() for i in range(n)], p.jpeg_status(0, n).tolist(), p.jpeg_stats(0, n), bytes(p.results(0, n))
        return p, out

    p, by_interval = run("interval", 0)
    p.close()
    assert not by_interval[2].any() and not any(by_interval[1])
    p, by_piece = run("pieces", 64)
    for i in range(n):
        assert by_piece[0][i] == by_interval[0][i], "slot %d differs between the entropy paths" % i
    assert by_piece[1] == by_interval[1] and by_piece[3] == by_interval[3]
    stats = by_piece[2]
    print("pieces, rounds, settled in round 0 per slot:", stats.tolist())
    assert ((stats[:, 0] > 0) == ~dri).all(), "pieces > 0 exactly on the frames without DRI"
    for i in np.flatnonzero(~dri):
        assert stats[i, 0] == -(-len(JS.entropy_of(streams[i])) // 64) and 1 <= stats[i, 1] <= stats[i, 0] and 1 <= stats[i, 2] <= stats[i, 0]
    # a refused slot still enqueues nothing
    p.wait_submitted()
    ring, lengths = p.host_ring(), p.jpeg_lengths()
    for i in range(4):
        fill(ring, lengths, i, streams[8 + i])
    prog = bytearray(streams[10])
    prog[prog.index(b"\xff\xc0") + 1] = 0xC2
    fill(ring, lengths, 2, bytes(prog))
    with pytest.raises(RuntimeError, match=r"slot 2.*progressive.*code -5"):
        p.submit(0, 4)
    p.wait_submitted()
    for i in range(4):
        assert p.download(0, i).tobytes() == by_interval[0][i], "slot %d was written by a refused submit" % i
    assert (p.jpeg_stats(0, 4) == stats[:4]).all()
    # the synchronous path takes the setting too, and AUTO is the piece path at the default size
    p.upload(1, streams[9], fmt="mjpeg")
    assert p.download(0, 1).tobytes() == by_interval[0][9] and p.jpeg_stats(1, 1)[0, 0] == stats[9, 0]
    p.set_jpeg_entropy("auto")
    fill(ring, lengths, 2, streams[10])
    p.submit(0, 4)
    p.wait_submitted()
    assert [p.download(0, i).tobytes() for i in range(4)] == by_interval[0][8:12]
    auto = p.jpeg_stats(0, 4)
    assert auto[2, 0] == -(-len(JS.entropy_of(streams[10])) // 64) and auto[0, 0] == -(-len(JS.entropy_of(streams[8])) // 64)
    p.close()


def test_set_jpeg_entropy_on_a_board_handle_is_a_state_error(gpu_ctx):
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, 2)
    p.configure(S.scaled_corners(W, H), enhance=False)
    b = p.add_board(S.scaled_corners(W, H))
    assert gpu_ctx.lib.cbv_pipeline_set_jpeg_entropy(b.h_, 2, 64) == -4
    out = np.zeros((1, 3), np.uint32)
    from chessboard_vision_amd import _native as N
    assert gpu_ctx.lib.cbv_pipeline_jpeg_stats(b.h_, 0, 1, N.ptr(out)) == -4
    assert gpu_ctx.lib.cbv_pipeline_set_jpeg_entropy(p.h_, 2, 6) == -1
    p.close()


def test_one_1080p_frame_without_dri_equals_the_twin(gpu_ctx):
    """jpeg_streams.frame_1080p()'s picture encoded without DRI: one scan of about a megabyte, thousands of pieces at the default size"""
    from chessboard_vision_amd.board_detection import jpeg_decode
    img, _ = JS.frame_1080p()
    d = R.encode_image(img, quality=90, sampling="422")
    assert R.parse(d)["dri"] == 0
    g = jpeg_decode(d, stats=True)  # AUTO, the default piece size
    t = jpeg_decode(d, host=True, stats=True)
    print("1080p without DRI: %d bytes of stream, status %d / %d, GPU %s, twin %s" % (len(d), g[3], t[3], g[4], t[4]))
    assert g[3] == t[3] == 0 and g[4] == t[4] and g[4]["pieces"] > 1024
    assert np.array_equal(g[1], t[1]) and np.array_equal(g[2], t[2]) and np.array_equal(g[0], t[0])
    s = jpeg_decode(d, host=True, entropy="interval")
    assert np.array_equal(s[1], t[1]) and np.array_equal(s[0], t[0])
    assert np.abs(g[0].astype(int) - img).mean() < 20
