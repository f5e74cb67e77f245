"""The segments mode of the JPEG entropy decode on the GPU (k_jpeg_pieces with restart intervals as segments) and the
decode depth of the Motion-JPEG ingest: jpeg_decode(entropy="segments") equals the host twin field for field, figures
included (both run the same rounds); the pipeline's frames depend neither on the entropy setting nor on the depth.  Every
stream here has passed the host twin against the serial decode in tests/test_jpeg_segments_host.py, and the damaged ones
(jpeg_segment_cases.gpu_damaged_streams) are the list that file hands, as they are, to the stand-alone program built with
AddressSanitizer and UBSan (tools/jpeg_segments_fuzz_host.cpp --fixed); no seeded or random damage runs on the GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import jpeg_segment_cases as SC  # noqa: E402
import jpeg_streams as JS  # noqa: E402
import ref_jpeg as R  # noqa: E402
from chessboard_vision_amd import synth as S  # noqa: E402

pytestmark = pytest.mark.gpu

LEVELS = ("BGR", "coefficients", "planes")


def assert_gpu_equals_twin(data, p, what):
    from chessboard_vision_amd.board_detection import jpeg_decode
    g = jpeg_decode(data, entropy="segments", piece_bytes=p, stats=True)
    t = jpeg_decode(data, host=True, entropy="segments", piece_bytes=p, stats=True)
    print("%s, pieces of %d bytes: differing BGR %d, coefficients %d, planes %d; status %d / %d; GPU %s, twin %s" % (
        what, p, *(np.count_nonzero(a != b) for a, b in zip(g[:3], t[:3])), g[3], t[3], g[4], t[4]))
    for lvl, a, b in zip(LEVELS, g[:3], t[:3]):
        assert np.array_equal(a, b), "%s: %s" % (what, lvl)
    assert g[3] == t[3], what
    assert g[4] == t[4], what
    return g


@pytest.mark.parametrize("p", (4, 16, 128))
@pytest.mark.parametrize("name", sorted(JS.RESTART_CASES) + ["long-422", "long-420"])
def test_restart_cases_and_long_intervals(gpu_ctx, name, p):
    d = SC.long_stream(name[5:]) if name.startswith("long-") else JS.restart_stream(name)
    g = assert_gpu_equals_twin(d, p, name)
    assert g[3] == 0 and g[4]["pieces"] == sum(SC.piece_counts(d, p)) and np.array_equal(g[0], JS.ref(d)["bgr"])
    if name == "dri-two-waves" and p == 4:
        assert g[4]["pieces"] > 1024  # the workgroup has 1024 lanes: each loops over its (segment, piece) pairs
    if name == "long-422" and p == 4:
        assert g[4]["pieces"] == 1374


@pytest.mark.parametrize("sampling", JS.SAMPLINGS)
def test_every_sampling_with_an_interval_per_mcu(gpu_ctx, sampling):
    d = R.encode_image(JS.scene(17, 23), quality=90, sampling=sampling, dri=1)
    for p in (4, 16):
        g = assert_gpu_equals_twin(d, p, "17x23 %s dri 1" % sampling)
        assert g[3] == 0 and np.array_equal(g[1], JS.ref(d)["coef"])


def test_a_stream_without_dri_is_the_piece_path(gpu_ctx):
    from chessboard_vision_amd.board_detection import jpeg_decode
    d = JS.shape_stream(33, 50, "420")
    g = assert_gpu_equals_twin(d, 4, "33x50 4:2:0 without DRI")
    p = jpeg_decode(d, entropy="pieces", piece_bytes=4, stats=True)
    assert g[4] == p[4] and np.array_equal(g[1], p[1]) and g[3] == p[3] == 0


def test_modes_that_are_refused(gpu_ctx):
    from chessboard_vision_amd import _native as N
    d = np.frombuffer(JS.restart_stream("dri-mcu-row"), np.uint8)
    out = np.zeros((48, 64, 3), np.uint8)
    st = C.c_int32()
    for mode, pb in ((3, 0), (5, 0), (4, 6)):
        assert gpu_ctx.lib.cbv_jpeg_decode_ex(gpu_ctx.h, N.ptr(d), d.size, N.ptr(out), 192, None, None, C.byref(st), mode, pb, None) == -1
    ps = N.JpegDecodeStats()
    gpu_ctx.check(gpu_ctx.lib.cbv_jpeg_decode_ex(gpu_ctx.h, N.ptr(d), d.size, N.ptr(out), 192, None, None, C.byref(st), 4, 0, C.byref(ps)))
    assert ps.pieces == sum(SC.piece_counts(d.tobytes(), 64)) and st.value == 0 and np.array_equal(out, JS.ref(d.tobytes())["bgr"])


def test_damaged_streams_stay_in_bounds_and_a_valid_frame_follows(gpu_ctx):
    """the four recorded damaged streams and the fixed ones of tests/jpeg_segment_cases.py: the twin's bytes, status and figures,
    the guard bytes around every output untouched, and a valid frame decoded afterwards is correct"""
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.board_detection import jpeg_decode, jpeg_probe
    lib = gpu_ctx.lib
    good = SC.long_stream("420")
    cases = list(zip(SC.gpu_damaged_names(), SC.gpu_damaged_streams()))  # the list the sanitizer program has decoded
    assert len(cases) == 12
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
                                             N.JPEG_ENTROPY["segments"], 4, C.byref(ps)))
        tw = jpeg_decode(d, host=True, entropy="segments", piece_bytes=4, stats=True)
        print("%s: status %d (twin %d), %d pieces, %d rounds" % (name, st.value, tw[3], ps.pieces, ps.rounds))
        assert st.value == tw[3] and st.value != 0
        assert (ps.pieces, ps.rounds, ps.settled_round0) == (tw[4]["pieces"], tw[4]["rounds"], tw[4]["settled_round0"])
        assert ps.pieces == sum(SC.piece_counts(data, 4))
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
    """the 16 streams of tests/test_gpu_pipeline_jpeg.py (mixed sampling, with and without DRI), encoded once for all files"""
    import test_gpu_pipeline_jpeg as TP
    assert (TP.W, TP.H, TP.N_FRAMES, TP.MIX) == (W, H, N_FRAMES, MIX)
    return TP.game()[0]


def fill(ring, lengths, slot, data):
    ring[slot, :len(data)] = np.frombuffer(data, np.uint8)
    lengths[slot] = len(data)


def run_game(streams, mode="auto", piece_bytes=0, depth=None, depth_first=False):
    """the 16 frames through a pipeline with the setting; (pipeline, (ring bytes, status, stats, results))"""
    from chessboard_vision_amd.stream import BoardPipeline
    n = N_FRAMES
    p = BoardPipeline(W, H, n)
    p.configure(S.scaled_corners(W, H), profile=S.SHIPPED_PROFILE, chunk=4, lanes=2, enhance=False)
    if depth is not None and depth_first:
        p.set_jpeg_depth(depth)
    p.set_input_format("mjpeg")
    p.set_jpeg_entropy(mode, piece_bytes)
    if depth is not None and not depth_first:
        p.set_jpeg_depth(depth)
    ring, lengths = p.host_ring(), p.jpeg_lengths()
    for i in range(n):
        fill(ring, lengths, i, streams[i])
    p.submit(0, 10)
    p.submit(10, 6)
    p.run(0, 10)
    p.run(10, 6)
    out = [p.download(0, i).tobytes() for i in range(n)], p.jpeg_status(0, n).tolist(), p.jpeg_stats(0, n), bytes(p.results(0, n))
    return p, out


def test_pipeline_frames_do_not_depend_on_the_entropy_setting(gpu_ctx):
    streams = game()
    n = N_FRAMES
    dri = np.array([MIX[i % len(MIX)][1] != 0 for i in range(n)])
    p, by_interval = run_game(streams, "interval")
    p.close()
    assert not by_interval[2].any() and not any(by_interval[1])
    p, auto = run_game(streams, "auto")
    p.close()
    p, seg = run_game(streams, "segments")
    for i in range(n):
        assert seg[0][i] == by_interval[0][i] == auto[0][i], "slot %d differs between the entropy paths" % i
    assert seg[1] == by_interval[1] == auto[1] and seg[3] == by_interval[3] == auto[3]
    print("segments: pieces, rounds, settled in round 0 per slot:", seg[2].tolist())
    assert (seg[2][:, 0] > 0).all(), "under segments every frame goes the piece path"
    assert ((auto[2][:, 0] > 0) == ~dri).all(), "under auto, pieces > 0 exactly on the frames without DRI"
    for i in range(n):
        want = SC.piece_counts(streams[i], 64)
        assert seg[2][i, 0] == sum(want) and 1 <= seg[2][i, 1] <= max(want) and len(want) <= seg[2][i, 2] <= sum(want), i
        if not dri[i]:
            assert (seg[2][i] == auto[2][i]).all(), i
    # the synchronous path takes the setting too
    p.upload(1, streams[12], fmt="mjpeg")
    assert p.download(0, 1).tobytes() == by_interval[0][12] and (p.jpeg_stats(1, 1)[0] == seg[2][12]).all()
    p.close()


def test_pipeline_frames_do_not_depend_on_the_depth(gpu_ctx):
    """depth 3 leaves a short last chunk in the submit of 10 (3 + 3 + 3 + 1; the submit of 6 is 3 + 3), depth 16 decodes each submit
    in one launch, depth 1 a frame at a time"""
    streams = game()
    n = N_FRAMES
    p, default = run_game(streams, "segments")
    assert p.jpeg_depth == 8
    p.close()
    for depth, first in ((1, False), (3, False), (16, False), (3, True)):
        p, got = run_game(streams, "segments", depth=depth, depth_first=first)
        assert p.jpeg_depth == depth  # (set before the format, it holds afterwards)
        for i in range(n):
            assert got[0][i] == default[0][i], "slot %d at depth %d" % (i, depth)
        assert got[1] == default[1] and (got[2] == default[2]).all() and got[3] == default[3], depth
        if depth == 3 and not first:  # a submit refused for a bad slot still enqueues nothing
            p.wait_submitted()
            ring, lengths = p.host_ring(), p.jpeg_lengths()
            for i in range(7):
                fill(ring, lengths, i, streams[8 + i])
            prog = bytearray(streams[13])
            prog[prog.index(b"\xff\xc0") + 1] = 0xC2
            fill(ring, lengths, 5, bytes(prog))
            with pytest.raises(RuntimeError, match=r"slot 5.*progressive.*code -5"):
                p.submit(0, 7)
            p.wait_submitted()
            for i in range(7):
                assert p.download(0, i).tobytes() == default[0][i], "slot %d was written by a refused submit" % i
            assert (p.jpeg_stats(0, 7) == default[2][:7]).all()
        p.close()
    p, auto_default = run_game(streams, "auto")
    p.close()
    p, auto_1 = run_game(streams, "auto", depth=1)
    p.close()
    assert auto_1[0] == auto_default[0] == default[0] and auto_1[1] == auto_default[1] and (auto_1[2] == auto_default[2]).all()


def test_depths_that_are_refused(gpu_ctx):
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, 2)
    p.configure(S.scaled_corners(W, H), enhance=False)
    b = p.add_board(S.scaled_corners(W, H))
    lib = gpu_ctx.lib
    assert lib.cbv_pipeline_set_jpeg_depth(p.h_, 0) == -1 and lib.cbv_pipeline_set_jpeg_depth(p.h_, 65) == -1
    assert lib.cbv_pipeline_set_jpeg_depth(b.h_, 4) == -4 and lib.cbv_pipeline_jpeg_depth(b.h_) == -4
    assert lib.cbv_pipeline_set_jpeg_entropy(p.h_, 3, 0) == -1 and lib.cbv_pipeline_set_jpeg_entropy(p.h_, 5, 0) == -1
    assert p.jpeg_depth == 8
    p.set_jpeg_depth(64)
    assert p.jpeg_depth == 64
    with pytest.raises(RuntimeError, match="code -1"):
        p.set_jpeg_depth(65)
    assert p.jpeg_depth == 64
    p.close()


def test_one_1080p_frame_with_an_interval_per_mcu_row_equals_the_twin(gpu_ctx):
    """68 restart intervals of about 16 KB each at the default piece size"""
    from chessboard_vision_amd.board_detection import jpeg_decode
    img, d = JS.frame_1080p()
    assert R.parse(d)["dri"] == 120
    g = jpeg_decode(d, entropy="segments", stats=True)
    t = jpeg_decode(d, host=True, entropy="segments", stats=True)
    print("1080p, 68 intervals: %d bytes of stream, status %d / %d, GPU %s, twin %s" % (len(d), g[3], t[3], g[4], t[4]))
    assert g[3] == t[3] == 0 and g[4] == t[4] and g[4]["pieces"] == sum(SC.piece_counts(d, 64)) > 1024
    assert np.array_equal(g[1], t[1]) and np.array_equal(g[2], t[2]) and np.array_equal(g[0], t[0])
    s = jpeg_decode(d, host=True, entropy="interval")
    assert np.array_equal(s[1], t[1]) and np.array_equal(s[0], t[0])
