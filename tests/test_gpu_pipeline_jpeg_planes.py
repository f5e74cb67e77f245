"""The planes mode of the Motion-JPEG ingest (set_input_format("mjpeg", planes=...), cbv_pipeline_set_jpeg_planes): on a
pipeline without enhancement the decode stops at the planes and the warp samples the plane ring (k_warp_jpeg,
k_warp_jpeg_profile), and everything the pipeline computes is, bit for bit, what the same pipeline with planes off computes,
whose decode fills the BGR ring.  640 x 480, 16 frames of mixed sampling and restart interval; ordering against runs in
flight; refused slots; slots never written; one 1080p frame."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import color_sweep_ref as CS  # noqa: E402
import jpeg_streams as JS  # noqa: E402
import piece_sweep_ref as PS  # noqa: E402
import ref_jpeg as R  # noqa: E402
from chessboard_vision_amd import synth as S  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, N_FRAMES = 640, 480, 16
# sampling and restart interval per slot: mixed within every chunk of 8 frames
MIX = [("420", 0), ("422", 0), ("444", 0), ("gray", 0), ("420", 40), ("422", 1), ("444", 80), ("420", 7)]
ARG, STATE, UNSUPPORTED = -1, -4, -5
MODES = {"plain": dict(enhance=False), "profile_raw": dict(enhance="profile", raw=True)}


@functools.lru_cache(maxsize=None)
def game():
    """16 frames of the synthetic scene as JPEG streams (mixed sampling and DRI), and the host twin's decode of each"""
    from chessboard_vision_amd.board_detection import jpeg_decode
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, N_FRAMES)
    p.synth(0, N_FRAMES, scene="normal", frames_per_ply=2)
    frames = [p.download(0, i) for i in range(N_FRAMES)]
    p.close()
    streams, bgr = [], []
    for i, f in enumerate(frames):
        sampling, dri = MIX[i % len(MIX)]
        d = R.encode_image(f, quality=90 if i % 3 else 75, sampling=sampling, dri=dri)
        out = jpeg_decode(d, host=True)
        assert out[3] == 0
        out[0].setflags(write=False)
        streams.append(d)
        bgr.append(out[0])
    return streams, bgr


def everything(p, n):
    return [bytes(p.results(0, n)), repr(p.noise_results(0, n))] + [bytes(p.square_stats(i)) for i in range(n)] + \
           [p.download(2, i).tobytes() for i in range(n)]


def fill(ring, lengths, slot, data):
    ring[slot, :len(data)] = np.frombuffer(data, np.uint8)
    lengths[slot] = len(data)


def make(planes, n=N_FRAMES, depth=None, chunk=8, **mode):
    """chunks of 8: a run of 10 frames is a chunk of 8 (the warp's many-frames form) and one of 2 (its one-frame form)"""
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, n)
    p.configure(S.scaled_corners(W, H), profile=S.SHIPPED_PROFILE, chunk=chunk, lanes=2, **mode)
    if depth is not None:
        p.set_jpeg_depth(depth)
    p.set_input_format("mjpeg", planes=planes)
    return p


def feed(p, streams, n=N_FRAMES):
    """submit in two parts (a whole chunk of 8 and a part of one, then the rest), then the runs"""
    ring, lengths = p.host_ring(), p.jpeg_lengths()
    ring[:] = 0xA5
    for i in range(n):
        fill(ring, lengths, i, streams[i])
    cut = min(10, n - 1)
    p.submit(0, cut)
    p.submit(cut, n - cut)
    p.run(0, cut)
    p.run(cut, n - cut)


@functools.lru_cache(maxsize=None)
def planes_off(mode):
    """everything of the planes-off pipeline in a mode: the parent's path"""
    streams, _ = game()
    p = make(False, **MODES[mode])
    assert p.jpeg_planes == "off" and p.frames_ptr()
    feed(p, streams)
    out = everything(p, N_FRAMES)
    p.close()
    return out


@pytest.mark.parametrize("mode", sorted(MODES))
def test_planes_on_equals_planes_off(gpu_ctx, mode):
    streams, bgr = game()
    n = N_FRAMES
    today = planes_off(mode)
    p = make(True, **MODES[mode])
    assert p.jpeg_planes == "444"
    assert not p.frames_ptr(), "the pipeline still holds a BGR ring"
    feed(p, streams)
    assert not p.jpeg_status(0, n).any()
    for i in range(n):
        assert np.array_equal(p.download(0, i), bgr[i]), "slot %d differs from the twin's decode" % i
    got = everything(p, n)
    assert got[0] == today[0], "results"
    assert got == today
    # the synchronous path, in another order of samplings per slot than the ring last held
    p.reset_state()
    for i in range(n):
        p.upload(i, streams[(i + 3) % n], fmt="mjpeg")
    for i in range(n):
        p.upload(i, streams[i], fmt="mjpeg")
    p.run(0, 10)
    p.run(10, 6)
    assert not p.jpeg_status(0, n).any()
    assert everything(p, n) == today
    # the entry points that write BGR frames have nothing to write into
    with pytest.raises(RuntimeError, match="planes mode"):
        p.upload(0, np.zeros((H, W, 3), np.uint8))
    with pytest.raises(RuntimeError, match="planes mode"):
        p.synth(0, 1)
    with pytest.raises(RuntimeError, match="planes mode"):
        p.upload(0, np.zeros((H * 3 // 2, W), np.uint8), fmt="nv12")
    p.close()


def test_with_enhancement_the_mode_has_no_effect(gpu_ctx):
    streams, bgr = game()
    n = 8
    outs = []
    for planes in (False, True):
        p = make(planes, n=n, enhance=True)
        assert p.frames_ptr()
        feed(p, streams, n)
        outs.append(everything(p, n) + [p.download(0, i).tobytes() for i in range(n)])
        p.close()
    assert outs[0] == outs[1]
    for mode in (dict(enhance="profile"),):  # the profile mode without raw: the BGR ring too
        p = make(True, n=n, **mode)
        assert p.frames_ptr()
        feed(p, streams, n)
        assert np.array_equal(p.download(0, 3), bgr[3])
        p.close()


def test_two_boards_with_a_profile_each(gpu_ctx):
    streams, _ = game()
    n = 8
    snaps = []
    for planes in (False, True):
        p = make(planes, n=n, enhance="profile", raw=True)
        b = p.add_board(S.scaled_corners(W, H) + np.float32(3), rot180=True, display_size=(800, 600), profile=CS.PROFILES["sat3"])
        feed(p, streams, n)
        snaps.append(everything(p, n) + everything(b, n))
        b.set_profile(CS.PROFILES["radical"])
        p.run(0, n)
        snaps[-1] += [b.download(2, i).tobytes() for i in range(n)]
        p.close()
    assert snaps[0] == snaps[1]


def test_color_sweep_gives_the_records_of_the_planes_off_pipeline(gpu_ctx):
    streams, _ = game()
    profs = [CS.SHIPPED, CS.PROFILES["sat3"], CS.PROFILES["radical"]]
    got = []
    for planes in (False, True):
        p = make(planes, n=4, enhance="profile", raw=True)
        ring, lengths = p.host_ring(), p.jpeg_lengths()
        for i in range(4):
            fill(ring, lengths, i, streams[i])
        p.submit(0, 4)
        p.wait_submitted()
        res = p.color_sweep(0, 4, profs)
        got.append((res.records, res.summary.tobytes()))
        p.close()
    assert PS.same_records(got[0][0], got[1][0]) and got[0][1] == got[1][1]
    assert got[1][0].shape[:2] == (3, 4)


def test_color_sweep_with_the_many_frames_form(gpu_ctx):
    """8 frames a chunk: the profile kernel's many-frames form"""
    streams, _ = game()
    profs = [CS.SHIPPED, CS.PROFILES["radical"]]
    got = []
    for planes in (False, True):
        p = make(planes, n=8, enhance="profile", raw=True)
        for i in range(8):
            p.upload(i, streams[i], fmt="mjpeg")
        res = p.color_sweep(0, 8, profs, chunk_frames=8)
        got.append((res.records, res.summary.tobytes()))
        p.close()
    assert PS.same_records(got[0][0], got[1][0]) and got[0][1] == got[1][1]


@pytest.mark.parametrize("depth", [1, 3, None], ids=["depth1", "depth3", "default"])
def test_every_depth(gpu_ctx, depth):
    streams, bgr = game()
    p = make(True, depth=depth, chunk=4 if depth == 3 else 16, enhance=False)
    feed(p, streams)
    assert everything(p, N_FRAMES) == planes_off("plain")
    assert np.array_equal(p.download(0, 13), bgr[13])
    p.close()


def test_the_420_mode_refuses_a_422_slot(gpu_ctx):
    from chessboard_vision_amd.board_detection import jpeg_probe
    from chessboard_vision_amd.stream import jpeg_plane_slot_bytes
    streams, bgr = game()
    # slot sizes: what the mode's largest admitted sampling needs
    assert jpeg_plane_slot_bytes(W, H, "420") == (jpeg_probe(streams[0])["plane_elems"] + 255) // 256 * 256 == W * H * 3 // 2
    p = make("420", n=4, enhance=False)
    assert p.jpeg_planes == "420" and not p.frames_ptr()
    ring, lengths = p.host_ring(), p.jpeg_lengths()
    first = [streams[0], streams[3], streams[4], streams[7]]  # 4:2:0, gray, 4:2:0, 4:2:0
    for i in range(4):
        fill(ring, lengths, i, first[i])
    p.submit(0, 4)
    p.wait_submitted()
    before = [p.download(0, i) for i in range(4)]
    second = [streams[8], streams[1], streams[11], streams[12]]  # slot 1 is 4:2:2
    for i in range(4):
        fill(ring, lengths, i, second[i])
    with pytest.raises(RuntimeError, match=r"slot 1.*4:2:2.*code -5"):
        p.submit(0, 4)
    fill(ring, lengths, 1, streams[2])  # 4:4:4
    with pytest.raises(RuntimeError, match=r"slot 1.*4:4:4.*code -5"):
        p.submit(0, 4)
    with pytest.raises(RuntimeError, match=r"4:2:2.*code -5"):
        p.upload(2, streams[5], fmt="mjpeg")
    p.wait_submitted()
    for i in range(4):
        assert np.array_equal(p.download(0, i), before[i]), "slot %d was written by a refused submit" % i
    for repl, want in ((streams[3], bgr[3]), (streams[15], bgr[15])):  # a gray stream, a 4:2:0 stream
        fill(ring, lengths, 1, repl)
        p.submit(0, 4)
        p.wait_submitted()
        assert np.array_equal(p.download(0, 1), want) and np.array_equal(p.download(0, 0), bgr[8])
    p.run(0, 4)
    assert p.download(2, 1).any()
    p.close()
    # with the BGR ring (enhancement on) the refusal is the same: a later configure cannot meet a slot it cannot hold
    p = make("420", n=2, enhance=True)
    ring, lengths = p.host_ring(), p.jpeg_lengths()
    fill(ring, lengths, 0, streams[0])
    fill(ring, lengths, 1, streams[1])
    with pytest.raises(RuntimeError, match=r"slot 1.*4:2:2.*code -5"):
        p.submit(0, 2)
    p.close()


def test_mode_before_the_format_board_handles_and_unknown_modes(gpu_ctx):
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.stream import BoardPipeline
    lib = gpu_ctx.lib
    streams, bgr = game()
    p = BoardPipeline(W, H, 2)
    p.configure(S.scaled_corners(W, H), enhance=False)
    assert lib.cbv_pipeline_jpeg_planes(p.h_) == 0 and p.frames_ptr()
    assert lib.cbv_pipeline_set_jpeg_planes(p.h_, N.JPEG_PLANES["422"]) == 0  # only stored
    assert p.jpeg_planes == "422" and p.frames_ptr()
    for bad in (-1, 5, 77):
        assert lib.cbv_pipeline_set_jpeg_planes(p.h_, bad) == ARG
        assert p.jpeg_planes == "422"
    assert lib.cbv_pipeline_set_input_format(p.h_, N.FMT_MJPEG) == 0
    p.input_format = "mjpeg"
    assert p.jpeg_planes == "422" and not p.frames_ptr()
    b = p.add_board(S.scaled_corners(W, H) + np.float32(2))
    assert lib.cbv_pipeline_set_jpeg_planes(b.h_, 1) == STATE and lib.cbv_pipeline_jpeg_planes(b.h_) == STATE
    assert p.jpeg_planes == "422"
    p.upload(0, streams[1], fmt="mjpeg")
    assert np.array_equal(p.download(0, 0), bgr[1])
    # off again: the BGR ring is back and the decode fills it
    p.set_input_format("mjpeg")
    assert p.jpeg_planes == "off" and p.frames_ptr()
    p.upload(0, streams[2], fmt="mjpeg")
    assert np.array_equal(p.download(0, 0), bgr[2])
    with pytest.raises(ValueError):
        p.set_input_format("nv12", planes=True)
    with pytest.raises(ValueError):
        p.set_input_format("mjpeg", planes="411")
    p.close()


def test_a_slot_never_written_is_a_black_frame(gpu_ctx):
    streams, bgr = game()
    p = make("420", n=4, enhance=False)
    p.upload(2, streams[0], fmt="mjpeg")
    p.run(0, 4)
    for i in (0, 1, 3):
        assert not p.download(0, i).any() and not p.download(2, i).any()
    assert np.array_equal(p.download(0, 2), bgr[0]) and p.download(2, 2).any()
    p.close()
    # through a profile: what the planes-off pipeline makes of black frames
    black = np.zeros((H, W, 3), np.uint8)
    outs = []
    for planes in (False, "gray"):
        p = make(planes, n=2, **MODES["profile_raw"])
        if not planes:
            p.upload(0, black)
            p.upload(1, black)
        p.run(0, 2)
        outs.append([bytes(p.results(0, 2))] + [p.download(2, i).tobytes() for i in range(2)] + [p.download(0, i).tobytes() for i in range(2)])
        p.close()
    assert outs[0] == outs[1]


def test_one_1080p_frame(gpu_ctx):
    from chessboard_vision_amd.board_detection import jpeg_decode
    from chessboard_vision_amd.stream import BoardPipeline
    img, d = JS.frame_1080p()
    outs = []
    for planes in (False, True):
        p = BoardPipeline(1920, 1080, 2)
        p.configure(S.scaled_corners(1920, 1080), enhance=False)
        p.set_input_format("mjpeg", slot_bytes=len(d), planes=planes)
        ring, lengths = p.host_ring(), p.jpeg_lengths()
        fill(ring, lengths, 1, d)
        p.submit(1, 1)
        p.run(1, 1)
        outs.append([bytes(p.results(1, 1)), bytes(p.square_stats(1)), p.download(2, 1).tobytes(), p.download(0, 1).tobytes()])
        assert p.jpeg_status(1, 1)[0] == 0
        p.close()
    assert outs[0] == outs[1]
    assert outs[1][3] == jpeg_decode(d, host=True)[0].tobytes()


def test_a_slot_rewritten_while_a_run_is_in_flight(gpu_ctx):
    """the rewritten slots get another sampling (4:2:0 to 4:4:4, 4:2:0 to gray): the run in flight reads the planes and the
    descriptors it was enqueued on, the next run the new ones"""
    streams, bgr = game()
    n = 8
    assert MIX[0][0] == MIX[4][0] == "420" and MIX[10 % 8][0] == "444" and MIX[11 % 8][0] == "gray"

    def fed(planes, which):
        p = make(planes, n=n, enhance=False)
        ring, lengths = p.host_ring(), p.jpeg_lengths()
        for i in range(n):
            fill(ring, lengths, i, streams[which[i]])
        p.submit(0, n)
        return p, ring, lengths

    old, new = list(range(n)), [10, 1, 2, 3, 11, 5, 6, 7]
    ref = fed(False, old)[0]
    ref.run(0, n)
    want = bytes(ref.results(0, n))
    ref.close()
    ref = fed(False, new)[0]
    ref.run(0, n)
    want_new = [ref.download(2, i).tobytes() for i in range(n)]
    ref.close()

    p, ring, lengths = fed(True, old)
    p.run(0, n)              # in flight
    p.wait_submitted()       # the copies have left the host ring: it may be rewritten
    fill(ring, lengths, 0, streams[10])
    fill(ring, lengths, 4, streams[11])
    p.submit(0, 1)           # waits for the run that still reads the planes and the descriptors
    p.submit(4, 1)
    assert bytes(p.results(0, n)) == want, "the run in flight saw a rewritten slot"
    p.run(0, n)
    assert [p.download(2, i).tobytes() for i in range(n)] == want_new, "the next run did not see the new frames"
    assert np.array_equal(p.download(0, 0), bgr[10]) and np.array_equal(p.download(0, 4), bgr[11]) and np.array_equal(p.download(0, 3), bgr[3])
    p.close()


@functools.lru_cache(maxsize=None)
def small_game():
    """13 frames of the synthetic scene at 322 x 242 (no multiple of an MCU) as JPEG streams, the samplings mixed"""
    from chessboard_vision_amd.stream import BoardPipeline
    w, h, n = 322, 242, 13
    p = BoardPipeline(w, h, n)
    p.synth(0, n, scene="normal", frames_per_ply=2)
    frames = [p.download(0, i) for i in range(n)]
    p.close()
    return [R.encode_image(f, quality=90, sampling=MIX[i % len(MIX)][0], dri=MIX[i % len(MIX)][1]) for i, f in enumerate(frames)]


@pytest.mark.parametrize("lens", [False, True], ids=["lens_free", "lens"])
@pytest.mark.parametrize("attached", [0, 1], ids=["1board", "2boards"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_short_last_group_and_taps_outside(gpu_ctx, mode, attached, lens):
    """the warp from the planes where the runs above do not take it: a quad whose right and top parts leave the 322 x 242
    frame, in one run of 11 frames in one chunk (plain: groups of four frames per thread and a last one of three; with a
    profile: five groups of two and a last one of one) and then in a run of 2 frames (one frame per thread), with one board
    and with two (the second smaller, rotated, with a profile of its own), lens-free and through a lens (the table-driven
    kernel), against the planes-off pipeline, whose decode fills the BGR ring"""
    import ref_lens as RL
    from chessboard_vision_amd.stream import BoardPipeline, Lens
    w, h, n = 322, 242, 13
    quad = S.scaled_corners(w, h) + np.float32([0.42 * w, -0.3 * h])
    assert (quad[:, 0] > w).any() and (quad[:, 1] < 0).any()
    streams = small_game()
    outs = []
    for planes in (False, True):
        p = BoardPipeline(w, h, n)
        p.configure(quad, profile=S.SHIPPED_PROFILE, chunk=11, lanes=1, lens=Lens(*(RL.BARREL[:2] + (w / 2, h / 2) + RL.BARREL[4:])) if lens else None,
                    **MODES[mode])
        p.set_input_format("mjpeg", planes=planes)
        assert bool(p.frames_ptr()) == (not planes)
        boards = [p]
        if attached:
            own = dict(profile=CS.PROFILES["sat3"]) if mode == "profile_raw" else {}
            boards.append(p.add_board(quad + np.float32(3), rot180=True, display_size=(800, 600), margin=100, **own))
        for i in range(n):
            p.upload(i, streams[i], fmt="mjpeg")
        p.run(0, 11)
        p.run(11, 2)
        assert not p.jpeg_status(0, n).any()
        outs.append([b.download(2, i) for b in boards for i in range(n)])
        p.close()
    assert len(outs[0]) == n * (1 + attached)
    for k, (off, on) in enumerate(zip(*outs)):
        assert np.array_equal(off, on), (mode, attached, lens, k, int((off != on).sum()))
        black = (~on.any(2)).mean()  # the part of the board that lies outside the frame
        assert 0.05 < black < 0.9, (k, black)
