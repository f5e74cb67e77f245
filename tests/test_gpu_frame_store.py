"""Where a pipeline's frames live, pinned from outside ("Where the frames live"): one pipeline is walked through
input formats, planes modes, configurations and the Motion-JPEG setters, and after every step it must look like the table
says and compute, byte for byte, what a fresh pipeline created directly in that state computes from the same bytes.

The table (configuration kinds E = enhancement, S1 = enhance=False, P = enhance="profile", PR = ... with raw=True; format
classes B = bgr, Y = a YUV or Bayer layout, J0 = mjpeg with planes off, J1 = mjpeg in a planes mode):
  the frames are raw (the warp reads the raw ring or the plane ring)   under S1 and PR with Y or J1
  there is no BGR ring (frames_ptr() is null)                          under PR with Y, under S1 and PR with J1
  upload of BGR / synth / upload of a foreign format are refused       where the frames are raw
  a host slot has                                                      w h 3 bytes (B), the packed raw frame (Y), the
                                                                       Motion-JPEG slot bytes (J0, J1), rounded to 256
  a run before any ingest                                              is refused on a raw ring that was never made (Y);
                                                                       reads black frames from a new plane ring (J1)
320 x 240, 4 slots, chunks of 2 on 2 lanes: the smallest size at which the Bayer and pipeline tests run whole chains."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref64_bayer as RB  # noqa: E402
import ref64_yuv as RY  # noqa: E402
import ref_jpeg as R  # noqa: E402
from chessboard_vision_amd import synth as S  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, N = 320, 240, 4
KINDS = {"E": dict(enhance=True), "S1": dict(enhance=False), "P": dict(enhance="profile"), "PR": dict(enhance="profile", raw=True)}
SAMPLINGS = ("gray", "420", "422", "444")  # the stream of frame i; the 4:2:0 one has a restart interval
BAYER = "bayer_rggb"
JPEG_DEFAULT_SLOT = ((W * H + 1) // 2 + 255) // 256 * 256


def r256(n):
    return (n + 255) // 256 * 256


@functools.lru_cache(maxsize=None)
def inputs():
    """four frames of the synthetic scene, downloaded once from a BGR pipeline, in every format of the walks"""
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, N)
    p.synth(0, N, scene="normal", frames_per_ply=2)
    bgr = [p.download(0, i) for i in range(N)]
    p.close()
    out = {"bgr": bgr, "nv12": [RY.bgr_to_nv12(f) for f in bgr], BAYER: [RB.mosaic(f, BAYER) for f in bgr],
           "mjpeg": [R.encode_image(f, quality=75, sampling=s, dri=7 if s == "420" else 0) for f, s in zip(bgr, SAMPLINGS)]}
    assert all(len(d) <= JPEG_DEFAULT_SLOT for d in out["mjpeg"])
    for fmt in ("bgr", "nv12", BAYER):
        for a in out[fmt]:
            a.setflags(write=False)
    return out


def fed(fmt, planes):
    """what slot i is fed in a state: frame i in the format; a 4:2:0 plane ring is fed the gray and the 4:2:0 stream twice"""
    data = inputs()[fmt]
    return [data[i % 2] for i in range(N)] if fmt == "mjpeg" and planes == "420" else list(data)


def expect(kind, fmt, planes):
    """the table"""
    raw_kind, y, j1 = kind in ("S1", "PR"), fmt in ("nv12", BAYER), fmt == "mjpeg" and bool(planes)
    return dict(raw=raw_kind and (y or j1), planes=raw_kind and j1, bgr_ring=not ((kind == "PR" and y) or (raw_kind and j1)),
                slot={"bgr": r256(W * H * 3), "nv12": r256(W * H * 3 // 2), BAYER: r256(W * H), "mjpeg": JPEG_DEFAULT_SLOT}[fmt])


def everything(p):
    return [bytes(p.results(0, N)), repr(p.noise_results(0, N))] + [bytes(p.square_stats(i)) for i in range(N)] + \
           [p.download(2, i).tobytes() for i in range(N)] + [p.download(0, i).tobytes() for i in range(N)]


def ingest_and_run(p, fmt, planes):
    """slots 0-2 by submit, slot 3 by upload, one run of the four"""
    data = fed(fmt, planes)
    p.reset_state()
    ring = p.host_ring()
    for i in range(3):
        if fmt == "mjpeg":
            ring[i, :len(data[i])] = np.frombuffer(data[i], np.uint8)
            p.jpeg_lengths()[i] = len(data[i])
        else:
            ring[i] = data[i]
    p.submit(0, 3)
    p.upload(3, data[3], fmt=fmt)
    p.run(0, N)
    return everything(p)


def configure(p, kind):
    p.configure(S.scaled_corners(W, H), profile=S.SHIPPED_PROFILE, chunk=2, lanes=2, **KINDS[kind])


@functools.lru_cache(maxsize=None)
def fresh(kind, fmt, planes):
    """everything of a pipeline created directly in the state and fed the same bytes"""
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, N)
    configure(p, kind)
    if fmt == "mjpeg":
        p.set_input_format(fmt, planes=planes)
    elif fmt != "bgr":
        p.set_input_format(fmt)
    out = ingest_and_run(p, fmt, planes)
    p.close()
    return out


RAW_Y = r"the pipeline runs without enhancement on a YUV or Bayer input format \(raw mode\): its frames are the raw ring"
RAW_J = r"the pipeline runs without enhancement on Motion-JPEG input in planes mode \(raw mode\): its frames are the decoded planes"


def check_step(p, lib, kind, fmt, planes, before_ingest=None, slot=None):
    """before_ingest: "refused" (no raw ring was made since the format changed), "black" (the plane ring is new) or None"""
    what = (kind, fmt, planes)
    e = expect(kind, fmt, planes)
    assert bool(p.frames_ptr()) == e["bgr_ring"], what                                    # 1
    assert lib.cbv_pipeline_host_slot_bytes(p.h_) == (slot or e["slot"]), what            # 2
    foreign = ("nv12", inputs()["nv12"][0]) if fmt != "nv12" else (BAYER, inputs()[BAYER][0])
    writers = (lambda: p.upload(0, inputs()["bgr"][0]), lambda: p.synth(0, 1), lambda: p.upload(0, foreign[1], fmt=foreign[0]))
    if e["raw"]:                                                                          # 3
        msg = RAW_J if e["planes"] else RAW_Y
        for fn, pat in zip(writers, ("cbv_pipeline_upload: " + msg, "cbv_pipeline_synth: " + msg,
                                     r"cbv_pipeline_upload_raw: format \d+, but " + msg + ("" if e["planes"] else r".* \(format \d+\)"))):
            with pytest.raises(RuntimeError, match=pat):
                fn()
    else:
        for fn in writers:
            fn()
    if before_ingest == "refused":                                                        # 4
        assert e["raw"] and not e["planes"]
        with pytest.raises(RuntimeError, match="cbv_pipeline_run: no raw frame was ever uploaded or submitted"):
            p.run(0, N)
        with pytest.raises(RuntimeError, match="cbv_pipeline_download: no raw frame was ever uploaded or submitted"):
            p.download(0, 0)
    elif before_ingest == "black":
        assert e["planes"]
        p.run(0, N)
        assert all(not p.download(0, i).any() for i in range(N)), what
        assert len({p.download(2, i).tobytes() for i in range(N)}) == 1 and len({bytes(p.square_stats(i)) for i in range(N)}) == 1, what
    got = ingest_and_run(p, fmt, planes)                                                  # 5
    want = fresh(kind, fmt, planes)
    assert got[0] == want[0], what + ("results",)
    assert got == want, what


def walk_formats(gpu_ctx, kind):
    from chessboard_vision_amd.stream import BoardPipeline
    lib = gpu_ctx.lib
    p = BoardPipeline(W, H, N)
    configure(p, kind)
    check_step(p, lib, kind, "bgr", False)
    p.set_input_format("nv12")
    check_step(p, lib, kind, "nv12", False, "refused")
    p.set_input_format(BAYER)
    check_step(p, lib, kind, BAYER, False, "refused")
    p.set_input_format("mjpeg")
    check_step(p, lib, kind, "mjpeg", False)
    p.set_input_format("mjpeg", planes="420")
    check_step(p, lib, kind, "mjpeg", "420", "black")
    # a 4:2:2 stream is refused by both ingest paths and leaves the slots untouched
    before = [p.download(0, i) for i in range(N)]
    s422 = inputs()["mjpeg"][2]
    ring, lengths = p.host_ring(), p.jpeg_lengths()
    ring[1, :len(s422)] = np.frombuffer(s422, np.uint8)
    lengths[1] = len(s422)
    with pytest.raises(RuntimeError, match=r"cbv_pipeline_submit: slot 1: a 4:2:2 frame, the plane ring's slots hold up to 4:2:0.*code -5"):
        p.submit(0, 2)
    with pytest.raises(RuntimeError, match=r"cbv_pipeline_upload_jpeg: slot 2: a 4:2:2 frame.*code -5"):
        p.upload(2, s422, fmt="mjpeg")
    p.wait_submitted()
    for i in range(N):
        assert np.array_equal(p.download(0, i), before[i]), "slot %d was written by a refused stream" % i
    p.set_input_format("mjpeg", planes="444")
    check_step(p, lib, kind, "mjpeg", "444", "black")
    p.set_input_format("nv12")
    check_step(p, lib, kind, "nv12", False, "refused")
    p.set_input_format("bgr")
    check_step(p, lib, kind, "bgr", False)
    p.close()


def test_walk_the_formats_without_enhancement(gpu_ctx):
    walk_formats(gpu_ctx, "S1")


def test_walk_the_formats_with_a_profile_on_raw_frames(gpu_ctx):
    walk_formats(gpu_ctx, "PR")


def test_walk_the_configurations_with_the_format_held(gpu_ctx):
    from chessboard_vision_amd.stream import BoardPipeline
    lib = gpu_ctx.lib
    p = BoardPipeline(W, H, N)
    configure(p, "E")
    p.set_input_format("mjpeg", planes="444")
    # the plane ring comes with the format and is idle under E and P: S1 finds it new, PR finds S1's frames in it
    for kind, before in (("E", None), ("S1", "black"), ("PR", None), ("P", None), ("E", None)):
        configure(p, kind)
        check_step(p, lib, kind, "mjpeg", "444", before)
    p.set_input_format("nv12")
    for kind in ("E", "S1", "PR", "P", "E"):  # (the raw ring is made by E's ingest and stays: no configuration frees it)
        configure(p, kind)
        check_step(p, lib, kind, "nv12", False)
    p.close()


def test_the_motion_jpeg_setters_between_submits(gpu_ctx):
    from chessboard_vision_amd import _native as Nat
    from chessboard_vision_amd.stream import BoardPipeline
    lib = gpu_ctx.lib
    p = BoardPipeline(W, H, N)
    configure(p, "S1")
    assert lib.cbv_pipeline_set_jpeg_planes(p.h_, Nat.JPEG_PLANES["444"]) == 0  # before the format: only stored
    assert p.jpeg_planes == "444" and p.frames_ptr() and lib.cbv_pipeline_host_slot_bytes(p.h_) == r256(W * H * 3)
    assert lib.cbv_pipeline_set_input_format(p.h_, Nat.FMT_MJPEG) == 0
    p.input_format = "mjpeg"
    check_step(p, lib, "S1", "mjpeg", "444", "black")
    p.set_jpeg_depth(1)
    check_step(p, lib, "S1", "mjpeg", "444")
    p.set_jpeg_depth(3)
    p.set_jpeg_entropy("segments")
    check_step(p, lib, "S1", "mjpeg", "444")
    assert lib.cbv_pipeline_set_jpeg_slot_bytes(p.h_, 65537) == 0  # frees both ingest rings; the plane ring keeps its frames
    assert [p.download(0, i).tobytes() for i in range(N)] == fresh("S1", "mjpeg", "444")[-N:]
    check_step(p, lib, "S1", "mjpeg", "444", slot=65792)
    p.set_jpeg_entropy("auto", 32)
    check_step(p, lib, "S1", "mjpeg", "444", slot=65792)
    # a submit still in flight when the next setter is called: its decode lands in the plane ring before the scratch goes
    data = fed("mjpeg", "444")
    ring, lengths = p.host_ring(), p.jpeg_lengths()
    for i, j in enumerate((3, 2, 1)):  # other frames than the slots hold
        ring[i, :len(data[j])] = np.frombuffer(data[j], np.uint8)
        lengths[i] = len(data[j])
    p.submit(0, 3)
    p.set_jpeg_depth(2)
    assert p.jpeg_depth == 2 and not p.jpeg_status(0, N).any()
    want = fresh("S1", "mjpeg", "444")[-N:]
    assert [p.download(0, i).tobytes() for i in range(N)] == [want[3], want[2], want[1], want[3]]
    check_step(p, lib, "S1", "mjpeg", "444", slot=65792)
    p.close()
