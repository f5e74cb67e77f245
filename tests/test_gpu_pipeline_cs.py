"""The colour space of a pipeline's YUV input (BoardPipeline.set_input_format(fmt, colorspace=...); include/cbv.h, CBV_CS_*):
a pipeline fed raw frames through the pinned ring and `submit` against a pipeline fed the BGR frames the int64 restatement
(tests/ref64_yuv_cs.py) makes of the same bytes.  640 x 480 (color_sweep_ref's frames and corners), a dozen frames of the
lilac stream with moves in them, turned into NV12 / BT.709 and YUYV / BT.601 full-range inputs by the restatement's forward
transform.  Everything a board reports must be identical: results, NoiseHandler records, square statistics, HoughCircles."""
import functools

import numpy as np
import pytest

import color_sweep_ref as CS
import ref64_yuv_cs as RC
from chessboard_vision_amd import synth as S

pytestmark = pytest.mark.gpu

W, H, N = CS.W, CS.H, 12
PTS = S.scaled_corners(W, H)
PAL, PROFILE = "lilac", CS.PROFILES["radical_lilac"]
CASES = (("nv12", "bt709"), ("yuyv", "bt601-full"))
MODES = {"raw": dict(enhance=False), "profile_raw": dict(enhance="profile", raw=True)}


@functools.lru_cache(maxsize=None)
def _inputs(fmt, cs):
    """(raw frames in the layout and colour space, the BGR frames the restatement makes of them)"""
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, N)
    p.synth(0, N, scene=CS.native_scene(PAL), frames_per_ply=CS.FRAMES_PER_PLY)
    bgr = [p.download(0, i) for i in range(N)]
    p.close()
    raw = [RC.from_bgr(f, fmt, cs) for f in bgr]
    conv = [np.ascontiguousarray(RC.to_bgr(f, fmt, cs)) for f in raw]
    for a in raw + conv:
        a.setflags(write=False)
    return raw, conv


def _pipeline(fmt, cs, frames, **mode):
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, N)
    p.configure(PTS, profile=PROFILE, chunk=4, lanes=2, **mode)
    if fmt == "bgr":
        for i, f in enumerate(frames):
            p.upload(i, f)
        return p
    p.set_input_format(fmt, colorspace=cs)
    assert (p.input_format, p.input_colorspace) == (fmt, cs)
    ring = p.host_ring()
    for i, f in enumerate(frames):
        ring[i] = f
    p.submit(0, 8)
    p.submit(8, N - 8)
    return p


def _snapshot(p):
    return (bytes(p.results(0, N)), [(st.name, sorted(d.items(), key=str)) for st, d in p.noise_results(0, N)],
            [bytes(p.square_stats(i)) for i in range(N)], [bytes(p.hough(i)) for i in range(N)], [p.download(2, i).tobytes() for i in range(N)])


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s" % c)
def test_raw_mode_equals_the_bgr_fed_pipeline(gpu_ctx, case, mode):
    fmt, cs = case
    raw, conv = _inputs(fmt, cs)
    ref = _pipeline("bgr", "bt601", conv, **MODES[mode])
    ref.run(0, N)
    want = _snapshot(ref)
    ref.close()
    assert len(set(want[4])) > 1   # the boards differ from frame to frame: moves are in them
    p = _pipeline(fmt, cs, raw, **MODES[mode])
    p.run(0, N)
    got = _snapshot(p)
    for name, g, w_ in zip(("results", "noise_results", "square_stats", "hough", "boards"), got, want):
        assert g == w_, (fmt, cs, mode, name)
    # the frame itself, converted on demand from the raw ring
    for i in (0, N - 1):
        assert np.array_equal(p.download(0, i), conv[i]), (fmt, cs, mode, i)
    p.close()
    # the colour space matters: the same bytes read as BT.601 limited range give other boards
    q = _pipeline(fmt, "bt601", raw, **MODES[mode])
    q.run(0, N)
    assert q.download(2, 0).tobytes() != want[4][0]
    q.close()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s" % c)
def test_enhancement_on_the_submitted_slots_are_the_restatement(gpu_ctx, case):
    fmt, cs = case
    raw, conv = _inputs(fmt, cs)
    p = _pipeline(fmt, cs, raw, enhance=True)
    p.run(0, N)
    for i in range(N):
        assert np.array_equal(p.download(0, i), conv[i]), (fmt, cs, i)
    ref = _pipeline("bgr", "bt601", conv, enhance=True)
    ref.run(0, N)
    assert _snapshot(p) == _snapshot(ref)
    # ... and upload(fmt=, colorspace=) converts into the BGR ring in the frame's own colour space
    p.upload(3, raw[5], fmt=fmt, colorspace=cs)
    assert np.array_equal(p.download(0, 3), conv[5])
    other = "bt709-full"
    p.upload(3, raw[5], fmt=fmt, colorspace=other)
    assert np.array_equal(p.download(0, 3), RC.to_bgr(raw[5], fmt, other))
    ref.close()
    p.close()


def test_color_sweep_on_the_raw_ring(gpu_ctx):
    import piece_sweep_ref as PS
    fmt, cs = CASES[0]
    raw, conv = _inputs(fmt, cs)
    profs = [CS.PROFILES[n] for n in ("none", "shipped", "radical_lilac", "sat3")]
    exp = CS.expected_bits(8)
    p = _pipeline(fmt, cs, raw, **MODES["profile_raw"])
    ref = _pipeline("bgr", "bt601", conv, **MODES["profile_raw"])
    got, want = p.color_sweep(0, 8, profs, expected=exp), ref.color_sweep(0, 8, profs, expected=exp)
    assert PS.same_records(got.records, want.records) and got.summary.tobytes() == want.summary.tobytes()
    assert np.array_equal(got.raw_occupied, want.raw_occupied) and np.array_equal(got.hough, want.hough)
    ref.close()
    p.close()


def test_a_raw_ring_refuses_a_frame_in_another_colour_space(gpu_ctx):
    fmt, cs = CASES[0]
    raw, conv = _inputs(fmt, cs)
    p = _pipeline(fmt, cs, raw, **MODES["raw"])
    with pytest.raises(RuntimeError, match=r"code -4\b"):
        p.upload(0, raw[0], fmt=fmt, colorspace="bt601")
    with pytest.raises(RuntimeError, match=r"code -4\b"):
        p.upload(0, raw[0], fmt=fmt)
    with pytest.raises(RuntimeError, match=r"code -4\b"):
        p.upload(0, raw[0], fmt=fmt, colorspace="bt709-full")
    p.upload(0, raw[1], fmt=fmt, colorspace=cs)   # its own: stored as it is
    assert np.array_equal(p.download(0, 0), conv[1])
    p.close()
