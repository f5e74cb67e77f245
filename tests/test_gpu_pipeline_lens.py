"""The camera's lens on the device-resident pipeline (cbv_pipeline_set_lens; BoardPipeline.configure(lens=...), set_lens):
the warped boards against tests/ref_lens.py, the numpy restatement of include/cbv.h's definition, byte for byte, in every
mode the pipeline warps in; enhance_region's footprint through the lens; switching the lens off; the colour sweep's scratch
warps; the refusals; and a lens-free pipeline, which must compute what it computed before the lens kernels existed.
256 x 192 frames, boards of 100 and 72 pixels (two 64-wide blocks, the second partial), batches of 1 (one frame per
thread) and 9 (four per thread, or two with a raw profile, and a partial last group)."""
import functools

import numpy as np
import pytest

import ref_jpeg as RJ
import ref_lens as R
from chessboard_vision_amd import synth as S
from helpers import random_frame

pytestmark = pytest.mark.gpu

W, H = 256, 192
CLICKED = [(40, 30), (215, 25), (30, 170), (225, 165)]    # board 0, as clicked in the delivered frame; 100 x 100
CLICKED_2 = [(70, 45), (190, 40), (60, 150), (200, 158)]  # the attached board; 72 x 72, rotated
SIZE_100, SIZE_72 = dict(display_size=(200, 200), margin=100), dict(display_size=(172, 172), margin=100)
MODES = ["enhanced", "plain", "profile", "nv12", "bayer_rggb", "nv12_profile", "mjpeg_planes"]
STATE, ARG = -4, -1


def _lens(t=R.BARREL):
    from chessboard_vision_amd.stream import Lens
    return Lens(*t)


@functools.lru_cache(maxsize=None)
def _bgr(i):
    f = random_frame(W, H, 100 + i)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _inputs(mode, i):
    """(what upload takes, its fmt, the BGR frame the warp is defined on: the product's own conversion of it)"""
    from chessboard_vision_amd.board_detection import bayer_to_bgr, jpeg_to_bgr, yuv_to_bgr
    import raw_profile_ref as RP
    if mode.startswith("nv12"):
        raw = RP.from_bgr(_bgr(i), "nv12")
        return raw, "nv12", yuv_to_bgr(raw, "nv12")
    if mode == "bayer_rggb":
        raw = RP.from_bgr(_bgr(i), "bayer_rggb")
        return raw, "bayer_rggb", bayer_to_bgr(raw, "bayer_rggb")
    if mode == "mjpeg_planes":
        data = RJ.encode_image(_bgr(i), quality=90, sampling=("420", "422", "444")[i % 3])
        return data, "mjpeg", jpeg_to_bgr(data)
    return _bgr(i), "bgr", _bgr(i)


def _configure(p, mode, lens, **kw):
    cfg = dict(chunk=16, lanes=1, **SIZE_100)
    cfg.update(kw)
    if mode == "enhanced":
        p.configure(CLICKED, profile=S.SHIPPED_PROFILE, lens=lens, **cfg)
    elif mode in ("profile", "nv12_profile"):
        p.configure(CLICKED, profile=S.SHIPPED_PROFILE, enhance="profile", raw=mode == "nv12_profile", lens=lens, **cfg)
    else:
        p.configure(CLICKED, enhance=False, lens=lens, **cfg)
    if mode.startswith("nv12") or mode == "bayer_rggb":
        p.set_input_format(mode.split("_profile")[0])
    if mode == "mjpeg_planes":
        p.set_input_format("mjpeg", planes=True)


def _pipeline(mode, n, lens, two_boards=False, **kw):
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(W, H, n)
    _configure(p, mode, lens, **kw)
    boards = [p]
    if two_boards:
        boards.append(p.add_board(CLICKED_2, rot180=True, **SIZE_72))
    for i in range(n):
        img, fmt, _ = _inputs(mode, i)
        p.upload(i, img, fmt=fmt)
    return p, boards


@functools.lru_cache(maxsize=None)
def _sources(mode, n):
    """the BGR frames the warp's bytes are defined on, per slot"""
    from chessboard_vision_amd import _native as N
    from chessboard_vision_amd.stream import BoardPipeline
    if mode == "enhanced":  # the enhanced, normalised frames of a lens-free pipeline that keeps them
        q = BoardPipeline(W, H, n)
        q.configure(CLICKED, profile=S.SHIPPED_PROFILE, keep_enhanced=True, chunk=16, lanes=1, **SIZE_100)
        for i in range(n):
            q.upload(i, _bgr(i))
        q.run(0, n)
        out = [q.download(1, i) for i in range(n)]
        q.close()
        return out
    out = []
    ctx = N.context()
    for i in range(n):
        f = np.ascontiguousarray(_inputs(mode, i)[2])
        if mode in ("profile", "nv12_profile"):
            g = np.empty_like(f)
            ctx.check(ctx.lib.cbv_apply_color_profile(ctx.h, N.ptr(f), W, H, f.strides[0], N.ColorProfile.from_dict(S.SHIPPED_PROFILE), N.ptr(g), g.strides[0]))
            f = g
        out.append(f)
    return out


def _everything(boards, n):
    return [(bytes(b.results(0, n)), [bytes(b.square_stats(i)) for i in range(n)], [b.download(2, i).tobytes() for i in range(n)]) for b in boards]


@pytest.mark.parametrize("two_boards", [False, True], ids=["one_board", "two_boards"])
@pytest.mark.parametrize("n", [1, 9])
@pytest.mark.parametrize("mode", MODES)
def test_warped_boards_equal_the_definition(gpu_ctx, mode, n, two_boards):
    p, boards = _pipeline(mode, n, _lens(), two_boards)
    p.run(0, n)
    src = _sources(mode, n)
    for b, rot in zip(boards, (False, True)):
        for i in range(n):
            want = R.warp(src[i], R.BARREL, b.matrix, b.board_size, b.board_size, rot)
            got = b.download(2, i)
            assert np.array_equal(got, want), (mode, n, b.board_size, i, int((got != want).sum()))
    p.close()


def test_the_points_are_taken_as_clicked_in_the_delivered_frame(gpu_ctx):
    """configure and add_board undistort their points with the pipeline's lens: the matrices are the ideal-coordinate ones"""
    from chessboard_vision_amd.board_detection import get_perspective_transform, undistort_points
    p, boards = _pipeline("plain", 1, _lens(R.PINCUSHION), True)
    for b, pts in zip(boards, (CLICKED, CLICKED_2)):
        s = b.board_size
        want = get_perspective_transform(np.float32(undistort_points(pts, _lens(R.PINCUSHION))), np.float32([[0, 0], [s, 0], [0, s], [s, s]]))
        assert np.array_equal(b.matrix, want)
    p.close()


def test_enhance_region_follows_the_lens(gpu_ctx):
    """region-limited enhancement with the lens: the bytes and results of the same run without the region"""
    n = 9
    whole, wb = _pipeline("enhanced", n, _lens(), True)
    whole.run(0, n)
    want = _everything(wb, n)
    whole.close()
    part, pb = _pipeline("enhanced", n, _lens(), True, enhance_region=True)
    part.run(0, n)
    assert _everything(pb, n) == want
    part.close()


@pytest.mark.parametrize("mode", ["enhanced", "plain", "nv12_profile"])
def test_set_lens_none_restores_the_lens_free_pipeline(gpu_ctx, mode):
    """...and a lens-free pipeline computes what it does with the feature compiled in but unused: the same launchers, the
    same kernels.  The matrices are those of the lens-free configuration in all three pipelines."""
    n = 9
    never, nb = _pipeline(mode, n, None, True)
    never.run(0, n)
    want = _everything(nb, n)
    never.close()
    p, boards = _pipeline(mode, n, None, True)
    p.set_lens(_lens())
    p.run(0, n)
    with_lens = _everything(boards, n)
    assert with_lens[0][2] != want[0][2] and with_lens[1][2] != want[1][2]  # the lens is on: other bytes on both boards
    p.set_lens(None)
    for b in boards:
        b.reset_state()
    p.run(0, n)
    assert _everything(boards, n) == want
    p.close()


def test_a_board_handle_and_a_bad_lens_are_refused_with_the_state_untouched(gpu_ctx):
    n = 2
    p, boards = _pipeline("plain", n, _lens(), True)
    p.run(0, n)
    want = _everything(boards, n)
    lib = gpu_ctx.lib
    assert lib.cbv_pipeline_set_lens(boards[1].h_, _lens(R.PINCUSHION).struct()) == STATE
    assert lib.cbv_pipeline_set_lens(None, _lens().struct()) == ARG
    for field, bad in (("fx", 0.0), ("fy", -1.0), ("k1", float("nan")), ("cy", float("inf"))):
        s = _lens(R.PINCUSHION).struct()
        setattr(s, field, bad)
        assert lib.cbv_pipeline_set_lens(p.h_, s) == ARG, field
    for b in boards:
        b.reset_state()
    p.run(0, n)
    assert _everything(boards, n) == want  # still the barrel lens
    p.close()


def test_color_sweep_with_the_pipelines_profile_reports_what_the_run_reports(gpu_ctx):
    """the sweep's scratch warps go through the lens too: the single profile the pipeline runs under, every square
    checked, gives the run's raw and smoothed occupancy (640 x 480 synthetic frames, 8 of them)"""
    from chessboard_vision_amd.stream import BoardPipeline
    w, h, n = 640, 480, 8
    lens = _lens((500.0, 500.0, 320.0, 240.0) + R.BARREL[4:])
    all_squares = {(f, r) for f in range(8) for r in range(8)}
    for raw in (False, True):
        p = BoardPipeline(w, h, n)
        p.configure(S.scaled_corners(w, h), profile=S.SHIPPED_PROFILE, enhance="profile", raw=raw, use_hough=2, chunk=8, lanes=1, lens=lens)
        p.synth(0, n, scene="dim", frames_per_ply=2)
        frames = [p.download(0, i) for i in range(n)]
        if raw:
            import raw_profile_ref as RP
            p.set_input_format("nv12")
            for i in range(n):
                p.upload(i, RP.from_bgr(frames[i], "nv12"), fmt="nv12")
        p.reset_state()
        p.set_check_squares(0, [all_squares] * n)
        p.run(0, n)
        out = p.results(0, n)
        res = p.color_sweep(0, n, [S.SHIPPED_PROFILE])
        for i in range(n):
            assert (out[i].raw_occupied, out[i].stable_occupied) == (int(res.raw_occupied[0, i]), int(res.stable_occupied[0, i])), (raw, i)
        assert any(out[i].raw_occupied for i in range(n))  # the frames show pieces
        p.close()


# --- every raw layout in the many-frames forms ---------------------------------------------------------------------------------
RAW_W, RAW_H, RAW_N = 322, 242, 13


@functools.lru_cache(maxsize=None)
def _raw_game(fmt):
    """13 frames of a scripted game in the raw layout (inputs), and the BGR frames the restatement makes of them (the
    reference pipeline's input)"""
    import raw_profile_ref as RP
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(RAW_W, RAW_H, RAW_N)
    p.synth(0, RAW_N, frames_per_ply=2)
    raw = [RP.from_bgr(p.download(0, i), fmt) for i in range(RAW_N)]
    p.close()
    return raw, [np.ascontiguousarray(RP.to_bgr(f, fmt)) for f in raw]


def _raw_boards(fmt, frames, profile, lens):
    """the warped boards of two boards of a pipeline fed `frames` in `fmt`: one run of 11 frames in one chunk, then one of 2"""
    import color_sweep_ref as CS
    from chessboard_vision_amd.stream import BoardPipeline
    quad = S.scaled_corners(RAW_W, RAW_H) + np.float32([0.42 * RAW_W, -0.3 * RAW_H])
    assert (quad[:, 0] > RAW_W).any() and (quad[:, 1] < 0).any()
    kw = dict(enhance="profile", raw=True) if profile else dict(enhance=False)
    p = BoardPipeline(RAW_W, RAW_H, RAW_N)
    p.configure(quad, profile=CS.PROFILES["radical"], chunk=11, lanes=1, lens=_lens(R.BARREL[:2] + (RAW_W / 2, RAW_H / 2) + R.BARREL[4:]) if lens else None, **kw)
    b = p.add_board(quad + np.float32(3), rot180=True, display_size=(800, 600), margin=100, **(dict(profile=CS.SHIPPED) if profile else {}))
    if fmt != "bgr":
        p.set_input_format(fmt)
    for i, f in enumerate(frames):
        p.upload(i, f, fmt=fmt)
    p.run(0, 11)
    p.run(11, 2)
    out = [x.download(2, i) for x in (p, b) for i in range(RAW_N)]
    p.close()
    return out


@pytest.mark.parametrize("lens", [False, True], ids=["lens_free", "lens"])
@pytest.mark.parametrize("profile", [False, True], ids=["plain", "profile"])
@pytest.mark.parametrize("fmt", ["nv12", "nv21", "yuv420p", "yv12", "yuyv", "yvyu", "uyvy", "bayer_rggb", "bayer_bggr", "bayer_grbg", "bayer_gbrg"])
def test_every_raw_layout_short_last_group_and_taps_outside(gpu_ctx, fmt, profile, lens):
    """the warp from raw frames of every layout, with a colour profile and without, lens-free and through the lens, where the
    tests of the layouts do not take it: two boards (the second smaller and rotated) whose quads leave the 322 x 242 frame
    to the right and at the top, one run of 11 frames in one chunk (groups of four frames per thread and a last one of three;
    where the form takes two frames per thread, five groups and a last one of one) and a run of 2 frames (one frame per
    thread), against the same pipeline fed the BGR frames that the restatement makes of the raw ones"""
    raw, bgr = _raw_game(fmt)
    got = _raw_boards(fmt, raw, profile, lens)
    want = _raw_boards("bgr", bgr, profile, lens)
    assert len(got) == 2 * RAW_N
    for k, (g, w_) in enumerate(zip(got, want)):
        assert np.array_equal(g, w_), (fmt, profile, lens, k, int((g != w_).sum()))
        black = (~g.any(2)).mean()  # the part of the board that lies outside the frame
        assert 0.05 < black < 0.9, (k, black)
