"""The warp of YUV frames in the colour spaces beside cv2's BT.601 limited range (k_warp_cs.hip, k_warp_lens_cs.hip): the
fused call on the raw frame must equal, byte for byte, the int64 conversion of tests/ref64_yuv_cs.py followed by the
product's BGR call of the same kind, which is pinned elsewhere (plain, with a colour profile, through a lens, both).
Single-frame calls on a 32 x 24 source warped to 40 x 40: the destination is no multiple of the 64-column block, and the
matrix puts taps outside the frame on all four sides and on odd and even source rows and columns.  The pipeline cases run
the kernels the single-frame calls do not: the many-frames-per-thread forms (batch 9: two groups of four and a short one;
planar 4:2:0 and the lens-profile forms take groups of two) and the _mb kernels of two boards."""
import functools

import numpy as np
import pytest

import color_sweep_ref as CS
import ref64_yuv_cs as RC
import ref_lens as RL
from chessboard_vision_amd import synth as S

pytestmark = pytest.mark.gpu

W, H, DEST = 32, 24, (40, 40)
QUAD = [[-3.4, -2.3], [34.6, -3.1], [-2.2, 26.4], [35.3, 25.7]]   # the board's corners in the frame: outside it on every side
LENS = (40.0, 40.0, 16.0, 12.0) + RL.BARREL[4:]                   # ref_lens's barrel coefficients on a 32 x 24 frame
PROFILES = {"none": None, "shipped": CS.SHIPPED, "radical": CS.PROFILES["radical"]}
PW, PH, N9 = 322, 242, 9


def _lens(t=LENS):
    from chessboard_vision_amd.stream import Lens
    return Lens(*t)


def _matrix():
    from chessboard_vision_amd.board_detection import get_perspective_transform
    return get_perspective_transform(np.float32(QUAD), np.float32([[0, 0], [DEST[0], 0], [0, DEST[1]], [DEST[0], DEST[1]]]))


def test_the_case_is_what_the_docstring_says():
    """taps outside the frame on all four sides, and inside it on odd and even rows and columns"""
    Minv = np.linalg.inv(np.asarray(_matrix(), np.float64))
    yy, xx = np.mgrid[0:DEST[1], 0:DEST[0]].astype(np.float64)
    den = Minv[2, 0] * xx + Minv[2, 1] * yy + Minv[2, 2]
    sx = np.floor((Minv[0, 0] * xx + Minv[0, 1] * yy + Minv[0, 2]) / den).astype(int)
    sy = np.floor((Minv[1, 0] * xx + Minv[1, 1] * yy + Minv[1, 2]) / den).astype(int)
    assert (sx < 0).any() and (sx + 1 >= W).any() and (sy < 0).any() and (sy + 1 >= H).any()
    inside = (sx >= 0) & (sx + 1 < W) & (sy >= 0) & (sy + 1 < H)
    assert {(int(a) & 1, int(b) & 1) for a, b in zip(sx[inside], sy[inside])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert DEST[0] % 64 and DEST[1] % 16


@pytest.mark.parametrize("fmt", RC.LAYOUTS)
@pytest.mark.parametrize("cs", RC.NEW)
def test_single_frame_calls_equal_conversion_then_the_bgr_call(gpu_ctx, fmt, cs):
    from chessboard_vision_amd.board_detection import warp_image_profiled, warp_lens, warp_perspective, warp_perspective_profiled
    M = _matrix()
    raw = RC.noise(W, H, fmt, 11 + RC.LAYOUTS.index(fmt))
    bgr = RC.to_bgr(raw, fmt, cs)
    assert np.array_equal(warp_perspective_profiled(raw, M, DEST, None, fmt=fmt, colorspace=cs), warp_perspective(bgr, M, DEST)), (fmt, cs, "plain")
    for name, prof in PROFILES.items():
        for rot in (False, True):
            got = warp_perspective_profiled(raw, M, DEST, prof, rot180=rot, fmt=fmt, colorspace=cs)
            want = warp_perspective_profiled(bgr, M, DEST, prof, rot180=rot)
            assert np.array_equal(got, want), (fmt, cs, name, rot, int((got != want).sum()))
            got = warp_lens(raw, M, DEST, _lens(), prof, rot180=rot, fmt=fmt, colorspace=cs)
            want = warp_lens(bgr, M, DEST, _lens(), prof, rot180=rot)
            assert np.array_equal(got, want), (fmt, cs, name, rot, "lens", int((got != want).sum()))
            assert np.array_equal(warp_perspective_profiled(raw, M, DEST, prof, rot180=rot, fmt=fmt, lens=_lens(), colorspace=cs), want)
    # the colour space matters, and the default is the call without the keyword
    plain = warp_perspective_profiled(raw, M, DEST, CS.SHIPPED, fmt=fmt)
    assert np.array_equal(warp_perspective_profiled(raw, M, DEST, CS.SHIPPED, fmt=fmt, colorspace="bt601"), plain)
    assert not np.array_equal(warp_perspective_profiled(raw, M, DEST, CS.SHIPPED, fmt=fmt, colorspace=cs), plain)
    # the points form
    pts = np.float32(QUAD)
    got, m1, s1 = warp_image_profiled(raw, pts, CS.SHIPPED, display_size=(140, 140), fmt=fmt, colorspace=cs)
    want, m2, s2 = warp_image_profiled(bgr, pts, CS.SHIPPED, display_size=(140, 140))
    assert s1 == s2 == 40 and np.array_equal(m1, m2) and np.array_equal(got, want)


def test_warp_image_with_a_lens_takes_the_format_and_the_colour_space(gpu_ctx):
    from chessboard_vision_amd.board_detection import warp_image
    raw = RC.noise(W, H, "nv12", 2)
    pts = np.float32([[4, 3], [27, 4], [5, 20], [28, 19]])
    got = warp_image(raw, pts, display_size=(140, 140), lens=_lens(), fmt="nv12", colorspace="bt709")[0]
    want = warp_image(RC.to_bgr(raw, "nv12", "bt709"), pts, display_size=(140, 140), lens=_lens())[0]
    assert np.array_equal(got, want) and got.any()
    with pytest.raises(ValueError):
        warp_image(raw, pts, fmt="nv12", colorspace="bt709")


# --- the pipeline: the many-frames forms and the _mb kernels --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frames(fmt, cs):
    """nine raw frames of a scripted game in the layout and colour space (inputs), and the BGR frames the restatement makes
    of them (the reference pipeline's input)"""
    from chessboard_vision_amd.stream import BoardPipeline
    p = BoardPipeline(PW, PH, N9)
    p.synth(0, N9, frames_per_ply=2)
    bgr = [p.download(0, i) for i in range(N9)]
    p.close()
    raw = [RC.from_bgr(f, fmt, cs) for f in bgr]
    return raw, [np.ascontiguousarray(RC.to_bgr(f, fmt, cs)) for f in raw]


KINDS = {"plain": dict(enhance=False), "profile": dict(enhance="profile", raw=True),
         "lens": dict(enhance=False, lens=True), "lens_profile": dict(enhance="profile", raw=True, lens=True)}


def _boards(kind, chunk, boards, fmt, cs, frames):
    """the warped boards of every frame and board of a raw-mode pipeline fed `frames` in (fmt, cs)"""
    from chessboard_vision_amd.stream import BoardPipeline
    kw = dict(KINDS[kind])
    lens = _lens(RL.BARREL[:2] + (PW / 2, PH / 2) + RL.BARREL[4:]) if kw.pop("lens", False) else None
    pts = S.scaled_corners(PW, PH)
    p = BoardPipeline(PW, PH, N9)
    p.configure(pts, profile=CS.PROFILES["radical"], chunk=chunk, lanes=1, lens=lens, **kw)
    if boards == 2:
        p.add_board(pts + np.float32(3), rot180=True, display_size=(800, 600), **(dict(profile=CS.SHIPPED) if "raw" in kw else {}))
    if fmt != "bgr":
        p.set_input_format(fmt, colorspace=cs)
        assert p.input_colorspace == cs
    for i, f in enumerate(frames):
        p.upload(i, f, fmt=fmt, colorspace=cs)
    p.run(0, N9)
    out = [[b.download(2, i).tobytes() for i in range(N9)] for b in [p] + list(p._boards)]
    p.close()
    return out


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("fmt", RC.LAYOUTS)
def test_pipeline_forms_equal_the_bgr_fed_pipeline(gpu_ctx, fmt, kind):
    """chunk 1 on one board (the single-board kernel, one frame a thread), chunk 9 on two boards (the _mb kernel, the
    many-frames form with a short last group; with a lens the table-driven kernel in both); the colour spaces are dealt round
    the layouts and kinds so that each meets every layout"""
    cs = RC.NEW[(RC.LAYOUTS.index(fmt) + list(KINDS).index(kind)) % 3]
    raw, bgr = _frames(fmt, cs)
    for chunk, boards in ((1, 1), (9, 2), (9, 1), (1, 2)):
        got = _boards(kind, chunk, boards, fmt, cs, raw)
        want = _boards(kind, chunk, boards, "bgr", "bt601", bgr)
        assert got == want, (fmt, cs, kind, chunk, boards)
        assert len(set(got[0])) > 1   # the frames differ: a move is in them
