"""cbv_warp_color_profile_raw (k_warp_raw_profile; board_detection.warp_perspective_profiled(fmt=...)) against the yardstick
of tests/raw_profile_ref.py, the oracle's warp_perspective(apply_color_profile(to_bgr(raw))) with the int64 conversions of
ref64_yuv / ref64_bayer, and against the product's own stages composed.  Every raw format; frames from 6 x 4 (the smallest
where a Bayer frame has an interior site and its clamped edge) to 640 x 480, white noise and a synthetic frame converted
into the format; destinations that are no multiple of the 64 x 16 workgroup tile and one of many tiles; quads inside, partly
outside, mirrored and entirely outside; both rotations; the profiles of color_sweep_ref plus the fractional one of the stage
tests.  Tolerance 0."""
import functools

import numpy as np
import pytest

import color_sweep_ref as CS
import raw_profile_ref as RP
from helpers import oracle_frame

pytestmark = pytest.mark.gpu

PROFILES = dict(CS.PROFILES, stages_fractional=CS.STAGES_FRACTIONAL)
NAMES = [n for n in PROFILES if PROFILES[n]]
DESTS = ((33, 21), (620, 620))
SIZES = ((6, 4), (38, 30), (318, 204), (640, 480))
ARG = -1


@functools.lru_cache(maxsize=None)
def _synth_bgr(w, h):
    f = np.array(CS.frame("lilac", 0)) if (w, h) == (CS.W, CS.H) else oracle_frame(w, h)
    f.setflags(write=False)
    return f


def _contents(w, h, fmt):
    return {"noise": RP.noise(w, h, fmt, 3), "synth": RP.from_bgr(_synth_bgr(w, h), fmt)}


def _matrix(quad, dw, dh):
    from chessboard_vision_amd.board_detection import get_perspective_transform
    return get_perspective_transform(np.float32(quad), np.float32([[0, 0], [dw, 0], [0, dh], [dw, dh]]))


def _to_bgr(raw, fmt):
    from chessboard_vision_amd.board_detection import bayer_to_bgr, yuv_to_bgr
    return bayer_to_bgr(raw, fmt) if fmt.startswith("bayer") else yuv_to_bgr(raw, fmt)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("fmt", RP.FORMATS)
def test_equals_the_yardstick_and_the_composed_entry_points(gpu_ctx, oracle, fmt, size):
    """every content, destination, quad and rotation; the profiles are dealt round the cases so that every profile meets
    every format and size, and the shipped one meets every case"""
    from chessboard_vision_amd.board_detection import warp_perspective_profiled
    w, h = size
    k = NAMES.index("radical") + RP.FORMATS.index(fmt) + SIZES.index(size)
    for cname, raw in _contents(w, h, fmt).items():
        assert RP.size_of(raw, fmt) == size
        bgr = RP.to_bgr(raw, fmt)
        own = _to_bgr(raw, fmt)
        assert np.array_equal(own, bgr), (fmt, size, cname)  # (the conversion itself: held elsewhere, needed for what follows)
        for dest in DESTS:
            for qname, quad in RP.quads(w, h).items():
                M = _matrix(quad, *dest)
                for name in {"shipped", NAMES[k % len(NAMES)]}:
                    prof = PROFILES[name]
                    want = RP.yardstick(oracle, bgr, prof, M, dest)
                    for rot in (False, True):
                        got = warp_perspective_profiled(raw, M, dest, prof, rot180=rot, fmt=fmt)
                        ref = oracle.rotate180(want) if rot else want
                        assert np.array_equal(got, ref), (fmt, size, cname, dest, qname, rot, name, int((got != ref).sum()))
                        if qname == "outside":
                            assert not got.any()  # BORDER_CONSTANT 0, not the profile of black
                        if name == "shipped":  # the product's own stages, composed
                            assert np.array_equal(got, warp_perspective_profiled(own, M, dest, prof, rot180=rot)), (fmt, size, cname, dest, qname, rot)
                k += 1


@pytest.mark.parametrize("fmt", RP.FORMATS)
def test_every_profile_meets_every_format(gpu_ctx, oracle, fmt):
    """all twelve profiles, the radical ones included, on a 38 x 30 noise frame and a quad partly outside it"""
    from chessboard_vision_amd.board_detection import warp_perspective_profiled
    w, h, dest = 38, 30, (33, 21)
    raw = RP.noise(w, h, fmt, 9)
    bgr = RP.to_bgr(raw, fmt)
    M = _matrix(RP.quads(w, h)["partly_outside"], *dest)
    for name, prof in PROFILES.items():
        got = warp_perspective_profiled(raw, M, dest, prof, fmt=fmt)
        want = RP.yardstick(oracle, bgr, prof, M, dest)
        assert np.array_equal(got, want), (fmt, name, int((got != want).sum()))


@pytest.mark.parametrize("fmt", RP.FORMATS)
def test_a_disabled_profile_is_ingest_then_the_plain_warp(gpu_ctx, fmt):
    from chessboard_vision_amd.board_detection import warp_perspective, warp_perspective_profiled
    for w, h in ((6, 4), (38, 30)):
        raw = RP.noise(w, h, fmt, 4)
        own = _to_bgr(raw, fmt)
        for quad in RP.quads(w, h).values():
            M = _matrix(quad, 33, 21)
            for prof in (None, {}):
                for rot in (False, True):
                    got = warp_perspective_profiled(raw, M, (33, 21), prof, rot180=rot, fmt=fmt)
                    assert np.array_equal(got, warp_perspective(own, M, (33, 21), rot180=rot)), (fmt, w, h, rot)


def test_strided_planes_and_plane_tuples(gpu_ctx, oracle):
    """views with a row stride of their own (an NV12 pair cut out of a larger frame, a mosaic window) give the result of the
    packed frame"""
    from chessboard_vision_amd.board_detection import warp_perspective_profiled
    w, h, dest = 38, 30, (33, 21)
    M = _matrix(RP.quads(w, h)["partly_outside"], *dest)
    big = np.random.default_rng(2).integers(0, 256, (80, 100), dtype=np.uint8)
    y, uv = big[3:3 + h, 10:10 + w], big[40:40 + h // 2, 20:20 + w]
    packed = np.concatenate([y, uv])
    want = RP.yardstick(oracle, RP.to_bgr(packed, "nv12"), CS.SHIPPED, M, dest)
    assert np.array_equal(warp_perspective_profiled((y, uv), M, dest, CS.SHIPPED, fmt="nv12"), want)
    win = big[5:5 + h, 7:7 + w]
    want = RP.yardstick(oracle, RP.to_bgr(np.ascontiguousarray(win), "bayer_gbrg"), CS.SHIPPED, M, dest)
    assert np.array_equal(warp_perspective_profiled(win, M, dest, CS.SHIPPED, fmt="bayer_gbrg"), want)


def test_errors_leave_out_untouched(gpu_ctx):
    from chessboard_vision_amd import _native as N
    lib, ctx = gpu_ctx.lib, gpu_ctx
    M = np.eye(3)
    prof = N.ColorProfile.from_dict(CS.SHIPPED)
    nan = N.ColorProfile.from_dict(dict(CS.SHIPPED, val_scale=float("nan")))
    out = np.full((21, 33, 3), 0x5A, np.uint8)

    def call(raw, w, h, profile=prof, m=M, dw=33, dh=21, o=out, ostride=99):
        return lib.cbv_warp_color_profile_raw(ctx.h, raw, w, h, profile, N.ptr(m) if m is not None else None, dw, dh, 0,
                                              N.ptr(o) if o is not None else None, ostride)

    def frame(fmt, w, h):
        a = np.zeros((h * 3 // 2, w) if fmt in N.FORMATS_420 else (h, w, 2) if fmt in N.FORMATS_422 else (h, w), np.uint8)
        r = N.RawFrame()
        r.fmt, r.stride0, r.plane0 = N.format_id(fmt), a.strides[0], a.ctypes.data
        if fmt in N.FORMATS_420:
            r.stride1, r.plane1 = w, a.ctypes.data + w * h
        if fmt in ("yuv420p", "yv12"):
            r.stride1 = r.stride2 = w // 2
            r.plane2 = r.plane1 + (w // 2) * (h // 2)
        return r, a

    good, keep = frame("nv12", 38, 30)
    assert call(good, 38, 30) == 0 and not (out == 0x5A).all()
    out[:] = 0x5A
    cases = [("odd width", frame("nv12", 38, 30)[0], 37, 30, {}), ("odd height, 4:2:0", frame("nv12", 38, 30)[0], 38, 29, {}),
             ("odd width, 4:2:2", frame("yuyv", 38, 30)[0], 37, 30, {}), ("odd height, Bayer", frame("bayer_rggb", 38, 30)[0], 38, 29, {}),
             ("2 x 2 Bayer", frame("bayer_grbg", 4, 4)[0], 2, 2, {}), ("a non-finite profile", good, 38, 30, dict(profile=nan)),
             ("no profile", good, 38, 30, dict(profile=None)), ("no matrix", good, 38, 30, dict(m=None)), ("no frame", None, 38, 30, {}),
             ("a short output stride", good, 38, 30, dict(ostride=98)), ("an empty destination", good, 38, 30, dict(dw=0))]
    for fmt in ("nv12", "yuv420p", "yuyv", "bayer_bggr"):
        r, _a = frame(fmt, 38, 30)
        keep = (keep, _a)
        r.plane0 = None
        cases.append(("no plane 0, %s" % fmt, r, 38, 30, {}))
    r, a1 = frame("nv21", 38, 30)
    r.plane1 = None
    cases.append(("no chroma plane", r, 38, 30, {}))
    r, a2 = frame("yv12", 38, 30)
    r.plane2 = None
    cases.append(("no third plane", r, 38, 30, {}))
    r, a3 = frame("uyvy", 38, 30)
    r.stride0 = 38 * 2 - 1
    cases.append(("a stride below the row", r, 38, 30, {}))
    r, a4 = frame("nv12", 38, 30)
    r.fmt = N.FMT_BGR
    cases.append(("BGR", r, 38, 30, {}))
    r, a5 = frame("nv12", 38, 30)
    r.fmt = 0x77
    cases.append(("an unknown format", r, 38, 30, {}))
    for what, raw, w, h, kw in cases:
        assert call(raw, w, h, **kw) == ARG, what
        assert (out == 0x5A).all(), what
    assert call(good, 38, 30, o=None) == ARG
