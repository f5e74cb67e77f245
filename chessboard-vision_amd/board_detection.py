"""warp_image / reorder / find_chessboard_corners — drop-in for board_detection.py:4-71.

warp_image and reorder are the hot path's; find_chessboard_corners is the widening row f3 (pixel
stages on the GPU, contour following on the host inside the same library).  The overlay-drawing helpers of the
reference module (board_detection.py:84-146) are UI code and are not part of this package."""
import ctypes as C

import numpy as np

from . import _native as N


def reorder(myPoints):
    """Order four corner points TL, TR, BL, BR by x+y and y-x extremes
    (board_detection.py:49-58).  Returns int32 (4,1,2)."""
    pts = np.asarray(myPoints).reshape((4, 2))
    out = np.zeros((4, 1, 2), np.int32)
    s = pts.sum(1)
    d = np.diff(pts, axis=1)
    out[0] = pts[np.argmin(s)]
    out[3] = pts[np.argmax(s)]
    out[1] = pts[np.argmin(d)]
    out[2] = pts[np.argmax(d)]
    return out


def get_perspective_transform(src_pts, dst_pts):
    """cv2.getPerspectiveTransform (8x8 LU in double); host-side, no GPU needed."""
    lib = N.load()
    s = np.ascontiguousarray(np.asarray(src_pts, dtype=np.float32).reshape(4, 2))
    d = np.ascontiguousarray(np.asarray(dst_pts, dtype=np.float32).reshape(4, 2))
    M = np.empty((3, 3), np.float64)
    rc = lib.cbv_get_perspective_transform(N.ptr(s), N.ptr(d), N.ptr(M))
    if rc != 0:
        raise RuntimeError(lib.cbv_last_error(None).decode())
    return M


def warp_perspective(img, M, dsize, rot180=False):
    c = N.context()
    f = N.as_bgr(img)
    M = np.ascontiguousarray(M, dtype=np.float64)
    dw, dh = int(dsize[0]), int(dsize[1])
    out = np.empty((dh, dw, 3), np.uint8)
    c.check(c.lib.cbv_warp_perspective(c.h, N.ptr(f), f.shape[1], f.shape[0], f.strides[0], N.ptr(M), dw, dh, 1 if rot180 else 0,
                                       N.ptr(out), out.strides[0]))
    return out


def _lens_struct(lens):
    return lens.struct() if lens is not None else N.LensStruct()


def _lens_points(fn, points, lens):
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 2))
    out = np.empty_like(p)
    lib = N.load()
    if getattr(lib, fn)(_lens_struct(lens), N.ptr(p), p.shape[0], N.ptr(out)) != 0:
        raise ValueError(lib.cbv_last_error(None).decode())
    return out


def undistort_points(points, lens):
    """Positions in the frame as the camera delivers it -> ideal (pinhole) positions, float64 [n, 2]: the fixed-point
    iteration of cv2.undistortPoints(points, K, dist, P=K) with exactly 40 rounds (include/cbv.h,
    cbv_lens_undistort_points).  `lens`: a stream.Lens.  Host only."""
    return _lens_points("cbv_lens_undistort_points", points, lens)


def distort_points(points, lens):
    """Ideal positions -> where the delivered frame shows them, float64 [n, 2]: the forward model of the lens
    (cbv_lens_distort_points).  Host only."""
    return _lens_points("cbv_lens_distort_points", points, lens)


def warp_lens(img, M, dsize, lens, profile=None, rot180=False, fmt="bgr", colorspace="bt601"):
    """warp_perspective_profiled through the camera's `lens` (a stream.Lens): the format's conversion, the profile, then the
    warp whose coordinates go through the lens model, in one kernel with one interpolation per pixel (include/cbv.h,
    cbv_warp_lens, cbv_warp_jpeg_lens).  `M` is the ideal-coordinate matrix.  lens=None is the lens-free call.  `colorspace`: of a
    YUV `fmt` (yuv_to_bgr)."""
    N.colorspace_bits(colorspace, fmt)  # (refused before the library is called)
    c = N.context()
    M = np.ascontiguousarray(M, dtype=np.float64)
    dw, dh = int(dsize[0]), int(dsize[1])
    out = np.empty((dh, dw, 3), np.uint8)
    if isinstance(fmt, str) and fmt.lower() == "mjpeg":
        a = _jpeg_bytes(img)
        st = C.c_int32(0)
        c.check(c.lib.cbv_warp_jpeg_lens(c.h, N.ptr(a), a.size, N.ColorProfile.from_dict(profile), _lens_struct(lens), N.ptr(M), dw, dh,
                                         1 if rot180 else 0, N.ptr(out), out.strides[0], C.byref(st)))
        return out
    raw, w, h, keep = N.raw_frame(img, fmt, colorspace)
    c.check(c.lib.cbv_warp_lens(c.h, raw, w, h, N.ColorProfile.from_dict(profile), _lens_struct(lens), N.ptr(M), dw, dh, 1 if rot180 else 0,
                                N.ptr(out), out.strides[0]))
    return out


def warp_image(img, points, display_size=(1280, 720), margin=100, lens=None, fmt="bgr", colorspace="bt601"):
    """Top-down view of the board (board_detection.py:61-71).
    Returns (warped, matrix, board_size).  With a `lens` (stream.Lens) the `points` are positions in the frame as delivered:
    they are undistorted before getPerspectiveTransform, the matrix returned is the ideal-coordinate one, and the warp
    corrects the distortion in its gather; there `fmt` / `colorspace` name a camera-native `img` (warp_lens)."""
    board_size = min(display_size) - margin
    pts1 = np.float32(points if lens is None else undistort_points(points, lens))
    pts2 = np.float32([[0, 0], [board_size, 0], [0, board_size], [board_size, board_size]])
    matrix = get_perspective_transform(pts1, pts2)
    if lens is None:
        if fmt != "bgr" or colorspace != "bt601":
            raise ValueError("fmt / colorspace belong to the lens form of warp_image; warp_image_profiled takes a camera-native frame without a lens")
        warped = warp_perspective(img, matrix, (board_size, board_size))
    else:
        warped = warp_lens(img, matrix, (board_size, board_size), lens, fmt=fmt, colorspace=colorspace)
    return warped, matrix, board_size


def warp_jpeg(data, M, dsize, profile=None, rot180=False, out=None):
    """warp_perspective_profiled(jpeg_to_bgr(data), M, dsize, profile, rot180), byte for byte, sampled from the decoded planes
    with the BGR frame never made (include/cbv.h, cbv_warp_jpeg).  `data`: one baseline JPEG stream, bytes or a uint8 array.
    Returns (warped, status), status = the decode's status word (jpeg_decode).  `out`: a uint8 [dh, dw, 3] array to write."""
    c = N.context()
    a = _jpeg_bytes(data)
    M = np.ascontiguousarray(M, dtype=np.float64)
    dw, dh = int(dsize[0]), int(dsize[1])
    if out is None:
        out = np.empty((dh, dw, 3), np.uint8)
    assert out.dtype == np.uint8 and out.shape == (dh, dw, 3) and out.strides[1:] == (3, 1)
    st = C.c_int32(0)
    c.check(c.lib.cbv_warp_jpeg(c.h, N.ptr(a), a.size, N.ColorProfile.from_dict(profile), N.ptr(M), dw, dh, 1 if rot180 else 0, N.ptr(out),
                                out.strides[0], C.byref(st)))
    return out, int(st.value)


def warp_perspective_profiled(img, M, dsize, profile, rot180=False, fmt="bgr", lens=None, colorspace="bt601"):
    """warp_perspective(ImageEnhancer(profile).apply_color_profile(img), M, dsize, rot180), byte for byte, in one kernel: the
    profile is applied to the four source pixels each destination pixel blends (include/cbv.h, cbv_warp_color_profile).
    `profile`: a dict with the keys of color_profile.json, `None` / `{}` = no profile.
    `fmt` other than "bgr": `img` is a camera-native frame in the layout yuv_to_bgr / bayer_to_bgr take, and the result is
    that of the converted frame, with neither the BGR frame nor the profiled frame made (cbv_warp_color_profile_raw).
    `fmt` "mjpeg": `img` is one baseline JPEG stream (bytes or a uint8 array), and the result is that of jpeg_to_bgr's frame,
    sampled from the decoded planes (cbv_warp_jpeg).
    `lens` (a stream.Lens): the warp corrects the camera's lens distortion in its gather and `M` is the ideal-coordinate
    matrix (warp_lens).
    `colorspace`: of a YUV `fmt`, "bt601" (default), "bt601-full", "bt709" or "bt709-full" (yuv_to_bgr); ValueError with
    another format."""
    if lens is not None:
        return warp_lens(img, M, dsize, lens, profile, rot180, fmt, colorspace)
    N.colorspace_bits(colorspace, fmt)  # (refused before the library is called)
    c = N.context()
    if isinstance(fmt, str) and fmt.lower() == "mjpeg":
        return warp_jpeg(img, M, dsize, profile, rot180)[0]
    if N.format_id(fmt) != N.FMT_BGR:
        raw, w, h, keep = N.raw_frame(img, fmt, colorspace)
        M = np.ascontiguousarray(M, dtype=np.float64)
        dw, dh = int(dsize[0]), int(dsize[1])
        out = np.empty((dh, dw, 3), np.uint8)
        c.check(c.lib.cbv_warp_color_profile_raw(c.h, raw, w, h, N.ColorProfile.from_dict(profile), N.ptr(M), dw, dh, 1 if rot180 else 0,
                                                 N.ptr(out), out.strides[0]))
        return out
    f = N.as_bgr(img)
    M = np.ascontiguousarray(M, dtype=np.float64)
    dw, dh = int(dsize[0]), int(dsize[1])
    out = np.empty((dh, dw, 3), np.uint8)
    c.check(c.lib.cbv_warp_color_profile(c.h, N.ptr(f), f.shape[1], f.shape[0], f.strides[0], N.ColorProfile.from_dict(profile), N.ptr(M), dw, dh,
                                         1 if rot180 else 0, N.ptr(out), out.strides[0]))
    return out


def warp_image_profiled(img, points, profile, display_size=(1280, 720), margin=100, rot180=False, fmt="bgr", colorspace="bt601"):
    """warp_image(ImageEnhancer(profile).apply_color_profile(img), points, display_size, margin) in one kernel
    (warp_perspective_profiled); `rot180` adds cv2.rotate(ROTATE_180); `fmt`: the format of a camera-native `img`, `colorspace`:
    the colour space of a YUV one.  Returns what warp_image returns: (warped, matrix, board_size)."""
    board_size = min(display_size) - margin
    pts2 = np.float32([[0, 0], [board_size, 0], [0, board_size], [board_size, board_size]])
    matrix = get_perspective_transform(np.float32(points), pts2)
    return warp_perspective_profiled(img, matrix, (board_size, board_size), profile, rot180, fmt, colorspace=colorspace), matrix, board_size


def yuv_to_bgr(frame, fmt, colorspace="bt601"):
    """cv2.cvtColor(frame, COLOR_YUV2BGR_NV12 / _NV21 / _I420 / _YV12 / _YUY2 / _YVYU / _UYVY) on the GPU (include/cbv.h,
    cbv_yuv_to_bgr): a new uint8 [h, w, 3] array.  `fmt` "nv12" / "nv21": one [h * 3 // 2, w] array or a (y, chroma) pair of
    planes; "yuv420p" / "yv12": one contiguous [h * 3 // 2, w] array or the three planes in memory order, (y, u, v) /
    (y, v, u); "yuyv" / "yvyu" / "uyvy": [h, w, 2].  cv2's I420 goes by libav's name "yuv420p"; "i420" is an unknown
    format (ValueError).  Strided views are taken as they are (_native.raw_frame).  A Bayer mosaic ("bayer_rggb", ...) goes
    to bayer_to_bgr and is refused here (ValueError).  (A BoardPipeline takes such frames directly: upload(fmt=...),
    set_input_format.)
    `colorspace`: "bt601" (default: cv2's BT.601 limited range, what a UVC webcam's YUYV needs), "bt601-full" (JFIF: phone
    cameras, full-range UVC modes), "bt709" (decoded video at 720p and above) or "bt709-full" (capture cards in PC range);
    the same fixed-point arithmetic with that colour space's constants (include/cbv.h, CBV_CS_*)."""
    from . import _native as N
    if N.is_bayer(fmt):
        raise ValueError("yuv_to_bgr converts YUV frames; a %s mosaic goes to bayer_to_bgr" % fmt)
    raw, w, h, keep = N.raw_frame(frame, fmt, colorspace)
    if raw.fmt == N.FMT_BGR:
        raise ValueError("yuv_to_bgr converts YUV frames (%s)" % ", ".join(k for k in N.FORMATS if k != "bgr"))
    ctx = N.context()
    out = np.empty((h, w, 3), np.uint8)
    ctx.check(ctx.lib.cbv_yuv_to_bgr(ctx.h, raw, w, h, N.ptr(out), w * 3))
    return out


def bayer_to_bgr(frame, fmt, develop=None):
    """cv2.cvtColor(frame, COLOR_Bayer??2BGR), the bilinear demosaic of an 8-bit mosaic, on the GPU (include/cbv.h,
    cbv_bayer_to_bgr): a new uint8 [h, w, 3] array.  `fmt` "bayer_rggb" / "bayer_bggr" / "bayer_grbg" /
    "bayer_gbrg" names the top-left 2 x 2 block read row by row; cv2 names its codes by the block at (1, 1), so
    "bayer_rggb" is COLOR_BayerBG2BGR, "bayer_bggr" COLOR_BayerRG2BGR, "bayer_grbg" COLOR_BayerGB2BGR and "bayer_gbrg"
    COLOR_BayerGR2BGR.  `frame` is one uint8 [h, w] array, w and h even and at least 4; strided views are taken as they are
    (_native.raw_frame).  With "16", "10p" or "12p" behind the name the samples are 10 to 16 bits in a little-endian 16-bit
    container (one uint16 [h, w] array), or MIPI RAW10 / RAW12 packed rows (uint8 [h, w * 5 // 4] / [h, w * 3 // 2]).
    `develop` (a `develop.Develop`, a uint8 [3, 2^bits] array with rows B, G, R, or None) is the per-colour table every
    sample goes through in front of the demosaic: black and white level, white-balance gains and a tone curve.  None is the
    format's default: the neutral table v * 255 / (2^bits - 1), rounded half up, for the three encodings, and no table at all
    for an 8-bit mosaic.  No colour matrix is applied.  (A BoardPipeline takes such frames directly: upload(fmt=...),
    set_input_format.)"""
    from . import _native as N
    from .develop import develop_tables
    if not N.is_bayer(fmt):
        raise ValueError("bayer_to_bgr converts Bayer mosaics (%s), got %r" % (", ".join(list(N.BAYER_FORMATS) + list(N.BAYER_DEEP_FORMATS)), fmt))
    raw, w, h, keep = N.raw_frame(frame, fmt)
    tables, bits = develop_tables(develop, raw.fmt)
    ctx = N.context()
    out = np.empty((h, w, 3), np.uint8)
    ctx.check(ctx.lib.cbv_bayer_to_bgr(ctx.h, raw, w, h, N.ptr(tables) if tables is not None else None, bits, N.ptr(out), w * 3))
    return out


def _jpeg_bytes(data):
    a = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    if a.size == 0:
        raise ValueError("an empty JPEG stream")
    return a


def jpeg_probe(data):
    """The header of one baseline JPEG stream (include/cbv.h, cbv_jpeg_probe) as a dict: w, h, components, hs, vs (luma
    sampling), restart_interval, intervals, std_tables (no DHT in the stream), entropy_offset, entropy_length, plane_elems,
    blocks (per component: blocks wide, blocks high).  Host only.  ValueError for a stream the decode refuses."""
    lib = N.load()
    a = _jpeg_bytes(data)
    info = N.JpegInfo()
    rc = lib.cbv_jpeg_probe(N.ptr(a), a.size, C.byref(info))
    if rc != 0:
        raise ValueError("%s (code %d)" % (lib.cbv_last_error(None).decode(), rc))
    d = {k: getattr(info, k) for k, _ in N.JpegInfo._fields_ if not k.startswith("blocks")}
    d["blocks"] = [(info.blocks_w[c], info.blocks_h[c]) for c in range(info.components)]
    return d


def jpeg_decode(data, host=False, entropy="auto", piece_bytes=0, stats=False):
    """One baseline JPEG stream with its stage outputs: (bgr [h, w, 3], coef int16 [plane_elems], planes uint8 [plane_elems],
    status).  On the GPU (cbv_jpeg_decode_ex), or with host=True by the library's host twin (cbv_jpeg_decode_host_ex, no
    GPU): the same bodies, byte for byte.  The layout of coef and planes: jpeg_probe(data)["blocks"] and include/cbv.h.
    status: _native.JPEG_BAD_CODE | JPEG_NO_DATA | JPEG_RESTART, 0 for an undamaged stream.  entropy: "auto" (pieces for a
    stream without DRI, restart intervals otherwise), "interval", "pieces" or "segments" (restart intervals cut into pieces
    too), and piece_bytes the piece size (0: the default, otherwise a multiple of 4); neither changes the result.
    stats=True appends a dict with pieces, rounds and settled_round0 (zeros for a stream decoded by interval)."""
    a = _jpeg_bytes(data)
    info = jpeg_probe(a)
    bgr = np.empty((info["h"], info["w"], 3), np.uint8)
    coef = np.empty(info["plane_elems"], np.int16)
    planes = np.empty(info["plane_elems"], np.uint8)
    st = C.c_int32()
    ps = N.JpegDecodeStats()
    mode = N.JPEG_ENTROPY[entropy]
    if host:
        lib = N.load()
        rc = lib.cbv_jpeg_decode_host_ex(N.ptr(a), a.size, N.ptr(bgr), info["w"] * 3, N.ptr(coef), N.ptr(planes), C.byref(st), mode, int(piece_bytes),
                                         C.byref(ps))
        if rc != 0:
            raise RuntimeError("libcbv_hip: %s (code %d)" % (lib.cbv_last_error(None).decode(), rc))
    else:
        ctx = N.context()
        ctx.check(ctx.lib.cbv_jpeg_decode_ex(ctx.h, N.ptr(a), a.size, N.ptr(bgr), info["w"] * 3, N.ptr(coef), N.ptr(planes), C.byref(st), mode,
                                             int(piece_bytes), C.byref(ps)))
    if stats:
        return bgr, coef, planes, st.value, {k: getattr(ps, k) for k, _ in N.JpegDecodeStats._fields_}
    return bgr, coef, planes, st.value


def jpeg_to_bgr(data):
    """cv2.imdecode(data, IMREAD_COLOR) of a baseline JPEG stream (a Motion-JPEG frame), on the GPU: a new uint8 [h, w, 3]
    array, the bytes libjpeg's defaults give (slow-integer IDCT, fancy upsampling; include/cbv.h).  `data`: bytes or a uint8
    array.  A damaged stream decodes as far as it goes (jpeg_decode returns the status word); a stream outside the
    accepted set raises ValueError."""
    a = _jpeg_bytes(data)
    info = jpeg_probe(a)
    ctx = N.context()
    bgr = np.empty((info["h"], info["w"], 3), np.uint8)
    st = C.c_int32()
    ctx.check(ctx.lib.cbv_jpeg_decode(ctx.h, N.ptr(a), a.size, N.ptr(bgr), info["w"] * 3, None, None, C.byref(st)))
    return bgr


def crop_inner_squares(img_warped, board_size, offset=0):
    """The warped board without an `offset`-pixel border, as a view, and the new board size (board_detection.py:74-82)."""
    cropped = img_warped[offset:board_size - offset, offset:board_size - offset]
    return cropped, board_size - 2 * offset


def corners_from_edges(edges):
    """Host half of find_chessboard_corners: (approx polygon int32 (4,1,2) or None, number of external contours)."""
    from . import _native as N
    import ctypes as C
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.uint8))
    pts = (C.c_int32 * 8)()
    n = C.c_int(0)
    rc = N.load().cbv_board_corners_from_edges(e.ctypes.data, e.shape[1], e.shape[0], e.strides[0], pts, C.byref(n))
    if rc < 0:
        raise ValueError("corners_from_edges: bad arguments")
    return (np.array(pts, np.int32).reshape(4, 1, 2) if rc == 1 else None), n.value


def external_contours(img):
    """Inspection: cv2.findContours(img, RETR_EXTERNAL, CHAIN_APPROX_NONE) with contourArea and arcLength(closed) of each
    contour: (list of int32 (n, 2) point arrays in cv2's order, areas, perimeters).  Host only."""
    from . import _native as N
    import ctypes as C
    e = np.ascontiguousarray(np.asarray(img, dtype=np.uint8))
    lib = N.load()
    nc, npts = C.c_int(0), C.c_int(0)
    args = (e.ctypes.data, e.shape[1], e.shape[0], e.strides[0])
    rc = lib.cbv_external_contours(*args, None, 0, None, None, None, 0, C.byref(nc), C.byref(npts))
    if rc < 0 and (nc.value == 0 and npts.value == 0):
        raise ValueError("external_contours: bad arguments")
    pts = np.zeros((max(npts.value, 1), 2), np.int32)
    lens = np.zeros(max(nc.value, 1), np.int32)
    areas, perims = np.zeros(max(nc.value, 1)), np.zeros(max(nc.value, 1))
    i32p, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rc = lib.cbv_external_contours(*args, pts.ctypes.data_as(i32p), npts.value, lens.ctypes.data_as(i32p), areas.ctypes.data_as(dp),
                                   perims.ctypes.data_as(dp), nc.value, C.byref(nc), C.byref(npts))
    if rc != 0:
        raise ValueError("external_contours: bad arguments")
    ends = np.cumsum(lens[:nc.value])
    return [pts[b - n:b].copy() for b, n in zip(ends, lens[:nc.value])], areas[:nc.value].copy(), perims[:nc.value].copy()


def approx_poly_closed(curve, eps):
    """Inspection: cv2.approxPolyDP(curve, eps, True) of an integer (n, 2) curve, as int32 (m, 2).  Host only."""
    from . import _native as N
    import ctypes as C
    c = np.ascontiguousarray(np.asarray(curve, dtype=np.int32).reshape(-1, 2))
    out = np.zeros((max(len(c), 1), 2), np.int32)
    i32p = C.POINTER(C.c_int32)
    n = N.load().cbv_approx_poly_closed(c.ctypes.data_as(i32p), len(c), float(eps), out.ctypes.data_as(i32p), len(c))
    if n < 0:
        raise ValueError("approx_poly_closed: bad arguments")
    return out[:n].copy()


def find_chessboard_corners(img, debug=False):
    """board_detection.py:4-28: the four corners (reordered TL, TR, BL, BR; int32 (4,1,2)) of the largest
    four-cornered contour of the dilated Canny edges, or an empty array.  Pixel stages on the GPU, contour
    following on the host (cbv_find_chessboard_corners); `debug=True` also returns the dilated edge image
    instead of showing a window."""
    from . import _native as N
    import ctypes as C
    a = N.as_bgr(img)
    ctx = N.context()
    pts = (C.c_int32 * 8)()
    dil = np.empty(a.shape[:2], np.uint8) if debug else None
    rc = ctx.lib.cbv_find_chessboard_corners(ctx.h, N.ptr(a), a.shape[1], a.shape[0], a.strides[0], pts,
                                             dil.ctypes.data if debug else None, dil.strides[0] if debug else 0)
    if rc < 0:
        ctx.check(rc)
    out = reorder(np.array(pts, np.int32).reshape(4, 1, 2)) if rc == 1 else np.array([])
    return (out, dil) if debug else out
