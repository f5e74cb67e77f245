"""The statistics kernels, the class API's gate and classes and the pipeline's decision byte and scan against the numpy
definitions from pixels (tests/ref_regions.py): every shape class of the region masks, and every comparison of the
detectors at or next to its threshold.  No expected value comes from the C oracle or from tests/ref_logic.py."""
import ctypes as C

import numpy as np
import pytest

import ref64 as R
import ref_regions as RR
import region_cases as RC
from chessboard_vision_amd import _native as N

pytestmark = pytest.mark.gpu

INTENSITY = {None: 0, "LEVE": 1, "PARCIAL": 2, "TOTAL": 3}


def _same_stats(st, want, tag, skip=()):
    got = RR.stats_of_struct(st)
    for k in want:
        if k not in skip:
            assert got[k] == want[k], (tag, k, got[k], want[k])


def _chunks(seq, n=N.MAX_SQUARES):
    return [seq[i:i + n] for i in range(0, len(seq), n)]


def _with_planes(gpu_ctx, planes):
    """A SquareSet with one square per plane (at most 64, any mix of shapes) whose GRAY planes are `planes` as given: the
    geometry comes from a load, then every plane is replaced, so no blur stands between the test's pixels and the sums."""
    from chessboard_vision_amd._squares import GRAY, SquareSet
    ss = SquareSet(gpu_ctx)
    ss.load({i: p for i, p in enumerate(planes)}, 5)
    for i, p in enumerate(planes):
        ss.set(GRAY, i, p)
    return ss


def _pack(squares, cn, gap=1):
    """One host image that holds the gray squares side by side (rows of at most 512 pixels), as `cn` equal channels,
    and the SquareLayout of their rectangles; the pixels between squares are noise, which no square may read."""
    from chessboard_vision_amd._squares import _image_of
    from chessboard_vision_amd.grid_extractor import SquareLayout
    rects, x, y, row_h = [], 0, 0, 0
    for g in squares:
        h, w = g.shape[:2]
        if x + w > 512:
            x, y, row_h = 0, y + row_h + gap, 0
        rects.append((x, y, w, h))
        x, row_h = x + w + gap, max(row_h, h)
    colour = squares[0].ndim == 3  # BGR squares: a BGR board as it is
    board = np.random.default_rng(99).integers(0, 256, (y + row_h, 512) + ((3,) if colour else ()), dtype=np.uint8)
    for g, (x0, y0, w, h) in zip(squares, rects):
        board[y0:y0 + h, x0:x0 + w] = g
    if cn == 3 and not colour:
        board = np.ascontiguousarray(np.repeat(board[:, :, None], 3, axis=2))  # BGR2GRAY of (v, v, v) is v: the weights sum to 2^15
    return board, _image_of(board), SquareLayout(list(range(len(squares))), rects)


# ---------------------------------------------------------------------------------------------------------------
# a. the statistics kernels at every shape class
# ---------------------------------------------------------------------------------------------------------------


def test_statistics_of_given_planes_at_every_shape_class(gpu_ctx):
    """k_squares_stats on planes the test wrote (set(GRAY), set(REF), set(MEAN), set(VAR)): every sum and count equals
    the numpy definition, for short sides 1 to 4 (corner size 0 and 1), odd and even centres, empty / full / clipped
    rings and 128 x 128 of 255 (sumsq at its u32 maximum)."""
    from chessboard_vision_amd._squares import MEAN, REF, VAR
    cases = RC.random_squares()
    planes = [g for _, g in cases]
    assert len(planes) <= N.MAX_SQUARES
    ss = _with_planes(gpu_ctx, planes)
    st = ss.stats()
    for i, (name, g) in enumerate(cases):
        _same_stats(st[i], RR.stats(g), name)
    assert st[len(RC.SHAPES) * 2 - 1].sumsq == 128 * 128 * 255 * 255
    small = [i for i, (_, g) in enumerate(cases) if min(g.shape) < 4]
    assert small and all(st[i].border_cnt == st[i].n and st[i].border_sum == st[i].sum for i in small)
    # with a reference and a background model: |gray - ref| and the z count
    rng = np.random.default_rng(8)
    ss.set_ref()
    ss.calibrate(1.0)
    refs, means, vars_ = [], [], []
    for i, g in enumerate(planes):
        refs.append(rng.integers(0, 256, g.shape, dtype=np.uint8))
        means.append(g.astype(np.float32) + np.float32(3) * rng.integers(-1, 2, g.shape).astype(np.float32))
        vars_.append(rng.choice(np.float32([1.0, 1.44, 4.0]), g.shape).astype(np.float32))  # z = 0, 3, 2.5, 1.5: at, above, below 2.5
        ss.set(REF, i, refs[i])
        ss.set(MEAN, i, means[i])
        ss.set(VAR, i, vars_[i])
    st = ss.stats(use_ref=True, use_model=True, z_threshold=2.5)
    counted = 0
    for i, (name, g) in enumerate(cases):
        want = RR.stats(g, ref=refs[i], mean=means[i], var=vars_[i], z_thr=2.5)
        _same_stats(st[i], want, name)
        counted += want["z_count"]
    assert counted > 1000


@pytest.mark.parametrize("cn", [3, 1], ids=["bgr", "gray"])
def test_statistics_behind_the_blur_at_every_shape_class(gpu_ctx, cn):
    """load(squares, 5) + stats(): BGR2GRAY, the 5 x 5 blur on the square alone and the statistics, against the
    definitions (the integer BGR2GRAY and the 8-bit GaussianBlur of tests/ref64.py, then ref_regions.stats)."""
    from chessboard_vision_amd._squares import GRAY, SquareSet
    rng = np.random.default_rng(21)
    imgs = [rng.integers(0, 256, s + ((3,) if cn == 3 else ()), dtype=np.uint8) for s in RC.SHAPES]
    imgs += [np.full(s + ((3,) if cn == 3 else ()), 255, np.uint8) for s in RC.SHAPES]
    ss = SquareSet(gpu_ctx)
    ss.load({i: im for i, im in enumerate(imgs)}, 5)
    st = ss.stats()
    for i, im in enumerate(imgs):
        g = R.gaussian_blur_u8(R.bgr2gray_q15(im) if cn == 3 else im, 5)
        assert np.array_equal(ss.get(GRAY, i), g), i
        _same_stats(st[i], RR.stats(g), (cn, i, im.shape))


QUIET_HOUGH = (1.2, 100.0, 1.0e6, 0.2, 0.55)  # an accumulator threshold no square reaches: HoughCircles runs and finds nothing


def test_fused_kernel_through_the_class_api_at_every_shape_class(gpu_ctx):
    """The fused preprocess + statistics kernel (BGR squares of one image: cbv_squares_detect_all with its gate,
    cbv_squares_detect_changes with the model) at every shape class, random and all-white.  What the two calls return is
    a function of the kernel's sums: has_piece, method, centre, radius and, bit for bit, confidence and
    center_border_diff of every square equal detect_piece on the blurred plane by its definition; z_count, n, z_max, the
    class and is_circular equal the definition against a model the test wrote.  The squares with a short side below 4
    read the mask whose border region is the whole square."""
    from chessboard_vision_amd._squares import GRAY, MEAN, VAR, SquareSet
    rng = np.random.default_rng(41)
    imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in RC.SHAPES] + [np.full(s + (3,), 255, np.uint8) for s in RC.SHAPES]
    for (h, w) in RC.SHAPES:  # a bright block around the centre of every shape: what is left of it behind the blur passes the
        g = np.full((h, w), 20, np.uint8)  # pre-filter where noise does not, so the centre and border means decide
        g[h // 2 - h // 5:h // 2 + h // 5 + 1, w // 2 - w // 5:w // 2 + w // 5 + 1] = 240
        imgs.append(np.repeat(g[:, :, None], 3, axis=2))
    board, img, lay = _pack(imgs, 3)
    grays = [R.gaussian_blur_u8(R.bgr2gray_q15(im), 5) for im in imgs]
    ss = SquareSet(gpu_ctx)
    ss.adopt(lay)
    prm = N.DetectParams()
    prm.change_threshold, prm.circle_threshold, prm.use_delta = 25.0, 0.6, 1
    prm.hough = N.HoughParams(*QUIET_HOUGH)
    rows = ss.detect_all(img, lay, prm)
    methods, small_diff = set(), 0
    for i, g in enumerate(grays):
        assert np.array_equal(ss.get(GRAY, i), g), i
        has_piece, method, changed, should, evaluated, cx, cy, radius, conf, diff = rows[i]
        assert changed and should and evaluated
        want = RR.detect_piece_no_hough(g)
        got = {"has_piece": bool(has_piece), "method": N.METHOD_NAMES[method], "center": (cx, cy) if has_piece else None,
               "radius": radius if has_piece else None, "confidence": conf, "center_border_diff": diff}
        _same_decision(got, want, (i, g.shape))
        methods.add(want["method"])
        small_diff += min(g.shape) < 4 and not RR.std_below_15(g)
    assert "center_diff" in methods and None in methods and small_diff >= 3
    # the same kernel with a background model
    ss.calibrate(1.0)
    means, vars_ = [], []
    for i, g in enumerate(grays):
        means.append(g.astype(np.float32) + np.float32(3) * rng.integers(-1, 2, g.shape).astype(np.float32))
        vars_.append(rng.choice(np.float32([1.0, 1.44, 4.0]), g.shape).astype(np.float32))
        ss.set(MEAN, i, means[i])
        ss.set(VAR, i, vars_[i])
    cp = N.ChangeParams()
    cp.z_threshold, cp.select, cp.circle_threshold, cp.hough = 2.5, lay.all_mask, 0.6, N.HoughParams(*QUIET_HOUGH)
    rows = ss.detect_changes(img, lay, 5, cp)
    reported = 0
    for i, g in enumerate(grays):
        z_count, pct, in_result, intensity = RR.change_class(g.astype(np.float32), means[i], vars_[i], 2.5)
        z_max = np.max(np.abs(g.astype(np.float32) - means[i]) / np.sqrt(vars_[i]))
        r_in, r_int, r_circ, r_zmax, r_zcount, r_n = rows[i]
        assert (r_zcount, r_n, bool(r_in), r_int) == (z_count, g.size, in_result, INTENSITY[intensity]), (i, g.shape, rows[i])
        assert np.float32(r_zmax).tobytes() == np.float32(z_max).tobytes(), (i, r_zmax, z_max)
        assert bool(r_circ) == (in_result and RR.detect_piece_no_hough(g)["has_piece"]), (i, g.shape)
        reported += in_result
    assert reported >= len(grays) // 2


# ---------------------------------------------------------------------------------------------------------------
# b. detect_all_pieces' gate at exact ties of mean |gray - reference|
# ---------------------------------------------------------------------------------------------------------------


def _gate(changed, cached, check_given, in_check, use_delta):
    """(should_process, evaluated) of one square, piece_detector.py:370-410"""
    should = bool(check_given and in_check)
    if not should and (not check_given or use_delta):
        if not cached or changed:
            should = True
    return should, (should or not cached)


@pytest.mark.parametrize("cn,thr,shape", [(3, 25, (8, 8)), (1, 25, (8, 8)), (3, 12.5, (8, 8)), (1, 12.5, (8, 8)), (3, 25, (7, 9)), (3, 12.5, (6, 11))],
                         ids=["bgr-25", "gray-25", "bgr-12.5", "gray-12.5", "bgr-25-odd", "bgr-12.5-6x11"])
def test_gate_at_exact_ties_of_the_mean_difference(gpu_ctx, cn, thr, shape):
    """64 squares whose reference is the plane the GPU produced moved by integer steps, so that sum |gray - ref| is
    exactly thr * n, one below and one above (thr * n is an integer: even n for 12.5): `changed`, `should_process` and
    `evaluated` of cbv_squares_detect_all equal np.mean(absdiff) > thr and the gate of detect_all_pieces, with and
    without cached results, with and without squares_to_check, with and without use_delta."""
    from chessboard_vision_amd._squares import GRAY, REF, SquareSet
    h, w = shape
    n = h * w
    total = thr * n
    assert total == int(total)
    rng = np.random.default_rng(13)
    board, img, lay = _pack([rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(64)], cn)
    ss = SquareSet(gpu_ctx)
    ss.adopt(lay)
    prm = N.DetectParams()
    prm.change_threshold, prm.circle_threshold, prm.use_delta = float(thr), 0.6, 1
    prm.hough = N.HoughParams(1.2, 100.0, 25.0, 0.2, 0.55)
    rows = ss.detect_all(img, lay, prm)
    assert all(r[2] == 1 and r[3] == 1 and r[4] == 1 for r in rows)  # no references yet: changed, processed, evaluated
    grays, refs, side = [], [], []
    for i in range(64):
        g = ss.get(GRAY, i)
        src = board[lay.rects[i][1]:lay.rects[i][1] + h, lay.rects[i][0]:lay.rects[i][0] + w]
        assert np.array_equal(g, R.gaussian_blur_u8(src[..., 0] if cn == 3 else src, 5))
        step = np.full(n, int(thr), np.int64)
        step[:int(total) - int(thr) * n] += 1          # 12.5: half the pixels move by 13, half by 12
        side.append((0, -1, 1)[i % 3])
        step[n - 1] += side[i]
        gi = g.astype(np.int64).ravel()
        ref = np.where(gi < 128, gi + step, gi - step).reshape(h, w)
        assert ref.min() >= 0 and ref.max() <= 255
        assert int(np.abs(ref - g).sum()) == int(total) + side[i]
        grays.append(g)
        refs.append(ref.astype(np.uint8))
        ss.set(REF, i, refs[i])
    has_ref = [i % 16 != 15 for i in range(64)]
    cached = [(i // 3) % 2 == 0 for i in range(64)]
    in_check = [(i // 6) % 2 == 0 for i in range(64)]
    bits = lambda flags: sum(1 << i for i, f in enumerate(flags) if f)
    prm.has_ref, prm.cached, prm.check = bits(has_ref), bits(cached), bits(in_check)
    want_changed = [(not has_ref[i]) or RR.has_changed(grays[i], refs[i], thr) for i in range(64)]
    tied = [i for i in range(64) if has_ref[i]]
    count = {s: sum(1 for i in tied if side[i] == s) for s in (-1, 0, 1)}
    print("mean |gray - ref| against %s: %d squares one step below, %d exactly at, %d one step above" % (thr, count[-1], count[0], count[1]))
    assert min(count.values()) >= 3
    for i in tied:
        assert want_changed[i] == (side[i] > 0), i  # the definition itself: equality is not a change
    for check_given, use_delta in ((0, 1), (1, 1), (1, 0), (0, 0)):
        prm.check_given, prm.use_delta = check_given, use_delta
        rows = ss.detect_all(img, lay, prm)
        for i, r in enumerate(rows):
            should, evaluated = _gate(want_changed[i], cached[i], check_given, in_check[i], use_delta)
            assert (bool(r[2]), bool(r[3]), bool(r[4])) == (want_changed[i], should, evaluated), (check_given, use_delta, i, r[2:5])
            if not evaluated:
                assert not r[0] and r[8] == 0.0 and r[9] == 0.0, i


# ---------------------------------------------------------------------------------------------------------------
# c. the uniformity pre-filter at a variance of exactly 225
# ---------------------------------------------------------------------------------------------------------------


def _decide(lib, st, shape, circle_threshold=0.6):
    out = N.PieceResult()
    assert lib.cbv_decide_piece(C.byref(st), None, shape[1], shape[0], circle_threshold, C.byref(out)) == 0
    has = bool(out.has_piece)
    return {"has_piece": has, "method": N.METHOD_NAMES[out.method], "center": (out.cx, out.cy) if has else None,
            "radius": out.radius if has else None, "confidence": out.confidence, "center_border_diff": out.center_border_diff}


def _same_decision(got, want, tag):
    for k in ("has_piece", "method", "center", "radius"):
        assert got[k] == want[k], (tag, k, got, want)
    for k in ("confidence", "center_border_diff"):
        assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), (tag, k, got, want)


def test_decisions_from_device_statistics_at_every_threshold(gpu_ctx):
    """Planes written by the test (set(GRAY)) at a variance of exactly 225 and one grey level of one pixel to either
    side, at a centre-vs-corner difference of exactly 40 and one step to either side, and at a symmetry score of exactly
    0.6 and one step to either side: the device's sums equal the definition's, and cbv_decide_piece on them gives what
    detect_piece gives on the pixels (np.std(gray) < 15 as numpy returns it for that very array)."""
    lib = gpu_ctx.lib
    for what, cases in (("std 15", RC.exact_225_squares()), ("diff 40", RC.center_diff_squares()), ("symmetry 0.6", RC.symmetry_squares())):
        lo, tie, hi = RC.sides(cases)
        print("%s: %d squares below, %d exactly at, %d above" % (what, lo, tie, hi))
        assert lo >= 3 and tie >= 3 and hi >= 3
        for part in _chunks(cases):
            ss = _with_planes(gpu_ctx, [g for _, g, _ in part])
            st = ss.stats()
            for i, (name, g, side) in enumerate(part):
                _same_stats(st[i], RR.stats(g), name)
                want = RR.detect_piece_no_hough(g)
                if what == "std 15":
                    assert RR.std_below_15(g) == (side < 0), name
                elif what == "diff 40":
                    assert (want["method"] == "center_diff") == (side > 0), name
                else:
                    assert (want["method"] == "symmetry") == (side > 0), name
                _same_decision(_decide(lib, st[i], g.shape), want, name)
            ss.close()


@pytest.mark.parametrize("cn", [3, 1], ids=["bgr", "gray"])
def test_detect_all_at_a_blurred_variance_of_exactly_225(gpu_ctx, cn):
    """detect_all_pieces preprocesses what it is given, so the squares here are images whose 5 x 5 blur has a variance of
    exactly 225, and their nearest single-pixel neighbours on either side.  Whether the square is evaluated past the
    uniformity pre-filter (HoughCircles listed, the statistics-based detectors run: a non-zero center_border_diff or a
    piece) must be what np.std(gray) < 15 returns in float64 for the blurred plane: for the two 10 x 10 ties numpy returns
    14.999999999999998, so they are uniform, while their exact variance is not below 225."""
    from chessboard_vision_amd._squares import GRAY, SquareSet
    cases = RC.blurred_225_images()
    lo, tie, hi = RC.sides(cases)
    print("std 15 behind the blur: %d squares below, %d exactly at, %d above" % (lo, tie, hi))
    assert lo >= 3 and tie >= 3 and hi >= 3
    board, img, lay = _pack([im for _, im, _ in cases], cn)
    ss = SquareSet(gpu_ctx)
    ss.adopt(lay)
    prm = N.DetectParams()
    prm.change_threshold, prm.circle_threshold, prm.use_delta = 25.0, 0.6, 1
    prm.hough = N.HoughParams(1.2, 100.0, 25.0, 0.2, 0.55)
    rows = ss.detect_all(img, lay, prm)
    st = ss.stats()
    numpy_uniform_at_tie = 0
    for i, (name, im, side) in enumerate(cases):
        g = R.gaussian_blur_u8(im, 5)
        assert np.array_equal(ss.get(GRAY, i), g), name
        n = g.size
        assert (RC.var_lhs(g) == 225 * n * n) == (side == 0) and (RC.var_lhs(g) < 225 * n * n) == (side < 0), name
        _same_stats(st[i], RR.stats(g), name)
        uniform = RR.std_below_15(g)
        numpy_uniform_at_tie += uniform and side == 0
        assert side == 0 or uniform == (side < 0), name
        want = RR.detect_piece_no_hough(g)
        assert uniform or want["center_border_diff"] != 0, name  # (else the row could not tell the two outcomes apart)
        has_piece, method, changed, should, evaluated, cx, cy, radius, conf, diff = rows[i]
        assert changed and should and evaluated
        assert (bool(has_piece) or diff != 0) == (not uniform), (name, rows[i], float(np.std(g)))
        if N.METHOD_NAMES[method] not in ("hough", "tower_top"):
            got = {"has_piece": bool(has_piece), "method": N.METHOD_NAMES[method], "center": (cx, cy) if has_piece else None,
                   "radius": radius if has_piece else None, "confidence": conf, "center_border_diff": diff}
            _same_decision(got, want, name)
    assert numpy_uniform_at_tie >= 1


def test_drop_in_detector_at_a_blurred_variance_of_exactly_225(gpu_ctx):
    """The same squares through PieceDetector.detect_piece (load, statistics and HoughCircles as separate calls, the
    decision in Python): has_piece is False exactly where np.std of the blurred plane is below 15."""
    from chessboard_vision_amd.piece_detector import PieceDetector
    det = PieceDetector()
    for name, im, side in RC.blurred_225_images():
        g = R.gaussian_blur_u8(im, 5)
        res = det.detect_piece(im)
        if RR.std_below_15(g):
            assert not res["has_piece"] and res["center_border_diff"] == 0 and res["method"] is None, name
        elif res["method"] not in ("hough", "tower_top"):
            want = RR.detect_piece_no_hough(g)
            assert {k: res[k] for k in want} == want, name


@pytest.mark.parametrize("cn", [3, 1], ids=["bgr", "gray"])
@pytest.mark.parametrize("blur", [5, 3])
def test_detect_changes_at_a_blurred_variance_of_exactly_225(gpu_ctx, cn, blur):
    """detect_changes_detailed reports every square here (the model's mean lies 100 grey levels from every pixel), so
    is_circular is detect_piece of the square preprocessed the PieceDetector way (k = 5, whatever the ChangeDetector's own
    blur): False where np.std of that plane is below 15, which includes the two ties numpy puts at 14.999999999999998
    although their centre-vs-corner difference is past 40, and detect_piece's answer everywhere else."""
    from chessboard_vision_amd._squares import GRAY, MEAN, SquareSet
    cases = RC.blurred_225_images()
    board, img, lay = _pack([im for _, im, _ in cases], cn)
    ss = SquareSet(gpu_ctx)
    ss.load_image(img, lay, blur)
    ss.calibrate(1.0)
    for i, (name, im, side) in enumerate(cases):
        g = R.gaussian_blur_u8(im, blur)
        assert np.array_equal(ss.get(GRAY, i), g), name
        ss.set(MEAN, i, g.astype(np.float32) + np.where(g < 128, np.float32(100), np.float32(-100)))
    cp = N.ChangeParams()
    cp.z_threshold, cp.select, cp.circle_threshold, cp.hough = 2.5, lay.all_mask, 0.6, N.HoughParams(*QUIET_HOUGH)
    rows = ss.detect_changes(img, lay, blur, cp)
    held_back, circular = 0, 0
    for i, (name, im, side) in enumerate(cases):
        g5 = R.gaussian_blur_u8(im, 5)
        want = RR.detect_piece_no_hough(g5)
        r_in, r_int, r_circ, r_zmax, r_zcount, r_n = rows[i]
        assert (bool(r_in), r_int, r_zcount) == (True, INTENSITY["TOTAL"], g5.size), (name, rows[i])
        assert bool(r_circ) == want["has_piece"], (name, rows[i], float(np.std(np.ascontiguousarray(g5))))
        held_back += side == 0 and RR.std_below_15(g5) and RR.center_border_diff(g5) > 40
        circular += want["has_piece"]
    print("variance exactly 225 and np.std below 15 with a difference past 40: %d squares; circular: %d" % (held_back, circular))
    assert held_back >= 2 and circular >= 3


def test_packed_view_path_at_a_blurred_variance_of_exactly_225(gpu_ctx):
    """The same squares as arrays that own their pixels (no common image: PieceDetector's packed-view path, with
    statistics and HoughCircles as separate calls and the decision in Python) through detect_all_pieces, and through
    calibrate_reference's cached results: uniform exactly where np.std of the blurred plane is below 15."""
    from chessboard_vision_amd.piece_detector import PieceDetector
    cases = RC.blurred_225_images()
    squares = {(i % 8, i // 8): im.copy() for i, (_, im, _) in enumerate(cases)}
    want = {}
    for (pos, _), (name, im, side) in zip(squares.items(), cases):
        want[pos] = RR.detect_piece_no_hough(R.gaussian_blur_u8(im, 5))
    for how in ("detect_all_pieces", "calibrate_reference"):
        det = PieceDetector()
        det.hough_param2 = QUIET_HOUGH[2]
        if how == "detect_all_pieces":
            results, visual = det.detect_all_pieces(squares)
            assert visual == set(squares)
        else:
            det.calibrate_reference(squares)
            results = det.cached_results
        held_back = 0
        for (pos, w_), (name, im, side) in zip(want.items(), cases):
            got = results[pos]
            assert {k: got[k] for k in w_} == w_, (how, name, got, w_)
            held_back += side == 0 and w_["method"] is None
        assert held_back >= 2, how


# ---------------------------------------------------------------------------------------------------------------
# d. ChangeDetector's classes at exact ties of the changed share
# ---------------------------------------------------------------------------------------------------------------

CHANGE_TIES = [((10, 10), (4, 5, 15, 16, 75, 76)), ((4, 5), (1, 3, 15)), ((5, 7), (1, 2, 5, 6, 26, 27))]


@pytest.mark.parametrize("cn", [3, 1], ids=["bgr", "gray"])
@pytest.mark.parametrize("blur", [5, 1])
def test_change_classes_at_exact_ties_of_the_changed_share(gpu_ctx, cn, blur):
    """detect_changes_detailed on squares of 100, 20 and 35 pixels of which exactly c pixels lie 100 grey levels from
    their background mean under a variance of 1: (5 / 100) * 100, (1 / 20) * 100, (15 / 100) * 100, (3 / 20) * 100,
    (75 / 100) * 100 and (15 / 20) * 100 are exactly 5.0, 15.0 and 75.0 as Python floats (3 / 20 and 15 / 100 are the same
    double), so those squares are LEVE, LEVE and PARCIAL; 4 and 16, 76 of 100 and the counts of 35 lie on either side.
    The model's mean is the plane the blur produced (checked against its definition)."""
    from chessboard_vision_amd._squares import GRAY, MEAN, SquareSet
    rng = np.random.default_rng(31)
    shapes, counts = [], []
    for shape, cs in CHANGE_TIES:
        for c in cs:
            shapes.append(shape)
            counts.append(c)
    board, img, lay = _pack([rng.integers(0, 256, s, dtype=np.uint8) for s in shapes], cn)
    ss = SquareSet(gpu_ctx)
    ss.load_image(img, lay, blur)
    ss.calibrate(1.0)
    means, grays = [], []
    for i, (shape, c) in enumerate(zip(shapes, counts)):
        x0, y0, w, h = lay.rects[i]
        src = board[y0:y0 + h, x0:x0 + w]
        g = R.gaussian_blur_u8(src[..., 0] if cn == 3 else src, blur)
        assert np.array_equal(ss.get(GRAY, i), g) and np.array_equal(ss.get(MEAN, i), g.astype(np.float32))
        mean = g.astype(np.float32).ravel()
        for j in rng.permutation(g.size)[:c]:
            mean[j] += np.float32(100 if mean[j] < 128 else -100)
        means.append(mean.reshape(shape))
        grays.append(g)
        ss.set(MEAN, i, means[i])
    prm = N.ChangeParams()
    prm.z_threshold, prm.select, prm.circle_threshold, prm.hough = 2.5, lay.all_mask, 0.6, N.HoughParams(1.2, 100.0, 25.0, 0.2, 0.55)
    rows = ss.detect_changes(img, lay, blur, prm)
    seen = {}
    for i, (shape, c) in enumerate(zip(shapes, counts)):
        z_count, pct, in_result, intensity = RR.change_class(grays[i].astype(np.float32), means[i], np.ones(shape, np.float32), 2.5)
        assert z_count == c, (shape, c)
        r_in, r_int, r_circ, r_zmax, r_zcount, r_n = rows[i]
        assert (r_zcount, r_n) == (c, grays[i].size), (shape, c, rows[i])
        assert (bool(r_in), r_int) == (in_result, INTENSITY[intensity]), (shape, c, pct, rows[i])
        seen[(grays[i].size, c)] = intensity
    print("changed share: " + ", ".join("%d/%d %s" % (c, n, v) for (n, c), v in sorted(seen.items())))
    assert seen == {(100, 4): None, (100, 5): "LEVE", (100, 15): "LEVE", (100, 16): "PARCIAL", (100, 75): "PARCIAL", (100, 76): "TOTAL",
                    (20, 1): "LEVE", (20, 3): "LEVE", (20, 15): "PARCIAL",
                    (35, 1): None, (35, 2): "LEVE", (35, 5): "LEVE", (35, 6): "PARCIAL", (35, 26): "PARCIAL", (35, 27): "TOTAL"}


# ---------------------------------------------------------------------------------------------------------------
# e. the pipeline's decision byte and scan
# ---------------------------------------------------------------------------------------------------------------

PIPE_W, PIPE_H, PIPE_S = 800, 400, 8 * RC.BOARD_SQ
QUAD_A = np.float32([[80, 40], [80 + PIPE_S, 40], [80, 40 + PIPE_S], [80 + PIPE_S, 40 + PIPE_S]])
QUAD_B = QUAD_A + np.float32([PIPE_S + 40, 0])
PIPE_SHIFTS = (0, 0, 0, 2, -2, 2)          # the ramps of the first three quarters move in the later frames: raw results flip
PIPE_PATCHES = (None, None, None, RC.PATCHES_A, None, RC.PATCHES_B)
PIPE_CONFIGS = {
    "one": dict(),
    "two": dict(),
    "thr12.5": dict(change_threshold=12.5),
    "presence": dict(min_presence=0.5, history_size=4),
}


def _pipe_offsets(thr):
    """grey levels added to the whole frame: frame 1 lies floor(thr) above frame 0 (for an integral threshold exactly at
    it: not changed), frame 2 one more (changed), and from then on every frame is far from the one before"""
    c = int(np.floor(thr))
    return (0, c, c + 1, 0, 2 * (c + 1), 0)


def _pipe_frames(thr, second):
    frames = []
    for t, off in enumerate(_pipe_offsets(thr)):
        f = np.full((PIPE_H, PIPE_W), 17, np.uint8)
        boards = [(QUAD_A, RC.board_image(PIPE_SHIFTS[t], PIPE_PATCHES[t]))]
        if second:
            other = RC.PATCHES_B if PIPE_PATCHES[t] is RC.PATCHES_A else (RC.PATCHES_A if PIPE_PATCHES[t] is RC.PATCHES_B else None)
            boards.append((QUAD_B, RC.board_image(PIPE_SHIFTS[t] + 1, other)))
        for quad, img in boards:
            x0, y0 = int(quad[0][0]), int(quad[0][1])
            f[y0:y0 + PIPE_S, x0:x0 + PIPE_S] = img
        assert int(f.max()) + off <= 255  # no saturation: the whole frame moves by `off`
        f = (f + off).astype(np.uint8)
        frames.append(np.ascontiguousarray(np.repeat(f[:, :, None], 3, axis=2)))
    return frames


class _RefScan:
    """detect_all_pieces(use_smoothing=True, use_delta=True, squares_to_check=None) (piece_detector.py:367-440) and
    detect_changes_detailed's classes (change_detector.py:128-150) over the frames of one board, from pixels, on
    ref_regions alone."""

    def __init__(self, n, thr, history_size, min_presence, z_thr, initial_variance):
        self.n, self.thr, self.hs, self.mp, self.z_thr, self.var0 = n, thr, history_size, min_presence, z_thr, initial_variance
        self.ref, self.cached, self.hist, self.model = {}, {}, {}, None
        self.seen = {"pct": [], "mean_diff": [], "presence": []}

    def calibrate(self, grays):
        self.model = [g.astype(np.float32) for g in grays]

    def frame(self, grays):
        masks = dict.fromkeys(("raw_occupied", "stable_occupied", "visual_changes", "processed", "changed", "parcial", "total", "circular"), 0)
        z_counts = []
        for i, g in enumerate(grays):
            bit = 1 << i
            fresh = RR.detect_piece_no_hough(g)
            changed = True
            if i in self.ref:
                changed = RR.has_changed(g, self.ref[i], self.thr)
                self.seen["mean_diff"].append(float(np.mean(np.abs(g.astype(np.int16) - self.ref[i].astype(np.int16)))))
            should = i not in self.cached or changed
            if should:
                self.cached[i] = fresh["has_piece"]
            raw = self.cached[i]
            hist = self.hist.setdefault(i, [])
            hist.append(raw)
            stable = RR.stable(hist, self.hs, self.mp)
            if len(hist) >= 3:
                kept = hist[-self.hs:]
                self.seen["presence"].append(sum(kept) / len(kept))
            if should and raw == stable:
                self.ref[i] = g.copy()
            masks["raw_occupied"] |= bit if raw else 0
            masks["stable_occupied"] |= bit if stable else 0
            masks["visual_changes"] |= bit if changed else 0
            masks["processed"] |= bit if should else 0
            z_count = 0
            if self.model is not None:
                z_count, pct, in_result, intensity = RR.change_class(g.astype(np.float32), self.model[i], np.full(g.shape, self.var0, np.float32), self.z_thr)
                self.seen["pct"].append((len(self.hist[i]) - 1, i, pct))  # (frame, square, share)
                if in_result:
                    masks["changed"] |= bit
                    masks["parcial"] |= bit if intensity == "PARCIAL" else 0
                    masks["total"] |= bit if intensity == "TOTAL" else 0
                    masks["circular"] |= bit if fresh["has_piece"] else 0
            z_counts.append(z_count)
        return masks, z_counts


def _split(board, rois, n):
    """the blurred gray squares of a downloaded warped board, by the pipeline's own square table"""
    gray = R.bgr2gray_q15(board)
    return [R.gaussian_blur_u8(gray[rois[i].y0:rois[i].y0 + rois[i].h, rois[i].x0:rois[i].x0 + rois[i].w], 5) for i in range(n)]


def _both_sides(values, thr, what, least=3):
    lo, at, hi = sum(v < thr for v in values), sum(v == thr for v in values), sum(v > thr for v in values)
    print("%s against %s: %d squares below, %d exactly at, %d above" % (what, thr, lo, at, hi))
    assert lo + at >= least and hi >= least, (what, thr, lo, at, hi)


@pytest.mark.parametrize("config", list(PIPE_CONFIGS))
def test_pipeline_decisions_and_scan_across_every_threshold(gpu_ctx, config):
    """Six frames of a board whose 64 squares each step one quantity across one threshold (np.std 15, centre-vs-corner
    difference 40, symmetry 0.6, the changed share 5 / 15 / 75 per cent), the whole frame moving by the change threshold
    (or to either side of 12.5) between frames: the statistics of every slot and all eight square sets of every frame's
    result equal a scan written from the reference's lines on the numpy definitions, fed with the squares of the warped
    board the pipeline itself holds.  With one board, with an attached second board, with change_threshold = 12.5 (the
    scan's non-integral comparison) and with min_presence = 0.5 over a history of 4."""
    from chessboard_vision_amd.stream import BoardPipeline
    kw = dict(history_size=5, min_presence=0.6, change_threshold=25, z_threshold=2.5, initial_variance=100)
    kw.update(PIPE_CONFIGS[config])
    thr = kw["change_threshold"]
    frames = _pipe_frames(thr, config == "two")
    p = BoardPipeline(PIPE_W, PIPE_H, len(frames))
    size = dict(display_size=(PIPE_S + 100, PIPE_S + 100), margin=100)
    p.configure(QUAD_A, enhance=False, use_hough=False, **size, **kw)
    boards = [p] + ([p.add_board(QUAD_B, use_hough=False, **size, **kw)] if config == "two" else [])
    for k, f in enumerate(frames):
        p.upload(k, f)
    p.run(0, 1)
    for b in boards:
        b.calibrate_changes(0)
    p.run(1, len(frames) - 1)
    for bi, b in enumerate(boards):
        n = len(b.rois_rc)
        assert n == 64 and b.board_size == PIPE_S
        rois = b._cfg.rois
        assert all((rois[i].w, rois[i].h) == (RC.BOARD_SQ, RC.BOARD_SQ) for i in range(n))
        scan = _RefScan(n, thr, kw["history_size"], kw["min_presence"], kw["z_threshold"], kw["initial_variance"])
        want, grays = [], []
        for t in range(len(frames)):
            grays.append(_split(b.download(2, t), rois, n))
            want.append(scan.frame(grays[t]))
            if t == 0:
                scan.calibrate(grays[0])
        # the conditions, from the reference side alone, before any answer of the pipeline is looked at
        off = _pipe_offsets(thr)
        for i in range(n):  # the whole frame moved by off[1]: every square's mean |gray - ref| is exactly that
            assert np.array_equal(grays[1][i].astype(np.int16) - grays[0][i], np.full(grays[0][i].shape, off[1]))
            assert float(np.mean(np.abs(grays[1][i].astype(np.int16) - grays[0][i]))) == float(off[1])
        if bi == 0:
            quarter = lambda q: [np.ascontiguousarray(grays[0][i]) for i in range(16 * q, 16 * q + 16)]
            _both_sides([float(np.std(g)) for g in quarter(0)], 15, "np.std")
            assert all(RR.center_border_diff(g) > 40 for g in quarter(0) if not RR.std_below_15(g))
            assert sum(1 for g in quarter(0) if RR.std_below_15(g) and RR.center_border_diff(g) > 40) >= 3  # only the pre-filter holds these back
            assert all(not RR.std_below_15(g) for g in quarter(1) + quarter(2))
            _both_sides([float(RR.center_border_diff(g)) for g in quarter(1)], 40, "centre-vs-corner difference")
            assert all(RR.radial_symmetry(g) <= 0.6 for g in quarter(1)) and all(RR.center_border_diff(g) <= 40 for g in quarter(2))
            _both_sides([float(RR.radial_symmetry(g)) for g in quarter(2)], 0.6, "symmetry")
            pcts = [pct for t, i, pct in scan.seen["pct"] if i >= 48 and PIPE_PATCHES[t] is not None]  # the patched frames, which lie at frame 0's level
            for edge in (5, 15, 75):
                _both_sides(pcts, edge, "changed share")
            _both_sides(scan.seen["mean_diff"], thr, "mean |gray - ref|", least=64)
            if thr == int(thr):
                assert scan.seen["mean_diff"][:64] == [float(thr)] * 64 and want[1][0]["visual_changes"] == 0  # equality is no change
            else:
                assert scan.seen["mean_diff"][:64] == [float(off[1])] * 64 and off[1] < thr < off[2]
                assert want[1][0]["visual_changes"] == 0 and want[2][0]["visual_changes"] == (1 << 64) - 1
            flips = sum(1 for i in range(n) if len(set((want[t][0]["raw_occupied"] >> i) & 1 for t in range(len(frames)))) == 2)
            differ = sum(1 for t in range(len(frames)) if want[t][0]["raw_occupied"] != want[t][0]["stable_occupied"])
            print("raw result flips on %d squares; stable differs from raw in %d frames" % (flips, differ))
            assert flips >= 3 and differ >= 1
            # the presence ratio sits exactly on min_presence for some (frame, square), and between 0.5 and 0.6 the two
            # settings of this test decide differently
            on_edge = sum(1 for r in scan.seen["presence"] if r == kw["min_presence"])
            between = sum(1 for r in scan.seen["presence"] if (r >= 0.5) != (r >= 0.6))
            print("presence ratio exactly %s on %d (frame, square) pairs; %d pairs where 0.5 and 0.6 decide differently" % (kw["min_presence"], on_edge, between))
            assert on_edge >= 1
            if kw["min_presence"] == 0.5:
                assert between >= 1
        res = b.results(0, len(frames))
        for t in range(len(frames)):
            masks, z_counts = want[t]
            st = b.square_stats(t)
            for i in range(n):
                ref_stats = RR.stats(grays[t][i])  # (sad_ref 0: the pipeline's record carries no reference sum, the scan
                ref_stats["z_count"] = z_counts[i]  # takes |gray - ref| itself and reports it as visual_changes)
                _same_stats(st[i], ref_stats, (config, bi, t, i))
            for name, value in masks.items():
                assert getattr(res[t], name) == value, (config, bi, t, name, hex(getattr(res[t], name)), hex(value))
    p.close()
