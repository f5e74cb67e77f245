"""The square regions (centre disc, corner region, four rings), the statistics over them and detect_piece's decision
against their numpy definitions from pixels (tests/ref_regions.py), on the host: the C oracle's masks and statistics at
every shape of the sweep, and cbv_decide_piece on squares that sit at and next to every threshold of the chain."""
import ctypes as C

import numpy as np
import pytest

import ref_regions as RR
import region_cases as RC
from chessboard_vision_amd import _native as N


def test_oracle_masks_match_numpy_slices_at_every_shape(oracle):
    """orc_piece_masks == the reference's numpy expressions at all 128 x 128 shapes; with a short side below 4 the corner
    size is 0 and `border_mask[-0:, -0:] = True` selects the whole square."""
    whole = 0
    for h in range(1, 129):
        for w in range(1, 129):
            m = oracle.piece_masks(w, h)
            centre, border, rings = RR.masks(h, w)
            assert np.array_equal((m & 1) != 0, centre), ("centre", h, w)
            assert np.array_equal((m & 2) != 0, border), ("border", h, w)
            for k in range(4):
                assert np.array_equal((m & (4 << k)) != 0, rings[k]), ("ring", k, h, w)
            if min(h, w) < 4:
                assert border.all()
                whole += 1
    assert whole == 128 * 128 - 125 * 125


def test_oracle_statistics_match_numpy_at_every_shape(oracle):
    """orc_square_stats (sums, counts, |gray - ref|, z count) == ref_regions.stats on random pixels at every shape of the
    sweep; the model's mean is the square itself moved by 0 or 3 grey levels under a variance of 1 (z = 0 or 3 > 2.5)."""
    rng = np.random.default_rng(17)
    for h in RC.SWEEP_H:
        for w in RC.SWEEP_W:
            g = rng.integers(0, 256, (h, w), dtype=np.uint8)
            ref = rng.integers(0, 256, (h, w), dtype=np.uint8)
            mean = g.astype(np.float32) + 3 * rng.integers(0, 2, (h, w)).astype(np.float32)
            var = np.ones((h, w), np.float32)
            got = RR.stats_of_struct(oracle.square_stats(g, ref=ref, mean=mean, var=var, z_thresh=2.5))
            assert got == RR.stats(g, ref=ref, mean=mean, var=var, z_thr=2.5), (h, w)


def _sq_stats(d):
    st = N.SqStats()
    for k in RR.INT_FIELDS:
        setattr(st, k, d[k])
    for k in range(4):
        st.ring_sum[k], st.ring_cnt[k] = d["ring_sum"][k], d["ring_cnt"][k]
    return st


def decide(lib, gray, circle_threshold=0.6):
    """cbv_decide_piece on the numpy statistics of `gray`, as detect_piece_no_hough's dict."""
    h, w = gray.shape
    st = _sq_stats(RR.stats(gray))
    out = N.PieceResult()
    assert lib.cbv_decide_piece(C.byref(st), None, w, h, circle_threshold, C.byref(out)) == 0
    has = bool(out.has_piece)
    return {"has_piece": has, "method": N.METHOD_NAMES[out.method], "center": (out.cx, out.cy) if has else None,
            "radius": out.radius if has else None, "confidence": out.confidence, "center_border_diff": out.center_border_diff}


def _same(got, want, tag):
    for k in ("has_piece", "method", "center", "radius"):
        assert got[k] == want[k], (tag, k, got, want)
    for k in ("confidence", "center_border_diff"):  # bit for bit
        assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), (tag, k, got, want)


def test_decide_piece_on_every_shape_class():
    """cbv_decide_piece on the numpy statistics of random and all-white squares of every shape class, the short sides
    below 4 included, where the border region is the whole square, the border mean a number and center_diff can fire.
    The statistics are ref_regions' own, so this holds the decision arithmetic to numpy and says nothing about the
    library's mask: build_piece_mask has no host entry point, its counts are checked on the GPU
    (tests/test_gpu_regions.py); on the host only the oracle's twin is (test_oracle_masks_match_numpy_slices_at_every_shape)."""
    lib = N.load()
    methods = set()
    fired_small = 0
    for name, g in RC.random_squares():
        want = RR.detect_piece_no_hough(g)
        _same(decide(lib, g), want, name)
        methods.add(want["method"])
        if min(g.shape) < 4 and not RR.std_below_15(g):
            assert not np.isnan(want["center_border_diff"]), name
            fired_small += want["method"] == "center_diff"
    assert "center_diff" in methods and None in methods
    assert fired_small >= 1  # center_diff does fire on a square with a short side below 4


def test_decide_piece_at_variance_exactly_225():
    """np.std(gray) < 15 as numpy evaluates it on the array against the product's integer test, at variance exactly 225
    and one grey level of one pixel to either side."""
    lib = N.load()
    cases = RC.exact_225_squares()
    lo, tie, hi = RC.sides(cases)
    print("std 15: %d squares below, %d exactly at, %d above" % (lo, tie, hi))
    assert lo >= 3 and tie >= 3 and hi >= 3
    for name, g, side in cases:
        assert RR.std_below_15(g) == (side < 0), name  # numpy agrees with the exact variance on every one of these
        _same(decide(lib, g), RR.detect_piece_no_hough(g), name)


def test_decide_piece_at_center_border_difference_40():
    lib = N.load()
    cases = RC.center_diff_squares()
    lo, tie, hi = RC.sides(cases)
    print("diff 40: %d squares below, %d exactly at, %d above" % (lo, tie, hi))
    assert lo >= 3 and tie >= 3 and hi >= 3
    for name, g, side in cases:
        want = RR.detect_piece_no_hough(g)
        assert (want["method"] == "center_diff") == (side > 0), name
        _same(decide(lib, g), want, name)


@pytest.mark.parametrize("circle_threshold", [0.6, 0.5])
def test_decide_piece_at_symmetry_threshold(circle_threshold):
    lib = N.load()
    cases = RC.symmetry_squares()
    lo, tie, hi = RC.sides(cases)
    print("symmetry 0.6: %d squares below, %d exactly at, %d above" % (lo, tie, hi))
    assert lo >= 3 and tie >= 3 and hi >= 3
    for name, g, side in cases:
        want = RR.detect_piece_no_hough(g, circle_threshold)
        if circle_threshold == 0.6:
            assert (want["method"] == "symmetry") == (side > 0), name
        else:
            assert want["method"] == "symmetry", name
        _same(decide(lib, g, circle_threshold), want, name)


def test_np_std_below_15_is_numpy_bit_for_bit():
    """cbv_np_std_below_15, which the one-call entry points ask at a variance of exactly 225, returns np.std's float64
    value bit for bit: on every exact tie of the case lists (among them two blurred 10 x 10 squares for which numpy returns
    14.999999999999998 although the variance is exactly 225), on their neighbours and on random squares of every size
    class of numpy's summation (below 8 elements, up to 128, above, and beyond one 8192-element chunk)."""
    import ref64 as R
    lib = N.load()
    rng = np.random.default_rng(23)
    arrays = [g for _, g, _ in RC.exact_225_squares()] + [R.gaussian_blur_u8(im, 5) for _, im, _ in RC.blurred_225_images()]
    for n in list(range(1, 40)) + [127, 128, 129, 255, 256, 1000, 5929, 8191, 8192, 8193, 8200, 12345, 16383, 16384]:
        arrays.append(rng.integers(0, 256, n, dtype=np.uint8))
        arrays.append((rng.integers(0, 4, n) * 20 + 90).astype(np.uint8))
    below_at_tie = 0
    for a in arrays:
        a = np.ascontiguousarray(a)
        sd = C.c_double()
        rc = lib.cbv_np_std_below_15(a.ctypes.data, a.size, C.byref(sd))
        want = np.std(a)
        assert np.float64(sd.value).tobytes() == np.float64(want).tobytes(), (a.shape, sd.value, float(want))
        assert rc == int(want < 15)
        below_at_tie += rc == 1 and RC.var_lhs(a) == 225 * a.size * a.size
    assert below_at_tie >= 1
    assert lib.cbv_np_std_below_15(None, 4, None) == -1
