"""Gray squares (uint8, already preprocessed) that put each comparison of detect_piece at or next to its threshold, shared
by tests/test_regions_host.py and tests/test_gpu_regions.py.  Every builder asserts, with numpy on the array itself,
that the square is where its name says; nothing here reads the oracle or the library."""
import numpy as np

import ref_regions as RR

# (h, w): short side 1, 2, 3 (corner 0: the border region is the whole square) and 4 (corner 1), odd and even centres,
# rings that are empty, full or clipped by the short side, and the largest square (u32 sumsq at its maximum)
SHAPES = [(1, 1), (1, 7), (2, 128), (3, 3), (3, 128), (128, 3), (4, 4), (5, 7), (7, 5), (8, 8), (39, 40), (40, 40), (41, 40), (77, 80),
          (127, 128), (128, 128)]

# the host sweep of the masks: every height against these widths
SWEEP_W = list(range(1, 20)) + [31, 32, 33, 64, 77, 100, 127, 128]
SWEEP_H = list(range(1, 129))


def random_squares(seed=3):
    """One random square per shape, and the all-255 square of every shape (128 x 128 of 255 is the largest sumsq)."""
    rng = np.random.default_rng(seed)
    out = [("random %dx%d" % s, rng.integers(0, 256, s, dtype=np.uint8)) for s in SHAPES]
    out += [("white %dx%d" % s, np.full(s, 255, np.uint8)) for s in SHAPES]
    return out


def var_lhs(g):
    """n * sum(x^2) - sum(x)^2 in exact integers: equals 225 n^2 iff the variance is exactly 225."""
    x = g.astype(np.int64).ravel()
    return int(x.size) * int((x * x).sum()) - int(x.sum()) ** 2


# three-valued 6 x 11 squares of variance exactly 225: values u, u + p, u + q on a, b, c pixels (a + b + c = 66); their
# mean is no dyadic rational, so numpy's float64 mean and deviations are rounded (the two-valued family below is exact)
THREE_VALUED = [(3, 33, 6, 33, 27), (6, 33, 15, 11, 40), (6, 36, 11, 33, 22), (9, 75, 22, 41, 3), (10, 55, 3, 55, 8), (12, 66, 6, 55, 5),
                (14, 36, 22, 21, 23), (15, 37, 22, 23, 21), (18, 40, 11, 1, 54), (18, 55, 1, 11, 54), (21, 99, 32, 33, 1), (22, 34, 21, 12, 33)]


def exact_225_squares(seed=5):
    """[(name, gray, side)]: side 0 = variance exactly 225, -1 / +1 = one pixel moved by one grey level so that the
    variance falls below / rises above 225."""
    rng = np.random.default_rng(seed)
    out = []

    def add(name, base):
        n = base.size
        assert var_lhs(base) == 225 * n * n, name
        out.append((name, base, 0))
        flat = base.ravel()
        lo_i, hi_i = int(np.argmin(flat)), int(np.argmax(flat))
        for side, idx, step in ((-1, lo_i, 1), (-1, hi_i, -1), (1, lo_i, -1), (1, hi_i, 1)):
            v = int(flat[idx]) + step
            if not 0 <= v <= 255:
                continue
            g = base.copy()
            g.ravel()[idx] = v
            assert (var_lhs(g) < 225 * n * n) == (side < 0) and var_lhs(g) != 225 * n * n, name
            out.append(("%s %+d at %s" % (name, step, "min" if idx == lo_i else "max"), g, side))

    for (h, w) in ((1, 2), (2, 2), (3, 128), (4, 4), (5, 8), (6, 11), (40, 40), (77, 80), (128, 128)):
        n = h * w
        for u in (0, 101, 225):
            vals = np.array([u] * (n // 2) + [u + 30] * (n // 2), np.uint8)
            add("half %d / %d %dx%d sorted" % (u, u + 30, h, w), vals.reshape(h, w))
            add("half %d / %d %dx%d shuffled" % (u, u + 30, h, w), rng.permutation(vals).reshape(h, w))
    for (p, q, a, b, c) in THREE_VALUED:
        for u in (0, 100, 255 - q):
            vals = np.array([u] * a + [u + p] * b + [u + q] * c, np.uint8)
            add("three-valued +%d +%d x(%d, %d, %d) from %d" % (p, q, a, b, c, u), rng.permutation(vals).reshape(6, 11))
    return out


def _filler(h, w, lo, hi):
    """a checkerboard of two values: enough variance to pass the uniformity pre-filter"""
    yy, xx = np.ogrid[:h, :w]
    return np.where((yy + xx) % 2 == 0, lo, hi).astype(np.uint8)


def center_diff_squares():
    """[(name, gray, side)]: flat centre disc and flat corners whose means differ by exactly 40 (side 0), and by
    40 -/+ 1 / count after one pixel of the centre disc or of the corners moved by one grey level."""
    out = []
    for (h, w) in ((8, 8), (5, 7), (40, 40), (41, 40), (77, 80), (128, 128)):
        centre, border, _ = RR.masks(h, w)
        assert not (centre & border).any()
        for (cv, bv) in ((140, 100), (60, 100), (255, 215), (0, 40)):
            base = _filler(h, w, 10, 240)
            base[centre] = cv
            base[border] = bv
            assert not RR.std_below_15(base)
            assert RR.center_border_diff(base) == 40.0
            out.append(("centre %d corners %d %dx%d" % (cv, bv, h, w), base, 0))
            sign = 1 if cv > bv else -1
            for region, name in ((centre, "centre"), (border, "corner")):
                for step in (-1, 1):
                    g = base.copy()
                    idx = tuple(np.argwhere(region)[0])
                    v = int(g[idx]) + step
                    if not 0 <= v <= 255:
                        continue
                    g[idx] = v
                    side = step * sign * (1 if region is centre else -1)
                    d = RR.center_border_diff(g)
                    assert (d > 40) == (side > 0) and d != 40.0 and abs(d - 40) < 1.5 / min(centre.sum(), border.sum())
                    out.append(("centre %d corners %d %dx%d, one %s pixel %+d" % (cv, bv, h, w, name, step), g, side))
    return out


def symmetry_squares():
    """[(name, gray, side)]: squares large enough for four disjoint rings, three flat rings at one value and one 40 above
    or below: np.var of the ring means is exactly 300 and 300 / 500 is the double 0.6 (side 0); one pixel of the odd ring
    moved by one grey level puts the score on either side.  The centre-vs-corner difference stays at or below 40."""
    out = []
    for (h, w) in ((128, 128), (127, 128), (128, 120)):
        centre, border, rings = RR.masks(h, w)
        for a in range(4):
            for b in range(a + 1, 4):
                assert not (rings[a] & rings[b]).any()
        for base_v, odd_v in ((100, 140), (140, 100), (0, 40), (255, 215)):
            base = np.full((h, w), base_v, np.uint8)
            base[rings[3]] = odd_v
            assert not RR.std_below_15(base) and RR.center_border_diff(base) <= 40
            assert RR.radial_symmetry(base) == 0.6
            out.append(("rings %d, outer %d %dx%d" % (base_v, odd_v, h, w), base, 0))
            idx = tuple(np.argwhere(rings[3])[0])
            for step in (-1, 1):
                v = odd_v + step
                if not 0 <= v <= 255:
                    continue
                g = base.copy()
                g[idx] = v
                side = step * (1 if odd_v > base_v else -1)
                s = RR.radial_symmetry(g)
                assert (s > 0.6) == (side > 0) and s != 0.6 and abs(s - 0.6) < 1e-3
                assert not RR.std_below_15(g) and RR.center_border_diff(g) <= 40
                out.append(("rings %d, outer %d %dx%d, one pixel %+d" % (base_v, odd_v, h, w, step), g, side))
    return out


def sides(cases):
    """how many squares lie below / at / above the threshold"""
    return tuple(sum(1 for c in cases if c[2] == s) for s in (-1, 0, 1))


# Unblurred gray squares whose 5 x 5 Gaussian blur (on the square alone, BORDER_REFLECT_101) has variance exactly 225:
# found by a hill climb on single pixels, kept as they are.  detect_all_pieces preprocesses what it is given, so the
# uniformity test of its gate can only be put on the tie through an image like these.
BLUR_TIES = [
    [[40, 50, 45, 41, 49, 46], [37, 46, 38, 92, 51, 35], [30, 40, 106, 105, 99, 50], [50, 105, 101, 108, 104, 107], [48, 37, 108, 103, 104, 50],
     [38, 45, 41, 106, 48, 44]],
    [[139, 134, 142, 129, 133, 132], [137, 133, 141, 193, 132, 137], [132, 128, 195, 198, 194, 138], [125, 203, 190, 194, 196, 193],
     [138, 136, 200, 200, 195, 142], [133, 128, 138, 203, 142, 131]],
    [[99, 89, 89, 108, 94, 100, 79, 113], [96, 86, 97, 90, 105, 109, 90, 101], [102, 93, 99, 116, 148, 118, 109, 104],
     [100, 94, 110, 144, 175, 153, 108, 109], [89, 101, 167, 156, 143, 157, 154, 114], [82, 90, 105, 162, 148, 143, 111, 93],
     [88, 92, 96, 108, 157, 102, 85, 95], [88, 106, 104, 99, 112, 107, 82, 98]],
    [[75, 77, 76, 83, 75, 86, 77, 75, 83, 73, 81], [78, 71, 74, 82, 84, 133, 82, 78, 77, 79, 75], [71, 83, 80, 79, 131, 132, 140, 76, 72, 75, 76],
     [77, 77, 73, 132, 135, 134, 131, 135, 76, 74, 79], [83, 74, 71, 87, 137, 138, 133, 81, 78, 85, 74], [84, 77, 86, 81, 76, 139, 77, 81, 77, 81, 63]],
    [[164, 155, 161, 181, 188, 169, 168, 157], [166, 171, 170, 190, 251, 176, 170, 161], [178, 169, 183, 245, 251, 234, 178, 157],
     [163, 165, 177, 201, 242, 201, 167, 155], [163, 162, 164, 185, 191, 183, 177, 170]],
    [[32, 23, 26, 37, 40, 38, 40, 29], [28, 7, 27, 40, 105, 42, 29, 35], [34, 23, 27, 106, 107, 110, 45, 24], [30, 10, 30, 42, 116, 36, 28, 29],
     [29, 19, 15, 48, 38, 34, 26, 21]],
    # the next two: np.std of the blurred plane (rows after rows in memory) is 14.999999999999998, below 15 at a variance of 225
    [[29, 40, 27, 33, 36, 33, 31, 33, 28, 42], [37, 36, 29, 36, 29, 35, 32, 32, 35, 33], [33, 35, 27, 36, 31, 89, 32, 31, 33, 42],
     [31, 29, 35, 85, 82, 75, 91, 85, 33, 38], [33, 26, 36, 80, 74, 83, 83, 74, 32, 32], [39, 38, 85, 77, 80, 82, 81, 80, 82, 26],
     [32, 27, 37, 80, 82, 77, 88, 78, 33, 28], [32, 36, 34, 81, 90, 88, 89, 78, 29, 36], [32, 32, 33, 38, 25, 87, 25, 30, 28, 37],
     [32, 38, 31, 41, 32, 34, 36, 45, 35, 27]],
    [[58, 56, 64, 61, 58, 51, 60, 63, 52, 54], [53, 53, 60, 57, 58, 62, 59, 60, 54, 62], [60, 51, 58, 66, 62, 101, 52, 57, 60, 67],
     [55, 63, 53, 112, 104, 105, 106, 110, 55, 47], [59, 50, 50, 107, 106, 107, 106, 109, 56, 56], [62, 62, 108, 113, 110, 105, 102, 100, 108, 66],
     [65, 53, 56, 102, 104, 104, 103, 102, 54, 50], [57, 59, 63, 99, 112, 112, 113, 110, 66, 59], [63, 54, 55, 55, 57, 114, 52, 58, 58, 66],
     [58, 60, 56, 52, 62, 54, 55, 48, 63, 57]],
]


_BLURRED_225 = []


def blurred_225_images():
    """[(name, image, side)]: the images of BLUR_TIES (side 0) and, for each, the two single-pixel changes of at most
    three grey levels whose blurred variance comes closest to 225 from below (-1) and from above (+1)."""
    import ref64 as R
    if _BLURRED_225:  # (the neighbour search runs once per process)
        return list(_BLURRED_225)
    out = []
    for k, rows in enumerate(BLUR_TIES):
        img = np.array(rows, np.uint8)
        n = img.size
        target = 225 * n * n
        assert var_lhs(R.gaussian_blur_u8(img, 5)) == target, k
        out.append(("blur tie %d (%dx%d)" % (k, img.shape[0], img.shape[1]), img, 0))
        best = {-1: None, 1: None}
        for y in range(img.shape[0]):
            for x in range(img.shape[1]):
                for d in (-3, -2, -1, 1, 2, 3):
                    v = int(img[y, x]) + d
                    if not 0 <= v <= 255:
                        continue
                    cand = img.copy()
                    cand[y, x] = v
                    off = var_lhs(R.gaussian_blur_u8(cand, 5)) - target
                    if off == 0:
                        continue
                    side = -1 if off < 0 else 1
                    if best[side] is None or abs(off) < best[side][0]:
                        best[side] = (abs(off), cand, (y, x, d))
        for side in (-1, 1):
            assert best[side] is not None, (k, side)
            out.append(("blur tie %d, pixel (%d, %d) %+d" % ((k,) + best[side][2]), best[side][1], side))
    _BLURRED_225.extend(out)
    return out


# ---------------------------------------------------------------------------------------------------------------
# A board of 8 x 8 squares of 40 x 40 pixels for the pipeline: every square steps one quantity across one threshold
# ---------------------------------------------------------------------------------------------------------------
BOARD_SQ = 40
# bright patches (w, h) of the last quarter's squares, sets A and B: the share of pixels the blurred patch pushes past
# z = 2.5 runs from below 5 to above 75 per cent
PATCHES_A = [(5, 5), (7, 6), (8, 7), (8, 9), (9, 9), (10, 10), (13, 12), (14, 14), (15, 15), (17, 17), (20, 20), (28, 28), (33, 33), (34, 34), (36, 36), (40, 40)]
PATCHES_B = [(4, 4), (6, 6), (7, 7), (9, 8), (10, 9), (11, 10), (13, 13), (14, 13), (15, 14), (16, 16), (24, 24), (30, 30), (32, 33), (35, 34), (38, 38), (40, 39)]


def board_square(quarter, k, patch=None):
    """The 40 x 40 gray square number k (any integer; 0..15 on the board) of a quarter:
    0: centre disc above and corners below a flat square by about 19 + k / 2 each: np.std crosses 15 along k, and where
       it is past 15 the centre-vs-corner difference is past 40 (a piece only if the pre-filter lets it through);
    1: left and right halves 30 apart (std well past 15), centre disc 33 + k above: the difference crosses 40;
    2: the same halves, centre disc and corners both 60 + k above: no difference, np.var of the ring means crosses 300;
    3: the halves alone; `patch` = (w, h) adds a block of + 100 at the top left."""
    s = BOARD_SQ
    centre, border, _ = RR.masks(s, s)
    g = np.full((s, s), 60 if quarter == 0 else 30, np.int64)
    if quarter != 0:
        g[:, s // 2:] += 30
    if quarter == 0:
        x2 = 38 + k  # a + b
        g[centre] += (x2 + 1) // 2
        g[border] -= x2 // 2
    elif quarter == 1:
        g[centre] += 33 + k
    elif quarter == 2:
        g[centre] += 60 + k
        g[border] += 60 + k
    if patch is not None:
        g[:patch[1], :patch[0]] += 100
    assert g.min() >= 0 and g.max() <= 255 - 60
    return g.astype(np.uint8)


def board_image(shift=0, patches=None):
    """The 320 x 320 gray board: ROI 8 * row + col is square k = (8 * row + col) % 16 of quarter (8 * row + col) // 16, the
    first three quarters `shift` steps further along their ramps; `patches`: the last quarter's blocks."""
    s = BOARD_SQ
    out = np.zeros((8 * s, 8 * s), np.uint8)
    for i in range(64):
        q, k = divmod(i, 16)
        sq = board_square(q, k + (shift if q < 3 else 0), patches[k] if (q == 3 and patches is not None) else None)
        out[(i // 8) * s:(i // 8 + 1) * s, (i % 8) * s:(i % 8 + 1) * s] = sq
    return out
