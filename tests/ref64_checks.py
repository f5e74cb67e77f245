"""Inputs and envelope checks shared by the float64-reference tests (test_ref64_oracle.py on the CPU oracle,
test_gpu_ref64.py on the HIP kernels): one checker per stage, fed the 8-bit output under test and the stage's input,
computing the expected value with tests/ref64.py only.

Every bound is derived from how the 8-bit operation is computed (rounding once, float32 accumulation, fixed-point
tables, 1/32-pixel warp coordinates), not fitted to a measurement; each constant says where it comes from.
A checker returns a small dict of statistics (max |out - ref|, share of values more than 1 LSB off, ties) so the
envelope table in DESIGN.md can be regenerated from the same code.
"""
import functools

import numpy as np

import ref64 as R

U32 = 2.0 ** -24                 # float32 unit roundoff
TIE_SHARE_CAP = 0.5              # more values than this on a .5 tie (either neighbour passes) and a check pins only +-1
LAB_MAX = 3.0                    # 8-bit Lab: 12/15-bit fixed-point tables and a 3072-entry cube-root table
LAB_SHARE_OVER_1 = 0.005         # ... off the float64 definition by more than 1 LSB on at most 0.5 % of values
WARP_SLACK = 0.05                # on top of 0.5 + (Gx + Gy)/64: float64 coordinate noise across a 1/32 boundary


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------


def smooth(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    img = np.empty((h, w, 3))
    for c in range(3):
        fx, fy, ph = rng.uniform(0.5, 3), rng.uniform(0.5, 3), rng.uniform(0, 6.28)
        img[..., c] = 127 + 110 * np.sin(fx * xx / max(w, 1) * 6.28 + ph) * np.cos(fy * yy / max(h, 1) * 6.28)
    img += rng.normal(0, 4, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def const(w, h, seed):
    return np.full((h, w, 3), (37 + seed) % 256, np.uint8)


def edges(w, h, seed):
    """0/255 in every channel, in blocks and a diagonal: the largest colour distance the bilateral can see."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    cell = int(rng.integers(1, 6))
    m = (((yy // cell) + (xx // cell)) % 2 == 0) ^ (xx * h > yy * w)
    return np.repeat((m * 255).astype(np.uint8)[..., None], 3, axis=2)


CONTENTS = {"smooth": smooth, "noise": noise, "const": const, "edges": edges}

# (w, h): the fixture sizes, 1xN / Nx1, sizes below the bilateral radius and the CLAHE grid, every width residue mod 4
SHAPES = [(96, 72), (160, 120), (37, 29), (13, 1), (1, 11), (3, 2), (3, 5), (7, 1), (61, 9), (62, 9), (63, 9), (64, 9)]


def view(img, seed=0):
    """The same pixels as a strided view (row stride larger than the row, start off alignment)."""
    h, w = img.shape[:2]
    big = np.random.default_rng(seed).integers(0, 256, (h, w + 7) + img.shape[2:], dtype=np.uint8)
    v = big[:, 3:3 + w]
    v[...] = img
    return v


def frame(content, w, h, seed=0):
    return CONTENTS[content](w, h, seed + 7 * w + 13 * h)


# ---------------------------------------------------------------------------------------------------------------
# inputs of the detector-side checks (GaussianBlur k = 1..31 on squares, Canny)
# ---------------------------------------------------------------------------------------------------------------

BLUR_KS = list(range(1, 32, 2))
# h x w (x 3 = BGR): smaller than the radius in one or both axes (reflection repeats), either side of the 16-lane column
# grid and of the row step, and the largest square the library takes
SQUARE_SHAPES = [(128, 128, 3), (1, 1), (5, 7, 3), (77, 80), (3, 128, 3), (128, 2), (16, 15), (1, 31), (17, 16, 3), (15, 33)]


def ramp(w, h, seed):
    yy, xx = np.mgrid[:h, :w]
    v = (xx * (2 + seed % 3) + yy * 3 + seed) % 512
    return np.repeat(np.where(v > 255, 511 - v, v).astype(np.uint8)[..., None], 3, axis=2)


def white(w, h, seed):
    return np.full((h, w, 3), 255, np.uint8)


SQUARE_CONTENTS = {"noise": noise, "ramp": ramp, "white": white, "edges": edges}


def blur_squares():
    """{(shape index, content): uint8 square} for every SQUARE_SHAPES x SQUARE_CONTENTS: 40 squares, one SquareSet."""
    out = {}
    for i, s in enumerate(SQUARE_SHAPES):
        for c, fn in SQUARE_CONTENTS.items():
            img = fn(s[1], s[0], 100 + i)
            out[(i, c)] = img if len(s) == 3 else img[..., 1].copy()
    return out


CANNY_SHAPES = [(131, 257), (64, 64), (65, 129), (5, 7), (1, 40), (40, 1), (2, 2), (200, 193)]          # h x w
CANNY_THRESHOLDS = [(30, 100), (50, 150), (150, 50), (50.5, 149.9)]
CANNY_TIE_CAP = {"texture": 0.02, "noise": 0.02, "poster": None}


def canny_input(content, h, w):
    """texture: the waves-and-checkers image of test_gpu_stages.test_canny_matches_oracle under the 5 x 5 blur (of this
    module's reference); noise: white noise; poster: the texture in 8 levels (plateaus: many equal magnitudes)."""
    rng = np.random.default_rng(h * 7 + w)
    if content == "noise":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    img = (96 + 60 * np.sin(xx / 9.0) * np.cos(yy / 13.0) + 50 * ((xx // 40 + yy // 40) % 2)).astype(np.float64)
    img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
    g = R.gaussian_blur_u8(img, 5) if min(h, w) >= 5 else img
    return g if content == "texture" else (g // 32 * 32).astype(np.uint8)


def canny_cases():
    return [(h, w, c, t) for (h, w) in CANNY_SHAPES for c in CANNY_TIE_CAP for t in CANNY_THRESHOLDS]


def canny_tie_cap(content, h, w):
    """The cap on the share of pixels where hyst(loose) and hyst(strict) differ: 2 % for texture and noise.  It is a share,
    so it binds only where one tied pixel is less than the cap (h * w >= 50); smaller images run without it, as the
    posterised ones do, and are held by the exact comparison alone."""
    cap = CANNY_TIE_CAP[content]
    return cap if cap is not None and h * w * cap >= 1 else None


# One weak curve across the 64 x 64 hysteresis tiles of a 130 x 197 image: the boundary y = 64 + 30 sin(x / 10) between
# gray 100 and 100 + a.  A step of height a gives M = 4a on a straight stretch and up to 6a on a diagonal one, so a = 10
# stays inside (20, 80] everywhere; over the 10 columns at one end a = 30 (M >= 120 > 80) and falls back to 10 over the next 12.
CURVE_SHAPE = (130, 197)
CURVE_THRESHOLDS = (20, 80)


def hysteresis_curve(end):
    """end = "left" / "right": where the strong stretch lies; None: no strong stretch at all."""
    h, w = CURVE_SHAPE
    yy, xx = np.mgrid[:h, :w]
    x = np.arange(w)
    d = {"left": x, "right": w - 1 - x, None: np.full(w, 1000)}[end]    # distance from the strong end
    a = np.where(d < 10, 30.0, np.clip(10 + (22 - d) * 20 / 12.0, 10, 30))
    return np.rint(np.where(yy > 64 + 30 * np.sin(xx / 10.0), 100 + a[None, :], 100)).astype(np.uint8)


def check_hysteresis_curve(edges, end):
    """First the case itself, on the reference alone: the curve crosses x = 64, x = 128 and y = 64 at least six times, all of
    it is weak except at the one end, hyst(conv) holds more than half of its pixels and reaches the far end, and without the
    strong stretch nothing is an edge.  Then the output under test equals hyst(conv)."""
    h, w = CURVE_SHAPE
    gray = hysteresis_curve(end)
    M, low, high, _, _, cand = R.canny_candidates(gray, *CURVE_THRESHOLDS)
    yc = 64 + 30 * np.sin(np.arange(w) / 10.0)
    assert int((np.diff(np.sign(yc - 64.0)) != 0).sum()) + 2 >= 6                     # y = 64, plus x = 64 and x = 128
    strong_cols = np.nonzero((cand & (M > high)).any(axis=0))[0]
    assert len(strong_cols) and (strong_cols.max() < 24 if end == "left" else strong_cols.min() > w - 25), strong_cols
    conv = R.canny_sets(gray, *CURVE_THRESHOLDS)[2]
    assert conv.sum() > cand.sum() / 2 and cand.sum() > 300, (int(conv.sum()), int(cand.sum()))
    cols = np.nonzero(conv.any(axis=0))[0]
    assert cols.min() == 0 and cols.max() == w - 1
    assert conv[:64].any() and conv[64:128].any() and all(conv[:, a:b].any() for a, b in ((0, 64), (64, 128), (128, w)))
    assert not R.canny_sets(hysteresis_curve(None), *CURVE_THRESHOLDS)[1].any()
    edges = np.asarray(edges)
    assert np.isin(edges, (0, 255)).all()
    diff = int(((edges > 0) != conv).sum())
    assert diff == 0, "weak curve, strong stretch at the %s end: %d of %d curve pixels differ" % (end, diff, int(conv.sum()))
    return {"edges": int(conv.sum())}


# Horizontal steps whose magnitude sits exactly on a threshold.  M is always even (dx + dy is), and a straight step of
# height a has M = 4a.  threshold_step(): gray 100 above row 20, below it 130 over the first 20 columns and 110 over the rest
# (M = 120 / 40).  At (40, 100) the weak stretch has M == low and is out; at (38, 100) it is in.  threshold_step(False): 130
# below row 20 all along.  At (38, 120) it has M == high everywhere, nothing is strong and nothing is an edge; at
# (38, 118) the whole row is.
THRESHOLD_STEP_CASES = [(True, (40, 100)), (True, (38, 100)), (False, (38, 120)), (False, (38, 118))]


def threshold_step(two_levels=True):
    g = np.full((40, 70), 100, np.uint8)
    g[20:] = 130
    if two_levels:
        g[20:, 20:] = 110
    return g


def check_threshold_step(canny_fn):
    """canny_fn(gray, t1, t2) under check_canny at the four THRESHOLD_STEP_CASES, after the reference alone has shown that
    the cases of a pair differ, and only through pixels whose magnitude equals a threshold."""
    M = R.canny_candidates(threshold_step(), 0, 0)[0]
    assert (M[19, 25:] == 40).all() and (M[19, :15] == 120).all()
    assert (R.canny_candidates(threshold_step(False), 0, 0)[0][19:21] == 120).all()
    conv = [R.canny_sets(threshold_step(two), *t)[2] for two, t in THRESHOLD_STEP_CASES]
    assert conv[1][:, 25:].sum() == 45 and not conv[0][:, 25:].any() and conv[0][:, :15].sum() == 15
    assert not conv[2].any() and conv[3].sum() == 70
    return [check_canny(canny_fn(threshold_step(two), *t), threshold_step(two), *t) for two, t in THRESHOLD_STEP_CASES]


def change_stats_ref(gray, ref, mean, var, z_threshold):
    """sad_ref, z_count, z_max of one square in numpy float32, as ChangeDetector writes them: z = |float32(g) - mu| /
    sqrt(var), counted with z > threshold; a variance of 0 gives inf (counts) or NaN (does not count; z_max is then NaN)."""
    sad = int(np.abs(gray.astype(np.int64) - ref.astype(np.int64)).sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.abs(gray.astype(np.float32) - mean.astype(np.float32)) / np.sqrt(var.astype(np.float32))
    assert z.dtype == np.float32
    return sad, int((z > np.float32(z_threshold)).sum()), np.float32(np.max(z))


# the (d, sigma_color, sigma_space) and (clip, grid) sweeps of test_gpu_stages.py
GPU_BILATERAL_SWEEP = [(3, 40.0, 10.0), (5, 75.0, 75.0), (7, 20.0, 3.0), (9, 150.0, 1.5), (-1, 30.0, 1.0)]
CLAHE_SWEEP = [(3.0, (8, 8)), (1.5, (5, 7)), (1.0, (8, 8)), (0.0, (3, 2)), (40.0, (1, 9)), (2.0, (9, 1)), (8.0, (4, 6))]


def shapes_and_contents():
    return [(w, h, c) for (w, h) in SHAPES for c in CONTENTS]


def random_kernels(seed, n):
    rng = np.random.default_rng(seed)
    return [rng.normal(0, 1, (3, 3)).astype(np.float32) for _ in range(n)]


def random_quad_case(seed):
    """A source frame and a quad like test_gpu_stages.test_randomised_warps: inside, partly outside the frame, nearly
    degenerate or mirrored; returns (img, M, dsize) with M the forward (source -> destination) matrix."""
    rng = np.random.default_rng(900 + seed)
    w, h = int(rng.integers(20, 300)), int(rng.integers(15, 240))
    img = smooth(w, h, seed) if seed % 2 else noise(w, h, seed)
    base = np.float64([[0, 0], [w, 0], [0, h], [w, h]])
    pts = base + rng.uniform(-0.35, 0.35, (4, 2)) * np.float64([w, h])
    if seed % 4 == 3:
        pts = pts[[1, 0, 3, 2]]
    dw, dh = int(rng.integers(1, 400)), int(rng.integers(1, 400))
    dst = np.float64([[0, 0], [dw, 0], [0, dh], [dw, dh]])
    return img, quad_matrix(pts, dst), (dw, dh)


def quad_matrix(src, dst):
    """The projective map taking the four src points onto the four dst points (8x8 linear solve in float64)."""
    A, b = [], []
    for (x, y), (u, v) in zip(src, dst):
        A.append([x, y, 1, 0, 0, 0, -x * u, -y * u])
        A.append([0, 0, 0, x, y, 1, -x * v, -y * v])
        b += [u, v]
    m = np.linalg.solve(np.array(A, np.float64), np.array(b, np.float64))
    return np.append(m, 1.0).reshape(3, 3)


# ---------------------------------------------------------------------------------------------------------------
# generic envelope
# ---------------------------------------------------------------------------------------------------------------


def _stats(d):
    return {"max": float(d.max()) if d.size else 0.0, "over1": float((d > 1).mean()) if d.size else 0.0}


def check_rounded(out, ref, eps, what, lo=0.0, hi=255.0):
    """out is ref rounded to an integer and saturated: |out - clip(ref)| <= 0.5 + eps everywhere, and at most
    TIE_SHARE_CAP of the values have ref within eps of a .5 tie (where either neighbour passes)."""
    out = np.asarray(out, np.float64)
    ref = np.clip(np.asarray(ref, np.float64), lo, hi)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    d = np.abs(out - ref)
    bad = d > 0.5 + eps
    if bad.any():
        i = np.unravel_index(np.argmax(d), d.shape)
        raise AssertionError("%s: %d of %d values outside 0.5 + %.3g, worst %.4f at %s (out %d, ref %.4f)"
                             % (what, int(bad.sum()), d.size, eps, d[i], i, out[i], ref[i]))
    ties = np.abs(np.abs(ref - np.floor(ref)) - 0.5) <= eps
    assert ties.mean() <= TIE_SHARE_CAP, "%s: %.2f %% of values on a rounding tie" % (what, 100 * ties.mean())
    s = _stats(d)
    s["ties"] = int(ties.sum())
    return s


def check_exact(out, ref, what):
    out, ref = np.asarray(out), np.asarray(ref)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    if not np.array_equal(out.astype(np.int64), ref.astype(np.int64)):
        d = np.abs(out.astype(np.int64) - ref.astype(np.int64))
        i = np.unravel_index(np.argmax(d), d.shape)
        raise AssertionError("%s: %d of %d values differ, worst %d at %s" % (what, int((d > 0).sum()), d.size, d[i], i))
    return {"max": 0.0, "over1": 0.0, "ties": 0}


# ---------------------------------------------------------------------------------------------------------------
# stages
# ---------------------------------------------------------------------------------------------------------------


def bilateral_eps(d, sigma_space):
    """float32 weights (two table roundings and a product) and float32 sums over n taps, then 1/sum and a product:
    relative error below (2n + 8) u on a value of at most 255.  The centre tap has weight 1, so sum(w) >= 1 and
    weights that underflow in float32 change the result by less than that."""
    n = len(R.bilateral_taps(d, sigma_space))
    return 255.0 * (2 * n + 8) * U32


def check_bilateral(out, img, d=9, sigma_color=75.0, sigma_space=75.0):
    ref = R.bilateral(img, d, sigma_color, sigma_space)
    return check_rounded(out, ref, bilateral_eps(d, sigma_space), "bilateral d=%d sc=%g ss=%g" % (d, sigma_color, sigma_space))


def check_bilateral_bands(out, img, d=9, sigma_color=75.0, sigma_space=75.0, band=48):
    """check_bilateral on the top, middle and bottom bands of rows of a large frame (full width): each band's reference
    is computed on the band plus radius rows of context, so its rows equal the whole-frame reference."""
    h = img.shape[0]
    r = R.bilateral_radius(d, sigma_space)
    stats = []
    for y0 in sorted({0, max(h // 2 - band // 2, 0), max(h - band, 0)}):
        y1 = min(y0 + band, h)
        c0, c1 = max(y0 - r, 0), min(y1 + r, h)
        ref = R.bilateral(img[c0:c1], d, sigma_color, sigma_space)[y0 - c0:y1 - c0]
        stats.append(check_rounded(out[y0:y1], ref, bilateral_eps(d, sigma_space), "bilateral rows %d-%d" % (y0, y1)))
    return {"max": max(s["max"] for s in stats), "over1": max(s["over1"] for s in stats), "ties": sum(s["ties"] for s in stats)}


def check_filter2d(out, img, kernel):
    """Integer kernels: the sum is an integer, so the saturated output is exact.  Float kernels: nine float32
    products and sums, each term at most |k| * 255: error below 12 u * 255 * sum|k|."""
    k = np.asarray(kernel, np.float64)
    ref = R.filter2d_3x3(img, k)
    if np.array_equal(k, np.round(k)):
        return check_exact(out, np.clip(ref, 0, 255), "filter2D integer kernel")
    return check_rounded(out, ref, 12 * U32 * 255 * np.abs(k).sum(), "filter2D float kernel")


def check_normalize(out, img):
    """scale and shift held as float32, one fused multiply-add per value on |terms| <= 255: below 8 u * 255."""
    return check_rounded(out, R.normalize_minmax(img), 8 * U32 * 255, "normalize")


def gray_eps():
    """Quantising the BT.601 weights to 15 bits moves the weighted sum by at most 255 * sum|w - q / 2^15|."""
    cb, cg, cr = R.gray_q15_coefficients()
    return 255 * (abs(0.114 - cb / 32768) + abs(0.587 - cg / 32768) + abs(0.299 - cr / 32768))


def check_gray(out, img):
    check_exact(out, R.bgr2gray_q15(img), "BGR2GRAY integer form")
    return check_rounded(out, R.bgr2gray(img), gray_eps(), "BGR2GRAY vs BT.601")


def check_blur(out, gray):
    """The binomial 5x5 is exact in 8.8 fixed point: the output is the exact sum rounded once."""
    check_exact(out, R.gaussian_blur_5x5_u8(gray), "GaussianBlur 5x5")
    d = np.abs(np.asarray(out, np.float64) - R.gaussian_blur_5x5(gray))
    assert d.max() <= 0.5
    return _stats(d)


def gaussian_e1(k):
    """||E||_1 of E = q (x) q / 65536 - c (x) c: how far the 8.8 fixed-point kernel is from the real one, from the
    coefficients of ref64.py alone (0 for k <= 7, 0.013 for k = 9, 0.060 for k = 31)."""
    q, c = R.gaussian_q8(k).astype(np.float64), R.gaussian_kernel(k)
    return float(np.abs(np.outer(q, q) / 65536.0 - np.outer(c, c)).sum())


def window_range(gray, k):
    """max - min of gray over every pixel's REFLECT_101 k x k window."""
    g = np.asarray(gray, np.int64)
    h, w = g.shape
    r = k // 2
    p = R._pad101(g, r, r)
    rows_hi = np.max([p[:, j:j + w] for j in range(k)], axis=0)
    rows_lo = np.min([p[:, j:j + w] for j in range(k)], axis=0)
    return np.max([rows_hi[i:i + h] for i in range(k)], axis=0) - np.min([rows_lo[i:i + h] for i in range(k)], axis=0)


def check_gaussian(out, gray, k):
    """cv2.GaussianBlur(gray, (k, k), 0) on 8 bits.  First the integer form, exactly.  Then the float64 definition: both
    kernels sum to 1, so out's exact value minus the definition is sum E_ij (g_ij - mid) for any mid, at most
    ||E||_1 * range / 2 with range = max - min of the pixel's window and mid their mean; rounding adds 0.5."""
    gray = np.asarray(gray)
    what = "GaussianBlur k=%d %s" % (k, gray.shape)
    check_exact(out, R.gaussian_blur_u8(gray, k), what + " integer form")
    d = np.abs(np.asarray(out, np.float64) - R.gaussian_blur(gray, k))
    e1 = gaussian_e1(k)
    bound = 0.5 + e1 * window_range(gray, k) / 2.0
    bad = d > bound
    if bad.any():
        i = np.unravel_index(np.argmax(d - bound), d.shape)
        raise AssertionError("%s: %d of %d values outside 0.5 + %.4f * range / 2, worst %.4f against %.4f at %s"
                             % (what, int(bad.sum()), d.size, e1, d[i], bound[i], i))
    return dict(_stats(d), e1=e1, bound=float(bound.max()))


def check_canny(edges, gray, t1, t2, tie_cap=None):
    """cv2.Canny(gray, t1, t2): 0 / 255 only; between hyst(strict) and hyst(loose) of ref64.canny_sets (true under any
    tie rule); equal to hyst(conv), OpenCV's tie rule.  With tie_cap, hyst(loose) and hyst(strict) may differ on at most
    that share of the pixels (else the sandwich says little)."""
    edges, gray = np.asarray(edges), np.asarray(gray)
    what = "Canny %s t=(%g, %g)" % (gray.shape, t1, t2)
    assert edges.shape == gray.shape, (what, edges.shape)
    assert np.isin(edges, (0, 255)).all(), what + ": values other than 0 / 255"
    e = edges > 0
    strict, loose, conv = R.canny_sets(gray, t1, t2)
    assert not (strict & ~loose).any(), what + ": reference sets not nested"
    gap = float((strict != loose).mean())
    if tie_cap is not None:
        assert gap <= tie_cap, "%s: hyst(loose) and hyst(strict) differ on %.2f %% of the pixels" % (what, 100 * gap)
    missing, extra = int((strict & ~e).sum()), int((e & ~loose).sum())
    assert missing == 0 and extra == 0, ("%s: outside the sandwich under any tie rule: %d pixels of hyst(strict) missing, "
                                         "%d edges outside hyst(loose)" % (what, missing, extra))
    diff = int((e != conv).sum())
    assert diff == 0, "%s: inside the sandwich, but %d pixels differ from OpenCV's tie rule" % (what, diff)
    return {"edges": int(e.sum()), "gap": gap, "strict": int(strict.sum()), "loose": int(loose.sum())}


def check_prepare_analysis(gray, binary, t, img):
    """gray exactly the integer BGR2GRAY; Otsu threshold t maximises the between-class variance of the blurred gray's
    histogram (to 1e-12 relative: the variance is evaluated in float64); binary == 255 where blurred > t."""
    s = check_gray(gray, img)
    blurred = R.gaussian_blur_5x5_u8(R.bgr2gray_q15(img))
    t_ref, var = R.otsu_threshold(np.bincount(blurred.ravel(), minlength=256))
    if t is not None:
        assert 0 <= t <= 255 and var[t] >= var.max() * (1 - 1e-12), ("otsu", t, t_ref, var[t], var.max())
    else:
        t = t_ref
    check_exact(binary, np.where(blurred > t, 255, 0), "Otsu binary (> t)")
    return s


def clahe_eps():
    """float32 bilinear blend of four u8 LUT values: a handful of roundings on values <= 255."""
    return 8 * U32 * 255


def check_clahe(out, gray, clip, tiles, luts=None):
    ref_luts = R.clahe_luts(gray, clip, tiles)
    if luts is not None:
        check_exact(luts, ref_luts, "CLAHE LUTs clip %g grid %r" % (clip, tiles))
    return check_rounded(out, R.clahe(gray, clip, tiles, luts=ref_luts), clahe_eps(), "CLAHE clip %g grid %r" % (clip, tiles))


HSV_EPS_H = 5 * 255 * 0.5 / 4096    # 12-bit reciprocal table (error <= 1/2) times a numerator of at most 5 * diff
HSV_EPS_S = 255 * 0.5 / 4096        # 12-bit reciprocal table times diff <= 255


def check_bgr2hsv(out, img):
    """H circular (180 == 0); V exact."""
    ref = R.bgr2hsv(img)
    out = np.asarray(out, np.float64)
    dh = np.abs(out[..., 0] - ref[..., 0])
    dh = np.minimum(dh, 180 - dh)
    assert dh.max() <= 0.5 + HSV_EPS_H, ("H", dh.max())
    assert out[..., 0].max() < 180
    s = check_rounded(out[..., 1], ref[..., 1], HSV_EPS_S, "BGR2HSV S")
    check_exact(out[..., 2], ref[..., 2], "BGR2HSV V")
    return {"max": max(float(dh.max()), s["max"]), "over1": 0.0, "ties": s["ties"]}


HSV2BGR_EPS = 8 * U32 * 255          # float32 evaluation of the sector formula


def check_hsv2bgr(out, hsv):
    return check_rounded(out, R.hsv2bgr(hsv), HSV2BGR_EPS, "HSV2BGR")


def _hsv_candidates(img):
    """Integer HSV triples an 8-bit BGR2HSV may return inside its envelope: round(ref), or both neighbours where
    ref is within the table error of a .5 tie."""
    ref = R.bgr2hsv(img)
    outs = []
    for c, eps in ((0, HSV_EPS_H), (1, HSV_EPS_S)):
        r = ref[..., c]
        near = np.abs(r - np.floor(r) - 0.5) <= eps
        outs.append((np.where(near, np.floor(r), np.rint(r)), np.where(near, np.floor(r) + 1, np.rint(r))))
    hs = [np.mod(h, 180) for h in outs[0]]
    return [np.stack([h, s, ref[..., 2]], axis=-1) for h in hs for s in outs[1]]


def check_profile_neutral(out, img):
    """apply_color_profile with the neutral profile is BGR -> HSV (8-bit) -> HSV2BGR: out must be HSV2BGR of one of
    the admissible integer HSV triples, within 0.5 + HSV2BGR_EPS."""
    out = np.asarray(out, np.float64)
    best = None
    for hsv in _hsv_candidates(img):
        d = np.abs(out - R.hsv2bgr(hsv)).max(axis=-1)
        best = d if best is None else np.minimum(best, d)
    assert best.max() <= 0.5 + HSV2BGR_EPS, ("neutral profile", float(best.max()), int((best > 0.5 + HSV2BGR_EPS).sum()))
    return _stats(best)


# ---------------------------------------------------------------------------------------------------------------
# apply_color_profile beyond the neutral setting: convertScaleAbs, BGR2HSV (integer form), the numpy middle, HSV2BGR
# ---------------------------------------------------------------------------------------------------------------

PROFILE_TIE_CAP = 0.05           # on the colour cubes; the reference alone gives at most 2.9 % (sat3)
PROFILE_FRAMES = [(37, 29), (13, 1), (1, 11), (3, 2), (61, 9), (62, 9), (63, 9), (64, 9)]      # (w, h)
PROFILE_FRAME_CONTENTS = ("noise", "smooth")
GRAY_RAMP = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)               # B = G = R = 0..255


def _profile_cases():
    import color_sweep_ref as CS
    cases = {n: p for n, p in CS.PROFILES.items() if p is not None}
    cases["stages_fractional"] = CS.STAGES_FRACTIONAL
    cases.update({
        "neg_scales": {"sat_scale": -0.5, "val_scale": -1.0},
        "neg_contrast": {"contrast": -0.71, "brightness": 12.9},     # levels 40, 140, 240 on a .5 tie of convertScaleAbs
        "zero_contrast": {"contrast": 0.0, "brightness": 77},
        "bright_300": {"brightness": 300},
        "huge_shift": {"hue_shift": 1000003.25},
        "neg_frac_shift": {"hue_shift": -0.25},
        "window0": {"radical_mode": 1, "target_hue": 60, "hue_window": 0},
        "window90": {"radical_mode": 1, "target_hue": 60, "hue_window": 90},
        "target_out": {"radical_mode": 1, "target_hue": 200, "hue_window": 15},
        "target_neg": {"radical_mode": 1, "target_hue": -10.5, "hue_window": 15.5},
        "radical_default_window": {"radical_mode": 1, "target_hue": 100},
    })
    return cases


PROFILE_CASES = _profile_cases()


def profile_cube_offsets(name):
    """The cubes a profile meets: the three are dealt round PROFILE_CASES in order; the shipped profile meets all three."""
    return (0, 1, 2) if name == "shipped" else (list(PROFILE_CASES).index(name) % 3,)


def profile_cube_cases():
    return [(n, o) for n in PROFILE_CASES for o in profile_cube_offsets(n)]


def color_cube(offset):
    """Every third level of each channel from `offset`: 86^3 (85^3 from 1 and 2) colours as one frame, blue slowest."""
    v = np.arange(offset, 256, 3, dtype=np.uint8)
    b, g, r = np.meshgrid(v, v, v, indexing="ij")
    return np.stack([b, g, r], axis=-1).reshape(len(v) * len(v), len(v), 3)


def profile_frames():
    """[(what, frame)]: PROFILE_FRAMES x PROFILE_FRAME_CONTENTS.  Feed the code under test view(frame)."""
    return [("%s %dx%d" % (c, w, h), frame(c, w, h)) for (w, h) in PROFILE_FRAMES for c in PROFILE_FRAME_CONTENTS]


def byte_map_profile(profile):
    """The profile whose output on GRAY_RAMP is the convertScaleAbs byte map: the profile itself where val_scale is 1 (gray
    has s = 0, which every saturation map keeps, and the hue of a gray does not show), else its contrast and brightness alone."""
    if profile.get("val_scale", 1.0) == 1:
        return profile
    return {"contrast": profile.get("contrast", 1.0), "brightness": profile.get("brightness", 0)}


def csa_eps(alpha, beta):
    """float32 alpha, beta and one fused multiply-add: error below 4 u (255 |alpha| + |beta|)."""
    return 4 * U32 * (255 * abs(alpha) + abs(beta))


def profile_byte_map(ramp_out, profile):
    """ramp_out: the code under test on GRAY_RAMP with byte_map_profile(profile).  It must be gray and convertScaleAbs of the
    level, rounded once and saturated, within csa_eps.  Returns the 256-entry byte map that check_profile indexes: rint of the
    float64 value, saturated, except at levels within csa_eps of a .5 tie, where the value just shown admissible is taken."""
    assert profile.get("val_scale", 1.0) == 1, "the byte map is read off a profile that leaves V alone: byte_map_profile()"
    alpha, beta = profile.get("contrast", 1.0), profile.get("brightness", 0)
    out = np.asarray(ramp_out).reshape(256, 3)
    assert (out == out[:, :1]).all(), ("profile on a gray ramp is not gray", int((out != out[:, :1]).any(axis=1).sum()))
    eps = csa_eps(alpha, beta)
    ref = np.clip(R.convert_scale_abs(np.arange(256), alpha, beta), 0, 255)
    check_rounded(out[:, 0], ref, eps, "convertScaleAbs alpha=%g beta=%g" % (alpha, beta))
    tie = np.abs(ref - np.floor(ref) - 0.5) <= eps
    return np.where(tie, out[:, 0], np.rint(ref)).astype(np.uint8)


def byte_map_definition(profile):
    """The byte map from the definition alone: rint of the float64 |alpha x + beta|, saturated (a tie goes to the even side)."""
    x = R.convert_scale_abs(np.arange(256), profile.get("contrast", 1.0), profile.get("brightness", 0))
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def profile_reference(img, profile, byte_map):
    """B, G, R unrounded: HSV2BGR of the numpy middle of the integer BGR2HSV of byte_map[img], from ref64 alone."""
    return R.hsv2bgr(R.color_profile_adjust(R.bgr2hsv_u8(np.asarray(byte_map, np.uint8)[img]), profile))


def check_profile(out, img, profile, byte_map, ref=None, tie_cap=None, what="profile"):
    """apply_color_profile(img, profile): every stage before HSV2BGR is defined on integers (the byte map, the integer
    BGR2HSV, the truncating cast), so there is one candidate per pixel, and out is HSV2BGR of it rounded once:
    check_rounded with HSV2BGR_EPS.  `ref`: profile_reference(img, profile, byte_map) where a caller shares it.  `tie_cap`:
    the share of values within HSV2BGR_EPS of a .5 tie that the case may have (check_rounded's TIE_SHARE_CAP without it)."""
    if ref is None:
        ref = profile_reference(img, profile, byte_map)
    s = check_rounded(out, ref, HSV2BGR_EPS, what)
    if tie_cap is not None:
        assert s["ties"] <= tie_cap * ref.size, "%s: %.2f %% of values on a rounding tie" % (what, 100.0 * s["ties"] / ref.size)
    return s


@functools.lru_cache(maxsize=None)
def cube_reference(name, offset, byte_map_bytes):
    """profile_reference of PROFILE_CASES[name] on color_cube(offset), computed once for the host and the GPU tests of one run
    (they arrive at the same byte map unless they take different neighbours of a convertScaleAbs tie).  Read-only."""
    ref = profile_reference(color_cube(offset), PROFILE_CASES[name], np.frombuffer(byte_map_bytes, np.uint8))
    ref.setflags(write=False)
    return ref


def observed_byte_map(apply, profile):
    """apply(img, profile) -> uint8 BGR is the code under test: its byte map, checked (profile_byte_map)."""
    bmp = byte_map_profile(profile)
    return profile_byte_map(apply(GRAY_RAMP, bmp), bmp)


def check_profile_cube(apply, name, offset):
    """The code under test on color_cube(offset) with PROFILE_CASES[name], one call, under check_profile and the cubes' tie cap."""
    profile, cube = PROFILE_CASES[name], color_cube(offset)
    byte_map = observed_byte_map(apply, profile)
    return check_profile(apply(cube, profile), cube, profile, byte_map, ref=cube_reference(name, offset, byte_map.tobytes()),
                         tie_cap=PROFILE_TIE_CAP, what="profile %s, cube %d" % (name, offset))


def check_profile_frames(apply, name):
    """The code under test on the small frames, as strided and misaligned views, with PROFILE_CASES[name]."""
    profile = PROFILE_CASES[name]
    byte_map = observed_byte_map(apply, profile)
    return [check_profile(apply(view(img), profile), img, profile, byte_map, what="profile %s, %s" % (name, what))
            for what, img in profile_frames()]


def check_lab(out, ref, what):
    """Per-channel max <= LAB_MAX and at most LAB_SHARE_OVER_1 of the values more than 1 LSB from the definition."""
    d = np.abs(np.asarray(out, np.float64) - ref)
    mx = d.reshape(-1, 3).max(axis=0)
    over = (d > 1).mean()
    assert (mx <= LAB_MAX).all(), (what, mx)
    assert over <= LAB_SHARE_OVER_1, (what, over)
    return {"max": float(mx.max()), "max_ch": [float(x) for x in mx], "over1": float(over)}


def warp_gradient(img, X, Y):
    """Gx, Gy: the largest horizontal / vertical neighbour difference (worst channel) among the source pixels
    floor(X, Y) - 1 ... floor(X, Y) + 2 that a bilinear tap at a point moved by up to 1/64 pixel can reach, samples
    outside the image counting as 0 (the constant border)."""
    f = np.asarray(img, np.float64)
    h, w = f.shape[:2]
    p = np.zeros((h + 8, w + 8) + f.shape[2:])
    p[4:4 + h, 4:4 + w] = f
    gx = np.abs(np.diff(p, axis=1)).max(axis=-1)       # gx[y, x] = |p[y, x+1] - p[y, x]|
    gy = np.abs(np.diff(p, axis=0)).max(axis=-1)       # gy[y, x] = |p[y+1, x] - p[y, x]|
    x0 = np.floor(np.clip(X, -3, w + 1)).astype(np.int64) + 4
    y0 = np.floor(np.clip(Y, -3, h + 1)).astype(np.int64) + 4
    Gx = np.zeros(X.shape)
    Gy = np.zeros(X.shape)
    for a in (-1, 0, 1, 2):
        for b in (-1, 0, 1):
            Gx = np.maximum(Gx, gx[y0 + a, x0 + b])
            Gy = np.maximum(Gy, gy[y0 + b, x0 + a])
    return Gx, Gy


def check_warp(out, img, M, dsize):
    """Source coordinates are quantised to 1/32 pixel (at most 1/64 off per axis), so the output is the exact-coordinate
    bilinear value within 0.5 + (Gx + Gy)/64 + WARP_SLACK.  A destination pixel whose source point is more than one
    pixel outside the image (plus the 1/32 quantisation) must be exactly 0."""
    ref, X, Y = R.warp_perspective(img, M, dsize)
    h, w = img.shape[:2]
    Gx, Gy = warp_gradient(img, X, Y)
    bound = 0.5 + (Gx + Gy) / 64 + WARP_SLACK
    out = np.asarray(out, np.float64)
    d = np.abs(out - ref).max(axis=-1)
    bad = d > bound
    assert not bad.any(), ("warp", int(bad.sum()), float((d - bound).max()))
    q = 1.0 / 32
    far = (X < -1 - q) | (X > w + q) | (Y < -1 - q) | (Y > h + q)
    assert not out[far].any(), ("warp: non-zero beyond the border", int((out[far] != 0).any(axis=-1).sum()))
    return dict(_stats(np.abs(out - ref)), far=int(far.sum()))


# ---------------------------------------------------------------------------------------------------------------
# correct_lighting: Lab -> CLAHE(L) -> BGR, composed from the definitions
# ---------------------------------------------------------------------------------------------------------------


def lighting_levels(min_gap=8.0):
    """Gray levels whose float64 L* (8-bit scale) lie at least min_gap apart: an 8-bit BGR2LAB inside its envelope
    (|dL| <= LAB_MAX) keeps them distinct and in order, so every CLAHE tile histogram is the reference's with each
    bin moved by at most LAB_MAX + 1/2 places."""
    g = np.arange(256, dtype=np.uint8)
    L = R.bgr2lab(np.repeat(g[:, None, None], 3, axis=2))[:, 0, 0]
    out, last = [], -1e9
    for v in range(256):
        if L[v] - last >= min_gap:
            out.append(v)
            last = L[v]
    return np.array(out, np.uint8)


def lighting_frame(w, h, seed, tiles=(8, 8)):
    """Gray image (B = G = R, so a* = b* = 128 by the white point) of lighting_levels(), one band of levels per
    tile-sized block so neighbouring tile LUTs differ strongly."""
    rng = np.random.default_rng(seed)
    lv = lighting_levels()
    tx, ty = tiles
    yy, xx = np.mgrid[:h, :w]
    cells = rng.integers(0, len(lv), (ty + 1, tx + 1))
    idx = cells[np.minimum(yy * ty // max(h, 1), ty), np.minimum(xx * tx // max(w, 1), tx)] + rng.integers(-2, 3, (h, w))
    return np.repeat(lv[np.clip(idx, 0, len(lv) - 1)][..., None], 3, axis=2)


def check_correct_lighting(out, img, clip, tiles):
    """For lighting_frame() inputs.  Reference: u8(round(ref Lab)); CLAHE of L from its definition, rounded to u8;
    ref LAB2BGR.  Bound: the LUT value a pixel reads differs from the reference's by at most
    255 (shift * batch + residual bumps in the shift window) / area + 1, shift = LAB_MAX + 1/2 bins (the histogram is
    the reference's with every bin moved that far, see lighting_levels, so clipping and excess are unchanged);
    one more LSB for rounding the blend; a*, b* within LAB_MAX; then LAB2BGR's own envelope LAB_MAX plus its spread
    over that box of (L, a, b), evaluated at the box corners."""
    lab = np.clip(np.rint(R.bgr2lab(img)), 0, 255)
    L = lab[..., 0].astype(np.uint8)
    luts = R.clahe_luts(L, clip, tiles)
    h, w = L.shape
    th, tw, eh, ew = R.clahe_tiling(h, w, tiles)
    area = th * tw
    shift = int(np.ceil(LAB_MAX + 0.5))
    dlut = 1.0
    cl = R.clahe_clip(clip, area)
    if cl:
        ext = L[R.reflect101_index(np.arange(eh), h)][:, R.reflect101_index(np.arange(ew), w)]
        for y in range(tiles[1]):
            for x in range(tiles[0]):
                hist = np.bincount(ext[y * th:(y + 1) * th, x * tw:(x + 1) * tw].ravel(), minlength=256)
                batch, residual = divmod(int(np.maximum(hist - cl, 0).sum()), 256)
                bumps = 0 if residual == 0 else min(residual, -(-shift // max(256 // residual, 1)) + 1)
                dlut = max(dlut, 255.0 * (shift * batch + bumps) / area + 1)
    dL = np.ceil(dlut + 1)
    lab2 = lab.copy()
    lab2[..., 0] = np.clip(np.rint(R.clahe(L, clip, tiles, luts=luts)), 0, 255)
    ref = R.lab2bgr(lab2)
    spread = np.zeros(ref.shape)
    for sl in (-1, 1):
        for sa in (-1, 1):
            for sb in (-1, 1):
                c = lab2.copy()
                c[..., 0] = np.clip(c[..., 0] + sl * dL, 0, 255)
                c[..., 1] += sa * LAB_MAX
                c[..., 2] += sb * LAB_MAX
                spread = np.maximum(spread, np.abs(R.lab2bgr(c) - ref))
    bound = LAB_MAX + spread
    d = np.abs(np.asarray(out, np.float64) - ref)
    bad = d > bound
    assert not bad.any(), ("correct_lighting clip %g grid %r" % (clip, tiles), int(bad.sum()), float((d - bound).max()), dL)
    return dict(_stats(d), dL=float(dL), bound_mean=float(bound.mean()))
