"""HoughCircles per square (k_hough, and the oracle's restatement of cv2.HoughCircles): the inputs, the checkers and the
branch ledger shared by test_hough_host.py (the CPU oracle) and test_gpu_hough_edges.py (the HIP kernel).

Three layers, each as independent of the code under test as the stage allows:
  1  equality with the oracle, record by record, at every LDS layout and dp (test_gpu_hough_edges.py only);
  2  stages with a statement of their own: the edge count is |hyst(conv)| of ref64's Canny, the support of a returned
     circle is the number of those edges whose distance to the centre lies in the window its radius names (float64,
     as a sandwich), and the list invariants need no reference at all;
  3  the vote, restated a third time in numpy (accumulator()): the number of accumulator maxima and the set of
     centres.  A restatement of the algorithm, not a definition.
Nothing here imports the oracle or the package: a record is a plain Rec, filled by the caller."""
import collections
import functools
import math

import numpy as np

import ref64 as R

KEEP = 6                    # CBV_HOUGH_KEEP: circles a cbv_hough_result carries
FIRST_PASS = 512            # HG_MAXC: accumulator maxima the first pass of k_hough keeps
F = np.float32

SHAPES = [(2, 2), (2, 128), (128, 2), (3, 5), (9, 12), (16, 16), (24, 24), (33, 29), (33, 30), (33, 31), (33, 32), (40, 40),
          (64, 64), (40, 128), (128, 40), (128, 128)]                                                             # h x w
CONTENTS = ("noise", "blurred", "disc", "disc_off", "const")
DPS = (1.0, 1.2, 1.5, 2.0, 3.0, 16.0)
PARAM_SETS = ((100, 25, .20, .55), (60, 1, 0, 0), (60, 1, .10, 1.0), (200, 3, .30, .30), (100, 8, .12, .30), (240, 8, .20, .55))
# the squares of one (dp, parameter set) in sets of at most 64 (CBV_MAX_SQUARES), each with a 128 x 128 square: the
# large layout.  The same squares shape by shape give every other layout.
MIXED_SETS = (("noise", "blurred", "const"), ("disc", "disc_off"))
# beside the grid: the thin strip whose minDist is dp (min_dim // 3 == 0), so that more than 64 circles survive
STRIP = ((5, 128), "noise", 1.0, (60, 0, 0, 0))

# beside the grid: a maximum radius of twice the square (the API takes ratios up to 4): more radius bins than a side has pixels
WIDE = ((100, 8, .20, 2.0), ((24, 24), (33, 29)), ("disc", "blurred"))

Rec = collections.namedtuple("Rec", "flags n_edges n_centres n_circles circles found cx cy r kind")
# circles: [(x, y, r, votes)] as float32 / int, the first KEEP (kernel) or all of them (oracle); cx, cy, r: the picked
# circle as float32 or None; kind: "hough" / "tower_top" / None; n_centres: None where the source does not export it


def case_ids():
    return [(dp, ps) for dp in DPS for ps in range(len(PARAM_SETS))]


@functools.lru_cache(maxsize=None)
def square(content, h, w):
    """Seeded content of a square; read-only, computed once."""
    rng = np.random.default_rng(1000 * h + w)
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
    if content == "noise":
        g = noise
    elif content == "blurred":
        g = R.gaussian_blur_5x5_u8(noise)
    elif content == "const":
        g = np.full((h, w), 128, np.uint8)
    else:
        m = min(h, w)
        off = 0.25 * m if content == "disc_off" else 0.0
        yy, xx = np.mgrid[:h, :w]
        disc = (xx - (w / 2.0 + 0.8 * off)) ** 2 + (yy - (h / 2.0 - 0.6 * off)) ** 2 <= (0.38 * m) ** 2
        g = R.gaussian_blur_5x5_u8(np.clip(np.where(disc, 210, 60) + rng.integers(-6, 7, (h, w)), 0, 255).astype(np.uint8))
    g = np.ascontiguousarray(g, dtype=np.uint8)
    g.setflags(write=False)
    return g


def squares_of(contents, shapes=SHAPES):
    """[((content, h, w), gray)]"""
    return [((c, h, w), square(c, h, w)) for (h, w) in shapes for c in contents]


CURVES = {"single_wave": ((40, 100), 12, 8.0), "block_wide": ((60, 128), 24, 6.0)}       # shape, amplitude, period
CURVE_PARAM1 = 80
CURVE_A, CURVE_STRONG = 12, 30


@functools.lru_cache(maxsize=None)
def curve(name, end):
    """A weak curve for the hysteresis inside HoughCircles, after ref64_checks.hysteresis_curve: the boundary
    y = h/2 + amp sin(x / per) between gray 100 and 100 + a.  A step of height a has M = 4a on a straight stretch and up
    to 6a on a diagonal one: a = 12 keeps M in 48..72, inside (40, 80] at param1 = 80.  Over the 8 columns at `end`
    ("left" / "right") a = 30, falling to 12 over the next 10; end None: no strong stretch."""
    (h, w), amp, per = CURVES[name]
    yy, xx = np.mgrid[:h, :w]
    x = np.arange(w)
    d = {"left": x, "right": w - 1 - x, None: np.full(w, 1000)}[end]
    a = np.where(d < 8, float(CURVE_STRONG), np.clip(CURVE_A + (18 - d) * (CURVE_STRONG - CURVE_A) / 10.0, CURVE_A, CURVE_STRONG))
    g = np.rint(np.where(yy > h / 2.0 + amp * np.sin(xx / per), 100 + a[None, :], 100)).astype(np.uint8)
    g.setflags(write=False)
    return g


def curve_facts(name, end):
    """The case itself, on ref64 alone: {"nweak", "edges"}.  The curve is weak everywhere except at the strong end, the
    weak count is on the intended side of 256 (hg_p3 floods with one wave up to 256 weak candidates, block-wide above),
    hysteresis reaches the far end, and without the strong stretch nothing is an edge."""
    g = curve(name, end)
    w = g.shape[1]
    M, low, high, _, _, cand = R.canny_candidates(g, CURVE_PARAM1 / 2, CURVE_PARAM1)
    assert (low, high) == (40, 80)
    nweak = int((cand & (M <= high)).sum())
    assert (nweak <= 256) if name == "single_wave" else (nweak > 256), (name, end, nweak)
    conv = R.canny_sets(g, CURVE_PARAM1 / 2, CURVE_PARAM1)[2]
    if end is None:
        assert not (cand & (M > high)).any() and not conv.any() and not R.canny_sets(g, CURVE_PARAM1 / 2, CURVE_PARAM1)[1].any()
        return {"nweak": nweak, "edges": 0}
    strong_cols = np.nonzero((cand & (M > high)).any(axis=0))[0]
    assert len(strong_cols) and (strong_cols.max() < 18 if end == "left" else strong_cols.min() > w - 19), strong_cols
    cols = np.nonzero(conv.any(axis=0))[0]
    assert cols.min() == 0 and cols.max() == w - 1 and len(cols) == w, (name, end, cols.min(), cols.max(), len(cols))
    assert conv.sum() > nweak / 2
    return {"nweak": nweak, "edges": int(conv.sum())}


# ------------------------------------------------------------------ the parameters, restated


def clamp_dp(dp):
    return F(1) if F(dp) < F(1) else F(dp)


def radii(h, w, min_ratio, max_ratio):
    """minRadius / maxRadius as PieceDetector passes them (int(min_dim * ratio)) and as HoughCircles reads them: a maximum
    <= 0 means max(w, h), a maximum <= the minimum means minimum + 2."""
    m = min(h, w)
    lo, hi = max(int(m * min_ratio), 0), int(m * max_ratio)
    return lo, (max(w, h) if hi <= 0 else (lo + 2 if hi <= lo else hi))


def n_bins(dp, min_radius, max_radius):
    return int(np.rint(F(max_radius - min_radius) / clamp_dp(dp) * F(10)))


def thresholds(param1):
    thr = int(np.rint(param1))
    return max(1, thr // 2), thr


@functools.lru_cache(maxsize=None)
def _edge_map(key, param1):
    g = _GRAYS[key]
    low, high = thresholds(param1)
    e = R.canny_sets(g, low, high)[2]
    e.setflags(write=False)
    return e


_GRAYS = {}


def edge_map(gray, param1):
    """hyst(conv) of ref64's Canny at (max(1, param1 // 2), param1), cached by content."""
    key = (gray.shape, gray.tobytes())
    _GRAYS.setdefault(key, gray)
    return _edge_map(key, param1)


# ------------------------------------------------------------------ layer 2


SUPPORT_EPS = 2e-3   # px.  The float32 chain of a bin index (r2, sqrt, subtract, divide, multiply, round) errs by at most
                     # about 6 roundings x 182 px x 2^-24 = 6.5e-5 px; 30-fold margin.


def window(r, dp, min_radius):
    """(s, lo, up): the radius of a circle names the bins (lo, up] of its window, r = (up + lo) / 2 / 10 * dp + minR.  A
    full window has up - lo = 10; one cut at bin 0 has lo = -1."""
    s = int(round(20.0 * (float(r) - min_radius) / float(clamp_dp(dp))))
    return (s, (s - 10) // 2, (s + 10) // 2) if s >= 8 else (s, -1, s + 1)


def support(gray, circle, dp, param1, min_radius, max_radius):
    """(strict, loose, s) for a returned circle (x, y, r, votes): the Canny edge pixels at a distance d from (x, y) with
    minR <= d <= maxR whose bin min((d - minR) * 10 / dp, nbins - 0.51), rounded, lies in the circle's window: both ends of
    the interval of d shrunk by SUPPORT_EPS (strict) and widened by it (loose).  float64."""
    dpf = float(clamp_dp(dp))
    ys, xs = np.nonzero(edge_map(gray, param1))
    d = np.hypot(xs - float(circle[0]), ys - float(circle[1]))
    s, lo, up = window(circle[2], dp, min_radius)
    nb = n_bins(dp, min_radius, max_radius)
    d_lo = max(float(min_radius), min_radius + (lo + 0.5) * dpf / 10)
    d_hi = float(max_radius) if up >= nb - 1 else min(float(max_radius), min_radius + (up + 0.5) * dpf / 10)
    e = SUPPORT_EPS
    return int(((d >= d_lo + e) & (d <= d_hi - e)).sum()), int(((d >= d_lo - e) & (d <= d_hi + e)).sum()), s


def before(a, b):
    """hg_before / cmp_circle: votes descending, then r descending, x ascending, y ascending"""
    return (-a[3], -a[2], a[0], a[1]) < (-b[3], -b[2], b[0], b[1])


def min_dist(h, w, dp):
    """minDist as PieceDetector passes it, min_dim // 3, and as HoughCircles floors it at dp; float32"""
    return max(F(min(h, w) // 3), clamp_dp(dp))


def _near(a, b, md):
    ex, ey = F(a[0]) - F(b[0]), F(a[1]) - F(b[1])
    return ex * ex + ey * ey < md * md


def suppress(cands, h, w, dp):
    """RemoveOverlaps: a sorted candidate is kept unless an earlier kept one is nearer than minDist (float32, strict)."""
    md, kept = min_dist(h, w, dp), []
    for c in cands:
        if not any(_near(k, c, md) for k in kept):
            kept.append(c)
    return kept


def pairs_at_min_dist(cs, h, w, dp):
    md = min_dist(h, w, dp)
    return sum(int((F(a[0]) - F(b[0])) ** 2 + (F(a[1]) - F(b[1])) ** 2 == md * md) for i, a in enumerate(cs) for b in cs[:i])


def check_list(rec, h, w, dp, ps, tag):
    """The invariants of a circle list that need no reference."""
    param1, param2, min_ratio, max_ratio = ps
    dpf = clamp_dp(dp)
    lo, hi = radii(h, w, min_ratio, max_ratio)
    m = min(h, w)
    cs = rec.circles
    assert len(cs) == min(rec.n_circles, len(cs)) and (len(cs) >= min(rec.n_circles, KEEP)), tag
    md = min_dist(h, w, dp)
    acols, arows = math.ceil(F(w) / dpf), math.ceil(F(h) / dpf)
    for k, c in enumerate(cs):
        assert c[3] > int(np.rint(param2)), (tag, k, c)
        assert lo <= c[2] <= hi, (tag, k, c, lo, hi)
        for v, n in ((c[0], acols), (c[1], arows)):
            i = int(np.rint(float(v) / float(dpf) - 0.5))
            assert 1 <= i <= n and F(F(i + 0.5) * dpf) == F(v), (tag, k, c)     # cell i of the accumulator; cell 0 is never a centre
        if k:
            assert before(cs[k - 1], c), (tag, k, cs[k - 1], c)
        for j in range(k):
            assert not _near(cs[j], c, md), (tag, j, k, cs[j], c)
    # the pick: the first circle nearest to (w // 2, h // 2) among those nearer than 0.3 min_dim (float32, as numpy)
    best, best_d = None, np.inf
    for c in cs:
        dist = np.sqrt((F(c[0]) - F(w // 2)) ** 2 + (F(c[1]) - F(h // 2)) ** 2)
        if dist < m * 0.3 and dist < best_d:
            best, best_d = c, dist
    if rec.n_circles <= len(cs):
        assert bool(rec.found) == (best is not None), (tag, rec.found, best)
    if rec.found:
        dist = np.sqrt((F(rec.cx) - F(w // 2)) ** 2 + (F(rec.cy) - F(h // 2)) ** 2)
        assert dist < m * 0.3, (tag, dist)
        assert best is None or best_d >= dist, (tag, best, dist)
        if best is not None and best_d == dist and rec.n_circles <= len(cs):
            assert (F(best[0]), F(best[1]), F(best[2])) == (F(rec.cx), F(rec.cy), F(rec.r)), (tag, best)
        assert rec.kind == ("tower_top" if int(rec.r) < m * 0.20 else "hough"), (tag, rec.kind, rec.r)
    else:
        assert best is None, (tag, best)


def check_stages(rec, gray, dp, ps, tag, tally):
    """Layer 2 and 3 on one record.  tally: dict that gathers circles / pinned / widest gap / the ledger's witnesses."""
    param1, param2, min_ratio, max_ratio = ps
    h, w = gray.shape
    lo, hi = radii(h, w, min_ratio, max_ratio)
    edges = edge_map(gray, param1)
    assert rec.n_edges == int(edges.sum()), (tag, rec.n_edges, int(edges.sum()))
    check_list(rec, h, w, dp, ps, tag)
    for k, c in enumerate(rec.circles):
        strict, loose, s = support(gray, c, dp, param1, lo, hi)
        assert strict <= c[3] <= loose, (tag, k, c, strict, loose)
        tally["circles"] = tally.get("circles", 0) + 1
        tally["pinned"] = tally.get("pinned", 0) + (strict == loose)
        tally["gap"] = max(tally.get("gap", 0), loose - strict)
        tally["cut"] = tally.get("cut", 0) + (s < 8)
    cm = centre_map(gray, dp, param1, param2, lo, hi)
    if rec.n_centres is not None:
        assert rec.n_centres == len(cm), (tag, rec.n_centres, len(cm))
    for k, c in enumerate(rec.circles):
        assert (F(c[0]), F(c[1])) in cm, (tag, k, c)
    return len(cm)


# ------------------------------------------------------------------ layer 3


def accumulator(gray, dp, param1, min_radius, max_radius):
    """The vote of HoughCirclesGradient, restated in numpy from ref64's Sobel and edge set: every edge pixel walks
    r = minR..maxR along its gradient in both directions, in 10-bit fixed point, from round((x / dp) * 1024) in steps of
    round((dx / dp) * 1024 / |grad|) (float32 scalar for scalar, np.rint rounds halves to even as cvRound does), until it
    leaves the accumulator of ceil(h / dp) x ceil(w / dp) cells.  int32; cell (y, x) is element [y, x] of an array two larger
    each way, as OpenCV stores it."""
    dpf = clamp_dp(dp)
    idp = F(1) / dpf
    h, w = gray.shape
    dx, dy = R.sobel3(gray)
    ys, xs = np.nonzero(edge_map(gray, param1))
    arows, acols = math.ceil(F(h) * idp), math.ceil(F(w) * idp)
    acc = np.zeros((arows + 2, acols + 2), np.int32)
    vx, vy = dx[ys, xs].astype(F), dy[ys, xs].astype(F)
    mag = np.sqrt(vx * vx + vy * vy)
    sx = np.rint((vx * idp) * F(1024) / mag).astype(np.int64)
    sy = np.rint((vy * idp) * F(1024) / mag).astype(np.int64)
    x0 = np.rint((xs.astype(F) * idp) * F(1024)).astype(np.int64)
    y0 = np.rint((ys.astype(F) * idp) * F(1024)).astype(np.int64)
    for sgn in (1, -1):
        alive = np.ones(len(xs), bool)
        for r in range(min_radius, max_radius + 1):
            x2, y2 = (x0 + sgn * r * sx) >> 10, (y0 + sgn * r * sy) >> 10
            alive &= (x2 >= 0) & (x2 < acols) & (y2 >= 0) & (y2 < arows)
            if not alive.any():
                break
            np.add.at(acc, (y2[alive], x2[alive]), 1)
    return acc


def maxima(acc, param2):
    """Elements [1..arows, 1..acols] of the accumulator above round(param2) that are local maxima by OpenCV's tie rule:
    > left and up, >= right and down.  Row 0 and column 0 hold votes but are neighbours only."""
    a = acc[1:-1, 1:-1]
    return (a > int(np.rint(param2))) & (a > acc[1:-1, :-2]) & (a >= acc[1:-1, 2:]) & (a > acc[:-2, 1:-1]) & (a >= acc[2:, 1:-1])


_CENTRES = {}


def centre_map(gray, dp, param1, param2, min_radius, max_radius):
    """{(x, y)} as float32 of the accumulator maxima: cell (y, x) has its centre at ((x + 0.5) dp, (y + 0.5) dp)."""
    key = (gray.shape, gray.tobytes(), float(dp), param1, param2, min_radius, max_radius)
    if key not in _CENTRES:
        dpf = clamp_dp(dp)
        ys, xs = np.nonzero(maxima(accumulator(gray, dp, param1, min_radius, max_radius), param2))
        _CENTRES[key] = {(F(F(x + 1.5) * dpf), F(F(y + 1.5) * dpf)) for x, y in zip(xs.tolist(), ys.tolist())}
    return _CENTRES[key]


# ------------------------------------------------------------------ the branch ledger


def check_tally(tallies):
    """At least half of the circles have their support pinned exactly (strict == loose).  Returns the figures."""
    tot = {k: (max if k == "gap" else sum)(t.get(k, 0) for t in tallies) for k in ("circles", "pinned", "gap", "cut")}
    assert tot["circles"] > 0 and 2 * tot["pinned"] >= tot["circles"], tot
    return tot


def check_ledger(get, curve_nweak):
    """get(key, dp, ps) -> Rec of a square of the grid (key = (content, h, w)) or of STRIP; curve_nweak: {name: nweak} from
    curve_facts.  Every row is a branch of hough_passes.h and the output that shows it ran."""
    seen = {}
    r = get(("noise", 64, 64), 1.0, PARAM_SETS[1])
    assert r.flags == 0 and r.n_centres > FIRST_PASS, r           # the second pass
    seen["second pass: centres of 64x64 noise"] = r.n_centres
    assert r.n_circles > KEEP, r                                  # more circles than a record carries
    seen["kept circles of 64x64 noise"] = r.n_circles
    (h, w), content, dp, ps = STRIP
    r = get((content, h, w), dp, ps)
    assert r.flags == 0 and r.n_circles >= 64 + 10, r             # the serial suppression: more than 64 candidates
    seen["kept circles of the 5x128 strip"] = r.n_circles
    assert curve_nweak["single_wave"] <= 256 < curve_nweak["block_wide"], curve_nweak       # both floods of hg_p3
    seen["weak candidates of the curves"] = (curve_nweak["single_wave"], curve_nweak["block_wide"])
    r = get(("noise", 9, 12), 1.2, PARAM_SETS[3])
    assert radii(9, 12, .30, .30) == (2, 4) and r.n_circles > 0, r         # max <= min: min + 2
    seen["circles of 9x12 noise, max <= min"] = r.n_circles
    r = get(("disc", 40, 40), 1.2, PARAM_SETS[1])
    assert radii(40, 40, 0, 0) == (0, 40) and r.n_circles > 0, r           # max_ratio <= 0: max(w, h)
    seen["circles of the 40x40 disc, max_ratio 0"] = r.n_circles
    r = get(("disc", 64, 64), 16.0, PARAM_SETS[2])
    assert r.n_circles > 0, r                                              # a 4 x 4 accumulator
    seen["circles of the 64x64 disc at dp 16"] = r.n_circles
    cut = 0
    for key in (("noise", 24, 24), ("noise", 9, 12)):
        r = get(key, 2.0, PARAM_SETS[2])
        cut += sum(window(c[2], 2.0, radii(key[1], key[2], .10, 1.0)[0])[0] < 8 for c in r.circles[:KEEP])
    assert cut > 0                                                          # the window cut at bin 0
    seen["returned circles with a cut window"] = cut
    return seen
