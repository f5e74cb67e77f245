"""HoughCircles per square on the CPU: the oracle's restatement (orc_hough_circles) under the checkers and inputs of
tests/hough_cases.py, which test_gpu_hough_edges.py runs on k_hough, plus the preconditions of the branch ledger.  The
oracle's edge count and the support of its circles have to meet float64 statements from ref64; its accumulator maxima a third
restatement of the vote in numpy.  A failure of the kernel's test that does not show here is the kernel's."""
import numpy as np
import pytest

import hough_cases as H

F = np.float32


def oracle_rec(oracle, gray, dp, ps):
    """(Rec, counts, candidates): the oracle's record of a square, in the shape of cbv_hough_result (every circle, not the
    first six), its (maxima, candidates, circles) counts and the sorted circles before the minDist suppression."""
    from ref_logic import detect_circle_unified
    param1, param2, min_ratio, max_ratio = ps
    m = min(gray.shape)
    found, center, radius, kind, circles = detect_circle_unified(gray, min_ratio, max_ratio, param1, param2, dp=dp)
    _, edges, counts, cands = oracle.hough_circles(gray, dp, m // 3, param1, param2, int(m * min_ratio), int(m * max_ratio), return_edges=True,
                                                   return_counts=True, return_candidates=True, max_out=gray.size)
    assert counts[2] == len(circles) and counts[1] == len(cands)
    cs = [(F(x), F(y), F(r), int(v)) for (x, y, r, v) in circles]
    pick = None
    if found:                                    # the circle behind (int(cx), int(cy)), int(r): the same loop, kept whole
        best = np.inf
        for c in cs:
            dist = np.sqrt((c[0] - (gray.shape[1] // 2)) ** 2 + (c[1] - (gray.shape[0] // 2)) ** 2)
            if dist < m * 0.3 and dist < best:
                best, pick = dist, c
        assert (int(pick[0]), int(pick[1])) == center and int(pick[2]) == radius
    return H.Rec(0, int((edges > 0).sum()), counts[0], len(cs), cs, found, pick[0] if found else None, pick[1] if found else None,
                 pick[2] if found else None, kind), counts, [(F(x), F(y), F(r), int(v)) for (x, y, r, v) in cands]


_RECS = {}


def oracle_recs(oracle, dp, ps):
    """{key: (gray, Rec, candidates)} of every square of the grid at (dp, parameter set), computed once."""
    if (dp, ps) not in _RECS:
        _RECS[(dp, ps)] = {}
        for key, g in H.squares_of(H.CONTENTS):
            rec, _, cands = oracle_rec(oracle, g, dp, ps)
            _RECS[(dp, ps)][key] = (g, rec, cands)
    return _RECS[(dp, ps)]


def test_inputs():
    keys = [k for k, _ in H.squares_of(H.CONTENTS)]
    assert len(keys) == len(set(keys)) == 80 and sorted({w % 4 for (_, h, w) in keys if h == 33}) == [0, 1, 2, 3]
    for contents in H.MIXED_SETS:
        sq = H.squares_of(contents)
        assert len(sq) <= 64 and any(g.shape == (128, 128) for _, g in sq)
    assert len({g.tobytes() for _, g in H.squares_of(H.CONTENTS)}) >= 80 - 15     # (a constant square per shape; 2 x 2 blurs flat)
    assert H.radii(9, 12, .30, .30) == (2, 4) and H.radii(40, 64, 0, 0) == (0, 64) and H.radii(77, 77, .2, .55) == (15, 42)
    assert H.n_bins(1.2, 2, 4) == 17 and H.n_bins(16.0, 2, 4) == 1 and H.n_bins(0.5, 0, 4) == 40
    assert H.window(4 + 1.2 * 0.05 * 30, 1.2, 4) == (30, 10, 20) and H.window(4.24, 1.2, 4) == (4, -1, 5) and H.window(4.48, 1.2, 4) == (8, -1, 9)


def test_accumulator_known_answer():
    """A vertical step: every edge pixel has the gradient (4a, 0), steps 1024 / dp cells along x, and votes once per radius in
    both directions until it leaves the accumulator; the maxima follow the tie rule."""
    g = np.full((6, 8), 50, np.uint8)
    g[:, 4:] = 90
    acc = H.accumulator(g, 1.0, 100, 1, 2)
    want = np.zeros((8, 10), np.int32)
    want[0:6, [1, 2, 4, 5]] = 1                    # the edge column is x = 3: cells 3 -+ 1, 3 -+ 2
    assert np.array_equal(acc, want)
    # dp = 2: rows pair up; from x = 1.5 cells the walk visits 2, 2.5 and 1, 0.5
    assert np.array_equal(H.accumulator(g, 2.0, 100, 1, 2)[:3, :4], [[2, 2, 4, 0]] * 3)
    flat = np.zeros((5, 6), np.int32)
    flat[1:4, 1:5] = 3
    assert np.array_equal(np.argwhere(H.maxima(flat, 2)), [[0, 0]]) and not H.maxima(flat, 3).any()   # > left and up, >= right and down


_TALLY = {}


def stage_tally(oracle, dp, ps):
    """Layer 2 and 3 on every square of the grid at (dp, parameter set), once; the tally of its circles."""
    if (dp, ps) not in _TALLY:
        tally = {}
        for key, (g, rec, cands) in oracle_recs(oracle, dp, H.PARAM_SETS[ps]).items():
            H.check_stages(rec, g, dp, H.PARAM_SETS[ps], (key, dp, ps), tally)
            kept = H.suppress(cands, g.shape[0], g.shape[1], dp)      # the oracle's suppression on its own candidates
            assert kept == rec.circles, (key, dp, ps, len(kept), len(rec.circles))
            tally["at_min_dist"] = tally.get("at_min_dist", 0) + H.pairs_at_min_dist(rec.circles, g.shape[0], g.shape[1], dp)
        _TALLY[(dp, ps)] = tally
    return _TALLY[(dp, ps)]


@pytest.mark.parametrize("dp,ps", H.case_ids())
def test_oracle_stages(oracle, dp, ps):
    """Layer 2 and 3 on the oracle: edge count, support sandwich, list invariants, number of maxima and centres."""
    print("dp %g set %d: %s" % (dp, ps, stage_tally(oracle, dp, ps)))


def test_oracle_support_is_mostly_pinned(oracle):
    """Over all cases at least half of the circles have strict == loose: the sandwich pins their support to one number.
    (Cell centres sit at half-integers, so distances on a bin's edge are real; wide bins at dp = 16 have the most.)"""
    tallies = [stage_tally(oracle, dp, ps) for dp, ps in H.case_ids()]
    print(H.check_tally(tallies))
    assert sum(t["at_min_dist"] for t in tallies) > 0      # kept pairs exactly minDist apart: `<` and `<=` differ on them


def test_oracle_dp_below_one_is_one(oracle):
    for ps in H.PARAM_SETS[:3]:
        for key, g in H.squares_of(("blurred", "disc"), [(33, 30), (40, 40)]):
            assert oracle_rec(oracle, g, 0.5, ps) == oracle_rec(oracle, g, 1.0, ps), (key, ps)


def test_oracle_radius_ratio_above_one(oracle):
    ps, shapes, contents = H.WIDE
    tally = {}
    for key, g in H.squares_of(contents, shapes):
        H.check_stages(oracle_rec(oracle, g, 1.2, ps)[0], g, 1.2, ps, key, tally)
    assert tally["circles"] > 0, tally


@pytest.mark.parametrize("name", list(H.CURVES))
@pytest.mark.parametrize("end", ["left", "right", None])
def test_oracle_curves(oracle, name, end):
    facts = H.curve_facts(name, end)
    g = H.curve(name, end)
    rec = oracle_rec(oracle, g, 1.2, (H.CURVE_PARAM1, 25, .20, .55))[0]
    assert rec.n_edges == facts["edges"], (rec.n_edges, facts)
    H.check_stages(rec, g, 1.2, (H.CURVE_PARAM1, 25, .20, .55), (name, end), {})


def test_oracle_ledger(oracle):
    """The witnesses of the branch ledger exist in the reference, so a kernel that misses one is wrong."""
    def get(key, dp, ps):
        return oracle_rec(oracle, H.square(*key), dp, ps)[0]
    nweak = {name: H.curve_facts(name, "left")["nweak"] for name in H.CURVES}
    print(H.check_ledger(get, nweak))
    (h, w), content, dp, ps = H.STRIP
    counts = oracle_rec(oracle, H.square(content, h, w), dp, ps)[1]
    assert counts[1] >= counts[2] > 64, counts                    # the strip: nothing is near enough to suppress
    counts = oracle_rec(oracle, H.square("noise", 24, 24), 1.0, H.PARAM_SETS[2])[1]
    assert counts[1] > 64 + 10 > counts[2] > 0, counts            # a square of the grid where the serial branch suppresses
