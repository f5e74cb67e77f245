"""k_hough (hough_passes.h) through SquareSet.hough at every square size, dp and branch: the inputs, checkers and branch
ledger of tests/hough_cases.py, which test_hough_host.py runs on the CPU oracle.

Layer 1: every record equals the oracle's (tolerance 0), with all squares in one set (the LDS layout of a 128 x 128 square)
and shape by shape (the layout of that shape alone); a square's record does not depend on the set it is in, on its index
there, or on a dp below 1.  Layer 2: the edge count and the support of every returned circle against float64 statements
from ref64, and the list invariants.  Layer 3: n_centres and the centres against the numpy restatement of the vote.  The
ledger: outputs that show each branch of hough_passes.h ran."""
import numpy as np
import pytest

import hough_cases as H
from test_hough_host import oracle_rec, oracle_recs

pytestmark = pytest.mark.gpu

F = np.float32


def gpu_rec(r):
    n = min(int(r.n_circles), H.KEEP)
    cs = [(F(r.circles[k][0]), F(r.circles[k][1]), F(r.circles[k][2]), int(r.circles[k][3])) for k in range(n)]
    found = bool(r.found)
    return H.Rec(int(r.flags), int(r.n_edges), int(r.n_centres), int(r.n_circles), cs, found, F(r.cx) if found else None,
                 F(r.cy) if found else None, F(r.r) if found else None, {0: None, 1: "hough", 2: "tower_top"}[int(r.kind)])


def run_set(gpu_ctx, grays, dp, ps):
    """[(Rec, bytes of the cbv_hough_result)] of the squares loaded as one set: the layout is sized for the largest."""
    from chessboard_vision_amd._squares import GRAY, SquareSet
    ss = SquareSet(gpu_ctx)
    try:
        ss.load({i: g for i, g in enumerate(grays)}, 5)
        for i, g in enumerate(grays):
            ss.set(GRAY, i, g)
        res = ss.hough(dp=dp, param1=ps[0], param2=ps[1], min_radius_ratio=ps[2], max_radius_ratio=ps[3])
        return [(gpu_rec(res[i]), bytes(res[i])) for i in range(len(grays))]
    finally:
        ss.close()


def check_equal(got, want, tag):
    """What test_hough_circles_match_oracle asserts of a record, and the pick through detect_circle_unified."""
    assert got.flags == 0, (tag, got)
    assert got.n_edges == want.n_edges, (tag, got.n_edges, want.n_edges)
    assert got.n_circles == want.n_circles, (tag, got.n_circles, want.n_circles)
    assert got.circles == want.circles[:H.KEEP], (tag, got.circles, want.circles[:H.KEEP])
    assert got.found == want.found, (tag, got, want.found)
    if want.found:
        assert (int(got.cx), int(got.cy), int(got.r), got.kind) == (int(want.cx), int(want.cy), int(want.r), want.kind), (tag, got, want[5:])
    else:
        assert got.kind is None, (tag, got)


_CASES = {}


def case(gpu_ctx, oracle, dp, ps):
    """Every square of the grid at (dp, parameter set), once: {"mixed": {key: (Rec, bytes)}, "tally": ...}."""
    if (dp, ps) in _CASES:
        return _CASES[(dp, ps)]
    P = H.PARAM_SETS[ps]
    want = oracle_recs(oracle, dp, P)
    mixed, tally = {}, {}
    for contents in H.MIXED_SETS:                            # the large layout
        sq = H.squares_of(contents)
        for (key, g), (rec, raw) in zip(sq, run_set(gpu_ctx, [g for _, g in sq], dp, P)):
            check_equal(rec, want[key][1], (key, dp, ps, "mixed"))
            H.check_stages(rec, g, dp, P, (key, dp, ps, "mixed"), tally)
            mixed[key] = (rec, raw)
    for shape in H.SHAPES:                                   # the layout of this shape
        sq = H.squares_of(H.CONTENTS, [shape])
        for (key, g), (rec, raw) in zip(sq, run_set(gpu_ctx, [g for _, g in sq], dp, P)):
            check_equal(rec, want[key][1], (key, dp, ps, "alone"))
            assert raw == mixed[key][1], (key, dp, ps, rec, mixed[key][0])
    _CASES[(dp, ps)] = {"mixed": mixed, "tally": tally}
    return _CASES[(dp, ps)]


@pytest.mark.parametrize("dp,ps", H.case_ids())
def test_kernel(gpu_ctx, oracle, dp, ps):
    print("dp %g set %d: %s" % (dp, ps, case(gpu_ctx, oracle, dp, ps)["tally"]))


def test_support_is_mostly_pinned(gpu_ctx, oracle):
    """Over all cases at least half of the returned circles have strict == loose; prints the measured share and gap."""
    print(H.check_tally([case(gpu_ctx, oracle, dp, ps)["tally"] for dp, ps in H.case_ids()]))


@pytest.mark.parametrize("ps", range(len(H.PARAM_SETS)))
def test_dp_below_one_is_one(gpu_ctx, oracle, ps):
    mixed = case(gpu_ctx, oracle, 1.0, ps)["mixed"]
    for contents in H.MIXED_SETS:
        sq = H.squares_of(contents)
        for (key, _), (rec, raw) in zip(sq, run_set(gpu_ctx, [g for _, g in sq], 0.5, H.PARAM_SETS[ps])):
            assert raw == mixed[key][1], (key, ps, rec, mixed[key][0])


@pytest.mark.parametrize("dp,ps", [(1.0, 1), (1.2, 0), (3.0, 2)])
def test_record_does_not_depend_on_the_index(gpu_ctx, oracle, dp, ps):
    """The squares of a mixed set in reverse order and rotated by 7: the same record for every square."""
    mixed = case(gpu_ctx, oracle, dp, ps)["mixed"]
    sq = H.squares_of(H.MIXED_SETS[0])
    for order in (sq[::-1], sq[7:] + sq[:7]):
        for (key, _), (rec, raw) in zip(order, run_set(gpu_ctx, [g for _, g in order], dp, H.PARAM_SETS[ps])):
            assert raw == mixed[key][1], (key, dp, ps, rec, mixed[key][0])


@pytest.mark.parametrize("name", list(H.CURVES))
@pytest.mark.parametrize("end", ["left", "right", None])
def test_weak_curves(gpu_ctx, oracle, name, end):
    """The hysteresis inside k_hough on a weak curve that hangs on one strong end: the single-wave flood (at most 256 weak
    candidates) and the block-wide one."""
    facts = H.curve_facts(name, end)
    g = H.curve(name, end)
    P = (H.CURVE_PARAM1, 25, .20, .55)
    rec = run_set(gpu_ctx, [g], 1.2, P)[0][0]
    assert rec.n_edges == facts["edges"], (rec.n_edges, facts)
    check_equal(rec, oracle_rec(oracle, g, 1.2, P)[0], (name, end))
    H.check_stages(rec, g, 1.2, P, (name, end), {})


def test_radius_ratio_above_one(gpu_ctx, oracle):
    """max_radius_ratio = 2: the radius histogram has more bins than a side has pixels."""
    ps, shapes, contents = H.WIDE
    sq = H.squares_of(contents, shapes)
    tally = {}
    for (key, g), (rec, _) in zip(sq, run_set(gpu_ctx, [g for _, g in sq], 1.2, ps)):
        check_equal(rec, oracle_rec(oracle, g, 1.2, ps)[0], key)
        H.check_stages(rec, g, 1.2, ps, key, tally)
    assert tally["circles"] > 0, tally


def test_ledger(gpu_ctx, oracle):
    """Every branch of hough_passes.h was reached: see hough_cases.check_ledger.  Each witness square runs alone and equals
    the oracle's record."""
    def get(key, dp, ps):
        g = H.square(*key)
        rec = run_set(gpu_ctx, [g], dp, ps)[0][0]
        check_equal(rec, oracle_rec(oracle, g, dp, ps)[0], (key, dp, ps))
        H.check_stages(rec, g, dp, ps, (key, dp, ps), {})
        return rec
    nweak = {name: H.curve_facts(name, "left")["nweak"] for name in H.CURVES}
    print(H.check_ledger(get, nweak))
