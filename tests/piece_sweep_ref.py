"""The yardstick of the PieceDetector settings sweep (cbv_pipeline_piece_sweep): a 640x480 stream of 12 frames on the raw
chain (synth -> warp_image -> split_board, no enhancement) with a low-contrast palette under which most pieces are decided
by HoughCircles alone, 18 settings, and the restated reference class (ref_logic.RefPieceDetector, pinned to the reference by
tests/golden/ref_piece_settings.json) driven as include/cbv.h defines a setting: a fresh detector per setting,
detect_all_pieces(squares, use_smoothing=True, squares_to_check=<all 64>) on the frames in order.  Nothing here touches the
code under test except `eval_host`, which calls it."""
import functools

import numpy as np

from chessboard_vision_amd import synth as S

W, H = 640, 480
N_FRAMES, FRAMES_PER_PLY = 12, 4
PALETTE = dict(bg_lo=60, bg_span=31, light=(190, 200, 210), dark=(90, 110, 135), white=(150, 160, 170), black=(120, 140, 165),
               noise=3, radius=0.36)
# (min_radius_ratio, max_radius_ratio, param1, param2)
SETTINGS = ((.20, .55, 100, 25), (.25, .55, 100, 25), (.25, .55, 100, 30), (.01, .25, 100, 25), (.12, .30, 100, 25), (.30, .42, 100, 25),
            (.38, .42, 100, 25), (.50, .70, 100, 25), (.01, .70, 100, 25), (.20, .55, 100, 45), (.20, .55, 100, 60), (.20, .55, 100, 10),
            (.20, .55, 100, 1), (.20, .55, 40, 25), (.20, .55, 200, 25), (.12, .19, 100, 10), (.34, .40, 100, 25), (.36, .70, 100, 25))
FIXTURE_SETTINGS = (0, 3, 12, 13)  # the settings recorded from the reference's own class (first 6 frames)
FIXTURE_FRAMES = 6
ROI_POS = [(c, 7 - r) for r in range(8) for c in range(8)]  # roi index = 8 * row + col, row 0 = rank 8
ALL_SQUARES = frozenset(ROI_POS)
METHODS = ("hough", "tower_top", "center_diff", "symmetry")


def hough_kw(s):
    return dict(min_radius_ratio=s[0], max_radius_ratio=s[1], param1=s[2], param2=s[3])


def oracle_scene():
    from oracle import cbv_oracle as O
    sc = O.Scene()
    sc.bg_lo, sc.bg_span, sc.noise, sc.radius = PALETTE["bg_lo"], PALETTE["bg_span"], PALETTE["noise"], PALETTE["radius"]
    for k in ("light", "dark", "white", "black"):
        for i in range(3):
            getattr(sc, k)[i] = PALETTE[k][i]
    return sc


def native_scene():
    from chessboard_vision_amd import _native as N
    return N.Scene.from_dict(PALETTE)


def frame(i, frames_per_ply=FRAMES_PER_PLY, w=W, h=H):
    from oracle import cbv_oracle as O
    Hinv = O.get_perspective_transform(S.scaled_corners(w, h), S.BOARD_UNIT_QUAD)
    board = S.board_array(S.position_for_frame(i, frames_per_ply))
    return O.synth_frame(S.frame_seed(0, i), w, h, Hinv, board, oracle_scene())


@functools.lru_cache(maxsize=None)
def stream_squares(n=N_FRAMES, frames_per_ply=FRAMES_PER_PLY, grid=None, display_size=(1280, 720)):
    """Per frame the {(file, rank): BGR square} dict of the raw chain.  `grid`: None = GridExtractor, else
    (grid_lines_x, grid_lines_y) tuples for SmartGridExtractor."""
    from oracle import cbv_oracle as O
    from chessboard_vision_amd.grid_extractor import GridExtractor, SmartGridExtractor
    pts = S.scaled_corners(W, H)
    if grid is None:
        ge = GridExtractor()
    else:
        ge = SmartGridExtractor()
        ge.grid_lines_x, ge.grid_lines_y = list(grid[0]), list(grid[1])
    return [ge.split_board(O.warp_image(frame(i, frames_per_ply), pts, display_size=display_size)[0]) for i in range(n)]


def bits(positions):
    """{(file, rank)} -> roi bitset"""
    m = 0
    for pos in positions:
        m |= 1 << ROI_POS.index(tuple(pos))
    return m


def expected_bits(n=N_FRAMES, frames_per_ply=FRAMES_PER_PLY):
    """the scripted position of every frame as roi bitsets"""
    return [bits(S.position_for_frame(i, frames_per_ply).keys()) for i in range(n)]


@functools.lru_cache(maxsize=None)
def run_setting(s, n=N_FRAMES, frames_per_ply=FRAMES_PER_PLY, grid=None, display_size=(1280, 720)):
    """The definition: per frame (results, raw) of a fresh RefPieceDetector with setting s; `results` is detect_all_pieces'
    dict (has_piece smoothed), `raw` = detect_piece's dict of every square of that frame."""
    from ref_logic import RefPieceDetector
    det = RefPieceDetector(hough=hough_kw(s))
    out = []
    for sq in stream_squares(n, frames_per_ply, grid, display_size):
        res, _ = det.detect_all_pieces(sq, use_smoothing=True, squares_to_check=set(sq.keys()))
        assert det.last_processed == set(sq.keys())
        out.append((res, {pos: dict(r) for pos, r in det.cached_results.items()}))
    return out


def record_of(results, raw):
    """cbv_piece_sweep_record's fields of one (setting, frame) from the yardstick's dicts"""
    rec = {"raw_occupied": bits(p for p, r in raw.items() if r["has_piece"]),
           "stable_occupied": bits(p for p, r in results.items() if r["has_piece"])}
    for m in METHODS:
        rec[m] = bits(p for p, r in raw.items() if r["has_piece"] and r["method"] == m)
    radii = [r["radius"] for r in raw.values() if r["has_piece"] and r["method"] in ("hough", "tower_top")]
    rec["r_min"], rec["r_max"] = (min(radii), max(radii)) if radii else (0, 0)
    rec["n_raw"], rec["n_stable"] = bin(rec["raw_occupied"]).count("1"), bin(rec["stable_occupied"]).count("1")
    rec["flags"] = 0
    rec["_radii"] = radii
    return rec


REC_FIELDS = ("raw_occupied", "stable_occupied") + METHODS + ("r_min", "r_max", "n_raw", "n_stable", "flags")
SUM_FIELDS = ("frames", "frames_exact", "missed", "false_pos", "n_hough", "n_tower_top", "n_center_diff", "n_symmetry", "r_min", "r_max", "n_r",
              "overflow", "r_sum")


@functools.lru_cache(maxsize=None)
def yardstick_records(n=N_FRAMES, frames_per_ply=FRAMES_PER_PLY, grid=None, display_size=(1280, 720), settings=SETTINGS):
    """[setting][frame] record dicts"""
    return [[record_of(*fr) for fr in run_setting(s, n, frames_per_ply, grid, display_size)] for s in settings]


def assert_records_equal(got, want, what):
    """got: [S, F] structured array (or None-free slice of it); want: [S][F] dicts"""
    assert got.shape == (len(want), len(want[0])), (what, got.shape)
    for j, row in enumerate(want):
        for i, rec in enumerate(row):
            for name in REC_FIELDS:
                assert int(got[name][j, i]) == rec[name], (what, j, i, name, int(got[name][j, i]), rec[name])


def same_records(a, b):
    """two record arrays field by field (a copy numpy makes leaves the struct's pad byte unset)"""
    return a.dtype == b.dtype and a.shape == b.shape and all(np.array_equal(a[name], b[name]) for name in a.dtype.names)


def reduce_records(rec, expected=None, radii=None):
    """cbv_piece_sweep_summary of every setting from its records ([S, F] structured array).  The radius sum and count are
    not in the records: `radii` = [S][F] lists of int(r), else r_sum / n_r are left out of the comparison by the caller."""
    from chessboard_vision_amd import _native as N
    out = np.zeros(rec.shape[0], N.record_dtype(N.PieceSweepSummary))
    pop = np.vectorize(lambda v: bin(int(v)).count("1"), otypes=[np.int64])
    out["frames"] = rec.shape[1]
    if expected is not None:
        e = np.array(expected, np.uint64)[None, :]
        out["frames_exact"] = (rec["stable_occupied"] == e).sum(axis=1)
        out["missed"] = pop(e & ~rec["stable_occupied"]).sum(axis=1)
        out["false_pos"] = pop(rec["stable_occupied"] & ~e).sum(axis=1)
    for m in METHODS:
        out["n_" + m] = pop(rec[m]).sum(axis=1)
    has = (rec["hough"] | rec["tower_top"]) != 0
    out["n_r"] = pop(rec["hough"] | rec["tower_top"]).sum(axis=1)
    for j in range(rec.shape[0]):
        if has[j].any():
            out["r_min"][j], out["r_max"][j] = rec["r_min"][j][has[j]].min(), rec["r_max"][j][has[j]].max()
    out["overflow"] = 0
    if radii is not None:
        out["r_sum"] = [sum(sum(fr) for fr in row) for row in radii]
    return out


@functools.lru_cache(maxsize=None)
def oracle_inputs(n=N_FRAMES, frames_per_ply=FRAMES_PER_PLY, settings=SETTINGS):
    """What the host twin reads, from the oracle alone: ([frames, 64] SqStats records, ws, hs, [S, frames, 64] PieceChoice
    records): the oracle's statistics of every square and ref_logic.detect_circle_unified's pick per setting."""
    from chessboard_vision_amd import _native as N
    from oracle import cbv_oracle as O
    from ref_logic import detect_circle_unified
    sq = stream_squares(n, frames_per_ply)
    stats = np.zeros((n, 64), N.record_dtype(N.SqStats))
    ch = np.zeros((len(settings), n, 64), N.record_dtype(N.PieceChoice))
    ws, hs = np.zeros(64, np.int32), np.zeros(64, np.int32)
    for f in range(n):
        for roi, pos in enumerate(ROI_POS):
            gray = O.square_preprocess(sq[f][pos], 5)
            hs[roi], ws[roi] = gray.shape
            st = O.square_stats(gray)
            for name in ("n", "sum", "sumsq", "center_sum", "center_cnt", "border_sum", "border_cnt"):
                stats[name][f, roi] = getattr(st, name)
            stats["ring_sum"][f, roi] = list(st.ring_sum)
            stats["ring_cnt"][f, roi] = list(st.ring_cnt)
            if np.std(gray) < 15:
                continue  # detect_piece returns before HoughCircles
            for j, s in enumerate(settings):
                found, center, radius, kind, _ = detect_circle_unified(gray, **hough_kw(s))
                if found:
                    ch[j, f, roi] = ({"hough": 1, "tower_top": 2}[kind], 0, radius, center[0], center[1])
    return stats, ws, hs, ch


def eval_host(stats, ws, hs, choices, expected=None):
    """cbv_piece_sweep_eval_host: ([S, F] records, [S] summaries)"""
    from chessboard_vision_amd import _native as N
    lib = N.load()
    ns, frames, n = choices.shape
    rec = np.zeros((ns, frames), N.record_dtype(N.PieceSweepRecord))
    summ = np.zeros(ns, N.record_dtype(N.PieceSweepSummary))
    exp = np.array(expected, np.uint64) if expected is not None else None
    st, ch = np.ascontiguousarray(stats), np.ascontiguousarray(choices)
    rc = lib.cbv_piece_sweep_eval_host(N.ptr(st), N.ptr(np.ascontiguousarray(ws)), N.ptr(np.ascontiguousarray(hs)), n, frames, N.ptr(ch), ns,
                                       N.ptr(exp) if exp is not None else None, N.ptr(rec), N.ptr(summ))
    assert rc == 0, rc
    return rec, summ
