"""The per-square regions and decisions of PieceDetector and ChangeDetector as plain numpy / float64, from pixels:
the centre disc, the corner region and the four rings (piece_detector.py:141-207), the decision chain of detect_piece
without its HoughCircles step (piece_detector.py:303-345), _has_changed (piece_detector.py:82-93), the pixel count and
classes of detect_changes_detailed (change_detector.py:128-150) and _get_stable_detection (piece_detector.py:111-122).

Independent of the C oracle, of the library and of tests/ref_logic.py (none is imported): the masks are built with
numpy's own slice assignments and np.ogrid, the comparisons are the reference's expressions evaluated by numpy on the
pixel arrays themselves, never an integer identity derived from them."""
import numpy as np

RING_RATIOS = (0.15, 0.25, 0.35, 0.45)


def masks(h, w):
    """(centre, border, [ring0..ring3]) boolean (h, w) arrays."""
    cy, cx = h // 2, w // 2
    yy, xx = np.ogrid[:h, :w]
    radius = min(h, w) // 4
    centre = ((xx - cx) ** 2 + (yy - cy) ** 2) <= radius ** 2
    c = min(h, w) // 4
    border = np.zeros((h, w), dtype=bool)
    # four slice assignments: with c == 0, `:0` is empty and `-0:` is `0:`, the whole axis
    border[:c, :c] = True
    border[:c, -c:] = True
    border[-c:, :c] = True
    border[-c:, -c:] = True
    dist = np.sqrt((xx - cx) ** 2 + (yy - cy) ** 2)
    rings = []
    for ratio in RING_RATIOS:
        r = min(h, w) * ratio
        rings.append((dist >= r - 5) & (dist <= r + 5))
    return centre, border, rings


def stats(gray, ref=None, mean=None, var=None, z_thr=2.5):
    """Every field of cbv_sq_stats that is a sum or a count, as Python ints (ring_sum / ring_cnt: lists of four).
    sad_ref is 0 without `ref`, z_count 0 without a model."""
    gray = np.asarray(gray)
    assert gray.dtype == np.uint8 and gray.ndim == 2
    h, w = gray.shape
    centre, border, rings = masks(h, w)
    g = gray.astype(np.int64)
    out = {"n": int(g.size), "sum": int(g.sum()), "sumsq": int((g * g).sum()), "sad_ref": 0,
           "center_sum": int(g[centre].sum()), "center_cnt": int(np.count_nonzero(centre)),
           "border_sum": int(g[border].sum()), "border_cnt": int(np.count_nonzero(border)),
           "ring_sum": [int(g[m].sum()) for m in rings], "ring_cnt": [int(np.count_nonzero(m)) for m in rings], "z_count": 0}
    if ref is not None:
        out["sad_ref"] = int(np.abs(g - np.asarray(ref).astype(np.int64)).sum())
    if mean is not None:
        out["z_count"] = change_class(gray.astype(np.float32), mean, var, z_thr)[0]
    return out


INT_FIELDS = ("n", "sum", "sumsq", "sad_ref", "center_sum", "center_cnt", "border_sum", "border_cnt", "z_count")


def stats_of_struct(st):
    """The same dict from a cbv_sq_stats / orc_sq_stats ctypes record."""
    out = {k: int(getattr(st, k)) for k in INT_FIELDS}
    out["ring_sum"] = [int(st.ring_sum[k]) for k in range(4)]
    out["ring_cnt"] = [int(st.ring_cnt[k]) for k in range(4)]
    return out


def center_border_diff(gray):
    centre, border, _ = masks(*gray.shape)
    return abs(np.mean(gray[centre]) - np.mean(gray[border]))


def radial_symmetry(gray):
    _, _, rings = masks(*gray.shape)
    ring_means = [np.mean(gray[m]) for m in rings if np.sum(m) > 0]
    if len(ring_means) < 2:
        return 0.0
    return min(1.0, np.var(ring_means) / 500)


def std_below_15(gray):
    """The uniformity pre-filter exactly as numpy evaluates it on the array.  The reference's squares come out of
    cv2.GaussianBlur, rows after rows in memory, and numpy adds in memory order: the array is brought to that layout."""
    return bool(np.std(np.ascontiguousarray(gray)) < 15)


def detect_piece_no_hough(gray, circle_threshold=0.6):
    """detect_piece on an already preprocessed gray square, its HoughCircles step left out."""
    gray = np.ascontiguousarray(gray)  # as cv2.GaussianBlur returns it: numpy's sums run in memory order
    h, w = gray.shape
    res = {"has_piece": False, "method": None, "center": None, "radius": None, "confidence": 0.0, "center_border_diff": 0}
    if np.std(gray) < 15:
        return res
    diff = center_border_diff(gray)
    res["center_border_diff"] = diff
    if diff > 40:
        res.update(has_piece=True, method="center_diff", center=(w // 2, h // 2), radius=min(h, w) // 3, confidence=min(1.0, diff / 80))
        return res
    symmetry = radial_symmetry(gray)
    if symmetry > circle_threshold:
        res.update(has_piece=True, method="symmetry", center=(w // 2, h // 2), radius=min(h, w) // 3, confidence=symmetry)
    return res


def has_changed(gray, ref, thr):
    """np.mean(cv2.absdiff(gray, ref)) > thr for uint8 arrays."""
    diff = np.abs(np.asarray(gray).astype(np.int16) - np.asarray(ref).astype(np.int16)).astype(np.uint8)
    return bool(np.mean(diff) > thr)


def change_class(gray_f32, mean, var, z_thr):
    """(z_count, pct, in_result, intensity) of one square; intensity is None when the square is not reported."""
    gray_f32 = np.asarray(gray_f32)
    assert gray_f32.dtype == np.float32
    std_dev = np.sqrt(np.asarray(var, np.float32))
    z = np.abs(gray_f32 - np.asarray(mean, np.float32)) / std_dev
    count = int(np.count_nonzero(z > z_thr))
    pct = (count / gray_f32.size) * 100
    if pct < 5.0:
        return count, pct, False, None
    if pct > 75:
        return count, pct, True, "TOTAL"
    if pct > 15:
        return count, pct, True, "PARCIAL"
    return count, pct, True, "LEVE"


def stable(history, history_size, min_presence):
    """_get_stable_detection after the raw results `history` (oldest first) were appended one by one."""
    hist = list(history)[-history_size:]
    if len(hist) < 3:
        return hist[-1] if hist else False
    return sum(hist) / len(hist) >= min_presence
