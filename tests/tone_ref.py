"""Piece colour per square (include/cbv.h, "piece colour per square") restated in numpy and plain Python floats: the
np.ogrid disc of _detect_center_vs_border, the tone sums, calibration and classification in float64, one rounding per
operation in the header's order.  The kernel and the host calls are held to this bit for bit."""
import numpy as np


def disc_mask(h, w):
    """piece_detector.py:184-190: the centre disc of an h x w square."""
    y, x = np.ogrid[:h, :w]
    cy, cx, r = h // 2, w // 2, min(w, h) // 4
    return (x - cx) ** 2 + (y - cy) ** 2 <= r * r


def tone_sums(board, rois):
    """[n, 4] uint32 (sum B, sum G, sum R, pixels) of the (x0, y0, w, h) rois of an HxWx3 uint8 board."""
    out = np.zeros((len(rois), 4), np.uint32)
    for i, (x0, y0, w, h) in enumerate(rois):
        sq = board[y0:y0 + h, x0:x0 + w].astype(np.int64)
        m = disc_mask(h, w)
        out[i, :3] = sq[m].sum(axis=0)
        out[i, 3] = int(m.sum())
    return out


def square_colour(roi):
    return ((roi >> 3) + (roi & 7)) & 1  # 1 = dark


def _f(rec):
    n = float(rec[3])
    return [float(rec[0]) / n, float(rec[1]) / n, float(rec[2]) / n]


def _dist2(a, b):
    e0, e1, e2 = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return (e0 * e0 + e1 * e1) + e2 * e2


def classify_one(centroid, margin, roi, rec):
    """"w", "b" or None for ROI `roi` with sums `rec` = (b, g, r, n); centroid[k][p] = [b, g, r] as Python floats."""
    if int(rec[3]) == 0:
        return None
    k = square_colour(roi)
    cW, cB = centroid[k][0], centroid[k][1]
    f = _f(rec)
    dW, dB, D = _dist2(f, cW), _dist2(f, cB), _dist2(cW, cB)
    T = (2.0 * margin) * D
    if dB - dW >= T:
        return "w"
    if dW - dB >= T:
        return "b"
    return None


def classify(centroid, margin, sums):
    """(white word, black word) of sums[n][4], index = ROI."""
    white = black = 0
    for i, rec in enumerate(sums):
        t = classify_one(centroid, margin, i, rec)
        if t == "w":
            white |= 1 << i
        elif t == "b":
            black |= 1 << i
    return white, black


def calibrate(sums, position, margin=0.125):
    """(centroid[2][2][3] as nested lists of floats, report dict) from sums[64][4] and 64 bytes (0 empty, 1 white,
    2 black); None when a class is empty or the two centroids of a square colour coincide."""
    acc = [[[0.0, 0.0, 0.0] for _ in range(2)] for _ in range(2)]
    cnt = [[0, 0], [0, 0]]
    for i in range(64):
        p = int(position[i])
        if not p:
            continue
        if int(sums[i][3]) == 0:
            return None
        k, f = square_colour(i), _f(sums[i])
        for c in range(3):
            acc[k][p - 1][c] = acc[k][p - 1][c] + f[c]
        cnt[k][p - 1] += 1
    if min(min(c) for c in cnt) == 0:
        return None
    centroid = [[[acc[k][p][c] / float(cnt[k][p]) for c in range(3)] for p in range(2)] for k in range(2)]
    D = [_dist2(centroid[k][0], centroid[k][1]) for k in range(2)]
    if 0.0 in D:
        return None
    mis = und = 0
    for i in range(64):
        p = int(position[i])
        if p:
            t = classify_one(centroid, margin, i, sums[i])
            if t is None:
                und |= 1 << i
            elif t != "wb"[p - 1]:
                mis |= 1 << i
    return centroid, {"samples": cnt, "D": D, "misclassified": mis, "undecided": und}


def true_tones(pos):
    """(white, black) ROI words of a {(file, rank): fen_char} position."""
    white = black = 0
    for (f, r), ch in pos.items():
        if ch.isupper():
            white |= 1 << ((7 - r) * 8 + f)
        else:
            black |= 1 << ((7 - r) * 8 + f)
    return white, black
