"""PieceTone — piece colour per square for the class API (include/cbv.h, "piece colour per square").

The reference detects occupancy only.  PieceTone measures, for the squares `split_board` returns, the mean B, G, R of
the centre disc of `_detect_center_vs_border` (piece_detector.py:184-190) with one kernel launch (cbv_tone_sums_image),
calibrates two centroids per square colour from one frame of a known position, and classifies every square as white,
black or undecided.  The move rules use the answer to break ties (GameState.process_occupancy_change(grid, tones),
StableMoveTracker.process(vision, tones=...)); it never overrides a move they find by themselves.
"""
import numpy as np

from . import _native as N
from . import chess_rules as chess
from ._squares import plan_of


def position_array(position=None):
    """64 bytes in synth.board_array's convention (0 empty, 1 white, 2 black; index 8 * (7 - rank) + file) from such an
    array, a FEN, a {(file, rank): fen_char} dict (synth.position_after) or None = the start position."""
    if position is None or isinstance(position, str):
        b = chess.Board()
        if position is not None:
            b.set_fen(position)
        out = np.zeros(64, np.uint8)
        for sq in range(64):
            p = b.piece_at(sq)
            if p is not None:
                out[(7 - (sq >> 3)) * 8 + (sq & 7)] = 1 if p.color == chess.WHITE else 2
        return out
    if isinstance(position, dict):
        out = np.zeros(64, np.uint8)
        for (f, r), ch in position.items():
            out[(7 - r) * 8 + f] = 1 if ch.isupper() else 2
        return out
    out = np.ascontiguousarray(position, dtype=np.uint8).reshape(-1)
    if out.size != 64 or out.max(initial=0) > 2:
        raise ValueError("a position is 64 bytes of 0 (empty), 1 (white) or 2 (black)")
    return out


def _squares_of(bits):
    return [(i & 7, 7 - (i >> 3)) for i in range(64) if (bits >> i) & 1]


def report_dict(rep):
    """cbv_tone_report as a dict; the two square sets as (file, rank) lists."""
    return {"samples": [[rep.samples[k][p] for p in range(2)] for k in range(2)], "D": [rep.D[0], rep.D[1]],
            "misclassified": _squares_of(rep.misclassified), "undecided": _squares_of(rep.undecided)}


class PieceTone:
    def __init__(self, margin=0.125, ctx=None):
        self.ctx = ctx or N.context()
        self.margin = margin
        self.model = None

    def sums(self, squares):
        """ToneSums[64] in ROI order (8 * (7 - rank) + file) of a {(file, rank): BGR view} dict; a square that is not in
        the dict keeps cnt = 0 and classifies as undecided."""
        plan = plan_of(squares)
        if plan is None or plan[0].cn != 3:  # separate arrays: pack them into one image (a host copy, no arithmetic)
            keys = list(squares.keys())
            arrs = [np.asarray(squares[k]) for k in keys]
            if not arrs or any(a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 for a in arrs):
                raise ValueError("PieceTone needs uint8 HxWx3 (BGR) squares")
            parent = np.zeros((sum(a.shape[0] for a in arrs), max(a.shape[1] for a in arrs), 3), np.uint8)
            y, packed = 0, {}
            for k, a in zip(keys, arrs):
                parent[y:y + a.shape[0], :a.shape[1]] = a
                packed[k] = parent[y:y + a.shape[0], :a.shape[1]]
                y += a.shape[0]
            plan = plan_of(packed)
        img, lay = plan
        n = len(lay.keys)
        got = (N.ToneSums * n)()
        self.ctx.check(self.ctx.lib.cbv_tone_sums_image(self.ctx.h, img, lay.rois, n, got))
        out = (N.ToneSums * 64)()
        for k, rec in zip(lay.keys, got):
            f, r = k
            out[(7 - r) * 8 + f] = rec
        return out

    def calibrate(self, squares, position=None):
        """The model from one frame's squares and the position they show (position_array's forms).  Returns the report."""
        pos = position_array(position)
        model, rep = N.ToneModel(), N.ToneReport()
        self.ctx.check(self.ctx.lib.cbv_tone_calibrate_host(self.sums(squares), N.ptr(pos), float(self.margin), model, rep))
        self.model = model
        return report_dict(rep)

    def classify(self, squares):
        """{(file, rank): "w" | "b" | None} for every square of the dict (an empty square's answer means nothing)."""
        if self.model is None:
            raise RuntimeError("PieceTone.classify: calibrate first (or set .model)")
        import ctypes as C
        w, b = C.c_uint64(), C.c_uint64()
        self.ctx.check(self.ctx.lib.cbv_tone_classify_host(self.model, self.sums(squares), 64, C.byref(w), C.byref(b)))
        out = {}
        for (f, r) in squares.keys():
            i = (7 - r) * 8 + f
            out[(f, r)] = "w" if (w.value >> i) & 1 else "b" if (b.value >> i) & 1 else None
        return out
