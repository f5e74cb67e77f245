"""GameState — drop-in for game_state.py on the native rules engine.

`process_occupancy_change` is one native call (cbv_game_process_occupancy,
include/cbv_chess.h) that restates game_state.py:40-195: diff the vision
occupancy against the board, recognise normal move (auto-queen promotion),
castling, en passant and capture, and push the move when it is legal.  The
statuses are the reference's strings.  `self.board` is a
`chess_rules.Board` with the python-chess surface the application touches
(game_session.py:147-380).
"""
import ctypes as C

from . import chess_rules as chess


def _bits(squares):
    bits = 0
    for f, r in squares:
        bits |= 1 << chess.square(f, r)
    return bits


class GameState:
    def __init__(self):
        self.board = chess.Board()

    def get_fen(self):
        return self.board.fen()

    def get_turn(self):
        return self.board.turn

    def get_turn_name(self):
        return "white" if self.board.turn == chess.WHITE else "black"

    def get_legal_moves(self):
        return list(self.board.legal_moves)

    def get_legal_moves_from(self, file, rank):
        src = chess.square(file, rank)
        return [m for m in self.board.legal_moves if m.from_square == src]

    def get_board_occupancy(self):
        """{(file, rank)} of the occupied squares, a1 = (0, 0) (game_state.py:26-38)."""
        bits = self.board.occupancy_bits()
        return {(s & 7, s >> 3) for s in range(64) if (bits >> s) & 1}

    def process_occupancy_change(self, vision_occupancy_grid, tones=None):
        """(move, status) like game_state.py:40-112; the board is advanced when a move is confirmed.  `tones`: (white,
        black) sets of (file, rank) squares whose piece looks white / black (BoardPipeline.piece_colours), which break
        the tie of a capture with two possible victims (include/cbv_chess.h) and change nothing else."""
        return self.process_occupancy_bits(_bits(vision_occupancy_grid), None if tones is None else (_bits(tones[0]), _bits(tones[1])))

    def process_occupancy_bits(self, square_bits, tones=None):
        """Same, from an occupancy word (bit = python-chess square), e.g.
        chess_rules.roi_bits_to_squares(frame_result.stable_occupied); `tones` = (white, black) words in the same numbering."""
        lib = chess._L()
        code = C.c_uint16(chess.MOVE_NONE)
        if tones is None:
            status = lib.cbv_game_process_occupancy(self.board._h, square_bits, C.byref(code))
        else:
            status = lib.cbv_game_process_occupancy_tones(self.board._h, square_bits, tones[0], tones[1], C.byref(code))
        return chess.Move._from_code(code.value), lib.cbv_game_status_name(status).decode()

    def radar(self, vision_occupied):
        """GameSession._update_radar_ui (game_session.py:271-291): (lifted square or None, [destinations]) as
        (file, rank) pairs — the one expected square vision misses, when its piece belongs to the side to move, and
        where that piece may go."""
        lifted = self.get_board_occupancy() - set(vision_occupied)
        if len(lifted) != 1:
            return None, []
        (f, r), = lifted
        piece = self.board.piece_at(chess.square(f, r))
        if not piece or piece.color != self.board.turn:
            return None, []
        return (f, r), [(chess.square_file(m.to_square), chess.square_rank(m.to_square)) for m in self.get_legal_moves_from(f, r)]

    def sync_moves(self, moves_str):
        """LichessSession._sync_moves' replay (lichess_session.py:99-105): reset, then every UCI token that is legal."""
        self.board.reset()
        for uci in (moves_str or "").split():
            try:
                self.board.push_uci(uci)
            except (ValueError, IndexError):
                pass

    def reset(self):
        self.board.reset()

    def set_fen(self, fen):
        self.board.set_fen(fen)


class FrameClock:
    """Time in frames for StableMoveTracker: a batched run has no wall clock, so the device session (include/cbv.h,
    cbv_pipeline_session_begin) counts frames, and a host tracker that shall agree with it does the same.  `tick()` once
    per frame before `process`; calling the clock returns the frame counter (1 for the first frame)."""

    def __init__(self):
        self.frame = 0

    def tick(self):
        self.frame += 1
        return self.frame

    def __call__(self):
        return self.frame


class StableMoveTracker:
    """The move-acceptance logic of GameSession._process_stable_move / _infer_move (game_session.py:181-265)
    without its UI and network side: an occupancy must stay identical for STABILITY_REQUIRED frames, differ from
    the board by at most 4 squares, the cooldown since the last move must have passed and the NoiseHandler must not
    report NOISE_ACTIVE; then exactly one legal move has to explain the difference.

    `on_move_detected(move) -> bool` is the reference's hook (True = apply locally); `after_move()` is where the
    session refreshes the detector references and resets the noise handler (game_session.py:220-223)."""

    STABILITY_REQUIRED = 20
    MOVE_COOLDOWN = 2.0

    def __init__(self, game, clock=None, on_move_detected=None, after_move=None, rule="session"):
        import time
        if rule not in ("session", "game_state"):
            raise ValueError("rule %r: expected 'session' (GameSession._infer_move) or 'game_state' (process_occupancy_change)" % (rule,))
        self.rule = rule
        self.last_status = None  # rule "game_state": the status string of the last process_occupancy_change
        self.game = game
        self.clock = clock or time.time
        self.on_move_detected = on_move_detected or (lambda move: True)
        self.after_move = after_move or (lambda: None)
        self.stable_occupancy = None
        self.stable_count = 0
        self.last_move_time = 0

    def use_frame_clock(self, fps=30, cooldown_frames=None):
        """Count time in frames, as the device session does: MOVE_COOLDOWN becomes `cooldown_frames` (default
        round(MOVE_COOLDOWN * fps): what "2.0 s" means at that frame rate), the clock a FrameClock the caller ticks once
        per frame, and no cooldown holds before the first move (the reference's last_move_time = 0 against time.time()).
        Returns the clock."""
        if cooldown_frames is None:
            cooldown_frames = int(round(type(self).MOVE_COOLDOWN * fps))
        self.MOVE_COOLDOWN = cooldown_frames
        self.clock = FrameClock()
        self.last_move_time = float("-inf")
        return self.clock

    def infer_move(self, vision_occupied, tones=None):
        """(move or None, number of candidate moves) — game_session.py:229-265.  `tones` = (white_set, black_set) of
        (file, rank) squares: with more than one candidate, the one whose destination does not look like a piece of
        the side not to move, if it is the only one (the count stays the number of candidates)."""
        lib = chess._L()
        code = C.c_uint16(chess.MOVE_NONE)
        if tones is None:
            n = lib.cbv_game_infer_move(self.game.board._h, _bits(vision_occupied), C.byref(code))
        else:
            n = lib.cbv_game_infer_move_tones(self.game.board._h, _bits(vision_occupied), _bits(tones[0]), _bits(tones[1]), C.byref(code))
        return chess.Move._from_code(code.value), n

    def process(self, vision_occupied, noise_active=False, tones=None):
        """One frame; returns the move that was pushed on the board, or None.  `tones` = (white_set, black_set): the
        frame's piece colours, for the rules' tie-break."""
        expected = self.game.get_board_occupancy()
        total_diff = len(expected - vision_occupied) + len(vision_occupied - expected)
        if total_diff > 4:                       # a hand or noise: start over
            self.stable_count = 0
            self.stable_occupancy = set()
        elif self.stable_occupancy == vision_occupied:
            self.stable_count += 1
        else:
            self.stable_occupancy = set(vision_occupied)
            self.stable_count = 1
        now = self.clock()
        if self.stable_count < self.STABILITY_REQUIRED or not (now - self.last_move_time) > self.MOVE_COOLDOWN or noise_active:
            return None
        if self.rule == "game_state":  # process_occupancy_change recognises and pushes in one step
            # (without tones the calls are the ones that were always made: callers wrap and replace these methods)
            move, self.last_status = (self.game.process_occupancy_change(vision_occupied) if tones is None
                                      else self.game.process_occupancy_change(vision_occupied, tones))
            if move is None:
                return None
        else:
            move, _ = self.infer_move(vision_occupied) if tones is None else self.infer_move(vision_occupied, tones)
            if move is None or not self.on_move_detected(move):
                return None
            if move not in self.game.board.legal_moves:
                return None
            self.game.board.push(move)
        self.last_move_time = now
        self.after_move()
        self.stable_count = 0
        return move


def smart_scan_squares(game):
    """The `squares_to_check` set GameSession builds between full scans (game_session.py:130-152): occupied squares
    plus, for every legal move, (file, 7 - rank) of its destination — the reference's own conversion, kept as is."""
    out = set(game.get_board_occupancy())
    for m in game.board.legal_moves:
        out.add((chess.square_file(m.to_square), 7 - chess.square_rank(m.to_square)))
    return out
