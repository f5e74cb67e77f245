// Game rules for SURVEY §8 f1 (include/cbv_chess.h): the part of python-chess that game_state.py uses,
// restated from the rules of chess and python-chess's documented behaviour (Board.fen() with
// en_passant="legal", cleaned castling rights, king-move encoding of castling, generation order of
// legal_moves), and GameState.process_occupancy_change (game_state.py:40-195).
// The rules themselves are the plain functions of chess_core.h, which the device compiles too (k_session.hip); this file
// is their host wrapper: the C-ABI, the std::vector undo stack and the FEN text.  The generator is checked against the
// published perft numbers in tests/test_chess_rules.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cbv_chess.h"
#include "session_core.h"

namespace {

typedef uint64_t u64;
enum { PAWN = CC_PAWN, KNIGHT = CC_KNIGHT, BISHOP = CC_BISHOP, ROOK = CC_ROOK, QUEEN = CC_QUEEN, KING = CC_KING };
enum { WK = CC_WK, WQ = CC_WQ, BK = CC_BK, BQ = CC_BQ };

inline int file_of(int s) { return s & 7; }
inline int rank_of(int s) { return s >> 3; }
inline u64 bit(int s) { return 1ull << s; }
inline int msb(u64 v) { return 63 - __builtin_clzll(v); }

struct Undo {
    cbv_move m;
    int8_t captured, castling, ep;
    int halfmove;
};

} // namespace

struct cbv_board : cbv_pos { // the POD board of chess_core.h and what only the host keeps
    std::vector<Undo> stack;
};

namespace {

inline cbv_move mk(int from, int to, int promo = 0) { return cc_mk(from, to, promo); }
inline int m_from(cbv_move m) { return cc_from(m); }
inline int m_to(cbv_move m) { return cc_to(m); }
inline int m_promo(cbv_move m) { return cc_promo(m); }
inline bool is_ep_move(const cbv_pos* b, cbv_move m) { return cc_is_ep(b, m); }
inline bool capture(const cbv_pos* b, cbv_move m) { return cc_capture(b, m); }
inline int clean_castling(const cbv_pos* b) { return cc_clean_castling(b); }

void do_push(cbv_board* b, cbv_move m)
{
    Undo u;
    u.m = m;
    u.castling = (int8_t)b->castling;
    u.ep = (int8_t)b->ep;
    u.halfmove = b->halfmove;
    u.captured = (int8_t)cc_push(b, m);
    b->stack.push_back(u);
}

cbv_move do_pop(cbv_board* b)
{
    if (b->stack.empty()) return CBV_MOVE_NONE;
    const Undo u = b->stack.back();
    b->stack.pop_back();
    b->turn ^= 1;
    const int from = m_from(u.m), to = m_to(u.m), promo = m_promo(u.m);
    int piece = b->sq[to];
    const int side = piece & 8;
    if (promo) piece = PAWN | side;
    b->castling = u.castling;
    b->ep = u.ep;
    b->halfmove = u.halfmove;
    if (!b->turn) b->fullmove--;
    b->sq[from] = (int8_t)piece;
    b->sq[to] = 0;
    // restore captures / en passant / castling rook (judged on the restored position)
    const bool was_ep = (piece & 7) == PAWN && b->ep >= 0 && to == b->ep && file_of(from) != file_of(to);
    if (was_ep) b->sq[to + (side ? 8 : -8)] = u.captured;
    else b->sq[to] = u.captured;
    if ((piece & 7) == KING && abs(file_of(from) - file_of(to)) == 2) {
        const int r = rank_of(from) * 8;
        if (file_of(to) == 6) {
            b->sq[r + 7] = b->sq[r + 5];
            b->sq[r + 5] = 0;
        } else {
            b->sq[r + 0] = b->sq[r + 3];
            b->sq[r + 3] = 0;
        }
    }
    return u.m;
}

void gen_legal(const cbv_pos* b, std::vector<cbv_move>& out)
{
    cbv_movelist legal, pseudo;
    cc_gen_legal(b, &legal, &pseudo);
    out.assign(legal.m, legal.m + cc_stored(&legal));
}

bool legal(const cbv_pos* b, cbv_move m)
{
    cbv_movelist l, pseudo;
    cc_gen_legal(b, &l, &pseudo);
    return cc_has(&l, m);
}

const char* START_FEN = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1";
const char PIECE_CHARS[] = ".pnbrqk";

bool parse_fen_pos(cbv_pos* b, const char* fen)
{
    cbv_pos t;
    memset(t.sq, 0, sizeof(t.sq));
    std::vector<std::string> parts;
    {
        std::string cur;
        for (const char* p = fen; *p; p++) {
            if (*p == ' ') {
                if (!cur.empty()) parts.push_back(cur);
                cur.clear();
            } else cur.push_back(*p);
        }
        if (!cur.empty()) parts.push_back(cur);
    }
    if (parts.empty()) return false;
    int r = 7, f = 0;
    for (char c : parts[0]) {
        if (c == '/') {
            if (f != 8) return false;
            r--;
            f = 0;
        } else if (c >= '1' && c <= '8') f += c - '0';
        else {
            const char lc = (char)(c | 32);
            const char* q = strchr(PIECE_CHARS + 1, lc);
            if (!q || r < 0 || f > 7) return false;
            t.sq[r * 8 + f] = (int8_t)((int)(q - PIECE_CHARS) | ((c & 32) ? 8 : 0));
            f++;
        }
        if (f > 8 || r < 0) return false;
    }
    if (r != 0 || f != 8) return false;
    t.turn = 1;
    if (parts.size() > 1) {
        if (parts[1] == "w") t.turn = 1;
        else if (parts[1] == "b") t.turn = 0;
        else return false;
    }
    t.castling = 0;
    if (parts.size() > 2 && parts[2] != "-")
        for (char c : parts[2]) {
            if (c == 'K') t.castling |= WK;
            else if (c == 'Q') t.castling |= WQ;
            else if (c == 'k') t.castling |= BK;
            else if (c == 'q') t.castling |= BQ;
            else return false;
        }
    t.ep = -1;
    if (parts.size() > 3 && parts[3] != "-") {
        if (parts[3].size() != 2 || parts[3][0] < 'a' || parts[3][0] > 'h' || parts[3][1] < '1' || parts[3][1] > '8') return false;
        t.ep = (parts[3][1] - '1') * 8 + (parts[3][0] - 'a');
    }
    t.halfmove = parts.size() > 4 ? atoi(parts[4].c_str()) : 0;
    t.fullmove = parts.size() > 5 ? atoi(parts[5].c_str()) : 1;
    if (t.halfmove < 0) return false;
    if (t.fullmove < 1) t.fullmove = 1; // python-chess: max(fullmove, 1)
    memcpy(b->sq, t.sq, sizeof(t.sq));
    b->turn = t.turn;
    b->castling = t.castling;
    b->ep = t.ep;
    b->halfmove = t.halfmove;
    b->fullmove = t.fullmove;
    return true;
}

bool parse_fen(cbv_board* b, const char* fen)
{
    if (!parse_fen_pos(b, fen)) return false;
    b->stack.clear();
    return true;
}

bool has_legal_ep(const cbv_pos* b)
{
    if (b->ep < 0) return false;
    std::vector<cbv_move> mv;
    gen_legal(b, mv);
    for (cbv_move m : mv)
        if (is_ep_move(b, m)) return true;
    return false;
}

std::string emit_fen(const cbv_pos* b)
{
    std::string s;
    for (int r = 7; r >= 0; r--) {
        int empty = 0;
        for (int f = 0; f < 8; f++) {
            const int p = b->sq[r * 8 + f];
            if (!p) {
                empty++;
                continue;
            }
            if (empty) s.push_back((char)('0' + empty));
            empty = 0;
            const char c = PIECE_CHARS[p & 7];
            s.push_back((p & 8) ? c : (char)(c - 32));
        }
        if (empty) s.push_back((char)('0' + empty));
        if (r) s.push_back('/');
    }
    s += b->turn ? " w " : " b ";
    const int c = clean_castling(b);
    if (!c) s += "-";
    else {
        if (c & WK) s += "K";
        if (c & WQ) s += "Q";
        if (c & BK) s += "k";
        if (c & BQ) s += "q";
    }
    s += " ";
    if (has_legal_ep(b)) {
        s.push_back((char)('a' + file_of(b->ep)));
        s.push_back((char)('1' + rank_of(b->ep)));
    } else s += "-";
    char buf[48];
    snprintf(buf, sizeof(buf), " %d %d", b->halfmove, b->fullmove);
    s += buf;
    return s;
}

u64 perft(cbv_board* b, int depth)
{
    if (depth <= 0) return 1;
    std::vector<cbv_move> mv;
    gen_legal(b, mv);
    if (depth == 1) return mv.size();
    u64 n = 0;
    for (cbv_move m : mv) {
        do_push(b, m);
        n += perft(b, depth - 1);
        do_pop(b);
    }
    return n;
}

} // namespace

extern "C" {

cbv_board* cbv_board_create(void)
{
    cbv_board* b = new cbv_board();
    parse_fen(b, START_FEN);
    return b;
}
void cbv_board_destroy(cbv_board* b) { delete b; }
void cbv_board_reset(cbv_board* b)
{
    if (b) parse_fen(b, START_FEN);
}
int cbv_board_set_fen(cbv_board* b, const char* fen) { return (b && fen && parse_fen(b, fen)) ? 0 : -1; }
int cbv_board_fen(const cbv_board* b, char* out, int cap)
{
    if (!b || !out || cap <= 0) return -1;
    const std::string s = emit_fen(b);
    snprintf(out, (size_t)cap, "%s", s.c_str());
    return (int)s.size();
}
int cbv_board_turn(const cbv_board* b) { return b ? b->turn : -1; }
void cbv_board_set_turn(cbv_board* b, int white)
{
    if (b) b->turn = white ? 1 : 0;
}
int cbv_board_piece_at(const cbv_board* b, int square) { return (b && square >= 0 && square < 64) ? b->sq[square] : 0; }
uint64_t cbv_board_occupancy(const cbv_board* b) { return b ? cc_occupancy(b) : 0; }
int cbv_board_legal_moves(const cbv_board* b, cbv_move* out, int cap)
{
    if (!b) return -1;
    std::vector<cbv_move> mv;
    gen_legal(b, mv);
    for (int i = 0; i < (int)mv.size() && i < cap && out; i++) out[i] = mv[i];
    return (int)mv.size();
}
int cbv_board_is_legal(const cbv_board* b, cbv_move m) { return b && m != CBV_MOVE_NONE && legal(b, m) ? 1 : 0; }
int cbv_board_is_capture(const cbv_board* b, cbv_move m) { return b && capture(b, m) ? 1 : 0; }
int cbv_board_is_en_passant(const cbv_board* b, cbv_move m) { return b && is_ep_move(b, m) ? 1 : 0; }
int cbv_board_is_check(const cbv_board* b)
{
    if (!b) return 0;
    const int k = cc_king_square(b, b->turn);
    return k >= 0 && cc_attacked(b, k, !b->turn) ? 1 : 0;
}
int cbv_board_push(cbv_board* b, cbv_move m)
{
    if (!b || m == CBV_MOVE_NONE) return -1;
    do_push(b, m);
    return 0;
}
cbv_move cbv_board_pop(cbv_board* b) { return b ? do_pop(b) : (cbv_move)CBV_MOVE_NONE; }
int cbv_board_ply(const cbv_board* b) { return b ? (int)b->stack.size() : 0; }
cbv_move cbv_board_peek(const cbv_board* b) { return (b && !b->stack.empty()) ? b->stack.back().m : (cbv_move)CBV_MOVE_NONE; }
uint64_t cbv_board_perft(cbv_board* b, int depth) { return b ? perft(b, depth) : 0; }

static const char* kStatus[] = {"no_valid_change", "move_confirmed", "illegal_move", "castling_confirmed",
                                "en_passant_confirmed", "capture_confirmed", "ambiguous_capture"};
const char* cbv_game_status_name(int status) { return (status >= 0 && status < 7) ? kStatus[status] : ""; }

int cbv_game_process_occupancy_tones(cbv_board* b, uint64_t vision, uint64_t tone_white, uint64_t tone_black, cbv_move* move_out)
{
    if (move_out) *move_out = CBV_MOVE_NONE;
    if (!b) return CBV_GAME_NO_VALID_CHANGE;
    cbv_movelist legal, pseudo;
    cc_gen_legal(b, &legal, &pseudo);
    cbv_pos t = *b; // the core pushes on the POD board; the move goes through the undo stack here
    cbv_move m;
    const int status = cc_process_occupancy_tones(&t, &legal, vision, tone_white, tone_black, &m);
    if (m != CBV_MOVE_NONE) do_push(b, m);
    if (move_out) *move_out = m;
    return status;
}

int cbv_game_process_occupancy(cbv_board* b, uint64_t vision, cbv_move* move_out)
{
    return cbv_game_process_occupancy_tones(b, vision, 0, 0, move_out);
}

int cbv_game_infer_move_tones(const cbv_board* b, uint64_t vision, uint64_t tone_white, uint64_t tone_black, cbv_move* move_out)
{
    if (move_out) *move_out = CBV_MOVE_NONE;
    if (!b) return 0;
    cbv_movelist legal, scratch;
    cc_gen_legal(b, &legal, &scratch);
    cbv_move m;
    const int n = cc_infer_move_tones(b, &legal, &scratch, vision, tone_white, tone_black, &m);
    if (move_out) *move_out = m;
    return n;
}

int cbv_game_infer_move(const cbv_board* b, uint64_t vision, cbv_move* move_out) { return cbv_game_infer_move_tones(b, vision, 0, 0, move_out); }

uint64_t cbv_roi_bits_to_squares(uint64_t roi_bits) { return cc_flip_rows(roi_bits); }

// ---- the game session's walk on host buffers (include/cbv.h) ----

int cbv_session_state_init(cbv_session_state* st, const char* fen)
{
    if (!st) return -1;
    cbv_session_state t;
    memset(&t, 0, sizeof(t));
    if (!parse_fen_pos(ses_pos(&t), fen ? fen : START_FEN)) return -1;
    cbv_movelist legal, pseudo;
    cc_gen_legal(ses_pos(&t), &legal, &pseudo);
    ses_refresh(&t, ses_dest_squares(&legal));
    t.last_candidates = -1;
    t.ignored_move = CBV_MOVE_NONE;
    t.ignored_frame = -1;
    *st = t;
    return 0;
}

int cbv_session_state_fen(const cbv_session_state* st, char* out, int cap)
{
    if (!st || !out || cap <= 0) return -1;
    const std::string s = emit_fen(ses_pos(st));
    snprintf(out, (size_t)cap, "%s", s.c_str());
    return (int)s.size();
}

int cbv_session_walk(const cbv_session_config* cfg, cbv_session_state* st, const cbv_frame_result* results,
                     const cbv_noise_result* noise, int n, cbv_session_move* move, int* accepted)
{
    if (accepted) *accepted = 0;
    if (!cfg || !st || !results || n < 0 || !move || !accepted) return -1;
    cbv_movelist legal, scratch;
    for (int t = 0; t < n; t++) {
        const u64 vision = results[t].stable_occupied;
        if (!ses_frame_pre(cfg, st, vision, noise && noise[t].state == 1)) continue;
        cc_gen_legal(ses_pos(st), &legal, &scratch);
        if (!ses_frame_rule(cfg, st, vision, 0, 0, &legal, &scratch, move)) continue;
        cc_gen_legal(ses_pos(st), &legal, &scratch);
        ses_refresh(st, ses_dest_squares(&legal));
        *accepted = 1;
        return t + 1;
    }
    return n;
}

int cbv_session_state_init_cfg(cbv_session_state* st, const cbv_session_config* cfg, const char* fen)
{
    if (!cfg || !ses_config_ok(cfg)) return CBV_ERR_ARG;
    cbv_session_state t;
    if (cbv_session_state_init(&t, fen) != 0) return CBV_ERR_ARG;
    t.waiting_for_opponent = ses_initial_waiting(cfg, &t);
    *st = t;
    return 0;
}

// LichessSession._sync_moves' replay (lichess_session.py:99-105): reset, push_uci per token, failures skipped.  As
// python-chess's parse_uci, castling is also taken as king-takes-own-rook; "0000" (a null move) is skipped.
int cbv_session_pos_from_moves(const char* moves, cbv_session_pos* out, int* pushed)
{
    if (pushed) *pushed = 0;
    if (!out) return CBV_ERR_ARG;
    static_assert(sizeof(cbv_session_pos) == sizeof(cbv_pos), "cbv_session_pos is the POD board");
    cbv_pos b;
    if (!parse_fen_pos(&b, START_FEN)) return CBV_ERR_ARG;
    int n = 0;
    for (const char* p = moves ? moves : ""; *p;) {
        while (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r') p++;
        const char* q = p;
        while (*q && *q != ' ' && *q != '\t' && *q != '\n' && *q != '\r') q++;
        const int len = (int)(q - p);
        if ((len == 4 || len == 5) && p[0] >= 'a' && p[0] <= 'h' && p[1] >= '1' && p[1] <= '8' && p[2] >= 'a' && p[2] <= 'h' &&
            p[3] >= '1' && p[3] <= '8') {
            const int from = (p[1] - '1') * 8 + (p[0] - 'a');
            int to = (p[3] - '1') * 8 + (p[2] - 'a');
            const char* pc = len == 5 ? strchr(PIECE_CHARS + 1, p[4]) : nullptr;
            const int promo = pc ? (int)(pc - PIECE_CHARS) : 0;
            if ((b.sq[from] & 7) == KING && file_of(from) == 4 && rank_of(from) == rank_of(to) && b.sq[to] == ((b.sq[from] & 8) | ROOK))
                to = rank_of(from) * 8 + (file_of(to) == 7 ? 6 : file_of(to) == 0 ? 2 : file_of(to));
            const cbv_move m = mk(from, to, promo);
            if ((len == 4 || pc) && legal(&b, m)) {
                cc_push(&b, m);
                n++;
            }
        }
        p = q;
    }
    memcpy(out, &b, sizeof(b));
    if (pushed) *pushed = n;
    return 0;
}

int cbv_session_walk_tones(const cbv_session_config* cfg, cbv_session_state* st, const cbv_frame_result* results,
                           const cbv_noise_result* noise, int n, const cbv_session_event* events, int n_events, int* events_used,
                           cbv_session_radar* radar, const cbv_tone_result* tones, cbv_session_move* move, int* accepted)
{
    if (accepted) *accepted = 0;
    if (events_used) *events_used = 0;
    if (!cfg || !st || !results || n < 0 || !move || !accepted || n_events < 0 || (n_events && !events) || !events_used) return CBV_ERR_ARG;
    if (!ses_config_ok(cfg)) return CBV_ERR_ARG;
    const int rc = ses_events_check(st->c, st->c, 0, events, n_events);
    if (rc != CBV_OK) return rc;
    cbv_movelist legal, scratch;
    bool have_legal = false; // of the board as it stands
    int e = 0;
    for (int t = 0; t < n; t++) {
        for (; e < n_events && events[e].at_frame == st->c; e++) {
            ses_apply_event(st, &events[e]);
            cc_gen_legal(ses_pos(st), &legal, &scratch);
            have_legal = true;
            ses_refresh(st, ses_dest_squares(&legal));
        }
        *events_used = e;
        const u64 vision = results[t].stable_occupied;
        if (radar) {
            radar[t].lifted = -1;
            radar[t].destinations = 0;
            const int roi = cfg->radar ? ses_radar_lifted(st, vision) : -1;
            if (roi >= 0) {
                if (!have_legal) cc_gen_legal(ses_pos(st), &legal, &scratch);
                have_legal = true;
                radar[t].lifted = (int8_t)roi;
                radar[t].destinations = cc_flip_rows(ses_radar_dests(&legal, roi ^ 56, 0, 1));
            }
        }
        if (!ses_frame_pre(cfg, st, vision, noise && noise[t].state == 1)) continue;
        if (!have_legal) cc_gen_legal(ses_pos(st), &legal, &scratch);
        have_legal = true;
        if (!ses_frame_rule(cfg, st, vision, tones ? tones[t].white : 0ull, tones ? tones[t].black : 0ull, &legal, &scratch, move)) continue;
        cc_gen_legal(ses_pos(st), &legal, &scratch);
        ses_refresh(st, ses_dest_squares(&legal));
        *accepted = 1;
        return t + 1;
    }
    return n;
}

int cbv_session_walk_events(const cbv_session_config* cfg, cbv_session_state* st, const cbv_frame_result* results,
                            const cbv_noise_result* noise, int n, const cbv_session_event* events, int n_events, int* events_used,
                            cbv_session_radar* radar, cbv_session_move* move, int* accepted)
{
    return cbv_session_walk_tones(cfg, st, results, noise, n, events, n_events, events_used, radar, nullptr, move, accepted);
}

} // extern "C"
