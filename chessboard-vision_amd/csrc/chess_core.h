// The rules core of SURVEY §8 f1 as plain functions over a POD board, compiled for the host (chess_rules.cpp, the C-ABI
// of include/cbv_chess.h) and for the device (k_session.hip, the game session of include/cbv.h): move generation in
// python-chess's order, `attacked`, push, GameSession._infer_move (game_session.py:229-265) and
// GameState.process_occupancy_change (game_state.py:40-195).  No std::, no recursion, no allocation: move lists have a
// fixed capacity (CBV_MAX_MOVES), make/unmake is a copy of the 84-byte board.  The undo stack and the FEN text stay in
// chess_rules.cpp.
#ifndef CBV_CHESS_CORE_H
#define CBV_CHESS_CORE_H
#include <stdint.h>

#include "../../include/cbv_chess.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CBV_HD __host__ __device__
#else
#define CBV_HD
#endif

typedef uint64_t cc_u64;
enum { CC_PAWN = 1, CC_KNIGHT, CC_BISHOP, CC_ROOK, CC_QUEEN, CC_KING };
enum { CC_WK = 1, CC_WQ = 2, CC_BK = 4, CC_BQ = 8 };

struct cbv_pos {
    int8_t sq[64]; // 0 empty, type | 8 for black
    int32_t turn;  // 1 white, 0 black
    int32_t castling, ep, halfmove, fullmove;
};

struct cbv_movelist {
    int n; // moves generated; the first min(n, CBV_MAX_MOVES) are stored
    cbv_move m[CBV_MAX_MOVES];
};

CBV_HD inline void cc_add(cbv_movelist* l, cbv_move m)
{
    if (l->n < CBV_MAX_MOVES) l->m[l->n] = m;
    l->n++;
}
CBV_HD inline int cc_stored(const cbv_movelist* l) { return l->n < CBV_MAX_MOVES ? l->n : CBV_MAX_MOVES; }
CBV_HD inline bool cc_has(const cbv_movelist* l, cbv_move m)
{
    for (int i = 0, n = cc_stored(l); i < n; i++)
        if (l->m[i] == m) return true;
    return false;
}

CBV_HD inline int cc_file(int s) { return s & 7; }
CBV_HD inline int cc_rank(int s) { return s >> 3; }
CBV_HD inline cc_u64 cc_bit(int s) { return 1ull << s; }
CBV_HD inline int cc_abs(int v) { return v < 0 ? -v : v; }
CBV_HD inline int cc_msb(cc_u64 v)
{
    return 63 - __builtin_clzll(v);
}
CBV_HD inline int cc_popcount(cc_u64 v)
{
    return __builtin_popcountll(v);
}

CBV_HD inline bool cc_own(const cbv_pos* b, int p) { return p != 0 && (b->turn ? !(p & 8) : (p & 8) != 0); }
CBV_HD inline bool cc_enemy(const cbv_pos* b, int p) { return p != 0 && (b->turn ? (p & 8) != 0 : !(p & 8)); }

CBV_HD inline cbv_move cc_mk(int from, int to, int promo = 0) { return (cbv_move)(from | (to << 6) | (promo << 12)); }
CBV_HD inline int cc_from(cbv_move m) { return m & 63; }
CBV_HD inline int cc_to(cbv_move m) { return (m >> 6) & 63; }
CBV_HD inline int cc_promo(cbv_move m) { return (m >> 12) & 7; }

// the i-th step of a knight (kind 0), of a king / queen ray (kind 1: even i orthogonal, odd i diagonal)
CBV_HD inline void cc_dir(int kind, int i, int* df, int* dr)
{
    // three bits per component, biased by 2: KN = (1,2)(2,1)(2,-1)(1,-2)(-1,-2)(-2,-1)(-2,1)(-1,2), KG = (1,0)(1,1)(0,1)(-1,1)(-1,0)(-1,-1)(0,-1)(1,-1)
    const uint32_t KN_F = 3u | 4u << 3 | 4u << 6 | 3u << 9 | 1u << 12 | 0u << 15 | 0u << 18 | 1u << 21;
    const uint32_t KN_R = 4u | 3u << 3 | 1u << 6 | 0u << 9 | 0u << 12 | 1u << 15 | 3u << 18 | 4u << 21;
    const uint32_t KG_F = 3u | 3u << 3 | 2u << 6 | 1u << 9 | 1u << 12 | 1u << 15 | 2u << 18 | 3u << 21;
    const uint32_t KG_R = 2u | 3u << 3 | 3u << 6 | 3u << 9 | 2u << 12 | 1u << 15 | 1u << 18 | 1u << 21;
    *df = (int)(((kind ? KG_F : KN_F) >> (3 * i)) & 7u) - 2;
    *dr = (int)(((kind ? KG_R : KN_R) >> (3 * i)) & 7u) - 2;
}

CBV_HD inline cc_u64 cc_step_mask(int s, int kind)
{
    cc_u64 m = 0;
    for (int i = 0; i < 8; i++) {
        int df, dr;
        cc_dir(kind, i, &df, &dr);
        const int f = cc_file(s) + df, r = cc_rank(s) + dr;
        if (f >= 0 && f < 8 && r >= 0 && r < 8) m |= cc_bit(r * 8 + f);
    }
    return m;
}

// rays from s up to and including the first piece: diag = 1 the four diagonals, 0 the four orthogonals
CBV_HD inline cc_u64 cc_ray_mask(const cbv_pos* b, int s, int diag)
{
    cc_u64 m = 0;
    for (int i = diag; i < 8; i += 2) {
        int df, dr;
        cc_dir(1, i, &df, &dr);
        int f = cc_file(s) + df, r = cc_rank(s) + dr;
        while (f >= 0 && f < 8 && r >= 0 && r < 8) {
            m |= cc_bit(r * 8 + f);
            if (b->sq[r * 8 + f]) break;
            f += df;
            r += dr;
        }
    }
    return m;
}

// squares a piece of `type` on `s` attacks (pawns excluded)
CBV_HD inline cc_u64 cc_attacks_from(const cbv_pos* b, int type, int s)
{
    switch (type) {
    case CC_KNIGHT: return cc_step_mask(s, 0);
    case CC_KING: return cc_step_mask(s, 1);
    case CC_BISHOP: return cc_ray_mask(b, s, 1);
    case CC_ROOK: return cc_ray_mask(b, s, 0);
    case CC_QUEEN: return cc_ray_mask(b, s, 1) | cc_ray_mask(b, s, 0);
    }
    return 0;
}

CBV_HD inline bool cc_any_piece(const cbv_pos* b, cc_u64 m, int p1, int p2)
{
    while (m) {
        const int t = cc_msb(m);
        m &= ~cc_bit(t);
        if (b->sq[t] == p1 || b->sq[t] == p2) return true;
    }
    return false;
}

// is square s attacked by the side `white` (1) / black (0)?
CBV_HD inline bool cc_attacked(const cbv_pos* b, int s, int white)
{
    const int side = white ? 0 : 8;
    if (cc_any_piece(b, cc_step_mask(s, 0), CC_KNIGHT | side, CC_KNIGHT | side)) return true;
    if (cc_any_piece(b, cc_step_mask(s, 1), CC_KING | side, CC_KING | side)) return true;
    // a white pawn on (f +- 1, r - 1) attacks (f, r)
    const int pr = cc_rank(s) + (white ? -1 : 1);
    if (pr >= 0 && pr < 8)
        for (int df = -1; df <= 1; df += 2) {
            const int f = cc_file(s) + df;
            if (f >= 0 && f < 8 && b->sq[pr * 8 + f] == (CC_PAWN | side)) return true;
        }
    if (cc_any_piece(b, cc_ray_mask(b, s, 1), CC_BISHOP | side, CC_QUEEN | side)) return true;
    return cc_any_piece(b, cc_ray_mask(b, s, 0), CC_ROOK | side, CC_QUEEN | side);
}

CBV_HD inline int cc_king_square(const cbv_pos* b, int white)
{
    const int k = CC_KING | (white ? 0 : 8);
    for (int s = 63; s >= 0; s--)
        if (b->sq[s] == k) return s;
    return -1;
}

CBV_HD inline cc_u64 cc_occupancy(const cbv_pos* b)
{
    cc_u64 m = 0;
    for (int s = 0; s < 64; s++)
        if (b->sq[s]) m |= cc_bit(s);
    return m;
}

// castling rights whose king and rook still stand where they must (python-chess clean_castling_rights)
CBV_HD inline int cc_clean_castling(const cbv_pos* b)
{
    int c = b->castling;
    if (b->sq[4] != CC_KING) c &= ~(CC_WK | CC_WQ);
    if (b->sq[7] != CC_ROOK) c &= ~CC_WK;
    if (b->sq[0] != CC_ROOK) c &= ~CC_WQ;
    if (b->sq[60] != (CC_KING | 8)) c &= ~(CC_BK | CC_BQ);
    if (b->sq[63] != (CC_ROOK | 8)) c &= ~CC_BK;
    if (b->sq[56] != (CC_ROOK | 8)) c &= ~CC_BQ;
    return c;
}

CBV_HD inline bool cc_is_ep(const cbv_pos* b, cbv_move m)
{
    const int from = cc_from(m), to = cc_to(m);
    if (b->ep < 0 || to != b->ep) return false;
    if ((b->sq[from] & 7) != CC_PAWN) return false;
    const int d = to - from;
    if (d != 7 && d != 9 && d != -7 && d != -9) return false;
    return b->sq[to] == 0;
}

CBV_HD inline bool cc_is_castling(const cbv_pos* b, cbv_move m)
{
    const int from = cc_from(m), to = cc_to(m);
    return (b->sq[from] & 7) == CC_KING && cc_abs(cc_file(from) - cc_file(to)) == 2 && cc_rank(from) == cc_rank(to);
}

CBV_HD inline bool cc_capture(const cbv_pos* b, cbv_move m) { return cc_enemy(b, b->sq[cc_to(m)]) || cc_is_ep(b, m); }

// board.push(move), not validated; returns the captured piece (the en-passant victim included), 0 = none
CBV_HD inline int cc_push(cbv_pos* b, cbv_move m)
{
    const int from = cc_from(m), to = cc_to(m), promo = cc_promo(m);
    const int piece = b->sq[from], type = piece & 7, side = piece & 8;
    int captured = b->sq[to];
    const bool ep_cap = cc_is_ep(b, m);
    const bool castle = cc_is_castling(b, m);
    const bool zeroing = type == CC_PAWN || b->sq[to] != 0 || ep_cap;
    b->halfmove = zeroing ? 0 : b->halfmove + 1;
    if (!b->turn) b->fullmove++;
    b->ep = -1;
    if (type == CC_KING) b->castling &= side ? ~(CC_BK | CC_BQ) : ~(CC_WK | CC_WQ);
    if (from == 7 || to == 7) b->castling &= ~CC_WK;
    if (from == 0 || to == 0) b->castling &= ~CC_WQ;
    if (from == 63 || to == 63) b->castling &= ~CC_BK;
    if (from == 56 || to == 56) b->castling &= ~CC_BQ;
    b->sq[from] = 0;
    if (ep_cap) {
        const int victim = to + (side ? 8 : -8);
        captured = b->sq[victim];
        b->sq[victim] = 0;
    }
    if (type == CC_PAWN && cc_abs(to - from) == 16) b->ep = (from + to) / 2;
    b->sq[to] = (int8_t)(promo ? (promo | side) : piece);
    if (castle) {
        const int r = cc_rank(from) * 8;
        if (cc_file(to) == 6) {
            b->sq[r + 5] = b->sq[r + 7];
            b->sq[r + 7] = 0;
        } else {
            b->sq[r + 3] = b->sq[r + 0];
            b->sq[r + 0] = 0;
        }
    }
    b->turn ^= 1;
    return captured;
}

// after the side to move played m, is its own king attacked?  (m is pseudo-legal)
CBV_HD inline bool cc_king_safe(const cbv_pos* b, cbv_move m)
{
    cbv_pos t = *b;
    const int white = t.turn;
    cc_push(&t, m);
    const int k = cc_king_square(&t, white);
    return k < 0 || !cc_attacked(&t, k, !white);
}

CBV_HD inline void cc_add_pawn_move(cbv_movelist* out, int from, int to)
{
    if (cc_rank(to) == 0 || cc_rank(to) == 7) {
        cc_add(out, cc_mk(from, to, CC_QUEEN));
        cc_add(out, cc_mk(from, to, CC_ROOK));
        cc_add(out, cc_mk(from, to, CC_BISHOP));
        cc_add(out, cc_mk(from, to, CC_KNIGHT));
    } else cc_add(out, cc_mk(from, to));
}

CBV_HD inline void cc_gen_ep(const cbv_pos* b, cbv_movelist* out, cc_u64 from_mask, cc_u64 to_mask)
{
    if (b->ep < 0 || b->sq[b->ep] || !(to_mask & cc_bit(b->ep))) return;
    const int want_rank = b->turn ? 4 : 3;
    const int pr = cc_rank(b->ep) + (b->turn ? -1 : 1);
    if (pr != want_rank) return;
    for (int f = cc_file(b->ep) + 1; f >= cc_file(b->ep) - 1; f -= 2) { // scan_reversed: higher square first
        if (f < 0 || f > 7) continue;
        const int s = pr * 8 + f;
        if ((from_mask & cc_bit(s)) && b->sq[s] == (CC_PAWN | (b->turn ? 0 : 8))) cc_add(out, cc_mk(s, b->ep));
    }
}

// python-chess generate_pseudo_legal_moves(from_mask, to_mask), in its order: pieces (high square first,
// targets high first), castling (h side first), pawn captures, single pushes, double pushes, en passant
CBV_HD inline void cc_gen_pseudo(const cbv_pos* b, cbv_movelist* out, cc_u64 from_mask, cc_u64 to_mask)
{
    cc_u64 ours = 0, theirs = 0;
    for (int s = 0; s < 64; s++) {
        if (cc_own(b, b->sq[s])) ours |= cc_bit(s);
        else if (b->sq[s]) theirs |= cc_bit(s);
    }
    const int side = b->turn ? 0 : 8;
    for (int s = 63; s >= 0; s--) {
        const int p = b->sq[s];
        if (!cc_own(b, p) || (p & 7) == CC_PAWN || !(from_mask & cc_bit(s))) continue;
        cc_u64 t = cc_attacks_from(b, p & 7, s) & ~ours & to_mask;
        while (t) {
            const int to = cc_msb(t);
            t &= ~cc_bit(to);
            cc_add(out, cc_mk(s, to));
        }
    }
    // castling
    {
        const int rights = cc_clean_castling(b);
        const int r = b->turn ? 0 : 56, ks = r + 4;
        if ((from_mask & cc_bit(ks)) && b->sq[ks] == (CC_KING | side)) {
            const bool k_right = (rights & (b->turn ? CC_WK : CC_BK)) != 0, q_right = (rights & (b->turn ? CC_WQ : CC_BQ)) != 0;
            if (k_right && (to_mask & cc_bit(r + 6)) && !b->sq[r + 5] && !b->sq[r + 6] && !cc_attacked(b, ks, !b->turn) &&
                !cc_attacked(b, r + 5, !b->turn) && !cc_attacked(b, r + 6, !b->turn))
                cc_add(out, cc_mk(ks, r + 6));
            if (q_right && (to_mask & cc_bit(r + 2)) && !b->sq[r + 3] && !b->sq[r + 2] && !b->sq[r + 1] &&
                !cc_attacked(b, ks, !b->turn) && !cc_attacked(b, r + 3, !b->turn) && !cc_attacked(b, r + 2, !b->turn))
                cc_add(out, cc_mk(ks, r + 2));
        }
    }
    const int fwd = b->turn ? 8 : -8;
    // pawn captures
    for (int s = 63; s >= 0; s--) {
        if (b->sq[s] != (CC_PAWN | side) || !(from_mask & cc_bit(s))) continue;
        const int tr = cc_rank(s) + (b->turn ? 1 : -1);
        if (tr < 0 || tr > 7) continue;
        for (int f = cc_file(s) + 1; f >= cc_file(s) - 1; f -= 2) { // higher target square first
            if (f < 0 || f > 7) continue;
            const int to = tr * 8 + f;
            if ((theirs & cc_bit(to)) && (to_mask & cc_bit(to))) cc_add_pawn_move(out, s, to);
        }
    }
    // single then double pushes, by target square from high to low
    for (int to = 63; to >= 0; to--) {
        const int from = to - fwd;
        if (from < 0 || from > 63 || b->sq[to] || b->sq[from] != (CC_PAWN | side)) continue;
        if (!(from_mask & cc_bit(from)) || !(to_mask & cc_bit(to))) continue;
        cc_add_pawn_move(out, from, to);
    }
    for (int to = 63; to >= 0; to--) {
        if (cc_rank(to) != (b->turn ? 3 : 4)) continue;
        const int mid = to - fwd, from = to - 2 * fwd;
        if (b->sq[to] || b->sq[mid] || b->sq[from] != (CC_PAWN | side)) continue;
        if (!(from_mask & cc_bit(from)) || !(to_mask & cc_bit(to))) continue;
        cc_add(out, cc_mk(from, to));
    }
    cc_gen_ep(b, out, from_mask, to_mask);
}

CBV_HD inline bool cc_aligned(int df, int dr) { return df == 0 || dr == 0 || cc_abs(df) == cc_abs(dr); }

CBV_HD inline cc_u64 cc_between_mask(int a, int c)
{
    const int df = cc_file(c) - cc_file(a), dr = cc_rank(c) - cc_rank(a);
    if (!cc_aligned(df, dr)) return 0;
    const int sf = (df > 0) - (df < 0), sr = (dr > 0) - (dr < 0);
    cc_u64 m = 0;
    int f = cc_file(a) + sf, r = cc_rank(a) + sr;
    while (f != cc_file(c) || r != cc_rank(c)) {
        m |= cc_bit(r * 8 + f);
        f += sf;
        r += sr;
    }
    return m;
}

CBV_HD inline cc_u64 cc_line_mask(int a, int c) // the whole line through a and c (python-chess ray), 0 if not aligned
{
    const int df = cc_file(c) - cc_file(a), dr = cc_rank(c) - cc_rank(a);
    if (!cc_aligned(df, dr) || (df == 0 && dr == 0)) return 0;
    const int sf = (df > 0) - (df < 0), sr = (dr > 0) - (dr < 0);
    cc_u64 m = cc_bit(a);
    for (int dir = -1; dir <= 1; dir += 2) {
        int f = cc_file(a) + dir * sf, r = cc_rank(a) + dir * sr;
        while (f >= 0 && f < 8 && r >= 0 && r < 8) {
            m |= cc_bit(r * 8 + f);
            f += dir * sf;
            r += dir * sr;
        }
    }
    return m;
}

CBV_HD inline cc_u64 cc_attackers_of(const cbv_pos* b, int s, int white)
{
    cc_u64 m = 0;
    const int side = white ? 0 : 8;
    for (int t = 0; t < 64; t++) {
        const int p = b->sq[t];
        if (!p || (p & 8) != side) continue;
        const int type = p & 7;
        if (type == CC_PAWN) {
            const int tr = cc_rank(t) + (white ? 1 : -1);
            if (tr == cc_rank(s) && cc_abs(cc_file(t) - cc_file(s)) == 1) m |= cc_bit(t);
        } else if (cc_attacks_from(b, type, t) & cc_bit(s)) m |= cc_bit(t);
    }
    return m;
}

// The moves python-chess's generate_legal_moves tests for king safety, in its order: every pseudo-legal move, or in
// check _generate_evasions (king steps first, then captures / blocks of a single checker).
CBV_HD inline void cc_gen_candidates(const cbv_pos* b, cbv_movelist* pseudo)
{
    pseudo->n = 0;
    const int k = cc_king_square(b, b->turn);
    const cc_u64 checkers = k >= 0 ? cc_attackers_of(b, k, !b->turn) : 0;
    if (!checkers) {
        cc_gen_pseudo(b, pseudo, ~0ull, ~0ull);
        return;
    }
    cc_u64 sliders = 0, attacked_line = 0, ours = 0;
    for (int s = 0; s < 64; s++) {
        const int t = b->sq[s] & 7;
        if ((checkers & cc_bit(s)) && (t == CC_BISHOP || t == CC_ROOK || t == CC_QUEEN)) sliders |= cc_bit(s);
        if (cc_own(b, b->sq[s])) ours |= cc_bit(s);
    }
    while (sliders) {
        const int c = cc_msb(sliders);
        sliders &= ~cc_bit(c);
        attacked_line |= cc_line_mask(k, c) & ~cc_bit(c);
    }
    cc_u64 t = cc_step_mask(k, 1) & ~ours & ~attacked_line;
    while (t) {
        const int to = cc_msb(t);
        t &= ~cc_bit(to);
        cc_add(pseudo, cc_mk(k, to));
    }
    const int checker = cc_msb(checkers);
    if (cc_bit(checker) == checkers) {
        const cc_u64 target = cc_between_mask(k, checker) | checkers;
        cc_gen_pseudo(b, pseudo, ~cc_bit(k), target);
        if (b->ep >= 0 && !(cc_bit(b->ep) & target)) {
            const int last_double = b->ep + (b->turn ? -8 : 8);
            if (last_double == checker) cc_gen_ep(b, pseudo, ~0ull, ~0ull);
        }
    }
}

// list(board.legal_moves); `pseudo` is scratch
CBV_HD inline void cc_gen_legal(const cbv_pos* b, cbv_movelist* out, cbv_movelist* pseudo)
{
    cc_gen_candidates(b, pseudo);
    out->n = 0;
    for (int i = 0, n = cc_stored(pseudo); i < n; i++)
        if (cc_king_safe(b, pseudo->m[i])) cc_add(out, pseudo->m[i]);
}

// The tie-break by piece tones (include/cbv_chess.h): is candidate m contradicted?  Its destination looks like a piece of
// the side NOT to move.  tone_w / tone_b: square-numbered sets; a square in both or in neither is undecided.
CBV_HD inline bool cc_tone_contradicted(const cbv_pos* b, cbv_move m, cc_u64 tone_w, cc_u64 tone_b)
{
    const cc_u64 bit = cc_bit(cc_to(m));
    const cc_u64 theirs = b->turn ? tone_b & ~tone_w : tone_w & ~tone_b;
    return (theirs & bit) != 0;
}

// cbv_game_process_occupancy_tones on a POD board; `legal` = its legal moves
CBV_HD inline int cc_process_occupancy_tones(cbv_pos* b, const cbv_movelist* legal, cc_u64 vision, cc_u64 tone_w, cc_u64 tone_b, cbv_move* move_out)
{
    *move_out = CBV_MOVE_NONE;
    const cc_u64 logical = cc_occupancy(b);
    const cc_u64 vanished = logical & ~vision, appeared = vision & ~logical;
    const int nv = cc_popcount(vanished), na = cc_popcount(appeared);
    if (nv == 1 && na == 1) { // normal move, queen promotion when the plain move is not legal (game_state.py:172-195)
        const int src = cc_msb(vanished), dst = cc_msb(appeared);
        if (cc_has(legal, cc_mk(src, dst))) *move_out = cc_mk(src, dst);
        else if (cc_has(legal, cc_mk(src, dst, CC_QUEEN))) *move_out = cc_mk(src, dst, CC_QUEEN);
        else return CBV_GAME_ILLEGAL_MOVE;
        cc_push(b, *move_out);
        return CBV_GAME_MOVE_CONFIRMED;
    }
    if (nv == 2 && na == 2) { // castling: the king left, a square two files away on its rank appeared (:114-137)
        for (cc_u64 v = vanished; v;) {
            const int s = cc_msb(v);
            v &= ~cc_bit(s);
            if ((b->sq[s] & 7) != CC_KING) continue;
            for (cc_u64 a = appeared; a;) {
                const int t = cc_msb(a);
                a &= ~cc_bit(t);
                if (cc_abs(cc_file(t) - cc_file(s)) == 2 && cc_rank(t) == cc_rank(s) && cc_has(legal, cc_mk(s, t))) {
                    *move_out = cc_mk(s, t);
                    cc_push(b, *move_out);
                    return CBV_GAME_CASTLING_CONFIRMED;
                }
            }
        }
    }
    if (nv == 2 && na == 1) { // en passant: attacker and victim left, the attacker appeared (:139-160)
        const int dst = cc_msb(appeared);
        for (cc_u64 v = vanished; v;) {
            const int s = cc_msb(v);
            v &= ~cc_bit(s);
            if ((b->sq[s] & 7) != CC_PAWN) continue;
            const cbv_move m = cc_mk(s, dst);
            if (cc_has(legal, m) && cc_is_ep(b, m)) {
                *move_out = m;
                cc_push(b, m);
                return CBV_GAME_EN_PASSANT_CONFIRMED;
            }
        }
    }
    if (nv == 1 && na == 0) { // capture: the attacker left and now stands on a square that was occupied (:162-183)
        const int src = cc_msb(vanished);
        int n = 0, kept = 0; // captures; those the tones do not contradict
        cbv_move cand = CBV_MOVE_NONE, cand_kept = CBV_MOVE_NONE;
        for (int i = 0, cnt = cc_stored(legal); i < cnt; i++) {
            const cbv_move m = legal->m[i];
            if (cc_from(m) == src && cc_capture(b, m) && (vision & cc_bit(cc_to(m)))) {
                if (n == 0) cand = m;
                n++;
                if (!cc_tone_contradicted(b, m, tone_w, tone_b)) {
                    if (kept == 0) cand_kept = m;
                    kept++;
                }
            }
        }
        if (n > 1 && kept == 1) { // the tie-break: one capture left
            cand = cand_kept;
            n = 1;
        }
        if (n == 1) {
            *move_out = cand;
            cc_push(b, cand);
            return CBV_GAME_CAPTURE_CONFIRMED;
        }
        if (n > 1) return CBV_GAME_AMBIGUOUS_CAPTURE;
    }
    return CBV_GAME_NO_VALID_CHANGE;
}

// cbv_game_process_occupancy on a POD board: no tone is decided, nothing is contradicted
CBV_HD inline int cc_process_occupancy(cbv_pos* b, const cbv_movelist* legal, cc_u64 vision, cbv_move* move_out)
{
    return cc_process_occupancy_tones(b, legal, vision, 0, 0, move_out);
}

// cbv_game_infer_move_tones on a POD board; `legal` = its legal moves, `cand` is scratch.  Returns the number of distinct
// candidates (before the tie-break), *move_out is set when it is exactly one or the tie-break leaves exactly one.
CBV_HD inline int cc_infer_move_tones(const cbv_pos* b, const cbv_movelist* legal, cbv_movelist* cand, cc_u64 vision, cc_u64 tone_w, cc_u64 tone_b,
                                      cbv_move* move_out)
{
    *move_out = CBV_MOVE_NONE;
    const cc_u64 logical = cc_occupancy(b);
    const cc_u64 missing = logical & ~vision, extra = vision & ~logical;
    cand->n = 0;
    // 1. origin vanished, destination appeared (queen promotion when the plain move is not legal)   game_session.py:235-248
    for (cc_u64 o = missing; o;) {
        const int s = cc_msb(o);
        o &= ~cc_bit(s);
        for (cc_u64 e = extra; e;) {
            const int t = cc_msb(e);
            e &= ~cc_bit(t);
            cbv_move m = CBV_MOVE_NONE;
            if (cc_has(legal, cc_mk(s, t))) m = cc_mk(s, t);
            else if (cc_has(legal, cc_mk(s, t, CC_QUEEN))) m = cc_mk(s, t, CC_QUEEN);
            if (m != CBV_MOVE_NONE && !cc_has(cand, m)) cc_add(cand, m);
        }
    }
    // 2. captures from a vanished origin onto a square vision still sees occupied   game_session.py:250-257
    for (int i = 0, cnt = cc_stored(legal); i < cnt; i++) {
        const cbv_move m = legal->m[i];
        if ((missing & cc_bit(cc_from(m))) && cc_capture(b, m) && (vision & cc_bit(cc_to(m))) && !cc_has(cand, m)) cc_add(cand, m);
    }
    if (cand->n == 1) *move_out = cand->m[0];
    else if (cand->n > 1 && (tone_w | tone_b)) { // the tie-break
        int kept = 0;
        cbv_move last = CBV_MOVE_NONE;
        for (int i = 0, cnt = cc_stored(cand); i < cnt; i++)
            if (!cc_tone_contradicted(b, cand->m[i], tone_w, tone_b)) {
                last = cand->m[i];
                kept++;
            }
        if (kept == 1) *move_out = last;
    }
    return cand->n;
}

CBV_HD inline int cc_infer_move(const cbv_pos* b, const cbv_movelist* legal, cbv_movelist* cand, cc_u64 vision, cbv_move* move_out)
{
    return cc_infer_move_tones(b, legal, cand, vision, 0, 0, move_out);
}

// ROI-numbered bits (8 * row + col, row 0 = rank 8) <-> python-chess square bits: the rows swap, i.e. the bytes
CBV_HD inline cc_u64 cc_flip_rows(cc_u64 v)
{
    cc_u64 out = 0;
    for (int r = 0; r < 8; r++) out |= ((v >> (8 * r)) & 0xFFull) << (8 * (7 - r));
    return out;
}

#endif // CBV_CHESS_CORE_H
