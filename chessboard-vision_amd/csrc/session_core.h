// The per-frame walk of the game session (include/cbv.h, cbv_pipeline_session_begin) over cbv_session_state, compiled for
// the host (cbv_session_walk) and for the device (k_session.hip).  The walk is split around the one expensive step, the
// legal move list, so that the device can build it with the whole wave and the host with the serial generator:
//   ses_frame_pre   steps 1-5 of a frame and the two exact shortcuts: does the rule have to run?
//   ses_frame_rule  the rule on the legal moves of the board; pushes and records an accepted move
//   ses_refresh     expected occupancy and smart mask from the legal moves of the (new) board
// and for online play (LichessSession): ses_frame_rule's turn gate, ses_apply_event (the board part of _sync_moves; the
// caller follows it with ses_refresh) and ses_radar_lifted / ses_radar_dests (_update_radar_ui).
#ifndef CBV_SESSION_CORE_H
#define CBV_SESSION_CORE_H
#include "../../include/cbv.h"
#include "chess_core.h"

CBV_HD inline cbv_pos* ses_pos(cbv_session_state* st) { return (cbv_pos*)st; } // the state starts with the POD board
CBV_HD inline const cbv_pos* ses_pos(const cbv_session_state* st) { return (const cbv_pos*)st; }

// squares_to_check of the frame whose counter (after its increment) is c: bit 64 of the pair = "given"
CBV_HD inline cc_u64 ses_check_mask(const cbv_session_config* cfg, cc_u64 smart_mask, int c)
{
    return (cfg->scan_period > 0 && c % cfg->scan_period == 0) ? 0ull : smart_mask;
}

// steps 1, 3, 4, 5: returns true when the rule has to look at `vision` (ROI numbering) on this frame
CBV_HD inline bool ses_frame_pre(const cbv_session_config* cfg, cbv_session_state* st, cc_u64 vision, bool noise_active)
{
    st->c += 1;
    if (cc_popcount(st->expected ^ vision) > cfg->max_diff) { // a hand or noise: start over
        st->stable_count = 0;
        st->stable_occupancy = 0;
    } else if (st->stable_count > 0 && vision == st->stable_occupancy) {
        st->stable_count += 1;
    } else { // (with stable_count == 0 the reference's equal and unequal branches both leave this set and a count of 1)
        st->stable_occupancy = vision;
        st->stable_count = 1;
    }
    if (st->stable_count < cfg->stability_required) return false;
    if (st->last_move_c != 0 && !(st->c - st->last_move_c > cfg->cooldown_frames)) return false;
    if (noise_active) return false;
    if (vision == st->expected) return false;                       // no candidate under either rule
    if (st->rejected_valid && vision == st->rejected) return false; // rejected once: rejected until the board changes
    return true;
}

// steps 6, 7 (board part): `legal` = legal moves of the board, `scratch` a second list; tone_w / tone_b = the frame's
// cbv_tone_result (ROI numbering like `vision`), read with cfg->tone only: the rules' tie-break (include/cbv_chess.h)
CBV_HD inline bool ses_frame_rule(const cbv_session_config* cfg, cbv_session_state* st, cc_u64 vision, cc_u64 tone_w, cc_u64 tone_b,
                                  const cbv_movelist* legal, cbv_movelist* scratch, cbv_session_move* rec)
{
    cbv_pos* b = ses_pos(st);
    const cc_u64 vis_sq = cc_flip_rows(vision);
    const cc_u64 tw = cfg->tone ? cc_flip_rows(tone_w) : 0ull, tb = cfg->tone ? cc_flip_rows(tone_b) : 0ull;
    cbv_move m = CBV_MOVE_NONE;
    int status = CBV_GAME_MOVE_CONFIRMED, cand = 1;
    if (cfg->rule == CBV_SESSION_RULE_OCCUPANCY) {
        status = cc_process_occupancy_tones(b, legal, vis_sq, tw, tb, &m);
        st->last_candidates = status;
    } else {
        cand = cc_infer_move_tones(b, legal, scratch, vis_sq, tw, tb, &m);
        st->last_candidates = cand;
        if (m != CBV_MOVE_NONE && cfg->online && st->waiting_for_opponent) {
            // on_move_detected returns False (lichess_session.py:46-48): nothing is pushed and nothing restarts; the
            // occupancy is remembered so that the identical frames behind this one do not ask again
            st->ignored_move = m;
            st->ignored_frame = st->c - 1;
            st->n_ignored += 1;
            m = CBV_MOVE_NONE;
        }
        if (m != CBV_MOVE_NONE) cc_push(b, m);
    }
    if (m == CBV_MOVE_NONE) {
        st->rejected = vision;
        st->rejected_valid = 1;
        return false;
    }
    rec->frame = st->c - 1;
    rec->move = m;
    rec->status = (uint8_t)status;
    rec->candidates = (uint8_t)(cand > 255 ? 255 : cand);
    st->last_move_c = st->c;
    st->stable_count = 0;
    st->rejected_valid = 0;
    st->n_moves += 1;
    if (cfg->online) st->waiting_for_opponent = 1; // make_move is taken as sent (lichess_session.py:53-55)
    return true;
}

// expected occupancy and smart mask (ROI numbering): occupied squares, plus (file, 7 - rank) of every legal destination,
// whose ROI index 8 * (7 - (7 - rank)) + file is the destination's own square index
CBV_HD inline void ses_refresh(cbv_session_state* st, cc_u64 legal_dest_squares)
{
    st->expected = cc_flip_rows(cc_occupancy(ses_pos(st)));
    st->smart_mask = st->expected | legal_dest_squares;
}

CBV_HD inline cc_u64 ses_dest_squares(const cbv_movelist* legal)
{
    cc_u64 d = 0;
    for (int i = 0, n = cc_stored(legal); i < n; i++) d |= cc_bit(cc_to(legal->m[i]));
    return d;
}

// ---- online play ----

CBV_HD inline bool ses_config_ok(const cbv_session_config* cfg)
{
    if (cfg->online < CBV_SESSION_ONLINE_OFF || cfg->online > CBV_SESSION_ONLINE_BLACK) return false;
    if (cfg->online && cfg->rule != CBV_SESSION_RULE_INFER) return false; // LichessSession is GameSession._infer_move
    if (cfg->tone != 0 && cfg->tone != 1) return false;
    return cfg->radar == 0 || cfg->radar == 1;
}

// waiting_for_opponent at the start of a session: not is_my_turn (lichess_client.py:193-204) by the side to move
CBV_HD inline int ses_initial_waiting(const cbv_session_config* cfg, const cbv_session_state* st)
{
    if (!cfg->online) return 0;
    return (ses_pos(st)->turn != 0) == (cfg->online == CBV_SESSION_ONLINE_WHITE) ? 0 : 1;
}

// events [0, n) against a session whose next frame is `c`, `waiting` of them already queued: CBV_OK, CBV_ERR_ARG (a frame
// in the past or out of order), CBV_ERR_UNSUPPORTED (the queue is full)
CBV_HD inline int ses_events_check(int c, int last_at, int waiting, const cbv_session_event* ev, int n)
{
    for (int i = 0; i < n; i++) {
        if (ev[i].at_frame < c || ev[i].at_frame < last_at) return CBV_ERR_ARG;
        last_at = ev[i].at_frame;
    }
    return waiting + n > CBV_SESSION_EVENTS ? CBV_ERR_UNSUPPORTED : CBV_OK;
}

// _sync_moves under the lock (lichess_session.py:98-111), the board part; ses_refresh(st, destinations of the new board)
// completes it.  stable_count, stable_occupancy and last_move_c stay.
CBV_HD inline void ses_apply_event(cbv_session_state* st, const cbv_session_event* ev)
{
    cbv_pos* b = ses_pos(st);
    for (int i = 0; i < 64; i++) b->sq[i] = ev->pos.sq[i];
    b->turn = ev->pos.turn;
    b->castling = ev->pos.castling;
    b->ep = ev->pos.ep;
    b->halfmove = ev->pos.halfmove;
    b->fullmove = ev->pos.fullmove;
    st->rejected_valid = 0; // the memo belongs to the board that was
    st->waiting_for_opponent = ev->waiting_for_opponent ? 1 : 0;
}

// _update_radar_ui (game_session.py:273-285): the ROI index of the one lifted piece of the side to move, or -1
CBV_HD inline int ses_radar_lifted(const cbv_session_state* st, cc_u64 vision)
{
    const cc_u64 lifted = st->expected & ~vision;
    if (cc_popcount(lifted) != 1) return -1;
    const int roi = cc_msb(lifted);
    const int piece = ses_pos(st)->sq[roi ^ 56]; // ROI 8 * (7 - rank) + file -> square 8 * rank + file
    if (!piece || ((piece & 8) == 0) != (ses_pos(st)->turn != 0)) return -1;
    return roi;
}

// destinations (square numbering) of the moves [i0, n) step `step` of `legal` that start on `from_sq`
CBV_HD inline cc_u64 ses_radar_dests(const cbv_movelist* legal, int from_sq, int i0, int step)
{
    cc_u64 d = 0;
    for (int i = i0, n = cc_stored(legal); i < n; i += step)
        if (cc_from(legal->m[i]) == from_sq) d |= cc_bit(cc_to(legal->m[i]));
    return d;
}

#endif // CBV_SESSION_CORE_H
