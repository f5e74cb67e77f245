// The per-frame walk of the game session (include/cbv.h, cbv_pipeline_session_begin) over cbv_session_state, compiled for
// the host (cbv_session_walk) and for the device (k_session.hip).  The walk is split around the one expensive step, the
// legal move list, so that the device can build it with the whole wave and the host with the serial generator:
//   ses_frame_pre   steps 1-5 of a frame and the two exact shortcuts: does the rule have to run?
//   ses_frame_rule  the rule on the legal moves of the board; pushes and records an accepted move
//   ses_refresh     expected occupancy and smart mask from the legal moves of the (new) board
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

// steps 6, 7 (board part): `legal` = legal moves of the board, `scratch` a second list
CBV_HD inline bool ses_frame_rule(const cbv_session_config* cfg, cbv_session_state* st, cc_u64 vision, const cbv_movelist* legal,
                                  cbv_movelist* scratch, cbv_session_move* rec)
{
    cbv_pos* b = ses_pos(st);
    const cc_u64 vis_sq = cc_flip_rows(vision);
    cbv_move m = CBV_MOVE_NONE;
    int status = CBV_GAME_MOVE_CONFIRMED, cand = 1;
    if (cfg->rule == CBV_SESSION_RULE_OCCUPANCY) {
        status = cc_process_occupancy(b, legal, vis_sq, &m);
        st->last_candidates = status;
    } else {
        cand = cc_infer_move(b, legal, scratch, vis_sq, &m);
        st->last_candidates = cand;
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

#endif // CBV_SESSION_CORE_H
