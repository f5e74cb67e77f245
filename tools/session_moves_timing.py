"""Frames/s of the game session on the device (BoardPipeline.session_begin) at 1080p, enhance=False, device-resident
frames, 128-frame runs, against the same runs without a session (the cost of the extra rounds and history records) and
against the alternative the session replaces: one frame per run plus the host logic.  Also the time of a round that exits
at once, the time per legal-move-generator call and the cost of sessions on a four-board pipeline.  And online play
(session_begin(online=...), Session.sync_moves): the 270-frame 640x480 scene of tests/test_gpu_session.py as one run, as white
with one board event per black ply, with and without the radar, against the same run with the session offline; the time
of k_session_event (60 more events queued on the frame of one that is there anyway: no further segment), the extra scan
rounds per event (SCAN launch counter, the event kernels taken off) and the radar's time per frame.

    python tools/session_moves_timing.py [--frames 512] [--reps 5]

Prints one JSON line.  Medians over `reps` repetitions after a warm-up; the scripted game runs at 32 frames per ply."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chessboard_vision_amd import _native as N  # noqa: E402
from chessboard_vision_amd import chess_rules as chess  # noqa: E402
from chessboard_vision_amd import synth as S  # noqa: E402
from chessboard_vision_amd.game_state import GameState, StableMoveTracker, smart_scan_squares  # noqa: E402
from chessboard_vision_amd.stream import BoardPipeline  # noqa: E402

W, H, RUN = 1920, 1080, 128


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    return statistics.median(out)


def online_leg(ctx, reps):
    w, h, fpp, nfr = 640, 480, 30, 270
    q = BoardPipeline(w, h, nfr)
    q.configure(S.scaled_corners(w, h), enhance=False)
    q.synth(0, nfr, scene="normal", frames_per_ply=fpp)
    uci = ["".join(S.SCRIPT[k][0]) for k in range(8)]
    events = [(ply * fpp + 12, " ".join(uci[:ply])) for ply in (2, 4, 6, 8)]
    info = {}

    def leg(name, online, radar, extra=0):
        def once(count=False):
            q.reset_state()
            ses = q.session_begin(rule="session", cooldown_frames=10, online="white" if online else None, radar=radar)
            if online:
                for k, (at, ms) in enumerate(events):
                    for _ in range(1 + (extra if k == 0 else 0)):
                        ses.sync_moves(ms, at_frame=at)
            ctx.synchronize()
            if count:
                ctx.profile_reset()
                ctx.profile_enable(-1)
            t = time.perf_counter()
            q.run(0, nfr)
            ctx.synchronize()
            dt = time.perf_counter() - t
            if count:
                info[name] = dict(scan_launches=ctx.profile_read(N.K_ALL["SCAN"])[1], moves=len(ses.moves()), ignored=ses.state().n_ignored)
                ctx.profile_enable(-2)
                ctx.profile_reset()
            ses.end()
            return dt
        once(True)
        once()
        return statistics.median(once() for _ in range(reps))

    t_off = leg("offline", False, False)
    t_off_radar = leg("offline_radar", False, True)
    t_on = leg("online", True, False)
    t_on_radar = leg("online_radar", True, True)
    t_on_60 = leg("online_60_more_events", True, False, extra=60)
    q.close()
    ne = len(events)
    return {"online_frames": nfr, "online_events": ne, "ms_offline": t_off * 1e3, "ms_offline_radar": t_off_radar * 1e3, "ms_online": t_on * 1e3,
            "ms_online_radar": t_on_radar * 1e3, "event_kernel_us": (t_on_60 - t_on) / 60 * 1e6,
            "extra_scan_rounds_per_event": (info["online"]["scan_launches"] - ne - info["offline"]["scan_launches"]) / ne,
            "radar_us_per_frame": (t_off_radar - t_off) / nfr * 1e6, "radar_us_per_frame_online": (t_on_radar - t_on) / nfr * 1e6, "online_info": info}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n = a.frames
    ctx = N.context()
    p = BoardPipeline(W, H, n)
    p.configure(S.scaled_corners(W, H), enhance=False)
    p.synth(0, n, scene="normal", frames_per_ply=32)

    def batched():
        for s0 in range(0, n, RUN):
            p.run(s0, min(RUN, n - s0))
        ctx.synchronize()

    plain = timed(batched, a.reps)
    ses = p.session_begin(rule="game_state")
    on = timed(batched, a.reps)
    moves = len(ses.moves())
    ses.end()
    # A round that exits at once: stability and cooldown of one frame enqueue 1 + RUN rounds, and on a board that stands
    # still in the start position (vision == expected) no move is ever accepted, so every round behind the first finds
    # the run finished.  Against the same run with 1 + 1 rounds.
    q = BoardPipeline(W, H, RUN)
    q.configure(S.scaled_corners(W, H), enhance=False)
    q.synth(0, RUN, scene="normal", frames_per_ply=1 << 20)

    def scan_launches():
        ctx.profile_reset()
        ctx.profile_enable(-1)
        try:
            q.run(0, RUN)
            ctx.synchronize()
            return ctx.profile_read(N.K_ALL["SCAN"])[1]
        finally:
            ctx.profile_enable(-2)
            ctx.profile_reset()

    ses = q.session_begin(rule="game_state", stability_required=1, cooldown_frames=0)
    assert scan_launches() == 1 + RUN
    many = timed(lambda: (q.run(0, RUN), ctx.synchronize()), a.reps)
    assert ses.moves() == []
    ses.end()
    ses = q.session_begin(rule="game_state", stability_required=1 << 24, cooldown_frames=1 << 24)
    assert scan_launches() == 2
    few = timed(lambda: (q.run(0, RUN), ctx.synchronize()), a.reps)
    ses.end()
    q.close()
    idle_round_us = (many - few) / (RUN - 1) * 1e6  # 1 + 128 rounds against 1 + 1

    # four boards in the frame: with a session on any board every board's scan stage is launched by itself
    mb = BoardPipeline(W, H, n)
    pts = S.scaled_corners(W, H)
    mb.configure(pts, enhance=False)
    for k in range(3):
        mb.add_board(pts + np.float32(2 * (k + 1)))
    mb.synth(0, n, scene="normal", frames_per_ply=32)

    def mb_batched():
        for s0 in range(0, n, RUN):
            mb.run(s0, min(RUN, n - s0))
        ctx.synchronize()

    mb_plain = timed(mb_batched, a.reps)
    one = mb.session_begin(rule="game_state")
    mb_one = timed(mb_batched, a.reps)
    rest = [b.session_begin(rule="game_state") for b in mb._boards]
    mb_all = timed(mb_batched, a.reps)
    for x in [one] + rest:
        x.end()
    mb.close()

    game = GameState()
    tracker = StableMoveTracker(game, rule="game_state")
    clock = tracker.use_frame_clock()

    def per_frame():
        for t in range(n):
            p.set_check_squares(t, [None if (clock.frame + 1) % 30 == 0 else smart_scan_squares(game)])
            p.run(t, 1)
            clock.tick()
            res = p.results(t, 1)[0]
            noise = (N.NoiseResult * 1)()
            ctx.check(ctx.lib.cbv_pipeline_noise_results(p.h_, t, 1, noise))
            if tracker.process(p.occupied(res), noise_active=noise[0].state == 1) is not None:
                p.update_references(t, reset_noise=True)

    host = timed(per_frame, max(1, a.reps // 2))
    ms1, ms2 = C.c_double(), C.c_double()
    fen = b"r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1"  # 48 legal moves
    for _ in range(2):
        ctx.check(ctx.lib.cbv_session_generator_time(ctx.h, fen, 1, C.byref(ms1)))
        ctx.check(ctx.lib.cbv_session_generator_time(ctx.h, fen, 1001, C.byref(ms2)))
    chess._L()
    online = online_leg(ctx, a.reps)
    print(json.dumps({**online, "frames": n, "run": RUN, "fps_no_session": n / plain, "fps_session": n / on, "session_moves_first_pass": moves,
                      "fps_one_frame_runs_host_logic": n / host, "idle_round_us": idle_round_us,
                      "fps_4_boards_no_session": n / mb_plain, "fps_4_boards_one_session": n / mb_one, "fps_4_boards_four_sessions": n / mb_all,
                      "generator_call_us": (ms2.value - ms1.value) / 1000 * 1e3}))
    p.close()


if __name__ == "__main__":
    main()
