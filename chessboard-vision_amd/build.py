"""Builds libcbv_hip.so (gfx950 only) in-tree with hipcc.

    python -m chessboard_vision_amd.build        # or __graft_entry__.build()

Each translation unit is compiled to an object in parallel, then linked.
-ffp-contract=off is part of the contract: the float stages are specified as
one rounding per operation, never fused.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libcbv_hip.so")
SOURCES = ["cbv_ctx.cpp", "cbv_api.cpp", "cbv_squares.cpp", "cbv_pipeline.cpp", "cbv_pipeline_run.cpp", "cbv_pipeline_ingest.cpp", "cbv_pipeline_sweep.cpp", "cbv_pipeline_session.cpp",
           "cbv_tables.cpp", "k_enhance.hip", "k_bilateral.hip", "k_warp.hip", "k_warp_raw_profile.hip", "k_warp_jpeg.hip", "k_analysis.hip",
           "k_squares.hip", "k_hough.hip", "k_canny.hip", "k_ingest.hip", "k_session.hip", "k_sweep.hip", "k_piece_sweep.hip", "chess_rules.cpp", "contours.cpp",
           "k_jpeg.hip", "cbv_jpeg.cpp", "cbv_pipeline_jpeg.cpp", "cbv_pipeline_frames.cpp", "k_warp_lens.hip", "k_warp_lens_profile.hip", "cbv_lens.cpp",
           "k_ingest_cs.hip", "k_warp_cs.hip", "k_warp_lens_cs.hip", "k_ingest_deep.hip", "k_warp_deep.hip", "k_warp_lens_deep.hip", "k_tone.hip", "cbv_tone.cpp"]
LONGEST = ("k_warp_deep.hip", "k_warp_lens_deep.hip")  # compiled first (build)
HEADERS = ["cbv_internal.h", "cbv_pipeline.h", "cbv_device.h", "cbv_profile_px.h", "cbv_yuv.h", "cbv_bayer.h", "cbv_bayer_deep.h", "warp_gather.h", "chess_core.h", "session_core.h", "noise_core.h", "change_blur.h", "sweep_core.h", "hough_passes.h", "piece_sweep_core.h", "jpeg_core.h", "frame_plan.h", "lens_core.h", "warp_lens.h", "tone_core.h", os.path.join("..", "..", "include", "cbv_chess.h"), os.path.join("..", "..", "include", "cbv.h")]
FLAGS = [*(["-DHG_TIMING"] if os.environ.get("HG_TIMING") else []), *(["-DBL_TWO_COPIES"] if os.environ.get("BL_TWO_COPIES") else []), *(["-DBL_NO_PAIRS"] if os.environ.get("BL_NO_PAIRS") else []), *(["-DBL_NT1024"] if os.environ.get("BL_NT1024") else []), *(["-DBL_NO_CAP"] if os.environ.get("BL_NO_CAP") else []), *(["-D" + k for k in ("BL_NO_CENTRE", "BL_ZERO_INIT", "BL_FULL_TILES") if os.environ.get(k)]), *(["-DSH_TIMING"] if os.environ.get("SH_TIMING") else []), *(["-DSW_HIST_PLAIN"] if os.environ.get("SW_HIST_PLAIN") else []), *(["-DRAW_PROFILE_FPT=%d" % int(os.environ["RAW_PROFILE_FPT"])] if os.environ.get("RAW_PROFILE_FPT") else []), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
         "-fvisibility=hidden", "-Wall", "-Wno-unused-function", "-x", "hip"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build(force=False, verbose=False):
    os.makedirs(LIBDIR, exist_ok=True)
    objdir = os.path.join(LIBDIR, "obj")
    os.makedirs(objdir, exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    jobs = []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(objdir, os.path.splitext(s)[0] + ".o")
        if force or _stale(obj, [src] + hdrs):
            jobs.append((src, obj))

    def compile_one(job):
        src, obj = job
        cmd = [_hipcc()] + FLAGS + ["-c", src, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s" % (src, r.stderr[-4000:]))
        if verbose and r.stderr:
            sys.stderr.write(r.stderr)
        return obj

    # the units that take longest start first (the link order stays SOURCES'): at the end of the queue they would run alone
    jobs.sort(key=lambda job: os.path.basename(job[0]) not in LONGEST)
    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(compile_one, jobs))
    objs = [os.path.join(objdir, os.path.splitext(s)[0] + ".o") for s in SOURCES]
    if force or jobs or _stale(LIB, objs):
        cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed:\n%s" % r.stderr[-4000:])
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
