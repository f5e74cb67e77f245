// The device-resident pipeline's state and the helpers its translation units (cbv_pipeline*.cpp) share.  Private.
#pragma once
#include <algorithm>

#include "cbv_internal.h"

// One board of a pipeline: what configure's squares part sets up (board_setup).  Board 0 is the pipeline's own; the
// boards cbv_pipeline_add_board attaches have the same shape.
struct Board {
    cbv_pipeline_config cfg; // the pipeline's configuration with the board's subset (cbv_board_config) in it
    double Minv[9];
    u8* warped = nullptr; // [max_frames][S][S][3]
    size_t warped_stride = 0;
    std::vector<SquareDesc> descs;
    size_t plane_total = 0;
    int max_px = 0; // pixels of the largest square
    DevBuf d_descs, d_masks, d_gray, d_stats, d_ref, d_state, d_results, d_flags, d_dec, d_mean, d_var, d_noise, d_noise_state, d_hough,
        d_check, d_hough_over;
    u8* h_stage = nullptr; // pinned mirror of d_results ([max_frames] records, then the HoughCircles overflow word): written by
                           // the last kernel of a SHORT run (ResultMirror), by a copy otherwise; read by cbv_pipeline_results
    u32* over_h = nullptr; // the overflow word in h_stage
    std::vector<u8> slot_mirrored; // per slot: the mirror holds the slot's newest record (once its run has finished)
    HoughCfg hough_cfg;
    bool calibrated = false, has_check = false; // has_check: squares_to_check masks were set
    int model_mode = CBV_MODEL_FROZEN;          // cbv_pipeline_set_model_update
    double model_alpha = 0.1;
    // cbv_pipeline_set_change_blur: ChangeDetector.blur_kernel.  With 5 the ChangeDetector stage reads d_gray, the
    // PieceDetector's planes, as it always did; otherwise d_cgray holds its own planes, [max_frames][plane_total], written by
    // k_change_blur_stats.  slot_blur = the kernel each slot was last run with (0: never run).
    int change_k = 5;
    DevBuf d_cgray;
    std::vector<u8> slot_blur;
    bool own_blur() const { return change_k != 5; }
    u8* change_planes() const { return (u8*)(own_blur() ? d_cgray.p : d_gray.p); }
    // game session (cbv_pipeline_session_begin): the device state, the per-frame history records of the scan and how many
    // of the session's move records the host has handed out
    bool session = false;
    cbv_session_config ses_cfg = {};
    DevBuf d_session, d_hist;
    int ses_drained = 0;
    // online play: the board events that wait for their frame (cbv_pipeline_session_sync), the session frames enqueued so
    // far (the session frame index of the next run's first frame) and the radar records, one per slot
    std::vector<cbv_session_event> ses_events;
    int ses_frames = 0;
    DevBuf d_radar;
    bool adaptive() const { return calibrated && model_mode != CBV_MODEL_FROZEN; } // k_model_scan runs for this board
    // the board's colour profile in the profile modes (cbv_pipeline_set_profile; the pipeline's configured one until then) and
    // its device table, which exists in those modes whether the profile is enabled or not
    cbv_color_profile profile = {};
    DevBuf d_ptabs;
    // piece tones (cbv_pipeline_set_tones): the model, its device copy, and per slot the 64 tone sums and the record; the
    // buffers are made when the board first enables tones
    bool tones = false;
    cbv_tone_model tone_model = {};
    DevBuf d_tone_sums, d_tone_res, d_tone_model;
};

struct Pipe;

// The opaque handle: one board of a pipeline.  cbv_pipeline_create returns board 0, which owns the pipeline.
struct cbv_pipeline {
    Pipe* pipe;
    Board b;
};

// What the boards of a pipeline share: frames, enhancement, lanes, ingest, runs, and the boards' kernel arguments.
struct Pipe {
    cbv_ctx* ctx = nullptr;
    int w = 0, h = 0, max_frames = 0;
    Geom g;
    bool configured = false;
    bool keep_enhanced = false;
    bool skip_enhance = false; // cfg.skip_enhance: the warp samples the frames as they are, no enhancement scratch exists
    // cfg.skip_enhance == CBV_SKIP_ENHANCE_PROFILE or CBV_SKIP_ENHANCE_PROFILE_RAW: the warp samples the frames and, when a
    // board has an enabled profile (profile_on), applies each board's colour profile to its taps (WarpProfile,
    // WarpRawProfile<FMT>: warp_gather.h) from the boards' own tables, Board::d_ptabs.  profile_raw: the latter mode
    bool profile_only = false, profile_on = false, profile_raw = false;
    int chunk = 8;
    u8* frames = nullptr; // the BGR frame ring; null where plan.bgr_ring says so
    // Lanes: chunk c runs on lane c % n_lanes, each lane with its own HIP stream and scratch, so a
    // VALU-bound bilateral launch of one chunk overlaps the memory-latency-bound kernels of another.
    enum { MAX_LANES = 4 };
    int n_lanes = 1;
    hipStream_t lane_stream[MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t lane_done[MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t start_ev = nullptr;
    u8* A[MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};
    u8* B[MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};
    u8* C[MAX_LANES] = {nullptr, nullptr, nullptr, nullptr}; // third scratch frame set: region-limited enhancement only
    bool use_region = false;                                  // cfg.enhance_region, keep_enhanced == 0, a usable footprint
    PxRect region = {0, 0, 0, 0};                             // source pixels the warps sample (+ margin), clipped
    DevBuf lane_small[MAX_LANES];
    DevBuf lane_work[MAX_LANES]; // HoughCircles worklist of the lane's current chunk: count, then frame << 8 | square
    u8* enhanced = nullptr;      // [max_frames] when keep_enhanced
    DevBuf d_synth;
    // ingest: pinned host mirror of the frame ring, filled by the capture side and copied on its own stream; with a YUV or
    // Bayer input format both it and `raw_ring`, its device copy, hold raw frames, which k_ingest converts into `frames`
    // behind the copy, unless the raw ring is THE frames (plan.source == FRAMES_RAW: the warp samples it, nothing is converted).
    // Motion-JPEG: both rings hold one JPEG stream per slot and the decode writes `frames` behind the copy, or, where the
    // plane ring is the frames (FRAMES_PLANES), stops at the planes, which it writes there (cbv_pipeline_jpeg.cpp).
    // `fs` says which of these holds and `plan` what follows from it (frame_plan.h); cbv_pipeline_frames.cpp alone changes
    // either, together with the buffers below, which always match `plan`.
    FrameSettings fs;
    FramePlan plan;
    // the tables of a Bayer input format (cbv_pipeline_set_bayer_tables; include/cbv.h, "developed mosaics"): d_btab holds them,
    // bdeep says what they are (tab null: none, an 8-bit id as it always ran).  Set with the format, to its default.
    DevBuf d_btab;
    BayerDeep bdeep;
    u8* host_ring = nullptr;
    u8* raw_ring = nullptr;   // [max_frames] slots of plan.slot_bytes; both made on first use, let go by every format change
    u8* plane_ring = nullptr; // [max_frames] slots of plan.plane_slot bytes and 256 more
    struct JpegScratch {      // the scratch of one launch of a submit's decode, plan.depth frames of everything
        u32* mpos = nullptr;     // [depth * max_int]
        int16_t* coef = nullptr; // [depth][frame_elems]
        u8* planes = nullptr;    // [depth][frame_elems] with plan.own_planes
        u32 *pieces = nullptr, *segs = nullptr; // [depth][piece_words], [depth][seg_words]
    } jsc;
    struct JpegState* jpeg = nullptr; // what lives as long as the slots, from the first Motion-JPEG frame or format on
    hipStream_t copy_stream = nullptr;
    struct CopyRec {
        int s0, cnt;
        hipEvent_t ev;
        bool pending;
    };
    std::vector<CopyRec> copies;
    // The temporal scan (+ NoiseHandler) of a run goes to its own stream behind the lanes' events, so the next run's
    // enhancement of OTHER slots overlaps it; scans of successive runs stay ordered on that stream.  (Runs of one or
    // two frames keep their scan on the caller's stream, after waiting for every run in flight: see cbv_pipeline_run.)
    hipStream_t scan_stream = nullptr;
    hipEvent_t main_done = nullptr;
    // Every run that may still be executing: its slot range and two events on the (in-order) scan stream,
    // `lanes_ev` = all lanes have read the input frames and written the per-slot buffers, `scan_ev` = the scan has
    // read them.  A later run (or ingest copy) that touches overlapping slots waits on the NEWEST overlapping
    // record, which covers the older ones because the scan stream is in order.  Records are recycled once their
    // scan event has completed.
    struct RunRec {
        int s0, cnt;
        unsigned long long seq;
        hipEvent_t lanes_ev, scan_ev;
        bool live;
        bool one_event; // a run of a frame or two, all on the caller's stream: only scan_ev is recorded (an event between two
                        // kernels is a ~5 us bubble in a 150 us chain), and it stands for lanes_ev too
        DevBuf retry; // HoughCircles second-pass list of this run (HoughCfg::retry), frames numbered from the run's slot0
    };
    std::vector<RunRec> runs;
    unsigned long long run_seq = 0;    // sequence number of the newest run
    unsigned long long joined_seq = 0; // runs up to this one are ordered before later work on `joined_stream`
    hipStream_t joined_stream = nullptr;
    // the boards (board 0 = the handle cbv_pipeline_create returned) and their kernel arguments: `tab` holds one BoardDev
    // per board (board_dev), tab[0] feeds the single-board launches; d_boards is its device copy, uploaded for a single board
    // too (k_model_scan is table-driven for every number of boards), for the multi-board launches, which also take the
    // maxima and the sum over the boards below
    std::vector<cbv_pipeline*> boards;
    std::vector<BoardDev> tab;
    DevBuf d_boards;
    // the camera's lens (cbv_pipeline_set_lens), shared by every board: with it on, every warp of a board goes through
    // launch_warp_lens with d_lens_tab, one LensBoard per board (pipeline_tables), whatever the number of boards
    bool lens_on = false;
    LensDev lens = {};
    DevBuf d_lens_tab;
    const LensDev* lens_ptr() const { return lens_on ? &lens : nullptr; }
    bool any_hough = false;
    bool any_adaptive = false; // some board's model follows the frames: k_model_scan runs in front of the temporal scan
    bool any_session = false;  // some board runs a game session: the boards' scans are launched board by board
    bool any_own_blur = false; // some board's ChangeDetector has a blur kernel of its own: k_change_blur_stats runs behind the statistics
    bool any_tones = false;    // some board's tones are on: k_piece_tone runs behind the warp of every chunk
    size_t hough_lds[2] = {0, 0};
    int max_px = 0, max_S = 0;
    int n_squares = 0; // the squares that exist, the boards' n_rois summed: sizes the statistics kernels' workgroups
    Board& b0() const { return boards[0]->b; }
};
// cbv_pipeline.cpp: board handles, the ordering of the runs in flight, the boards' kernel arguments, read-backs
bool attached(const cbv_pipeline* p);
bool ranges_overlap(int a0, int an, int b0, int bn);
void retire_runs(Pipe& P);
Pipe::RunRec* newest_run(Pipe& P, int s0, int cnt, unsigned long long after);
int join_scan(Pipe& P);
int join_slots(Pipe& P, int s0, int cnt);
ChangeBlur change_blur_coef(int k);
int pipeline_tables(Pipe& P);
int board_set_profile(Pipe& P, Board& b, const cbv_color_profile* profile, const char* who);
int pipeline_update_region(Pipe& P);
int pipeline_readback(Pipe& P, void* out, const void* dev, size_t bytes);
// The pipeline whose frames the handle stands for, or null with *rc set: a null handle is CBV_ERR_ARG, with "<who>: <null_msg>"
// as the error text unless null_msg is null; a board's handle is CBV_ERR_STATE, "<who>: frames go to the parent of a board".
Pipe* frames_owner(cbv_pipeline* p, const char* who, const char* null_msg, int* rc);
// cbv_pipeline_frames.cpp: the one place where the frame store's settings and buffers change.  Makes the buffers match
// frame_plan(next) and commits `next`; on failure every setting and buffer is as it was.  drop_ingest: the call is a format
// change, which lets both ingest rings go (they come back on first use).
int pipeline_set_frames(Pipe& P, const FrameSettings& next, const char* who, bool drop_ingest);
int pipeline_host_ring(Pipe& P); // the lazy ingest rings: the pinned one (and, for a format other than BGR, the device one)
int pipeline_raw_ring(Pipe& P);
int pipeline_jpeg_ensure(Pipe& P);
void pipeline_frames_free(Pipe& P);
// cbv_pipeline_ingest.cpp
RawPlanes slot_planes(const Pipe& P, int slot);
// what the warp samples where plan.raw(), whatever the raw format
WarpSrc pipeline_raw_warp_src(const Pipe& P, int slot0, const ProfileTabs* ptabs = nullptr, int np = 1, size_t dst_profile_stride = 0);
// cbv_pipeline_jpeg.cpp: the Motion-JPEG ingest
struct JpegState {
    enum { NSETS = 16 };
    // pinned
    u32* h_lengths = nullptr;   // [max_frames], the capture side's
    JpegDesc* h_desc = nullptr; // [max_frames]
    u32* h_ioff = nullptr;      // [2 * max_frames]: the chunk that starts at slot s has its prefix sums at 2 s
    JpegTables* h_tabs = nullptr; // [NSETS] the table sets seen, by content
    int nsets = 0;
    // device
    JpegDesc* d_desc = nullptr;
    u32* d_ioff = nullptr;
    JpegTables* d_tabs = nullptr;
    int* d_status = nullptr; // [max_frames]
    int* d_nfound = nullptr; // [max_frames]
    u32* d_stats = nullptr;  // [max_frames][3]
    // the descriptors the WARP reads beside the plane ring, which change only behind the wait for the runs that read them
    // (d_desc is the decode's)
    JpegDesc* d_wdesc = nullptr; // [max_frames]
};
int pipeline_jpeg_submit(Pipe& P, int slot0, int count, hipEvent_t read_ev);
// what the warp samples on the plane ring: `slot0`'s planes and descriptor, the frames behind them
WarpSrc pipeline_jpeg_warp_src(const Pipe& P, int slot0, const ProfileTabs* ptabs = nullptr, int np = 1, size_t dst_profile_stride = 0);
// cbv_pipeline_download(which = 0) on the plane ring: k_jpeg_color of the slot into `bgr` (device, P.g)
int pipeline_jpeg_slot_bgr(Pipe& P, int slot, u8* bgr);
// cbv_jpeg.cpp: one stream through the decode kernels on ctx->stream with the context's scratch
int jpeg_single_dev(cbv_ctx* ctx, const uint8_t* data, size_t n, JpegDesc& D, const JpegTables& T, u32 S, int segments, u8* bgr_dev, Geom g,
                    JpegBatch* Bout, u8* planes_dev = nullptr, bool no_bgr = false);
