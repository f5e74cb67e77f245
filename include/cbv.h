/*
 * cbv.h — C-ABI of libcbv_hip.so: the MI355X (gfx950) implementation of the
 * per-frame digitisation path of hericmr/chessboard-vision.
 *
 * This is the drop-in boundary.  Every entry point replaces one cv2/numpy
 * call sequence of the reference (cited as reference file:line); the Python
 * classes in chessboard-vision_amd/ bind them with ctypes and mirror the
 * reference's class surface (ImageEnhancer, warp_image, ChangeDetector,
 * PieceDetector).  Plain pointers and sizes only; no torch types.
 *
 * Conventions
 *   - every function returns CBV_OK (0) or a negative CBV_ERR_* code; the
 *     message is available from cbv_last_error().
 *   - images are uint8, HWC, BGR, row stride in bytes given explicitly
 *     (numpy frames from cv2.VideoCapture; views into them are fine).
 *   - "host" entry points copy in, run the kernels, copy out and synchronise;
 *     the library keeps no host pointer after returning, and no copy from or
 *     to the caller's memory is still in flight then, with an error code as
 *     with CBV_OK (the cbv_pipeline_* ring calls document their own rules).
 *   - "dev" entry points take device pointers, enqueue on the context's
 *     stream and do not synchronise.
 *   - one cbv_ctx per GPU is the intended use.  A ctx is ONE queue of work (shared scratch buffers, one current
 *     stream): every entry point that touches the GPU holds the context's lock for its whole call, so calls from
 *     several threads on one ctx (and on the cbv_squares / cbv_pipeline objects created on it) serialise; they never
 *     run concurrently.  Use one ctx per thread for concurrency.  Host buffers passed to a call must stay valid and
 *     unmodified until it returns; the pinned host ring (cbv_pipeline_host_ring) until cbv_pipeline_wait_submitted.
 *   - there is no CPU fallback: without a usable gfx950 device
 *     cbv_ctx_create() fails with CBV_ERR_NODEV.
 */
#ifndef CBV_H
#define CBV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define CBV_API __attribute__((visibility("default")))
#else
#define CBV_API
#endif

#define CBV_OK 0
#define CBV_ERR_ARG (-1)
#define CBV_ERR_HIP (-2)
#define CBV_ERR_NODEV (-3)
#define CBV_ERR_STATE (-4)
#define CBV_ERR_UNSUPPORTED (-5)

#define CBV_MAX_SQUARES 64
#define CBV_MAX_SQUARE_DIM 128

typedef struct cbv_ctx cbv_ctx;
typedef struct cbv_squares cbv_squares;
typedef struct cbv_pipeline cbv_pipeline;

/* color_profile.json as read by ImageEnhancer.load_profile
 * (frame_enhancer.py:46-54,61-68).  enabled = 0 is the `{}` profile. */
typedef struct {
    double hue_shift, sat_scale, val_scale, contrast, brightness;
    int32_t radical_mode;
    double target_hue, hue_window;
    int32_t enabled;
} cbv_color_profile;

/* Parameters of ImageEnhancer.process_pipeline (frame_enhancer.py:28-44,161-181). */
typedef struct {
    cbv_color_profile profile;
    double clahe_clip_limit;       /* 3.0 */
    int32_t tiles_x, tiles_y;      /* (8, 8) */
    int32_t bilateral_d;           /* 9 */
    double sigma_color, sigma_space; /* 75, 75 */
    float sharpen_kernel[9];       /* [[-1,-1,-1],[-1,9,-1],[-1,-1,-1]] */
} cbv_enhance_params;

typedef struct {
    int32_t x0, y0, w, h;
} cbv_roi;

/* One square handed over by the host: a (possibly strided) view, 1 or 3 channels. */
typedef struct {
    const uint8_t* data;
    int32_t w, h, stride, cn;
} cbv_square_view;

/* Integer statistics of one preprocessed (gray + Gaussian-blurred) square.
 * Everything the host decision chains of PieceDetector.detect_piece
 * (piece_detector.py:272-345) and ChangeDetector.detect_changes_detailed
 * (change_detector.py:105-167) need. */
typedef struct {
    uint32_t n;                 /* pixels */
    uint32_t sum, sumsq;        /* sum g, sum g^2  -> np.std (piece_detector.py:305) */
    uint32_t sad_ref;           /* sum |g - ref|   -> _has_changed (piece_detector.py:90-93) */
    uint32_t center_sum, center_cnt, border_sum, border_cnt; /* piece_detector.py:177-207 */
    uint32_t ring_sum[4], ring_cnt[4];                       /* piece_detector.py:141-175 */
    uint32_t z_count;           /* #(z > z_threshold)  (change_detector.py:136-137) */
    float z_max;                /* np.max(z)           (change_detector.py:160) */
} cbv_sq_stats;

/* Synthetic scene (bench / tests only; see chessboard-vision_amd/synth.py). */
typedef struct {
    uint8_t bg_lo, bg_span;
    uint8_t light[3], dark[3], white[3], black[3];
    uint8_t noise;
    uint8_t pad[3];
    double radius;
} cbv_scene;

/* ------------------------------------------------------------------ */
/* context                                                             */
/* ------------------------------------------------------------------ */
CBV_API int cbv_device_count(void);
CBV_API int cbv_ctx_create(int device_id, cbv_ctx** out);
CBV_API void cbv_ctx_destroy(cbv_ctx* ctx);
/* ctx may be NULL: last error of a failed cbv_ctx_create / host-only call. */
CBV_API const char* cbv_last_error(const cbv_ctx* ctx);
/* Launch on a caller-owned hipStream_t (e.g. torch's current stream); NULL
 * restores the context's own stream. */
CBV_API int cbv_ctx_set_stream(cbv_ctx* ctx, void* hip_stream);
CBV_API int cbv_ctx_synchronize(cbv_ctx* ctx);
CBV_API const char* cbv_device_name(const cbv_ctx* ctx);

/* Per-kernel timing with HIP events on the launch stream.  While enabled,
 * every launch of kernel `kid` (CBV_K_*) is bracketed by an event pair;
 * cbv_profile_read synchronises and returns the accumulated time. */
enum {
    CBV_K_COLOR_LAB_HIST = 0, CBV_K_CLAHE_LUT, CBV_K_CLAHE_APPLY, CBV_K_BILATERAL, CBV_K_SHARPEN,
    CBV_K_NORM_LUT, CBV_K_NORMALIZE, CBV_K_WARP, CBV_K_SQUARES, CBV_K_GRAY_BLUR, CBV_K_OTSU,
    CBV_K_THRESHOLD, CBV_K_SCAN, CBV_K_SYNTH, CBV_K_RESET, CBV_K_HOUGH, CBV_K_INGEST, CBV_K_MODEL_SCAN, CBV_K_WARP_YUV,
    CBV_K_COUNT
};
/* The enumeration above is closed: callers size arrays by CBV_K_COUNT.  Kernels added since then take the ids behind it,
 * and CBV_K_END is one past the last id cbv_profile_read and cbv_kernel_name know. */
#define CBV_K_CHANGE_BLUR CBV_K_COUNT /* k_change_blur_stats (cbv_pipeline_set_change_blur) */
/* (CBV_K_COUNT + 1 is no kernel and has the empty name) */
#define CBV_K_INGEST_BAYER_DEEP (CBV_K_COUNT + 2) /* k_ingest_deep: developed mosaics (CBV_BAYER_*, cbv_pipeline_set_bayer_tables) to BGR */
#define CBV_K_WARP_BAYER_DEEP (CBV_K_COUNT + 3)   /* the warp kernels of a developed mosaic (raw mode) */
/* (CBV_K_COUNT + 4 is no kernel and has the empty name) */
#define CBV_K_TONE (CBV_K_COUNT + 5) /* k_piece_tone: piece colour per square (cbv_pipeline_set_tones, cbv_tone_sums_image) */
#define CBV_K_END (CBV_K_COUNT + 6)
CBV_API int cbv_profile_enable(cbv_ctx* ctx, int kid /* -1 = all, -2 = none */);
CBV_API int cbv_profile_read(cbv_ctx* ctx, int kid, double* total_ms, long long* launches);
CBV_API int cbv_profile_reset(cbv_ctx* ctx);
CBV_API const char* cbv_kernel_name(int kid);

/* ------------------------------------------------------------------ */
/* ImageEnhancer stages, host buffers (frame_enhancer.py)              */
/* ------------------------------------------------------------------ */
/* apply_color_profile, frame_enhancer.py:56-99 */
CBV_API int cbv_apply_color_profile(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride,
                            const cbv_color_profile* profile, uint8_t* out, int out_stride);
/* correct_lighting, frame_enhancer.py:101-120 */
CBV_API int cbv_correct_lighting(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, double clip_limit,
                         int tiles_x, int tiles_y, uint8_t* out, int out_stride);
/* cv2.CLAHE.apply on a single-channel 8-bit image: what `ImageEnhancer.clahe.apply(l)` does inside correct_lighting
 * (frame_enhancer.py:36,114), callable on its own because `clahe` is a public attribute of the class. */
CBV_API int cbv_clahe_apply(cbv_ctx* ctx, const uint8_t* gray, int w, int h, int stride, double clip_limit, int tiles_x,
                            int tiles_y, uint8_t* out, int out_stride);
/* reduce_noise, frame_enhancer.py:122-131 */
CBV_API int cbv_reduce_noise(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, int d, double sigma_color,
                     double sigma_space, uint8_t* out, int out_stride);
/* sharpen, frame_enhancer.py:133-138 (any 3x3 float kernel) */
CBV_API int cbv_sharpen(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, const float* kernel9, uint8_t* out,
                int out_stride);
/* normalize_intensity, frame_enhancer.py:140-146 */
CBV_API int cbv_normalize_intensity(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, uint8_t* out,
                            int out_stride);
/* prepare_analysis, frame_enhancer.py:148-159: returns unblurred gray and Otsu binary */
CBV_API int cbv_prepare_analysis(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, uint8_t* gray,
                         int gray_stride, uint8_t* binary, int binary_stride, int* otsu_threshold);
/* process_pipeline, frame_enhancer.py:161-181 */
CBV_API int cbv_process_pipeline(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride,
                         const cbv_enhance_params* params, uint8_t* out, int out_stride);

/* ------------------------------------------------------------------ */
/* warp (board_detection.py:61-71, game_session.py:124-126)            */
/* ------------------------------------------------------------------ */
/* cv2.getPerspectiveTransform: host-only, 4 (x,y) float32 pairs each. */
CBV_API int cbv_get_perspective_transform(const float* src8, const float* dst8, double* M9);
/* cv2.warpPerspective(img, M, (dw, dh)) INTER_LINEAR / BORDER_CONSTANT 0,
 * optionally followed by cv2.rotate(ROTATE_180). */
CBV_API int cbv_warp_perspective(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, const double* M9, int dw,
                         int dh, int rot180, uint8_t* out, int out_stride);

/* = cbv_apply_color_profile followed by cbv_warp_perspective (+ rotate 180), byte for byte; profile->enabled = 0 is the
 * plain warp.  One kernel (k_warp_profile): warpPerspective blends four source pixels of apply_color_profile(frame), and the
 * profile is a function of the pixel alone, so the four taps are converted and then blended; no converted frame exists.  A
 * tap outside the frame is BGR 0 (BORDER_CONSTANT), not the profile of black.  The profile's tables belong to the call. */
CBV_API int cbv_warp_color_profile(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, const cbv_color_profile* profile,
                                   const double* M9, int dw, int dh, int rot180, uint8_t* out, int out_stride);
/* ------------------------------------------------------------------ */
/* per-square detector state (change_detector.py, piece_detector.py)   */
/* ------------------------------------------------------------------ */
CBV_API int cbv_squares_create(cbv_ctx* ctx, cbv_squares** out);
CBV_API void cbv_squares_destroy(cbv_squares* sq);
/* _preprocess / _preprocess_square of n squares (change_detector.py:49-56,
 * piece_detector.py:124-135): upload the views, BGR2GRAY when cn == 3,
 * GaussianBlur((k,k),0) per square.  Defines the squares' geometry; the
 * result becomes the "current" gray of each square on the device.  A view
 * whose data is NULL keeps that square's current gray (subset updates). */
CBV_API int cbv_squares_load(cbv_squares* sq, const cbv_square_view* views, int n, int blur_k);
/* Same, reading the ROIs from a device-resident image. */
CBV_API int cbv_squares_load_dev(cbv_squares* sq, const void* dev_img, int w, int h, int stride, int cn,
                         const cbv_roi* rois, int n, int blur_k);
/* calibrate (change_detector.py:36-47): mean = gray, var = initial_variance, for selected squares */
CBV_API int cbv_squares_calibrate(cbv_squares* sq, double initial_variance, const uint8_t* select /* n flags or NULL */);
/* update_all_references EMA (change_detector.py:73-92) */
CBV_API int cbv_squares_ema(cbv_squares* sq, double alpha, const uint8_t* select);
/* reference_squares[pos] = gray.copy() (piece_detector.py:95-97) */
CBV_API int cbv_squares_set_ref(cbv_squares* sq, const uint8_t* select);
/* statistics of the current gray of every square; use_ref / use_model say
 * whether sad_ref / z_* are wanted (they need set_ref / calibrate first). */
CBV_API int cbv_squares_stats(cbv_squares* sq, int use_ref, int use_model, double z_threshold, cbv_sq_stats* out);

/* PieceDetector._detect_circle_unified (piece_detector.py:210-270): cv2.HoughCircles(gray,
 * HOUGH_GRADIENT, dp, minDist = min_dim // 3, param1, param2, minRadius = int(min_dim * min_radius_ratio),
 * maxRadius = int(min_dim * max_radius_ratio)) on every loaded square's preprocessed gray, then the
 * circle nearest to (w // 2, h // 2) within 0.3 * min_dim.  The transform is restated from the
 * published OpenCV 4.x algorithm (parity unpinned). */
typedef struct {
    double dp;                 /* 1.2  piece_detector.py:234 */
    double param1, param2;     /* 100, 25  piece_detector.py:229-230 */
    double min_radius_ratio;   /* 0.20, or piece_detector_settings.json min_radius / 100 */
    double max_radius_ratio;   /* 0.55 */
} cbv_hough_params;
#define CBV_HOUGH_KEEP 6
#define CBV_HOUGH_OVERFLOW 1 /* more than 512 accumulator maxima, the rest were dropped */
#define CBV_HOUGH_SKIPPED 2  /* pipeline only: the statistics-based detectors already decided the square */
typedef struct {
    uint8_t found;             /* _detect_circle_unified's `found` */
    uint8_t kind;              /* 1 'hough', 2 'tower_top' */
    uint16_t n_circles;        /* circles HoughCircles returned for the square */
    float cx, cy, r;           /* the chosen circle (float32, before the reference's int()) */
    int32_t votes;
    uint32_t n_edges;          /* Canny edge pixels */
    uint16_t n_centres;        /* accumulator maxima above param2 */
    uint16_t flags;            /* CBV_HOUGH_* */
    float circles[CBV_HOUGH_KEEP][4]; /* first circles in HoughCircles' order: x, y, r, support */
} cbv_hough_result;
CBV_API int cbv_squares_hough(cbv_squares* sq, const cbv_hough_params* prm, cbv_hough_result* out);
/* download / upload per-square planes (tight w*h): which = 0 gray(u8) 1 ref(u8) 2 mean(f32) 3 var(f32), and for
   cbv_squares_get alone 4 sqrt(var)(f32) as the statistics kernels read it.  Plane 4 is derived: writing plane 3
   refreshes it, and cbv_squares_set(4) returns CBV_ERR_ARG and writes nothing. */
CBV_API int cbv_squares_get(cbv_squares* sq, int which, int index, void* out);
CBV_API int cbv_squares_set(cbv_squares* sq, int which, int index, const void* in);
CBV_API int cbv_squares_geometry(cbv_squares* sq, int index, int* w, int* h);

/* ------------------------------------------------------------------ */
/* one call per frame for the reference's own call pattern              */
/* (game_session.py:124-161, calibrate_sensitivity.py:142-157):         */
/* warp_image -> split_board -> detect_all_pieces / detect_changes      */
/* ------------------------------------------------------------------ */
/* The image all squares of a split_board() dict are views of (grid_extractor.py:46,153: img_warped[y:y+h, x:x+w]). */
typedef struct {
    const uint8_t* data;
    int32_t w, h, stride, cn;
} cbv_host_image;

/* _preprocess / _preprocess_square of the n ROIs of ONE host image: the rows of the image the ROIs cover are uploaded
 * with one copy at call time (no host pointer is kept, so pixels the caller drew on the board since warp_image are
 * seen), then as cbv_squares_load_dev.  Replaces cbv_squares_load's 64 packed view copies for split_board's case. */
CBV_API int cbv_squares_load_image(cbv_squares* sq, const cbv_host_image* img, const cbv_roi* rois, int n, int blur_k);
/* reference_squares[pos] = gray.copy() (piece_detector.py:95-97) for the squares of a 64-bit set (bit i = square i);
 * asynchronous: the set rides in the launch, nothing is read from host memory afterwards. */
CBV_API int cbv_squares_set_ref_mask(cbv_squares* sq, uint64_t mask);

#define CBV_METHOD_NONE 0
#define CBV_METHOD_HOUGH 1        /* 'hough'       confidence 0.9  (piece_detector.py:310-317) */
#define CBV_METHOD_TOWER_TOP 2    /* 'tower_top'   confidence 0.75 */
#define CBV_METHOD_CENTER_DIFF 3  /* 'center_diff' confidence min(1, diff / 80) (piece_detector.py:324-331) */
#define CBV_METHOD_SYMMETRY 4     /* 'symmetry'    confidence = score (piece_detector.py:337-343) */
/* detect_piece's result dict (piece_detector.py:289-299) + detect_all_pieces' per-square gate (piece_detector.py:367-395) */
typedef struct {
    uint8_t has_piece;        /* raw result of detect_piece (before the temporal smoothing, which stays with the caller) */
    uint8_t method;           /* CBV_METHOD_* */
    uint8_t changed;          /* has_changed_visual: no reference yet, or mean |gray - reference| > change_threshold */
    uint8_t should_process;   /* piece_detector.py:381-389 */
    uint8_t evaluated;        /* should_process or not cached: the fields of detect_piece below are fresh */
    uint8_t pad[3];
    int32_t cx, cy, radius;   /* result['center'], result['radius'] when has_piece */
    double confidence;
    double center_border_diff;
} cbv_piece_result;
/* detect_piece for one square from its statistics and its HoughCircles record (NULL = HoughCircles not run); host
 * only, no GPU.  CBV_ERR_UNSUPPORTED when the record carries CBV_HOUGH_OVERFLOW. */
CBV_API int cbv_decide_piece(const cbv_sq_stats* st, const cbv_hough_result* hg, int w, int h, double circle_threshold,
                             cbv_piece_result* out);
/* np.std(gray) < 15 (piece_detector.py:305) of n contiguous pixels as numpy evaluates it in float64: 1 / 0, and np.std's
 * value in *std_out when given; host only.  It differs from the exact test on the sums that cbv_decide_piece makes only
 * where the variance is exactly 225, where rounding can leave 14.999999999999998; cbv_squares_detect_all and
 * cbv_squares_detect_changes, which hold the pixels, ask it there.
 * The numpy behaviour this restates (numpy 1.22 to 2.2, default settings; none of it is documented API):
 *  - np.std of an integer array works in float64: mean = exact sum / n, one division;
 *  - `arr - mean` and the square are two element-wise steps, each rounded once (no fused multiply-add);
 *  - np.add.reduce over a C-contiguous float64 array runs in memory order, in pieces of the ufunc buffer, 8192 elements
 *    (np.getbufsize()), each piece's sum added to the running total, which starts at 0;
 *  - within a piece, pairwise summation: below 8 elements left to right; up to 128 elements eight interleaved partial
 *    sums, combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the tail left to right; above 128 the
 *    piece is halved at a multiple of 8 and the halves' sums are added;
 *  - one division by n, one correctly rounded square root.
 * np.setbufsize, another array layout or a numpy whose reduction differs changes the last bit of np.std and with it the
 * verdict at a tie; tests/test_regions_host.py::test_np_std_below_15_is_numpy_bit_for_bit compares this function with the
 * installed numpy bit for bit and fails when that happens. */
CBV_API int cbv_np_std_below_15(const uint8_t* gray, int n, double* std_out);

typedef struct {
    double change_threshold;   /* 25   piece_detector.py:50 */
    double circle_threshold;   /* 0.6  piece_detector.py:36 */
    cbv_hough_params hough;
    uint64_t has_ref;          /* bit i: square i is in reference_squares */
    uint64_t cached;           /* bit i: square i is in cached_results */
    uint64_t check;            /* squares_to_check (piece_detector.py:348), bit i */
    int32_t check_given;       /* squares_to_check is not None */
    int32_t use_delta;
} cbv_detect_params;
/* The device half of PieceDetector.detect_all_pieces (piece_detector.py:348-440) on the n squares of one host image, in
 * ONE call with one wait: upload, _preprocess_square, _has_changed against the device-resident references, the
 * should_process gate, HoughCircles on exactly the squares the reference would run it on (evaluated squares whose std
 * is >= 15), detect_piece's decision.  History, smoothing and the reference refresh (cbv_squares_set_ref_mask) stay
 * with the caller, which owns detection_history / cached_results like the reference's class does. */
CBV_API int cbv_squares_detect_all(cbv_squares* sq, const cbv_host_image* img, const cbv_roi* rois, int n,
                                   const cbv_detect_params* prm, cbv_piece_result* out /* n */);

typedef struct {
    double z_threshold;        /* change_detector.py:23 */
    uint64_t select;           /* squares to report on: focus_squares, or all, that are in `squares` and calibrated */
    double circle_threshold;   /* of the detector's own PieceDetector (change_detector.py:33) */
    cbv_hough_params hough;
} cbv_change_params;
typedef struct {
    uint8_t in_result;         /* pct_changed >= 5: the square is in detect_changes_detailed's dict */
    uint8_t intensity;         /* 1 LEVE, 2 PARCIAL, 3 TOTAL (change_detector.py:141-148) */
    uint8_t is_circular;       /* piece_detector.detect_piece(square)['has_piece'] (change_detector.py:152-154) */
    uint8_t pad;
    float z_max;               /* np.max(z_score) */
    uint32_t z_count, n;       /* pct_changed = z_count / n * 100 */
} cbv_change_result;
/* ChangeDetector.detect_changes_detailed (change_detector.py:105-167) on the n squares of one host image in one call:
 * upload, _preprocess with the detector's blur, z-score statistics against the device-resident model, and for the
 * squares that changed the circular test on the same pixels preprocessed the PieceDetector way (k = 5). */
CBV_API int cbv_squares_detect_changes(cbv_squares* sq, const cbv_host_image* img, const cbv_roi* rois, int n, int blur_k,
                                       const cbv_change_params* prm, cbv_change_result* out /* n */);
/* tests: fill partially uploaded staging buffers (cbv_warp_perspective's frame, the squares' image rows, the raw frame of
 * cbv_yuv_to_bgr / cbv_pipeline_upload_raw) with 0xA5 before the copy, so a read outside the uploaded part cannot go
 * unnoticed */
CBV_API int cbv_debug_poison(cbv_ctx* ctx, int on);

/* cv2.Canny(img, threshold1, threshold2) with the default aperture 3 and L1 gradient, as
 * SmartGridExtractor.refine_grid (grid_extractor.py:66-121) uses it on the warped board at calibration time
 * (SURVEY §8 f3).  img: 1 or 3 channels (BGR is converted with BGR2GRAY first); edges: 0 / 255. */
CBV_API int cbv_canny(cbv_ctx* ctx, const uint8_t* img, int w, int h, int stride, int cn, double threshold1,
                      double threshold2, uint8_t* edges, int edges_stride);

/* board_detection.find_chessboard_corners (board_detection.py:4-46) up to, not including, reorder(): BGR2GRAY,
 * GaussianBlur((7,7), 1), Canny(30, 100), dilate(5x5, 3 iterations) on the GPU; findContours(RETR_EXTERNAL,
 * CHAIN_APPROX_NONE), contourArea > 100000, approxPolyDP(0.02 * arcLength) with four vertices, largest area on the
 * host.  Returns 1 and the polygon's four (x, y) vertices in pts8, 0 when no contour qualifies, negative on error.
 * dilated_out (optional) receives the dilated edge image.  Calibration-time code; parity unpinned. */
/* The host half of it alone (no GPU): external contours of a 0 / non-zero image -> the largest contour with
 * area > 100000 whose approxPolyDP(0.02 * arcLength) has four vertices.  n_contours (optional) = contours found. */
CBV_API int cbv_board_corners_from_edges(const uint8_t* edges, int w, int h, int stride, int32_t* pts8, int* n_contours);
/* Inspection helper: approxPolyDP (eps = eps_frac * arcLength) of the largest external contour; returns its vertex
 * count (the first `cap` are written), its area and its length in pixels. */
CBV_API int cbv_largest_contour_polygon(const uint8_t* edges, int w, int h, int stride, double eps_frac, int32_t* pts,
                                        int cap, double* area, int* contour_len);
CBV_API int cbv_find_chessboard_corners(cbv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, int32_t* pts8,
                                        uint8_t* dilated_out, int dilated_stride);
/* Calibration and inspection calls: the stages of cbv_find_chessboard_corners one at a time, so that each can be held to
 * its definition on its own (cbv_canny above is the third pixel stage).
 * cv2.GaussianBlur(gray, (k, k), sigma) on 8 bits: img has 1 or 3 channels (BGR is converted with BGR2GRAY first), k is
 * odd and 1..15, sigma <= 0 means cv2's sigma-from-k kernel; out is one w x h plane.  coef_out (optional, k entries)
 * receives the 8.8 fixed-point taps the kernel ran with. */
CBV_API int cbv_gaussian_blur(cbv_ctx* ctx, const uint8_t* img, int w, int h, int stride, int cn, int k, double sigma,
                              uint8_t* out, int out_stride, int32_t* coef_out);
/* Host only: those taps alone (k odd, 1..15). */
CBV_API int cbv_gaussian_q8(int k, double sigma, int32_t* coef);
/* cv2.dilate with a (2r + 1) x (2r + 1) rectangle of ones on any u8 plane, r = 0..7: the maximum over the window, pixels
 * outside the image not taking part. */
CBV_API int cbv_dilate_rect(cbv_ctx* ctx, const uint8_t* img, int w, int h, int stride, int r, uint8_t* out,
                            int out_stride);
/* Host only: cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_NONE) of a 0 / non-zero image, contours in the order cv2 lists
 * them (the last one found first).  n_contours and n_points always receive the sizes needed.  When pts_cap points and
 * contours_cap contours suffice, pts receives every contour's (x, y) points one contour after the other, lens each
 * contour's point count, areas its contourArea and perims its closed arcLength, and the call returns 0; otherwise
 * nothing is written to those four and it returns CBV_ERR_ARG.  The four may be null when their capacity is 0. */
CBV_API int cbv_external_contours(const uint8_t* img, int w, int h, int stride, int32_t* pts, int pts_cap, int32_t* lens,
                                  double* areas, double* perims, int contours_cap, int* n_contours, int* n_points);
/* Host only: cv2.approxPolyDP(curve, eps, closed=True) of n integer (x, y) points.  Returns the vertex count, or
 * CBV_ERR_ARG when it exceeds cap (nothing is written then) or an argument is bad. */
CBV_API int cbv_approx_poly_closed(const int32_t* pts, int n, double eps, int32_t* out, int cap);

/* ------------------------------------------------------------------ */
/* device-resident batched pipeline: enhance -> warp -> 64-square detect */
/* over frames that stay in HBM (bench configs C2..C5)                  */
/* ------------------------------------------------------------------ */
typedef struct {
    cbv_enhance_params enhance;
    double M[9];                 /* getPerspectiveTransform result */
    int32_t board_size;          /* 620 */
    int32_t rot180;
    int32_t n_rois;              /* 64 */
    cbv_roi rois[CBV_MAX_SQUARES];   /* index = 8*row + col of the warped image (row 0 = rank 8) */
    int32_t history_size;        /* 5   piece_detector.py:40 */
    double min_presence;         /* 0.6 piece_detector.py:41 */
    double change_threshold;     /* 25  piece_detector.py:50 */
    int32_t chunk;               /* frames per kernel launch (0 = default) */
    int32_t lanes;               /* HIP streams the chunks are spread over (0 = default 2, max 4) */
    /* ChangeDetector stage on the same squares (change_detector.py:105-167), active once
     * cbv_pipeline_calibrate() has captured the background model: */
    double z_threshold;          /* 2.5  change_detector.py:23 */
    double initial_variance;     /* 100  change_detector.py:24 */
    int32_t keep_enhanced;       /* 1: materialise process_pipeline's output per frame (cbv_pipeline_download
                                    which = 1); 0: fold the final normalize into the warp gather */
    int32_t use_hough;           /* 1: detect_piece includes HoughCircles (piece_detector.py:308-317).  has_piece is
                                    an OR of three detectors, so the transform runs only on the squares the other
                                    two left undecided; 2: run it on every non-uniform square (inspection) */
    cbv_hough_params hough;
    int32_t enhance_region;      /* 1 (only with keep_enhanced = 0): CLAHE apply, bilateral and sharpen first run on the part
                                    of each frame the warp samples (+ stencil halos); the rest of the frame is processed
                                    only for frames whose region does not already hold both a 0 and a 255 after sharpen
                                    (normalize's global min / max are then 0 / 255 whatever the rest holds).  Every
                                    output is identical to whole-frame enhancement; 0 = always the whole frame */
    int32_t skip_enhance;        /* 1: no enhancement; the warp samples the camera frame as it is, which is what
                                    GameSession.on_frame (game_session.py:123-128) and calibrate_sensitivity.py:142-146 run
                                    in front of the detectors: warp -> rotate -> split -> detect.  `enhance` is ignored;
                                    with keep_enhanced or enhance_region: CBV_ERR_ARG; cbv_pipeline_download(which = 1):
                                    CBV_ERR_STATE.  With a YUV input format the warp reads the raw frames (see
                                    cbv_pipeline_set_input_format).  0: the composed chain enhance -> warp -> detect.
                                    CBV_SKIP_ENHANCE_PROFILE (2): the colour profile only: apply_color_profile -> warp ->
                                    rotate -> split -> detect, the profile applied to the warp's taps (k_warp_profile), no
                                    enhancement scratch.  Of `enhance` only enhance.profile is read and checked; it is
                                    the profile every board starts with (cbv_pipeline_set_profile gives a board its own);
                                    keep_enhanced / enhance_region / download (which = 1) as for 1.  While no board has an
                                    enabled profile the plain warp runs.  With a YUV or Bayer input format the frames are
                                    converted into the BGR ring as with enhancement.
                                    CBV_SKIP_ENHANCE_PROFILE_RAW (3): as 2, and a YUV or Bayer input format makes the raw
                                    ring THE frames, as with 1 (raw mode, cbv_pipeline_set_input_format): the warp converts
                                    its taps and applies the profile to them (k_warp_raw_profile), no frame is converted,
                                    and while the input format is raw the pipeline holds no BGR frame ring (it is freed
                                    and allocated again as the mode and the format change).  With BGR input 3 is 2.  Every other non-zero value means 1 */
} cbv_pipeline_config;
#define CBV_SKIP_ENHANCE_PROFILE 2 /* cbv_pipeline_config::skip_enhance: the colour profile and nothing else of the enhancement */
#define CBV_SKIP_ENHANCE_PROFILE_RAW 3 /* ... and camera-native frames are sampled as they are (raw mode) */

/* Per frame result of PieceDetector.detect_all_pieces(use_smoothing=True,
 * use_delta=True, squares_to_check=None) (piece_detector.py:348-440);
 * bit i = roi i. */
typedef struct {
    uint64_t raw_occupied;     /* raw has_piece per square (cached result when not processed) */
    uint64_t stable_occupied;  /* after 5-frame smoothing = results[pos]['has_piece'] */
    uint64_t visual_changes;   /* _has_changed */
    uint64_t processed;        /* should_process */
    /* ChangeDetector.detect_changes_detailed on the same frame (zero until calibrated): */
    uint64_t changed;          /* pct_changed >= 5: the square is in the result dict */
    uint64_t parcial;          /* 15 < pct_changed <= 75 */
    uint64_t total;            /* pct_changed > 75 */
    uint64_t circular;         /* detect_piece(current square)['has_piece'], evaluated fresh */
} cbv_frame_result;

/* NoiseHandler.process (noise_handler.py:49-213) evaluated on the device for every frame from its
 * visual_changes set.  `msg` selects the shape of the reference's data dict:
 *  0 waiting            1 hand_detected {changed_count}    2 detecting (from IDLE) {squares, lifted, stable, progress}
 *  3 noise_cleared      4 clearing {cooldown, progress}     5 stabilizing (NOISE) {changed_count}
 *  6 hand_active {changed_count}   7 detecting (from NOISE) {squares, stable}   8 interrupted_by_hand {changed_count}
 *  9 move_ready {squares, stable}  10 stabilizing (PENDING) {squares, stable, progress}
 * 11 stable_ready {squares, stable, progress}  12 counting {squares, lifted, stable, progress}  13 updated {...} */
typedef struct {
    uint8_t state;    /* returned state: 0 IDLE, 1 NOISE_ACTIVE, 2 MOVE_PENDING */
    uint8_t msg;
    uint8_t stable;   /* data["stable"] */
    int8_t lifted;    /* roi index of data["lifted"], -1 = None */
    uint16_t count;   /* changed_count, cooldown or stable_count (progress = count / 5 or / 12), by msg */
    uint16_t blocked; /* is_blocked() after the frame */
    uint64_t squares; /* data["squares"] */
} cbv_noise_result;

typedef struct {
    uint32_t state, stable_count, cooldown_count;
    int32_t lifted;   /* roi index + 1 of last_lifted_square, 0 = None */
    uint64_t pending;
} cbv_noise_state;

/* Run the state machine over `n` change sets (bit i = roi i); `state` is read and updated
 * (zero-initialised = a fresh NoiseHandler).  Host buffers. */
CBV_API int cbv_noise_run(cbv_ctx* ctx, const uint64_t* changes, int n, cbv_noise_state* state, cbv_noise_result* out);

CBV_API int cbv_pipeline_create(cbv_ctx* ctx, int w, int h, int max_frames, cbv_pipeline** out);
CBV_API void cbv_pipeline_destroy(cbv_pipeline* p);
CBV_API int cbv_pipeline_configure(cbv_pipeline* p, const cbv_pipeline_config* cfg);
/* device pointer of the input frame ring: [max_frames][h][w][3] uint8 (NULL while a pipeline configured with
 * CBV_SKIP_ENHANCE_PROFILE_RAW has a YUV or Bayer input format: it holds no BGR ring) */
CBV_API void* cbv_pipeline_frames_dev(cbv_pipeline* p);
CBV_API int cbv_pipeline_upload(cbv_pipeline* p, int slot, const uint8_t* bgr, int stride);
/* Ingest front end: a pinned host mirror of the frame ring ([max_frames][h][w][3], or raw frames after
 * cbv_pipeline_set_input_format; allocated on first call) that
 * the capture / decode side writes frames into, and an asynchronous copy of slots [slot0, slot0+count) to the
 * device ring on the pipeline's copy stream.  cbv_pipeline_run of those slots waits for their copy; a submit waits
 * for every run still in flight that reads the slots it would overwrite (however many runs back).  Submitting batch k+1 before running batch k
 * overlaps PCIe with compute. */
CBV_API uint8_t* cbv_pipeline_host_ring(cbv_pipeline* p);
CBV_API int cbv_pipeline_submit(cbv_pipeline* p, int slot0, int count);
/* Block until every submitted copy has left the pinned host ring (the copy stream only: runs stay in flight).
 * After it returns the capture side may overwrite any host-ring slot again. */
CBV_API int cbv_pipeline_wait_submitted(cbv_pipeline* p);
/* fill slots with synthetic frames generated on the device */
CBV_API int cbv_pipeline_synth(cbv_pipeline* p, int slot0, int count, const uint64_t* seeds, const double* Hinv9,
                       const uint8_t* boards /* count*64 */, const cbv_scene* scene);
/* reset the temporal detector state (reference squares, cache, history) */
CBV_API int cbv_pipeline_reset_state(cbv_pipeline* p);
/* ChangeDetector.calibrate (change_detector.py:36-47) from a slot that a previous cbv_pipeline_run
 * has processed: mean = its preprocessed squares, variance = cfg.initial_variance. */
CBV_API int cbv_pipeline_calibrate(cbv_pipeline* p, int slot);
/* detect_all_pieces' `squares_to_check` (piece_detector.py:348,381-389; game_session.py:130-152): per frame a set of
 * squares (bit = roi) that are processed even when unchanged and cached.  NULL clears the slots' sets (= None).  The
 * masks stay with the slots until changed. */
CBV_API int cbv_pipeline_set_check_squares(cbv_pipeline* p, int slot0, int count, const uint64_t* roi_masks);
/* What the session does after it accepted a move (game_session.py:219-223): PieceDetector.update_references with the
 * squares of an already processed slot (reference = that frame, cached results cleared, history kept) and, when
 * reset_noise, NoiseHandler.reset(). */
CBV_API int cbv_pipeline_update_references(cbv_pipeline* p, int slot, int reset_noise);
/* enqueue enhance -> warp -> detect for frames [slot0, slot0+count) in stream order; asynchronous */
CBV_API int cbv_pipeline_run(cbv_pipeline* p, int slot0, int count);
/* CBV_ERR_UNSUPPORTED (with `out` filled) when a HoughCircles candidate list overflowed even the second pass in a run
 * since the previous call: the counter is cleared on read, so later frames are not affected; cbv_pipeline_hough's flags
 * name the squares. */
CBV_API int cbv_pipeline_results(cbv_pipeline* p, int slot0, int count, cbv_frame_result* out);
/* NoiseHandler outputs of the same frames (fed by their visual_changes, like game_session.py:165) */
CBV_API int cbv_pipeline_noise_results(cbv_pipeline* p, int slot0, int count, cbv_noise_result* out);
/* download intermediates of one slot for parity checks: which = 0 input, 1 enhanced, 2 warped */
CBV_API int cbv_pipeline_download(cbv_pipeline* p, int which, int slot, uint8_t* out);
CBV_API int cbv_pipeline_square_stats(cbv_pipeline* p, int slot, cbv_sq_stats* out /* n_rois */);
/* HoughCircles outcome of one processed slot (cfg.use_hough): CBV_MAX_SQUARES entries, index = roi */
CBV_API int cbv_pipeline_hough(cbv_pipeline* p, int slot, cbv_hough_result* out);

/* ------------------------------------------------------------------ */
/* camera-native frames (NV12, NV21, yuv420p, YV12, YUYV, YVYU, UYVY, Bayer mosaics of 8 to 16 bits), converted to BGR on the device */
/* ------------------------------------------------------------------ */
/* Cameras deliver YUYV / UYVY / YVYU, hardware decoders NV12 / NV21 and software decoders yuv420p / YV12;
 * cv2.VideoCapture converts them to BGR on a host core before the application sees a frame.  Here the raw frame crosses
 * PCIe (2 or 1.5 bytes per pixel instead of 3) and one kernel writes BGR into the pipeline's frame ring, so everything
 * downstream is unchanged.  The conversion is cv2.cvtColor's COLOR_YUV2BGR_NV12 / _NV21 / _I420 / _YV12 / _YUY2 / _YVYU /
 * _UYVY on 8-bit data: BT.601, limited range, fixed point with 20 fraction bits, no chroma interpolation (a pixel takes
 * the U, V of its 2x2 block or of its horizontal pair).  With
 * y = max(0, Y - 16) * 1220542, u = U - 128, v = V - 128, h = 1 << 19, in signed 32-bit arithmetic:
 *     B = sat_u8((y + h + 2116026 * u) >> 20)
 *     G = sat_u8((y + h -  852492 * v - 409993 * u) >> 20)
 *     R = sat_u8((y + h + 1673527 * v) >> 20)
 * Only where the bytes lie differs between the layouts.
 * 4:2:0 (w and h even), plane0 = h rows of w luma bytes, then
 *     NV12:    plane1 = h / 2 rows of w bytes U V U V ...
 *     NV21:    plane1 = h / 2 rows of w bytes V U V U ...
 *     YUV420P: plane1 = U, h / 2 rows of w / 2 bytes; plane2 = V, the same shape   (I420 / IYUV)
 *     YV12:    as YUV420P with V in plane1 and U in plane2
 * packed 4:2:2 (w even), plane0 = h rows of 2 w bytes
 *     YUYV (YUY2): Y0 U Y1 V      YVYU: Y0 V Y1 U      UYVY: U Y0 V Y1
 * The ids are bit fields: the low nibble is the family (1 = 4:2:0, 2 = packed 4:2:2), 0x10 = V comes before U, 0x20 =
 * planar chroma (4:2:0) or chroma-first bytes (4:2:2).  Every id not listed here is refused. */
#define CBV_FMT_BGR     0
#define CBV_FMT_NV12    1
#define CBV_FMT_YUYV    2
#define CBV_FMT_NV21    0x11
#define CBV_FMT_YUV420P 0x21
#define CBV_FMT_YV12    0x31
#define CBV_FMT_YVYU    0x12
#define CBV_FMT_UYVY    0x22

/* The colour space of a YUV frame travels in its format id: CBV_CS_* bits OR-ed onto any of the seven YUV ids above, wherever
 * a raw format id is taken (cbv_raw_frame::fmt of cbv_yuv_to_bgr, cbv_warp_color_profile_raw, cbv_warp_lens and
 * cbv_pipeline_upload_raw; cbv_pipeline_set_input_format).  No bits = the arithmetic above, which is what most UVC webcams'
 * YUYV needs.  The other three replace its constants and nothing else:
 *     yy = max(0, Y - yoff) * CY, u = U - 128, v = V - 128, h = 1 << 19
 *     B = clamp(yy + h + CUB * u, 0, (256 << 20) - 1) >> 20
 *     G = clamp(yy + h + CVG * v + CUG * u, 0, (256 << 20) - 1) >> 20
 *     R = clamp(yy + h + CVR * v, 0, (256 << 20) - 1) >> 20
 *     bits                         matrix, range        yoff  CY       CUB      CUG      CVG      CVR
 *     0                            BT.601 (cv2), limited  16  1220542  2116026  -409993  -852492  1673527
 *     CBV_CS_FULL                  BT.601 (JFIF), full     0  1048576  1858077  -360853  -748826  1470104
 *     CBV_CS_BT709                 BT.709, limited        16  1220945  2215014  -223607  -558796  1879825
 *     CBV_CS_BT709 | CBV_CS_FULL   BT.709, full            0  1048576  1945738  -196424  -490864  1651297
 * The last three rows are round(c * 2^20) of the exact coefficients (Kr, Kb = 0.299, 0.114 / 0.2126, 0.0722; luma scale
 * 255 / 219 and chroma scale 255 / 224 for limited range, 1 for full).  Every sum stays inside signed 32 bits.  Chroma siting
 * and upsampling are unchanged.  Decoded video at 720p and above is BT.709 limited; phone cameras and JFIF-like sources are
 * BT.601 full.  Colour-space bits on CBV_FMT_BGR, a Bayer id or CBV_FMT_MJPEG (JFIF by definition) are CBV_ERR_ARG.  A
 * pipeline in raw mode compares the whole id: an NV12 / BT.709 ring refuses an NV12 / BT.601 frame.  (The bits lie above
 * 0x3FF: ids such as 0x121 and 0x104 were always refused as unassigned, and stay so.) */
#define CBV_CS_FULL  0x400
#define CBV_CS_BT709 0x800
#define CBV_CS_MASK  0xC00

/* 8-bit Bayer mosaics (machine-vision cameras, the raw mode of most sensors): one plane of h rows of w bytes, one byte and
 * one colour per pixel, a third of BGR's bytes.  The conversion is the bilinear demosaic of
 * cv2.cvtColor(raw, COLOR_Bayer??2BGR) on 8-bit data (not the _VNG or _EA variants).  White balance, black and white level and
 * a tone curve are per-colour tables in front of it ("developed mosaics" below); no colour matrix is applied.  A layout is named by its top-left 2 x 2 block, read row by row.  OpenCV names its codes by the block
 * at (1, 1) instead, so the code of a layout carries the OTHER pair of letters:
 *     id                        rows 0 / 1     cv2 code                                     libav / V4L2
 *     CBV_FMT_BAYER_RGGB 0x04   R G / G B      COLOR_BayerBG2BGR (= COLOR_BayerRGGB2BGR)    bayer_rggb8 / SRGGB8
 *     CBV_FMT_BAYER_BGGR 0x14   B G / G R      COLOR_BayerRG2BGR (= COLOR_BayerBGGR2BGR)    bayer_bggr8 / SBGGR8
 *     CBV_FMT_BAYER_GRBG 0x24   G R / B G      COLOR_BayerGB2BGR (= COLOR_BayerGRBG2BGR)    bayer_grbg8 / SGRBG8
 *     CBV_FMT_BAYER_GBRG 0x34   G B / R G      COLOR_BayerGR2BGR (= COLOR_BayerGBRG2BGR)    bayer_gbrg8 / SGBRG8
 * The ids are bit fields like those above: the low nibble 4 is the family, 0x10 = blue sits where RGGB has red, 0x20 = the
 * row starts with green.  Site (x, y) carries the colour of (x & 1, y & 1) in the 2 x 2 block; p(x, y) is the raw byte.
 * Interior (1 <= x <= w - 2, 1 <= y <= h - 2), value D(x, y):
 *   a red or blue site, own colour C:
 *     C = p(x, y)
 *     G = (p(x-1,y) + p(x+1,y) + p(x,y-1) + p(x,y+1) + 2) >> 2
 *     the other of red / blue = (p(x-1,y-1) + p(x+1,y-1) + p(x-1,y+1) + p(x+1,y+1) + 2) >> 2
 *   a green site:
 *     G = p(x, y)
 *     the colour whose samples lie in this row              = (p(x-1,y) + p(x+1,y) + 1) >> 1
 *     the colour whose samples lie in the rows above, below = (p(x,y-1) + p(x,y+1) + 1) >> 1
 * which is "each missing colour is the mean of the nearest samples of that colour, rounded half up".
 * Frame edge: the outermost rows and columns copy their neighbours' results,
 *     out(x, y) = D(clamp(x, 1, w - 2), clamp(y, 1, h - 2)),
 * as OpenCV fills them (the left and right pixel of each row from columns 1 and w - 2, then the first and last row from
 * rows 1 and h - 2).  w and h must be even and at least 4: otherwise CBV_ERR_ARG, and nothing has changed.
 * Like the YUV conversion above this is restated from the published algorithm and is not pinned
 * against a cv2 build. */
#define CBV_FMT_BAYER_RGGB 0x04
#define CBV_FMT_BAYER_BGGR 0x14
#define CBV_FMT_BAYER_GRBG 0x24
#define CBV_FMT_BAYER_GBRG 0x34

/* Developed mosaics: sample encodings of more than 8 bits, and per-colour tables in front of the demosaic.
 * A developed mosaic is  m8(x, y) = T[c(x, y)][min(s(x, y), 2^bits - 1)]:  s is the raw sample at site (x, y), c the colour
 * the site carries in the layout (above), as the BGR channel index (0 blue, 1 green, 2 red), and T three tables of 2^bits
 * bytes in B, G, R order.  The clamp on the index is part of the definition: a 16-bit container may hold anything, and no
 * table is ever read outside.  The BGR frame is the 8-bit demosaic above of m8, edge rule included; nothing else is new
 * arithmetic.  Black level, white level, white-balance gains and a tone curve are all functions of one sample of one
 * colour, so they are all one table (the caller builds it; the library evaluates no power function).
 * The sample encoding is a field of the format id, CBV_BAYER_* OR-ed onto one of the four layouts above; row B of the mosaic:
 *     field            row bytes  sample x                                                       bits         V4L2 / libav
 *     0 (the ids above) w         B[x]                                                           8            SRGGB8 / bayer_rggb8
 *     CBV_BAYER_16      2 w       B[2x] | B[2x+1] << 8            (little-endian container)      10 12 14 16  SRGGB10, 12, 14, 16 / bayer_rggb16le
 *     CBV_BAYER_10P     5 w / 4   g = x >> 2, i = x & 3: B[5g+i] << 2 | (B[5g+4] >> 2i) & 3      10           SRGGB10P (MIPI RAW10), w % 4 == 0
 *     CBV_BAYER_12P     3 w / 2   g = x >> 1: even B[3g] << 4 | B[3g+2] & 15,                    12           SRGGB12P (MIPI RAW12)
 *                                             odd  B[3g+1] << 4 | B[3g+2] >> 4
 * w and h are even and at least 4 as above, CBV_BAYER_10P also needs w % 4 == 0, and a row stride is at least the row
 * bytes (V4L2's bytesperline padding is a stride).  Every other value of the field, and colour-space bits on any Bayer
 * id, are CBV_ERR_ARG.  (GenICam's LSB-first 10p / 12p packings are not these: such cameras go through the 16-bit container.)
 * The NEUTRAL table of `bits` bits is T[c][v] = (510 v + M) / (2 M) in integer division with M = 2^bits - 1: v 255 / M
 * rounded half up.  It is the default of the three encodings above (bits 10 for 10P, 12 for 12P, 16 for the container: a
 * 16-bit table also covers MSB-aligned data).  The 8-bit ids have NO table by default and then run the kernels they always
 * ran; a table given for them (bits 8) makes them developed mosaics too.
 * Where ids are taken: cbv_raw_frame::fmt of cbv_yuv_to_bgr (the default table), cbv_bayer_to_bgr and cbv_pipeline_upload_raw,
 * and cbv_pipeline_set_input_format.  The single-frame raw warps (cbv_warp_color_profile_raw, cbv_warp_lens with a raw
 * frame) refuse the three encodings with CBV_ERR_ARG and have no tables: a pipeline warps from developed mosaics. */
#define CBV_BAYER_16       0x1000
#define CBV_BAYER_10P      0x2000
#define CBV_BAYER_12P      0x3000
#define CBV_BAYER_ENC_MASK 0xF000

/* One raw frame in host memory.  stride2 and plane2 are read only for the three-plane formats (YUV420P, YV12): stride2
 * lies in what was padding and plane2 behind what was the end of the struct, so a caller built against the 32-byte struct
 * of the two-plane formats keeps working. */
typedef struct {
    int32_t fmt;            /* CBV_FMT_* */
    int32_t stride0, stride1;   /* bytes per row of plane0 / plane1 */
    int32_t stride2;        /* bytes per row of plane2 */
    const uint8_t* plane0;  /* BGR, the packed 4:2:2 bytes, the Bayer mosaic, or the luma plane */
    const uint8_t* plane1;  /* NV12 / NV21 chroma plane, YUV420P's U or YV12's V plane, else NULL */
    const uint8_t* plane2;  /* YUV420P's V or YV12's U plane */
} cbv_raw_frame;

/* host in, host out: the cvtColor call on its own (fmt = any CBV_FMT_* but BGR, the Bayer mosaics included; a
 * CBV_BAYER_* encoding is developed with its default table) */
CBV_API int cbv_yuv_to_bgr(cbv_ctx* ctx, const cbv_raw_frame* raw, int w, int h, uint8_t* bgr, int bgr_stride);
/* host in, host out: one developed mosaic to BGR.  raw->fmt is a Bayer id of any encoding; tables = [3][1 << bits] bytes,
 * B G R, or NULL for the format's default (bits is then ignored; an 8-bit id: no table, cbv_yuv_to_bgr's result).
 * CBV_ERR_ARG: not a Bayer id, a size or stride the format refuses, bits that do not go with the encoding. */
CBV_API int cbv_bayer_to_bgr(cbv_ctx* ctx, const cbv_raw_frame* raw, int w, int h, const uint8_t* tables, int bits, uint8_t* bgr, int bgr_stride);
/* cbv_warp_color_profile on one camera-native frame (any CBV_FMT_* but BGR): = cbv_yuv_to_bgr, then
 * cbv_apply_color_profile, then cbv_warp_perspective (+ rotate 180), byte for byte, in one kernel (k_warp_raw_profile):
 * the four taps are converted (YUV) or demosaiced (Bayer), the profile is applied to each tap inside the frame, and they
 * are blended; neither the BGR frame nor the profiled frame exists.  A tap outside the frame is BGR 0.  profile->enabled
 * = 0 is the plain raw warp (k_warp_yuv, k_warp_bayer).  Host in, host out.  CBV_ERR_ARG, with `out` untouched: null
 * arguments, BGR or an unknown format, odd w, odd h with a 4:2:0 or Bayer format, a Bayer frame below 4 x 4, a missing
 * plane or a stride below its row, a profile field that is not finite. */
CBV_API int cbv_warp_color_profile_raw(cbv_ctx* ctx, const cbv_raw_frame* raw, int w, int h, const cbv_color_profile* profile,
                                       const double* M9, int dw, int dh, int rot180, uint8_t* out, int out_stride);
/* one frame of any format into a slot of the frame ring, synchronous, like cbv_pipeline_upload */
CBV_API int cbv_pipeline_upload_raw(cbv_pipeline* p, int slot, const cbv_raw_frame* raw);
/* Format of the pinned ingest ring; CBV_FMT_BGR is the default.  Waits for the submitted copies, then FREES the pinned
 * ring: a pointer cbv_pipeline_host_ring returned earlier is dead after this call, and the next cbv_pipeline_host_ring
 * allocates the ring in the new format ([max_frames] raw frames, tightly packed in the layout above, each slot rounded
 * to 256 bytes: cbv_pipeline_host_slot_bytes).  With a YUV format cbv_pipeline_submit copies the raw slots to a device
 * ring of the same layout and converts them into the BGR frame ring behind the copy; its ordering promises are the
 * same (a run of the slots waits for the copy and its conversion).  On the pipeline only (a board handle:
 * CBV_ERR_STATE); CBV_ERR_ARG for an unknown format, odd w, odd h with a 4:2:0 or Bayer format, or a Bayer frame below
 * 4 x 4, and then nothing has changed.
 * Raw mode: on a pipeline configured with skip_enhance 1 or CBV_SKIP_ENHANCE_PROFILE_RAW a YUV or Bayer format makes the raw ring
 * THE frames (with the latter the warp also applies the boards' colour profiles to its taps, k_warp_raw_profile).  cbv_pipeline_submit
 * only copies the raw slots, cbv_pipeline_upload_raw (that format only) writes a raw slot, cbv_pipeline_run warps straight
 * from the raw frames (k_warp_yuv, k_warp_bayer: byte for byte what the conversion followed by the warp gives) and no BGR frame is ever
 * written; cbv_pipeline_upload (BGR), cbv_pipeline_synth and cbv_pipeline_upload_raw in another format return
 * CBV_ERR_STATE, cbv_pipeline_download(which = 0) converts the slot on demand.  One format per pipeline at a time. */
CBV_API int cbv_pipeline_set_input_format(cbv_pipeline* p, int fmt);
/* The tables of a pipeline whose input format is a Bayer id (developed mosaics, above): [3][1 << bits] bytes, B G R, copied
 * by the call.  tables == NULL restores the format's default (bits is ignored).  cbv_pipeline_set_input_format resets them to
 * the new format's default.  They are used wherever the ring's mosaics become BGR: cbv_pipeline_submit's conversion, raw
 * mode's warp (no BGR ring exists under CBV_SKIP_ENHANCE_PROFILE_RAW, as for 8-bit mosaics), cbv_pipeline_upload_raw of a
 * frame in the pipeline's format, cbv_pipeline_download(which = 0) in raw mode, cbv_pipeline_color_sweep.  Call it between
 * runs: it waits for the runs and copies in flight.  Detector, model and session state are kept, as with
 * cbv_pipeline_set_profile.  On the pipeline only (a board handle: CBV_ERR_STATE); CBV_ERR_STATE when the input format is
 * not a Bayer id; CBV_ERR_ARG when bits does not go with the encoding (8 / 10, 12, 14 or 16 / 10 / 12), and then nothing
 * has changed.  Frames converted earlier stay as they were converted. */
CBV_API int cbv_pipeline_set_bayer_tables(cbv_pipeline* p, const uint8_t* tables, int bits);
/* bytes from one host-ring slot to the next in the current format (a multiple of 256); 0 for a board handle */
CBV_API size_t cbv_pipeline_host_slot_bytes(cbv_pipeline* p);

/* ------------------------------------------------------------------ */
/* Motion-JPEG frames: baseline JPEG decoded on the GPU                */
/* ------------------------------------------------------------------ */
/* CBV_FMT_MJPEG 0x08: one frame is one JPEG stream as a camera emits it (a UVC webcam at 1080p, an IP camera, AVI MJPEG).
 * The single-frame entry points below decode it, and cbv_pipeline_set_input_format takes it as the format of the ingest ring.
 *
 * Accepted: SOF0 (baseline, Huffman, 8-bit samples); one interleaved scan; three components YCbCr with luma sampling
 * 1x1 / 2x1 / 2x2 and chroma 1x1 (4:4:4, 4:2:2, 4:2:0), or one gray component; 8-bit DQT, ids 0..3; up to two DC and two AC
 * tables, several per DHT segment; NO DHT AT ALL = the typical tables of T.81 Annex K.3 (UVC cameras and AVI MJPEG omit
 * them; ids DC 0 / AC 0 luminance, DC 1 / AC 1 chrominance); DRI with any interval; APPn, COM and other segments with a
 * length, skipped; fill 0xFF bytes before a marker; any w, h >= 1 with w * h <= 2^28, partial MCUs cropped.
 * CBV_ERR_UNSUPPORTED, the message naming the reason: progressive, arithmetic, extended or lossless SOFs, 12-bit samples,
 * a 16-bit DQT, a scan that does not hold every component (several scans), four components, an Adobe marker with
 * transform 0, any other sampling, a Huffman table id above 1.  CBV_ERR_ARG: a malformed header.
 *
 * Samples, as libjpeg computes them with its defaults (JDCT_ISLOW, fancy upsampling; what cv2.imdecode calls):
 *   IDCT      jidctint's slow-integer transform on dequantised coefficients: CONST_BITS 13, PASS1_BITS 2, constants 2446,
 *             3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172; columns first with descale 11, rows
 *             with descale 18, DESCALE(x, n) = (x + 2^(n-1)) >> n; sample = clamp(x + 128, 0, 255); int32 arithmetic.
 *             libjpeg's range-limit table WRAPS for x outside [-512, 511]; this definition is the clamp and does not follow
 *             the wrap.  No stream encoded from 8-bit pixels gets near it.
 *   upsample  the "fancy" triangle filter on the component's true size ceil(w * hs / hmax) x ceil(h * vs / vmax), edges
 *             replicated.  h2v1: out[2i] = (3 p[i] + p[i-1] + 1) >> 2, out[2i+1] = (3 p[i] + p[i+1] + 2) >> 2.  h2v2: the
 *             column sum s = 3 p[row] + p[nearer row] (the row above for even output rows, below for odd ones), then
 *             (3 s[i] + s[i-1] + 8) >> 4 and (3 s[i] + s[i+1] + 7) >> 4.  A chroma component whose true width is 1 or 2
 *             (w <= 4) is not filtered but replicated, 2 x 1 or 2 x 2: libjpeg-turbo does so, and its bytes are the pin.
 *   colour    with cb, cr less 128 and F(c) = int(c * 65536 + 0.5): R = y + ((F(1.402) cr + 32768) >> 16),
 *             B = y + ((F(1.772) cb + 32768) >> 16), G = y + ((-F(0.34414) cb - F(0.71414) cr + 32768) >> 16), each
 *             clamped.  A gray stream gives B = G = R = Y, as imdecode(IMREAD_COLOR) does.
 *
 * Damaged entropy data never fails a call and never leaves bounds.  The frame decodes by restart interval (the whole
 * frame without DRI); an interval's bytes end at its restart marker, reads past them return zero bits, decoding of an
 * interval stops at its first bad code, and the coefficients not decoded are 0.  *status gets CBV_JPEG_BAD_CODE (a bit
 * pattern that is no code, a DC size above 15, a run past coefficient 63), CBV_JPEG_NO_DATA (an interval used bits past
 * its end) and CBV_JPEG_RESTART (the number of restart markers is not intervals - 1, or they do not count 0..7 in cycles;
 * intervals whose marker is missing have no data). */
#define CBV_FMT_MJPEG 0x08
#define CBV_JPEG_BAD_CODE 1
#define CBV_JPEG_NO_DATA 2
#define CBV_JPEG_RESTART 4
typedef struct {
    int32_t w, h;
    int32_t components;        /* 1 or 3 */
    int32_t hs, vs;            /* luma sampling: 1,1 (4:4:4, gray) 2,1 (4:2:2) 2,2 (4:2:0) */
    int32_t restart_interval;  /* MCUs, 0 = none */
    int32_t intervals;         /* restart intervals of the frame, 1 without DRI */
    int32_t std_tables;        /* 1: the stream has no DHT */
    uint32_t entropy_offset, entropy_length; /* from the byte behind SOS to the end of the stream */
    /* Stage outputs: samples of all component planes, each padded to whole MCUs, back to back (Y, Cb, Cr).  Component c
     * is blocks_w[c] x blocks_h[c] blocks; its plane has rows of blocks_w[c] * 8 bytes, and its coefficients are
     * [block row][block column][64] int16 in natural (row-major) order at the same element offset. */
    uint32_t plane_elems;
    int32_t blocks_w[3], blocks_h[3];
} cbv_jpeg_info;
/* the header of a stream, up to SOS; host only, reads no entropy data */
CBV_API int cbv_jpeg_probe(const uint8_t* data, size_t n, cbv_jpeg_info* info);
/* The host twin: the same bodies as the kernels, serial, no GPU.  bgr = h rows of w * 3 bytes `stride` apart; coef
 * (int16[plane_elems]) and planes (uint8[plane_elems]) may be NULL. */
CBV_API int cbv_jpeg_decode_host(const uint8_t* data, size_t n, uint8_t* bgr, int stride, int16_t* coef, uint8_t* planes, int32_t* status);
/* the same on the GPU: the single-frame call and the stage entry point */
CBV_API int cbv_jpeg_decode(cbv_ctx* ctx, const uint8_t* data, size_t n, uint8_t* bgr, int stride, int16_t* coef, uint8_t* planes,
                            int32_t* status);
/* The entropy decode has two paths, and the result does not depend on which one runs.
 *   by interval  a lane per restart interval.  A stream without DRI (what a UVC webcam, an IP camera and AVI MJPEG send) is
 *                one interval: one lane.
 *   by piece     A SEGMENT is a stretch of entropy data in front of which the decoder's state is known: the whole scan of a
 *                frame without DRI, or one restart interval (bit 0, block 0, a DC symbol next, predictions 0).  A segment
 *                is cut into pieces of piece_bytes bytes, a lane each.  The state between two symbols is (byte, bit, block
 *                within the MCU, zig-zag index).  The lane of a segment's first piece starts from the true state, every
 *                other lane from a guess, and each stores the state it leaves its piece with.  In every further round a
 *                lane decodes its piece again from the state the lane before it IN ITS SEGMENT left, until a round changes
 *                nothing.  With the true state in front of a segment's piece 0 that fixpoint is unique, the serial decode's
 *                state at every boundary: after round r the exits of pieces 0..r of every segment are true whatever was
 *                guessed, so there are at most as many rounds as the longest segment has pieces, and Huffman codes
 *                resynchronise, so there are few.  Per segment, a prefix sum over the blocks the pieces hold numbers the
 *                blocks from the segment's first one, a last pass writes the coefficients with the DC differences (no
 *                block outside the segment's own MCUs, and nothing behind the piece where the serial decode of that
 *                interval dies or runs out of data), and a per-component scan that starts from 0 at every segment sums the
 *                differences of the blocks decoded.  Coefficients, planes, BGR and status are the interval path's bit for
 *                bit, for damaged data as well (markers missing, extra or misnumbered, truncated data, bad codes), at every
 *                piece size.  The zero bits behind a segment's end are decoded by one lane, as by interval, and no piece
 *                reads a restart marker.
 * CBV_JPEG_ENTROPY_AUTO (the default) takes pieces for frames without DRI and intervals otherwise; _INTERVAL takes intervals
 * for every frame; _PIECES is AUTO's choice: a frame with DRI still goes by interval and reports zero figures; _SEGMENTS takes
 * the piece path for every frame, a frame with DRI with its restart intervals as segments (segment j = the bytes between
 * markers j - 1 and j of those found, empty at the data's end where its marker is missing;
 * n_j = max(1, ceil(bytes / piece_bytes)) pieces), a frame without DRI exactly as _PIECES.  3 is no mode and stays
 * CBV_ERR_ARG (tests of the piece path hold that).  piece_bytes: 0 = the library's default (64), otherwise a multiple of 4
 * from 4 to 2^24; small pieces exist for tests (a symbol then spans several pieces, and a piece
 * inside one symbol decodes nothing and passes its entry on). */
#define CBV_JPEG_ENTROPY_AUTO 0
#define CBV_JPEG_ENTROPY_INTERVAL 1
#define CBV_JPEG_ENTROPY_PIECES 2
#define CBV_JPEG_ENTROPY_SEGMENTS 4
/* By segments: pieces = the sum of the n_j, rounds <= the largest n_j, settled_round0 >= the intervals (every first piece
 * is true in round 0). */
typedef struct {
    uint32_t pieces;          /* pieces of the frame, ceil(entropy_length / piece_bytes); 0: the frame was decoded by interval */
    uint32_t rounds;          /* rounds until no exit of the frame changed, round 0 counted: 1 <= rounds <= pieces */
    uint32_t settled_round0;  /* pieces whose exit state of round 0 was already the true one */
} cbv_jpeg_decode_stats;
/* cbv_jpeg_decode_host / cbv_jpeg_decode with the path chosen; stats may be NULL.  The plain calls are these with AUTO, 0, NULL. */
CBV_API int cbv_jpeg_decode_host_ex(const uint8_t* data, size_t n, uint8_t* bgr, int stride, int16_t* coef, uint8_t* planes, int32_t* status,
                                    int mode, uint32_t piece_bytes, cbv_jpeg_decode_stats* stats);
CBV_API int cbv_jpeg_decode_ex(cbv_ctx* ctx, const uint8_t* data, size_t n, uint8_t* bgr, int stride, int16_t* coef, uint8_t* planes,
                               int32_t* status, int mode, uint32_t piece_bytes, cbv_jpeg_decode_stats* stats);
/* The ingest ring in Motion-JPEG: cbv_pipeline_set_input_format(p, CBV_FMT_MJPEG).  A slot of the host ring holds one
 * stream from its first byte; cbv_pipeline_host_slot_bytes is the capacity of a slot, w * h / 2 rounded up to 256 unless
 * cbv_pipeline_set_jpeg_slot_bytes set another (rounded up to 256; with the format set it frees both rings, as a format
 * change does).  The capture side writes a stream's length into its entry of cbv_pipeline_host_jpeg_lengths (a pinned
 * uint32[max_frames] that lives as long as the pipeline; NULL before the format was first set).
 * cbv_pipeline_submit then parses the headers of the slots straight from the pinned ring (it never reads the entropy
 * data).  On the first slot it cannot take it returns that slot's error, the message naming the slot, with nothing
 * enqueued: a length of 0 or above the capacity (CBV_ERR_ARG), a malformed or unsupported stream (as above), a size that
 * differs from the pipeline's (CBV_ERR_UNSUPPORTED), more than 16 different table sets (Huffman and quantisation tables, by
 * content) since the cache was last emptied (CBV_ERR_UNSUPPORTED; a camera's tables do not change).  Otherwise it copies no
 * more than each slot's used bytes (rounded up to 256) and enqueues the decode into the BGR frame ring on the copy stream
 * behind the copy, with the ordering promises of the other formats.  Frames of different sampling and restart interval may
 * share a submit.  The decode's device scratch is sized when the format is set, for chunks of cbv_pipeline_jpeg_depth
 * frames (8 unless set) in the sampling that needs most; submit allocates nothing.  Unless the planes mode below is set,
 * Motion-JPEG is not a raw format: a pipeline without enhancement keeps its BGR ring, as for BGR input, and the decode
 * fills it.  Until the copy has completed (cbv_pipeline_wait_submitted) the slots' bytes and lengths belong to it. */
CBV_API uint32_t* cbv_pipeline_host_jpeg_lengths(cbv_pipeline* p);
CBV_API int cbv_pipeline_set_jpeg_slot_bytes(cbv_pipeline* p, size_t bytes);
/* one stream decoded into a slot of the frame ring, synchronous, like cbv_pipeline_upload; in any input format but not in
 * the raw mode of a YUV or Bayer format (CBV_ERR_STATE).  In the raw mode of the planes mode below it decodes into the
 * slot of the plane ring and writes status, figures and descriptor as cbv_pipeline_submit does. */
CBV_API int cbv_pipeline_upload_jpeg(cbv_pipeline* p, int slot, const uint8_t* data, size_t n);
/* the status words (CBV_JPEG_*) of the streams last decoded into the slots; waits for the submitted decodes */
CBV_API int cbv_pipeline_jpeg_status(cbv_pipeline* p, int slot0, int count, int32_t* status);
/* The entropy path of the pipeline's decodes (submit and upload_jpeg) and its piece size; call between runs.  The piece
 * path's device scratch, depth x ceil(slot bytes / piece_bytes) piece states (by segments ceil(w / 8) x ceil(h / 8) more
 * per frame, and three words per possible interval), is sized here and when the format is set; submit still allocates
 * nothing.  When the scratch cannot be allocated the call fails and the setting that was stays with its scratch.
 * CBV_ERR_STATE on a board handle. */
CBV_API int cbv_pipeline_set_jpeg_entropy(cbv_pipeline* p, int mode, uint32_t piece_bytes);
/* the figures of the streams last decoded into the slots (zeros for a frame decoded by interval); waits like cbv_pipeline_jpeg_status */
CBV_API int cbv_pipeline_jpeg_stats(cbv_pipeline* p, int slot0, int count, cbv_jpeg_decode_stats* stats);
/* The decode depth: how many frames a Motion-JPEG submit decodes per launch through one set of scratch buffers, 1 to 64,
 * 8 unless set.  A frame on the piece path is one workgroup, so the depth is how many of them a launch puts on the GPU.
 * Frames, status, figures and detector results do not depend on it.  Call between runs: it waits for the copy stream and
 * sizes the coefficient, plane, marker, piece and segment scratch anew, all of which scale with it; before the format is
 * set it is only stored.  The cost: per frame of depth, 3 bytes per sample of the frame in the sampling that needs most
 * (4:4:4 padded to 16 x 16 MCUs: 18.8 MB at 1080p; 2 bytes per sample, 12.5 MB, where the planes go to the plane ring of
 * the planes mode below and the scratch holds none) and 4 bytes per possible restart interval (ceil(w / 8) x ceil(h / 8) of
 * them), plus the piece states (36 bytes per piece; by segments 40 per piece and 12 more per possible interval, the
 * segment words; the piece counts are cbv_pipeline_set_jpeg_entropy's).  CBV_ERR_ARG outside 1..64, CBV_ERR_STATE on a board handle; when the scratch
 * cannot be allocated the call fails and the depth that was stays with its scratch. */
#define CBV_JPEG_DEPTH_DEFAULT 8
#define CBV_JPEG_DEPTH_MAX 64
CBV_API int cbv_pipeline_set_jpeg_depth(cbv_pipeline* p, int frames);
/* the depth set (or the default); negative: an error */
CBV_API int cbv_pipeline_jpeg_depth(cbv_pipeline* p);
/* The planes mode: Motion-JPEG as a raw format.  Off by default, and then everything above holds as it stands.  With a
 * mode other than CBV_JPEG_PLANES_OFF, CBV_FMT_MJPEG is a raw format like the YUV and Bayer ones: on a pipeline configured
 * with skip_enhance 1 or CBV_SKIP_ENHANCE_PROFILE_RAW the decode stops at the planes, which the inverse DCT writes straight
 * into the frame's slot of a device plane ring; the colour step is not run, the decode's scratch holds no plane buffer, the
 * pipeline holds no BGR ring, and the warp samples the plane ring: a tap at (x, y) is the pixel defined above (the luma
 * sample, the chroma upsampled on the component's true size, the colour step), through the board's colour profile in the
 * profile mode, so the results are byte for byte those of the decode followed by the warp.  A tap outside the frame is BGR 0.
 * On a pipeline with enhancement, or configured CBV_SKIP_ENHANCE_PROFILE, the mode changes nothing but the refusal below:
 * the decode fills the BGR ring.
 *   The mode names the largest sampling a slot of the ring can hold; samplings in the order gray, 4:2:0, 4:2:2, 4:4:4:
 * _GRAY admits gray streams, _420 gray and 4:2:0, _422 those and 4:2:2, _444 all.  cbv_jpeg_plane_slot_bytes(w, h, mode) is
 * the size of a slot: the largest plane_elems (cbv_jpeg_info) among the samplings the mode admits, whole MCUs, rounded up
 * to 256 (at 16 x 1, 4:2:0 needs 384 samples and 4:2:2 256); 0 for _OFF, an unknown mode, w < 1 or h < 1.  Host only.  At
 * 1080p a _420 slot is 3.1 MB, a _422 slot 4.1 MB and a _444 slot 6.2 MB, as much as a BGR slot.
 *   cbv_pipeline_set_jpeg_planes: on the pipeline only (CBV_ERR_STATE on a board handle); an unknown mode is CBV_ERR_ARG and
 * changes nothing.  Before the format is set the mode is only stored; with the format set it waits for what is in flight,
 * makes the new ring before it lets the old one go (when an allocation fails the setting that was stays, with its rings),
 * and frees the ingest rings as a format change does.  The ring is zeroed and the descriptors the warp reads are gray
 * frames of the pipeline's size, so a slot never decoded is a black frame and every read is in bounds.
 *   In planes mode, whatever the configuration, cbv_pipeline_submit and cbv_pipeline_upload_jpeg refuse a stream whose
 * sampling the mode does not admit like a stream of another size: CBV_ERR_UNSUPPORTED, the message naming the slot and
 * the sampling, nothing enqueued.  A run in flight reads the planes and the descriptors of its slots; submit changes both
 * only behind its wait for the newest run that reads the slots.  Every address the warp forms comes from the descriptor the
 * host parser has validated, none from entropy data: a damaged stream changes sample values and nothing else.
 *   In the raw mode of the planes mode: cbv_pipeline_download(which = 0) converts the slot on demand (the colour step on
 * that slot: cbv_jpeg_decode_host's frame byte for byte); cbv_pipeline_upload, _synth and _upload_raw return CBV_ERR_STATE;
 * status, figures, entropy path and depth work as before; cbv_pipeline_color_sweep samples the plane ring. */
#define CBV_JPEG_PLANES_OFF 0
#define CBV_JPEG_PLANES_GRAY 1
#define CBV_JPEG_PLANES_420 2
#define CBV_JPEG_PLANES_422 3
#define CBV_JPEG_PLANES_444 4
CBV_API int cbv_pipeline_set_jpeg_planes(cbv_pipeline* p, int mode);
/* the mode set; negative: an error */
CBV_API int cbv_pipeline_jpeg_planes(cbv_pipeline* p);
CBV_API size_t cbv_jpeg_plane_slot_bytes(int w, int h, int mode);
/* The stage entry point, host in, host out, beside cbv_warp_color_profile_raw: cbv_jpeg_decode, then
 * cbv_apply_color_profile when profile->enabled, then cbv_warp_perspective (and the rotation by 180 degrees), byte for
 * byte, with the BGR frame never made.  A tap outside the frame is BGR 0.  *status = the decode's status word.  Refusals:
 * those of cbv_jpeg_decode and those of cbv_warp_color_profile_raw, with `out` untouched. */
CBV_API int cbv_warp_jpeg(cbv_ctx* ctx, const uint8_t* data, size_t n, const cbv_color_profile* profile, const double* M9, int dw, int dh, int rot180,
                          uint8_t* out, int out_stride, int32_t* status);

/* ------------------------------------------------------------------ */
/* several boards seen by one camera                                   */
/* ------------------------------------------------------------------ */
/* A configured pipeline holds up to CBV_MAX_BOARDS boards; the pipeline itself is board 0.  Extra boards share its frame
 * ring, ingest ring, enhancement (cbv_pipeline_config::enhance, chunk, lanes, keep_enhanced, enhance_region) and lanes:
 * every frame is uploaded and enhanced once, whatever the number of boards.  Each board has its own geometry, detector
 * settings and temporal state (reference squares, history, ChangeDetector model, NoiseHandler, squares_to_check), and
 * computes exactly what a pipeline configured with the parent's enhancement and the board's settings computes on the
 * same frames.  The per-board stages of a run are one kernel launch each for all boards. */
#define CBV_MAX_BOARDS 8

/* The per-board subset of cbv_pipeline_config (same meaning, same checks). */
typedef struct {
    double M[9];                 /* getPerspectiveTransform of the board's quad */
    int32_t board_size;
    int32_t rot180;
    int32_t n_rois;
    cbv_roi rois[CBV_MAX_SQUARES];
    int32_t history_size;
    double min_presence;
    double change_threshold;
    double z_threshold;
    double initial_variance;
    int32_t use_hough;
    cbv_hough_params hough;
} cbv_board_config;

/* Attach a board to a configured pipeline `parent` (not itself a board handle) and return its handle in *board.
 * cbv_pipeline_run(parent, ...) then processes every attached board for those slots.  A board handle is accepted by the
 * per-board calls, which act on that board alone: cbv_pipeline_results, _noise_results, _square_stats, _hough,
 * _download (which = 2), _calibrate, _update_references, _set_check_squares, _reset_state, _set_model_update, _set_change_blur, _model.  On a board handle
 * cbv_pipeline_run, _upload, _upload_raw, _submit, _set_input_format, _synth, _configure, _host_ring and _download with
 * which 0 or 1 fail with CBV_ERR_STATE (_host_ring returns NULL, _host_slot_bytes 0); cbv_pipeline_reset_state(parent) resets board 0 only.
 * Lifecycle: cbv_pipeline_destroy(board) detaches and frees the board (the other boards are unchanged);
 * cbv_pipeline_destroy(parent) frees its boards too, and their handles are dead from then on.
 * cbv_pipeline_configure(parent) fails with CBV_ERR_STATE while boards are attached: destroy them first.
 * With enhance_region the enhanced region is the bounding rectangle of every board's warp footprint, recomputed on
 * attach and detach.  Fails with CBV_ERR_ARG on bad arguments (those cbv_pipeline_configure rejects, or a ninth board),
 * and leaves the parent and its other boards as they were on any failure. */
CBV_API int cbv_pipeline_add_board(cbv_pipeline* parent, const cbv_board_config* b, cbv_pipeline** board);

/* ------------------------------------------------------------------ */
/* per-frame update of the ChangeDetector background model             */
/* ------------------------------------------------------------------ */
/* cbv_pipeline_calibrate captures the model once; by default it then stays as it is and every later frame is compared
 * with the calibration frame.  With a model-update mode the board also runs the second half of the reference's class,
 * ChangeDetector.update_all_references (change_detector.py:67-92), after every frame: for each frame of a run in slot
 * order (and the runs in the order they were enqueued), first detect_changes_detailed against the model as the frame
 * before left it (`changed`, `parcial`, `total` of cbv_frame_result and `z_count`, `z_max` of cbv_pipeline_square_stats,
 * change_detector.py:105-167), then
 *   CBV_MODEL_FROZEN     nothing (the default);
 *   CBV_MODEL_EVERY      update_all_references(squares) with no focus squares: mean = (1 - alpha) mean + alpha gray,
 *                        var = max((1 - alpha) var + alpha (gray - new mean)^2, 10) on every pixel of every square
 *                        (change_detector.py:77-92), float32 with one rounding per operation, as cbv_squares_ema does it;
 *   CBV_MODEL_UNCHANGED  the same update on the squares that are NOT in the frame's result dict (pct_changed < 5,
 *                        change_detector.py:139-141) only, i.e. set_focus_squares(all - reported), update_all_references,
 *                        clear_focus (change_detector.py:49-65): a square under a hand or a piece that has just moved
 *                        keeps its model until the caller calibrates again, the others follow the light.  A frame that
 *                        reports every square updates none.
 * The PieceDetector side of the results (raw / stable occupancy, visual_changes, processed, circular, NoiseHandler) does
 * not read the model and is the same in every mode. */
#define CBV_MODEL_FROZEN    0
#define CBV_MODEL_EVERY     1
#define CBV_MODEL_UNCHANGED 2
/* Mode and `alpha` (ChangeDetector's attribute, change_detector.py:25: 0.1) of one board, any board handle.  Applies to
 * the runs enqueued after the call; runs in flight keep what they were launched with.  Allowed before or after
 * cbv_pipeline_calibrate: an uncalibrated board has no model and nothing is updated until it is calibrated.
 * CBV_ERR_ARG for an unknown mode or an alpha outside [0, 1], and then nothing has changed. */
CBV_API int cbv_pipeline_set_model_update(cbv_pipeline* board, int mode, double alpha);
/* ChangeDetector.blur_kernel / _kernel of a board (pipeline or attached board), default 5.  Values below 1 count as 1,
 * then k |= 1 (calibrate_sensitivity.py:139).  Applies to the runs enqueued after the call; the model is kept: the next
 * frames are preprocessed with the new kernel (change_detector.py:49-56: BGR2GRAY, GaussianBlur((k, k), 0) on the square
 * alone) and judged against the means and variances as they are.  Only the ChangeDetector side reads it (`changed`,
 * `parcial`, `total`, `z_count`, `z_max`, cbv_pipeline_calibrate, the model updates, cbv_pipeline_model); detect_piece has
 * its own 5 x 5 preprocess, so `circular`, the PieceDetector, the NoiseHandler and the game session do not depend on it.
 * With k = 5 the board is what it was without this call; with another kernel it gets a second ring of planes and one more
 * kernel per chunk (k_change_blur_stats, CBV_K_CHANGE_BLUR).  Allowed before cbv_pipeline_configure: the kernel stays with
 * the board.  cbv_pipeline_calibrate(slot) of a slot whose last run used another kernel than the board's current one fails
 * with CBV_ERR_STATE: run the slot again first.  k > 31: CBV_ERR_UNSUPPORTED (cbv_squares_load's limit), and then nothing
 * has changed.  REFLECT_101 folds as often as needed, so every kernel fits every square. */
CBV_API int cbv_pipeline_set_change_blur(cbv_pipeline* board, int blur_kernel);
/* The colour profile of a board (pipeline = board 0, or an attached board) in the profile modes (skip_enhance =
 * CBV_SKIP_ENHANCE_PROFILE or CBV_SKIP_ENHANCE_PROFILE_RAW; otherwise CBV_ERR_STATE): one camera may watch a lilac board
 * beside a green one.  Every board starts with the pipeline's configured profile (cfg.enhance.profile).  Joins the runs in
 * flight and applies to the runs enqueued after the call; detector, model, noise and session state are kept.  While no
 * board has an enabled profile the plain warp is launched; otherwise the profile kernel runs with one table per board,
 * and a board whose profile is disabled keeps its taps as they are.  CBV_ERR_ARG for a profile field that is not finite,
 * and then nothing has changed.  cbv_pipeline_configure sets every board's profile anew. */
CBV_API int cbv_pipeline_set_profile(cbv_pipeline* board, const cbv_color_profile* profile);
/* The model of square `roi` after every run enqueued so far (waits for them): which = 0 the mean plane
 * (change_detector.py:44), 1 the variance plane (change_detector.py:45), `out` = w * h floats, row major.  Read only.
 * CBV_ERR_STATE while the board is not calibrated. */
CBV_API int cbv_pipeline_model(cbv_pipeline* board, int which, int roi, float* out);

/* ------------------------------------------------------------------ */
/* ChangeDetector sensitivity sweep on the device                       */
/* ------------------------------------------------------------------ */
/* What calibrate_sensitivity.py's loop computes (:110-162) for many trackbar positions at once, on frames already in the
 * board's warped ring.  The tool calibrates once and never updates the model, so every frame is judged against the blurred
 * gray of the calibration frame (a u8 plane) with the constant variance initial_variance: a pixel's score is
 * z = fdiv_rn((float)d, sqrt_rn((float)initial_variance)) with d = |gray - mean| an integer in 0..255, and the 256-bin
 * histogram of d per (blur kernel, frame, square) answers every (z_threshold, initial_variance) exactly.
 * DEFINITION: setting s on frame i is what a board gives that was configured with z_threshold, initial_variance and
 * blur_kernel of s (the float32 casts of cbv_pipeline_configure, the normalisation of cbv_pipeline_set_change_blur: below 1
 * counts as 1, then |= 1), calibrated by cbv_pipeline_calibrate(calib_slot), left frozen, and run on slot slot0 + i. */
typedef struct { double z_threshold; double initial_variance; int32_t blur_kernel; int32_t pad; } cbv_sweep_setting;
typedef struct {              /* one (setting, frame): 32 bytes */
    uint64_t changed, parcial, total;  /* as in cbv_frame_result */
    float z_max;              /* max z_score over the reported squares, 0 if none */
    uint8_t n_changed, n_total;
    uint8_t flags;            /* 1 is_hand, 2 is_move (classify_hand_pattern, change_detector.py:169-201) */
    int8_t lifted;            /* roi of the single move candidate when n_changed == 1 and not is_hand, else -1 */
} cbv_sweep_record;
#define CBV_SWEEP_HAND 1
#define CBV_SWEEP_MOVE 2
typedef struct {              /* one setting over the call's frames */
    uint32_t frames_changed, frames_hand, frames_move, frames_lifted;
    uint32_t squares_reported;   /* sum of n_changed */
    float z_max;
} cbv_sweep_summary;
typedef struct { float planes_ms, hist_ms, eval_ms; int32_t kernels_distinct, chunk_frames; } cbv_sweep_info;
#define CBV_SWEEP_MAX_SETTINGS 65536  /* the tool's trackbars span 51 x 80 x 8 positions */
#define CBV_SWEEP_MAX_CHUNK 64        /* frames per chunk at most */
#define CBV_SWEEP_DEFAULT_CHUNK 16    /* chunk_frames = 0 */
/* Any board handle.  Reads the board's warped ring only: model, planes, statistics, results, temporal state and settings
 * of the board are neither read nor written, and a pipeline that never calls this launches and allocates nothing for it.
 * Waits for the runs in flight and returns when `records` ([ns][count], setting major; may be NULL) and `summaries` ([ns],
 * may be NULL) are filled; `info` (may be NULL) gets the GPU time of the three stages (event pairs: calibration planes,
 * k_change_hist, k_sweep_eval), the number of distinct blur kernels and the chunk used.  Histograms are made and consumed
 * in chunks of `chunk_frames` frames (0 = CBV_SWEEP_DEFAULT_CHUNK, at most CBV_SWEEP_MAX_CHUNK), which bounds the call's
 * own device memory whatever `count` is: chunk x 16 kernels x 32 KiB of histograms (at most 32 MiB), 16 plane sets of the
 * board, ns x 40 bytes of settings and summaries and, with `records`, ns x chunk x 32 bytes of staging.  The result does not
 * depend on the chunk.  All of it is freed before the call returns.
 * CBV_ERR_STATE: not configured, or calib_slot or one of the frame slots was never run.  CBV_ERR_ARG: null or empty
 * arguments, slots outside the ring, chunk_frames outside 0..CBV_SWEEP_MAX_CHUNK, ns above CBV_SWEEP_MAX_SETTINGS, or an
 * initial_variance whose float32 value is not finite or not above 0.  CBV_ERR_UNSUPPORTED: a blur kernel above 31.  After
 * any error nothing has changed. */
CBV_API int cbv_pipeline_sweep(cbv_pipeline* board, int calib_slot, int slot0, int count, const cbv_sweep_setting* settings, int ns,
                               int chunk_frames, cbv_sweep_record* records, cbv_sweep_summary* summaries, cbv_sweep_info* info);
/* The histogram itself: out[roi][d] = pixels of square roi in slot `slot` with |gray - calibration gray| == d under
 * `blur_kernel` (normalised as above); a square has at most 128 x 128 pixels.  Errors as cbv_pipeline_sweep. */
CBV_API int cbv_pipeline_change_hist(cbv_pipeline* board, int calib_slot, int slot, int blur_kernel, uint16_t* out);
/* The host twin of k_sweep_eval, no GPU: hist[n][256] and n_px[n] (pixels per square) of ONE frame, n <= CBV_MAX_SQUARES
 * -> out[ns]; a setting's blur_kernel is not read (the histograms were made with it).  0, or CBV_ERR_ARG. */
CBV_API int cbv_sweep_eval_host(const uint16_t* hist, const int32_t* n_px, int n, const cbv_sweep_setting* s, int ns, cbv_sweep_record* out);

/* ------------------------------------------------------------------ */
/* game session on the device: stable moves, smart scan, FEN           */
/* ------------------------------------------------------------------ */
/* The back half of GameSession.on_frame (game_session.py:130-265) for every frame of every run of a board, on the
 * device: the smart-scan `squares_to_check` set (:130-154), _process_stable_move (:181-225), the move rule, and after an
 * accepted move update_references(squares) and noise.reset() (:219-223).  Time is counted in frames.  Per frame, in this
 * order: c += 1; the frame's check set is None when c % scan_period == 0, else the smart mask (occupied squares plus
 * (file, 7 - rank) of every legal destination, the reference's own conversion); vision = stable_occupied; when
 * popcount(expected ^ vision) > max_diff the stable set is emptied and stable_count = 0, else stable_count counts the
 * frames the set stayed the same; a move is looked for when stable_count >= stability_required, c - last move's c >
 * cooldown_frames and the frame's NoiseHandler state is not NOISE_ACTIVE; the rule must find exactly one legal move; it
 * is pushed and recorded, stable_count = 0, the references become THIS frame's squares (cache cleared, history kept,
 * as cbv_pipeline_update_references) and the NoiseHandler restarts.  on_move_detected is taken as always True unless
 * the session is `online` (below: LichessSession's hook, turn gate and opponent moves).  The frames of a run behind an
 * accepted move are scanned again from that state inside the run, so a run of any length gives what one-frame runs
 * driven from the host give. */
#define CBV_SESSION_RULE_INFER     0  /* GameSession._infer_move (game_session.py:229-265) */
#define CBV_SESSION_RULE_OCCUPANCY 1  /* GameState.process_occupancy_change (game_state.py:40-195) */
#define CBV_SESSION_RING 1024         /* move records kept between two cbv_pipeline_session_moves calls */
typedef struct {
    int32_t rule;               /* CBV_SESSION_RULE_* */
    int32_t stability_required; /* 20   game_session.py STABILITY_REQUIRED */
    int32_t cooldown_frames;    /* 60   MOVE_COOLDOWN (2.0 s) at 30 fps */
    int32_t scan_period;        /* 30   full scan every scan_period-th frame (game_session.py:130) */
    int32_t max_diff;           /* 4    game_session.py:189 */
    int32_t smart_scan;         /* 1: the session owns the boards' check sets; 0: they stay the caller's */
    int32_t online;             /* CBV_SESSION_ONLINE_*: 0 off, 1 the player is white, 2 black (rule INFER only) */
    int32_t radar;              /* 1: every frame leaves a cbv_session_radar record (cbv_pipeline_session_radar) */
    int32_t tone;               /* 1: the rule breaks ties with the board's piece tones (cbv_pipeline_set_tones); 0: off */
} cbv_session_config;
typedef struct {
    int32_t frame;      /* frames since cbv_pipeline_session_begin, 0 based */
    uint16_t move;      /* cbv_move of include/cbv_chess.h */
    uint8_t status;     /* CBV_GAME_* (rule 0: CBV_GAME_MOVE_CONFIRMED) */
    uint8_t candidates; /* candidate moves the rule saw (1) */
} cbv_session_move;
typedef struct {
    int8_t sq[64];              /* 0 empty, piece type | 8 for black; index = python-chess square */
    int32_t turn, castling, ep, halfmove, fullmove;
    uint64_t expected;          /* the board's occupancy, ROI numbering */
    uint64_t smart_mask;        /* the smart-scan set, ROI numbering */
    uint64_t stable_occupancy;  /* ROI numbering */
    uint64_t rejected;          /* the last occupancy the rule rejected on this board (valid with rejected_valid) */
    int32_t rejected_valid;
    int32_t stable_count;
    int32_t c;                  /* frames since begin */
    int32_t last_move_c;        /* c of the last accepted move, 0 = none yet */
    int32_t n_moves;            /* moves accepted since begin */
    int32_t last_candidates;    /* candidates (rule 0) or status (rule 1) of the last rule call, -1 = none yet */
    /* online sessions (all zero / none otherwise): */
    int32_t waiting_for_opponent; /* LichessSession.waiting_for_opponent: a move the rule finds now is turned down */
    int32_t ignored_move;       /* cbv_move of the last move turned down, CBV_MOVE_NONE = none yet */
    int32_t ignored_frame;      /* its frame (as cbv_session_move.frame), -1 = none yet */
    int32_t n_ignored;          /* rule calls turned down since begin (not the later identical frames the memo skips) */
} cbv_session_state;
/* Start a session on a board (any board handle) of a configured pipeline, from `fen` (NULL = the start position).
 * CBV_ERR_STATE before cbv_pipeline_configure or on a board that has not 64 squares, CBV_ERR_ARG for a bad FEN or
 * configuration.  A running session is replaced.  With smart_scan, cbv_pipeline_set_check_squares on the board returns
 * CBV_ERR_STATE until the session ends; cbv_pipeline_update_references and cbv_pipeline_reset_state stay legal.
 * cfg.tone: the rule breaks ties with the frame's piece tones (include/cbv_chess.h, "tie-break"); CBV_ERR_STATE on a board
 * whose tones are off (cbv_pipeline_set_tones). */
CBV_API int cbv_pipeline_session_begin(cbv_pipeline* board, const cbv_session_config* cfg, const char* fen);
/* End it: later runs are what they were before the session, with the check sets the caller had set before it. */
CBV_API int cbv_pipeline_session_end(cbv_pipeline* board);
/* The moves accepted since the previous call, oldest first (waits for the runs in flight).  *n = records written.
 * CBV_ERR_UNSUPPORTED, with the newest records in `out`, when more than CBV_SESSION_RING (or `cap`) were waiting. */
CBV_API int cbv_pipeline_session_moves(cbv_pipeline* board, cbv_session_move* out, int cap, int* n);
CBV_API int cbv_pipeline_session_state(cbv_pipeline* board, cbv_session_state* out);
/* Host buffers, no GPU (ctx may be NULL): the walk itself over n frames from their result and NoiseHandler records;
 * `state` is read and updated.  Stops behind the first accepted move: returns the frames consumed (n when none was
 * accepted), *accepted = 1 and *move filled when one was.  Negative on bad arguments. */
CBV_API int cbv_session_walk(const cbv_session_config* cfg, cbv_session_state* state, const cbv_frame_result* results,
                             const cbv_noise_result* noise, int n, cbv_session_move* move, int* accepted);
/* a cbv_session_state at the start of a session from `fen` (NULL = the start position); 0, or CBV_ERR_ARG */
CBV_API int cbv_session_state_init(cbv_session_state* state, const char* fen);
/* the FEN of a session state (python-chess Board.fen()); returns the length */
CBV_API int cbv_session_state_fen(const cbv_session_state* state, char* out, int cap);

/* ---- online play: opponent moves, the turn gate and the radar (LichessSession, lichess_session.py) ----
 * The network client stays with the caller; the session logic it feeds runs on the device.
 * Turn gate (cfg.online, LichessSession.on_move_detected, lichess_session.py:44-65): waiting_for_opponent starts as
 * "the side to move is not the player's" (is_my_turn("") for the start position).  While it is set, a move the rule
 * finds is NOT pushed: no reference refresh, no NoiseHandler restart, stable_count stays; the move goes to ignored_move /
 * ignored_frame, n_ignored counts the rule call, and the occupancy goes into the `rejected` memo, so the identical frames
 * behind it do not run the rule again (they are not counted either; the reference runs and turns down the same move on
 * each of them, which changes nothing).  An accepted own move sets waiting_for_opponent.  lichess.make_move failing is a
 * network outcome and is taken as success.  cfg.online with CBV_SESSION_RULE_OCCUPANCY is CBV_ERR_ARG.
 * Board events (LichessSession._sync_moves, lichess_session.py:89-117): the caller replays the game's move list into a
 * cbv_session_pos and queues it for a frame of the session.  The event takes effect BEFORE frame `at_frame` is processed
 * (the stream thread holds the lock between two on_frame calls), inside a run of any length and without waiting for the
 * host: it replaces the board, recomputes `expected` and the smart mask, clears the `rejected` memo and sets
 * waiting_for_opponent, and nothing else (stable_count, stable_occupancy, last_move_c, the detector's references, cache
 * and history and the NoiseHandler stay, as in the reference).  The frames from at_frame on use the new smart mask.
 * Radar (cfg.radar, GameSession._update_radar_ui, game_session.py:271-291): per frame, before its stable-move step and
 * with the board in force at that frame (events due there applied): when expected & ~vision has exactly one member and
 * the piece on it has the side to move's colour, `lifted` is that square and `destinations` the union of to_square over
 * the legal moves from it; else -1 and 0.  ROI numbering, like every square set here.
 * Out of scope: the HTTP client and its threads, make_move failures and drawing.  (The radar of calibrate_sensitivity.py
 * works on ChangeDetector move candidates, not occupancy: the sensitivity sweep below gives `lifted` per setting and frame,
 * and the binding's change_radar finishes it on the host.) */
#define CBV_SESSION_ONLINE_OFF   0
#define CBV_SESSION_ONLINE_WHITE 1
#define CBV_SESSION_ONLINE_BLACK 2
#define CBV_SESSION_EVENTS 64         /* board events that may wait on a board at a time */
typedef struct {                /* the board part of cbv_session_state */
    int8_t sq[64];
    int32_t turn, castling, ep, halfmove, fullmove;
} cbv_session_pos;
typedef struct {
    int32_t at_frame;           /* session frame (0 based since begin) in front of which the event applies */
    int32_t waiting_for_opponent;
    cbv_session_pos pos;
} cbv_session_event;
typedef struct {
    int8_t lifted;              /* ROI index of the lifted piece, -1 = none */
    uint64_t destinations;      /* ROI-numbered set of its legal destinations */
} cbv_session_radar;
/* `moves`: UCI tokens separated by blanks (NULL or "" = none), replayed from the start position as _sync_moves does:
 * a token that is not a legal move there is skipped.  *pushed (may be NULL) = tokens played.  0, or CBV_ERR_ARG. */
CBV_API int cbv_session_pos_from_moves(const char* moves, cbv_session_pos* out, int* pushed);
/* Queue a board event on a board with a session.  CBV_ERR_ARG when at_frame lies below the frames already enqueued for
 * the session (runs in flight included) or below the last queued event's at_frame; CBV_ERR_UNSUPPORTED when
 * CBV_SESSION_EVENTS events are waiting; nothing changes in either case.  Does not wait for the runs in flight.  An
 * event whose frame no run reaches before cbv_pipeline_session_end (or a new begin) is dropped. */
CBV_API int cbv_pipeline_session_sync(cbv_pipeline* board, int at_frame, const cbv_session_pos* pos, int waiting_for_opponent);
/* *frames = the frames enqueued for the board's session so far = the session frame index of the next run's first frame
 * (does not wait for the runs in flight) */
CBV_API int cbv_pipeline_session_frames(cbv_pipeline* board, int* frames);
/* the radar records of processed slots (cfg.radar; CBV_ERR_STATE without) */
CBV_API int cbv_pipeline_session_radar(cbv_pipeline* board, int slot0, int n, cbv_session_radar* out);
/* cbv_session_walk with board events and the radar, host buffers: `events` (non-decreasing at_frame, none below
 * state->c, at most CBV_SESSION_EVENTS) apply in front of the frame whose index (state->c before it) they name;
 * *events_used = how many applied among the frames consumed; `radar` (may be NULL) gets one record per frame consumed.
 * Returns the frames consumed like cbv_session_walk; CBV_ERR_ARG / CBV_ERR_UNSUPPORTED as cbv_pipeline_session_sync and
 * cbv_pipeline_session_begin give them, and then nothing has changed. */
CBV_API int cbv_session_walk_events(const cbv_session_config* cfg, cbv_session_state* state, const cbv_frame_result* results,
                                    const cbv_noise_result* noise, int n, const cbv_session_event* events, int n_events,
                                    int* events_used, cbv_session_radar* radar, cbv_session_move* move, int* accepted);
/* cbv_session_state_init for a session with `cfg` (waiting_for_opponent from cfg->online and the side to move) */
CBV_API int cbv_session_state_init_cfg(cbv_session_state* state, const cbv_session_config* cfg, const char* fen);

/* The device's wave-parallel legal move generator on one position, for tests: list(board.legal_moves) of `fen` in
 * python-chess order; *n = count. */
CBV_API int cbv_session_device_legal_moves(cbv_ctx* ctx, const char* fen, uint16_t* out, int cap, int* n);
/* ... and its time: one launch that builds the list `reps` times, *ms = the launch's GPU time (timing tools) */
CBV_API int cbv_session_generator_time(cbv_ctx* ctx, const char* fen, int reps, double* ms);

/* ------------------------------------------------------------------ */
/* piece colour per square (tones) and the tie-break of the move rules  */
/* ------------------------------------------------------------------ */
/* The reference detects occupancy only.  This stage adds one measurement per square, whether the piece on it is white or
 * black, and the move rules use it to break ties and for nothing else.
 * Tone sums of a square: over the pixels of the centre disc of _detect_center_vs_border (piece_detector.py:184-190),
 * (x - w/2)^2 + (y - h/2)^2 <= (min(w, h)/4)^2 with integer divisions (bit 0 of the square's mask; SquareDesc::cnt[0]
 * pixels), of the warped board as the detectors receive it (3 channels, not blurred): the three channel sums (B, G, R)
 * and the pixel count.  Squares of 1 x 1 to CBV_MAX_SQUARE_DIM are legal; a radius of 0 leaves the centre pixel; the sums
 * of a 128 x 128 square stay far below 2^32.
 * Square colour: ROI i = 8 * row + col is dark iff row + col is odd (a1 = row 7, col 0 is dark): tones need the 64 ROIs of
 * a board in that numbering.
 * Classification of one square, all in float64, every multiply, add and divide rounded by itself, in this order:
 *   f[c] = (double)sum[c] / (double)cnt
 *   dW = (f[0]-cW[0])^2 + (f[1]-cW[1])^2 + (f[2]-cW[2])^2, left to right; dB likewise; D likewise from cW - cB,
 *   cW / cB = centroid[colour of the square][0 / 1];  T = (2.0 * margin) * D
 *   white iff dB - dW >= T, otherwise black iff dW - dB >= T, otherwise undecided (so is a square with cnt == 0).
 * That is the sign of the projection onto the axis between the two centroids with a dead zone of `margin` on either side
 * of the midpoint; margin lies in [0, 0.5), 0.125 by default. */
typedef struct { uint32_t sum[3]; uint32_t cnt; } cbv_tone_sums; /* B, G, R */
typedef struct {
    double centroid[2][2][3]; /* [light, dark][white piece, black piece][b, g, r] */
    double margin;
    int32_t calibrated, pad;
} cbv_tone_model;
/* bit i = ROI i; all 64 squares whatever their occupancy: the bits of an empty square mean nothing, AND with the occupancy */
typedef struct { uint64_t white, black; } cbv_tone_result;
typedef struct {
    int32_t samples[2][2];    /* calibration squares per class: [light, dark][white piece, black piece] */
    double D[2];              /* squared distance of the two centroids per square colour */
    uint64_t misclassified;   /* calibration squares the new model gives the other colour (bit = ROI) */
    uint64_t undecided;       /* ... or leaves undecided */
} cbv_tone_report;
/* Tone sums of n ROIs (any table, n <= CBV_MAX_SQUARES) of one 3-channel board in host memory: k_piece_tone on one frame. */
CBV_API int cbv_tone_sums_image(cbv_ctx* ctx, const cbv_host_image* board, const cbv_roi* rois, int n, cbv_tone_sums* out);
/* Host only.  A model from the sums of the 64 squares of one frame and a known position: position[i] = 0 empty, 1 white,
 * 2 black for ROI i.  Each centroid is the mean of f over its class, the squares summed in ROI order and divided by their
 * number.  CBV_ERR_ARG for an empty class, D == 0 of a square colour, an occupied square with cnt == 0 or a margin outside
 * [0, 0.5).  *report (may be NULL) says how the new model classifies its own samples: a calibration that does not is
 * returned, not hidden. */
CBV_API int cbv_tone_calibrate_host(const cbv_tone_sums* sums, const uint8_t* position, double margin, cbv_tone_model* model,
                                    cbv_tone_report* report);
/* Host only.  Squares [0, n) (n <= 64, index = ROI) -> the two words.  CBV_ERR_ARG for an uncalibrated model. */
CBV_API int cbv_tone_classify_host(const cbv_tone_model* model, const cbv_tone_sums* sums, int n, uint64_t* white, uint64_t* black);
/* Tones of a board of a pipeline: with a model every processed frame leaves its sums and its cbv_tone_result (k_piece_tone
 * behind the warp of each chunk, one launch for the sums of all boards and one for their records).  NULL turns them off.
 * CBV_ERR_ARG for an uncalibrated model, CBV_ERR_STATE on a board that has not 64 squares, and for NULL while a session
 * with cfg.tone runs on the board.  A pipeline that never calls this or cbv_pipeline_tone_sums launches and allocates
 * nothing for it. */
CBV_API int cbv_pipeline_set_tones(cbv_pipeline* board, const cbv_tone_model* model);
/* the sums of the 64 squares of a processed slot, with tones on or off (calibration reads them) */
CBV_API int cbv_pipeline_tone_sums(cbv_pipeline* board, int slot, cbv_tone_sums* out);
/* the records of processed slots; CBV_ERR_STATE while tones are off */
CBV_API int cbv_pipeline_tones(cbv_pipeline* board, int slot0, int count, cbv_tone_result* out);
/* cbv_session_walk_events with the frames' tone records (NULL = all undecided); read only with cfg->tone */
CBV_API int cbv_session_walk_tones(const cbv_session_config* cfg, cbv_session_state* state, const cbv_frame_result* results,
                                   const cbv_noise_result* noise, int n, const cbv_session_event* events, int n_events,
                                   int* events_used, cbv_session_radar* radar, const cbv_tone_result* tones, cbv_session_move* move,
                                   int* accepted);

/* ------------------------------------------------------------------ */
/* PieceDetector radius and Hough settings sweep on the device          */
/* ------------------------------------------------------------------ */
/* What calibrate_piece_detector.py shows for a still scene ("Pecas: n/32", the methods, the radii) for many positions of
 * its MinRadius%, MaxRadius% and Hough trackbars at once, on frames a board has already processed.
 * DEFINITION: setting s (a cbv_hough_params) on the frames slot0 .. slot0 + count - 1 is what a fresh reference
 * PieceDetector (history_size 5, min_presence 0.6, circle_threshold 0.6) returns whose min_radius_ratio,
 * max_radius_ratio, hough_param1 and hough_param2 are s (dp too) when detect_all_pieces(squares_i, use_smoothing=True,
 * squares_to_check=<all squares>) is called on the frames in order: every square is processed on every frame, so the raw
 * result of a frame is detect_piece(square) of that frame, the history holds the raw values of the last five frames or
 * fewer, and has_piece is _get_stable_detection (piece_detector.py:111-122).  Only the HoughCircles step depends on the
 * setting; the std < 15 gate, the centre-versus-corner difference and the ring symmetry come from the statistics the
 * board's run left for the slot.  Out of scope: the delta-gated chain per setting (squares_to_check = None keeps the
 * delta gate on, piece_detector.py:387, so the tool's literal loop is the pipeline's own mode and would need a reference
 * plane per setting), and visual_changes. */
typedef struct {              /* one (setting, frame): 56 bytes */
    uint64_t raw_occupied, stable_occupied;             /* as in cbv_frame_result, bit i = roi i */
    uint64_t hough, tower_top, center_diff, symmetry;   /* the raw result's method, as square sets */
    int16_t r_min, r_max;     /* extremes of int(r) over the squares whose method is hough or tower_top, 0 if none */
    uint8_t n_raw, n_stable;  /* popcounts of raw_occupied and stable_occupied */
    uint8_t flags;            /* CBV_PIECE_SWEEP_OVERFLOW */
    uint8_t pad;
} cbv_piece_sweep_record;
#define CBV_PIECE_SWEEP_OVERFLOW 1 /* a HoughCircles candidate list of the frame overflowed: the record may be wrong */
typedef struct {              /* one setting over the call's frames: 56 bytes */
    uint32_t frames;
    uint32_t frames_exact;    /* frames with stable_occupied == expected (0 without `expected`) */
    uint32_t missed;          /* sum of popcount(expected & ~stable_occupied) (0 without `expected`) */
    uint32_t false_pos;       /* sum of popcount(stable_occupied & ~expected) */
    uint32_t n_hough, n_tower_top, n_center_diff, n_symmetry; /* sums of the method sets' popcounts */
    int32_t r_min, r_max;     /* over every (frame, square) with a circle, 0 if none */
    uint32_t n_r;             /* how many of those */
    uint32_t overflow;        /* (frame, square) pairs whose candidate list overflowed */
    uint64_t r_sum;           /* sum of int(r) over them */
} cbv_piece_sweep_summary;
typedef struct { float hough_ms, eval_ms; int32_t param1_distinct, chunk_frames; } cbv_piece_sweep_info;
#define CBV_PIECE_SWEEP_MAX_SETTINGS 65536
/* Any board handle.  Reads the board's gray ring (the PieceDetector's 5 x 5 planes), its square table and the statistics of
 * the slots; writes nothing of the board's, and a pipeline that never calls this launches and allocates nothing for it.
 * Waits for the runs in flight and returns when `records` ([ns][count], setting major; may be NULL) and `summary` ([ns]) are
 * filled; `expected` (may be NULL) = one occupancy set per frame for frames_exact / missed / false_pos; `info` (may be
 * NULL) gets the GPU time of the two kernels (event pairs: k_piece_sweep_hough, k_piece_sweep_eval), the number of distinct
 * param1 values and the chunk used.  Frames are processed in chunks of `chunk_frames` (0 = CBV_SWEEP_DEFAULT_CHUNK, at most
 * CBV_SWEEP_MAX_CHUNK): the call's own device memory is ns x chunk x 64 x 8 bytes of circle choices, ns x 128 bytes of
 * history and summaries, the sorted settings and, with `records`, ns x chunk x 56 bytes of staging, all freed before the call
 * returns.  The result does not depend on the chunk or on the order of the settings.  HoughCircles keeps as many
 * accumulator maxima per square as the pipeline's second pass does (fewer where the sweep's own LDS table needs the room);
 * there is no retry: an overflow sets CBV_PIECE_SWEEP_OVERFLOW and counts in `overflow`.
 * CBV_ERR_STATE: not configured, or a slot that was never run.  CBV_ERR_ARG: null or empty arguments, slots outside the
 * ring, chunk_frames outside 0..CBV_SWEEP_MAX_CHUNK, ns above CBV_PIECE_SWEEP_MAX_SETTINGS, a ratio that is negative or
 * not finite, or dp, param1 or param2 not above 0 (or not finite).  CBV_ERR_UNSUPPORTED: squares that do not fit the
 * kernel's LDS layout, a radius ratio above 1 (the trackbars end at 0.5 and 0.7), or dp above 16.  After any error nothing
 * has changed. */
CBV_API int cbv_pipeline_piece_sweep(cbv_pipeline* board, int slot0, int count, const cbv_hough_params* settings, int ns,
                                     const uint64_t* expected, int chunk_frames, cbv_piece_sweep_record* records,
                                     cbv_piece_sweep_summary* summary, cbv_piece_sweep_info* info);
/* detect_piece's dict of every square for ONE (setting, frame), by the sweep's own HoughCircles kernel with ns = 1 and
 * count = 1: out[n_rois] with has_piece (raw), method, centre, radius, confidence and center_border_diff; changed = 0,
 * should_process = evaluated = 1.  Errors as cbv_pipeline_piece_sweep; CBV_ERR_UNSUPPORTED (with `out` filled) when a
 * candidate list overflowed. */
CBV_API int cbv_pipeline_piece_detail(cbv_pipeline* board, int slot, const cbv_hough_params* setting, cbv_piece_result* out);
/* The host twin of k_piece_sweep_eval, no GPU: stats[frames][n] (n <= CBV_MAX_SQUARES), ws[n] / hs[n] the squares' sizes,
 * choices[ns][frames][n] the circle of every (setting, frame, square) as k_piece_sweep_hough leaves it, 8 bytes each:
 * kind (0 none, 1 hough, 2 tower_top), flags (CBV_HOUGH_OVERFLOW), int16 int(r), int16 int(cx), int16 int(cy).  The frames
 * are walked in order from an empty history.  expected[frames] may be NULL; records [ns][frames] may be NULL;
 * summary [ns].  0, or CBV_ERR_ARG. */
CBV_API int cbv_piece_sweep_eval_host(const cbv_sq_stats* stats, const int32_t* ws, const int32_t* hs, int n, int frames,
                                      const void* choices, int ns, const uint64_t* expected, cbv_piece_sweep_record* records,
                                      cbv_piece_sweep_summary* summary);

/* ------------------------------------------------------------------ */
/* Colour profile sweep on the device                                   */
/* ------------------------------------------------------------------ */
/* What calibrate_colors.py's eight trackbars (hue_shift, sat_scale, val_scale, contrast, brightness, radical_mode,
 * target_hue, hue_window) do to the PieceDetector, for many positions at once, on frames in the ring.
 * DEFINITION: profile c on the frames slot0 .. slot0 + count - 1 is what a fresh reference PieceDetector (history_size 5,
 * min_presence 0.6, circle_threshold 0.6; radii and Hough parameters: the board's configured ones) returns when
 * detect_all_pieces(squares_i, use_smoothing=True, squares_to_check=<all squares>) is called on the frames in order with
 * squares_i = split_board(rotate?(warp_image(ImageEnhancer(profile = c).apply_color_profile(frame_i)))), the board's corners,
 * rotation and grid.  That is what a board configured with CBV_SKIP_ENHANCE_PROFILE, profile c, use_hough = 2 and every
 * square checked reports.  The result is in cbv_pipeline_piece_sweep's terms: records [np][count] (profile major; may be
 * NULL), summary [np], `expected` (may be NULL), CBV_PIECE_SWEEP_OVERFLOW.  An entry with enabled = 0 is the frame as it is.
 * Any board handle.  Reads the BGR frame ring (the frames as uploaded, before any enhancement, whatever the pipeline's
 * mode), or, in the raw mode of CBV_SKIP_ENHANCE_PROFILE_RAW, the raw ring through k_warp_raw_profile (the same scratch
 * layout, stages, records, summaries and `info`; the result is that of the converted frames), and the board's geometry, square table, masks and Hough settings (cfg.hough, whether or not use_hough is set);
 * writes nothing of the board's, does not need the slots to have been run, and a pipeline that never calls it launches
 * and allocates nothing for it.  Waits for the runs in flight.  Per chunk of profiles x chunk of frames: k_warp_profile
 * into scratch boards [profile][frame], the fused gray + 5 x 5 blur + statistics kernel on them, the sweep's HoughCircles
 * kernel (k_piece_sweep_hough, one setting) on every square the std < 15 gate lets through, k_piece_sweep_eval with the
 * statistics of each profile; history and summaries stay on the device from chunk to chunk.  `info` (may be NULL) gets the
 * four stages' GPU time (event pairs) and the chunk sizes used.  chunk_frames: 0 = CBV_SWEEP_DEFAULT_CHUNK, at most
 * CBV_SWEEP_MAX_CHUNK; the profiles of a chunk are as many as keep the scratch below 256 MiB (and the launch's grid inside
 * its limits).  Device memory of the call, with P = profiles per chunk, F = chunk_frames, S = board_size:
 * P x F x (3 S^2 + the squares' gray planes + n_rois x 72 bytes of statistics + 64 x 8 bytes of circle choices),
 * P x 6.5 KB of tables, np x (256 bytes of history + 56 of summary) and, with `records`, P x F x 56 bytes of staging (and as
 * much pinned host memory), all freed before the call returns.  The result does not depend on the chunk sizes, on the order of the profiles
 * or on duplicates.
 * CBV_ERR_STATE: not configured.  CBV_ERR_ARG: null or empty arguments, no summary, slots outside the ring, chunk_frames
 * outside 0..CBV_SWEEP_MAX_CHUNK, np above CBV_COLOR_SWEEP_MAX_PROFILES, a profile field that is not finite.
 * CBV_ERR_UNSUPPORTED: the raw mode of skip_enhance = 1 (there is no BGR ring and no profile kernel; configure
 * CBV_SKIP_ENHANCE_PROFILE_RAW with a disabled profile instead: that runs the plain raw warp and can sweep), or squares that do not fit the HoughCircles kernel's LDS layout.
 * After any error nothing has changed. */
typedef struct { float warp_ms, squares_ms, hough_ms, eval_ms; int32_t chunk_frames, chunk_profiles; } cbv_color_sweep_info;
#define CBV_COLOR_SWEEP_MAX_PROFILES 65536
CBV_API int cbv_pipeline_color_sweep(cbv_pipeline* board, int slot0, int count, const cbv_color_profile* profiles, int np,
                                     const uint64_t* expected, int chunk_frames, cbv_piece_sweep_record* records,
                                     cbv_piece_sweep_summary* summary, cbv_color_sweep_info* info);

/* ---------------------------------------------------------------------------
 * Lens distortion corrected in the warp's gather
 * ---------------------------------------------------------------------------
 * OpenCV's five-coefficient Brown-Conrady model: the camera_matrix (fx, fy, cx, cy) and dist_coeffs (k1, k2, p1, p2, k3)
 * that cv2.calibrateCamera writes.  The new camera matrix equals the camera matrix and there is no rectification.  The
 * homography of a warp then lives in IDEAL (pinhole) pixel coordinates, and the lens says where the delivered frame shows
 * an ideal position.  A destination pixel (dx, dy) gets its ideal position as the lens-free warp computes it, in the
 * block-origin form: bx = (dx / bw0) * bw0, x1 = dx - bx, X0, Y0, W0 evaluated at (bx, dy), W = W0 + M[6] * x1 (M = the
 * inverse of the matrix passed).  Then, in float64, every operation rounded once and never fused, in this order:
 *     Wi = W != 0 ? 1.0 / W : 0.0
 *     u  = (X0 + M[0]*x1) * Wi          v  = (Y0 + M[3]*x1) * Wi
 *     x  = (u - cx) / fx                y  = (v - cy) / fy
 *     r2 = x*x + y*y
 *     kr = 1.0 + ((k3*r2 + k2)*r2 + k1)*r2
 *     xy2 = 2.0*x*y
 *     xd = x*kr + p1*xy2 + p2*(r2 + 2.0*x*x)
 *     yd = y*kr + p1*(r2 + 2.0*y*y) + p2*xy2
 *     fX = (xd*fx + cx) * 32.0          fY = (yd*fy + cy) * 32.0
 * and from there the warp's own step: clamp to the int32 range, round to nearest even, split into sx, sy and the 1/32
 * fractions, four taps (BGR 0 for a tap outside the frame), the 15-bit fixed-point blend, the optional rotation by 180
 * degrees.  One interpolation per pixel, for every source format.  If fX or fY is not a number, both become the lowest
 * int32: the pixel lies outside the frame, reads nothing and is 0.  An infinite coordinate is clamped and is outside too.
 * In exact arithmetic this is cv2.remap(frame, map, INTER_LINEAR, BORDER_CONSTANT 0) with the map of
 * cv2.initUndistortRectifyMap(K, dist, I, K) composed with the inverse homography; it is not pinned against a cv2 build,
 * which keeps its maps in float32.
 * enabled = 0 (or a null lens) is the lens-free warp, bit for bit.  A lens whose coefficients are all zero is NOT promised
 * to equal the lens-free warp: ((u - cx) / fx) * fx + cx rounds differently from u.
 * Refused with CBV_ERR_ARG and nothing changed: a field that is not finite, fx <= 0 or fy <= 0. */
typedef struct { int32_t enabled, pad; double fx, fy, cx, cy, k1, k2, p1, p2, k3; } cbv_lens;
/* The forward model on n points (x, y pairs): ideal pixel positions -> positions in the frame as delivered.  Host only. */
CBV_API int cbv_lens_distort_points(const cbv_lens* lens, const double* xy_in, int n, double* xy_out);
/* The inverse, for the corner points a person clicks in the delivered frame: cv2.undistortPoints' fixed-point iteration,
 * start at x = xd, exactly 40 rounds of x = (xd - tangential(x, y)) / kr(x, y) (the same for y), back with * fx + cx.  The
 * count is fixed: the result is a function of the input alone.  Host only.  Both ignore `enabled`. */
CBV_API int cbv_lens_undistort_points(const cbv_lens* lens, const double* xy_in, int n, double* xy_out);
/* The host twin of the kernels' coordinates: XY[dh][dw][2] = the rounded 1/32-px X, Y of every destination pixel of a
 * dw x dh warp with the inverse homography M9 (NOT inverted here), before the split into sx, sy and the fractions. */
CBV_API int cbv_lens_warp_coords(const cbv_lens* lens, const double* M9, int dw, int dh, int32_t* XY);
/* The source pixels a dw x dh warp can sample in a w x h frame, [x0, x1) x [y0, y1): every border pixel of the destination
 * through the full map, the bounding box with 4 pixels of margin, clipped.  Returns 1 with rect4 filled, 0 when there is no
 * usable footprint (callers take the whole frame).  lens may be null: the four corners, 3 pixels. */
CBV_API int cbv_lens_warp_footprint(const cbv_lens* lens, const double* Minv9, int dw, int dh, int w, int h, int32_t* rect4);
/* One frame through the lens, host in, host out: raw->fmt = any CBV_FMT_*, CBV_FMT_BGR included (plane0 / stride0 = the
 * BGR rows); profile may be null; = the format's conversion, then cbv_apply_color_profile when the profile is enabled,
 * then the warp defined above on that frame, byte for byte, in one kernel.  M9 is the matrix as cbv_warp_perspective takes
 * it (board <- ideal frame).  A null or disabled lens is the lens-free call of the format. */
CBV_API int cbv_warp_lens(cbv_ctx* ctx, const cbv_raw_frame* raw, int w, int h, const cbv_color_profile* profile, const cbv_lens* lens,
                          const double* M9, int dw, int dh, int rot180, uint8_t* out, int out_stride);
/* ... and one Motion-JPEG frame, as cbv_warp_jpeg takes it */
CBV_API int cbv_warp_jpeg_lens(cbv_ctx* ctx, const uint8_t* data, size_t n, const cbv_color_profile* profile, const cbv_lens* lens, const double* M9,
                               int dw, int dh, int rot180, uint8_t* out, int out_stride, int32_t* status);
/* The camera's lens of a pipeline, shared by every board: every warp of a board of the pipeline goes through it
 * (cbv_pipeline_run in all modes, the colour sweep's scratch warps), and enhance_region's footprint follows it.  The
 * pipeline's own handle only: a board's handle is CBV_ERR_STATE.  Allowed between runs, waits for the runs in flight.  Null
 * or enabled = 0 turns it off.  The boards' matrices are then ideal-coordinate ones (cbv_lens_undistort_points on the
 * clicked corners before cbv_get_perspective_transform). */
CBV_API int cbv_pipeline_set_lens(cbv_pipeline* p, const cbv_lens* lens);

#ifdef __cplusplus
}
#endif
#endif /* CBV_H */
