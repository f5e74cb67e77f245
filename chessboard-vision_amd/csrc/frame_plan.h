// Where a pipeline's frames live ("Where the frames live"): the settings that decide it and ONE function from
// them to the plan of the frame store: what the warp reads, which rings exist and how large their slots are, and the
// dimensions of the Motion-JPEG decode's scratch.  cbv_pipeline_frames.cpp makes the buffers match a plan; everything else
// asks the plan.  Host code that needs neither HIP nor a GPU (tools/frame_plan_host.cpp prints it cell by cell).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cbv.h"
#include "jpeg_core.h"

// the bit fields of a format id (include/cbv.h)
static constexpr bool raw_fmt_bayer8(int fmt)
{
    return fmt == CBV_FMT_BAYER_RGGB || fmt == CBV_FMT_BAYER_BGGR || fmt == CBV_FMT_BAYER_GRBG || fmt == CBV_FMT_BAYER_GBRG;
}
// the sample encoding of a Bayer id (0: bytes; CBV_BAYER_16, _10P, _12P >> 12) and the Bayer ids of every assigned encoding
enum { BAYER_ENC_8 = 0, BAYER_ENC_16 = CBV_BAYER_16 >> 12, BAYER_ENC_10P = CBV_BAYER_10P >> 12, BAYER_ENC_12P = CBV_BAYER_12P >> 12 };
static constexpr int raw_fmt_enc(int fmt) { return (fmt & CBV_BAYER_ENC_MASK) >> 12; }
static constexpr bool raw_fmt_bayer(int fmt) { return raw_fmt_bayer8(fmt & ~CBV_BAYER_ENC_MASK) && raw_fmt_enc(fmt) <= BAYER_ENC_12P; }
// bytes of a row of w samples of a Bayer id (10P: w % 4 == 0)
static constexpr int bayer_row_bytes(int fmt, int w)
{
    return raw_fmt_enc(fmt) == BAYER_ENC_16 ? 2 * w : raw_fmt_enc(fmt) == BAYER_ENC_10P ? w / 4 * 5 : raw_fmt_enc(fmt) == BAYER_ENC_12P ? w / 2 * 3 : w;
}
// The tables of a developed mosaic (include/cbv.h): the bits an encoding's tables may have, its default's (0: the 8-bit ids
// have no table by default), and the neutral table, v * 255 / M rounded half up, of one colour
static constexpr bool bayer_bits_ok(int fmt, int bits)
{
    return raw_fmt_enc(fmt) == BAYER_ENC_16 ? (bits == 10 || bits == 12 || bits == 14 || bits == 16)
                                            : bits == (raw_fmt_enc(fmt) == BAYER_ENC_10P ? 10 : raw_fmt_enc(fmt) == BAYER_ENC_12P ? 12 : 8);
}
static constexpr int bayer_default_bits(int fmt)
{
    return raw_fmt_enc(fmt) == BAYER_ENC_16 ? 16 : raw_fmt_enc(fmt) == BAYER_ENC_10P ? 10 : raw_fmt_enc(fmt) == BAYER_ENC_12P ? 12 : 0;
}
static inline void bayer_neutral_table(int bits, uint8_t* t /* [1 << bits] */)
{
    const uint32_t M = (1u << bits) - 1;
    for (uint32_t v = 0; v <= M; v++) t[v] = (uint8_t)((510u * v + M) / (2u * M));
}
static inline bool raw_fmt_420(int fmt) { return (fmt & 15) == CBV_FMT_NV12; }
// the YUV families (of a known layout)
static constexpr bool raw_fmt_yuv(int fmt) { return (fmt & 15) == CBV_FMT_NV12 || (fmt & 15) == CBV_FMT_YUYV; }
// An id as a caller passes it = layout | colour space (CBV_CS_*, YUV only).  It is split once, where it enters the library;
// everything below sees the layout, and the colour space (0 .. 3, the row of cbv_yuv.h's table) travels beside it.
static constexpr int raw_fmt_layout(int fmt) { return fmt & ~CBV_CS_MASK; }
static constexpr int raw_fmt_cs(int fmt) { return (fmt & CBV_CS_MASK) / CBV_CS_FULL; }
// tightly packed raw frames, planes back to back (the ingest rings round each frame to 256 bytes); fmt BGR: tight_geom's bytes
static inline size_t raw_frame_bytes(int fmt, int w, int h)
{
    if (raw_fmt_bayer(fmt)) return (size_t)bayer_row_bytes(fmt, w) * h;
    return raw_fmt_420(fmt) ? (size_t)w * h * 3 / 2 : (size_t)w * h * (fmt == CBV_FMT_BGR ? 3 : 2);
}

enum { JPEG_PIECE_WORDS = 9 }; // four states (this round's and the last one's exit, the entry, round 0's exit) and a block count
enum { JPEG_SEG_WORDS = 3 };   // a segment's first piece, its last written piece, one past its last block with a decoded DC symbol
// the piece path's scratch per frame, in u32 words, for `pieces` pieces and (in segments mode) `intervals` restart intervals
inline size_t jpeg_piece_words(size_t pieces, int segments) { return pieces * (size_t)(JPEG_PIECE_WORDS + (segments ? 1 : 0)); }
inline size_t jpeg_seg_words(size_t intervals) { return intervals * JPEG_SEG_WORDS + 1; }

// the piece size a mode and a piece_bytes argument mean (0: every frame by restart interval), and whether frames with DRI
// go the piece path too (CBV_JPEG_ENTROPY_SEGMENTS); or CBV_ERR_ARG and why in `msg`
static inline int jpeg_piece_size(int mode, uint32_t piece_bytes, uint32_t* S, int* segments, char* msg, size_t nmsg)
{
    if (mode != CBV_JPEG_ENTROPY_AUTO && mode != CBV_JPEG_ENTROPY_INTERVAL && mode != CBV_JPEG_ENTROPY_PIECES && mode != CBV_JPEG_ENTROPY_SEGMENTS) {
        snprintf(msg, nmsg, "entropy mode %d", mode);
        return CBV_ERR_ARG;
    }
    if (piece_bytes && (piece_bytes < 4 || (piece_bytes & 3u) || piece_bytes > (1u << 24))) {
        snprintf(msg, nmsg, "pieces of %u bytes (a multiple of 4, from 4 to 2^24, or 0 for the default)", piece_bytes);
        return CBV_ERR_ARG;
    }
    *S = mode == CBV_JPEG_ENTROPY_INTERVAL ? 0u : piece_bytes ? piece_bytes : (uint32_t)JP_PIECE_DEFAULT;
    *segments = mode == CBV_JPEG_ENTROPY_SEGMENTS;
    return CBV_OK;
}

static inline bool jpeg_planes_mode_ok(int mode) { return mode >= CBV_JPEG_PLANES_OFF && mode <= CBV_JPEG_PLANES_444; }
// plane_total of a w x h frame in a sampling (jpeg_parse_header's, whole MCUs); the samplings are numbered as the planes
// modes that admit them: CBV_JPEG_PLANES_<X> admits those up to X
static inline size_t jpeg_plane_elems(int w, int h, int sampling)
{
    const size_t hs = sampling == CBV_JPEG_PLANES_420 || sampling == CBV_JPEG_PLANES_422 ? 2 : 1, vs = sampling == CBV_JPEG_PLANES_420 ? 2 : 1;
    const size_t mcux = ((size_t)w + 8 * hs - 1) / (8 * hs), mcuy = ((size_t)h + 8 * vs - 1) / (8 * vs);
    return mcux * mcuy * 64 * (sampling == CBV_JPEG_PLANES_GRAY ? 1 : hs * vs + 2);
}
// cbv_jpeg_plane_slot_bytes: the largest admitted sampling's planes, rounded to 256; 0 for OFF, an unknown mode or a bad size
static inline size_t jpeg_plane_slot_bytes(int w, int h, int mode)
{
    if (w < 1 || h < 1 || !jpeg_planes_mode_ok(mode) || mode == CBV_JPEG_PLANES_OFF) return 0;
    size_t most = 0;
    for (int s = CBV_JPEG_PLANES_GRAY; s <= mode; s++) most = jpeg_plane_elems(w, h, s) > most ? jpeg_plane_elems(w, h, s) : most;
    return (most + 255) & ~(size_t)255;
}
static inline size_t jpeg_default_slot_bytes(int w, int h) { return (((size_t)w * h + 1) / 2 + 255) & ~(size_t)255; }

// cfg.skip_enhance as the frame store sees it: enhancement on, skip_enhance = 1, CBV_SKIP_ENHANCE_PROFILE, .._PROFILE_RAW
enum FrameKind { FRAMES_ENHANCE = 0, FRAMES_SKIP, FRAMES_PROFILE, FRAMES_PROFILE_RAW };
static inline FrameKind frame_kind(int skip_enhance)
{
    return !skip_enhance ? FRAMES_ENHANCE : skip_enhance == CBV_SKIP_ENHANCE_PROFILE ? FRAMES_PROFILE : skip_enhance == CBV_SKIP_ENHANCE_PROFILE_RAW ? FRAMES_PROFILE_RAW : FRAMES_SKIP;
}
// what the warp (or the enhancement) reads: the BGR ring, the raw ring of a YUV or Bayer format, the plane ring of Motion-JPEG
enum FrameSource { FRAMES_BGR = 0, FRAMES_RAW, FRAMES_PLANES };

struct FrameSettings {
    int kind = FRAMES_ENHANCE;
    int fmt = CBV_FMT_BGR;                // cbv_pipeline_set_input_format: the layout
    int cs = 0;                           // ... and the colour space of a YUV layout (raw_fmt_cs); the plan does not depend on it
    int planes = CBV_JPEG_PLANES_OFF;     // cbv_pipeline_set_jpeg_planes; means something with CBV_FMT_MJPEG only
    int w = 0, h = 0, max_frames = 0;
    size_t jpeg_slot_bytes = 0;           // cbv_pipeline_set_jpeg_slot_bytes; 0: the default
    int entropy = CBV_JPEG_ENTROPY_AUTO;  // cbv_pipeline_set_jpeg_entropy
    uint32_t piece_bytes = 0;             // 0: the default
    int depth = CBV_JPEG_DEPTH_DEFAULT;   // cbv_pipeline_set_jpeg_depth
};

struct FramePlan {
    int source = FRAMES_BGR;
    bool bgr_ring = false;   // false only where nothing reads or writes BGR frames
    size_t slot_bytes = 0;   // between the slots of the two ingest rings (which are made on first use)
    int plane_mode = CBV_JPEG_PLANES_OFF; // the plane ring: with Motion-JPEG in a planes mode, whatever the configuration
    size_t plane_slot = 0;
    // the piece path of every Motion-JPEG decode of the pipeline (cbv_pipeline_upload_jpeg's too)
    uint32_t piece_bytes = 0; // 0: every frame by restart interval
    int segments = 0;
    // the decode scratch of a submit, with Motion-JPEG only (depth 0: none): `depth` frames of the pipeline's size (the
    // coefficients, 2 bytes a sample, and, unless the planes go to the plane ring, the planes, 1 byte a sample) in the sampling
    // that needs most (4:4:4 padded to the 16 x 16 MCUs of 4:2:0) and a restart interval of one MCU; a frame's pieces are at
    // most ceil(slot bytes / S), and with segments max_int more (every interval's last piece may be a short one, an empty
    // interval is one piece)
    int depth = 0;
    bool own_planes = false;
    size_t frame_elems = 0, max_int = 0;
    uint32_t piece_cap = 0;
    size_t piece_words = 0, seg_words = 0; // u32 words per frame
    bool raw() const { return source != FRAMES_BGR; }
    bool same_scratch(const FramePlan& o) const
    {
        return depth == o.depth && own_planes == o.own_planes && piece_cap == o.piece_cap && piece_words == o.piece_words && seg_words == o.seg_words;
    }
};

// THE derivation; CBV_ERR_ARG and why in `msg` for an entropy setting jpeg_piece_size refuses or more pieces than a u32 counts
static inline int frame_plan(const FrameSettings& s, FramePlan* out, char* msg, size_t nmsg)
{
    FramePlan p;
    const bool mjpeg = s.fmt == CBV_FMT_MJPEG, j1 = mjpeg && s.planes != CBV_JPEG_PLANES_OFF;
    const bool raw_fmt = (s.fmt != CBV_FMT_BGR && !mjpeg) || j1;                     // YUV, Bayer, or JPEG planes
    const bool raw_kind = s.kind == FRAMES_SKIP || s.kind == FRAMES_PROFILE_RAW;     // a raw format's frames stay raw
    p.source = !(raw_kind && raw_fmt) ? FRAMES_BGR : j1 ? FRAMES_PLANES : FRAMES_RAW;
    // skip_enhance = 1 keeps an idle BGR ring beside the raw ring, as it always did; the plane ring replaces it in both
    p.bgr_ring = !(p.source == FRAMES_PLANES || (p.source == FRAMES_RAW && s.kind == FRAMES_PROFILE_RAW));
    p.slot_bytes = mjpeg ? (s.jpeg_slot_bytes ? s.jpeg_slot_bytes : jpeg_default_slot_bytes(s.w, s.h)) : (raw_frame_bytes(s.fmt, s.w, s.h) + 255) & ~(size_t)255;
    p.plane_mode = j1 ? s.planes : CBV_JPEG_PLANES_OFF;
    p.plane_slot = jpeg_plane_slot_bytes(s.w, s.h, p.plane_mode);
    const int rc = jpeg_piece_size(s.entropy, s.piece_bytes, &p.piece_bytes, &p.segments, msg, nmsg);
    if (rc) return rc;
    if (mjpeg) {
        const size_t pw = ((size_t)s.w + 15) & ~(size_t)15, ph = ((size_t)s.h + 15) & ~(size_t)15;
        p.depth = s.depth;
        p.own_planes = p.source != FRAMES_PLANES;
        p.frame_elems = 3 * pw * ph;
        p.max_int = ((size_t)s.w + 7) / 8 * (((size_t)s.h + 7) / 8);
        const size_t S = p.piece_bytes, cap = S ? (p.slot_bytes + S - 1) / S + (p.segments ? p.max_int : 0) : 0;
        if (cap > 0xFFFFFFFFu) {
            snprintf(msg, nmsg, "%zu pieces per frame", cap);
            return CBV_ERR_ARG;
        }
        p.piece_cap = (uint32_t)cap;
        p.piece_words = jpeg_piece_words(cap, p.segments);
        p.seg_words = p.segments ? jpeg_seg_words(p.max_int) : 0;
    }
    *out = p;
    return CBV_OK;
}
