// Motion-JPEG as a stage (include/cbv.h): the header probe, the host twin, the single-frame GPU decode and the warp from a
// stream's planes.  The host reads the header only; the entropy data is the kernels' (k_jpeg.hip).  The pipeline's ingest of
// the format is cbv_pipeline_jpeg.cpp.
#include <algorithm>

#include "cbv_pipeline.h"

#include "jpeg_core.h"

static int jpeg_header(cbv_ctx* ctx, const char* who, const uint8_t* data, size_t n, JpegDesc* D, JpegTables* T)
{
    char msg[200];
    const int rc = jpeg_parse_header(data, n, D, T, msg, sizeof(msg));
    if (rc) return cbv_fail(ctx, rc, "%s: %s", who, msg);
    return CBV_OK;
}

extern "C" int cbv_jpeg_probe(const uint8_t* data, size_t n, cbv_jpeg_info* info)
{
    if (!data || !info) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_jpeg_probe: null argument");
    JpegDesc D;
    JpegTables T;
    RC(jpeg_header(nullptr, "cbv_jpeg_probe", data, n, &D, &T));
    memset(info, 0, sizeof(*info));
    info->w = D.w;
    info->h = D.h;
    info->components = D.ncomp;
    info->hs = D.hs;
    info->vs = D.vs;
    info->restart_interval = D.dri;
    info->intervals = D.nint;
    info->std_tables = D.std_tables;
    info->entropy_offset = D.ent_off;
    info->entropy_length = D.ent_len;
    info->plane_elems = D.plane_total;
    for (int c = 0; c < D.ncomp; c++) {
        info->blocks_w[c] = D.bw[c];
        info->blocks_h[c] = D.bh[c];
    }
    return CBV_OK;
}

// frame_plan.h's jpeg_piece_size with its refusal as the context's error
static int jpeg_piece_size(cbv_ctx* ctx, const char* who, int mode, uint32_t piece_bytes, u32* S, int* segments)
{
    char msg[120];
    const int rc = jpeg_piece_size(mode, piece_bytes, S, segments, msg, sizeof(msg));
    return rc ? cbv_fail(ctx, rc, "%s: %s", who, msg) : CBV_OK;
}

extern "C" int cbv_jpeg_decode_host_ex(const uint8_t* data, size_t n, uint8_t* bgr, int stride, int16_t* coef, uint8_t* planes, int32_t* status,
                                       int mode, uint32_t piece_bytes, cbv_jpeg_decode_stats* stats)
{
    const char* who = "cbv_jpeg_decode_host";
    if (!data || !bgr || !status) return cbv_fail(nullptr, CBV_ERR_ARG, "%s: null argument", who);
    u32 S;
    int segments;
    RC(jpeg_piece_size(nullptr, who, mode, piece_bytes, &S, &segments));
    JpegDesc D;
    JpegTables T;
    RC(jpeg_header(nullptr, who, data, n, &D, &T));
    if (stride < D.w * 3) return cbv_fail(nullptr, CBV_ERR_ARG, "%s: stride %d below the %d bytes of a row", who, stride, D.w * 3);
    std::vector<int16_t> cbuf;
    std::vector<uint8_t> pbuf;
    if (!coef) {
        cbuf.resize(D.plane_total);
        coef = cbuf.data();
    }
    if (!planes) {
        pbuf.resize(D.plane_total);
        planes = pbuf.data();
    }
    int st = 0;
    JpegPieceStats ps;
    jpeg_decode_host(data, D, T, coef, planes, bgr, (size_t)stride, &st, S, &ps, segments != 0);
    *status = st;
    if (stats) {
        stats->pieces = ps.pieces;
        stats->rounds = ps.rounds;
        stats->settled_round0 = ps.settled;
    }
    return CBV_OK;
}

extern "C" int cbv_jpeg_decode_host(const uint8_t* data, size_t n, uint8_t* bgr, int stride, int16_t* coef, uint8_t* planes, int32_t* status)
{
    return cbv_jpeg_decode_host_ex(data, n, bgr, stride, coef, planes, status, CBV_JPEG_ENTROPY_AUTO, 0, nullptr);
}

// One stream through the kernels on ctx->stream, with the context's scratch: the stream in ctx->in, coefficients in
// ctx->a, planes in ctx->b, the small block (descriptor, tables, interval prefix, counters, marker positions, and the piece
// path's states and segment table, sized from the stream's length and its intervals) in ctx->small.  S = the piece size, 0:
// by restart interval; segments: a frame with DRI goes the piece path too.
// bgr_dev null: the BGR frame goes to ctx->c, tightly packed.  planes_dev: the planes go there instead of ctx->b; no_bgr: the
// decode stops at the planes.  ctx->b keeps 256 bytes behind the planes (the slack warp_src_jpeg asks for).  Nothing is
// waited for; *B tells where everything lies.
int jpeg_single_dev(cbv_ctx* ctx, const uint8_t* data, size_t n, JpegDesc& D, const JpegTables& T, u32 S, int segments, u8* bgr_dev, Geom g, JpegBatch* Bout,
                    u8* planes_dev, bool no_bgr)
{
    const size_t o_desc = 0, o_tab = (sizeof(JpegDesc) + 255) & ~(size_t)255, o_ioff = (o_tab + sizeof(JpegTables) + 255) & ~(size_t)255;
    const size_t o_nfound = o_ioff + 16, o_status = o_ioff + 32, o_stats = o_ioff + 48, o_mpos = o_ioff + 64;
    const size_t head = o_mpos; // what the host fills
    segments = segments && S;
    const int pieces = S && (!D.dri || segments);
    const size_t o_pieces = (o_mpos + (size_t)D.nint * sizeof(u32) + 255) & ~(size_t)255;
    // the intervals' pieces: sum ceil(len_j / S) <= ceil(ent_len / S) + intervals, an empty interval counted as one piece
    const size_t piece_cap = pieces ? (size_t)jpeg_piece_count(D, S) + (segments && D.dri ? (size_t)D.nint : 0) : 0;
    const size_t piece_words = jpeg_piece_words(piece_cap, segments);
    const size_t o_segs = (o_pieces + piece_words * sizeof(u32) + 255) & ~(size_t)255;
    const size_t seg_words = segments ? jpeg_seg_words((size_t)D.nint) : 0;
    RC(dev_ensure(ctx, &ctx->small, o_segs + seg_words * sizeof(u32)));
    ctx->small.tag = 0; // (not the enhancement chain's layout any more)
    RC(dev_ensure(ctx, &ctx->in, n + 256));
    RC(dev_ensure(ctx, &ctx->a, (size_t)D.plane_total * sizeof(int16_t)));
    if (!planes_dev) RC(dev_ensure(ctx, &ctx->b, (size_t)D.plane_total + 256));
    if (!bgr_dev && !no_bgr) {
        RC(dev_ensure(ctx, &ctx->c, g.frame_stride));
        bgr_dev = (u8*)ctx->c.p;
    }
    u8* hs;
    RC(ctx_hstage(ctx, head, &hs));
    memset(hs, 0, head);
    D.table_set = 0;
    memcpy(hs + o_desc, &D, sizeof(D));
    memcpy(hs + o_tab, &T, sizeof(T));
    const u32 ioff[2] = {0u, (u32)D.nint};
    memcpy(hs + o_ioff, ioff, sizeof(ioff));
    u8* sm = (u8*)ctx->small.p;
    CBV_HIP(ctx, hipMemcpyAsync(sm, hs, head, hipMemcpyHostToDevice, ctx->stream));
    CBV_HIP(ctx, hipMemcpyAsync(ctx->in.p, data, n, hipMemcpyHostToDevice, ctx->stream));
    JpegBatch B;
    B.data = (const u8*)ctx->in.p;
    B.data_stride = 0;
    B.descs = (const JpegDesc*)(sm + o_desc);
    B.tables = (const JpegTables*)(sm + o_tab);
    B.ioff = (const u32*)(sm + o_ioff);
    B.mpos = (u32*)(sm + o_mpos);
    B.nfound = (int*)(sm + o_nfound);
    B.status = (int*)(sm + o_status);
    B.coef = (int16_t*)ctx->a.p;
    B.coef_stride = D.plane_total;
    B.planes = planes_dev ? planes_dev : (u8*)ctx->b.p;
    B.plane_stride = D.plane_total;
    B.bgr = no_bgr ? nullptr : bgr_dev;
    B.bgr_stride = g.stride;
    B.bgr_frame_stride = g.frame_stride;
    B.nframes = 1;
    B.piece_bytes = S;
    B.pieces = (u32*)(sm + o_pieces);
    B.piece_stride = piece_words;
    B.piece_cap = (u32)piece_cap;
    B.segments = segments;
    B.segs = (u32*)(sm + o_segs);
    B.seg_stride = seg_words;
    B.stats = (u32*)(sm + o_stats);
    *Bout = B;
    return launch_jpeg_decode(ctx, B, (u32)D.nint, D.dri != 0, pieces, D.plane_total / 64u, D.w, D.h);
}

extern "C" int cbv_jpeg_decode_ex(cbv_ctx* ctx, const uint8_t* data, size_t n, uint8_t* bgr, int stride, int16_t* coef, uint8_t* planes,
                                  int32_t* status, int mode, uint32_t piece_bytes, cbv_jpeg_decode_stats* stats)
{
    const char* who = "cbv_jpeg_decode";
    if (!ctx) return cbv_fail(nullptr, CBV_ERR_ARG, "%s: ctx is null", who);
    if (!data || !bgr || !status) return cbv_fail(ctx, CBV_ERR_ARG, "%s: null argument", who);
    u32 S;
    int segments;
    RC(jpeg_piece_size(ctx, who, mode, piece_bytes, &S, &segments));
    JpegDesc D;
    JpegTables T;
    RC(jpeg_header(ctx, who, data, n, &D, &T));
    if (stride < D.w * 3) return cbv_fail(ctx, CBV_ERR_ARG, "%s: stride %d below the %d bytes of a row", who, stride, D.w * 3);
    if (D.h > 65535) return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "%s: %d rows", who, D.h);
    CBV_ENTER(ctx);
    const Geom g = tight_geom(D.w, D.h);
    JpegBatch B;
    RC(jpeg_single_dev(ctx, data, n, D, T, S, segments, nullptr, g, &B));
    int st = 0;
    u32 ps[3] = {0, 0, 0};
    CBV_HIP(ctx, hipMemcpyAsync(&st, B.status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (stats) CBV_HIP(ctx, hipMemcpyAsync(ps, B.stats, sizeof(ps), hipMemcpyDeviceToHost, ctx->stream));
    if (coef) CBV_HIP(ctx, hipMemcpyAsync(coef, B.coef, (size_t)D.plane_total * sizeof(int16_t), hipMemcpyDeviceToHost, ctx->stream));
    if (planes) CBV_HIP(ctx, hipMemcpyAsync(planes, B.planes, D.plane_total, hipMemcpyDeviceToHost, ctx->stream));
    if (stride == g.stride) CBV_HIP(ctx, hipMemcpyAsync(bgr, B.bgr, (size_t)g.stride * D.h, hipMemcpyDeviceToHost, ctx->stream));
    else CBV_HIP(ctx, hipMemcpy2DAsync(bgr, stride, B.bgr, g.stride, g.stride, D.h, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *status = st;
    if (stats) {
        stats->pieces = ps[0];
        stats->rounds = ps[1];
        stats->settled_round0 = ps[2];
    }
    return CBV_OK;
}

extern "C" int cbv_jpeg_decode(cbv_ctx* ctx, const uint8_t* data, size_t n, uint8_t* bgr, int stride, int16_t* coef, uint8_t* planes,
                               int32_t* status)
{
    return cbv_jpeg_decode_ex(ctx, data, n, bgr, stride, coef, planes, status, CBV_JPEG_ENTROPY_AUTO, 0, nullptr);
}

extern "C" size_t cbv_jpeg_plane_slot_bytes(int w, int h, int mode) { return jpeg_plane_slot_bytes(w, h, mode); }

// cbv_warp_jpeg, and with a lens cbv_warp_jpeg_lens: the lens's table of one entry lies behind the call's profile table
static int warp_jpeg_call(cbv_ctx* ctx, const char* who, const uint8_t* data, size_t n, const cbv_color_profile* profile, const cbv_lens* lens,
                          const double* M9, int dw, int dh, int rot180, uint8_t* out, int out_stride, int32_t* status)
{
    if (!ctx) return cbv_fail(nullptr, CBV_ERR_ARG, "%s: ctx is null", who);
    if (!data || !out || !M9 || !profile || !status || dw <= 0 || dh <= 0 || dw > 8192 || dh > 8192 || out_stride < dw * 3)
        return cbv_fail(ctx, CBV_ERR_ARG, "%s: bad arguments", who);
    JpegDesc D;
    JpegTables T;
    RC(jpeg_header(ctx, who, data, n, &D, &T));
    if (D.h > 65535) return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "%s: %d rows", who, D.h);
    ProfileTabs pt;
    RC(profile_tabs_checked(ctx, profile, &pt, who));
    LensDev L;
    if (lens) RC(lens_checked(ctx, lens, &L, who));
    u32 S;
    int segments;
    RC(jpeg_piece_size(ctx, who, CBV_JPEG_ENTROPY_AUTO, 0, &S, &segments));
    CBV_ENTER_DRAINED(ctx);
    double Minv[9];
    if (!host_invert3x3(M9, Minv)) memset(Minv, 0, sizeof(Minv));
    const Geom g = tight_geom(D.w, D.h);
    // the warped board in ctx->c, the call's tables behind it
    const size_t o_tabs = ((size_t)dw * dh * 3 + 255) & ~(size_t)255;
    const size_t o_lens = o_tabs + ((sizeof(ProfileTabs) + 255) & ~(size_t)255);
    RC(dev_ensure(ctx, &ctx->c, o_lens + sizeof(LensBoard) + 256));
    JpegBatch B;
    RC(jpeg_single_dev(ctx, data, n, D, T, S, segments, nullptr, g, &B, nullptr, true)); // the decode stops at the planes
    const ProfileTabs* dpt = nullptr; // a disabled profile: the plain warp
    if (profile->enabled) {
        CBV_HIP(ctx, hipMemcpyAsync((u8*)ctx->c.p + o_tabs, &pt, sizeof(pt), hipMemcpyHostToDevice, ctx->stream));
        CBV_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (pt is on this stack)
        dpt = (const ProfileTabs*)((u8*)ctx->c.p + o_tabs);
    }
    const WarpSrc src = warp_src_jpeg(B.planes, B.plane_stride, B.descs, g, dpt);
    if (lens) {
        const LensBoard T = lens_board(Minv, dw, dh, rot180, (u8*)ctx->c.p, dw * 3, (size_t)dw * dh * 3, dpt);
        CBV_HIP(ctx, hipMemcpyAsync((u8*)ctx->c.p + o_lens, &T, sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        CBV_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (T is on this stack)
        RC(launch_warp_lens(ctx, src, L, (const LensBoard*)((u8*)ctx->c.p + o_lens), 1, dw, dh, 0, 1, nullptr, nullptr));
    } else
        RC(launch_warp(ctx, src, Minv, dw, dh, rot180, (u8*)ctx->c.p, dw * 3, (size_t)dw * dh * 3, 1));
    int st = 0;
    CBV_HIP(ctx, hipMemcpyAsync(&st, B.status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipMemcpy2DAsync(out, out_stride, ctx->c.p, (size_t)dw * 3, (size_t)dw * 3, dh, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *status = st;
    return CBV_DONE(CBV_OK);
}

extern "C" int cbv_warp_jpeg(cbv_ctx* ctx, const uint8_t* data, size_t n, const cbv_color_profile* profile, const double* M9, int dw, int dh, int rot180,
                             uint8_t* out, int out_stride, int32_t* status)
{
    return warp_jpeg_call(ctx, "cbv_warp_jpeg", data, n, profile, nullptr, M9, dw, dh, rot180, out, out_stride, status);
}

extern "C" int cbv_warp_jpeg_lens(cbv_ctx* ctx, const uint8_t* data, size_t n, const cbv_color_profile* profile, const cbv_lens* lens, const double* M9,
                                  int dw, int dh, int rot180, uint8_t* out, int out_stride, int32_t* status)
{
    const cbv_color_profile none = {};
    return warp_jpeg_call(ctx, "cbv_warp_jpeg_lens", data, n, profile ? profile : &none, lens && lens->enabled ? lens : nullptr, M9, dw, dh, rot180, out,
                          out_stride, status);
}
