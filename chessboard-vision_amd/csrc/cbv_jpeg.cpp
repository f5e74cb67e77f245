// Motion-JPEG entry points (include/cbv.h): the header probe, the host twin and the single-frame GPU decode.  The host
// reads the header only; the entropy data is the kernels' (k_jpeg.hip).
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

// the piece size a mode and a piece_bytes argument mean (0: every frame by restart interval), and whether frames with DRI
// go the piece path too (CBV_JPEG_ENTROPY_SEGMENTS); or an error
static int jpeg_piece_size(cbv_ctx* ctx, const char* who, int mode, uint32_t piece_bytes, u32* S, int* segments)
{
    if (mode != CBV_JPEG_ENTROPY_AUTO && mode != CBV_JPEG_ENTROPY_INTERVAL && mode != CBV_JPEG_ENTROPY_PIECES && mode != CBV_JPEG_ENTROPY_SEGMENTS)
        return cbv_fail(ctx, CBV_ERR_ARG, "%s: entropy mode %d", who, mode);
    if (piece_bytes && (piece_bytes < 4 || (piece_bytes & 3u) || piece_bytes > (1u << 24)))
        return cbv_fail(ctx, CBV_ERR_ARG, "%s: pieces of %u bytes (a multiple of 4, from 4 to 2^24, or 0 for the default)", who, piece_bytes);
    *S = mode == CBV_JPEG_ENTROPY_INTERVAL ? 0u : piece_bytes ? piece_bytes : (u32)JP_PIECE_DEFAULT;
    *segments = mode == CBV_JPEG_ENTROPY_SEGMENTS;
    return CBV_OK;
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
static int jpeg_single_dev(cbv_ctx* ctx, const uint8_t* data, size_t n, JpegDesc& D, const JpegTables& T, u32 S, int segments, u8* bgr_dev, Geom g,
                           JpegBatch* Bout, u8* planes_dev = nullptr, bool no_bgr = false)
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

// ---------------------------------------------------------------------------------------------------------------------
// The pipeline's Motion-JPEG ingest (cbv_pipeline_set_input_format(p, CBV_FMT_MJPEG)).  The host ring holds one stream per
// slot, `lengths` says how many bytes of each slot are used.  cbv_pipeline_submit parses the slots' headers out of the
// pinned ring (a few hundred bytes each; the entropy data is never read on the host), copies the used bytes and enqueues the
// decode on the copy stream behind the copy, `depth` frames at a time through one set of scratch buffers
// (cbv_pipeline_set_jpeg_depth).
// ---------------------------------------------------------------------------------------------------------------------
// the scratch of one launch, `depth` frames of everything: allocated as a set, replaced as a set
struct JpegScratch {
    int depth = 0;
    u32* mpos = nullptr;     // [depth * max_intervals]
    int16_t* coef = nullptr; // [depth][frame_elems]
    u8* planes = nullptr;    // null where the decode writes the plane ring
    bool has_planes = false;
    // the piece path: `depth` frames of piece_cap pieces and, in segments mode, of max_intervals segments
    u32* pieces = nullptr;
    size_t piece_stride = 0; // u32 words per frame
    u32 piece_cap = 0;       // pieces a frame may have
    u32 piece_bytes = 0;     // 0: every frame by restart interval
    int segments = 0;
    u32* segs = nullptr;
    size_t seg_stride = 0;   // u32 words per frame
};
struct JpegState {
    enum { NSETS = 16 };
    // pinned, with the slots' lifetime
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
    size_t frame_elems = 0;
    size_t max_int = 0;       // the intervals a frame can have: a restart interval of one MCU in the sampling with most MCUs
    u32* d_stats = nullptr;   // [max_frames][3]
    // planes mode (cbv_pipeline_set_jpeg_planes): the plane ring, [max_frames] slots of plane_slot bytes and 256 more, and the
    // descriptors the WARP reads, which change only behind the wait for the runs that read them (d_desc is the decode's)
    u8* d_pring = nullptr;
    size_t plane_slot = 0;
    int pring_mode = CBV_JPEG_PLANES_OFF;
    JpegDesc* d_wdesc = nullptr; // [max_frames]
    JpegScratch sc;           // sized with the format, the entropy setting and the depth (pipeline_jpeg_size_scratch)
};

// the samplings in the order in which the planes modes admit them: CBV_JPEG_PLANES_<X> admits those up to X
static int jpeg_sampling(const JpegDesc& D) { return D.ncomp == 1 ? CBV_JPEG_PLANES_GRAY : D.hs == 1 ? CBV_JPEG_PLANES_444 : D.vs == 1 ? CBV_JPEG_PLANES_422 : CBV_JPEG_PLANES_420; }
static const char* jpeg_sampling_name(int s)
{
    return s == CBV_JPEG_PLANES_GRAY ? "gray" : s == CBV_JPEG_PLANES_420 ? "4:2:0" : s == CBV_JPEG_PLANES_422 ? "4:2:2" : s == CBV_JPEG_PLANES_444 ? "4:4:4" : "off";
}
static bool jpeg_planes_mode_ok(int mode) { return mode >= CBV_JPEG_PLANES_OFF && mode <= CBV_JPEG_PLANES_444; }
// plane_total of a w x h frame in a sampling (jpeg_parse_header's, whole MCUs)
static size_t jpeg_plane_elems(int w, int h, int sampling)
{
    const size_t hs = sampling == CBV_JPEG_PLANES_420 || sampling == CBV_JPEG_PLANES_422 ? 2 : 1, vs = sampling == CBV_JPEG_PLANES_420 ? 2 : 1;
    const size_t mcux = ((size_t)w + 8 * hs - 1) / (8 * hs), mcuy = ((size_t)h + 8 * vs - 1) / (8 * vs);
    return mcux * mcuy * 64 * (sampling == CBV_JPEG_PLANES_GRAY ? 1 : hs * vs + 2);
}

extern "C" size_t cbv_jpeg_plane_slot_bytes(int w, int h, int mode)
{
    if (w < 1 || h < 1 || !jpeg_planes_mode_ok(mode) || mode == CBV_JPEG_PLANES_OFF) return 0;
    size_t most = 0;
    for (int s = CBV_JPEG_PLANES_GRAY; s <= mode; s++) most = std::max(most, jpeg_plane_elems(w, h, s));
    return (most + 255) & ~(size_t)255;
}

// a gray frame of the pipeline's size: what the warp reads of a slot that was never decoded, over zeroed planes
static JpegDesc jpeg_gray_desc(int w, int h)
{
    JpegDesc D;
    memset(&D, 0, sizeof(D));
    D.w = w;
    D.h = h;
    D.ncomp = 1;
    D.hs = D.vs = 1;
    D.mcux = (w + 7) / 8;
    D.mcuy = (h + 7) / 8;
    D.nint = 1;
    D.bw[0] = D.mcux;
    D.bh[0] = D.mcuy;
    D.cw[0] = w;
    D.ch[0] = h;
    D.plane_total = (uint32_t)D.mcux * (uint32_t)D.mcuy * 64u;
    D.std_tables = 1;
    return D;
}

bool pipeline_jpeg_has_planes(const Pipe& P) { return P.jpeg && P.jpeg->d_pring; }

// a new ring for `mode` (null for OFF): zeroed, 256 bytes of slack behind the last slot
static int jpeg_plane_ring_alloc(Pipe& P, int mode, const char* who, u8** ring, size_t* slot)
{
    *ring = nullptr;
    *slot = cbv_jpeg_plane_slot_bytes(P.w, P.h, mode);
    if (!*slot) return CBV_OK;
    const size_t bytes = *slot * (size_t)P.max_frames + 256;
    if (hipMalloc((void**)ring, bytes) != hipSuccess || hipMemset(*ring, 0, bytes) != hipSuccess) {
        (void)hipGetLastError();
        if (*ring) (void)hipFree(*ring);
        *ring = nullptr;
        return cbv_fail(P.ctx, CBV_ERR_HIP, "%s: the plane ring of %zu bytes could not be allocated", who, bytes);
    }
    return CBV_OK;
}

// the ring `ring` takes the place of the one that is there; the warp's descriptors become gray frames
static int jpeg_plane_ring_install(Pipe& P, u8* ring, size_t slot, int mode)
{
    cbv_ctx* ctx = P.ctx;
    JpegState* J = P.jpeg;
    if (J->d_pring) (void)hipFree(J->d_pring);
    J->d_pring = ring;
    J->plane_slot = slot;
    J->pring_mode = ring ? mode : CBV_JPEG_PLANES_OFF;
    if (ring) {
        const std::vector<JpegDesc> gray((size_t)P.max_frames, jpeg_gray_desc(P.w, P.h));
        CBV_HIP(ctx, hipMemcpy(J->d_wdesc, gray.data(), gray.size() * sizeof(JpegDesc), hipMemcpyHostToDevice));
    }
    return CBV_OK;
}

int pipeline_jpeg_plane_ring(Pipe& P, const char* who)
{
    JpegState* J = P.jpeg;
    if (!J) return CBV_OK;
    const int mode = P.jpeg_planes_on() ? P.jpeg_planes : CBV_JPEG_PLANES_OFF;
    if (J->pring_mode == mode && (J->d_pring != nullptr) == (mode != CBV_JPEG_PLANES_OFF)) return CBV_OK;
    u8* ring;
    size_t slot;
    RC(jpeg_plane_ring_alloc(P, mode, who, &ring, &slot));
    return jpeg_plane_ring_install(P, ring, slot, mode);
}

WarpSrc pipeline_jpeg_warp_src(const Pipe& P, int slot0, const ProfileTabs* ptabs, int np, size_t dst_profile_stride)
{
    const JpegState* J = P.jpeg;
    return warp_src_jpeg(J->d_pring + J->plane_slot * slot0, J->plane_slot, J->d_wdesc + slot0, P.g, ptabs, np, dst_profile_stride);
}

int pipeline_jpeg_slot_bgr(Pipe& P, int slot, u8* bgr)
{
    JpegState* J = P.jpeg;
    JpegBatch B;
    memset(&B, 0, sizeof(B));
    B.descs = J->d_wdesc + slot;
    B.planes = J->d_pring + J->plane_slot * slot;
    B.plane_stride = J->plane_slot;
    B.bgr = bgr;
    B.bgr_stride = P.g.stride;
    B.bgr_frame_stride = P.g.frame_stride;
    B.nframes = 1;
    return launch_jpeg_color(P.ctx, B, P.w, P.h);
}

size_t pipeline_jpeg_default_slot_bytes(int w, int h) { return (((size_t)w * h + 1) / 2 + 255) & ~(size_t)255; }

static void jpeg_scratch_free(JpegScratch& sc)
{
    void* dev[] = {sc.mpos, sc.coef, sc.planes, sc.pieces, sc.segs};
    for (void* q : dev)
        if (q) (void)hipFree(q);
    sc = JpegScratch();
}

void pipeline_jpeg_free(Pipe& P)
{
    JpegState* J = P.jpeg;
    if (!J) return;
    if (J->h_lengths) (void)hipHostFree(J->h_lengths);
    if (J->h_desc) (void)hipHostFree(J->h_desc);
    if (J->h_ioff) (void)hipHostFree(J->h_ioff);
    if (J->h_tabs) (void)hipHostFree(J->h_tabs);
    void* dev[] = {J->d_desc, J->d_ioff, J->d_tabs, J->d_status, J->d_nfound, J->d_stats, J->d_pring, J->d_wdesc};
    for (void* q : dev)
        if (q) (void)hipFree(q);
    jpeg_scratch_free(J->sc);
    delete J;
    P.jpeg = nullptr;
}

// what lives as long as the slots; the decode's scratch is pipeline_jpeg_size_scratch's
int pipeline_jpeg_ensure(Pipe& P)
{
    cbv_ctx* ctx = P.ctx;
    if (P.jpeg) return CBV_OK;
    if (P.h > 65535) return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "Motion-JPEG frames of %d rows", P.h);
    JpegState* J = new JpegState;
    P.jpeg = J;
    const size_t n = (size_t)P.max_frames;
    const size_t pw = ((size_t)P.w + 15) & ~(size_t)15, ph = ((size_t)P.h + 15) & ~(size_t)15;
    J->frame_elems = 3 * pw * ph;
    J->max_int = ((size_t)P.w + 7) / 8 * (((size_t)P.h + 7) / 8);
    bool ok = hipHostMalloc((void**)&J->h_lengths, n * sizeof(u32), hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc((void**)&J->h_desc, n * sizeof(JpegDesc), hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc((void**)&J->h_ioff, 2 * n * sizeof(u32), hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc((void**)&J->h_tabs, JpegState::NSETS * sizeof(JpegTables), hipHostMallocDefault) == hipSuccess &&
              hipMalloc((void**)&J->d_desc, n * sizeof(JpegDesc)) == hipSuccess && hipMalloc((void**)&J->d_ioff, 2 * n * sizeof(u32)) == hipSuccess &&
              hipMalloc((void**)&J->d_tabs, JpegState::NSETS * sizeof(JpegTables)) == hipSuccess &&
              hipMalloc((void**)&J->d_status, n * sizeof(int)) == hipSuccess && hipMalloc((void**)&J->d_nfound, n * sizeof(int)) == hipSuccess &&
              hipMalloc((void**)&J->d_stats, n * 3 * sizeof(u32)) == hipSuccess && hipMalloc((void**)&J->d_wdesc, n * sizeof(JpegDesc)) == hipSuccess;
    if (ok) ok = hipMemset(J->d_status, 0, n * sizeof(int)) == hipSuccess && hipMemset(J->d_stats, 0, n * 3 * sizeof(u32)) == hipSuccess;
    if (!ok) {
        pipeline_jpeg_free(P);
        return cbv_fail(ctx, CBV_ERR_HIP, "the Motion-JPEG decode's buffers could not be allocated");
    }
    memset(J->h_lengths, 0, n * sizeof(u32));
    return CBV_OK;
}

// The decode's scratch for the pipeline's slot size, entropy setting and depth: `depth` frames of the pipeline's size (the
// coefficients, 2 bytes a sample, and, unless the planes go to the plane ring, the planes, 1 byte a sample) in the
// sampling that needs most (4:4:4 padded to the 16 x 16 MCUs of 4:2:0) and a restart interval of one MCU; a frame's pieces
// are at most ceil(slot bytes / S), and with segments max_intervals more (every interval's last piece may be a short one,
// an empty interval is one piece).  The new set is allocated before the old one is freed: when it cannot be had the old one
// stays as it is.  The caller has waited for the copy stream; `who` names it in the messages.
int pipeline_jpeg_size_scratch(Pipe& P, const char* who)
{
    cbv_ctx* ctx = P.ctx;
    JpegState* J = P.jpeg;
    u32 S = 0;
    int segments = 0;
    RC(jpeg_piece_size(ctx, who, P.jpeg_entropy, P.jpeg_piece_bytes, &S, &segments));
    const size_t depth = (size_t)P.jpeg_depth;
    JpegScratch n;
    n.depth = P.jpeg_depth;
    n.piece_bytes = S;
    n.segments = segments;
    const size_t cap = S ? (P.jpeg_slot_bytes + S - 1) / S + (segments ? J->max_int : 0) : 0;
    if (cap > 0xFFFFFFFFu) return cbv_fail(ctx, CBV_ERR_ARG, "%s: %zu pieces per frame", who, cap);
    n.piece_cap = (u32)cap;
    n.piece_stride = jpeg_piece_words(cap, segments);
    n.seg_stride = segments ? jpeg_seg_words(J->max_int) : 0;
    n.has_planes = !(P.jpeg_planes != CBV_JPEG_PLANES_OFF && P.raw_config()); // (there the decode writes the plane ring)
    const JpegScratch& o = J->sc;
    if (o.depth == n.depth && o.has_planes == n.has_planes && o.piece_stride == n.piece_stride && o.seg_stride == n.seg_stride && o.piece_cap == n.piece_cap) { // the buffers serve
        J->sc.piece_bytes = S;
        J->sc.segments = segments;
        return CBV_OK;
    }
    const size_t b_mpos = depth * J->max_int * sizeof(u32), b_coef = depth * J->frame_elems * sizeof(int16_t), b_planes = n.has_planes ? depth * J->frame_elems : 0;
    const size_t b_pieces = depth * n.piece_stride * sizeof(u32), b_segs = depth * n.seg_stride * sizeof(u32);
    const bool ok = hipMalloc((void**)&n.mpos, b_mpos) == hipSuccess && hipMalloc((void**)&n.coef, b_coef) == hipSuccess &&
                    (!b_planes || hipMalloc((void**)&n.planes, b_planes) == hipSuccess) && (!b_pieces || hipMalloc((void**)&n.pieces, b_pieces) == hipSuccess) &&
                    (!b_segs || hipMalloc((void**)&n.segs, b_segs) == hipSuccess);
    if (!ok) {
        (void)hipGetLastError();
        jpeg_scratch_free(n);
        return cbv_fail(ctx, CBV_ERR_HIP, "%s: the Motion-JPEG decode's scratch (%zu bytes for %zu frames per launch) could not be allocated", who,
                        b_mpos + b_coef + b_planes + b_pieces + b_segs, depth);
    }
    jpeg_scratch_free(J->sc);
    J->sc = n;
    return CBV_OK;
}

// a stream's header against the pipeline: its size, and a table set for it (one of the cache, or a new one at *new_sets)
static int jpeg_slot_header(Pipe& P, const char* who, int slot, const u8* data, size_t n, JpegDesc* D)
{
    cbv_ctx* ctx = P.ctx;
    JpegState* J = P.jpeg;
    JpegTables T;
    char msg[200];
    const int rc = jpeg_parse_header(data, n, D, &T, msg, sizeof(msg));
    if (rc) return cbv_fail(ctx, rc, "%s: slot %d: %s", who, slot, msg);
    if (D->w != P.w || D->h != P.h)
        return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "%s: slot %d: a %d x %d frame, the pipeline's are %d x %d", who, slot, D->w, D->h, P.w, P.h);
    if (P.jpeg_planes_on() && jpeg_sampling(*D) > P.jpeg_planes)
        return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "%s: slot %d: a %s frame, the plane ring's slots hold up to %s (cbv_pipeline_set_jpeg_planes)", who, slot,
                        jpeg_sampling_name(jpeg_sampling(*D)), jpeg_sampling_name(P.jpeg_planes));
    int k = 0;
    while (k < J->nsets && memcmp(&J->h_tabs[k], &T, sizeof(T))) k++;
    if (k == J->nsets) {
        if (k == JpegState::NSETS) return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "%s: slot %d: more than %d different table sets in flight", who, slot, k);
        memcpy(&J->h_tabs[k], &T, sizeof(T));
        J->nsets++;
    }
    D->table_set = k;
    return CBV_OK;
}

// cbv_pipeline_submit with the Motion-JPEG format: called under the context's lock with the copy stream made; read_ev = what the
// writes into the frame ring wait for (may be null)
int pipeline_jpeg_submit(Pipe& P, int slot0, int count, hipEvent_t read_ev)
{
    cbv_ctx* ctx = P.ctx;
    JpegState* J = P.jpeg;
    const char* who = "cbv_pipeline_submit";
    const size_t sb = P.jpeg_slot_bytes;
    if (J->sc.depth < 1) return cbv_fail(ctx, CBV_ERR_STATE, "%s: the Motion-JPEG decode has no scratch", who);
    const bool to_ring = P.jpeg_raw(); // raw mode on the plane ring: the decode stops at the slots' planes
    if (to_ring ? !J->d_pring : !J->sc.planes) return cbv_fail(ctx, CBV_ERR_STATE, "%s: the Motion-JPEG decode has nowhere to put the planes", who);
    if (J->nsets == JpegState::NSETS) { // the cache is full: start again once nothing reads it
        CBV_HIP(ctx, hipStreamSynchronize(P.copy_stream));
        J->nsets = 0;
    }
    const int sets_before = J->nsets;
    // 1. every header, before anything is enqueued
    for (int s = slot0; s < slot0 + count; s++) {
        const u32 len = J->h_lengths[s];
        int rc = CBV_OK;
        if (len == 0 || len > sb) rc = cbv_fail(ctx, CBV_ERR_ARG, "%s: slot %d: length %u, a slot holds %zu bytes", who, s, len, sb);
        else rc = jpeg_slot_header(P, who, s, P.host_ring + sb * s, len, &J->h_desc[s]);
        if (rc) {
            J->nsets = sets_before;
            return rc;
        }
    }
    for (int c0 = 0; c0 < count; c0 += J->sc.depth) {
        const int s = slot0 + c0, cf = std::min<int>(J->sc.depth, count - c0);
        u32 acc = 0;
        for (int i = 0; i < cf; i++) {
            J->h_ioff[2 * s + i] = acc;
            acc += (u32)J->h_desc[s + i].nint;
        }
        J->h_ioff[2 * s + cf] = acc;
    }
    // 2. the used bytes of every slot, the descriptors, the new table sets
    for (int s = slot0; s < slot0 + count; s++) {
        const size_t bytes = std::min(sb, ((size_t)J->h_lengths[s] + 255) & ~(size_t)255);
        CBV_HIP(ctx, hipMemcpyAsync(P.raw_ring + sb * s, P.host_ring + sb * s, bytes, hipMemcpyHostToDevice, P.copy_stream));
    }
    CBV_HIP(ctx, hipMemcpyAsync(J->d_desc + slot0, J->h_desc + slot0, (size_t)count * sizeof(JpegDesc), hipMemcpyHostToDevice, P.copy_stream));
    CBV_HIP(ctx, hipMemcpyAsync(J->d_ioff + 2 * slot0, J->h_ioff + 2 * slot0, (size_t)2 * count * sizeof(u32), hipMemcpyHostToDevice, P.copy_stream));
    if (J->nsets > sets_before)
        CBV_HIP(ctx, hipMemcpyAsync(J->d_tabs + sets_before, J->h_tabs + sets_before, (size_t)(J->nsets - sets_before) * sizeof(JpegTables),
                                    hipMemcpyHostToDevice, P.copy_stream));
    if (read_ev) CBV_HIP(ctx, hipStreamWaitEvent(P.copy_stream, read_ev, 0));
    // The runs in flight read the plane ring and the warp's descriptors of their slots: both change only from here on, behind
    // the wait.  (d_desc above is read by the decode alone, whose launches of these slots are in stream order.)
    if (to_ring)
        CBV_HIP(ctx, hipMemcpyAsync(J->d_wdesc + slot0, J->d_desc + slot0, (size_t)count * sizeof(JpegDesc), hipMemcpyDeviceToDevice, P.copy_stream));
    // 3. the decode, a chunk of frames at a time through the one set of scratch buffers (stream order keeps them apart)
    hipStream_t caller = ctx->stream;
    ctx->stream = P.copy_stream;
    int rc = CBV_OK;
    for (int c0 = 0; c0 < count && !rc; c0 += J->sc.depth) {
        const int s = slot0 + c0, cf = std::min<int>(J->sc.depth, count - c0);
        JpegBatch B;
        B.data = P.raw_ring + sb * s;
        B.data_stride = sb;
        B.descs = J->d_desc + s;
        B.tables = J->d_tabs;
        B.ioff = J->d_ioff + 2 * s;
        B.mpos = J->sc.mpos;
        B.nfound = J->d_nfound + s;
        B.status = J->d_status + s;
        B.coef = J->sc.coef;
        B.coef_stride = J->frame_elems;
        B.planes = to_ring ? J->d_pring + J->plane_slot * s : J->sc.planes;
        B.plane_stride = to_ring ? J->plane_slot : J->frame_elems;
        B.bgr = to_ring ? nullptr : P.frames + P.g.frame_stride * s;
        B.bgr_stride = P.g.stride;
        B.bgr_frame_stride = P.g.frame_stride;
        B.nframes = cf;
        B.piece_bytes = J->sc.piece_bytes;
        B.pieces = J->sc.pieces;
        B.piece_stride = J->sc.piece_stride;
        B.piece_cap = J->sc.piece_cap;
        B.segments = J->sc.segments;
        B.segs = J->sc.segs;
        B.seg_stride = J->sc.seg_stride;
        B.stats = J->d_stats + 3 * (size_t)s;
        int any_dri = 0, any_pieces = 0;
        u32 max_blocks = 0;
        for (int i = 0; i < cf; i++) {
            any_dri |= J->h_desc[s + i].dri != 0;
            any_pieces |= J->sc.piece_bytes && (J->sc.segments || !J->h_desc[s + i].dri);
            max_blocks = std::max(max_blocks, J->h_desc[s + i].plane_total / 64u);
        }
        rc = launch_jpeg_decode(ctx, B, J->h_ioff[2 * s + cf], any_dri, any_pieces, max_blocks, P.w, P.h);
    }
    ctx->stream = caller;
    return rc;
}

extern "C" uint32_t* cbv_pipeline_host_jpeg_lengths(cbv_pipeline* p)
{
    if (!p || attached(p) || !p->pipe->jpeg) return nullptr;
    return p->pipe->jpeg->h_lengths;
}

extern "C" int cbv_pipeline_jpeg_status(cbv_pipeline* p, int slot0, int count, int32_t* out)
{
    if (!p) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_pipeline_jpeg_status: the pipeline is null");
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    if (attached(p)) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_jpeg_status: frames go to the parent of a board");
    if (!out || slot0 < 0 || count <= 0 || slot0 + count > P.max_frames) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_jpeg_status: bad slot range");
    if (!P.jpeg) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_jpeg_status: no Motion-JPEG frame was ever given to the pipeline");
    CBV_ENTER(ctx);
    if (P.copy_stream) CBV_HIP(ctx, hipStreamSynchronize(P.copy_stream));
    CBV_HIP(ctx, hipMemcpy(out, P.jpeg->d_status + slot0, (size_t)count * sizeof(int), hipMemcpyDeviceToHost));
    return CBV_OK;
}

extern "C" int cbv_pipeline_jpeg_stats(cbv_pipeline* p, int slot0, int count, cbv_jpeg_decode_stats* out)
{
    if (!p) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_pipeline_jpeg_stats: the pipeline is null");
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    if (attached(p)) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_jpeg_stats: frames go to the parent of a board");
    if (!out || slot0 < 0 || count <= 0 || slot0 + count > P.max_frames) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_jpeg_stats: bad slot range");
    if (!P.jpeg) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_jpeg_stats: no Motion-JPEG frame was ever given to the pipeline");
    CBV_ENTER(ctx);
    if (P.copy_stream) CBV_HIP(ctx, hipStreamSynchronize(P.copy_stream));
    static_assert(sizeof(cbv_jpeg_decode_stats) == 3 * sizeof(u32), "cbv_jpeg_decode_stats is three words");
    CBV_HIP(ctx, hipMemcpy(out, P.jpeg->d_stats + 3 * (size_t)slot0, (size_t)count * sizeof(cbv_jpeg_decode_stats), hipMemcpyDeviceToHost));
    return CBV_OK;
}

extern "C" int cbv_pipeline_set_jpeg_entropy(cbv_pipeline* p, int mode, uint32_t piece_bytes)
{
    const char* who = "cbv_pipeline_set_jpeg_entropy";
    if (!p) return cbv_fail(nullptr, CBV_ERR_ARG, "%s: the pipeline is null", who);
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    if (attached(p)) return cbv_fail(ctx, CBV_ERR_STATE, "%s: frames go to the parent of a board", who);
    u32 S;
    int segments;
    RC(jpeg_piece_size(ctx, who, mode, piece_bytes, &S, &segments));
    CBV_ENTER(ctx);
    const int mode_was = P.jpeg_entropy;
    const uint32_t bytes_was = P.jpeg_piece_bytes;
    P.jpeg_entropy = mode;
    P.jpeg_piece_bytes = piece_bytes;
    if (!P.jpeg || !P.jpeg_slot_bytes) return CBV_OK; // sized when the format is set
    const int rc = P.copy_stream && hipStreamSynchronize(P.copy_stream) != hipSuccess // the decodes in flight use the scratch
                       ? cbv_fail(ctx, CBV_ERR_HIP, "%s: the copy stream could not be waited for", who)
                       : pipeline_jpeg_size_scratch(P, who);
    if (rc) { // the setting that was stays, with its scratch (the new one is allocated before the old one is let go)
        P.jpeg_entropy = mode_was;
        P.jpeg_piece_bytes = bytes_was;
    }
    return rc;
}

extern "C" int cbv_pipeline_set_jpeg_depth(cbv_pipeline* p, int frames)
{
    const char* who = "cbv_pipeline_set_jpeg_depth";
    if (!p) return cbv_fail(nullptr, CBV_ERR_ARG, "%s: the pipeline is null", who);
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    if (attached(p)) return cbv_fail(ctx, CBV_ERR_STATE, "%s: frames go to the parent of a board", who);
    if (frames < 1 || frames > CBV_JPEG_DEPTH_MAX) return cbv_fail(ctx, CBV_ERR_ARG, "%s: %d frames per launch (1 to %d)", who, frames, CBV_JPEG_DEPTH_MAX);
    CBV_ENTER(ctx);
    const int was = P.jpeg_depth;
    P.jpeg_depth = frames;
    if (!P.jpeg || !P.jpeg_slot_bytes) return CBV_OK; // sized when the format is set
    const int rc = P.copy_stream && hipStreamSynchronize(P.copy_stream) != hipSuccess // the decodes in flight use the scratch
                       ? cbv_fail(ctx, CBV_ERR_HIP, "%s: the copy stream could not be waited for", who)
                       : pipeline_jpeg_size_scratch(P, who);
    if (rc) P.jpeg_depth = was; // with its scratch
    return rc;
}

extern "C" int cbv_pipeline_jpeg_depth(cbv_pipeline* p)
{
    const char* who = "cbv_pipeline_jpeg_depth";
    if (!p) return cbv_fail(nullptr, CBV_ERR_ARG, "%s: the pipeline is null", who);
    if (attached(p)) return cbv_fail(p->pipe->ctx, CBV_ERR_STATE, "%s: frames go to the parent of a board", who);
    return p->pipe->jpeg_depth;
}

extern "C" int cbv_pipeline_set_jpeg_slot_bytes(cbv_pipeline* p, size_t bytes)
{
    if (!p) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_pipeline_set_jpeg_slot_bytes: the pipeline is null");
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    if (attached(p)) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_set_jpeg_slot_bytes: frames go to the parent of a board");
    if (bytes < 256 || bytes > ((size_t)1 << 30)) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_set_jpeg_slot_bytes: %zu bytes", bytes);
    P.jpeg_slot_bytes = (bytes + 255) & ~(size_t)255;
    if (P.in_fmt != CBV_FMT_MJPEG) return CBV_OK;
    return cbv_pipeline_set_input_format(p, CBV_FMT_MJPEG); // frees both rings, as a format change does
}

extern "C" int cbv_pipeline_upload_jpeg(cbv_pipeline* p, int slot, const uint8_t* data, size_t n)
{
    const char* who = "cbv_pipeline_upload_jpeg";
    if (!p) return cbv_fail(nullptr, CBV_ERR_ARG, "%s: the pipeline is null", who);
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    if (attached(p)) return cbv_fail(ctx, CBV_ERR_STATE, "%s: frames go to the parent of a board", who);
    if (!data || slot < 0 || slot >= P.max_frames) return cbv_fail(ctx, CBV_ERR_ARG, "%s: bad arguments", who);
    JpegDesc D;
    JpegTables T;
    char msg[200];
    const int rc = jpeg_parse_header(data, n, &D, &T, msg, sizeof(msg));
    if (rc) return cbv_fail(ctx, rc, "%s: %s", who, msg);
    if (D.w != P.w || D.h != P.h) return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "%s: a %d x %d frame, the pipeline's are %d x %d", who, D.w, D.h, P.w, P.h);
    CBV_ENTER(ctx);
    const bool to_ring = P.jpeg_raw(); // raw mode on the plane ring: the decode stops at the slot's planes
    if (P.raw_mode() && !to_ring)
        return cbv_fail(ctx, CBV_ERR_STATE, "%s: the pipeline's frames are its raw ring (raw mode); it has no BGR frames to decode into", who);
    if (P.jpeg_planes_on() && jpeg_sampling(D) > P.jpeg_planes)
        return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "%s: slot %d: a %s frame, the plane ring's slots hold up to %s (cbv_pipeline_set_jpeg_planes)", who, slot,
                        jpeg_sampling_name(jpeg_sampling(D)), jpeg_sampling_name(P.jpeg_planes));
    RC(pipeline_jpeg_ensure(P));
    RC(join_scan(P)); // lanes and scan of the last run
    if (P.copy_stream) CBV_HIP(ctx, hipStreamSynchronize(P.copy_stream)); // a submitted decode of this slot lands first
    JpegBatch B;
    u32 S;
    int segments;
    RC(jpeg_piece_size(ctx, who, P.jpeg_entropy, P.jpeg_piece_bytes, &S, &segments));
    if (to_ring) {
        JpegState* J = P.jpeg;
        if (!J->d_pring) return cbv_fail(ctx, CBV_ERR_STATE, "%s: the pipeline has no plane ring", who);
        RC(jpeg_single_dev(ctx, data, n, D, T, S, segments, nullptr, P.g, &B, J->d_pring + J->plane_slot * slot, true));
    } else RC(jpeg_single_dev(ctx, data, n, D, T, S, segments, P.frames + P.g.frame_stride * slot, P.g, &B));
    if (to_ring) // the slot's descriptor for the warp (the runs are joined)
        CBV_HIP(ctx, hipMemcpyAsync(P.jpeg->d_wdesc + slot, B.descs, sizeof(JpegDesc), hipMemcpyDeviceToDevice, ctx->stream));
    CBV_HIP(ctx, hipMemcpyAsync(P.jpeg->d_status + slot, B.status, sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
    CBV_HIP(ctx, hipMemcpyAsync(P.jpeg->d_stats + 3 * (size_t)slot, B.stats, 3 * sizeof(u32), hipMemcpyDeviceToDevice, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_OK;
}

extern "C" int cbv_pipeline_set_jpeg_planes(cbv_pipeline* p, int mode)
{
    const char* who = "cbv_pipeline_set_jpeg_planes";
    if (!p) return cbv_fail(nullptr, CBV_ERR_ARG, "%s: the pipeline is null", who);
    Pipe& P = *p->pipe;
    cbv_ctx* ctx = P.ctx;
    if (attached(p)) return cbv_fail(ctx, CBV_ERR_STATE, "%s: frames go to the parent of a board", who);
    if (!jpeg_planes_mode_ok(mode)) return cbv_fail(ctx, CBV_ERR_ARG, "%s: mode %d", who, mode);
    CBV_ENTER(ctx);
    if (P.in_fmt != CBV_FMT_MJPEG) { // only stored: the ring comes with the format
        P.jpeg_planes = mode;
        return CBV_OK;
    }
    if (mode == P.jpeg_planes) return CBV_OK;
    // what is in flight reads the rings that go away here
    RC(join_scan(P));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (P.copy_stream) CBV_HIP(ctx, hipStreamSynchronize(P.copy_stream));
    // the new ring before the old one is let go: when it cannot be had, the setting that was stays, with its rings
    u8* ring;
    size_t slot;
    RC(jpeg_plane_ring_alloc(P, mode, who, &ring, &slot));
    const int was = P.jpeg_planes;
    P.jpeg_planes = mode;
    int rc = pipeline_jpeg_size_scratch(P, who); // (allocates before it frees)
    if (rc == CBV_OK && !P.frames && !P.jpeg_raw()) rc = pipeline_frame_ring(P); // the BGR ring comes back
    if (rc) {
        P.jpeg_planes = was;
        if (ring) (void)hipFree(ring);
        return rc;
    }
    RC(jpeg_plane_ring_install(P, ring, slot, mode));
    return cbv_pipeline_set_input_format(p, CBV_FMT_MJPEG); // frees the ingest rings (and a BGR ring no longer needed), as a format change does
}

extern "C" int cbv_pipeline_jpeg_planes(cbv_pipeline* p)
{
    const char* who = "cbv_pipeline_jpeg_planes";
    if (!p) return cbv_fail(nullptr, CBV_ERR_ARG, "%s: the pipeline is null", who);
    if (attached(p)) return cbv_fail(p->pipe->ctx, CBV_ERR_STATE, "%s: frames go to the parent of a board", who);
    return p->pipe->jpeg_planes;
}

extern "C" int cbv_warp_jpeg(cbv_ctx* ctx, const uint8_t* data, size_t n, const cbv_color_profile* profile, const double* M9, int dw, int dh, int rot180,
                             uint8_t* out, int out_stride, int32_t* status)
{
    const char* who = "cbv_warp_jpeg";
    if (!ctx) return cbv_fail(nullptr, CBV_ERR_ARG, "%s: ctx is null", who);
    if (!data || !out || !M9 || !profile || !status || dw <= 0 || dh <= 0 || dw > 8192 || dh > 8192 || out_stride < dw * 3)
        return cbv_fail(ctx, CBV_ERR_ARG, "%s: bad arguments", who);
    JpegDesc D;
    JpegTables T;
    RC(jpeg_header(ctx, who, data, n, &D, &T));
    if (D.h > 65535) return cbv_fail(ctx, CBV_ERR_UNSUPPORTED, "%s: %d rows", who, D.h);
    ProfileTabs pt;
    RC(profile_tabs_checked(ctx, profile, &pt, who));
    u32 S;
    int segments;
    RC(jpeg_piece_size(ctx, who, CBV_JPEG_ENTROPY_AUTO, 0, &S, &segments));
    CBV_ENTER_DRAINED(ctx);
    double Minv[9];
    if (!host_invert3x3(M9, Minv)) memset(Minv, 0, sizeof(Minv));
    const Geom g = tight_geom(D.w, D.h);
    // the warped board in ctx->c, the call's tables behind it
    const size_t o_tabs = ((size_t)dw * dh * 3 + 255) & ~(size_t)255;
    RC(dev_ensure(ctx, &ctx->c, o_tabs + sizeof(ProfileTabs) + 256));
    JpegBatch B;
    RC(jpeg_single_dev(ctx, data, n, D, T, S, segments, nullptr, g, &B, nullptr, true)); // the decode stops at the planes
    const ProfileTabs* dpt = nullptr; // a disabled profile: the plain warp
    if (profile->enabled) {
        CBV_HIP(ctx, hipMemcpyAsync((u8*)ctx->c.p + o_tabs, &pt, sizeof(pt), hipMemcpyHostToDevice, ctx->stream));
        CBV_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (pt is on this stack)
        dpt = (const ProfileTabs*)((u8*)ctx->c.p + o_tabs);
    }
    RC(launch_warp(ctx, warp_src_jpeg(B.planes, B.plane_stride, B.descs, g, dpt), Minv, dw, dh, rot180, (u8*)ctx->c.p, dw * 3, (size_t)dw * dh * 3, 1));
    int st = 0;
    CBV_HIP(ctx, hipMemcpyAsync(&st, B.status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipMemcpy2DAsync(out, out_stride, ctx->c.p, (size_t)dw * 3, (size_t)dw * 3, dh, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *status = st;
    return CBV_DONE(CBV_OK);
}
