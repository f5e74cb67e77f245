// ---------------------------------------------------------------------------
// piece colour per square (include/cbv.h): host classification and calibration, the one-board entry point, and a board's
// tone stage in the pipeline (set / sums / records)
// ---------------------------------------------------------------------------
#include "cbv_pipeline.h"
#include "tone_core.h"

// pixels of the centre disc of a w x h square (bit 0 of build_piece_mask, SquareDesc::cnt[0])
static u32 tone_disc_count(int w, int h)
{
    const int cx = w / 2, cy = h / 2, r = std::min(w, h) / 4;
    u32 n = 0;
    for (int y = cy - r; y <= cy + r; y++)
        for (int x = cx - r; x <= cx + r; x++) n += (x - cx) * (x - cx) + (y - cy) * (y - cy) <= r * r ? 1u : 0u;
    return n;
}

extern "C" int cbv_tone_classify_host(const cbv_tone_model* model, const cbv_tone_sums* sums, int n, uint64_t* white, uint64_t* black)
{
    if (!model || !sums || !white || !black || n < 0 || n > CBV_MAX_SQUARES) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_tone_classify_host: bad arguments");
    if (!model->calibrated) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_tone_classify_host: the model is not calibrated");
    u64 w = 0, b = 0;
    for (int i = 0; i < n; i++) {
        const int t = tone_classify(model, i, &sums[i]);
        if (t == TONE_WHITE) w |= 1ull << i;
        if (t == TONE_BLACK) b |= 1ull << i;
    }
    *white = w;
    *black = b;
    return CBV_OK;
}

extern "C" int cbv_tone_calibrate_host(const cbv_tone_sums* sums, const uint8_t* position, double margin, cbv_tone_model* model,
                                       cbv_tone_report* report)
{
    if (!sums || !position || !model) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_tone_calibrate_host: null argument");
    if (!(margin >= 0.0 && margin < 0.5)) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_tone_calibrate_host: margin %g is outside [0, 0.5)", margin);
    cbv_tone_model m;
    memset(&m, 0, sizeof(m));
    cbv_tone_report rep;
    memset(&rep, 0, sizeof(rep));
    double acc[2][2][3] = {};
    for (int i = 0; i < CBV_MAX_SQUARES; i++) {
        const int p = position[i];
        if (p == 0) continue;
        if (p > 2) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_tone_calibrate_host: position[%d] = %d (0 empty, 1 white, 2 black)", i, p);
        if (sums[i].cnt == 0) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_tone_calibrate_host: square %d has no pixels", i);
        const int k = tone_square_colour(i);
        double f[3];
        tone_mean(&sums[i], f);
        for (int c = 0; c < 3; c++) acc[k][p - 1][c] = acc[k][p - 1][c] + f[c];
        rep.samples[k][p - 1] += 1;
    }
    for (int k = 0; k < 2; k++) {
        for (int p = 0; p < 2; p++) {
            if (!rep.samples[k][p])
                return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_tone_calibrate_host: no %s piece stands on a %s square", p ? "black" : "white", k ? "dark" : "light");
            for (int c = 0; c < 3; c++) m.centroid[k][p][c] = acc[k][p][c] / (double)rep.samples[k][p];
        }
        rep.D[k] = tone_dist2(m.centroid[k][0], m.centroid[k][1]);
        if (rep.D[k] == 0.0) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_tone_calibrate_host: white and black pieces look the same on %s squares", k ? "dark" : "light");
    }
    m.margin = margin;
    m.calibrated = 1;
    for (int i = 0; i < CBV_MAX_SQUARES; i++) {
        if (!position[i]) continue;
        const int t = tone_classify(&m, i, &sums[i]);
        if (t == TONE_UNDECIDED) rep.undecided |= 1ull << i;
        else if (t != position[i]) rep.misclassified |= 1ull << i;
    }
    *model = m;
    if (report) *report = rep;
    return CBV_OK;
}

extern "C" int cbv_tone_sums_image(cbv_ctx* ctx, const cbv_host_image* img, const cbv_roi* rois, int n, cbv_tone_sums* out)
{
    if (!ctx) return CBV_ERR_ARG;
    if (!img || !img->data || !rois || !out || n <= 0 || n > CBV_MAX_SQUARES || img->cn != 3 || img->w <= 0 || img->h <= 0 || img->stride < img->w * 3)
        return cbv_fail(ctx, CBV_ERR_ARG, "cbv_tone_sums_image: a 3-channel host image and 1..%d ROIs are needed (n=%d)", CBV_MAX_SQUARES, n);
    int y0 = img->h, y1 = 0;
    for (int i = 0; i < n; i++) {
        const cbv_roi& r = rois[i];
        if (r.w <= 0 || r.h <= 0 || r.w > CBV_MAX_SQUARE_DIM || r.h > CBV_MAX_SQUARE_DIM || r.x0 < 0 || r.y0 < 0 || r.x0 + r.w > img->w || r.y0 + r.h > img->h)
            return cbv_fail(ctx, CBV_ERR_ARG, "cbv_tone_sums_image: roi %d (%d,%d %dx%d) is outside the %dx%d image or larger than %d", i, r.x0, r.y0, r.w, r.h,
                            img->w, img->h, CBV_MAX_SQUARE_DIM);
        y0 = std::min(y0, r.y0);
        y1 = std::max(y1, r.y0 + r.h);
    }
    CBV_ENTER_DRAINED(ctx);
    // the rows the ROIs cover, tightly packed
    const int rowb = img->w * 3;
    const size_t bytes = (size_t)rowb * (y1 - y0);
    std::vector<SquareDesc> descs((size_t)n);
    memset(descs.data(), 0, sizeof(SquareDesc) * n);
    for (int i = 0; i < n; i++) {
        SquareDesc& d = descs[i];
        d.w = rois[i].w;
        d.h = rois[i].h;
        d.cn = 3;
        d.stride = rowb;
        d.src_off = (rois[i].y0 - y0) * rowb + rois[i].x0 * 3;
        d.cnt[0] = tone_disc_count(d.w, d.h);
    }
    const size_t o_out = (sizeof(SquareDesc) * n + 255) & ~(size_t)255;
    RC(dev_ensure(ctx, &ctx->in, bytes + 256));
    RC(dev_ensure(ctx, &ctx->c, o_out + sizeof(cbv_tone_sums) * CBV_MAX_SQUARES));
    u8* small = (u8*)ctx->c.p; // descriptors, then the records
    CBV_HIP(ctx, hipMemcpy2DAsync(ctx->in.p, rowb, img->data + (size_t)y0 * img->stride, img->stride, rowb, y1 - y0, hipMemcpyHostToDevice, ctx->stream));
    CBV_HIP(ctx, hipMemcpyAsync(small, descs.data(), sizeof(SquareDesc) * n, hipMemcpyHostToDevice, ctx->stream));
    RC(launch_piece_tone(ctx, (const u8*)ctx->in.p, 0, (const SquareDesc*)small, n, (cbv_tone_sums*)(small + o_out), 1));
    CBV_HIP(ctx, hipMemcpyAsync(out, small + o_out, sizeof(cbv_tone_sums) * n, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_DONE(CBV_OK);
}

// ---- a board's tone stage ----

extern "C" int cbv_pipeline_set_tones(cbv_pipeline* p, const cbv_tone_model* model)
{
    if (!p) return cbv_fail(nullptr, CBV_ERR_ARG, "cbv_pipeline_set_tones: the board is null");
    Pipe& P = *p->pipe;
    Board& B = p->b;
    cbv_ctx* ctx = P.ctx;
    if (!P.configured) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_set_tones: the pipeline is not configured");
    if (model && !model->calibrated) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_set_tones: the model is not calibrated");
    if (model && !(model->margin >= 0.0 && model->margin < 0.5)) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_set_tones: margin %g is outside [0, 0.5)", model->margin);
    if (B.cfg.n_rois != 64) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_set_tones: tones need the 64 squares of a board, this one has %d", B.cfg.n_rois);
    if (!model && B.session && B.ses_cfg.tone)
        return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_set_tones: the board's session breaks ties with the tones; end it first");
    CBV_ENTER(ctx);
    if (!model && !B.tones) return CBV_OK;
    RC(join_scan(P)); // the runs in flight keep their arguments; the tables are rebuilt behind them
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (model) {
        // the board's buffers, made when it first enables tones: 1 KB of sums and 16 bytes of record per slot
        RC(dev_ensure(ctx, &B.d_tone_sums, sizeof(cbv_tone_sums) * CBV_MAX_SQUARES * (size_t)P.max_frames));
        RC(dev_ensure(ctx, &B.d_tone_res, sizeof(cbv_tone_result) * (size_t)P.max_frames));
        RC(dev_ensure(ctx, &B.d_tone_model, sizeof(cbv_tone_model)));
        if (!B.tones) {
            CBV_HIP(ctx, hipMemset(B.d_tone_sums.p, 0, sizeof(cbv_tone_sums) * CBV_MAX_SQUARES * (size_t)P.max_frames));
            CBV_HIP(ctx, hipMemset(B.d_tone_res.p, 0, sizeof(cbv_tone_result) * (size_t)P.max_frames));
        }
        CBV_HIP(ctx, hipMemcpy(B.d_tone_model.p, model, sizeof(cbv_tone_model), hipMemcpyHostToDevice));
        B.tone_model = *model;
    }
    B.tones = model != nullptr;
    return pipeline_tables(P);
}

extern "C" int cbv_pipeline_tone_sums(cbv_pipeline* p, int slot, cbv_tone_sums* out)
{
    if (!p || !out) return cbv_fail(p ? p->pipe->ctx : nullptr, CBV_ERR_ARG, "cbv_pipeline_tone_sums: null argument");
    Pipe& P = *p->pipe;
    const Board& B = p->b;
    cbv_ctx* ctx = P.ctx;
    if (!P.configured) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_tone_sums: the pipeline is not configured");
    if (B.cfg.n_rois != 64) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_tone_sums: tones need the 64 squares of a board, this one has %d", B.cfg.n_rois);
    if (slot < 0 || slot >= P.max_frames) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_tone_sums: bad slot %d", slot);
    CBV_ENTER_DRAINED(ctx);
    // the same kernel on the slot's warped board, whether the board's tones are on or off
    RC(join_scan(P));
    RC(dev_ensure(ctx, &ctx->c, sizeof(cbv_tone_sums) * CBV_MAX_SQUARES));
    RC(launch_piece_tone(ctx, B.warped + B.warped_stride * slot, 0, (const SquareDesc*)B.d_descs.p, 64, (cbv_tone_sums*)ctx->c.p, 1));
    CBV_HIP(ctx, hipMemcpyAsync(out, ctx->c.p, sizeof(cbv_tone_sums) * CBV_MAX_SQUARES, hipMemcpyDeviceToHost, ctx->stream));
    CBV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CBV_DONE(CBV_OK);
}

extern "C" int cbv_pipeline_tones(cbv_pipeline* p, int slot0, int count, cbv_tone_result* out)
{
    if (!p || !out) return cbv_fail(p ? p->pipe->ctx : nullptr, CBV_ERR_ARG, "cbv_pipeline_tones: null argument");
    Pipe& P = *p->pipe;
    const Board& B = p->b;
    cbv_ctx* ctx = P.ctx;
    if (!P.configured || !B.tones) return cbv_fail(ctx, CBV_ERR_STATE, "cbv_pipeline_tones: the board's tones are off (cbv_pipeline_set_tones)");
    if (slot0 < 0 || count <= 0 || slot0 + count > P.max_frames) return cbv_fail(ctx, CBV_ERR_ARG, "cbv_pipeline_tones: bad slot range");
    CBV_ENTER(ctx);
    return pipeline_readback(P, out, (const cbv_tone_result*)B.d_tone_res.p + slot0, sizeof(cbv_tone_result) * (size_t)count);
}
