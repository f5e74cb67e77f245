// The ChangeDetector sensitivity sweep on the device (include/cbv.h, cbv_pipeline_sweep): what calibrate_sensitivity.py's
// loop computes for every trackbar position, from frames already in a board's warped ring.
//
// k_change_hist   one workgroup per (square, frame), one launch per distinct blur kernel: ChangeDetector._preprocess exactly
//                 as k_change_blur_stats does it (change_blur.h), |gray - calibration gray| as the pixels leave the vertical
//                 pass, a 256-bin histogram in LDS, written as u16 (a square has at most 128 x 128 pixels).
// k_sweep_eval    one workgroup of four waves per (frame, blur kernel, slice of that kernel's settings), lane = square:
//                 suffix sums of the lanes' histograms once, then each wave takes a quarter of the slice; a setting is one cut (four divisions and ballots for the wave), one LDS
//                 lookup per square, the classes of ms_frame_finish and three ballots for the record's square sets.
// The histograms are read once per wave, never per setting.  Neither kernel has a profile id (the enumeration is closed):
// cbv_pipeline_sweep times them with event pairs.
#include <algorithm>
#include <cmath>

#include "change_blur.h"
#include "sweep_core.h"

namespace {

// One pixel into the wave's own histogram.  A quiet square puts nearly every pixel into bins 0..3, so the 64 increments of
// a wave mostly meet in one or two words: the lanes that hold the first active lane's value are counted by a ballot and
// added once, the others add for themselves.  (SW_HIST_PLAIN: every lane adds for itself, the form this is measured against.)
__device__ __forceinline__ void hist_add(u32* wave_hist, int dv)
{
#if defined(SW_HIST_PLAIN)
    atomicAdd(&wave_hist[dv], 1u);
#else
    const int lead = __builtin_amdgcn_readfirstlane(dv);
    const u64 same = __ballot(dv == lead);
    if (dv != lead) atomicAdd(&wave_hist[dv], 1u);
    else if ((int)(threadIdx.x & 63) == __builtin_ctzll(same)) atomicAdd(&wave_hist[lead], (u32)__builtin_popcountll(same));
#endif
}

template <int NT>
__global__ __launch_bounds__(NT) void k_change_hist(const u8* __restrict__ src, size_t src_frame_stride, const SquareDesc* __restrict__ descs,
                                                      const u8* __restrict__ calib, u16* __restrict__ out, size_t out_frame_stride,
                                                      const ChangeBlur cb)
{
    constexpr int NW = NT / 64;
    __shared__ u32 cf[16];
    __shared__ u32 wh[NW][256]; // per wave: no two waves meet in a word
    extern __shared__ __attribute__((aligned(16))) u8 smem[];
    const SquareDesc d = descs[blockIdx.x];
    const int n = d.w * d.h;
    u8* g = smem;
    u16* hb = (u16*)(smem + ((n + 15) & ~15));
    if (threadIdx.x < 16) cf[threadIdx.x] = cb.cf[threadIdx.x];
    for (int i = threadIdx.x; i < NW * 256; i += NT) (&wh[0][0])[i] = 0u;
    stage_gray_bgr<NT>(src + (size_t)blockIdx.z * src_frame_stride + d.src_off, d, g);
    __syncthreads();
    const u8* cp = calib + d.plane_off;
    u32* mine = wh[threadIdx.x >> 6];
    change_blur_passes<NT>(d, g, hb, cb.k, cf, [&](int i, int gv) { hist_add(mine, abs(gv - (int)cp[i])); });
    __syncthreads();
    u16* o = out + (size_t)blockIdx.z * out_frame_stride + (size_t)blockIdx.x * 256;
    for (int b = threadIdx.x; b < 256; b += NT) {
        u32 s = 0;
#pragma unroll
        for (int k = 0; k < NW; k++) s += wh[k][b];
        o[b] = (u16)s;
    }
}

#define SWEEP_EVAL_WAVES 4 // waves of a workgroup: they share the suffix sums and split the workgroup's settings
__global__ __launch_bounds__(64 * SWEEP_EVAL_WAVES) void k_sweep_eval(const u16* __restrict__ hist, int nk, const SquareDesc* __restrict__ descs,
                                                                      int n, const SweepSet* __restrict__ sets, const int* __restrict__ k_begin,
                                                                      cbv_sweep_record* __restrict__ rec, int rec_stride,
                                                                      cbv_sweep_summary* __restrict__ sums)
{
    // suf[d][square] = pixels of the square with a difference >= d, d = 0..256 (row 256 = 0): lanes read their own column
    __shared__ u16 suf[257 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, frame = blockIdx.x, ki = blockIdx.y;
    // this workgroup's slice of the kernel's settings
    const int kb = k_begin[ki], ke = k_begin[ki + 1];
    const int per = (ke - kb + (int)gridDim.z - 1) / (int)gridDim.z;
    const int g0 = kb + (int)blockIdx.z * per, g1 = min(ke, g0 + per);
    if (g0 >= g1) return;
    const u16* H = hist + ((size_t)frame * nk + ki) * SWEEP_HIST_WORDS;
    // lane = square here too: 8 bytes of its row per step (the rows' cache lines serve 16 steps), and the 64 lanes write
    // 64 consecutive u16 of an LDS row
    for (int c = wave; c < 64; c += SWEEP_EVAL_WAVES) {
        ushort4 v = make_ushort4(0, 0, 0, 0);
        if (lane < n) v = *(const ushort4*)(H + lane * 256 + c * 4);
        suf[(c * 4 + 0) * 64 + lane] = v.x;
        suf[(c * 4 + 1) * 64 + lane] = v.y;
        suf[(c * 4 + 2) * 64 + lane] = v.z;
        suf[(c * 4 + 3) * 64 + lane] = v.w;
    }
    if (wave == 0) suf[256 * 64 + lane] = 0;
    __syncthreads();
    const u32 npx = lane < n ? (u32)(descs[lane].w * descs[lane].h) : 0u;
    int dmax = 0; // the highest occupied bin: the square's z_max is z(dmax)
    u32 run = 0;
    for (int dd = 255; dd >= 0; dd--) { // (every wave walks the column for dmax; wave 0 turns it into the sums)
        const u32 hv = suf[dd * 64 + lane];
        if (run == 0 && hv != 0) dmax = dd;
        run += hv;
    }
    __syncthreads();
    if (wave == 0) {
        run = 0;
        for (int dd = 255; dd >= 0; dd--) {
            run += suf[dd * 64 + lane];
            suf[dd * 64 + lane] = (u16)run; // <= 16384
        }
    }
    __syncthreads();
    const int wper = (g1 - g0 + SWEEP_EVAL_WAVES - 1) / SWEEP_EVAL_WAVES;
    const int s0 = g0 + wave * wper, s1 = min(g1, s0 + wper);
    for (int si = s0; si < s1; si++) {
        const SweepSet st = sets[si];
        const float sd = sweep_sd(st.ivf);
        // z(d) does not fall as d grows, so the differences over the threshold are the bins from a cut on
        int over = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) over += __builtin_popcountll(__ballot(sweep_z(lane + 64 * j, sd) > st.zt));
        const int cut = 256 - over;
        const int cls = lane < n ? sweep_class(suf[cut * 64 + lane], npx) : 0;
        const u64 changed = __ballot(cls != 0), parcial = __ballot(cls == 2), total = __ballot(cls == 3);
        const float zmax = wave_max_f32(cls != 0 ? sweep_z(dmax, sd) : 0.f);
        if (lane == 0) {
            const cbv_sweep_record r = sweep_record(changed, parcial, total, zmax);
            if (rec) rec[(size_t)st.index * rec_stride + frame] = r;
            if (sums && r.n_changed) { // a frame that reports nothing adds nothing
                cbv_sweep_summary* S = sums + st.index;
                atomicAdd(&S->frames_changed, 1u);
                if (r.flags & CBV_SWEEP_HAND) atomicAdd(&S->frames_hand, 1u);
                if (r.flags & CBV_SWEEP_MOVE) atomicAdd(&S->frames_move, 1u);
                if (r.lifted >= 0) atomicAdd(&S->frames_lifted, 1u);
                atomicAdd(&S->squares_reported, (u32)r.n_changed);
                atomicMax((u32*)&S->z_max, __float_as_uint(zmax)); // z >= 0: the bit patterns order as the values do
            }
        }
    }
}

} // namespace

int launch_change_hist(cbv_ctx* ctx, const u8* src, size_t src_frame_stride, const SquareDesc* descs, int n, const u8* calib, u16* out,
                       size_t out_frame_stride, int batch, const ChangeBlur& cb, int max_px)
{
    hipLaunchKernelGGL((k_change_hist<256>), dim3(n, 1, batch), dim3(256), change_blur_lds(max_px), ctx->stream, src, src_frame_stride, descs,
                       calib, out, out_frame_stride, cb);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

int launch_sweep_eval(cbv_ctx* ctx, const u16* hist, int nk, const SquareDesc* descs, int n, const SweepSet* sets, const int* k_begin,
                      int max_per_k, int frames, cbv_sweep_record* rec, int rec_stride, cbv_sweep_summary* sums)
{
    // slices of a kernel's settings: enough workgroups to fill the chip (four fit a CU's LDS), at least 64 settings a wave (a
    // workgroup's suffix sums cost about as much as that many settings)
    int parts = (4 * ctx->num_cus + frames * nk - 1) / (frames * nk);
    parts = std::max(1, std::min(parts, (max_per_k + 64 * SWEEP_EVAL_WAVES - 1) / (64 * SWEEP_EVAL_WAVES)));
    hipLaunchKernelGGL(k_sweep_eval, dim3(frames, nk, parts), dim3(64 * SWEEP_EVAL_WAVES), 0, ctx->stream, hist, nk, descs, n, sets, k_begin, rec, rec_stride, sums);
    CBV_HIP(ctx, hipGetLastError());
    return CBV_OK;
}

// the host twin of k_sweep_eval: the same suffix sums, cut and classes (sweep_core.h), one frame
extern "C" int cbv_sweep_eval_host(const uint16_t* hist, const int32_t* n_px, int n, const cbv_sweep_setting* s, int ns, cbv_sweep_record* out)
{
    if (!hist || !n_px || n <= 0 || n > CBV_MAX_SQUARES || !s || ns <= 0 || !out) return CBV_ERR_ARG;
    for (int i = 0; i < n; i++)
        if (n_px[i] <= 0) return CBV_ERR_ARG;
    for (int k = 0; k < ns; k++) {
        const float ivf = (float)s[k].initial_variance;
        if (!(ivf > 0.f) || !std::isfinite(ivf)) return CBV_ERR_ARG;
    }
    std::vector<u32> suf((size_t)n * 257);
    int dmax[CBV_MAX_SQUARES];
    for (int i = 0; i < n; i++) {
        u32 run = 0;
        dmax[i] = 0;
        suf[(size_t)i * 257 + 256] = 0;
        for (int d = 255; d >= 0; d--) {
            const u32 hv = hist[(size_t)i * 256 + d];
            if (run == 0 && hv != 0) dmax[i] = d;
            run += hv;
            suf[(size_t)i * 257 + d] = run;
        }
    }
    for (int k = 0; k < ns; k++) {
        const float zt = (float)s[k].z_threshold, sd = sweep_sd((float)s[k].initial_variance);
        int over = 0;
        for (int d = 0; d < 256; d++) over += sweep_z(d, sd) > zt ? 1 : 0;
        const int cut = 256 - over;
        u64 changed = 0, parcial = 0, total = 0;
        float zmax = 0.f;
        for (int i = 0; i < n; i++) {
            const int cls = sweep_class(suf[(size_t)i * 257 + cut], (u32)n_px[i]);
            if (!cls) continue;
            changed |= 1ull << i;
            if (cls == 2) parcial |= 1ull << i;
            if (cls == 3) total |= 1ull << i;
            zmax = fmaxf(zmax, sweep_z(dmax[i], sd));
        }
        out[k] = sweep_record(changed, parcial, total, zmax);
    }
    return CBV_OK;
}
