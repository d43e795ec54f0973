// conv_igemm.hip -- implicit-GEMM convolution on the gfx950 matrix cores (v_mfma_f32_16x16x32_{bf16,f16}).
//
// One kernel serves forward convolution, data gradient (a convolution with flipped / transposed weights) and each of
// the four sub-pixel phases of a stride-2 transposed convolution: the host describes the launch as a tap list
//     y[n, oy*ysh + .., ox*ysw + .., co] (+)= sum_t sum_ci x[n, oy*stride + dy[t], ox*stride + dx[t], ci] * w[slab[t]][co][ci]
// (see include/sbg_hip.h).  This replaces the cuDNN calls behind conv2d_gradfix.conv2d / conv_transpose2d
// (stylegan2ada/torch_utils/ops/conv2d_gradfix.py:107-137).
//
// GEMM view: D[co][pixel] = sum_k W[co][k] * X[k][pixel], k = (tap, ci).  The weights are the MFMA A operand and the
// gathered activations the B operand, so a lane ends up holding 4 consecutive output channels of one pixel -- a
// contiguous 8-B (bf16) / 16-B (fp32) channel-minor store.
//
// Workgroup = 256 lanes = 4 waves (64-wide), tile BC output channels x BP output pixels, K-step 32 (one MFMA deep).
// Activations are channel-minor, so for a fixed tap the 32-channel slice of a pixel is 64 contiguous bytes: every lane
// stages 16-B pieces global -> VGPR -> LDS (issue early / write late, 2 LDS stages, one barrier per K-step).
// LDS image per operand: [k-group g = 0..3][row][8 x 16-bit] (16-B cells).  A ds_read_b128 of MFMA fragments touches 16
// rows that are distinct mod 16 -> 16 distinct 16-B slots of the 256-B bank row: conflict-free; the staging writes put 8
// consecutive rows of one k-group in each 8-lane store group: 128 contiguous bytes, conflict-free.
//
// What this file holds: the kernel described above, which is the generic fallback -- operands of 2 GiB or more and negative strides, which
// the buffer descriptors of the LDS-DMA kernels cannot address -- and the host side of the family: conv_plan decides everything about a call
// once (which kernels, tiles, grids, K split, tap order, profiler records; it asks conv_thin.hip, conv_up2.hip and conv_k64.hip whether a
// launch fits them), and the three entry points read it: sbg_conv2d_igemm launches what it lists, sbg_conv2d_igemm_workspace returns the size of
// the split it chose, sbg_conv2d_igemm_plan prints it.
#include "conv_device.h"

using namespace sbgconv;

namespace {

// lane -> (row within a 16-row staging group, k-group): 8 consecutive lanes share a k-group and walk 8 rows.
static __device__ __forceinline__ int stage_row16(int lane) { return (lane & 7) | ((lane >> 5) << 3); }
static __device__ __forceinline__ int stage_kgrp(int lane)  { return (lane >> 3) & 3; }

// Epilogue: lane holds channels c0 + wc + 16 i + 4 fg + {0..3} of pixel p0 + wp + 16 j + fr.
template <int TC, int TP>
static __device__ __forceinline__ void conv_epilogue(const ConvArgs& p, float4_t (&acc)[TC][TP], int c0, int p0, int wc, int wp, int fr, int fg)
{
    // per-channel terms depend on the channel tile only: fetch them once (16-B loads when the 4 channels are in range)
    float4_t bias4[TC];
    bool full4[TC];
#pragma unroll
    for (int i = 0; i < TC; i++) {
        const int co = c0 + wc + 16 * i + 4 * fg;
        full4[i] = (co + 4 <= p.Cout);
        bias4[i] = float4_t{0.f, 0.f, 0.f, 0.f};
        if (p.bias) {
#pragma unroll
            for (int e = 0; e < 4; e++) if (co + e < p.Cout) bias4[i][e] = p.bias[co + e];
        }
    }
    const bool plain = conv_is_plain(p);
#pragma unroll
    for (int j = 0; j < TP; j++) {
        const int pix = p0 + wp + 16 * j + fr;
        if (pix >= p.P) continue;
        const int ox = pix % p.OW, t = pix / p.OW, oy = t % p.OH, n = t / p.OH;
        const int64_t yoff = (int64_t)n * p.ys_n + (int64_t)oy * p.ys_h + (int64_t)ox * p.ys_w;
        const float nz = (!plain && p.noise) ? p.noise[(int64_t)n * p.noise_sn + (int64_t)oy * p.OW + ox] : 0.f;
#pragma unroll
        for (int i = 0; i < TC; i++) {
            const int co = c0 + wc + 16 * i + 4 * fg;
            if (co >= p.Cout) continue;
            float4_t v = acc[i][j];
            if (!plain) {
#pragma unroll
                for (int e = 0; e < 4; e++) if (co + e < p.Cout) v[e] = tail(p, v[e], (int64_t)n * p.Cout + co + e, nz + bias4[i][e]);
            }
            const bool full = full4[i];
            if (p.ydtype == SBG_F32) {
                float* dst = (float*)p.y + yoff + co;
                if (full && ((((uintptr_t)dst) & 15) == 0)) {
                    float4_t o = v;
                    if (p.accumulate) { float4_t old = *reinterpret_cast<float4_t*>(dst); o += old; }
                    *reinterpret_cast<float4_t*>(dst) = o;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++) if (co + e < p.Cout) dst[e] = p.accumulate ? dst[e] + v[e] : v[e];
                }
            } else {
                unsigned short* dst = (unsigned short*)p.y + yoff + co;
                unsigned short h[4];
#pragma unroll
                for (int e = 0; e < 4; e++) h[e] = (p.ydtype == SBG_BF16) ? f32_to_bf16_bits(v[e]) : f32_to_f16_bits(v[e]);
                if (full && ((((uintptr_t)dst) & 7) == 0)) {
                    short4_t o = {(short)h[0], (short)h[1], (short)h[2], (short)h[3]};
                    *reinterpret_cast<short4_t*>(dst) = o;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++) if (co + e < p.Cout) dst[e] = h[e];
                }
            }
        }
    }
}

template <class MF, int BC, int BP, int WGC, int WGP>
__global__ __launch_bounds__(256) void conv_igemm_kernel(ConvArgs p)
{
    static_assert(WGC * WGP == 4, "4 waves per workgroup");
    constexpr int WC = BC / WGC, WP = BP / WGP;        // wave tile
    constexpr int TC = WC / 16,  TP = WP / 16;         // 16x16 MFMA tiles per wave
    constexpr int RA = BC / 64,  RB = BP / 64;         // staging rows per lane (16 rows per wave-instruction, 4 waves)
    static_assert(BC % 64 == 0 && BP % 64 == 0, "tile must be a multiple of 64");

    // LDS: 2 stages x { A [4][BC] cells, B [4][BP] cells }, cell = 16 B.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int A_BYTES = 4 * BC * 16, B_BYTES = 4 * BP * 16, STAGE = A_BYTES + B_BYTES;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bid = xcd_tile_order(blockIdx.x, gridDim.x);
    const int ct = bid % p.ctiles, pt = bid / p.ctiles;
    const int c0 = ct * BC, p0 = pt * BP;

    // ---- per-lane staging coordinates -------------------------------------------------------------------------
    const int srow = wave * 16 + stage_row16(lane), sg = stage_kgrp(lane);
    // B operand rows = output pixels: decode (n, oy, ox) once.
    int  b_iy0[RB], b_ix0[RB]; int64_t b_base[RB]; bool b_ok[RB];
#pragma unroll
    for (int i = 0; i < RB; i++) {
        const int pix = p0 + srow + 64 * i;
        b_ok[i] = pix < p.P;
        const int pp = b_ok[i] ? pix : 0;
        const int ox = pp % p.OW, t = pp / p.OW, oy = t % p.OH, n = t / p.OH;
        b_iy0[i] = oy * p.stride; b_ix0[i] = ox * p.stride; b_base[i] = (int64_t)n * p.xs_n;
    }
    // A operand rows = output channels.
    int64_t a_off[RA]; bool a_ok[RA];
#pragma unroll
    for (int i = 0; i < RA; i++) {
        const int co = c0 + srow + 64 * i;
        a_ok[i] = co < p.Cout;
        a_off[i] = (int64_t)(a_ok[i] ? co : 0) * p.ws_co;
    }

    const int kchunks = (p.Cin + 31) >> 5;
    const int nsteps = p.ntaps * kchunks;

    short8_t ra[RA], rb[RB];
    auto issue_loads = [&](int step) {
        const int t = step / kchunks, ck = (step - t * kchunks) * 32 + sg * 8;
        const bool kok = ck < p.Cin;
        const int dy = p.tap_dy[t], dx = p.tap_dx[t];
        const unsigned short* wslab = p.w + (int64_t)p.tap_slab[t] * p.ws_slab + ck;
#pragma unroll
        for (int i = 0; i < RA; i++) {
            short8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (kok && a_ok[i]) v = *reinterpret_cast<const short8_t*>(wslab + a_off[i]);
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < RB; i++) {
            const int iy = b_iy0[i] + dy, ix = b_ix0[i] + dx;
            short8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (kok && b_ok[i] && (unsigned)iy < (unsigned)p.IH && (unsigned)ix < (unsigned)p.IW)
                v = *reinterpret_cast<const short8_t*>(p.x + b_base[i] + (int64_t)iy * p.xs_h + (int64_t)ix * p.xs_w + ck);
            rb[i] = v;
        }
    };
    auto write_stage = [&](int buf) {
        unsigned char* sa = smem + buf * STAGE;
        unsigned char* sb = sa + A_BYTES;
#pragma unroll
        for (int i = 0; i < RA; i++) *reinterpret_cast<short8_t*>(sa + (sg * BC + srow + 64 * i) * 16) = ra[i];
#pragma unroll
        for (int i = 0; i < RB; i++) *reinterpret_cast<short8_t*>(sb + (sg * BP + srow + 64 * i) * 16) = rb[i];
    };

    // ---- MFMA coordinates ---------------------------------------------------------------------------------------
    const int wc = (wave / WGP) * WC, wp = (wave % WGP) * WP;
    const int fr = lane & 15, fg = lane >> 4;
    float4_t acc[TC][TP];
#pragma unroll
    for (int i = 0; i < TC; i++)
#pragma unroll
        for (int j = 0; j < TP; j++) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};

    issue_loads(0);
    write_stage(0);
    __syncthreads();
    for (int s = 0; s < nsteps; s++) {
        const int buf = s & 1;
        if (s + 1 < nsteps) issue_loads(s + 1);
        const unsigned char* sa = smem + buf * STAGE;
        const unsigned char* sb = sa + A_BYTES;
        short8_t fa[TC], fb[TP];
#pragma unroll
        for (int i = 0; i < TC; i++) fa[i] = *reinterpret_cast<const short8_t*>(sa + (fg * BC + wc + 16 * i + fr) * 16);
#pragma unroll
        for (int j = 0; j < TP; j++) fb[j] = *reinterpret_cast<const short8_t*>(sb + (fg * BP + wp + 16 * j + fr) * 16);
#pragma unroll
        for (int i = 0; i < TC; i++)
#pragma unroll
            for (int j = 0; j < TP; j++) acc[i][j] = Mfma<MF>::run(fa[i], fb[j], acc[i][j]);
        if (s + 1 < nsteps) write_stage(buf ^ 1);
        __syncthreads();
    }

    conv_epilogue<TC, TP>(p, acc, c0, p0, wc, wp, fr, fg);
}

template <class MF>
static int launch_generic(const ConvLaunch& l, hipStream_t stream)
{
    if (l.bc == 64) return conv_launch<conv_igemm_kernel<MF, 64, 256, 1, 4>>(l, stream);
    return conv_launch<conv_igemm_kernel<MF, 128, 128, 2, 2>>(l, stream);
}

// tile choice: few output channels -> pixel-heavy tile; otherwise 128 x 128.
static void fit_generic(ConvLaunch& l)
{
    ConvArgs& a = l.a;
    l.family = CONV_GENERIC; l.bc = a.Cout <= 64 ? 64 : 128; l.bp = a.Cout <= 64 ? 256 : 128;
    a.ptiles = (a.P + l.bp - 1) / l.bp;
    a.ctiles = (a.Cout + l.bc - 1) / l.bc;
    l.grid_x = (int64_t)a.ptiles * a.ctiles; l.grid_y = 1; l.block = 256; l.lds = 2 * (4 * l.bc * 16 + 4 * l.bp * 16);
    conv_prof_phases(l, l.bc * 1000 + l.bp);
}

// Smallest tile count for which a transposed convolution runs as ONE multi-phase launch.  256 -> 16: the 4x4 .. 32x32 up-sampling layers
// as one launch instead of four latency-bound ones (-1.4 ms per step).
constexpr int kPhaseMinTiles = 16;

int conv_validate(const sbg_conv_params* q)
{
    SBG_CHECK(q && q->x && q->w && q->y, "conv2d_igemm: null pointer");
    SBG_CHECK(q->xdtype == SBG_BF16 || q->xdtype == SBG_F16, "conv2d_igemm: x/w must be bf16 or f16 (fp32 inputs are split by the host)");
    SBG_CHECK(q->ydtype == SBG_F32 || q->ydtype == SBG_BF16 || q->ydtype == SBG_F16, "conv2d_igemm: bad output dtype");
    SBG_CHECK(q->N >= 0 && q->IH >= 1 && q->IW >= 1 && q->OH >= 1 && q->OW >= 1 && q->Cin >= 8 && q->Cout >= 1, "conv2d_igemm: bad sizes");
    SBG_CHECK((q->Cin % 8) == 0, "conv2d_igemm: Cin must be a multiple of 8 (pad on the host)");
    SBG_CHECK(q->ntaps >= 1 && q->ntaps <= SBG_MAX_TAPS, "conv2d_igemm: 1..%d taps", SBG_MAX_TAPS);
    SBG_CHECK(q->stride >= 1, "conv2d_igemm: stride must be >= 1");
    SBG_CHECK(!q->accumulate || q->ydtype == SBG_F32, "conv2d_igemm: accumulate needs an fp32 output");
    SBG_CHECK(q->ksplit >= 0, "conv2d_igemm: ksplit must be 0 (the library chooses), 1 (never) or a cap");
    SBG_CHECK(q->act == 0 || q->act == SBG_ACT_LINEAR || q->act == SBG_ACT_RELU || q->act == SBG_ACT_LRELU, "conv2d_igemm: fused activation must be linear, relu or lrelu");
    SBG_CHECK(sbg_aligned16(q->x) && sbg_aligned16(q->w), "conv2d_igemm: x and w must be 16-byte aligned");
    SBG_CHECK((q->xs_n % 8) == 0 && (q->xs_h % 8) == 0 && (q->xs_w % 8) == 0 && (q->ws_slab % 8) == 0 && (q->ws_co % 8) == 0,
              "conv2d_igemm: pixel / row strides must be multiples of 8 elements");
    const int64_t P = (int64_t)q->N * q->OH * q->OW;
    SBG_CHECK(P <= INT32_MAX, "conv2d_igemm: too many output pixels");
    if (P == 0) return SBG_OK;                           // nothing to do (and nothing planned)
    for (int t = 0; t < q->ntaps; t++) SBG_CHECK(q->tap_slab[t] >= 0, "conv2d_igemm: negative weight slab");
    if (q->nphase > 1) {
        SBG_CHECK(q->nphase <= 4, "conv2d_igemm: at most 4 phases");
        SBG_CHECK(conv_is_plain(*q) && (q->ksplit <= 1), "conv2d_igemm: phases exclude the fused epilogue and the K split");
        int t0 = 0;
        for (int i = 0; i < q->nphase; i++) {
            SBG_CHECK(q->ph_ntaps[i] >= 1 && q->ph_oh[i] >= 1 && q->ph_ow[i] >= 1, "conv2d_igemm: bad phase %d", i);
            t0 += q->ph_ntaps[i];
        }
        SBG_CHECK(t0 <= q->ntaps, "conv2d_igemm: phases use %d taps, %d given", t0, q->ntaps);
    }
    return SBG_OK;
}

// the kernel argument block of the call as the caller described it
void conv_fill(const sbg_conv_params& q, ConvArgs& a)
{
    a.x = (const unsigned short*)q.x; a.w = (const unsigned short*)q.w; a.y = q.y; a.oscale = q.oscale;
    a.bias = q.bias; a.noise = q.noise; a.noise_sn = q.noise_stride_n;
    a.act = q.act; a.alpha = q.alpha; a.gain = (q.act == 0 && q.gain == 0.f) ? 1.f : q.gain; a.clamp = (q.act == 0 && q.clamp == 0.f && q.gain == 0.f) ? -1.f : q.clamp;
    a.ydtype = q.ydtype;
    a.N = q.N; a.IH = q.IH; a.IW = q.IW; a.Cin = q.Cin; a.Cout = q.Cout; a.OH = q.OH; a.OW = q.OW;
    a.xs_n = q.xs_n; a.xs_h = q.xs_h; a.xs_w = q.xs_w; a.ys_n = q.ys_n; a.ys_h = q.ys_h; a.ys_w = q.ys_w;
    a.ws_slab = q.ws_slab; a.ws_co = q.ws_co;
    a.stride = q.stride; a.ntaps = q.ntaps;
    for (int t = 0; t < SBG_MAX_TAPS; t++) { a.tap_dy[t] = q.tap_dy[t]; a.tap_dx[t] = q.tap_dx[t]; a.tap_slab[t] = q.tap_slab[t]; }
    a.accumulate = q.accumulate;
    a.P = q.N * q.OH * q.OW; a.ptiles = a.ctiles = 0; a.lds_params = 0; a.ksplit = 1; a.y_split_stride = 0;
    a.nphase = q.nphase > 1 ? q.nphase : 1; a.ph_rot_div = 1;
    for (int i = 0, t0 = 0; i < 4; i++) {
        const bool on = q.nphase > 1 && i < q.nphase;
        a.ph_tap0[i] = on ? t0 : 0; a.ph_ntaps[i] = on ? q.ph_ntaps[i] : 0; a.ph_OH[i] = on ? q.ph_oh[i] : 0; a.ph_OW[i] = on ? q.ph_ow[i] : 0;
        a.ph_P[i] = on ? q.N * q.ph_oh[i] * q.ph_ow[i] : 0; a.ph_yoff[i] = on ? q.ph_yoff[i] : 0;
        if (on) t0 += q.ph_ntaps[i];
    }
}

// The K split of a single launch that the K-step-64 kernels take: worth it when the output tiles alone leave most CUs idle and the reduction is
// long (the 4x4 fp32 block: 16 tiles x 432 K-steps; the 16-bit 4x4 .. 8x8 layers: 16-64 tiles x 72).  q.ksplit: 0 = as computed here, 1 = never,
// k = at most k.  The slabs need a dense channel-minor y; a plain fp32 sum may accumulate and have any channel count (the 513-channel data gradient
// of the discriminator's epilogue convolution); otherwise the reduction applies the epilogue / output cast, storing 16-B vectors of 8 channels
// (reduce_epi, which means something only when the result is > 1).
int conv_ksplit(const sbg_conv_params& q, const ConvArgs& a, bool have_ws, bool& reduce_epi)
{
    const bool dense_y = a.ys_w == a.Cout && a.ys_h == (int64_t)a.OW * a.Cout && a.ys_n == (int64_t)a.OH * a.OW * a.Cout;
    const bool simple = a.ydtype == SBG_F32 && conv_is_plain(a);
    const bool epi_ok = !a.accumulate && (a.Cout & 7) == 0 && sbg_aligned16(a.y);
    reduce_epi = !simple;
    if (!have_ws || q.ksplit == 1 || a.Cout <= 64 || !dense_y || !(simple || epi_ok)) return 1;
    const int64_t tiles = (int64_t)((a.P + 127) / 128) * ((a.Cout + 127) / 128);       // 128 x 128 output tiles
    const int ksteps = a.ntaps * ((a.Cin + 63) >> 6);
    if (tiles >= 128 || ksteps < 16) return 1;
    int k = (int)((256 + tiles - 1) / tiles);           // about 256 workgroups ...
    if (k > ksteps / 4) k = ksteps / 4;                 // ... of at least four K-steps each
    if (q.ksplit > 1 && k > q.ksplit) k = q.ksplit;
    return k < 2 ? 1 : k;
}

int push(ConvPlan& pl, const ConvLaunch& l)
{
    if (pl.nlaunch >= 5) return sbg_fail(SBG_ERR_INVALID, "conv2d_igemm: more than five launches");
    pl.launch[pl.nlaunch++] = l;
    return SBG_OK;
}

// Appends the launches of one (validated) call to the plan.  Pure host arithmetic.  Precedence: thin -> [phased: up2 (+ its border, planned as a
// call of its own) -> multi-phase gather -> every phase as a call of its own] -> K-step-64 kernels (sbg_conv_k64_fit has the tile order), with
// the K split -> generic.  have_ws: the caller has (or, for the size query, will have) a workspace for the K split.
int conv_plan_add(const sbg_conv_params& q, bool have_ws, ConvPlan& pl)
{
    if ((int64_t)q.N * q.OH * q.OW == 0) return SBG_OK;
    ConvLaunch l = {};
    ConvArgs& a = l.a;
    conv_fill(q, a);
    if (pl.nlaunch == 0) pl.call = a;
    int maxslab = 0;
    for (int t = 0; t < q.ntaps; t++) if (q.tap_slab[t] > maxslab) maxslab = q.tap_slab[t];
    const int64_t x_bytes = 2 * ((int64_t)(q.N - 1) * q.xs_n + (int64_t)(q.IH - 1) * q.xs_h + (int64_t)(q.IW - 1) * q.xs_w + q.Cin);
    const int64_t w_bytes = 2 * ((int64_t)maxslab * q.ws_slab + (int64_t)(q.Cout - 1) * q.ws_co + q.Cin);
    const bool fwd_strides = q.xs_n >= 0 && q.xs_h >= 0 && q.xs_w >= 0 && q.ws_slab >= 0 && q.ws_co >= 0;
    // LDS-DMA addressable: what the buffer descriptors of conv_up2.hip / conv_k64.hip can reach
    const bool dma = fwd_strides && x_bytes < (int64_t)SBG_OOB_OFFSET && w_bytes < (int64_t)SBG_OOB_OFFSET;
    l.x_bytes = (unsigned)x_bytes; l.w_bytes = (unsigned)w_bytes;
    if (q.nphase > 1) {
        if (fwd_strides && sbg_conv_thin_fit(l)) return push(pl, l);      // few channels: one streaming launch over all phases
        if (dma && q.nphase == 4) {      // stride-2 3x3 transposed convolution: every phase from one staged halo, then its border
            sbg_conv_params border;
            if (sbg_conv_up2_fit(l, q, border) == UP2_FITS) {
                const int rc = push(pl, l);
                return rc != SBG_OK || border.nphase == 0 ? rc : conv_plan_add(border, false, pl);
            }
        }
        int64_t ptot = 0;
        for (int i = 0; i < q.nphase; i++) ptot += a.ph_P[i];
        const int64_t tiles = ((ptot / q.nphase + 255) / 256) * q.nphase * ((q.Cout + 127) / 128);
        if (dma && q.Cout > 64 && tiles >= kPhaseMinTiles) { sbg_conv_k64_fit(l); return push(pl, l); }
        for (int i = 0; i < q.nphase; i++) {      // too few tiles, or operands only the generic kernel reaches: one call per phase (the caller's tap order)
            sbg_conv_params one = q;
            one.nphase = 0; one.ksplit = 1; one.OH = q.ph_oh[i]; one.OW = q.ph_ow[i]; one.ntaps = q.ph_ntaps[i];
            one.y = (char*)q.y + q.ph_yoff[i] * (q.ydtype == SBG_F32 ? 4 : 2);
            for (int t = 0; t < one.ntaps; t++) { one.tap_dy[t] = q.tap_dy[a.ph_tap0[i] + t]; one.tap_dx[t] = q.tap_dx[a.ph_tap0[i] + t]; one.tap_slab[t] = q.tap_slab[a.ph_tap0[i] + t]; }
            const int rc = conv_plan_add(one, false, pl);
            if (rc != SBG_OK) return rc;
        }
        return SBG_OK;
    }
    if (q.ksplit <= 1 && fwd_strides && sbg_conv_thin_fit(l)) return push(pl, l);      // few channels on both sides: the streaming kernel
    if (!dma) { fit_generic(l); return push(pl, l); }
    const int k = conv_ksplit(q, a, have_ws, pl.reduce_epi);
    if (k > 1) {       // the launch writes k raw fp32 slabs into the workspace; the reduction finishes the call
        pl.ksplit = k; pl.workspace_bytes = (int64_t)k * a.P * a.Cout * (int64_t)sizeof(float);
        a.y = q.workspace; a.accumulate = 0; a.ksplit = k; a.y_split_stride = (int64_t)a.P * a.Cout;
        a.ydtype = SBG_F32; a.act = SBG_ACT_LINEAR; a.gain = 1.f; a.clamp = -1.f; a.bias = nullptr; a.noise = nullptr; a.oscale = nullptr;
    }
    sbg_conv_k64_fit(l);
    return push(pl, l);
}

int conv_plan(const sbg_conv_params* q, bool have_ws, ConvPlan& pl)
{
    const int rc = conv_validate(q);
    if (rc != SBG_OK) return rc;
    pl.nlaunch = 0; pl.ksplit = 1; pl.reduce_epi = false; pl.workspace_bytes = 0;
    return conv_plan_add(*q, have_ws, pl);
}

} // namespace

extern "C" int64_t sbg_conv2d_igemm_workspace(const sbg_conv_params* q)
{
    ConvPlan pl;
    return conv_plan(q, true, pl) == SBG_OK ? pl.workspace_bytes : -1;
}

extern "C" int sbg_conv2d_igemm_plan(const sbg_conv_params* q, sbg_conv_launch_info* out, int max)
{
    ConvPlan pl;
    if (conv_plan(q, q && q->workspace, pl) != SBG_OK) return -1;
    for (int i = 0; i < pl.nlaunch && i < max && out; i++) {
        const ConvLaunch& l = pl.launch[i];
        for (int d = 0; d < 7; d++) out[i].dims[d] = l.dims[d];
        out[i].flops = l.flops; out[i].bytes = l.bytes;
        out[i].grid_x = l.grid_x; out[i].grid_y = (int)l.grid_y; out[i].block = (int)l.block; out[i].lds = l.lds;
    }
    return pl.nlaunch;
}

extern "C" int sbg_conv2d_igemm(const sbg_conv_params* q, sbg_stream_t stream)
{
    ConvPlan pl;
    int rc = conv_plan(q, q && q->workspace, pl);
    if (rc != SBG_OK) return rc;
    SBG_CHECK(q->ksplit <= 1 || q->workspace != nullptr, "conv2d_igemm: ksplit > 1 needs a workspace");
    hipStream_t s = (hipStream_t)stream;
    const bool bf16 = q->xdtype == SBG_BF16;
    for (int i = 0; i < pl.nlaunch && rc == SBG_OK; i++) {
        const ConvLaunch& l = pl.launch[i];
        switch (l.family) {
        case CONV_THIN:    rc = sbg_conv_thin_launch(l, bf16, s); break;
        case CONV_UP2:     rc = sbg_conv_up2_launch(l, bf16, s); break;
        case CONV_GENERIC: rc = bf16 ? launch_generic<bf16_mfma>(l, s) : launch_generic<f16_mfma>(l, s); break;
        default:           rc = sbg_conv_k64_launch(l, bf16, s); break;
        }
    }
    return rc != SBG_OK || pl.ksplit == 1 ? rc : sbg_conv_ksplit_reduce(pl.call, q->workspace, pl.ksplit, pl.reduce_epi, s);
}
