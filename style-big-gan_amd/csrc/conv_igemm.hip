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
// What this file holds: the entry point sbg_conv2d_igemm, which offers every launch to the specialised kernels first (conv_thin.hip,
// conv_up2.hip, conv_k64.hip), and the kernel described above as the generic fallback -- operands of 2 GiB or more and negative strides,
// which the buffer descriptors of the LDS-DMA kernels cannot address.
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

template <class MF, int BC, int BP, int WGC, int WGP>
static int launch_conv(ConvArgs& a, hipStream_t stream)
{
    a.ptiles = (a.P + BP - 1) / BP;
    a.ctiles = (a.Cout + BC - 1) / BC;
    constexpr int lds = 2 * (4 * BC * 16 + 4 * BP * 16);
    return conv_launch<conv_igemm_kernel<MF, BC, BP, WGC, WGP>>((int64_t)a.ptiles * a.ctiles, 1, 256, lds, stream, 2.0 * a.P * a.Cout * (double)a.Cin * a.ntaps,
                                                                conv_prof_bytes(a, a.P), {a.P, a.Cout, a.Cin, a.ntaps, a.stride, a.OH, BC * 1000 + BP}, a);
}

// tile choice: few output channels -> pixel-heavy tile; otherwise 128 x 128.
template <class MF>
static int dispatch_conv(ConvArgs& a, hipStream_t stream)
{
    if (a.Cout <= 64)  return launch_conv<MF, 64, 256, 1, 4>(a, stream);
    return launch_conv<MF, 128, 128, 2, 2>(a, stream);
}

} // namespace

// Smallest tile count for which a transposed convolution runs as ONE multi-phase launch.  256 -> 16: the 4x4 .. 32x32 up-sampling layers
// as one launch instead of four latency-bound ones (-1.4 ms per step).
static constexpr int kPhaseMinTiles = 16;

extern "C" int sbg_conv2d_igemm(const sbg_conv_params* q, sbg_stream_t stream)
{
    SBG_CHECK(q && q->x && q->w && q->y, "conv2d_igemm: null pointer");
    SBG_CHECK(q->xdtype == SBG_BF16 || q->xdtype == SBG_F16, "conv2d_igemm: x/w must be bf16 or f16 (fp32 inputs are split by the host)");
    SBG_CHECK(q->ydtype == SBG_F32 || q->ydtype == SBG_BF16 || q->ydtype == SBG_F16, "conv2d_igemm: bad output dtype");
    SBG_CHECK(q->N >= 0 && q->IH >= 1 && q->IW >= 1 && q->OH >= 1 && q->OW >= 1 && q->Cin >= 8 && q->Cout >= 1, "conv2d_igemm: bad sizes");
    SBG_CHECK((q->Cin % 8) == 0, "conv2d_igemm: Cin must be a multiple of 8 (pad on the host)");
    SBG_CHECK(q->ntaps >= 1 && q->ntaps <= SBG_MAX_TAPS, "conv2d_igemm: 1..%d taps", SBG_MAX_TAPS);
    SBG_CHECK(q->stride >= 1, "conv2d_igemm: stride must be >= 1");
    SBG_CHECK(!q->accumulate || q->ydtype == SBG_F32, "conv2d_igemm: accumulate needs an fp32 output");
    SBG_CHECK(q->ksplit <= 1 || q->workspace != nullptr, "conv2d_igemm: ksplit > 1 needs a workspace");
    SBG_CHECK(q->act == 0 || q->act == SBG_ACT_LINEAR || q->act == SBG_ACT_RELU || q->act == SBG_ACT_LRELU, "conv2d_igemm: fused activation must be linear, relu or lrelu");
    SBG_CHECK(sbg_aligned16(q->x) && sbg_aligned16(q->w), "conv2d_igemm: x and w must be 16-byte aligned");
    SBG_CHECK((q->xs_n % 8) == 0 && (q->xs_h % 8) == 0 && (q->xs_w % 8) == 0 && (q->ws_slab % 8) == 0 && (q->ws_co % 8) == 0,
              "conv2d_igemm: pixel / row strides must be multiples of 8 elements");
    const int64_t P = (int64_t)q->N * q->OH * q->OW;
    SBG_CHECK(P <= INT32_MAX, "conv2d_igemm: too many output pixels");
    if (P == 0) return SBG_OK;

    ConvArgs a;
    a.x = (const unsigned short*)q->x; a.w = (const unsigned short*)q->w; a.y = q->y; a.oscale = q->oscale;
    a.bias = q->bias; a.noise = q->noise; a.noise_sn = q->noise_stride_n;
    a.act = q->act; a.alpha = q->alpha; a.gain = (q->act == 0 && q->gain == 0.f) ? 1.f : q->gain; a.clamp = (q->act == 0 && q->clamp == 0.f && q->gain == 0.f) ? -1.f : q->clamp;
    a.ydtype = q->ydtype;
    a.N = q->N; a.IH = q->IH; a.IW = q->IW; a.Cin = q->Cin; a.Cout = q->Cout; a.OH = q->OH; a.OW = q->OW;
    a.xs_n = q->xs_n; a.xs_h = q->xs_h; a.xs_w = q->xs_w; a.ys_n = q->ys_n; a.ys_h = q->ys_h; a.ys_w = q->ys_w;
    a.ws_slab = q->ws_slab; a.ws_co = q->ws_co;
    a.stride = q->stride; a.ntaps = q->ntaps;
    for (int t = 0; t < SBG_MAX_TAPS; t++) { a.tap_dy[t] = q->tap_dy[t]; a.tap_dx[t] = q->tap_dx[t]; a.tap_slab[t] = q->tap_slab[t]; }
    a.accumulate = q->accumulate;
    a.P = (int)P; a.ptiles = a.ctiles = 0; a.lds_params = 0; a.ksplit = 1; a.y_split_stride = 0;
    a.nphase = 1; a.ph_rot_div = 1;
    for (int i = 0; i < 4; i++) { a.ph_tap0[i] = 0; a.ph_ntaps[i] = 0; a.ph_OH[i] = 0; a.ph_OW[i] = 0; a.ph_P[i] = 0; a.ph_yoff[i] = 0; }
    hipStream_t s = (hipStream_t)stream;
    int maxslab = 0;
    for (int t = 0; t < q->ntaps; t++) { SBG_CHECK(q->tap_slab[t] >= 0, "conv2d_igemm: negative weight slab"); if (q->tap_slab[t] > maxslab) maxslab = q->tap_slab[t]; }
    const int64_t x_bytes = 2 * ((int64_t)(q->N - 1) * q->xs_n + (int64_t)(q->IH - 1) * q->xs_h + (int64_t)(q->IW - 1) * q->xs_w + q->Cin);
    const int64_t w_bytes = 2 * ((int64_t)maxslab * q->ws_slab + (int64_t)(q->Cout - 1) * q->ws_co + q->Cin);
    const bool fwd_strides = q->xs_n >= 0 && q->xs_h >= 0 && q->xs_w >= 0 && q->ws_slab >= 0 && q->ws_co >= 0;
    if (q->nphase > 1) {
        // phases: one persistent launch when the shape fits that kernel, otherwise one launch per phase through this same entry point
        SBG_CHECK(q->nphase <= 4, "conv2d_igemm: at most 4 phases");
        SBG_CHECK(conv_is_plain(*q) && (q->ksplit <= 1), "conv2d_igemm: phases exclude the fused epilogue and the K split");
        int t0 = 0; int64_t ptot = 0;
        for (int i = 0; i < q->nphase; i++) {
            SBG_CHECK(q->ph_ntaps[i] >= 1 && q->ph_oh[i] >= 1 && q->ph_ow[i] >= 1, "conv2d_igemm: bad phase %d", i);
            a.ph_tap0[i] = t0; a.ph_ntaps[i] = q->ph_ntaps[i]; a.ph_OH[i] = q->ph_oh[i]; a.ph_OW[i] = q->ph_ow[i];
            a.ph_P[i] = q->N * q->ph_oh[i] * q->ph_ow[i]; a.ph_yoff[i] = q->ph_yoff[i];
            t0 += q->ph_ntaps[i]; ptot += a.ph_P[i];
        }
        SBG_CHECK(t0 <= q->ntaps, "conv2d_igemm: phases use %d taps, %d given", t0, q->ntaps);
        {   // few channels: one streaming launch over all phases (conv_thin.hip)
            a.nphase = q->nphase;
            const int rc = sbg_conv_thin_dispatch(a, q->xdtype == SBG_BF16, s);
            if (rc >= 0) return rc;
            a.nphase = 1;
        }
        if (fwd_strides && q->nphase == 4) {      // stride-2 3x3 transposed convolution: every phase from one staged halo (conv_up2.hip), then its border
            a.nphase = 4;
            if (sbg_conv_up2_canonical_taps(a, x_bytes, w_bytes)) {      // (from here on `a` lists every phase's taps by (dy, dx), whichever kernel runs)
                sbg_conv_params border;
                const int rc = sbg_conv_up2_dispatch(a, q->xdtype == SBG_BF16, x_bytes, w_bytes, &border, q, s);
                if (rc > 0) return rc;
                if (rc == SBG_OK) return border.nphase > 0 ? sbg_conv2d_igemm(&border, stream) : SBG_OK;
            }
            a.nphase = 1;
        }
        const int64_t tiles = ((ptot / q->nphase + 255) / 256) * q->nphase * ((q->Cout + 127) / 128);
        if (fwd_strides && q->Cout > 64 && tiles >= kPhaseMinTiles && x_bytes < (int64_t)SBG_OOB_OFFSET && w_bytes < (int64_t)SBG_OOB_OFFSET) {
            a.nphase = q->nphase;
            const int rc = sbg_conv_k64_dispatch(a, q->xdtype == SBG_BF16, x_bytes, w_bytes, nullptr, 1, s);
            if (rc >= 0) return rc;
            a.nphase = 1;
        }
        for (int i = 0; i < q->nphase; i++) {
            sbg_conv_params one = *q;
            one.nphase = 0; one.OH = q->ph_oh[i]; one.OW = q->ph_ow[i]; one.ntaps = q->ph_ntaps[i];
            one.y = (char*)q->y + q->ph_yoff[i] * (q->ydtype == SBG_F32 ? 4 : 2);
            for (int t = 0; t < one.ntaps; t++) { one.tap_dy[t] = q->tap_dy[a.ph_tap0[i] + t]; one.tap_dx[t] = q->tap_dx[a.ph_tap0[i] + t]; one.tap_slab[t] = q->tap_slab[a.ph_tap0[i] + t]; }
            const int rc = sbg_conv2d_igemm(&one, stream);
            if (rc != SBG_OK) return rc;
        }
        return SBG_OK;
    }
    if (q->ksplit <= 1) {   // few channels on both sides: the streaming kernel of conv_thin.hip
        const int rc = sbg_conv_thin_dispatch(a, q->xdtype == SBG_BF16, s);
        if (rc >= 0) return rc;
    }
    if (fwd_strides) {    // K-step-64 kernels (conv_k64.hip) take every launch whose operands fit a 2 GiB buffer descriptor
        const int rc = sbg_conv_k64_dispatch(a, q->xdtype == SBG_BF16, x_bytes, w_bytes, q->workspace, q->ksplit, s);
        if (rc >= 0) return rc;
    }
    if (q->xdtype == SBG_BF16) return dispatch_conv<bf16_mfma>(a, s);
    return dispatch_conv<f16_mfma>(a, s);
}
