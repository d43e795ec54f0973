// biggan_ops.hip -- BigGAN-specific kernels: spectral-norm power iteration and the non-local self-attention core.
//
//  * sn_*: one power iteration of SN.W_ (biggan/layers.py:28-50,87-99) as two streaming passes over the fp32 weight matrix
//    (column sums, then row sums) with the normalisations and sigma folded into the small tail kernels.  HBM-bound:
//    2 * rows * cols * 4 bytes.
//  * attention_fwd_kernel: out = softmax(theta phi^T) g per sample (biggan/layers.py:162-166) on the fp32-input matrix cores
//    (v_mfma_f32_16x16x4_f32: bit-for-bit an fp32 fma chain, so parity with the fp32 reference is to rounding).  One wave
//    owns 16 query rows: S = Q K^T lives in accumulator registers, the row softmax runs on them (16-lane shuffles), P goes
//    through a 16 x M LDS strip to become the A operand of P V.  Keys <= 256 take these kernels: no online-softmax rescaling.
//  * attention_fwd_stream_kernel / attention_bwd_dq_stream_kernel: the same wave-per-16-queries structure for any number of keys,
//    walking them in chunks with a running (max, sum, output) per row; the [Q, M] map still never reaches HBM.
#include "sbg_common.h"
#include <type_traits>

namespace {

// ---------------------------------------------------------------------------------------------------------------- SN
#define SN_ROWS_PER_BLOCK 32

// partial[rb][k] = sum_{o in row block rb} u[o] * W[o][k]
__global__ __launch_bounds__(256) void sn_colsum_kernel(const float* W, const float* u, float* partial, int rows, int cols)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int r0 = blockIdx.y * SN_ROWS_PER_BLOCK;
    if (k >= cols) return;
    float acc = 0.f;
    const int r1 = (r0 + SN_ROWS_PER_BLOCK < rows) ? r0 + SN_ROWS_PER_BLOCK : rows;
    for (int o = r0; o < r1; o++) acc += u[o] * W[(int64_t)o * cols + k];
    partial[(int64_t)blockIdx.y * cols + k] = acc;
}

// v_raw[k] = sum_rb partial[rb][k]  (fixed order); block 0 also leaves |v_raw|^2 partial sums for the next kernel
__global__ __launch_bounds__(256) void sn_vfinish_kernel(const float* partial, float* v_raw, float* vnorm2_parts, int cols, int nrb)
{
    __shared__ float red[256];
    const int k = blockIdx.x * 256 + threadIdx.x;
    float acc = 0.f;
    if (k < cols) {
        for (int rb = 0; rb < nrb; rb++) acc += partial[(int64_t)rb * cols + k];
        v_raw[k] = acc;
    }
    red[threadIdx.x] = acc * acc;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) { if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    if (threadIdx.x == 0) vnorm2_parts[blockIdx.x] = red[0];
}

// one workgroup per row: t[o] = sum_k v_hat[k] W[o][k], v_hat = v_raw / max(|v_raw|, eps); also writes v (normalised) from row 0
__global__ __launch_bounds__(256) void sn_rowsum_kernel(const float* W, const float* v_raw, const float* vnorm2_parts, int nparts,
                                                         float* v_out, float* t, int rows, int cols, float eps)
{
    __shared__ float red[256];
    float n2 = 0.f;
    for (int i = 0; i < nparts; i++) n2 += vnorm2_parts[i];
    const float inv = 1.f / fmaxf(sqrtf(n2), eps);
    const int o = blockIdx.x;
    float acc = 0.f;
    for (int k = threadIdx.x; k < cols; k += 256) {
        const float vh = v_raw[k] * inv;
        if (o == 0) v_out[k] = vh;
        acc += vh * W[(int64_t)o * cols + k];
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) { if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    if (threadIdx.x == 0) t[o] = red[0];
}

// u_new = t / max(|t|, eps), sigma = t . u_new   (single workgroup)
__global__ __launch_bounds__(256) void sn_ufinish_kernel(const float* t, float* u_new, float* sigma, int rows, float eps)
{
    __shared__ float red[256];
    float acc = 0.f;
    for (int o = threadIdx.x; o < rows; o += 256) acc += t[o] * t[o];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) { if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    const float n2 = red[0];
    const float inv = 1.f / fmaxf(sqrtf(n2), eps);
    __syncthreads();
    float dot = 0.f;
    for (int o = threadIdx.x; o < rows; o += 256) { const float un = t[o] * inv; u_new[o] = un; dot += t[o] * un; }
    red[threadIdx.x] = dot;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) { if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    if (threadIdx.x == 0) sigma[0] = red[0];
}

// ---------------------------------------------------------------------------------------------------------------- attention
#define ATT_MAX_M 256

// The tile counts the attention kernels are instantiated for: 1, 2, 4, 8, 16, up to MAXT (M / 16 key tiles of the single-chunk kernels, DV / 16
// output tiles, ceil(D / 16) column tiles with MAXT = 4).  This switch is the only list of them: the launchers dispatch through it and the
// shape predicates ask it (att_tiles_dispatched), so a shape the predicates accept is a shape the launchers serve.
// f(std::integral_constant<int, T>) -> status; ATT_NO_TILES for a count that has no instantiation.
#define ATT_NO_TILES (-1)
template <int MAXT, class F>
static int att_for_tiles(int tiles, F&& f)
{
    switch (tiles) {
        case 1:  return f(std::integral_constant<int, 1>{});
        case 2:  if constexpr (MAXT >= 2) return f(std::integral_constant<int, 2>{}); else return ATT_NO_TILES;
        case 4:  if constexpr (MAXT >= 4) return f(std::integral_constant<int, 4>{}); else return ATT_NO_TILES;
        case 8:  if constexpr (MAXT >= 8) return f(std::integral_constant<int, 8>{}); else return ATT_NO_TILES;
        case 16: if constexpr (MAXT >= 16) return f(std::integral_constant<int, 16>{}); else return ATT_NO_TILES;
        default: return ATT_NO_TILES;
    }
}
template <int MAXT>
static bool att_tiles_dispatched(int tiles) { return att_for_tiles<MAXT>(tiles, [](auto) { return (int)SBG_OK; }) == SBG_OK; }

template <int MT>   // MT = M / 16 key tiles held in accumulators
__global__ __launch_bounds__(256) void attention_fwd_kernel(const float* theta, const float* phi, const float* g, float* out,
                                                            int Q, int M, int D, int DV)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.y;
    const int q0 = (blockIdx.x * 4 + wave) * 16;            // this wave's 16 query rows
    float* P = reinterpret_cast<float*>(smem) + wave * 16 * (ATT_MAX_M + 4);   // 16 x M strip (row pitch M + 4: conflict-free column reads)
    const int pitch = ATT_MAX_M + 4;
    if (q0 >= Q) return;                                     // whole wave out of range (Q % 16 == 0)
    const float* Qp = theta + ((int64_t)n * Q + q0) * D;
    const float* Kp = phi + (int64_t)n * M * D;
    const float* Vp = g + (int64_t)n * M * DV;
    const int fr = lane & 15, fk = lane >> 4;                // A: row fr, k = fk ; B: k = fk, col fr ; C: col fr, rows 4*fk + reg

    // ---- S = Q K^T : MT accumulator tiles of 16 queries x 16 keys
    float4_t S[MT];
#pragma unroll
    for (int j = 0; j < MT; j++) S[j] = float4_t{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < D; k0 += 4) {
        const float a = Qp[(int64_t)fr * D + k0 + fk];
#pragma unroll
        for (int j = 0; j < MT; j++) {
            const float b = Kp[(int64_t)(16 * j + fr) * D + k0 + fk];       // B[k][col] = K[col][k]
            S[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, S[j], 0, 0, 0);
        }
    }
    // ---- row softmax: row r = 4*fk + e is spread over the 16 lanes sharing fk (cols) and the MT tiles
    float mx[4], sum[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        float m = S[0][e];
#pragma unroll
        for (int j = 1; j < MT; j++) m = fmaxf(m, S[j][e]);
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        mx[e] = m;
    }
#pragma unroll
    for (int e = 0; e < 4; e++) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < MT; j++) { const float pv = expf(S[j][e] - mx[e]); S[j][e] = pv; s += pv; }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) s += __shfl_xor(s, off, 64);
        sum[e] = s;
    }
#pragma unroll
    for (int j = 0; j < MT; j++)
#pragma unroll
        for (int e = 0; e < 4; e++) P[(4 * fk + e) * pitch + 16 * j + fr] = S[j][e] / sum[e];
    __builtin_amdgcn_s_waitcnt(0xC07F);     // lgkmcnt(0): this wave's own LDS writes are visible to its own later reads
    __builtin_amdgcn_wave_barrier();

    // ---- O = P V, 16 output columns at a time
    float* Op = out + ((int64_t)n * Q + q0) * DV;
    for (int c0 = 0; c0 < DV; c0 += 16) {
        float4_t O = float4_t{0.f, 0.f, 0.f, 0.f};
        for (int m0 = 0; m0 < M; m0 += 4) {
            const float a = P[fr * pitch + m0 + fk];                         // A[row fr][k = m0 + fk]
            const float b = Vp[(int64_t)(m0 + fk) * DV + c0 + fr];           // B[k][col fr]
            O = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, O, 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 4; e++) Op[(int64_t)(4 * fk + e) * DV + c0 + fr] = O[e];
    }
}

// ---- backward, first order (no [N, Q, M] map in HBM): the standard two-pass split, everything recomputed from theta / phi / g.
// Pass A (one wave per 16 queries, like the forward): S, P = softmax(S), dP = dO V^T, delta = rowsum(dP o P), dS = P o (dP - delta),
// dtheta = dS K; also writes the row statistics lse = max + log(sum) and delta for pass B.
template <int MT>
__global__ __launch_bounds__(256) void attention_bwd_dq_kernel(const float* theta, const float* phi, const float* g, const float* dout,
                                                               float* dtheta, float* lse, float* delta, int Q, int M, int D, int DV)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.y;
    const int q0 = (blockIdx.x * 4 + wave) * 16;
    const int pitch = ATT_MAX_M + 4;
    float* P = reinterpret_cast<float*>(smem) + wave * 16 * pitch;
    if (q0 >= Q) return;
    const float* Qp = theta + ((int64_t)n * Q + q0) * D;
    const float* Kp = phi + (int64_t)n * M * D;
    const float* Vp = g + (int64_t)n * M * DV;
    const float* dOp = dout + ((int64_t)n * Q + q0) * DV;
    const int fr = lane & 15, fk = lane >> 4;

    float4_t S[MT], dP[MT];
#pragma unroll
    for (int j = 0; j < MT; j++) { S[j] = float4_t{0.f, 0.f, 0.f, 0.f}; dP[j] = float4_t{0.f, 0.f, 0.f, 0.f}; }
    for (int k0 = 0; k0 < D; k0 += 4) {
        const float a = Qp[(int64_t)fr * D + k0 + fk];
#pragma unroll
        for (int j = 0; j < MT; j++) S[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Kp[(int64_t)(16 * j + fr) * D + k0 + fk], S[j], 0, 0, 0);
    }
    for (int k0 = 0; k0 < DV; k0 += 4) {                    // dP = dO V^T
        const float a = dOp[(int64_t)fr * DV + k0 + fk];
#pragma unroll
        for (int j = 0; j < MT; j++) dP[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Vp[(int64_t)(16 * j + fr) * DV + k0 + fk], dP[j], 0, 0, 0);
    }
    float mx[4], sum[4], dl[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        float m = S[0][e];
#pragma unroll
        for (int j = 1; j < MT; j++) m = fmaxf(m, S[j][e]);
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        mx[e] = m;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < MT; j++) { const float pv = expf(S[j][e] - m); S[j][e] = pv; s += pv; }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) s += __shfl_xor(s, off, 64);
        sum[e] = s;
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < MT; j++) { S[j][e] = S[j][e] / s; d += S[j][e] * dP[j][e]; }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) d += __shfl_xor(d, off, 64);
        dl[e] = d;
    }
    if (fr == 0) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            lse[(int64_t)n * Q + q0 + 4 * fk + e] = mx[e] + logf(sum[e]);
            delta[(int64_t)n * Q + q0 + 4 * fk + e] = dl[e];
        }
    }
#pragma unroll
    for (int j = 0; j < MT; j++)
#pragma unroll
        for (int e = 0; e < 4; e++) P[(4 * fk + e) * pitch + 16 * j + fr] = S[j][e] * (dP[j][e] - dl[e]);       // dS
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
    float* dQp = dtheta + ((int64_t)n * Q + q0) * D;
    for (int c0 = 0; c0 < D; c0 += 16) {                    // dtheta = dS K
        const bool colok = c0 + fr < D;
        float4_t O = float4_t{0.f, 0.f, 0.f, 0.f};
        for (int m0 = 0; m0 < M; m0 += 4) {
            const float a = P[fr * pitch + m0 + fk];
            const float b = colok ? Kp[(int64_t)(m0 + fk) * D + c0 + fr] : 0.f;
            O = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, O, 0, 0, 0);
        }
        if (colok) {
#pragma unroll
            for (int e = 0; e < 4; e++) dQp[(int64_t)(4 * fk + e) * D + c0 + fr] = O[e];
        }
    }
}

// Pass B (one wave per 16 keys, walking over all query blocks): P^T = exp(K Q^T - lse), dP^T = V dO^T, dS^T = P^T o (dP^T - delta),
// dg += P^T dO, dphi += dS^T Q.  Sums over the queries stay inside one wave: fixed order, reproducible.
template <int DVT, int DT>     // DV / 16 and ceil(D / 16) accumulator tiles
__global__ __launch_bounds__(256) void attention_bwd_dkv_kernel(const float* theta, const float* phi, const float* g, const float* dout,
                                                                const float* lse, const float* delta, float* dphi, float* dg,
                                                                int Q, int M, int D, int DV)
{
    __shared__ float tiles[4][2][16 * 17];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.y;
    const int m0 = (blockIdx.x * 4 + wave) * 16;
    if (m0 >= M) return;
    float* Pt = tiles[wave][0];
    float* dSt = tiles[wave][1];
    const float* Qp = theta + (int64_t)n * Q * D;
    const float* Kp = phi + ((int64_t)n * M + m0) * D;
    const float* Vp = g + ((int64_t)n * M + m0) * DV;
    const float* dOp = dout + (int64_t)n * Q * DV;
    const int fr = lane & 15, fk = lane >> 4;
    float4_t aV[DVT], aK[DT];
#pragma unroll
    for (int i = 0; i < DVT; i++) aV[i] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < DT; i++) aK[i] = float4_t{0.f, 0.f, 0.f, 0.f};
    for (int qb = 0; qb < Q; qb += 16) {
        float4_t St = float4_t{0.f, 0.f, 0.f, 0.f}, dPt = float4_t{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < D; k0 += 4)                   // S^T tile: rows = keys, cols = queries
            St = __builtin_amdgcn_mfma_f32_16x16x4f32(Kp[(int64_t)fr * D + k0 + fk], Qp[(int64_t)(qb + fr) * D + k0 + fk], St, 0, 0, 0);
        for (int k0 = 0; k0 < DV; k0 += 4)
            dPt = __builtin_amdgcn_mfma_f32_16x16x4f32(Vp[(int64_t)fr * DV + k0 + fk], dOp[(int64_t)(qb + fr) * DV + k0 + fk], dPt, 0, 0, 0);
        const float l = lse[(int64_t)n * Q + qb + fr], dl = delta[(int64_t)n * Q + qb + fr];      // statistics of this lane's query column
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float pv = expf(St[e] - l);
            Pt[(4 * fk + e) * 17 + fr] = pv;
            dSt[(4 * fk + e) * 17 + fr] = pv * (dPt[e] - dl);
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < 4; i++) {                       // k = 4 queries per MFMA
            const float ap = Pt[fr * 17 + 4 * i + fk], as = dSt[fr * 17 + 4 * i + fk];
            const float* dor = dOp + (int64_t)(qb + 4 * i + fk) * DV;
            const float* qr = Qp + (int64_t)(qb + 4 * i + fk) * D;
#pragma unroll
            for (int c = 0; c < DVT; c++) aV[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap, dor[16 * c + fr], aV[c], 0, 0, 0);
#pragma unroll
            for (int c = 0; c < DT; c++) aK[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(as, (16 * c + fr < D) ? qr[16 * c + fr] : 0.f, aK[c], 0, 0, 0);
        }
    }
    float* dVp = dg + ((int64_t)n * M + m0) * DV;
    float* dKp = dphi + ((int64_t)n * M + m0) * D;
#pragma unroll
    for (int c = 0; c < DVT; c++)
#pragma unroll
        for (int e = 0; e < 4; e++) dVp[(int64_t)(4 * fk + e) * DV + 16 * c + fr] = aV[c][e];
#pragma unroll
    for (int c = 0; c < DT; c++)
        if (16 * c + fr < D) {
#pragma unroll
            for (int e = 0; e < 4; e++) dKp[(int64_t)(4 * fk + e) * D + 16 * c + fr] = aK[c][e];
        }
}

// ---- streaming (online-softmax) form, M > ATT_MAX_M.  A wave still owns 16 query rows and walks the keys in chunks of ATT_CHUNK (the last
// chunk holds the remainder, a multiple of 16): one chunk is the S[] / LDS-strip structure of the kernels above.  ATT_CHUNK is 128, not
// ATT_MAX_M: with the output tiles resident next to S[] a 256-key chunk takes the whole register file (one wave per SIMD); at 128 keys
// two to three waves fit and the strip is 33 KiB per workgroup.  Per row it carries a running
// maximum m, a running sum l of exp(s - m) and the DV / 16 output tiles O = sum exp(s - m) v.  A chunk with maximum mc moves the state to
//   m' = max(m, mc),  c = exp(m - m'),  l' = c l + sum_chunk exp(s - m'),  O' = c O + exp(S_chunk - m') V_chunk
// (m starts at -FLT_MAX, so the first chunk's c is exp(-huge) = 0 on l = 0, O = 0: no infinity enters the arithmetic).  One division by l at
// the end; lse = m + log(l).
#ifndef ATT_CHUNK
#define ATT_CHUNK 128                // keys of one chunk (<= ATT_MAX_M)
#endif
#define ATT_CT (ATT_CHUNK / 16)     // key tiles of one chunk
#define ATT_NEG_HUGE (-3.402823466e+38f)

// S[j] += Q K_chunk^T for the nt <= ATT_CT key tiles of the chunk at Kc (tiles >= nt stay untouched)
static __device__ __forceinline__ void att_chunk_scores(float4_t (&S)[ATT_CT], const float* Qp, const float* Kc, int nt, int D, int fr, int fk)
{
    for (int k0 = 0; k0 < D; k0 += 4) {
        const float a = Qp[(int64_t)fr * D + k0 + fk];
#pragma unroll
        for (int j = 0; j < ATT_CT; j++)
            if (j < nt) S[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Kc[(int64_t)(16 * j + fr) * D + k0 + fk], S[j], 0, 0, 0);
    }
}

// STATS = false: the forward, out columns [16 * DVT * blockIdx.z, +16 * DVT).  STATS = true (backward, whole DV = 16 * DVT): the forward
// recomputed for the row statistics only -- lse and delta = rowsum(dout o out) -- nothing else is written.
template <int DVT, bool STATS>
__global__ __launch_bounds__(256) void attention_fwd_stream_kernel(const float* theta, const float* phi, const float* g, const float* dout,
                                                                   float* out, float* lse, float* delta, int Q, int M, int D, int DV)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.y;
    const int q0 = (blockIdx.x * 4 + wave) * 16;
    const int cb = blockIdx.z * DVT * 16;                    // first output column of this workgroup
    const int pitch = ATT_CHUNK + 4;
    float* P = reinterpret_cast<float*>(smem) + wave * 16 * pitch;
    if (q0 >= Q) return;
    const float* Qp = theta + ((int64_t)n * Q + q0) * D;
    const float* Kp = phi + (int64_t)n * M * D;
    const float* Vp = g + (int64_t)n * M * DV + cb;
    const int fr = lane & 15, fk = lane >> 4;

    float4_t O[DVT];
#pragma unroll
    for (int c = 0; c < DVT; c++) O[c] = float4_t{0.f, 0.f, 0.f, 0.f};
    float mrun[4], lrun[4];
#pragma unroll
    for (int e = 0; e < 4; e++) { mrun[e] = ATT_NEG_HUGE; lrun[e] = 0.f; }

    for (int mb = 0; mb < M; mb += ATT_CHUNK) {
        const int nt = (M - mb < ATT_CHUNK ? M - mb : ATT_CHUNK) / 16;
        float4_t S[ATT_CT];
#pragma unroll
        for (int j = 0; j < ATT_CT; j++) S[j] = float4_t{0.f, 0.f, 0.f, 0.f};
        att_chunk_scores(S, Qp, Kp + (int64_t)mb * D, nt, D, fr, fk);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            float m = S[0][e];
#pragma unroll
            for (int j = 1; j < ATT_CT; j++) if (j < nt) m = fmaxf(m, S[j][e]);
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
            const float mnew = fmaxf(mrun[e], m);
            const float sc = expf(mrun[e] - mnew);
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < ATT_CT; j++) if (j < nt) { const float pv = expf(S[j][e] - mnew); S[j][e] = pv; s += pv; }
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) s += __shfl_xor(s, off, 64);
            lrun[e] = lrun[e] * sc + s;
            mrun[e] = mnew;
#pragma unroll
            for (int c = 0; c < DVT; c++) O[c][e] *= sc;     // row 4 * fk + e of every output tile
        }
        __builtin_amdgcn_wave_barrier();                     // the previous chunk's strip reads are issued before it is overwritten
#pragma unroll
        for (int j = 0; j < ATT_CT; j++)
            if (j < nt) {
#pragma unroll
                for (int e = 0; e < 4; e++) P[(4 * fk + e) * pitch + 16 * j + fr] = S[j][e];
            }
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
        const float* Vc = Vp + (int64_t)mb * DV;
        for (int m0 = 0; m0 < 16 * nt; m0 += 4) {
            const float a = P[fr * pitch + m0 + fk];
            const float* vr = Vc + (int64_t)(m0 + fk) * DV + fr;
#pragma unroll
            for (int c = 0; c < DVT; c++) O[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, vr[16 * c], O[c], 0, 0, 0);
        }
    }
    if (STATS) {
        const float* dOp = dout + ((int64_t)n * Q + q0) * DV;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            float d = 0.f;
#pragma unroll
            for (int c = 0; c < DVT; c++) d += dOp[(int64_t)(4 * fk + e) * DV + 16 * c + fr] * (O[c][e] / lrun[e]);
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) d += __shfl_xor(d, off, 64);
            if (fr == 0) {
                lse[(int64_t)n * Q + q0 + 4 * fk + e] = mrun[e] + logf(lrun[e]);
                delta[(int64_t)n * Q + q0 + 4 * fk + e] = d;
            }
        }
    } else {
        float* Op = out + ((int64_t)n * Q + q0) * DV + cb;
#pragma unroll
        for (int c = 0; c < DVT; c++)
#pragma unroll
            for (int e = 0; e < 4; e++) Op[(int64_t)(4 * fk + e) * DV + 16 * c + fr] = O[c][e] / lrun[e];
    }
}

// Pass A of the backward, streamed: lse and delta are known (attention_fwd_stream_kernel<., true>), so the key chunks are walked once:
// P = exp(S - lse), dP = dO V^T, dS = P o (dP - delta) through the strip, dtheta += dS K_chunk in ceil(D / 16) accumulator tiles.
template <int DT>
__global__ __launch_bounds__(256) void attention_bwd_dq_stream_kernel(const float* theta, const float* phi, const float* g, const float* dout,
                                                                      const float* lse, const float* delta, float* dtheta, int Q, int M, int D, int DV)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.y;
    const int q0 = (blockIdx.x * 4 + wave) * 16;
    const int pitch = ATT_CHUNK + 4;
    float* P = reinterpret_cast<float*>(smem) + wave * 16 * pitch;
    if (q0 >= Q) return;
    const float* Qp = theta + ((int64_t)n * Q + q0) * D;
    const float* Kp = phi + (int64_t)n * M * D;
    const float* Vp = g + (int64_t)n * M * DV;
    const float* dOp = dout + ((int64_t)n * Q + q0) * DV;
    const int fr = lane & 15, fk = lane >> 4;
    float l[4], dl[4];
#pragma unroll
    for (int e = 0; e < 4; e++) { l[e] = lse[(int64_t)n * Q + q0 + 4 * fk + e]; dl[e] = delta[(int64_t)n * Q + q0 + 4 * fk + e]; }
    float4_t A[DT];
#pragma unroll
    for (int c = 0; c < DT; c++) A[c] = float4_t{0.f, 0.f, 0.f, 0.f};

    for (int mb = 0; mb < M; mb += ATT_CHUNK) {
        const int nt = (M - mb < ATT_CHUNK ? M - mb : ATT_CHUNK) / 16;
        const float* Kc = Kp + (int64_t)mb * D;
        const float* Vc = Vp + (int64_t)mb * DV;
        float4_t S[ATT_CT], dP[ATT_CT];
#pragma unroll
        for (int j = 0; j < ATT_CT; j++) { S[j] = float4_t{0.f, 0.f, 0.f, 0.f}; dP[j] = float4_t{0.f, 0.f, 0.f, 0.f}; }
        att_chunk_scores(S, Qp, Kc, nt, D, fr, fk);
        att_chunk_scores(dP, dOp, Vc, nt, DV, fr, fk);       // dP = dO V_chunk^T: the same product with (dO, V, DV) for (Q, K, D)
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < ATT_CT; j++)
            if (j < nt) {
#pragma unroll
                for (int e = 0; e < 4; e++) P[(4 * fk + e) * pitch + 16 * j + fr] = expf(S[j][e] - l[e]) * (dP[j][e] - dl[e]);       // dS
            }
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
        for (int m0 = 0; m0 < 16 * nt; m0 += 4) {
            const float a = P[fr * pitch + m0 + fk];
            const float* kr = Kc + (int64_t)(m0 + fk) * D;
#pragma unroll
            for (int c = 0; c < DT; c++) A[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, (16 * c + fr < D) ? kr[16 * c + fr] : 0.f, A[c], 0, 0, 0);
        }
    }
    float* dQp = dtheta + ((int64_t)n * Q + q0) * D;
#pragma unroll
    for (int c = 0; c < DT; c++)
        if (16 * c + fr < D) {
#pragma unroll
            for (int e = 0; e < 4; e++) dQp[(int64_t)(4 * fk + e) * D + 16 * c + fr] = A[c][e];
        }
}

// records of kind SBG_K_ATTENTION: dims = (N, Q, M, D, DV, 0 forward / 1 backward, variant)
enum { ATT_V_SINGLE = 0, ATT_V_STREAM = 1, ATT_V_STREAM_STATS = 2, ATT_V_STREAM_DQ = 3, ATT_V_STREAM_DKV = 4 };

#define ATT_STREAM_LDS (4 * 16 * (ATT_CHUNK + 4) * (int)sizeof(float))

template <int DVT, bool STATS>
static int launch_att_stream(const float* theta, const float* phi, const float* g, const float* dout, float* out, float* lse, float* delta,
                             int N, int Q, int M, int D, int DV, hipStream_t s)
{
    if (!SBG_RAISE_LDS_ONCE((attention_fwd_stream_kernel<DVT, STATS>), ATT_STREAM_LDS))
        return sbg_fail(SBG_ERR_LAUNCH, "attention (streamed): cannot raise the dynamic LDS limit to %d bytes", ATT_STREAM_LDS);
    SBG_LAUNCH((attention_fwd_stream_kernel<DVT, STATS>), dim3((Q + 63) / 64, N, DV / (16 * DVT)), dim3(256), ATT_STREAM_LDS, s,
               theta, phi, g, dout, out, lse, delta, Q, M, D, DV);
    return SBG_OK;
}

template <bool STATS>
static int launch_att_stream_dvt(int dvt, const float* theta, const float* phi, const float* g, const float* dout, float* out, float* lse, float* delta,
                                 int N, int Q, int M, int D, int DV, hipStream_t s)
{
    const int rc = att_for_tiles<16>(dvt, [&](auto t) {
        return launch_att_stream<decltype(t)::value, STATS>(theta, phi, g, dout, out, lse, delta, N, Q, M, D, DV, s); });
    return rc == ATT_NO_TILES ? sbg_fail(SBG_ERR_UNSUPPORTED, "attention (streamed): %d output tiles per workgroup", dvt) : rc;
}

template <int DT>
static int launch_att_bwd_dq_stream(const float* theta, const float* phi, const float* g, const float* dout, const float* lse, const float* delta,
                                    float* dtheta, int N, int Q, int M, int D, int DV, hipStream_t s)
{
    if (!SBG_RAISE_LDS_ONCE(attention_bwd_dq_stream_kernel<DT>, ATT_STREAM_LDS))
        return sbg_fail(SBG_ERR_LAUNCH, "attention_bwd (streamed): cannot raise the dynamic LDS limit to %d bytes", ATT_STREAM_LDS);
    SBG_LAUNCH((attention_bwd_dq_stream_kernel<DT>), dim3((Q + 63) / 64, N), dim3(256), ATT_STREAM_LDS, s, theta, phi, g, dout, lse, delta, dtheta, Q, M, D, DV);
    return SBG_OK;
}

template <int MT>
static int launch_att(const float* theta, const float* phi, const float* g, float* out, int N, int Q, int M, int D, int DV, hipStream_t s)
{
    const int lds = 4 * 16 * (ATT_MAX_M + 4) * (int)sizeof(float);
    if (!SBG_RAISE_LDS_ONCE(attention_fwd_kernel<MT>, lds)) return sbg_fail(SBG_ERR_LAUNCH, "attention_fwd: cannot raise the dynamic LDS limit to %d bytes", lds);
    SBG_LAUNCH((attention_fwd_kernel<MT>), dim3((Q + 63) / 64, N), dim3(256), lds, s, theta, phi, g, out, Q, M, D, DV);
    return SBG_OK;
}

} // namespace

extern "C" int64_t sbg_sn_workspace(int rows, int cols)
{
    const int64_t nrb = (rows + SN_ROWS_PER_BLOCK - 1) / SN_ROWS_PER_BLOCK;
    const int64_t kb = (cols + 255) / 256;
    return (nrb * cols + cols + kb + rows + 16) * (int64_t)sizeof(float);
}

extern "C" int sbg_sn_power_iteration(const float* W, const float* u, float* v, float* u_new, float* sigma, void* workspace,
                                      int rows, int cols, float eps, sbg_stream_t stream)
{
    SBG_CHECK(W && u && v && u_new && sigma && workspace, "sn_power_iteration: null pointer");
    SBG_CHECK(rows >= 1 && cols >= 1, "sn_power_iteration: bad sizes");
    hipStream_t s = (hipStream_t)stream;
    const int nrb = (rows + SN_ROWS_PER_BLOCK - 1) / SN_ROWS_PER_BLOCK, kb = (cols + 255) / 256;
    float* partial = (float*)workspace;
    float* v_raw = partial + (int64_t)nrb * cols;
    float* vn2 = v_raw + cols;
    float* t = vn2 + kb;
    SbgProfScope prof(s, SBG_K_SN_POWER, 4.0 * rows * (double)cols, 8.0 * rows * (double)cols, {rows, cols});
    SBG_LAUNCH(sn_colsum_kernel, dim3(kb, nrb), dim3(256), 0, s, W, u, partial, rows, cols);
    SBG_LAUNCH(sn_vfinish_kernel, dim3(kb), dim3(256), 0, s, partial, v_raw, vn2, cols, nrb);
    SBG_LAUNCH(sn_rowsum_kernel, dim3(rows), dim3(256), 0, s, W, v_raw, vn2, kb, v, t, rows, cols, eps);
    SBG_LAUNCH(sn_ufinish_kernel, dim3(1), dim3(256), 0, s, t, u_new, sigma, rows, eps);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int sbg_attention_supported(int Q, int M, int D, int DV)
{
    if (!(Q >= 16 && Q % 16 == 0 && M >= 16 && M % 16 == 0 && D >= 4 && D % 4 == 0 && DV >= 16 && DV % 16 == 0)) return 0;
    if (M <= ATT_MAX_M) return att_tiles_dispatched<16>(M / 16) ? 1 : 0;     // the whole key strip at once: M / 16 must be an instantiated MT
    // streamed form: any M whose per-sample matrices keep 32-bit element counts (sample bases are 64-bit)
    const int64_t w = D > DV ? D : DV;
    return ((int64_t)M * w <= INT32_MAX && (int64_t)Q * w <= INT32_MAX) ? 1 : 0;
}

template <int MT>
static int launch_att_bwd_dq(const float* theta, const float* phi, const float* g, const float* dout, float* dtheta, float* lse, float* delta,
                             int N, int Q, int M, int D, int DV, hipStream_t s)
{
    const int lds = 4 * 16 * (ATT_MAX_M + 4) * (int)sizeof(float);
    if (!SBG_RAISE_LDS_ONCE(attention_bwd_dq_kernel<MT>, lds)) return sbg_fail(SBG_ERR_LAUNCH, "attention_bwd: cannot raise the dynamic LDS limit to %d bytes", lds);
    SBG_LAUNCH((attention_bwd_dq_kernel<MT>), dim3((Q + 63) / 64, N), dim3(256), lds, s, theta, phi, g, dout, dtheta, lse, delta, Q, M, D, DV);
    return SBG_OK;
}

template <int DVT>
static int launch_att_bwd_dkv(const float* theta, const float* phi, const float* g, const float* dout, const float* lse, const float* delta,
                              float* dphi, float* dg, int N, int Q, int M, int D, int DV, hipStream_t s)
{
    const dim3 grid((M + 63) / 64, N);
    const int rc = att_for_tiles<4>((D + 15) / 16, [&](auto t) -> int {
        SBG_LAUNCH((attention_bwd_dkv_kernel<DVT, decltype(t)::value>), grid, dim3(256), 0, s, theta, phi, g, dout, lse, delta, dphi, dg, Q, M, D, DV);
        return (int)SBG_OK; });
    return rc == ATT_NO_TILES ? sbg_fail(SBG_ERR_UNSUPPORTED, "attention_bwd: D = %d needs 1, 2 or 4 column tiles of 16", D) : rc;
}

// both directions' per-key-tile pass: DV / 16 output tiles
static int launch_att_bwd_dkv_dvt(const float* theta, const float* phi, const float* g, const float* dout, const float* lse, const float* delta,
                                  float* dphi, float* dg, int N, int Q, int M, int D, int DV, hipStream_t s)
{
    const int rc = att_for_tiles<16>(DV / 16, [&](auto t) {
        return launch_att_bwd_dkv<decltype(t)::value>(theta, phi, g, dout, lse, delta, dphi, dg, N, Q, M, D, DV, s); });
    return rc == ATT_NO_TILES ? sbg_fail(SBG_ERR_UNSUPPORTED, "attention_bwd: DV / 16 must be 1, 2, 4, 8 or 16 (got DV = %d)", DV) : rc;
}

extern "C" int sbg_attention_bwd_supported(int Q, int M, int D, int DV)
{
    return (sbg_attention_supported(Q, M, D, DV) && att_tiles_dispatched<4>((D + 15) / 16) && att_tiles_dispatched<16>(DV / 16)) ? 1 : 0;
}

extern "C" int64_t sbg_attention_bwd_workspace(int N, int Q) { return 2 * (int64_t)N * Q * (int64_t)sizeof(float); }

// Streamed backward, M > ATT_MAX_M: three launches, each with its own record.  O is not taken from the forward: the first launch recomputes
// it in registers for lse and delta = rowsum(dout o out), so the saved state is the three inputs, as for the single-chunk kernels.
static int attention_bwd_stream(const float* theta, const float* phi, const float* g, const float* dout, float* dtheta, float* dphi, float* dg,
                                float* lse, float* delta, int N, int Q, int M, int D, int DV, hipStream_t s)
{
    const double qm = 2.0 * N * (double)Q * M, qd = (double)Q * D, qv = (double)Q * DV, mk = (double)M * (D + DV);
    int rc = SBG_OK;
    {
        SbgProfScope prof(s, SBG_K_ATTENTION, qm * (D + DV), 4.0 * N * (qd + mk + qv + 2.0 * Q), {N, Q, M, D, DV, 1, ATT_V_STREAM_STATS});
        rc = launch_att_stream_dvt<true>(DV / 16, theta, phi, g, dout, nullptr, lse, delta, N, Q, M, D, DV, s);
    }
    if (rc != SBG_OK) return rc;
    {
        SbgProfScope prof(s, SBG_K_ATTENTION, qm * (2.0 * D + DV), 4.0 * N * (2.0 * qd + mk + qv + 2.0 * Q), {N, Q, M, D, DV, 1, ATT_V_STREAM_DQ});
        rc = att_for_tiles<4>((D + 15) / 16, [&](auto t) {
            return launch_att_bwd_dq_stream<decltype(t)::value>(theta, phi, g, dout, lse, delta, dtheta, N, Q, M, D, DV, s); });
        if (rc == ATT_NO_TILES) rc = sbg_fail(SBG_ERR_UNSUPPORTED, "attention_bwd: D = %d needs 1, 2 or 4 column tiles of 16", D);
    }
    if (rc != SBG_OK) return rc;
    {
        SbgProfScope prof(s, SBG_K_ATTENTION, qm * (2.0 * D + 2.0 * DV), 4.0 * N * (qd + qv + 2.0 * mk + 2.0 * Q), {N, Q, M, D, DV, 1, ATT_V_STREAM_DKV});
        rc = launch_att_bwd_dkv_dvt(theta, phi, g, dout, lse, delta, dphi, dg, N, Q, M, D, DV, s);
    }
    if (rc != SBG_OK) return rc;
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

// First-order gradients of out = softmax(theta phi^T) g.  workspace: sbg_attention_bwd_workspace(N, Q) bytes (row statistics).
extern "C" int sbg_attention_bwd(const float* theta, const float* phi, const float* g, const float* dout, float* dtheta, float* dphi, float* dg,
                                 void* workspace, int N, int Q, int M, int D, int DV, sbg_stream_t stream)
{
    SBG_CHECK(theta && phi && g && dout && dtheta && dphi && dg && workspace, "attention_bwd: null pointer");
    SBG_CHECK(sbg_attention_bwd_supported(Q, M, D, DV), "attention_bwd: unsupported shape Q=%d M=%d D=%d DV=%d", Q, M, D, DV);
    if (N == 0) return SBG_OK;
    hipStream_t s = (hipStream_t)stream;
    float* lse = (float*)workspace;
    float* delta = lse + (int64_t)N * Q;
    if (M > ATT_MAX_M) return attention_bwd_stream(theta, phi, g, dout, dtheta, dphi, dg, lse, delta, N, Q, M, D, DV, s);
    SbgProfScope prof(s, SBG_K_ATTENTION, 2.0 * N * (double)Q * M * (3.0 * D + 3.0 * DV), 4.0 * N * (2.0 * Q * D + 2.0 * M * (D + DV) + 2.0 * Q * DV), {N, Q, M, D, DV, 1});
    int rc = att_for_tiles<16>(M / 16, [&](auto t) {
        return launch_att_bwd_dq<decltype(t)::value>(theta, phi, g, dout, dtheta, lse, delta, N, Q, M, D, DV, s); });
    if (rc == ATT_NO_TILES) return sbg_fail(SBG_ERR_UNSUPPORTED, "attention_bwd: M / 16 must be 1, 2, 4, 8 or 16 (got M = %d)", M);
    if (rc != SBG_OK) return rc;
    rc = launch_att_bwd_dkv_dvt(theta, phi, g, dout, lse, delta, dphi, dg, N, Q, M, D, DV, s);
    if (rc != SBG_OK) return rc;
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int sbg_attention_fwd(const float* theta, const float* phi, const float* g, float* out, int N, int Q, int M, int D, int DV,
                                 sbg_stream_t stream)
{
    SBG_CHECK(theta && phi && g && out, "attention_fwd: null pointer");
    SBG_CHECK(sbg_attention_supported(Q, M, D, DV), "attention_fwd: unsupported shape Q=%d M=%d D=%d DV=%d", Q, M, D, DV);
    if (N == 0) return SBG_OK;
    hipStream_t s = (hipStream_t)stream;
    SbgProfScope prof(s, SBG_K_ATTENTION, 2.0 * N * (double)Q * M * (D + DV), 4.0 * N * ((double)Q * D + (double)M * (D + DV) + (double)Q * DV), {N, Q, M, D, DV});
    int rc = SBG_OK;
    if (M > ATT_MAX_M) {
        // as many of the DV / 16 output tiles per workgroup as divide them (16, 8, 4, 2 or 1); the other column groups go to grid.z
        int dvt = 16;
        while ((DV / 16) % dvt) dvt >>= 1;
        prof.set_dim(6, ATT_V_STREAM);
        rc = launch_att_stream_dvt<false>(dvt, theta, phi, g, nullptr, out, nullptr, nullptr, N, Q, M, D, DV, s);
        if (rc != SBG_OK) return rc;
        SBG_HIP_LAUNCH_CHECK();
        return SBG_OK;
    }
    rc = att_for_tiles<16>(M / 16, [&](auto t) { return launch_att<decltype(t)::value>(theta, phi, g, out, N, Q, M, D, DV, s); });
    if (rc == ATT_NO_TILES) return sbg_fail(SBG_ERR_UNSUPPORTED, "attention_fwd: M / 16 must be 1, 2, 4, 8 or 16 (got M = %d)", M);
    if (rc != SBG_OK) return rc;
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}
