// swd.hip -- device arithmetic of the sliced Wasserstein distance on Laplacian-pyramid patches (Karras et al., "Progressive Growing of
// GANs", ICLR 2018, section 5; `swd16k` of metrics/metric_main.py).  All fp32 unless said otherwise, dense tensors.
//
// Pyramid.  g = [1, 4, 6, 4, 1] / 16, separable, boundaries mirrored without repeating the edge sample (index -k -> k, S - 1 + k -> S - 1 - k),
// resolved inside the kernels: there is no padded copy.  One 1-D pass over five samples a0..a4 with the taps w0..w4 is the chain
//   ((((w0 a0 + w1 a1) + w1 a2) + w2' a2) + w1 a3) + w0 a4,      the centre tap 6 split as 4 + 2 (w1 = 4 w0, w2' = 2 w0), so every tap is a power of
// two, every product is exact and every step rounds once, fused or not,
// rows first (a pixel's five source rows each filtered along x), then the five row results along y.  torch_utils/ops/swd.py states the same
// chain with torch ops for CPU tensors, so both devices give the same bits on any input.
//   pyr_down  y[oy, ox] = the chain with taps g at the source centre (2 oy, 2 ox)                                       [B,C,S,S] -> [B,C,S/2,S/2]
//   pyr_lap   out = fine - up(coarse);  up = the chain with taps 2 g over the zero-inserted image z[2i, 2j] = coarse[i, j] (zero elsewhere)
//             of side S, mirrored like any image (the reflection keeps the parity of an index); `out` may be `fine` itself.
// gather.  Row row_offset + b P + p of the [M, 49 C] descriptor matrix = the 7 x 7 x C patch of image b around centres[b, p] = (y, x), in
// (c, dy, dx) order.  A centre outside [3, S - 4] is never dereferenced: its row is filled with NaN.
// Sums (moments, l1): float64, fixed order.  The data of one output value is cut into chunks whose length depends on the shape alone
// (moments: 1024 descriptor rows of one channel = 50176 values; l1: 16384 elements of one direction).  In a chunk, lane t of the 256 adds the
// elements t, t + 256, ... in ascending order, block_sum (reduce.h) adds the lanes; one workgroup per chunk writes one float64 partial.
// The partials of one output value are added by the shared merge kernel (merge.h, div = 1).  No atomics, no dependence on the launch
// geometry: two runs give the same bits.
//   moments   out[c] = {sum, sum of squares} of channel c over all M * 49 values, each value widened to float64 before squaring
//   l1        out[d] = sum_m |(double)a[d, m] - (double)b[d, m]|
// project.  p[d, m] = the fp32 chain over k = 0..K-1 from 0:  acc = fmaf(fmaf(x[m, k], s[c(k)], t[c(k)]), dir[k, d], acc),  c(k) = k / 49,
// on v_mfma_f32_32x32x2_f32, which is that chain bit for bit (one rounding per product-and-add, k ascending).  The MFMA rows are directions,
// its columns descriptor rows, so a wave's store of one accumulator register is 32 consecutive floats of the direction-major output [D, M].
// A workgroup (4 waves) owns 128 descriptor rows x 128 directions, a wave 32 rows x 4 accumulators; K is walked in chunks of 32 staged in
// LDS, the normalisation applied while staging (no normalised copy in HBM).  Tails: rows >= M and directions >= D are staged as zeros and
// never stored; k >= K is staged as zero in BOTH operands (K = 49, 147 are odd: the last MFMA carries one such k; fmaf(0, 0, acc) = acc).
// Launch-log key: kind SBG_K_SWD, dims = {variant, ...}: 0 pyr_down (B, C, S) / 1 pyr_lap (B, C, S) / 2 gather (B, C, S, P) /
// 3 moments (M clipped, C, chunks) / 4 project (M clipped, K, D) / 5 l1 (D, M clipped, chunks) / 6 merge (values, chunks).
#include "sbg_common.h"
#include "reduce.h"
#include "merge.h"

namespace {

constexpr int kDown = 0, kLap = 1, kGather = 2, kMoments = 3, kProject = 4, kL1 = 5, kMerge = 6;
constexpr int NT = 256;
constexpr int kPatch = 7, kPP = kPatch * kPatch;        // 49 values per channel and descriptor row
constexpr int kMomRows = 1024;                          // descriptor rows per moments chunk
constexpr int kL1Chunk = 16384;                         // elements per l1 chunk

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

__device__ __forceinline__ int mirror(int i, int S) { i = i < 0 ? -i : i; return i >= S ? 2 * (S - 1) - i : i; }

// every tap is a power of two (6 = 4 + 2), so each product is exact and a step rounds once whether or not the compiler fuses it
__device__ __forceinline__ float chain5(float a0, float a1, float a2, float a3, float a4, float w0, float w1, float w2)
{
    float r = w0 * a0 + w1 * a1;
    r += w1 * a2;
    r += w2 * a2;
    r += w1 * a3;
    return r + w0 * a4;
}

__global__ __launch_bounds__(NT) void swd_pyr_down_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t total, int S)
{
    const int H = S / 2;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
        const int ox = (int)(i % H), oy = (int)((i / H) % H);
        const int64_t plane = i / ((int64_t)H * H);
        const float* xp = x + plane * S * S;
        int cx[5];
#pragma unroll
        for (int j = 0; j < 5; j++) cx[j] = mirror(2 * ox + j - 2, S);
        float h[5];
#pragma unroll
        for (int r = 0; r < 5; r++) {
            const float* row = xp + (int64_t)mirror(2 * oy + r - 2, S) * S;
            h[r] = chain5(row[cx[0]], row[cx[1]], row[cx[2]], row[cx[3]], row[cx[4]], 0.0625f, 0.25f, 0.125f);
        }
        y[i] = chain5(h[0], h[1], h[2], h[3], h[4], 0.0625f, 0.25f, 0.125f);
    }
}

__global__ __launch_bounds__(NT) void swd_pyr_lap_kernel(const float* fine, const float* __restrict__ coarse, float* out, int64_t total, int S)
{
    const int H = S / 2;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
        const int px = (int)(i % S), py = (int)((i / S) % S);
        const int64_t plane = i / ((int64_t)S * S);
        const float* cp = coarse + plane * H * H;
        int cx[5];
#pragma unroll
        for (int j = 0; j < 5; j++) cx[j] = mirror(px + j - 2, S);
        float h[5];
#pragma unroll
        for (int r = 0; r < 5; r++) {
            const int ry = mirror(py + r - 2, S);
            float a[5];
#pragma unroll
            for (int j = 0; j < 5; j++) a[j] = ((ry | cx[j]) & 1) ? 0.f : cp[(int64_t)(ry >> 1) * H + (cx[j] >> 1)];
            h[r] = chain5(a[0], a[1], a[2], a[3], a[4], 0.125f, 0.5f, 0.25f);
        }
        out[i] = fine[i] - chain5(h[0], h[1], h[2], h[3], h[4], 0.125f, 0.5f, 0.25f);
    }
}

__global__ __launch_bounds__(NT) void swd_gather_kernel(const float* __restrict__ level, const int* __restrict__ centres, float* __restrict__ desc,
                                                        int64_t total, int C, int S, int P, int64_t row_offset)
{
    const int K = C * kPP;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
        const int k = (int)(i % K);
        const int64_t r = i / K;                        // b * P + p
        const int64_t b = r / P;
        const int cy = centres[2 * r], cx = centres[2 * r + 1];
        const int c = k / kPP, rem = k - c * kPP, dy = rem / kPatch, dx = rem - dy * kPatch;
        const bool ok = cy >= 3 && cy <= S - 4 && cx >= 3 && cx <= S - 4;
        desc[(row_offset + r) * K + k] = ok ? level[((b * C + c) * S + (cy + dy - 3)) * (int64_t)S + (cx + dx - 3)] : __int_as_float(0x7fc00000);
    }
}

// one workgroup per (chunk, channel): partial[(2 c + j) * chunks + chunk]
__global__ __launch_bounds__(NT) void swd_moments_kernel(const float* __restrict__ desc, double* __restrict__ partial, int64_t M, int C, int chunks)
{
    __shared__ double red[NT / 64];
    const int chunk = (int)blockIdx.x, c = (int)blockIdx.y;
    const int64_t m0 = (int64_t)chunk * kMomRows;
    const int rows = (int)(M - m0 < kMomRows ? M - m0 : kMomRows);
    const int K = C * kPP;
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < rows * kPP; i += NT) {
        const int r = i / kPP, j = i - r * kPP;
        const double v = (double)desc[(m0 + r) * K + c * kPP + j];
        s1 += v; s2 += v * v;
    }
    s1 = block_sum<NT>(s1, red);
    s2 = block_sum<NT>(s2, red);
    if (threadIdx.x == 0) { partial[(int64_t)(2 * c) * chunks + chunk] = s1; partial[(int64_t)(2 * c + 1) * chunks + chunk] = s2; }
}

// one workgroup per (chunk, direction): partial[d * chunks + chunk]
__global__ __launch_bounds__(NT) void swd_l1_kernel(const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ partial, int64_t M, int chunks)
{
    __shared__ double red[NT / 64];
    const int chunk = (int)blockIdx.x, d = (int)blockIdx.y;
    const int64_t e0 = (int64_t)chunk * kL1Chunk;
    const int n = (int)(M - e0 < kL1Chunk ? M - e0 : kL1Chunk);
    const float* ap = a + (int64_t)d * M + e0;
    const float* bp = b + (int64_t)d * M + e0;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += NT) s += fabs((double)ap[i] - (double)bp[i]);
    s = block_sum<NT>(s, red);
    if (threadIdx.x == 0) partial[(int64_t)d * chunks + chunk] = s;
}

constexpr int PM = 128, PD = 128, KC = 32;              // project: descriptor rows, directions and k per staged chunk
constexpr int PLD = PM + 1;                             // LDS row pitch (floats)

__global__ __launch_bounds__(NT) void swd_project_kernel(const float* __restrict__ desc, const float* __restrict__ sc, const float* __restrict__ tc,
                                                         const float* __restrict__ dirs, float* __restrict__ out, int64_t M, int K, int D, int64_t ld)
{
    __shared__ float xs[KC][PLD];                       // xs[k][row]: normalised descriptors
    __shared__ float ds[KC][PLD];                       // ds[k][direction]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * PM;
    const int d0 = (int)blockIdx.y * PD;
    const int nt = (D - d0 + 31) / 32 < 4 ? (D - d0 + 31) / 32 : 4;        // 32-direction tiles of this workgroup that hold a direction
    f32x16_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[t][r] = 0.f;

    for (int k0 = 0; k0 < K; k0 += KC) {
        __syncthreads();                                // the previous chunk's reads are over
        for (int i = tid; i < PM * KC; i += NT) {       // 32 consecutive k of one row per half wave
            const int kk = i & (KC - 1), r = i >> 5;
            const int k = k0 + kk;
            const int64_t m = m0 + r;
            float v = 0.f;
            if (k < K && m < M) { const int c = k / kPP; v = __fmaf_rn(desc[m * K + k], sc[c], tc[c]); }
            xs[kk][r] = v;
        }
        for (int i = tid; i < PD * KC; i += NT) {       // 128 consecutive directions of one k
            const int dd = i & (PD - 1), kk = i >> 7;
            const int k = k0 + kk, d = d0 + dd;
            ds[kk][dd] = (k < K && d < D) ? dirs[(int64_t)k * ld + d] : 0.f;
        }
        __syncthreads();
        const int steps = ((K - k0 < KC ? K - k0 : KC) + 1) / 2;
        for (int st = 0; st < steps; st++) {
            const int kk = 2 * st + (lane >> 5);
            const float bx = xs[kk][wave * 32 + (lane & 31)];
#pragma unroll
            for (int t = 0; t < 4; t++)
                if (t < nt) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ds[kk][t * 32 + (lane & 31)], bx, acc[t], 0, 0, 0);
        }
    }
    const int64_t m = m0 + wave * 32 + (lane & 31);
    if (m >= M) return;
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int d = d0 + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (d < D) out[(int64_t)d * M + m] = acc[t][r];
        }
}

int merge(const double* partial, double* out, int values, int chunks, hipStream_t s)
{
    SbgProfScope prof(s, SBG_K_SWD, 0.0, 8.0 * values * (double)chunks + 8.0 * values, {kMerge, values, chunks});
    return merge_partials<double>(partial, out, values, chunks, 1.0, s);
}

} // namespace

extern "C" int sbg_swd_pyr_down(const float* x, float* y, int B, int C, int S, sbg_stream_t stream)
{
    SBG_CHECK(B >= 0 && C >= 1, "swd_pyr_down: bad sizes B=%d C=%d", B, C);
    SBG_CHECK(sbg_pow2_in(S, 4, 16384), "swd_pyr_down: side %d, a power of two in [4, 16384] is supported", S);
    if (B == 0) return SBG_OK;
    SBG_CHECK(x && y && x != y && sbg_aligned(x, 4) && sbg_aligned(y, 4), "swd_pyr_down: x and y must be distinct 4-byte aligned device pointers");
    const int64_t total = (int64_t)B * C * (S / 2) * (S / 2);
    hipStream_t s = (hipStream_t)stream;
    SbgProfScope prof(s, SBG_K_SWD, 0.0, 20.0 * total, {kDown, B, C, S});
    SBG_LAUNCH(swd_pyr_down_kernel, dim3(sbg_stream_grid(total, NT)), dim3(NT), 0, s, x, y, total, S);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int sbg_swd_pyr_lap(const float* fine, const float* coarse, float* out, int B, int C, int S, sbg_stream_t stream)
{
    SBG_CHECK(B >= 0 && C >= 1, "swd_pyr_lap: bad sizes B=%d C=%d", B, C);
    SBG_CHECK(sbg_pow2_in(S, 4, 16384), "swd_pyr_lap: side %d, a power of two in [4, 16384] is supported", S);
    if (B == 0) return SBG_OK;
    SBG_CHECK(fine && coarse && out && sbg_aligned(fine, 4) && sbg_aligned(coarse, 4) && sbg_aligned(out, 4), "swd_pyr_lap: null or misaligned pointer");
    SBG_CHECK(coarse != out, "swd_pyr_lap: `out` may be `fine`, never `coarse`");
    const int64_t total = (int64_t)B * C * S * S;
    hipStream_t s = (hipStream_t)stream;
    SbgProfScope prof(s, SBG_K_SWD, 0.0, 9.0 * total, {kLap, B, C, S});
    SBG_LAUNCH(swd_pyr_lap_kernel, dim3(sbg_stream_grid(total, NT)), dim3(NT), 0, s, fine, coarse, out, total, S);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int sbg_swd_gather(const float* level, const int32_t* centres, float* desc, int B, int C, int S, int P, int64_t row_offset, int64_t M,
                              sbg_stream_t stream)
{
    SBG_CHECK(B >= 0 && C >= 1 && C <= 4 && P >= 1, "swd_gather: bad sizes B=%d C=%d P=%d (1..4 channels)", B, C, P);
    SBG_CHECK(S >= kPatch && S <= 16384, "swd_gather: side %d, [7, 16384] is supported", S);
    SBG_CHECK(row_offset >= 0 && M >= 0 && row_offset + (int64_t)B * P <= M, "swd_gather: rows [%lld, +%lld) leave the %lld descriptor rows",
              (long long)row_offset, (long long)B * P, (long long)M);
    if (B == 0) return SBG_OK;
    SBG_CHECK(level && centres && desc && sbg_aligned(level, 4) && sbg_aligned(centres, 4) && sbg_aligned(desc, 4), "swd_gather: null or misaligned pointer");
    const int64_t total = (int64_t)B * P * C * kPP;
    hipStream_t s = (hipStream_t)stream;
    SbgProfScope prof(s, SBG_K_SWD, 0.0, 8.0 * total + 8.0 * B * P, {kGather, B, C, S, P});
    SBG_LAUNCH(swd_gather_kernel, dim3(sbg_stream_grid(total, NT)), dim3(NT), 0, s, level, centres, desc, total, C, S, P, row_offset);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int64_t sbg_swd_moments_workspace(int64_t M, int C)
{
    if (M < 1 || C < 1 || C > 4 || M > ((int64_t)1 << 40)) return -1;
    return 8 * 2 * C * ((M + kMomRows - 1) / kMomRows);
}

extern "C" int sbg_swd_moments(const float* desc, double* out, void* workspace, int64_t M, int C, sbg_stream_t stream)
{
    SBG_CHECK(sbg_swd_moments_workspace(M, C) >= 0, "swd_moments: bad sizes M=%lld C=%d (M >= 1, 1..4 channels)", (long long)M, C);
    SBG_CHECK(desc && out && workspace && sbg_aligned(desc, 4) && sbg_aligned(out, 8) && sbg_aligned(workspace, 8), "swd_moments: null or misaligned pointer");
    const int chunks = (int)((M + kMomRows - 1) / kMomRows);
    hipStream_t s = (hipStream_t)stream;
    {
        SbgProfScope prof(s, SBG_K_SWD, 0.0, 4.0 * (double)M * C * kPP, {kMoments, sbg_clip31(M), C, chunks});
        SBG_LAUNCH(swd_moments_kernel, dim3((unsigned)chunks, (unsigned)C), dim3(NT), 0, s, desc, (double*)workspace, M, C, chunks);
        SBG_HIP_LAUNCH_CHECK();
    }
    return merge((const double*)workspace, out, 2 * C, chunks, s);
}

extern "C" int sbg_swd_project(const float* desc, const float* s_c, const float* t_c, const float* dirs, float* out, int64_t M, int C, int D,
                               int64_t dirs_ld, sbg_stream_t stream)
{
    SBG_CHECK(M >= 1 && C >= 1 && C <= 4 && D >= 1, "swd_project: bad sizes M=%lld C=%d D=%d (1..4 channels)", (long long)M, C, D);
    SBG_CHECK(dirs_ld >= D, "swd_project: the directions' row pitch %lld is below D=%d", (long long)dirs_ld, D);
    SBG_CHECK((M + PM - 1) / PM <= INT32_MAX && (D + PD - 1) / PD <= 65535, "swd_project: M=%lld D=%d is too large", (long long)M, D);
    SBG_CHECK(desc && s_c && t_c && dirs && out && sbg_aligned(desc, 4) && sbg_aligned(s_c, 4) && sbg_aligned(t_c, 4) && sbg_aligned(dirs, 4) && sbg_aligned(out, 4),
              "swd_project: null or misaligned pointer");
    const int K = C * kPP;
    hipStream_t s = (hipStream_t)stream;
    SbgProfScope prof(s, SBG_K_SWD, 2.0 * (double)M * K * D, 4.0 * ((double)M * K + (double)K * D + (double)M * D), {kProject, sbg_clip31(M), K, D});
    SBG_LAUNCH(swd_project_kernel, dim3((unsigned)((M + PM - 1) / PM), (unsigned)((D + PD - 1) / PD)), dim3(NT), 0, s, desc, s_c, t_c, dirs, out, M, K, D,
               dirs_ld);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int64_t sbg_swd_l1_workspace(int D, int64_t M)
{
    if (D < 1 || D > 65535 || M < 1 || M > ((int64_t)1 << 40)) return -1;
    const int64_t chunks = (M + kL1Chunk - 1) / kL1Chunk;
    if (chunks > INT32_MAX) return -1;
    return 8 * (int64_t)D * chunks;
}

extern "C" int sbg_swd_l1(const float* a, const float* b, double* out, void* workspace, int D, int64_t M, sbg_stream_t stream)
{
    SBG_CHECK(sbg_swd_l1_workspace(D, M) >= 0, "swd_l1: bad sizes D=%d M=%lld (1 <= D <= 65535, M >= 1)", D, (long long)M);
    SBG_CHECK(a && b && out && workspace && sbg_aligned(a, 4) && sbg_aligned(b, 4) && sbg_aligned(out, 8) && sbg_aligned(workspace, 8), "swd_l1: null or misaligned pointer");
    const int chunks = (int)((M + kL1Chunk - 1) / kL1Chunk);
    hipStream_t s = (hipStream_t)stream;
    {
        SbgProfScope prof(s, SBG_K_SWD, 0.0, 8.0 * (double)D * (double)M, {kL1, D, sbg_clip31(M), chunks});
        SBG_LAUNCH(swd_l1_kernel, dim3((unsigned)chunks, (unsigned)D), dim3(NT), 0, s, a, b, (double*)workspace, M, chunks);
        SBG_HIP_LAUNCH_CHECK();
    }
    return merge((const double*)workspace, out, D, chunks, s);
}
