// directions.hip -- device arithmetic of the latent directions tool (directions.py; GANSpace: Harkonen et al., NeurIPS 2020; SeFa: Shen & Zhou,
// CVPR 2021): the column mean and the Gram matrix of a latent table x fp32 [N, D], 1 <= D <= 1024, and the table of
// edited latents.  torch_utils/ops/directions.py states the same orders in numpy for CPU tensors, so both devices give the same bits.
//
// mean.  out[d] = (float64 sum of column d) / N.  The rows are cut into chunks of 1024; in a chunk, lane t of the 256 adds the rows t, t + 256,
// t + 512, t + 768 in ascending order from 0, block_sum (reduce.h) adds the lanes; the chunk sums of a column are added by the merge kernel
// (merge.h), which divides once by N.  A workgroup owns one chunk of 32 columns, staged through LDS 256 rows at a time so that the global reads
// are whole 128-byte row segments; rows past N and columns past D are staged as +0.0 (adding it changes nothing) and never stored.
//
// gram.  THE ORDER IS THE CONTRACT:
//   1. c[n, i] = x[n, i] - mean[i], one fp32 subtraction (mean == NULL: c = x);
//   2. the rows are cut into chunks of kChunkRows = 256; a chunk with an odd row count gets one more row of +0.0 (after centring), so the
//      chain always runs over whole 2-row steps of the matrix-core instruction;
//   3. per chunk q, P_q[i, j] = the fp32 chain from +0.0 over the rows in ascending order, acc = fmaf(c[n, i], c[n, j], acc), on
//      v_mfma_f32_32x32x2_f32, which is that chain bit for bit (one rounding per product-and-add, k ascending);
//   4. per group g of kGroupChunks = 16 consecutive chunks, S_g = ((0 + (double)P_0) + (double)P_1) + ... in chunk order, held in the
//      registers of the workgroup that computed the chunks;
//   5. G[i, j] = the merge.h sum of the S_g over g (div = 1).
// The order depends on (N, D) alone.  fmaf(a, b, .) = fmaf(b, a, .), so G is symmetric bit for bit: only 32 x 32 tile pairs with jt >= it are
// computed, and an off-diagonal tile is stored to both places.  A workgroup (4 waves) owns a 64 x 64 block pair (ib <= jb) of one group, a wave
// one 32 x 32 tile of it (the tile below the diagonal of a diagonal block idles).  Rows are staged through LDS 32 at a time as
// as[k][column]: lane l reads [k = l >> 5][i = l & 31], 32 consecutive floats, conflict-free; the next 32 rows are fetched into registers
// while the matrix cores run.  Columns past D are staged as zeros and never stored.  LDS: 16 KiB.  Workspace: groups x D x D doubles, laid
// out value-major ([D * D][groups]) as the merge kernel reads it.
//
// edit.  out[(s K + k) T + t, l, d] = fmaf(step, comps[k, d], ws[s, l, d]) with step = sigmas[t] * scale[k] (one fp32 product) where
// layer_mask[l] != 0, ws[s, l, d] unchanged elsewhere.  One streaming launch.
// Launch-log key: kind SBG_K_DIRECTIONS, dims = {variant, ...}: 0 mean (N clipped, D, chunks) / 1 gram (N clipped, D, groups) /
// 2 merge (N clipped, D, chunks or groups) / 3 edit (S, K, T, L, D).
#include "sbg_common.h"
#include "reduce.h"
#include "merge.h"

namespace {

constexpr int kMean = 0, kGram = 1, kMerge = 2, kEdit = 3;
constexpr int NT = 256;
constexpr int kMaxD = 1024;
constexpr int kMeanRows = 1024;                         // rows per chunk of the mean
constexpr int kMeanCols = 32;                           // columns per workgroup of the mean
constexpr int kChunkRows = 256;                         // rows per fp32 chain of the Gram matrix
constexpr int kGroupChunks = 16;                        // chunks per float64 register sum
constexpr int kGroupRows = kChunkRows * kGroupChunks;
constexpr int KC = 32;                                  // rows per staged step
constexpr int BW = 64;                                  // columns per block
constexpr int kStage = KC * BW / NT;                    // staged values per work-item and operand

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

// one workgroup per (chunk, 32 columns): partial[d * chunks + chunk]
__global__ __launch_bounds__(NT) void directions_mean_kernel(const float* __restrict__ x, double* __restrict__ partial, int64_t N, int D, int chunks)
{
    __shared__ float tile[NT][kMeanCols + 1];
    __shared__ double red[NT / 64];
    const int tid = threadIdx.x;
    const int chunk = (int)blockIdx.x, d0 = (int)blockIdx.y * kMeanCols;
    const int64_t m0 = (int64_t)chunk * kMeanRows;
    double acc[kMeanCols];
#pragma unroll
    for (int c = 0; c < kMeanCols; c++) acc[c] = 0.0;
    for (int j = 0; j < kMeanRows / NT; j++) {
        __syncthreads();                                // the previous pass's reads are over
        for (int i = tid; i < NT * kMeanCols; i += NT) {
            const int c = i & (kMeanCols - 1), r = i >> 5;
            const int64_t row = m0 + (int64_t)j * NT + r;
            tile[r][c] = (row < N && d0 + c < D) ? x[row * D + d0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < kMeanCols; c++) acc[c] += (double)tile[tid][c];
    }
#pragma unroll
    for (int c = 0; c < kMeanCols; c++) {
        const double s = block_sum<NT>(acc[c], red);
        if (tid == 0 && d0 + c < D) partial[(int64_t)(d0 + c) * chunks + chunk] = s;
    }
}

// one workgroup per (block pair ib <= jb, group): partial[(i * D + j) * groups + group]
__global__ __launch_bounds__(NT) void directions_gram_kernel(const float* __restrict__ x, const float* __restrict__ mean, double* __restrict__ partial,
                                                             int64_t N, int D, int groups)
{
    __shared__ float as[KC][BW];                        // as[k][column of block ib]
    __shared__ float bs[KC][BW];                        // bs[k][column of block jb]; unused on a diagonal block
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = (D + BW - 1) / BW;
    int ib = 0, rem = (int)blockIdx.x;
    while (rem >= nb - ib) { rem -= nb - ib; ib++; }
    const int jb = ib + rem;
    const bool same = ib == jb;
    const int group = (int)blockIdx.y;
    const int64_t row0 = (int64_t)group * kGroupRows;
    const int rows_g = (int)(N - row0 < kGroupRows ? N - row0 : kGroupRows);
    const int wi = wave >> 1, wj = wave & 1;
    const int it = 2 * ib + wi, jt = 2 * jb + wj;
    const bool active = jt >= it && it * 32 < D && jt * 32 < D;

    // staging: this work-item's column of both blocks is fixed, its rows are (tid >> 6) + 4 j
    const int col = tid & (BW - 1), kk0 = tid >> 6;
    const int ca = ib * BW + col, cb = jb * BW + col;
    const float ma = (mean && ca < D) ? mean[ca] : 0.f, mb = (mean && cb < D) ? mean[cb] : 0.f;
    float ra[kStage], rb[kStage];                       // the raw values of the next step; bit j of va / vb: entry j is inside the table
    unsigned va = 0, vb = 0;
    auto fetch = [&](int sub) {
        va = vb = 0;
#pragma unroll
        for (int j = 0; j < kStage; j++) {
            const int r = sub * KC + kk0 + 4 * j;
            const bool in = r < rows_g;
            const int64_t off = (row0 + r) * D;
            ra[j] = rb[j] = 0.f;
            if (in && ca < D) { ra[j] = x[off + ca]; va |= 1u << j; }
            if (!same && in && cb < D) { rb[j] = x[off + cb]; vb |= 1u << j; }
        }
    };
    // centred when it is written to LDS, so that the loads stay in flight behind the matrix-core steps; outside the table: +0.0
    auto centred = [&](float v, float m, unsigned valid, int j) { return ((valid >> j) & 1) ? (mean ? v - m : v) : 0.f; };

    double S[16];
#pragma unroll
    for (int r = 0; r < 16; r++) S[r] = 0.0;
    f32x16_t acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int nsub = (rows_g + KC - 1) / KC;            // chunks are whole multiples of KC rows: a staged step never straddles two chunks
    fetch(0);
    for (int sub = 0; sub < nsub; sub++) {
        __syncthreads();                                // the previous step's reads are over
#pragma unroll
        for (int j = 0; j < kStage; j++) {
            as[kk0 + 4 * j][col] = centred(ra[j], ma, va, j);
            if (!same) bs[kk0 + 4 * j][col] = centred(rb[j], mb, vb, j);
        }
        __syncthreads();
        if (sub + 1 < nsub) fetch(sub + 1);
        const int q = sub / (kChunkRows / KC), k0 = (sub % (kChunkRows / KC)) * KC;
        const int rows = rows_g - q * kChunkRows < kChunkRows ? rows_g - q * kChunkRows : kChunkRows;
        if (k0 == 0) {
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = 0.f;
        }
        const int steps = ((rows - k0 < KC ? rows - k0 : KC) + 1) / 2;     // an odd tail takes the staged row of zeros
        if (active) {
            const float (*bt)[BW] = same ? as : bs;
            const int ai = wi * 32 + (lane & 31), bj = wj * 32 + (lane & 31), half = lane >> 5;
            if (steps == KC / 2) {                      // a whole step: unrolled, so the LDS reads run ahead of the chain
#pragma unroll
                for (int st = 0; st < KC / 2; st++)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[2 * st + half][ai], bt[2 * st + half][bj], acc, 0, 0, 0);
            } else {
                for (int st = 0; st < steps; st++)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[2 * st + half][ai], bt[2 * st + half][bj], acc, 0, 0, 0);
            }
        }
        if (k0 + KC >= rows) {                          // the chunk's chain is complete
#pragma unroll
            for (int r = 0; r < 16; r++) S[r] += (double)acc[r];
        }
    }
    if (!active) return;
    const int j = jt * 32 + (lane & 31);
    if (j >= D) return;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int i = it * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (i < D) {
            partial[((int64_t)i * D + j) * groups + group] = S[r];
            if (it != jt) partial[((int64_t)j * D + i) * groups + group] = S[r];
        }
    }
}

__global__ __launch_bounds__(NT) void directions_edit_kernel(const float* __restrict__ ws, const float* __restrict__ comps, const float* __restrict__ scale,
                                                             const float* __restrict__ sigmas, const int32_t* __restrict__ layer_mask,
                                                             float* __restrict__ out, int64_t total, int L, int D, int K, int T)
{
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
        const int d = (int)(i % D), l = (int)((i / D) % L);
        const int64_t row = i / ((int64_t)D * L);       // (s K + k) T + t
        const int t = (int)(row % T), k = (int)((row / T) % K);
        const int64_t s = row / ((int64_t)T * K);
        const float base = ws[(s * L + l) * D + d];
        out[i] = layer_mask[l] ? __fmaf_rn(__fmul_rn(sigmas[t], scale[k]), comps[(int64_t)k * D + d], base) : base;
    }
}

int merge(const double* partial, double* out, int64_t values, int count, double div, int64_t N, int D, hipStream_t s)
{
    SbgProfScope prof(s, SBG_K_DIRECTIONS, 0.0, 8.0 * (double)values * count + 8.0 * (double)values, {kMerge, sbg_clip31(N), D, count});
    return merge_partials<double>(partial, out, values, count, div, s);
}

int64_t gram_groups(int64_t N) { return (N + kGroupRows - 1) / kGroupRows; }

} // namespace

extern "C" int64_t sbg_directions_mean_workspace(int64_t N, int D)
{
    if (N < 1 || D < 1 || D > kMaxD || N > ((int64_t)1 << 40)) return -1;
    const int64_t chunks = (N + kMeanRows - 1) / kMeanRows;
    if (chunks > INT32_MAX) return -1;
    return 8 * (int64_t)D * chunks;
}

extern "C" int sbg_directions_mean(const float* x, double* out, void* workspace, int64_t N, int D, sbg_stream_t stream)
{
    SBG_CHECK(sbg_directions_mean_workspace(N, D) >= 0, "directions_mean: bad shape [%lld, %d] (N >= 1, 1 <= D <= %d)", (long long)N, D, kMaxD);
    SBG_CHECK(x && out && workspace && sbg_aligned(x, 4) && sbg_aligned(out, 8) && sbg_aligned(workspace, 8), "directions_mean: null or misaligned pointer");
    const int chunks = (int)((N + kMeanRows - 1) / kMeanRows);
    hipStream_t s = (hipStream_t)stream;
    {
        SbgProfScope prof(s, SBG_K_DIRECTIONS, 0.0, 4.0 * (double)N * D, {kMean, sbg_clip31(N), D, chunks});
        SBG_LAUNCH(directions_mean_kernel, dim3((unsigned)chunks, (unsigned)((D + kMeanCols - 1) / kMeanCols)), dim3(NT), 0, s, x, (double*)workspace, N, D,
                   chunks);
        SBG_HIP_LAUNCH_CHECK();
    }
    return merge((const double*)workspace, out, D, chunks, (double)N, N, D, s);
}

extern "C" int64_t sbg_directions_gram_workspace(int64_t N, int D)
{
    if (N < 1 || D < 1 || D > kMaxD || gram_groups(N) > 65535) return -1;
    return 8 * gram_groups(N) * D * D;
}

extern "C" int sbg_directions_gram(const float* x, const float* mean, double* out, void* workspace, int64_t N, int D, sbg_stream_t stream)
{
    SBG_CHECK(sbg_directions_gram_workspace(N, D) >= 0, "directions_gram: bad shape [%lld, %d] (1 <= N <= %lld, 1 <= D <= %d)", (long long)N, D,
              (long long)65535 * kGroupRows, kMaxD);
    SBG_CHECK(x && out && workspace && sbg_aligned(x, 4) && sbg_aligned(out, 8) && sbg_aligned(workspace, 8) && (!mean || sbg_aligned(mean, 4)),
              "directions_gram: null or misaligned pointer");
    const int groups = (int)gram_groups(N);
    const int nb = (D + BW - 1) / BW;
    hipStream_t s = (hipStream_t)stream;
    {
        SbgProfScope prof(s, SBG_K_DIRECTIONS, 2.0 * (double)N * D * D, 4.0 * (double)N * D + 8.0 * (double)groups * D * D, {kGram, sbg_clip31(N), D, groups});
        SBG_LAUNCH(directions_gram_kernel, dim3((unsigned)(nb * (nb + 1) / 2), (unsigned)groups), dim3(NT), 0, s, x, mean, (double*)workspace, N, D, groups);
        SBG_HIP_LAUNCH_CHECK();
    }
    return merge((const double*)workspace, out, (int64_t)D * D, groups, 1.0, N, D, s);
}

extern "C" int sbg_directions_edit(const float* ws, const float* comps, const float* scale, const float* sigmas, const int32_t* layer_mask, float* out,
                                   int S, int L, int D, int K, int T, sbg_stream_t stream)
{
    SBG_CHECK(S >= 0 && K >= 0 && T >= 0 && L >= 1 && D >= 1 && D <= kMaxD, "directions_edit: bad sizes S=%d L=%d D=%d K=%d T=%d (L >= 1, 1 <= D <= %d)", S, L, D,
              K, T, kMaxD);
    const int64_t rows = (int64_t)S * K * T;
    if (rows == 0) return SBG_OK;
    SBG_CHECK(rows <= ((int64_t)1 << 40) / ((int64_t)L * D), "directions_edit: a table of %lld x %d x %d is too large", (long long)rows, L, D);
    SBG_CHECK(ws && comps && scale && sigmas && layer_mask && out && sbg_aligned(ws, 4) && sbg_aligned(comps, 4) && sbg_aligned(scale, 4) &&
              sbg_aligned(sigmas, 4) && sbg_aligned(layer_mask, 4) && sbg_aligned(out, 4), "directions_edit: null or misaligned pointer");
    const int64_t total = rows * L * D;
    hipStream_t s = (hipStream_t)stream;
    SbgProfScope prof(s, SBG_K_DIRECTIONS, 2.0 * (double)total, 8.0 * (double)total, {kEdit, S, K, T, L, D});
    SBG_LAUNCH(directions_edit_kernel, dim3(sbg_stream_grid(total, NT)), dim3(NT), 0, s, ws, comps, scale, sigmas, layer_mask, out, total, L, D, K, T);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}
