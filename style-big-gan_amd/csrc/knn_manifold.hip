// knn_manifold.hip -- the k-nearest-neighbour arithmetic of the precision / recall metric (metrics/precision_recall.py of the reference,
// `compute_distances` + `kthvalue` + `(dist <= kth).any`) as an implicit rows x manifold GEMM on the matrix cores whose [R, C] distance
// matrix never leaves the chip.  Features are fp16 [*, F], dense rows.
//   kth_radius:   out[i] = (k + 1)-th smallest of d(rows[i], manifold[j]) over j            (fp16)
//   in_manifold:  out[i] = any_j d(probes[i], manifold[j]) <= radius[j]                      (uint8)
//   probe:        count[i] = |{ j : d(probes[i], manifold[j]) <= radius[j] }|  (int32),  nearest[i] = min_j d(probes[i], manifold[j])  (fp16)
//                 -- the pass behind density / coverage (Naeem et al., ICML 2020) and, as count > 0, behind precision / recall
//   topk:         d2[i, t], index[i, t] = the t-th smallest (d2(queries[i], manifold[j]), j) over j != exclude[i]   (fp32, int32; t < k <= 8)
//                 -- the feature-space search of nearest_neighbors.py; selection is on d2 itself, nothing is rounded to fp16
//   realism:      score[i] = max_j radius[j] / d(probes[i], manifold[j]) over the j with radius[j] >= 0 and j != exclude[i]  (fp32; +inf where
//                 d == 0; 0 when there is no such j),  index[i] = the lowest j attaining it  (int32; -1 when there is none)
//                 -- the realism score of Kynkaanniemi et al. (NeurIPS 2019, section 5); a pruned ball is a negative radius
// Arithmetic: n(x) = sum x_f^2 and s(x, y) = sum x_f y_f are fp32 sums of fp16 products; d2 = max((n(x) + n(y)) - 2 s, 0) in fp32;
// d = fp16_rn(sqrt_f32(d2)).  Rounding is monotone, so the radius kernel selects on d2 (and the probe pass takes its minimum on d2) and
// rounds the selected value once.
//
// Launches: a norm pass (one wave per row), the tile kernel, and -- when the manifold columns are split over workgroups -- a merge.
// Tile kernel: workgroup = 256 lanes = 4 waves, tile 128 manifold points (MFMA A operand, rows of the accumulator = registers of a
// lane) x 128 query rows (B operand, accumulator column = lane & 15), K-step 64, v_mfma_f32_16x16x32_f16.  So a lane holds, for each
// of 4 query rows, 16 manifold candidates per tile, and reduces them into per-query registers: a sorted list of the KL smallest d2
// (radius), a flag (membership) or a count and a running minimum (probe).  Staging is global -> VGPR -> LDS in full 128-B lines
// (8 lanes per row), issue early / write late, two LDS stages, one barrier per K-step.  LDS image per operand: [k-group 0..7][130
// cells of 16 B]: the 2-cell pad makes the 16 cells a quarter-wave writes (2 rows x 8 k-groups) distinct mod 16, and a fragment read
// touches 16 consecutive cells: both conflict-free.
// A workgroup owns one query tile and a contiguous run of manifold tiles.  With one run per query tile the result is written directly
// (variant `single`); otherwise every run writes its partial list / flag / {count, minimum} pair to the workspace and a second launch
// merges the runs in index order (`split` + `merge`).  The lists, their keys, the split and the merge of lists are knn_select.h's, with
// its order and tie rules; an OR, an integer sum and a minimum do not depend on the order either, and there are no atomics: two runs
// give the same bits.
// Realism candidates are RealismKey (below): one unsigned maximum orders by score, then by the lower index, and is order-free as well.
// Top-k candidates are knn_select.h's KeyF32, which needs d2 never negative and never -0: n(x) + n(y) is a sum of squares, so +0 or
// positive; a - b of two floats is -0 only for a = -0, b = +0 (a - a is +0 under round-to-nearest), so (n(x) + n(y)) - 2 s is +0,
// positive, or negative and then replaced by the +0 of fmaxf(., 0).  A row past the end, or equal to exclude[q], gets the sentinel.
// Launch-log key: kind SBG_K_PR, dims = {variant (0 single, 1 split, 2 merge, 3 norms), R, C, F, k, runs, 0 radius / 1 membership / 2 probe / 3 top-k / 4 realism}.
#include "conv_common.h"
#include "knn_select.h"
#include "reduce.h"

using namespace sbgconv;
using namespace knnsel;

namespace {

constexpr int kPrSingle = 0, kPrSplit = 1, kPrMerge = 2, kPrNorms = 3;
constexpr int kRadius = 0, kMember = 1, kProbe = 2, kTopk = 3, kRealism = 4;       // what the tile kernel reduces a query row's distances to (dims[6] of a record)

constexpr int BK = 64;                      // K-step
constexpr int KG = BK / 8;                  // 16-B k-groups per K-step
constexpr int KGS = BT + 2;                 // cells per k-group (padded, see above)
constexpr int OP_BYTES = KG * KGS * 16;     // one operand of one stage
constexpr int STAGE = 2 * OP_BYTES;
constexpr int PARAM_OFF = 2 * STAGE;        // behind the two stages: norms and radii of the manifold tile, double-buffered by tile parity
constexpr int LDS_BYTES = PARAM_OFF + 2 * 2 * BT * 4;
constexpr int kMaxK1 = 8;                   // k + 1 <= 8
constexpr int kMaxTopk = 8;                 // top-k: 1 <= k <= 8

struct KnnArgs {
    const unsigned short* q; const unsigned short* m;     // query rows [R, F], manifold [C, F]
    const float* nq; const float* nm;                      // their squared norms
    const unsigned short* radius;                          // membership and probe: fp16 [C]
    union { void* out; float* d2; };                       // radius fp16 [R], membership uint8 [R], probe count int32 [R]; top-k: d2 [R, k]; realism: score fp32 [R]
    union { void* nearest = nullptr; int32_t* index; };    // the probe's second output, fp16 [R]; top-k: index [R, k]; realism: index [R]
    void* part;
    const int32_t* exclude = nullptr;                      // top-k and realism: [R] or null
    int R, C, F, k, runs, ctiles, tiles_per_run;
};

// n[r] = sum_f x[r, f]^2: one wave per row, 16-B loads, a lane-strided fp32 sum and a butterfly.
__global__ __launch_bounds__(256) void knn_norms_kernel(const unsigned short* __restrict__ x, float* __restrict__ n, int rows, int F)
{
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const unsigned short* p = x + (int64_t)row * F;
    float s = 0.f;
    for (int c = lane * 8; c < F; c += 512) {
        const short8_t v = *reinterpret_cast<const short8_t*>(p + c);
#pragma unroll
        for (int e = 0; e < 8; e++) { const float f = f16_bits_to_f32((unsigned short)v[e]); s = fmaf(f, f, s); }
    }
    s = wave_sum(s);
    if (lane == 0) n[row] = s;
}

__device__ __forceinline__ float dist2(float nx, float ny, float s)
{
#pragma clang fp contract(off)
    return fmaxf((nx + ny) - 2.0f * s, 0.f);
}

__device__ __forceinline__ float dist_f16(float d2) { return (float)(_Float16)sqrtf(d2); }

struct ProbePart { int count; float d2; };                 // a run's share of a probe row: balls that hold it, smallest d2

// A realism candidate: (uint64(bits(score)) << 32) | ~row, unsigned, so the LARGEST key is the highest score and, among equal scores, the
// lowest row.  A score is +0, positive or +inf (radius >= 0 over d > 0, its sign bit cleared so that a radius of -0 counts as +0): such
// floats order as their bits do.  Rows are below 2^24, so ~row is never 0 and every candidate's key is above `none`; `none` itself
// decodes to what a row without candidates gets, score 0 and index -1.  Keys of distinct rows are distinct: a maximum over them does
// not depend on the order, the split or the launch.  Every candidate is divided: there is no pre-test.
struct RealismKey {
    static constexpr uint64_t none = 0;
    static __device__ __forceinline__ uint64_t make(float radius, float d, int row)
    {
        const float q = d == 0.f ? __builtin_inff() : radius / d;          // one IEEE division of the two fp16 values; 0 / 0 is never kept
        return ((uint64_t)(__float_as_uint(q) & 0x7fffffffu) << 32) | (uint32_t)~row;
    }
    static __device__ __forceinline__ void store(uint64_t key, float* score, int32_t* index)
    {
        *score = __uint_as_float((uint32_t)(key >> 32));
        *index = (int32_t)~(uint32_t)key;
    }
};

// What the radius mode writes for row q from its merged list of d2 (a multiset: kthvalue counts duplicates): the k-th entry, as fp16
struct RadiusFinish {
    using type = float;
    static constexpr float none = __builtin_inff();
    unsigned short* out; int k;
    template <int KL>
    __device__ __forceinline__ void operator()(int q, const float (&M)[KL]) const
    {
        float r = M[0];         // a select of loaded values: written `(t == k) ? M[t] : r` it compiles to one load at a computed address and M goes to scratch
#pragma unroll
        for (int t = 1; t < KL; t++) { const float m = M[t]; r = (t == k) ? m : r; }
        out[q] = f32_to_f16_bits(sqrtf(r));
    }
};

template <int KL, int MODE>
__device__ __forceinline__ void knn_tile_body(const KnnArgs& p)
{
    constexpr bool MEMBER = MODE == kMember, PROBE = MODE == kProbe, TOPK = MODE == kTopk, REALISM = MODE == kRealism;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* const prm = reinterpret_cast<float*>(smem + PARAM_OFF);          // [parity][0: norm, 1: radius][BT]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qt = blockIdx.x / p.runs, run = blockIdx.x - qt * p.runs;
    const int q0 = qt * BT;
    const int t_begin = run * p.tiles_per_run;
    const int t_end = min(t_begin + p.tiles_per_run, p.ctiles);

    // staging coordinates: 8 consecutive lanes read one 128-B line of a row
    const int lrow = tid >> 3, kg = tid & 7;
    int64_t q_off[4]; bool q_ok[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int r = q0 + lrow + 32 * i;
        q_ok[i] = r < p.R;
        q_off[i] = (int64_t)(q_ok[i] ? r : 0) * p.F;
    }

    // MFMA coordinates: waves 2 (manifold) x 2 (query), wave tile 64 x 64 = 4 x 4 MFMA tiles
    const int wc = (wave >> 1) * 64, wp = (wave & 1) * 64;
    const int fr = lane & 15, fg = lane >> 4;
    float nqv[4];
#pragma unroll
    for (int j = 0; j < 4; j++) { const int r = q0 + wp + 16 * j + fr; nqv[j] = r < p.R ? p.nq[r] : 0.f; }

    uint64_t T[4][TOPK ? KL : 1];       // top-k: the lists of keys
    uint64_t best[4];                   // realism: the largest key
    int excl[4];
    if constexpr (TOPK || REALISM) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int r = q0 + wp + 16 * j + fr;
            excl[j] = (r < p.R && p.exclude) ? p.exclude[r] : -1;
            best[j] = RealismKey::none;
            if constexpr (TOPK) {
#pragma unroll
                for (int t = 0; t < KL; t++) T[j][t] = KeyF32::none;
            }
        }
    }

    float L[4][KL];
    int inside[4];                      // membership: the flag; probe: the count
    float nearest[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        inside[j] = 0;
        nearest[j] = __builtin_inff();
#pragma unroll
        for (int t = 0; t < KL; t++) L[j][t] = __builtin_inff();
    }

    const int nsteps = (p.F + BK - 1) / BK;
    for (int tile = t_begin; tile < t_end; tile++) {
        const int c0 = tile * BT, par = (tile - t_begin) & 1;
        int64_t m_off[4]; bool m_ok[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int c = c0 + lrow + 32 * i;
            m_ok[i] = c < p.C;
            m_off[i] = (int64_t)(m_ok[i] ? c : 0) * p.F;
        }
        if (tid < BT) {       // a padded column is at +inf (and has a negative radius): read after the K loop's barriers
            const int c = c0 + tid;
            prm[(par * 2 + 0) * BT + tid] = c < p.C ? p.nm[c] : __builtin_inff();
            if (MEMBER || PROBE || REALISM) prm[(par * 2 + 1) * BT + tid] = c < p.C ? f16_bits_to_f32(p.radius[c]) : -1.f;
        }

        short8_t ra[4], rb[4];
        auto issue_loads = [&](int step) {
            const int k0 = step * BK + kg * 8;
            const bool kok = k0 < p.F;          // F % 8 == 0: a 16-B piece is wholly inside or outside the row
#pragma unroll
            for (int i = 0; i < 4; i++) {
                short8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
                if (kok && m_ok[i]) v = *reinterpret_cast<const short8_t*>(p.m + m_off[i] + k0);
                ra[i] = v;
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                short8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
                if (kok && q_ok[i]) v = *reinterpret_cast<const short8_t*>(p.q + q_off[i] + k0);
                rb[i] = v;
            }
        };
        auto write_stage = [&](int buf) {
            unsigned char* sa = smem + buf * STAGE;
            unsigned char* sb = sa + OP_BYTES;
#pragma unroll
            for (int i = 0; i < 4; i++) *reinterpret_cast<short8_t*>(sa + (kg * KGS + lrow + 32 * i) * 16) = ra[i];
#pragma unroll
            for (int i = 0; i < 4; i++) *reinterpret_cast<short8_t*>(sb + (kg * KGS + lrow + 32 * i) * 16) = rb[i];
        };

        float4_t acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};

        issue_loads(0);
        write_stage(0);
        __syncthreads();
        for (int s = 0; s < nsteps; s++) {
            const int buf = s & 1;
            if (s + 1 < nsteps) issue_loads(s + 1);
            const unsigned char* sa = smem + buf * STAGE;
            const unsigned char* sb = sa + OP_BYTES;
#pragma unroll
            for (int ks = 0; ks < 2; ks++) {
                short8_t fa[4], fb[4];
#pragma unroll
                for (int i = 0; i < 4; i++) fa[i] = *reinterpret_cast<const short8_t*>(sa + ((4 * ks + fg) * KGS + wc + 16 * i + fr) * 16);
#pragma unroll
                for (int j = 0; j < 4; j++) fb[j] = *reinterpret_cast<const short8_t*>(sb + ((4 * ks + fg) * KGS + wp + 16 * j + fr) * 16);
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[i][j] = Mfma<f16_mfma>::run(fa[i], fb[j], acc[i][j]);
            }
            if (s + 1 < nsteps) write_stage(buf ^ 1);
            __syncthreads();
        }

        // the lane holds manifold points c0 + wc + 16 i + 4 fg + e of query rows q0 + wp + 16 j + fr
#pragma unroll
        for (int i = 0; i < 4; i++) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int col = wc + 16 * i + 4 * fg + e;
                const float nmv = prm[(par * 2 + 0) * BT + col];
                const float rv = (MEMBER || PROBE || REALISM) ? prm[(par * 2 + 1) * BT + col] : 0.f;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float d2 = dist2(nqv[j], nmv, acc[i][j][e]);
                    if constexpr (TOPK) { const int row = c0 + col; keep_smallest<KL>(T[j], (row < p.C && row != excl[j]) ? KeyF32::make(d2, row) : KeyF32::none); }
                    else if constexpr (REALISM) {       // a padded column has radius -1, as a pruned point has: its row needs no test
                        const int row = c0 + col;
                        const uint64_t key = (rv >= 0.f && row != excl[j]) ? RealismKey::make(rv, dist_f16(d2), row) : RealismKey::none;
                        best[j] = key > best[j] ? key : best[j];
                    }
                    else if (MEMBER) inside[j] |= (dist_f16(d2) <= rv) ? 1 : 0;
                    else if (PROBE) { inside[j] += (dist_f16(d2) <= rv) ? 1 : 0; nearest[j] = fminf(nearest[j], d2); }
                    else keep_smallest<KL>(L[j], d2);
                }
            }
        }
    }

    // merge the lane groups and the two manifold waves that share a query row; the staging area is free after the last barrier
    const int q = q0 + tid;
    if constexpr (TOPK) {       // at KL = 8 the image is 128 * 65 * 8 B = 66560 B, the two stages exactly
        finish_run<KL, PARAM_OFF>(smem, T, q0, p.R, p.runs, run, reinterpret_cast<uint64_t*>(p.part), KeyFinish<KeyF32>{p.d2, p.index, p.k});
    } else if (MEMBER) {
        int* fl = reinterpret_cast<int*>(smem);                  // [manifold wave][BT]
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int v = inside[j];
            v |= __shfl_xor(v, 16, 64);
            v |= __shfl_xor(v, 32, 64);
            if (fg == 0) fl[(wave >> 1) * BT + wp + 16 * j + fr] = v;
        }
        __syncthreads();
        if (tid < BT && q < p.R) {
            const unsigned char f = (unsigned char)((fl[tid] | fl[BT + tid]) != 0);
            if (p.runs == 1) reinterpret_cast<unsigned char*>(p.out)[q] = f;
            else reinterpret_cast<unsigned char*>(p.part)[(int64_t)run * p.R + q] = f;
        }
    } else if (PROBE) {
        int* cn = reinterpret_cast<int*>(smem);                  // [manifold wave][BT] counts, then [manifold wave][BT] minima
        float* mn = reinterpret_cast<float*>(smem) + 2 * BT;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int c = inside[j];
            float v = nearest[j];
            c += __shfl_xor(c, 16, 64); v = fminf(v, __shfl_xor(v, 16, 64));
            c += __shfl_xor(c, 32, 64); v = fminf(v, __shfl_xor(v, 32, 64));
            if (fg == 0) { cn[(wave >> 1) * BT + wp + 16 * j + fr] = c; mn[(wave >> 1) * BT + wp + 16 * j + fr] = v; }
        }
        __syncthreads();
        if (tid < BT && q < p.R) {
            const int c = cn[tid] + cn[BT + tid];
            const float v = fminf(mn[tid], mn[BT + tid]);
            if (p.runs == 1) {
                reinterpret_cast<int*>(p.out)[q] = c;
                reinterpret_cast<unsigned short*>(p.nearest)[q] = f32_to_f16_bits(sqrtf(v));
            } else {
                reinterpret_cast<ProbePart*>(p.part)[(int64_t)run * p.R + q] = ProbePart{c, v};
            }
        }
    } else if constexpr (REALISM) {
        uint64_t* bs = reinterpret_cast<uint64_t*>(smem);        // [manifold wave][BT] keys
#pragma unroll
        for (int j = 0; j < 4; j++) {
            uint64_t v = best[j], o;
            o = __shfl_xor(v, 16, 64); v = o > v ? o : v;
            o = __shfl_xor(v, 32, 64); v = o > v ? o : v;
            if (fg == 0) bs[(wave >> 1) * BT + wp + 16 * j + fr] = v;
        }
        __syncthreads();
        if (tid < BT && q < p.R) {
            const uint64_t a = bs[tid], b = bs[BT + tid], v = a > b ? a : b;
            if (p.runs == 1) RealismKey::store(v, p.d2 + q, p.index + q);
            else reinterpret_cast<uint64_t*>(p.part)[(int64_t)run * p.R + q] = v;
        }
    } else {
        finish_run<KL, PARAM_OFF>(smem, L, q0, p.R, p.runs, run, reinterpret_cast<float*>(p.part), RadiusFinish{reinterpret_cast<unsigned short*>(p.out), p.k});
    }
}

template <int KL, bool MEMBER>
__global__ __launch_bounds__(256) void knn_tile_kernel(KnnArgs p) { knn_tile_body<KL, MEMBER ? kMember : kRadius>(p); }

__global__ __launch_bounds__(256) void knn_probe_tile_kernel(KnnArgs p) { knn_tile_body<4, kProbe>(p); }

__global__ __launch_bounds__(256) void knn_realism_tile_kernel(KnnArgs p) { knn_tile_body<4, kRealism>(p); }

// two waves per SIMD: without the bound KL = 8 takes 198 + 64 registers and a CU holds one workgroup; with it 254, no scratch
template <int KL>
__global__ __launch_bounds__(256, 2) void knn_topk_tile_kernel(KnnArgs p) { knn_tile_body<KL, kTopk>(p); }

// Second stage of the split variant: one work-item per query row walks the runs in index order (the lists: knn_select.h's merge_runs).
__global__ __launch_bounds__(256) void knn_merge_member_kernel(const unsigned char* __restrict__ part, unsigned char* __restrict__ out, int R, int runs)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= R) return;
    unsigned char f = 0;
    for (int s = 0; s < runs; s++) f |= part[(int64_t)s * R + q];
    out[q] = f;
}

__global__ __launch_bounds__(256) void knn_merge_probe_kernel(const ProbePart* __restrict__ part, int* __restrict__ count, unsigned short* __restrict__ nearest,
                                                              int R, int runs)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= R) return;
    int c = 0;
    float v = __builtin_inff();
    for (int s = 0; s < runs; s++) { const ProbePart t = part[(int64_t)s * R + q]; c += t.count; v = fminf(v, t.d2); }
    count[q] = c;
    nearest[q] = f32_to_f16_bits(sqrtf(v));
}

__global__ __launch_bounds__(256) void knn_merge_realism_kernel(const uint64_t* __restrict__ part, float* __restrict__ score, int32_t* __restrict__ index,
                                                                int R, int runs)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= R) return;
    uint64_t v = RealismKey::none;
    for (int s = 0; s < runs; s++) { const uint64_t t = part[(int64_t)s * R + q]; v = t > v ? t : v; }
    RealismKey::store(v, score + q, index + q);
}

int list_len(int k) { return k + 1 <= 4 ? 4 : 8; }         // radius: the (k + 1)-th neighbour

// The plan of a mode: its k limits, and what a run leaves per query row -- a list of floats (radius), one byte (membership; the bytes
// of all rows together are rounded up to 16), a ProbePart (probe), a list of 64-bit keys (top-k), one RealismKey (realism).
bool knn_plan(int R, int C, int k, int mode, RunPlan& pl)
{
    if (mode == kTopk ? (k < 1 || k > kMaxTopk) : (k < 0 || k + 1 > kMaxK1)) return false;
    const int64_t part = mode == kMember ? 1 : mode == kProbe ? (int64_t)sizeof(ProbePart) : mode == kRealism ? 8 : mode == kTopk ? 8 * topk_list_len(k) : 4 * list_len(k);
    if (!plan_runs(R, C, 4, part, pl)) return false;
    if (mode == kMember) pl.bytes = up16(pl.bytes);
    return true;
}

// one_excluded: a top-k search that may skip one manifold row per query
int knn_check(const char* what, const void* q, const void* m, const void* out, const void* ws, int R, int C, int64_t F, int k, int mode, bool one_excluded,
              RunPlan& pl)
{
    SBG_CHECK(q && m && out && ws, "%s: null pointer", what);
    if (mode == kTopk) {
        SBG_CHECK(k >= 1 && k <= kMaxTopk, "%s: k = %d neighbours, 1 to %d are supported", what, k, kMaxTopk);
        SBG_CHECK(R >= 1 && C >= 1 && R <= kMaxRows && C <= kMaxRows, "%s: bad sizes Q=%d M=%d (1 to 2^24 each)", what, R, C);
        SBG_CHECK(C - (one_excluded ? 1 : 0) >= k, "%s: the manifold has %d rows%s, %d neighbours need %d", what, C, one_excluded ? " and one may be excluded" : "", k,
                  k + (one_excluded ? 1 : 0));
    } else {
        SBG_CHECK(k >= 0 && k + 1 <= kMaxK1, "%s: k + 1 = %d neighbours, at most %d are supported", what, k + 1, kMaxK1);
        SBG_CHECK(R >= 1 && C >= 1 && R <= kMaxRows && C <= kMaxRows, "%s: bad sizes R=%d C=%d", what, R, C);
        SBG_CHECK(C >= k + 1, "%s: the manifold has %d points, the (k + 1)-th neighbour needs %d", what, C, k + 1);
    }
    SBG_CHECK(F >= 8 && F % 8 == 0 && F <= (1 << 24), "%s: the feature width %lld must be a multiple of 8 (16-byte pieces) in [8, 2^24]", what, (long long)F);
    SBG_CHECK(sbg_aligned16(q) && sbg_aligned16(m) && sbg_aligned16(ws), "%s: features and workspace must be 16-byte aligned", what);
    SBG_CHECK(knn_plan(R, C, k, mode, pl), "%s: bad sizes", what);
    return SBG_OK;
}

int knn_norms(const unsigned short* x, float* n, int rows, int F, hipStream_t s)
{
    SbgProfScope prof(s, SBG_K_PR, 2.0 * rows * (double)F, 2.0 * rows * (double)F + 4.0 * rows, {kPrNorms, rows, 0, F});
    SBG_LAUNCH(knn_norms_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, n, rows, F);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

template <int KL, int MODE>
constexpr auto knn_tile_kernel_of()
{
    if constexpr (MODE == kTopk) return knn_topk_tile_kernel<KL>;
    else if constexpr (MODE == kProbe) return knn_probe_tile_kernel;
    else if constexpr (MODE == kRealism) return knn_realism_tile_kernel;
    else return knn_tile_kernel<KL, MODE == kMember>;
}

template <int KL, int MODE>
int knn_launch_tiles(const KnnArgs& a, const RunPlan& pl, hipStream_t s)
{
    constexpr auto kernel = knn_tile_kernel_of<KL, MODE>();
    if (!SBG_RAISE_LDS_ONCE(kernel, LDS_BYTES))
        return sbg_fail(SBG_ERR_LAUNCH, "knn_manifold: cannot raise the dynamic LDS limit to %d bytes", LDS_BYTES);
    SbgProfScope prof(s, SBG_K_PR, 2.0 * a.R * (double)a.C * a.F, 2.0 * ((double)a.R + a.C) * a.F,
                      {pl.runs == 1 ? kPrSingle : kPrSplit, a.R, a.C, a.F, a.k, pl.runs, MODE});
    SBG_LAUNCH(kernel, dim3((unsigned)(pl.rtiles * pl.runs)), dim3(256), LDS_BYTES, s, a);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

// What the entry points share: argument checks, the plan, the norm passes and the tile launch.  On SBG_OK with pl.runs > 1 the
// caller launches its merge over a.part.  The caller has set the fields of `a` that only its mode has (nearest | index, exclude).
template <int MODE>
int knn_run(const char* what, const void* q, const void* m, const void* radius, int R, int C, int64_t F, int k, void* out, void* workspace,
            hipStream_t s, KnnArgs& a, RunPlan& pl)
{
    const int rc = knn_check(what, q, m, out, workspace, R, C, F, k, MODE, a.exclude != nullptr, pl);
    if (rc != SBG_OK) return rc;
    char* ws = (char*)workspace;
    a.q = (const unsigned short*)q; a.m = (const unsigned short*)m;
    a.nq = (const float*)(ws + pl.nq_off); a.nm = (const float*)(ws + pl.nm_off); a.radius = (const unsigned short*)radius;
    a.out = out; a.part = ws + pl.part_off;
    a.R = R; a.C = C; a.F = (int)F; a.k = k; a.runs = pl.runs; a.ctiles = pl.ctiles; a.tiles_per_run = pl.tiles_per_run;
    int st = knn_norms(a.q, (float*)(ws + pl.nq_off), R, a.F, s);
    if (st != SBG_OK) return st;
    st = knn_norms(a.m, (float*)(ws + pl.nm_off), C, a.F, s);
    if (st != SBG_OK) return st;
    if constexpr (MODE == kTopk) return with_list_len(topk_list_len(k), [&](auto kl) { return knn_launch_tiles<decltype(kl)::value, kTopk>(a, pl, s); });
    else if constexpr (MODE != kRadius) return knn_launch_tiles<4, MODE>(a, pl, s);
    else return list_len(k) == 4 ? knn_launch_tiles<4, kRadius>(a, pl, s) : knn_launch_tiles<8, kRadius>(a, pl, s);
}

} // namespace

extern "C" int64_t sbg_knn_workspace(int R, int C, int k, int membership)
{
    RunPlan pl;
    if (!knn_plan(R, C, membership ? 0 : k, membership ? kMember : kRadius, pl)) return -1;
    return pl.bytes;
}

extern "C" int sbg_knn_kth_radius(const void* rows, const void* manifold, int R, int C, int64_t F, int k, void* out, void* workspace, sbg_stream_t stream)
{
    hipStream_t s = (hipStream_t)stream;
    KnnArgs a; RunPlan pl;
    const int st = knn_run<kRadius>("knn_kth_radius", rows, manifold, nullptr, R, C, F, k, out, workspace, s, a, pl);
    if (st != SBG_OK) return st;
    if (pl.runs > 1) {
        const int KL = list_len(k);
        SbgProfScope prof(s, SBG_K_PR, 0.0, 4.0 * R * (double)pl.runs * KL + 2.0 * R, {kPrMerge, R, C, a.F, k, pl.runs, 0});
        return merge_runs(KL, a.part, R, pl.runs, RadiusFinish{(unsigned short*)out, k}, s);       // KL = 1 is built and never taken here
    }
    return SBG_OK;
}

extern "C" int sbg_knn_in_manifold(const void* probes, const void* manifold, const void* radius, int P, int C, int64_t F, uint8_t* out, void* workspace,
                                   sbg_stream_t stream)
{
    SBG_CHECK(radius, "knn_in_manifold: null pointer");
    hipStream_t s = (hipStream_t)stream;
    KnnArgs a; RunPlan pl;
    const int st = knn_run<kMember>("knn_in_manifold", probes, manifold, radius, P, C, F, 0, out, workspace, s, a, pl);
    if (st != SBG_OK) return st;
    if (pl.runs > 1) {
        SbgProfScope prof(s, SBG_K_PR, 0.0, (double)P * pl.runs + P, {kPrMerge, P, C, a.F, 0, pl.runs, 1});
        SBG_LAUNCH(knn_merge_member_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, (const unsigned char*)a.part, (unsigned char*)out, P, pl.runs);
        SBG_HIP_LAUNCH_CHECK();
    }
    return SBG_OK;
}

extern "C" int64_t sbg_knn_probe_workspace(int P, int C)
{
    RunPlan pl;
    if (!knn_plan(P, C, 0, kProbe, pl)) return -1;
    return pl.bytes;
}

extern "C" int sbg_knn_probe(const void* probes, const void* manifold, const void* radius, int P, int C, int64_t F, int32_t* count, void* nearest,
                             void* workspace, sbg_stream_t stream)
{
    SBG_CHECK(radius && nearest, "knn_probe: null pointer");
    hipStream_t s = (hipStream_t)stream;
    KnnArgs a; RunPlan pl;
    a.nearest = nearest;
    const int st = knn_run<kProbe>("knn_probe", probes, manifold, radius, P, C, F, 0, count, workspace, s, a, pl);
    if (st != SBG_OK) return st;
    if (pl.runs > 1) {
        SbgProfScope prof(s, SBG_K_PR, 0.0, 8.0 * P * (double)pl.runs + 6.0 * P, {kPrMerge, P, C, a.F, 0, pl.runs, kProbe});
        SBG_LAUNCH(knn_merge_probe_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, (const ProbePart*)a.part, (int*)count, (unsigned short*)nearest,
                   P, pl.runs);
        SBG_HIP_LAUNCH_CHECK();
    }
    return SBG_OK;
}

extern "C" int64_t sbg_knn_realism_workspace(int P, int C)
{
    RunPlan pl;
    if (!knn_plan(P, C, 0, kRealism, pl)) return -1;
    return pl.bytes;
}

extern "C" int sbg_knn_realism(const void* probes, const void* manifold, const void* radius, int P, int C, int64_t F, const int32_t* exclude, float* score,
                               int32_t* index, void* workspace, sbg_stream_t stream)
{
    SBG_CHECK(radius && index, "knn_realism: null pointer");
    hipStream_t s = (hipStream_t)stream;
    KnnArgs a; RunPlan pl;
    a.index = index; a.exclude = exclude;
    const int st = knn_run<kRealism>("knn_realism", probes, manifold, radius, P, C, F, 0, score, workspace, s, a, pl);
    if (st != SBG_OK) return st;
    if (pl.runs > 1) {
        SbgProfScope prof(s, SBG_K_PR, 0.0, 8.0 * P * (double)pl.runs + 8.0 * P, {kPrMerge, P, C, a.F, 0, pl.runs, kRealism});
        SBG_LAUNCH(knn_merge_realism_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, (const uint64_t*)a.part, score, index, P, pl.runs);
        SBG_HIP_LAUNCH_CHECK();
    }
    return SBG_OK;
}

extern "C" int64_t sbg_knn_topk_workspace(int Q, int M, int k)
{
    RunPlan pl;
    if (!knn_plan(Q, M, k, kTopk, pl)) return -1;
    return pl.bytes;
}

extern "C" int sbg_knn_topk(const void* queries, const void* manifold, int Q, int M, int64_t F, int k, const int32_t* exclude, float* d2, int32_t* index,
                            void* workspace, sbg_stream_t stream)
{
    SBG_CHECK(index, "knn_topk: null pointer");
    hipStream_t s = (hipStream_t)stream;
    KnnArgs a; RunPlan pl;
    a.index = index; a.exclude = exclude;
    const int st = knn_run<kTopk>("knn_topk", queries, manifold, nullptr, Q, M, F, k, d2, workspace, s, a, pl);
    if (st != SBG_OK) return st;
    if (pl.runs > 1) {
        const int KL = topk_list_len(k);
        SbgProfScope prof(s, SBG_K_PR, 0.0, 8.0 * Q * (double)pl.runs * KL + 8.0 * Q * k, {kPrMerge, Q, M, a.F, k, pl.runs, kTopk});
        return merge_runs(KL, a.part, Q, pl.runs, KeyFinish<KeyF32>{d2, index, k}, s);
    }
    return SBG_OK;
}
