// nn_u8.hip -- exact nearest stored images of uint8 queries: for query q the k rows j of `store` with the smallest
// d2(q, j) = sum_f (queries[q, f] - store[j, f])^2, as an implicit store x queries GEMM on the i8 matrix cores whose [M, Q] distance
// matrix never leaves the chip.  Rows are dense uint8 [*, F], F a multiple of 16.
// Arithmetic (all integer, exact): a' = a - 128 (XOR 0x80 per byte as an operand is staged) is a signed byte and leaves every
// difference unchanged; n(a') = sum a'^2 comes from a norm pass (v_dot4_u32_u8 sums of a^2 and a, n = sum a^2 - 256 sum a + 16384 F,
// int64); s = sum q' x' comes from v_mfma_i32_16x16x64_i8; d2 = n(q') + n(x') - 2 s in int64.  One product is at most 128 * 128 in
// magnitude, so an i32 accumulator holds 131071 of them; every kFlushSteps steps (kFlushSteps * BK = 65536 products) the K loop moves
// the upper part of each accumulator, acc >> 16, into a second i32 sum that counts units of 65536 (at most 3.3e9 / 65536 of them) and
// keeps acc & 0xffff, so s = 65536 hi + acc as a 64-bit integer at the end.  A launch whose F fits one such span keeps no second sum
// (variant WIDE = false).
//
// Launches: a norm pass per operand (one wave per row), the tile kernel, and -- when the stored rows are split over workgroups -- a
// merge.  The tile kernel has knn_manifold.hip's frame: workgroup = 256 lanes = 4 waves, tile 128 stored rows (MFMA A operand, rows of the
// accumulator = registers of a lane) x 128 queries (B operand, accumulator column = lane & 15), K-step 256 bytes = 4 MFMA steps
// (the kernel waits on memory, not on the matrix cores: a long K-step keeps 64 KB in flight per workgroup and halves the barriers).
// Both operands are staged by one rule (lane group g of MFMA step ks takes bytes [64 ks + 16 g, +16) of the K-step of its row), so the
// order of k inside an MFMA step cannot matter.  Staging is global -> VGPR -> LDS in full 128-B lines (16 lanes per row, two lines),
// issue early / write late, two LDS stages, one barrier per K-step; LDS image per operand [k-group 0..15][129 cells of 16 B]: the
// 1-cell pad makes the 16 cells a quarter-wave writes (one row x 16 k-groups) distinct mod 16, and a fragment read touches 16
// consecutive cells: both conflict-free.
// A candidate is the pair (d2, j) as knn_select.h's KeyU8 (d2 < 2^38, j < 2^24); a row that does not exist or is the query's excluded
// row gets the sentinel.  The lists a lane keeps per query, the split of the store tiles into runs and the merges (`single`, or
// `split` + `merge`) are knn_select.h's, with its order and tie rules: two calls give the same bits.
// Launch-log key: kind SBG_K_NN_U8, dims = {variant (0 norms, 1 single, 2 split, 3 merge), Q, M, F clipped to int, k, runs}.
#include "knn_select.h"

using namespace knnsel;

namespace {

constexpr int kNnNorms = 0, kNnSingle = 1, kNnSplit = 2, kNnMerge = 3;

constexpr int BK = 256;                    // K-step in bytes: four MFMA steps of 64
constexpr int KG = BK / 16;                 // 16-B k-groups per K-step
constexpr int KGS = BT + 1;                 // cells per k-group (padded)
constexpr int OP_BYTES = KG * KGS * 16;     // one operand of one stage
constexpr int STAGE = 2 * OP_BYTES;
constexpr int PARAM_OFF = 2 * STAGE;        // behind the two stages: norms of the store tile, double-buffered by tile parity
constexpr int LDS_BYTES = PARAM_OFF + 2 * BT * 8;
constexpr int kMaxK = 8;
constexpr int kFlushSteps = 256;            // K-steps between two flushes: 256 * 256 = 65536 products <= 131071
constexpr int64_t kMaxF = 3 * 1024 * 1024;

static_assert((int64_t)kFlushSteps * BK <= 131071, "an i32 accumulator holds at most 131071 products of 128 * 128");
static_assert(kMaxF * 65025 < ((int64_t)1 << (63 - kIndexBits)), "d2 must fit the key above the row index");
static_assert(LDS_BYTES <= 160 * 1024, "LDS of a CU");

struct NnArgs {
    const uint8_t* q; const uint8_t* m;         // queries [Q, F], store [M, F]
    const int64_t* nq; const int64_t* nm;       // n(q'), n(x')
    const int32_t* exclude;                     // [Q] or null
    int64_t* d2; int32_t* index;                // [Q, k]
    int64_t* part;                              // [Q, runs, KL] keys
    int64_t F;
    int Q, M, k, runs, ctiles, tiles_per_run;
};

static __device__ __forceinline__ int64_t wave_sum_i64(int64_t v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += (int64_t)__shfl_xor((long long)v, off, 64);
    return v;
}

// n[r] = sum_f (x[r, f] - 128)^2: one wave per row, 16-B loads.  A lane sees at most 3 * 2^20 / 64 bytes, so its sums of a^2
// (<= 49152 * 65025) and of a fit 32 unsigned bits.
__global__ __launch_bounds__(256) void nn_norms_kernel(const uint8_t* __restrict__ x, int64_t* __restrict__ n, int rows, int64_t F)
{
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const uint8_t* p = x + (int64_t)row * F;
    unsigned sq = 0, su = 0;
    for (int64_t c = lane * 16; c < F; c += 1024) {
        const int4_t v = *reinterpret_cast<const int4_t*>(p + c);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            sq = __builtin_amdgcn_udot4((unsigned)v[e], (unsigned)v[e], sq, false);
            su = __builtin_amdgcn_udot4((unsigned)v[e], 0x01010101u, su, false);
        }
    }
    const int64_t a2 = wave_sum_i64((int64_t)sq), a1 = wave_sum_i64((int64_t)su);
    if (lane == 0) n[row] = a2 - 256 * a1 + 16384 * F;
}

template <int KL, bool WIDE>
__global__ __launch_bounds__(256) void nn_tile_kernel(NnArgs p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int64_t* const prm = reinterpret_cast<int64_t*>(smem + PARAM_OFF);       // [parity][BT] norms of the store tile

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qt = blockIdx.x / p.runs, run = blockIdx.x - qt * p.runs;
    const int q0 = qt * BT;
    const int t_begin = run * p.tiles_per_run;
    const int t_end = min(t_begin + p.tiles_per_run, p.ctiles);

    // staging coordinates: 16 consecutive lanes read two 128-B lines of a row; pass i of 8 takes row lrow + 16 i of the tile
    const int lrow = tid >> 4, kg = tid & 15;

    // MFMA coordinates: waves 2 (store) x 2 (query), wave tile 64 x 64 = 4 x 4 MFMA tiles
    const int wc = (wave >> 1) * 64, wp = (wave & 1) * 64;
    const int fr = lane & 15, fg = lane >> 4;
    int64_t nqv[4]; int excl[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int r = q0 + wp + 16 * j + fr;
        nqv[j] = r < p.Q ? p.nq[r] : 0;
        excl[j] = (r < p.Q && p.exclude) ? p.exclude[r] : -1;
    }

    int64_t L[4][KL];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int t = 0; t < KL; t++) L[j][t] = KeyU8::none;

    const int nsteps = (int)((p.F + BK - 1) / BK);
    for (int tile = t_begin; tile < t_end; tile++) {
        const int c0 = tile * BT, par = (tile - t_begin) & 1;
        if (tid < BT) {       // read after the K loop's barriers
            const int c = c0 + tid;
            prm[par * BT + tid] = c < p.M ? p.nm[c] : 0;
        }

        int4_t ra[8], rb[8];
        // Every load is unconditional, from an address clamped into the tensor (the last row, the row's first piece), so that all 16
        // are in flight together; what lies outside the tensor is replaced when the stage is written.  F % 16 == 0: a 16-B piece is
        // wholly inside or outside the row.
        auto issue_loads = [&](int step) {
            const int64_t k0 = (int64_t)step * BK + kg * 16;
            const int64_t kc = k0 < p.F ? k0 : 0;
#pragma unroll
            for (int i = 0; i < 8; i++) ra[i] = *reinterpret_cast<const int4_t*>(p.m + (int64_t)min(c0 + lrow + 16 * i, p.M - 1) * p.F + kc);
#pragma unroll
            for (int i = 0; i < 8; i++) rb[i] = *reinterpret_cast<const int4_t*>(p.q + (int64_t)min(q0 + lrow + 16 * i, p.Q - 1) * p.F + kc);
        };
        auto write_stage = [&](int buf, int step) {     // re-centre; outside the tensor 0 AFTER the re-centring: it adds nothing to s
            unsigned char* sa = smem + buf * STAGE;
            unsigned char* sb = sa + OP_BYTES;
            const bool kok = (int64_t)step * BK + kg * 16 < p.F;
            const int4_t zero = {0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 8; i++)
                *reinterpret_cast<int4_t*>(sa + (kg * KGS + lrow + 16 * i) * 16) = (kok && c0 + lrow + 16 * i < p.M) ? (ra[i] ^ (int)0x80808080) : zero;
#pragma unroll
            for (int i = 0; i < 8; i++)
                *reinterpret_cast<int4_t*>(sb + (kg * KGS + lrow + 16 * i) * 16) = (kok && q0 + lrow + 16 * i < p.Q) ? (rb[i] ^ (int)0x80808080) : zero;
        };

        int4_t acc[4][4];
        int wide[WIDE ? 4 : 1][WIDE ? 4 : 1][WIDE ? 4 : 1];        // units of 65536: s = 65536 wide + acc
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                acc[i][j] = int4_t{0, 0, 0, 0};
                if (WIDE) {
#pragma unroll
                    for (int e = 0; e < 4; e++) wide[WIDE ? i : 0][WIDE ? j : 0][WIDE ? e : 0] = 0;
                }
            }

        issue_loads(0);
        write_stage(0, 0);
        __syncthreads();
        int since_flush = 0;
        for (int s = 0; s < nsteps; s++) {
            const int buf = s & 1;
            if (s + 1 < nsteps) issue_loads(s + 1);
            const unsigned char* sa = smem + buf * STAGE;
            const unsigned char* sb = sa + OP_BYTES;
#pragma unroll
            for (int ks = 0; ks < BK / 64; ks++) {
                int4_t fa[4], fb[4];
#pragma unroll
                for (int i = 0; i < 4; i++) fa[i] = *reinterpret_cast<const int4_t*>(sa + ((4 * ks + fg) * KGS + wc + 16 * i + fr) * 16);
#pragma unroll
                for (int j = 0; j < 4; j++) fb[j] = *reinterpret_cast<const int4_t*>(sb + ((4 * ks + fg) * KGS + wp + 16 * j + fr) * 16);
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
            }
            if (WIDE && ++since_flush == kFlushSteps) {       // uniform over the workgroup
                since_flush = 0;
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++)
#pragma unroll
                        for (int e = 0; e < 4; e++) {       // acc = 65536 (acc >> 16) + (acc & 0xffff) with the arithmetic shift
                            wide[WIDE ? i : 0][WIDE ? j : 0][WIDE ? e : 0] += acc[i][j][e] >> 16;
                            acc[i][j][e] &= 0xffff;
                        }
            }
            if (s + 1 < nsteps) write_stage(buf ^ 1, s + 1);
            __syncthreads();
        }

        // the lane holds stored rows c0 + wc + 16 i + 4 fg + e of queries q0 + wp + 16 j + fr
#pragma unroll
        for (int i = 0; i < 4; i++) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int col = wc + 16 * i + 4 * fg + e;
                const int row = c0 + col;
                const int64_t nmv = prm[par * BT + col];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    int64_t s = (int64_t)acc[i][j][e];
                    if (WIDE) s += (int64_t)wide[WIDE ? i : 0][WIDE ? j : 0][WIDE ? e : 0] << 16;
                    const int64_t d2 = nqv[j] + nmv - 2 * s;
                    keep_smallest<KL>(L[j], (row < p.M && row != excl[j]) ? KeyU8::make(d2, row) : KeyU8::none);
                }
            }
        }
    }

    // merge the lane groups and the two store waves that share a query; the staging area is free after the last barrier
    finish_run<KL, PARAM_OFF>(smem, L, q0, p.Q, p.runs, run, p.part, KeyFinish<KeyU8>{p.d2, p.index, p.k});
}

// int64 norms; a run leaves a list of KL keys per query
bool nn_plan(int Q, int M, int k, RunPlan& pl)
{
    return k >= 1 && k <= kMaxK && plan_runs(Q, M, 8, 8 * topk_list_len(k), pl);
}

int nn_norms(const uint8_t* x, int64_t* n, int rows, int64_t F, int as_q, hipStream_t s)
{
    const int Fc = (int)(F > INT32_MAX ? INT32_MAX : F);
    SbgProfScope prof(s, SBG_K_NN_U8, 4.0 * rows * (double)F, rows * (double)F + 8.0 * rows,
                      {kNnNorms, as_q ? rows : 0, as_q ? 0 : rows, Fc, 0, 0});
    SBG_LAUNCH(nn_norms_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, n, rows, F);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

template <int KL, bool WIDE>
int nn_launch_tiles(const NnArgs& a, const RunPlan& pl, hipStream_t s)
{
    if (!SBG_RAISE_LDS_ONCE((nn_tile_kernel<KL, WIDE>), LDS_BYTES))
        return sbg_fail(SBG_ERR_LAUNCH, "u8_nn_topk: cannot raise the dynamic LDS limit to %d bytes", LDS_BYTES);
    const int Fc = (int)(a.F > INT32_MAX ? INT32_MAX : a.F);
    SbgProfScope prof(s, SBG_K_NN_U8, 2.0 * a.Q * (double)a.M * (double)a.F, ((double)pl.rtiles * a.M + (double)a.Q * pl.runs) * (double)a.F,
                      {pl.runs == 1 ? kNnSingle : kNnSplit, a.Q, a.M, Fc, a.k, pl.runs});
    SBG_LAUNCH((nn_tile_kernel<KL, WIDE>), dim3((unsigned)(pl.rtiles * pl.runs)), dim3(256), LDS_BYTES, s, a);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

} // namespace

extern "C" int64_t sbg_u8_nn_workspace(int Q, int M, int k)
{
    RunPlan pl;
    if (!nn_plan(Q, M, k, pl)) return -1;
    return pl.bytes;
}

extern "C" int sbg_u8_nn_topk(const uint8_t* queries, const uint8_t* store, int Q, int M, int64_t F, int k, const int32_t* exclude, int64_t* d2,
                              int32_t* index, void* workspace, sbg_stream_t stream)
{
    const char* what = "u8_nn_topk";
    hipStream_t s = (hipStream_t)stream;
    SBG_CHECK(queries && store && d2 && index && workspace, "%s: null pointer", what);
    SBG_CHECK(k >= 1 && k <= kMaxK, "%s: k = %d neighbours, 1 to %d are supported", what, k, kMaxK);
    SBG_CHECK(Q >= 1 && M >= 1 && Q <= kMaxRows && M <= kMaxRows, "%s: bad sizes Q=%d M=%d (1 to 2^%d each)", what, Q, M, kIndexBits);
    SBG_CHECK(M - (exclude ? 1 : 0) >= k, "%s: the store has %d rows%s, %d neighbours need %d", what, M, exclude ? " and one may be excluded" : "", k,
              k + (exclude ? 1 : 0));
    SBG_CHECK(F >= 16 && F % 16 == 0 && F <= kMaxF, "%s: the row length %lld must be a multiple of 16 in [16, %lld]", what, (long long)F, (long long)kMaxF);
    SBG_CHECK(sbg_aligned16(queries) && sbg_aligned16(store) && sbg_aligned16(workspace), "%s: queries, store and workspace must be 16-byte aligned", what);
    RunPlan pl;
    SBG_CHECK(nn_plan(Q, M, k, pl), "%s: bad sizes", what);

    char* ws = (char*)workspace;
    NnArgs a;
    a.q = queries; a.m = store;
    a.nq = (const int64_t*)(ws + pl.nq_off); a.nm = (const int64_t*)(ws + pl.nm_off);
    a.exclude = exclude; a.d2 = d2; a.index = index; a.part = (int64_t*)(ws + pl.part_off);
    a.F = F; a.Q = Q; a.M = M; a.k = k; a.runs = pl.runs; a.ctiles = pl.ctiles; a.tiles_per_run = pl.tiles_per_run;
    int st = nn_norms(queries, (int64_t*)(ws + pl.nq_off), Q, F, 1, s);
    if (st != SBG_OK) return st;
    st = nn_norms(store, (int64_t*)(ws + pl.nm_off), M, F, 0, s);
    if (st != SBG_OK) return st;
    const int KL = topk_list_len(k);
    const bool wide = F > (int64_t)kFlushSteps * BK;
    st = with_list_len(KL, [&](auto kl) {
        return wide ? nn_launch_tiles<decltype(kl)::value, true>(a, pl, s) : nn_launch_tiles<decltype(kl)::value, false>(a, pl, s);
    });
    if (st != SBG_OK) return st;
    if (pl.runs > 1) {
        const int Fc = (int)(F > INT32_MAX ? INT32_MAX : F);
        SbgProfScope prof(s, SBG_K_NN_U8, 0.0, 8.0 * Q * (double)pl.runs * KL + 12.0 * Q * k, {kNnMerge, Q, M, Fc, k, pl.runs});
        return merge_runs(KL, a.part, Q, pl.runs, KeyFinish<KeyU8>{d2, index, k}, s);
    }
    return SBG_OK;
}
