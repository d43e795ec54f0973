// knn_select.h -- the one definition of selection, run split and run merge behind the k-NN search kernels (knn_manifold.hip: radius
// and fp16 top-k; nn_u8.hip).  Their tile kernels share a frame -- 256 lanes = 4 waves as 2 (columns) x 2 (queries), tile BT x BT, the
// columns on the accumulator's rows -- so a lane holds, for each of 4 queries, 16 candidates per tile.  Shared here is everything
// behind the candidate: the list a lane keeps per query, the candidates' keys, the merge of the 8 lane lists of a query at the end of a
// run, the split of the columns into runs, and the launch that merges the runs.  The K loops, the staging and the membership / probe
// reductions (an OR; a sum and a minimum) are not selections and stay with their kernels.
// THE ORDER AND TIE RULES ARE PART OF THE CONTRACT: the bit-for-bit tests and DESIGN.md sections 14, 18 and 19 rest on them.
//   keep_smallest:  a list holds the KL smallest values it was offered, ascending; equal values are kept as often as they occur.
//   keys:           (d2, row) packed so that one integer compare orders by d2, then row: a tie goes to the lower row.  Keys of distinct
//                   rows are distinct, so the k smallest do not depend on the order they arrive in.  A row that is absent or excluded
//                   gets the sentinel, which is larger than every key and never enters a list.
//   finish_run:     the 8 lane lists of a query are folded in slot order (column wave, lane group), one work-item per query.
//   plan_runs:      the split is a function of the shape alone, so the workspace query and the launch agree and a result does not
//                   depend on the device it ran on.
//   merge_runs:     one work-item per query walks the runs' lists in index order.  No atomics anywhere: two calls give the same bits.
#pragma once
#include "sbg_common.h"
#include <type_traits>

namespace knnsel {

constexpr int BT = 128;                     // tile side: columns (stored rows, manifold points) and queries
constexpr int kTargetGroups = 512;          // workgroups to aim for: 256 CUs x 2
constexpr int kIndexBits = 24;
constexpr int kMaxRows = 1 << kIndexBits;   // queries and columns of a search

// The lower / upper step of an insertion: v_min / v_max for the radius list's floats (and their NaN behaviour), compare and select for keys.
static __device__ __forceinline__ float lower_of(float a, float b) { return fminf(a, b); }
static __device__ __forceinline__ float upper_of(float a, float b) { return fmaxf(a, b); }
template <class T> static __device__ __forceinline__ T lower_of(T a, T b) { return a < b ? a : b; }
template <class T> static __device__ __forceinline__ T upper_of(T a, T b) { return a < b ? b : a; }

template <int KL, class T>
static __device__ __forceinline__ void keep_smallest(T (&L)[KL], T v)
{
    if (v < L[KL - 1]) {
#pragma unroll
        for (int t = 0; t < KL; t++) { const T lo = lower_of(L[t], v); v = upper_of(L[t], v); L[t] = lo; }
    }
}

// fp32 d2: (uint64(bits(d2)) << 32) | row, unsigned.  d2 must be +0 or positive: such floats order as their bits do.
struct KeyF32 {
    using type = uint64_t;
    using dist = float;
    static constexpr type none = ~(uint64_t)0;
    static __device__ __forceinline__ type make(float d2, int row) { return ((uint64_t)__float_as_uint(d2) << 32) | (uint32_t)row; }
    static __device__ __forceinline__ void store(type key, float* d2, int32_t* index)
    {
        *d2 = __uint_as_float((uint32_t)(key >> 32));
        *index = (int32_t)(uint32_t)key;
    }
};

// int64 d2 < 2^(63 - kIndexBits): d2 << kIndexBits | row, signed.
struct KeyU8 {
    using type = int64_t;
    using dist = int64_t;
    static constexpr type none = INT64_MAX;
    static __device__ __forceinline__ type make(int64_t d2, int row) { return (d2 << kIndexBits) | (int64_t)row; }
    static __device__ __forceinline__ void store(type key, int64_t* d2, int32_t* index)
    {
        *d2 = key >> kIndexBits;
        *index = (int32_t)(key & ((1 << kIndexBits) - 1));
    }
};

// What a top-k search writes for query q from its merged list: d2 and index of the first k keys, [Q, k] each.
template <class Key>
struct KeyFinish {
    using type = typename Key::type;
    static constexpr type none = Key::none;
    typename Key::dist* d2; int32_t* index; int k;
    template <int KL>
    __device__ __forceinline__ void operator()(int q, const type (&M)[KL]) const
    {
        typename Key::dist* const d = d2 + (int64_t)q * k;
        int32_t* const i = index + (int64_t)q * k;
#pragma unroll
        for (int t = 0; t < KL; t++)
            if (t < k) Key::store(M[t], d + t, i + t);
    }
};

// End of a run of a tile kernel; every work-item of the workgroup calls it once, after the last barrier of its K loops.  Lane list j
// belongs to query (wave & 1) * 64 + 16 j + (lane & 15) of the tile.  The lists go to an LDS image [BT queries][8 lists][KL] at `smem`
// (the staging area, STAGING bytes, free by then) with the odd stride 8 KL + 1, so the folding work-items hit distinct banks; behind
// one barrier work-item q < BT folds the 8 KL entries of its query and either finishes it (one run) or leaves the run's list in
// part[q][run][KL] for merge_runs.  Finish: `type`, `none` (the value an empty list is filled with) and operator()(q, M).
template <int KL, int STAGING, class Finish>
static __device__ __forceinline__ void finish_run(unsigned char* smem, const typename Finish::type (&L)[4][KL], int q0, int R, int runs, int run,
                                                  typename Finish::type* part, const Finish& finish)
{
    using T = typename Finish::type;
    constexpr int QS = 8 * KL + 1;
    static_assert(BT * QS * sizeof(T) <= STAGING, "the merge image must fit the staging area");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wp = (wave & 1) * 64, fr = lane & 15, fg = lane >> 4;
    T* ms = reinterpret_cast<T*>(smem);
    const int slot = (wave >> 1) * 4 + fg;
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int t = 0; t < KL; t++) ms[(wp + 16 * j + fr) * QS + slot * KL + t] = L[j][t];
    __syncthreads();
    const int q = q0 + tid;
    if (tid < BT && q < R) {
        T M[KL];
#pragma unroll
        for (int t = 0; t < KL; t++) M[t] = Finish::none;
        for (int s = 0; s < 8 * KL; s++) keep_smallest<KL>(M, ms[tid * QS + s]);
        if (runs == 1) {
            finish(q, M);
        } else {
            T* dst = part + ((int64_t)q * runs + run) * KL;
#pragma unroll
            for (int t = 0; t < KL; t++) dst[t] = M[t];
        }
    }
}

// Second stage of a split search: one work-item per query walks its runs' lists in index order.
template <int KL, class Finish>
__global__ __launch_bounds__(256) void merge_runs_kernel(const typename Finish::type* __restrict__ part, int R, int runs, Finish finish)
{
    using T = typename Finish::type;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= R) return;
    T M[KL];
#pragma unroll
    for (int t = 0; t < KL; t++) M[t] = Finish::none;
    const T* src = part + (int64_t)q * runs * KL;
    for (int s = 0; s < runs * KL; s++) keep_smallest<KL>(M, src[s]);
    finish(q, M);
}

// f(std::integral_constant<int, KL>) for the list length KL in {1, 4, 8}
template <class F>
int with_list_len(int KL, F&& f)
{
    return KL == 1 ? f(std::integral_constant<int, 1>{}) : KL == 4 ? f(std::integral_constant<int, 4>{}) : f(std::integral_constant<int, 8>{});
}

template <class Finish>
int merge_runs(int KL, const void* part, int R, int runs, const Finish& finish, hipStream_t s)
{
    return with_list_len(KL, [&](auto kl) -> int {
        SBG_LAUNCH((merge_runs_kernel<decltype(kl)::value, Finish>), dim3((unsigned)((R + 255) / 256)), dim3(256), 0, s,
                   (const typename Finish::type*)part, R, runs, finish);
        SBG_HIP_LAUNCH_CHECK();
        return SBG_OK;
    });
}

inline int topk_list_len(int k) { return k == 1 ? 1 : k <= 4 ? 4 : 8; }

inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// Workspace: [norms of the R queries][norms of the C columns][runs' partial results, only when runs > 1], each part 16-byte aligned.
struct RunPlan { int rtiles, ctiles, tiles_per_run, runs; int64_t nq_off, nm_off, part_off, bytes; };

// Runs per query tile: enough workgroups to fill the chip twice when the query tiles alone do not.  norm_bytes: one row's norm;
// part_bytes: what one run leaves for one query.
inline bool plan_runs(int R, int C, int64_t norm_bytes, int64_t part_bytes, RunPlan& pl)
{
    if (R < 1 || C < 1 || R > kMaxRows || C > kMaxRows) return false;
    pl.rtiles = (R + BT - 1) / BT;
    pl.ctiles = (C + BT - 1) / BT;
    int want = kTargetGroups / pl.rtiles;
    want = want < 1 ? 1 : (want > pl.ctiles ? pl.ctiles : want);
    pl.tiles_per_run = (pl.ctiles + want - 1) / want;
    pl.runs = (pl.ctiles + pl.tiles_per_run - 1) / pl.tiles_per_run;
    pl.nq_off = 0;
    pl.nm_off = up16(norm_bytes * R);
    pl.part_off = pl.nm_off + up16(norm_bytes * C);
    pl.bytes = pl.part_off + (pl.runs > 1 ? part_bytes * R * pl.runs : 0);
    return true;
}

} // namespace knnsel
