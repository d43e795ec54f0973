// kmeans_u8.hip -- the centroid update of the mode coverage tool (modes.py; NDB: Richardson & Weiss, "On GANs and GMMs", NeurIPS 2018; DESIGN.md
// section 26): for points uint8 [N, F], labels int32 [N] and K byte centroids,
//   counts[k]       = the number of rows n with labels[n] == k,
//   sums[k, f]      = the int64 sum of points[n, f] over those rows,
//   centroids[k, f] = (2 sums[k, f] + counts[k]) / (2 counts[k]) in integer division, the mean rounded half up;
// an empty cluster keeps old_centroids[k] and has a sums row of 0.  Everything is integer arithmetic: the result depends on the inputs alone, not
// on the launch plan below, and torch_utils/ops/kmeans_u8.py states the same definition in torch for CPU tensors.  A label outside [0, K) is the
// caller's error (the op layer refuses it); the kernel skips such a row.
//
// accumulate.  A streaming pass that reads `points` once in 16-byte loads.  A lane owns 16 consecutive columns; LPR lanes side by side own a column
// tile of 16 LPR columns of one row, so a workgroup of 256 holds 256 / LPR rows at a time; a lane has 8 such loads in flight and fetches the next 8
// rows before it adds the current 8 (the LDS adds of a batch take longer than its loads: without the prefetch the pass ran 10 % longer).  The partial sums are
// [K][column tile] i32 in LDS: LPR is the largest power of two with K LPR <= 1024 (and no wider than the table), 4 for K = 256 up to 64 for
// K <= 16.  The label is uniform per row; every byte is one LDS integer add (`ds_add_u32`, nothing returned; integer adds commute, so the order in
// which the rows of a workgroup meet is immaterial).  In LDS, column c of the tile sits at (c & 15) LPR + (c >> 4), so the lanes of a row hit
// consecutive banks, and a cluster's row is 17 LPR dwords long, so rows of different clusters start LPR banks apart.  Rows whose labels are equal
// and that sit in one wave serialise on the address: labels sorted by cluster are the slow case (and a data set in random order the common one).
// The rows are split over gridDim.y chunks so that tiles x chunks reaches kTargetGroups workgroups (two per CU, what the LDS allows), never
// below kMinChunkRows rows per chunk; a chunk never exceeds kMaxChunkRows = 2^23 rows, so a partial stays below 2^31.  Every workgroup stores its
// partial as i32 [chunk][K][F] into the workspace with plain stores; the workgroups of column tile 0 count the labels as well ([chunk][K]).
// finish.  A second launch: a work-item owns 4 columns of one cluster, adds the chunks' partials and counts in ascending order in int64, stores
// `sums` and `counts`, and divides.  No floating point and no global atomics anywhere.  merge.h is not used: it sums a value-major [values][count]
// layout that this kernel could only write with strided stores, and the division here is per element.
// Launch-log key: kind SBG_K_KMEANS_U8, dims = {variant, N clipped, F clipped, K, chunks, LPR}: 0 accumulate / 1 finish.
#include "sbg_common.h"

namespace {

constexpr int kAccumulate = 0, kFinish = 1;
constexpr int NT = 256;
constexpr int kMaxK = 256;
constexpr int64_t kMaxN = (int64_t)1 << 24;
constexpr int64_t kMaxF = (int64_t)3 << 20;
constexpr int kVec = 16;                                // columns per lane: one 16-byte load
constexpr int kSlots = 1024;                            // K * LPR at most: 17 / 16 * 64 KiB of partial sums
constexpr int kMaxLpr = 64;
constexpr int kUnroll = 8;                              // rows per lane in flight
constexpr int kTargetGroups = 512;                      // workgroups wanted: 256 CUs x the 2 that fit a CU's LDS
constexpr int kMinChunkRows = 256;
constexpr int kMaxChunkRows = 1 << 23;
static_assert((int64_t)255 * kMaxChunkRows < ((int64_t)1 << 31), "an i32 partial holds at most 2^23 rows of bytes");
static_assert(kMaxN / kMaxChunkRows <= 65535, "the chunks are a grid dimension");

struct Plan {
    int lpr;                                            // lanes per row
    int tiles;                                          // column tiles of 16 * lpr columns
    int chunks, chunk_rows;
    int lds;                                            // bytes
};

bool sizes_ok(int64_t N, int64_t F, int K) { return N >= 1 && N <= kMaxN && K >= 1 && K <= kMaxK && F >= kVec && F <= kMaxF && F % kVec == 0; }

Plan make_plan(int64_t N, int64_t F, int K)
{
    Plan p;
    p.lpr = kMaxLpr;
    while (p.lpr > 1 && ((int64_t)K * p.lpr > kSlots || (int64_t)kVec * (p.lpr / 2) >= F)) p.lpr /= 2;
    const int tile = kVec * p.lpr;
    p.tiles = (int)((F + tile - 1) / tile);
    int64_t chunks = (kTargetGroups + p.tiles - 1) / p.tiles;
    const int64_t most = (N + kMinChunkRows - 1) / kMinChunkRows, least = (N + kMaxChunkRows - 1) / kMaxChunkRows;
    if (chunks > most) chunks = most;
    if (chunks < least) chunks = least;
    p.chunk_rows = (int)((N + chunks - 1) / chunks);
    p.chunks = (int)((N + p.chunk_rows - 1) / p.chunk_rows);
    p.lds = 4 * (K * (kVec + 1) * p.lpr + K);
    return p;
}

// grid (tiles, chunks).  LDS: acc[K][17 LPR] then cnt[K].
template <int LPR>
__global__ __launch_bounds__(NT) void kmeans_u8_accumulate_kernel(const uint8_t* __restrict__ points, const int32_t* __restrict__ labels,
                                                                  int32_t* __restrict__ partial, int32_t* __restrict__ cpartial, int64_t N, int64_t F, int K,
                                                                  int chunk_rows)
{
    extern __shared__ int32_t lds[];
    constexpr int STRIDE = (kVec + 1) * LPR, ROWS = NT / LPR, TILE = kVec * LPR;
    int32_t* acc = lds;
    int32_t* cnt = lds + K * STRIDE;
    const int tid = threadIdx.x;
    for (int i = tid; i < K * STRIDE + K; i += NT) lds[i] = 0;
    __syncthreads();

    const int lir = tid % LPR, slot = tid / LPR;
    const int chunk = (int)blockIdx.y;
    const int64_t col0 = (int64_t)blockIdx.x * TILE;
    const int64_t col = col0 + kVec * lir;
    const bool live = col < F;                          // F is a multiple of 16: a lane's columns are all inside or all outside
    const bool counting = blockIdx.x == 0 && lir == 0;
    const int64_t r0 = (int64_t)chunk * chunk_rows;
    const int64_t r1 = r0 + chunk_rows < N ? r0 + chunk_rows : N;
    if (live) {                                         // a lane past the table's last column has nothing to add (and never counts)
        const int64_t step = (int64_t)ROWS * kUnroll;
        auto fetch = [&](int64_t r, int4_t (&v)[kUnroll], int (&lab)[kUnroll]) {
#pragma unroll
            for (int u = 0; u < kUnroll; u++) {
                const int64_t rr = r + (int64_t)u * ROWS;
                const bool in = rr < r1;
                lab[u] = in ? labels[rr] : -1;
                v[u] = int4_t{0, 0, 0, 0};
                if (in) v[u] = *reinterpret_cast<const int4_t*>(points + rr * F + col);
            }
        };
        int4_t v[kUnroll], ahead[kUnroll];
        int lab[kUnroll], lab_ahead[kUnroll];
        int64_t r = r0 + slot;
        fetch(r, v, lab);
        for (; r < r1; r += step) {
            fetch(r + step, ahead, lab_ahead);          // the next rows are in flight while this batch goes into LDS
#pragma unroll
            for (int u = 0; u < kUnroll; u++) {
                if ((unsigned)lab[u] < (unsigned)K) {   // not past the chunk, and not a label outside [0, K): that row is skipped
                    int32_t* row = acc + lab[u] * STRIDE + lir;
#pragma unroll
                    for (int j = 0; j < kVec; j++)
                        __hip_atomic_fetch_add(row + j * LPR, (int32_t)(((unsigned)v[u][j >> 2] >> (8 * (j & 3))) & 0xffu), __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (counting) __hip_atomic_fetch_add(cnt + lab[u], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                v[u] = ahead[u];
                lab[u] = lab_ahead[u];
            }
        }
    }
    __syncthreads();

    for (int i = tid; i < K * (TILE / 4); i += NT) {
        const int k = i / (TILE / 4), c = (i % (TILE / 4)) * 4;
        if (col0 + c >= F) continue;                    // F is a multiple of 4: the four columns are all inside or all outside
        const int32_t* row = acc + k * STRIDE + (c >> 4);
        const int4_t out = {row[((c & 15) + 0) * LPR], row[((c & 15) + 1) * LPR], row[((c & 15) + 2) * LPR], row[((c & 15) + 3) * LPR]};
        *reinterpret_cast<int4_t*>(partial + ((int64_t)chunk * K + k) * F + col0 + c) = out;
    }
    if (blockIdx.x == 0)
        for (int k = tid; k < K; k += NT) cpartial[(int64_t)chunk * K + k] = cnt[k];
}

// a work-item owns 4 columns of one cluster
__global__ __launch_bounds__(NT) void kmeans_u8_finish_kernel(const int32_t* __restrict__ partial, const int32_t* __restrict__ cpartial,
                                                              const uint8_t* __restrict__ old_centroids, uint8_t* __restrict__ centroids,
                                                              int64_t* __restrict__ sums, int64_t* __restrict__ counts, int64_t F, int K, int chunks)
{
    const int64_t quads = F / 4, total = quads * K;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
        const int k = (int)(i / quads);
        const int64_t c = (i % quads) * 4, at = (int64_t)k * F + c;
        int64_t n = 0, s[4] = {0, 0, 0, 0};
        for (int q = 0; q < chunks; q++) {
            n += cpartial[(int64_t)q * K + k];
            const int4_t p = *reinterpret_cast<const int4_t*>(partial + ((int64_t)q * K + k) * F + c);
#pragma unroll
            for (int t = 0; t < 4; t++) s[t] += p[t];
        }
        unsigned packed = 0;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            sums[at + t] = s[t];
            const unsigned byte = n > 0 ? (unsigned)((2 * s[t] + n) / (2 * n)) : (unsigned)old_centroids[at + t];
            packed |= byte << (8 * t);
        }
        *reinterpret_cast<unsigned*>(centroids + at) = packed;
        if (c == 0) counts[k] = n;
    }
}

template <int LPR>
int launch_accumulate(const Plan& p, const uint8_t* points, const int32_t* labels, int32_t* partial, int32_t* cpartial, int64_t N, int64_t F, int K,
                      hipStream_t s)
{
    if (p.lds > 64 * 1024 && !SBG_RAISE_LDS_ONCE(kmeans_u8_accumulate_kernel<LPR>, 4 * (kSlots / LPR * (kVec + 1) * LPR + kMaxK)))
        return sbg_fail(SBG_ERR_LAUNCH, "kmeans_u8_update: cannot raise the dynamic LDS limit to %d bytes", p.lds);
    SbgProfScope prof(s, SBG_K_KMEANS_U8, 0.0, (double)N * F + 4.0 * N + 4.0 * p.chunks * K * ((double)F + 1),
                      {kAccumulate, sbg_clip31(N), sbg_clip31(F), K, p.chunks, p.lpr});
    SBG_LAUNCH(kmeans_u8_accumulate_kernel<LPR>, dim3((unsigned)p.tiles, (unsigned)p.chunks), dim3(NT), p.lds, s, points, labels, partial, cpartial, N, F, K,
               p.chunk_rows);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

} // namespace

extern "C" int64_t sbg_kmeans_u8_update_workspace(int64_t N, int64_t F, int K)
{
    if (!sizes_ok(N, F, K)) return -1;
    const Plan p = make_plan(N, F, K);
    return 4 * (int64_t)p.chunks * K * (F + 1);         // i32 [chunks][K][F] and behind it i32 [chunks][K]
}

extern "C" int sbg_kmeans_u8_update(const uint8_t* points, const int32_t* labels, const uint8_t* old_centroids, uint8_t* centroids, int64_t* sums,
                                    int64_t* counts, void* workspace, int64_t N, int64_t F, int K, sbg_stream_t stream)
{
    SBG_CHECK(sizes_ok(N, F, K), "kmeans_u8_update: bad sizes N=%lld F=%lld K=%d (1 <= N <= %lld, 1 <= K <= %d, F a multiple of %d, at most %lld)",
              (long long)N, (long long)F, K, (long long)kMaxN, kMaxK, kVec, (long long)kMaxF);
    SBG_CHECK(points && labels && old_centroids && centroids && sums && counts && workspace && sbg_aligned(points, 16) && sbg_aligned(labels, 4) &&
              sbg_aligned(old_centroids, 16) && sbg_aligned(centroids, 16) && sbg_aligned(sums, 16) && sbg_aligned(counts, 8) && sbg_aligned(workspace, 16),
              "kmeans_u8_update: null or misaligned pointer (N=%lld F=%lld K=%d)", (long long)N, (long long)F, K);
    const Plan p = make_plan(N, F, K);
    int32_t* partial = (int32_t*)workspace;
    int32_t* cpartial = partial + (int64_t)p.chunks * K * F;
    hipStream_t s = (hipStream_t)stream;
    int status = SBG_ERR_INVALID;
    switch (p.lpr) {
    case 1:  status = launch_accumulate<1>(p, points, labels, partial, cpartial, N, F, K, s); break;
    case 2:  status = launch_accumulate<2>(p, points, labels, partial, cpartial, N, F, K, s); break;
    case 4:  status = launch_accumulate<4>(p, points, labels, partial, cpartial, N, F, K, s); break;
    case 8:  status = launch_accumulate<8>(p, points, labels, partial, cpartial, N, F, K, s); break;
    case 16: status = launch_accumulate<16>(p, points, labels, partial, cpartial, N, F, K, s); break;
    case 32: status = launch_accumulate<32>(p, points, labels, partial, cpartial, N, F, K, s); break;
    case 64: status = launch_accumulate<64>(p, points, labels, partial, cpartial, N, F, K, s); break;
    }
    if (status != SBG_OK) return status;
    SbgProfScope prof(s, SBG_K_KMEANS_U8, 0.0, 4.0 * p.chunks * K * ((double)F + 1) + 10.0 * K * (double)F, {kFinish, sbg_clip31(N), sbg_clip31(F), K, p.chunks, p.lpr});
    SBG_LAUNCH(kmeans_u8_finish_kernel, dim3(sbg_stream_grid((int64_t)K * (F / 4), NT)), dim3(NT), 0, s, partial, cpartial, old_centroids, centroids, sums, counts,
               F, K, p.chunks);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}
