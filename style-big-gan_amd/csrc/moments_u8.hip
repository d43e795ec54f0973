// moments_u8.hip -- device arithmetic of the variation tool (variation.py): running first and second moments of uint8
// images, the exact integer numerator of the per-pixel variance, and its rendering as heat maps.  torch_utils/ops/moments_u8.py states the same
// arithmetic for CPU tensors in numpy int64, so both devices give the same bits.  Integers only: no floating point, no atomics; integer sums do
// not depend on the order, so every result depends on the inputs alone.
//
// accumulate.  images uint8 [G, N, F] (image (g, n) starts at images + g * group_stride + n * row_stride, any base alignment: a slice of a larger
// batch) -> sum[g, f] += sum_n images[g, n, f], sumsq[g, f] += sum_n images[g, n, f]^2, both int64 [G, F] dense.
//   * A work-item owns W consecutive columns of one group and walks the rows of its split, four loads in flight.  W is the widest load every row
//     can share: 16 when row_stride and group_stride are multiples of 16, 4 when multiples of 4, else 1.  Column vectors are cut at the W-byte
//     boundaries of the ADDRESS (vector v holds the columns [v W - shift, v W - shift + W), shift = images mod W), so every whole vector is one
//     aligned load; the first and the last vector of a row may be partial and are read byte by byte, never outside [0, F).
//   * Its partial sums are uint32: a call takes at most kMaxN = 32768 rows, and 255^2 * 32768 = 2 130 739 200 < 2^32 (the bound is
//     255^2 N < 2^32, N <= 66051; 32768 leaves a factor of two).  The int64 running sums are touched once per call.
//   * THE SPLIT RULE.  tiles = ceil(F / 4096) (256 work-items of 16 bytes).  G * tiles workgroups do not fill the chip at low resolution, so N is
//     split:  want = min(ceil(1024 / (G * tiles)), ceil(N / 16)), at least 1;  rows = ceil(N / want);  splits = ceil(N / rows).
//     1024 = 256 CUs x 4 workgroups; 16 rows per split keep the partials (16 bytes a column) no larger than the bytes read for them.  With one
//     split the work-item adds into sum and sumsq itself (it is the only one that touches its columns).  Otherwise it stores int64 partials
//     [splits, G, 2, F] to the workspace and a second launch adds them in split order, one work-item per (g, f).
// numerator.  sum, sumsq int64 [G, C, P], n -> num int64 [G, P], num[g, p] = sum_c (n sumsq[g, c, p] - sum[g, c, p]^2): n (n - 1) times the
//   unbiased variance summed over channels, exact and never negative for moments of n bytes.  Every term is at most 65025 n^2, so the int64
//   arithmetic cannot overflow while n^2 * 65025 * C < 2^63; a larger n is refused.  One work-item per (g, p).
// render.  num int64 [G, P], thresholds int64 [255], table uint8 [256, 3] -> heat uint8 [G, 3, P] = table[level], level = the number of
//   thresholds <= num[g, p] (counted one by one: exact whatever their order), and dominant uint8 [P] = the g of the largest num[g, p], ties to
//   the lower g, 255 where every group is 0 (so G <= 255).  Thresholds and table are staged in LDS; one work-item per pixel.
// Launch-log key: kind SBG_K_MOMENTS, dims = {variant, ...}: 0 accumulate (G, N, F, splits, W) / 1 merge (G, N, F, splits) / 2 numerator (G, C, P) /
// 3 render (G, P); F and P clipped to INT32_MAX.
#include "sbg_common.h"

namespace {

constexpr int kAccumulate = 0, kMerge = 1, kNumerator = 2, kRender = 3;
constexpr int NT = 256;
constexpr int kTile = 4096;                             // columns of a nominal workgroup: 256 work-items of 16 bytes
constexpr int kTargetBlocks = 1024;                     // 256 CUs x 4
constexpr int kMinRows = 16;
constexpr int64_t kMaxN = 32768, kMaxF = (int64_t)1 << 26, kMaxG = 65535;
constexpr int64_t kMaxC = 1024, kMaxP = (int64_t)1 << 26, kMaxRenderG = 255;

template <int W> struct Bytes;
template <> struct Bytes<16> { typedef uint4 type; };
template <> struct Bytes<4> { typedef unsigned type; };
template <> struct Bytes<1> { typedef uint8_t type; };

static __device__ __forceinline__ unsigned byte_of(const uint4& v, int j)
{
    const unsigned w = j < 4 ? v.x : j < 8 ? v.y : j < 12 ? v.z : v.w;
    return (w >> (8 * (j & 3))) & 255u;
}
static __device__ __forceinline__ unsigned byte_of(unsigned v, int j) { return (v >> (8 * j)) & 255u; }
static __device__ __forceinline__ unsigned byte_of(uint8_t v, int) { return v; }

template <int W, class V>
static __device__ __forceinline__ void add_vector(const V& v, unsigned (&a)[W], unsigned (&q)[W])
{
#pragma unroll
    for (int j = 0; j < W; j++) {
        const unsigned x = byte_of(v, j);
        a[j] += x;
        q[j] += x * x;
    }
}

// grid (column blocks, splits, G).  shift = images mod W; rows = rows per split.  SPLIT: store partials [splits, G, 2, F], else add into sum / sumsq.
template <int W, bool SPLIT>
__global__ __launch_bounds__(NT) void moments_accumulate_kernel(const uint8_t* __restrict__ images, int64_t row_stride, int64_t group_stride,
                                                                int64_t* __restrict__ sum, int64_t* __restrict__ sumsq, int64_t* __restrict__ partial,
                                                                int N, int64_t F, int rows, int shift)
{
    typedef typename Bytes<W>::type V;
    const int64_t c0 = ((int64_t)blockIdx.x * NT + threadIdx.x) * W - shift;       // the first column of this vector; negative in the first one only
    if (c0 >= F) return;
    const int g = (int)blockIdx.z, G = (int)gridDim.z, s = (int)blockIdx.y;
    const int n0 = s * rows, n1 = n0 + rows < N ? n0 + rows : N;
    const int lo = c0 < 0 ? (int)-c0 : 0, hi = F - c0 < W ? (int)(F - c0) : W;     // the bytes [lo, hi) of the vector are columns of the row
    const uint8_t* p = images + (int64_t)g * group_stride + (int64_t)n0 * row_stride + c0;
    unsigned a[W], q[W];
#pragma unroll
    for (int j = 0; j < W; j++) a[j] = q[j] = 0;
    if (lo == 0 && hi == W) {
        int n = n0;
        for (; n + 4 <= n1; n += 4, p += 4 * row_stride) {
            const V v0 = *reinterpret_cast<const V*>(p), v1 = *reinterpret_cast<const V*>(p + row_stride);
            const V v2 = *reinterpret_cast<const V*>(p + 2 * row_stride), v3 = *reinterpret_cast<const V*>(p + 3 * row_stride);
            add_vector<W>(v0, a, q);
            add_vector<W>(v1, a, q);
            add_vector<W>(v2, a, q);
            add_vector<W>(v3, a, q);
        }
        for (; n < n1; n++, p += row_stride) add_vector<W>(*reinterpret_cast<const V*>(p), a, q);
    } else {
        for (int n = n0; n < n1; n++, p += row_stride) {
#pragma unroll
            for (int j = 0; j < W; j++)
                if (j >= lo && j < hi) {
                    const unsigned x = p[j];
                    a[j] += x;
                    q[j] += x * x;
                }
        }
    }
    if constexpr (SPLIT) {
        int64_t* dst = partial + ((int64_t)s * G + g) * 2 * F + c0;
#pragma unroll
        for (int j = 0; j < W; j++)
            if (j >= lo && j < hi) {
                dst[j] = (int64_t)a[j];
                dst[F + j] = (int64_t)q[j];
            }
    } else {
        const int64_t at = (int64_t)g * F + c0;
#pragma unroll
        for (int j = 0; j < W; j++)
            if (j >= lo && j < hi) {
                sum[at + j] += (int64_t)a[j];
                sumsq[at + j] += (int64_t)q[j];
            }
    }
}

// one work-item per (g, f): the partials of the splits 0, 1, ... in this order, then the running sums
__global__ __launch_bounds__(NT) void moments_merge_kernel(const int64_t* __restrict__ partial, int64_t* __restrict__ sum, int64_t* __restrict__ sumsq,
                                                           int64_t GF, int64_t F, int splits)
{
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < GF; i += (int64_t)gridDim.x * NT) {
        const int64_t g = i / F, f = i - g * F;
        const int64_t* p = partial + g * 2 * F + f;
        int64_t a = 0, q = 0;
        for (int s = 0; s < splits; s++, p += 2 * GF) {
            a += p[0];
            q += p[F];
        }
        sum[i] += a;
        sumsq[i] += q;
    }
}

// unsigned arithmetic: the same bits as numpy's wrapping int64 for moments that are not those of n bytes (the caller's error)
__global__ __launch_bounds__(NT) void moments_numerator_kernel(const int64_t* __restrict__ sum, const int64_t* __restrict__ sumsq, int64_t* __restrict__ num,
                                                               int64_t GP, int64_t P, int C, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < GP; i += (int64_t)gridDim.x * NT) {
        const int64_t g = i / P, p = i - g * P;
        const int64_t at = g * C * P + p;
        uint64_t acc = 0;
        for (int c = 0; c < C; c++) {
            const uint64_t s = (uint64_t)sum[at + (int64_t)c * P], q = (uint64_t)sumsq[at + (int64_t)c * P];
            acc += (uint64_t)n * q - s * s;
        }
        num[i] = (int64_t)acc;
    }
}

__global__ __launch_bounds__(NT) void moments_render_kernel(const int64_t* __restrict__ num, const int64_t* __restrict__ thresholds,
                                                            const uint8_t* __restrict__ table, uint8_t* __restrict__ heat, uint8_t* __restrict__ dominant,
                                                            int G, int64_t P)
{
    __shared__ long long thr[255];
    __shared__ uint8_t rgb[768];
    for (int i = threadIdx.x; i < 255; i += NT) thr[i] = thresholds[i];
    for (int i = threadIdx.x; i < 768; i += NT) rgb[i] = table[i];
    __syncthreads();
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < P; p += (int64_t)gridDim.x * NT) {
        long long best = 0;
        int who = 255;
        for (int g = 0; g < G; g++) {
            const long long v = num[(int64_t)g * P + p];
            int level = 0;
            for (int t = 0; t < 255; t++) level += thr[t] <= v ? 1 : 0;
            uint8_t* h = heat + (int64_t)g * 3 * P + p;
            h[0] = rgb[3 * level];
            h[P] = rgb[3 * level + 1];
            h[2 * P] = rgb[3 * level + 2];
            if (v > best) {
                best = v;
                who = g;
            }
        }
        dominant[p] = (uint8_t)who;
    }
}

int64_t accumulate_splits(int64_t G, int64_t N, int64_t F)
{
    if (G < 1 || G > kMaxG || N < 0 || N > kMaxN || F < 1 || F > kMaxF) return -1;
    if (N == 0) return 0;
    const int64_t tiles = (F + kTile - 1) / kTile;
    int64_t want = (kTargetBlocks + G * tiles - 1) / (G * tiles);
    const int64_t most = (N + kMinRows - 1) / kMinRows;
    if (want > most) want = most;
    if (want < 1) want = 1;
    const int64_t rows = (N + want - 1) / want;
    return (N + rows - 1) / rows;
}

template <int W>
int launch_accumulate(const uint8_t* images, int64_t row_stride, int64_t group_stride, int64_t* sum, int64_t* sumsq, int64_t* partial, int G, int N,
                      int64_t F, int splits, hipStream_t s)
{
    const int shift = (int)(reinterpret_cast<uintptr_t>(images) & (uintptr_t)(W - 1));
    const int64_t vectors = (shift + F + W - 1) / W;
    const int rows = (N + splits - 1) / splits;
    const dim3 grid((unsigned)((vectors + NT - 1) / NT), (unsigned)splits, (unsigned)G);
    if (splits > 1)
        SBG_LAUNCH((moments_accumulate_kernel<W, true>), grid, dim3(NT), 0, s, images, row_stride, group_stride, sum, sumsq, partial, N, F, rows, shift);
    else
        SBG_LAUNCH((moments_accumulate_kernel<W, false>), grid, dim3(NT), 0, s, images, row_stride, group_stride, sum, sumsq, partial, N, F, rows, shift);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

// the largest n with n^2 * 65025 * C < 2^63
bool numerator_fits(int64_t n, int64_t C)
{
    const unsigned __int128 v = (unsigned __int128)n * (unsigned __int128)n * 65025u * (unsigned __int128)C;
    return v < ((unsigned __int128)1 << 63);
}

} // namespace

extern "C" int64_t sbg_moments_accumulate_max_n(void) { return kMaxN; }

extern "C" int64_t sbg_moments_accumulate_splits(int64_t G, int64_t N, int64_t F) { return accumulate_splits(G, N, F); }

extern "C" int64_t sbg_moments_accumulate_workspace(int64_t G, int64_t N, int64_t F)
{
    const int64_t splits = accumulate_splits(G, N, F);
    return splits < 0 ? -1 : splits <= 1 ? 0 : 16 * splits * G * F;
}

extern "C" int sbg_moments_accumulate(const uint8_t* images, int64_t row_stride, int64_t group_stride, int64_t* sum, int64_t* sumsq, void* workspace,
                                      int64_t G, int64_t N, int64_t F, sbg_stream_t stream)
{
    const int64_t splits64 = accumulate_splits(G, N, F);
    SBG_CHECK(splits64 >= 0, "moments_accumulate: bad shape [%lld, %lld, %lld] (1 <= G <= 65535, 0 <= N <= 32768 per call, 1 <= F <= 2^26)",
              (long long)G, (long long)N, (long long)F);
    if (N == 0) return SBG_OK;
    SBG_CHECK(row_stride >= F && (G == 1 || group_stride >= (N - 1) * row_stride + F) && row_stride <= ((int64_t)1 << 40) &&
              group_stride <= ((int64_t)1 << 44), "moments_accumulate: images [%lld, %lld, %lld] with rows %lld and groups %lld bytes apart overlap "
              "(row_stride >= F, group_stride >= (N - 1) row_stride + F)", (long long)G, (long long)N, (long long)F, (long long)row_stride,
              (long long)group_stride);
    const int splits = (int)splits64;
    SBG_CHECK(images && sum && sumsq && sbg_aligned(sum, 8) && sbg_aligned(sumsq, 8) && (splits == 1 || (workspace && sbg_aligned(workspace, 8))),
              "moments_accumulate: null or misaligned pointer for [%lld, %lld, %lld]", (long long)G, (long long)N, (long long)F);
    hipStream_t s = (hipStream_t)stream;
    const int64_t strides = row_stride | (G == 1 ? 0 : group_stride);
    const int W = (strides & 15) == 0 ? 16 : (strides & 3) == 0 ? 4 : 1;
    {
        SbgProfScope prof(s, SBG_K_MOMENTS, 0.0, (double)G * N * F + (splits == 1 ? 32.0 : 16.0 * splits) * (double)G * F,
                          {kAccumulate, (int)G, (int)N, sbg_clip31(F), splits, W});
        const int status = W == 16 ? launch_accumulate<16>(images, row_stride, group_stride, sum, sumsq, (int64_t*)workspace, (int)G, (int)N, F, splits, s)
                         : W == 4  ? launch_accumulate<4>(images, row_stride, group_stride, sum, sumsq, (int64_t*)workspace, (int)G, (int)N, F, splits, s)
                                   : launch_accumulate<1>(images, row_stride, group_stride, sum, sumsq, (int64_t*)workspace, (int)G, (int)N, F, splits, s);
        if (status != SBG_OK) return status;
    }
    if (splits == 1) return SBG_OK;
    SbgProfScope prof(s, SBG_K_MOMENTS, 0.0, (16.0 * splits + 32.0) * (double)G * F, {kMerge, (int)G, (int)N, sbg_clip31(F), splits});
    SBG_LAUNCH(moments_merge_kernel, dim3(sbg_stream_grid(G * F, NT)), dim3(NT), 0, s, (const int64_t*)workspace, sum, sumsq, G * F, F, splits);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int64_t sbg_moments_numerator_max_n(int64_t C)
{
    if (C < 1 || C > kMaxC) return -1;
    int64_t lo = 0, hi = (int64_t)1 << 31;                  // numerator_fits(lo), !numerator_fits(hi)
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        (numerator_fits(mid, C) ? lo : hi) = mid;
    }
    return lo;
}

extern "C" int sbg_moments_numerator(const int64_t* sum, const int64_t* sumsq, int64_t* num, int64_t G, int64_t C, int64_t P, int64_t n, sbg_stream_t stream)
{
    SBG_CHECK(G >= 1 && G <= kMaxG && C >= 1 && C <= kMaxC && P >= 1 && P <= kMaxP && G * C * P <= ((int64_t)1 << 40),
              "moments_numerator: bad shape [%lld, %lld, %lld] (1 <= G <= 65535, 1 <= C <= 1024, 1 <= P <= 2^26, G C P <= 2^40)", (long long)G, (long long)C,
              (long long)P);
    SBG_CHECK(n >= 0 && n < ((int64_t)1 << 31) && numerator_fits(n, C), "moments_numerator: n = %lld is above %lld, the largest count with "
              "n^2 * 65025 * C < 2^63 at C = %lld, for [%lld, %lld, %lld]", (long long)n, (long long)sbg_moments_numerator_max_n(C), (long long)C,
              (long long)G, (long long)C, (long long)P);
    SBG_CHECK(sum && sumsq && num && sbg_aligned(sum, 8) && sbg_aligned(sumsq, 8) && sbg_aligned(num, 8),
              "moments_numerator: null or misaligned pointer for [%lld, %lld, %lld]", (long long)G, (long long)C, (long long)P);
    hipStream_t s = (hipStream_t)stream;
    SbgProfScope prof(s, SBG_K_MOMENTS, 0.0, 16.0 * (double)G * C * P + 8.0 * (double)G * P, {kNumerator, (int)G, (int)C, sbg_clip31(P)});
    SBG_LAUNCH(moments_numerator_kernel, dim3(sbg_stream_grid(G * P, NT)), dim3(NT), 0, s, sum, sumsq, num, G * P, P, (int)C, n);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int sbg_moments_render(const int64_t* num, const int64_t* thresholds, const uint8_t* table, uint8_t* heat, uint8_t* dominant, int64_t G, int64_t P,
                                  sbg_stream_t stream)
{
    SBG_CHECK(G >= 1 && G <= kMaxRenderG && P >= 1 && P <= kMaxP, "moments_render: bad shape [%lld, %lld] (1 <= G <= 255, 1 <= P <= 2^26)", (long long)G,
              (long long)P);
    SBG_CHECK(num && thresholds && table && heat && dominant && sbg_aligned(num, 8) && sbg_aligned(thresholds, 8),
              "moments_render: null or misaligned pointer for [%lld, %lld]", (long long)G, (long long)P);
    hipStream_t s = (hipStream_t)stream;
    SbgProfScope prof(s, SBG_K_MOMENTS, 0.0, 11.0 * (double)G * P + (double)P, {kRender, (int)G, sbg_clip31(P)});
    SBG_LAUNCH(moments_render_kernel, dim3(sbg_stream_grid(P, NT)), dim3(NT), 0, s, num, thresholds, table, heat, dominant, (int)G, P);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}
