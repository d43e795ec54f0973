// walk.hip -- device arithmetic of the latent walk tool (interpolate.py): the table of blended latents of a walk through
// key latents, and the exact squared difference of consecutive uint8 frames.  torch_utils/ops/walk.py states the same arithmetic for CPU
// tensors, so both devices give the same bits.
//
// blend.  keys fp32 [K, L, D], index int32 [T, 4], weight fp32 [T, 4] -> out fp32 [T, L, D].  THE CHAIN IS THE CONTRACT: on a layer whose
// layer_mask entry is nonzero (layer_mask == NULL: every layer)
//     acc = weight[t, 0] * keys[index[t, 0], l, d]                      one rounded fp32 product
//     acc = fmaf(weight[t, j], keys[index[t, j], l, d], acc)            j = 1, 2, 3, in this order
// and on the other layers out[t, l, d] = keys[hold[t], l, d], a copy (the bits, -0.0 included).  The file is compiled with contraction off and
// the three fused steps are explicit fmaf calls, so the compiler neither fuses the first product into the chain nor splits a step.  One
// streaming launch, one output element per work-item and grid stride.  The caller checks every index and hold value against [0, K) before the
// launch (the op reads them back); an element whose index lies outside is skipped all the same, so nothing is read out of bounds for it.
//
// sqdiff.  a, b uint8 [N, F] (rows F bytes apart, any base alignment) -> out int64 [N], out[n] = sum_f (a[n, f] - b[n, f])^2, exact.  A row is
// cut into chunks of kChunk = 16384 bytes, one workgroup of 256 per (chunk, row); the rows are walked with a grid stride.  b - a is the same
// for every row, so the widest load both streams can share is fixed per call: 16 bytes when (b - a) % 16 == 0, 4 when % 4 == 0, else 1.  A
// work-item sums into an int32: it sees at most kChunk / 256 + 32 = 96 elements of at most 255^2 = 65025 each (the bound is 2^15 elements:
// 65025 * 2^15 < 2^31), the lanes and waves are added in int64.  With one chunk per row the workgroup stores out[n] itself; otherwise it stores
// partial[n * splits + chunk] and a second launch adds the partials of a row, one wave per row.  No atomics; integer sums do not depend on the
// order, so the result depends on the inputs alone.
// Launch-log key: kind SBG_K_WALK, dims = {variant, ...}: 0 blend (T, L, D, layers given) / 1 sqdiff (N, F, splits) / 2 merge (N, F, splits);
// N and F clipped to INT32_MAX.
#pragma clang fp contract(off)
#include "sbg_common.h"

namespace {

constexpr int kBlend = 0, kSqdiff = 1, kMerge = 2;
constexpr int NT = 256;
constexpr int kMaxD = 1024;
constexpr int kChunk = 16384;                           // bytes of a row per workgroup
constexpr int64_t kMaxN = (int64_t)1 << 24, kMaxF = (int64_t)1 << 26;

__global__ __launch_bounds__(NT) void walk_blend_kernel(const float* __restrict__ keys, const int32_t* __restrict__ index, const float* __restrict__ weight,
                                                        const int32_t* __restrict__ layer_mask, const int32_t* __restrict__ hold, float* __restrict__ out,
                                                        int total, int K, int L, int D)
{
    const int LD = L * D;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
        const int t = (int)(i / LD), ld = (int)(i - (int64_t)t * LD);
        if (layer_mask && !layer_mask[ld / D]) {
            const unsigned h = (unsigned)hold[t];
            if (h < (unsigned)K) out[i] = keys[(int64_t)h * LD + ld];
            continue;
        }
        const unsigned i0 = (unsigned)index[4 * t], i1 = (unsigned)index[4 * t + 1], i2 = (unsigned)index[4 * t + 2], i3 = (unsigned)index[4 * t + 3];
        if (i0 >= (unsigned)K || i1 >= (unsigned)K || i2 >= (unsigned)K || i3 >= (unsigned)K) continue;
        float acc = weight[4 * t] * keys[(int64_t)i0 * LD + ld];
        acc = fmaf(weight[4 * t + 1], keys[(int64_t)i1 * LD + ld], acc);
        acc = fmaf(weight[4 * t + 2], keys[(int64_t)i2 * LD + ld], acc);
        acc = fmaf(weight[4 * t + 3], keys[(int64_t)i3 * LD + ld], acc);
        out[i] = acc;
    }
}

static __device__ __forceinline__ int sq(int x, int y) { const int d = x - y; return d * d; }

static __device__ __forceinline__ int sq4(unsigned x, unsigned y)
{
    return sq((int)(x & 255u), (int)(y & 255u)) + sq((int)((x >> 8) & 255u), (int)((y >> 8) & 255u)) +
           sq((int)((x >> 16) & 255u), (int)((y >> 16) & 255u)) + sq((int)(x >> 24), (int)(y >> 24));
}

static __device__ __forceinline__ long long wave_sum_i64(long long v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// W: bytes per load of the body, 16 / 4 / 1; the host picks it so that (b - a) % W == 0.  grid (splits, rows walked with a stride of gridDim.y)
template <int W>
__global__ __launch_bounds__(NT) void walk_sqdiff_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int64_t* __restrict__ out, int64_t N,
                                                         int64_t F, int splits)
{
    __shared__ long long red[NT / 64];
    const int tid = threadIdx.x, s = (int)blockIdx.x;
    const int64_t lo = (int64_t)s * kChunk;
    const int len = (int)(F - lo < kChunk ? F - lo : kChunk);
    for (int64_t n = blockIdx.y; n < N; n += gridDim.y) {
        const uint8_t* pa = a + n * F + lo;
        const uint8_t* pb = b + n * F + lo;
        // the bytes before pa's next W-byte boundary (pb reaches its own there too), whole loads, the bytes left: each at most one per work-item
        int head = W == 1 ? 0 : (int)((W - (reinterpret_cast<uintptr_t>(pa) & (W - 1))) & (W - 1));
        if (head > len) head = len;
        const int body = W == 1 ? 0 : (len - head) / W;
        const int tail0 = head + body * W;
        int acc = 0;                                    // at most 1 + (kChunk / W / NT + 1) * W + 1 <= 96 elements (W > 1), kChunk / NT = 64 (W = 1)
        if (tid < head) acc += sq(pa[tid], pb[tid]);
        if constexpr (W == 16) {
            const uint4* va = reinterpret_cast<const uint4*>(pa + head);
            const uint4* vb = reinterpret_cast<const uint4*>(pb + head);
            for (int v = tid; v < body; v += NT) {
                const uint4 x = va[v], y = vb[v];
                acc += sq4(x.x, y.x) + sq4(x.y, y.y) + sq4(x.z, y.z) + sq4(x.w, y.w);
            }
        } else if constexpr (W == 4) {
            const unsigned* va = reinterpret_cast<const unsigned*>(pa + head);
            const unsigned* vb = reinterpret_cast<const unsigned*>(pb + head);
            for (int v = tid; v < body; v += NT) acc += sq4(va[v], vb[v]);
        }
        for (int i = tail0 + tid; i < len; i += NT) acc += sq(pa[i], pb[i]);
        const long long w = wave_sum_i64((long long)acc);
        __syncthreads();                                // the previous row's reads of red are over
        if ((tid & 63) == 0) red[tid >> 6] = w;
        __syncthreads();
        if (tid == 0) out[n * splits + s] = (int64_t)(red[0] + red[1] + red[2] + red[3]);
    }
}

// one wave per row: lane t adds the partials t, t + 64, ...
__global__ __launch_bounds__(NT) void walk_sqdiff_merge_kernel(const int64_t* __restrict__ partial, int64_t* __restrict__ out, int64_t N, int splits)
{
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    long long s = 0;
    if (n < N)
        for (int i = lane; i < splits; i += 64) s += partial[n * splits + i];
    s = wave_sum_i64(s);
    if (n < N && lane == 0) out[n] = (int64_t)s;
}

int64_t sqdiff_splits(int64_t N, int64_t F)
{
    if (N < 1 || N > kMaxN || F < 1 || F > kMaxF) return -1;
    return (F + kChunk - 1) / kChunk;
}

template <int W>
int launch_sqdiff(const uint8_t* a, const uint8_t* b, int64_t* dst, int64_t N, int64_t F, int splits, hipStream_t s)
{
    SBG_LAUNCH(walk_sqdiff_kernel<W>, dim3((unsigned)splits, (unsigned)(N < 65535 ? N : 65535)), dim3(NT), 0, s, a, b, dst, N, F, splits);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

} // namespace

extern "C" int sbg_walk_blend(const float* keys, const int32_t* index, const float* weight, const int32_t* layer_mask, const int32_t* hold, float* out,
                              int K, int T, int L, int D, sbg_stream_t stream)
{
    SBG_CHECK(K >= 1 && T >= 0 && L >= 1 && D >= 1 && D <= kMaxD, "walk_blend: bad sizes K=%d T=%d L=%d D=%d (K >= 1, L >= 1, 1 <= D <= %d)", K, T, L, D, kMaxD);
    if (T == 0) return SBG_OK;
    SBG_CHECK((int64_t)T * L * D <= INT32_MAX && (int64_t)K * L * D <= ((int64_t)1 << 40), "walk_blend: a table of %d x %d x %d from %d keys is too large "
              "(T L D < 2^31)", T, L, D, K);
    SBG_CHECK(keys && index && weight && out && (!layer_mask || hold) && sbg_aligned(keys, 4) && sbg_aligned(index, 4) && sbg_aligned(weight, 4) &&
              sbg_aligned(out, 4) && sbg_aligned(layer_mask, 4) && sbg_aligned(hold, 4), "walk_blend: null or misaligned pointer (a layer mask needs hold)");
    const int total = T * L * D;
    hipStream_t s = (hipStream_t)stream;
    SbgProfScope prof(s, SBG_K_WALK, 7.0 * (double)total, 8.0 * (double)total + 4.0 * (double)K * L * D, {kBlend, T, L, D, layer_mask ? 1 : 0});
    SBG_LAUNCH(walk_blend_kernel, dim3(sbg_stream_grid(total, NT)), dim3(NT), 0, s, keys, index, weight, layer_mask, hold, out, total, K, L, D);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int64_t sbg_walk_sqdiff_splits(int64_t N, int64_t F) { return sqdiff_splits(N, F); }

extern "C" int64_t sbg_walk_sqdiff_workspace(int64_t N, int64_t F)
{
    const int64_t splits = sqdiff_splits(N, F);
    return splits < 0 ? -1 : splits == 1 ? 0 : 8 * N * splits;
}

extern "C" int sbg_walk_sqdiff(const uint8_t* a, const uint8_t* b, int64_t* out, void* workspace, int64_t N, int64_t F, sbg_stream_t stream)
{
    const int64_t splits64 = sqdiff_splits(N, F);
    SBG_CHECK(splits64 >= 1, "walk_sqdiff: bad shape [%lld, %lld] (1 <= N <= 2^24, 1 <= F <= 2^26)", (long long)N, (long long)F);
    const int splits = (int)splits64;
    SBG_CHECK(a && b && out && sbg_aligned(out, 8) && (splits == 1 || (workspace && sbg_aligned(workspace, 8))), "walk_sqdiff: null or misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    int64_t* dst = splits == 1 ? out : (int64_t*)workspace;
    const uintptr_t delta = reinterpret_cast<uintptr_t>(a) - reinterpret_cast<uintptr_t>(b);
    {
        SbgProfScope prof(s, SBG_K_WALK, 3.0 * (double)N * (double)F, 2.0 * (double)N * (double)F + 8.0 * (double)N * splits,
                          {kSqdiff, sbg_clip31(N), sbg_clip31(F), splits});
        const int status = (delta & 15) == 0 ? launch_sqdiff<16>(a, b, dst, N, F, splits, s)
                         : (delta & 3) == 0  ? launch_sqdiff<4>(a, b, dst, N, F, splits, s)
                                             : launch_sqdiff<1>(a, b, dst, N, F, splits, s);
        if (status != SBG_OK) return status;
    }
    if (splits == 1) return SBG_OK;
    SbgProfScope prof(s, SBG_K_WALK, 0.0, 8.0 * (double)N * splits + 8.0 * (double)N, {kMerge, sbg_clip31(N), sbg_clip31(F), splits});
    SBG_LAUNCH(walk_sqdiff_merge_kernel, dim3((unsigned)((N + NT / 64 - 1) / (NT / 64))), dim3(NT), 0, s, (const int64_t*)workspace, out, N, splits);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}
