// diffaug.hip -- DiffAugment (Zhao et al., NeurIPS 2020: colour, translation, cutout) in front of the discriminator, as one per-sample
// sum plus one streaming pass, and its adjoint of the same shape.  fp32, dense NCHW, C = 1..4.
// Per sample the published chain (brightness, saturation, contrast, zero-padded integer shift, cutout) is affine in the image.  With
// the sample's parameters (b, s, k, t_row, t_col, r0, r1, c0, c1) and M = mean(x) + b, output pixel (i, j) is `live` when it lies
// outside the rectangle [r0, r1) x [c0, c1) and its source (p, q) = (i + t_row, j + t_col) lies inside the image; then
//   v = x[:, p, q] + b;   v <- s v + (1 - s) mean_c(v);   y[:, i, j] = k v + (1 - k) M,        every other output pixel is 0.
// Adjoint (g = dL/dy -> dL/dx): u[:, p, q] = g[:, p - t_row, q - t_col] where that output pixel is live, else 0;  S = sum(u) / (C H W);
//   w = k u + (1 - k) S;   dx = s w + (1 - s) mean_c(w).      The shift is injective: a gather, no atomics.
// The adjoint of the adjoint is the forward form with b = 0 (`drop_b`), so two entry points serve every order of derivative.
//
// Sums.  A sample is cut into chunks of 4096 consecutive elements.  In a chunk, lane t of the 256 owns the four 4-element groups
// 4 (256 u + t) .. + 3, u = 0..3, and adds their elements in ascending order; block_sum (reduce.h) adds the lanes.  The chunk sums of a
// sample are added by lane r % 256 in ascending r, then block_sum: an order fixed by C H W alone, the same in every kernel below and
// for every alignment, so a sample's bits do not depend on N, on its place in the batch or on the run.  No atomics.
//
// Kernels.  C H W <= 4096 (3 x 32 x 32 is 12 KB): ONE launch, one workgroup per sample; the sample is staged in LDS (16 KB) by the
// loads that feed the sum, the shifted gather reads LDS, one read and one write of HBM.  Larger samples: a sum launch (one workgroup
// per chunk, one float each into the workspace) and an apply launch (every workgroup adds its sample's chunk sums again, then one
// work-item per 4 consecutive pixels of a row, all channels).  W % 4 == 0 with 16-byte aligned tensors: 16-byte loads in the sum, 16-byte
// stores in the apply; the column shift misaligns the source of the apply, which is read as predicated dwords.  Any other W or
// alignment: the same ownership with dword accesses (one pixel per work-item in the apply).
// Safety: the shifts are clamped to [-H, H] / [-W, W] and the rectangle to the image on load, every source index is predicated.
// Launch-log key: kind SBG_K_DIFFAUG, dims = {variant, N, C, H, W, 1 16-byte / 2 dword accesses}.
#include "sbg_common.h"
#include "reduce.h"

namespace {

constexpr int kSum = 0, kApply = 1, kAdjSum = 2, kAdjApply = 3, kSingle = 4, kAdjSingle = 5;
constexpr int NT = 256;
constexpr int U = 4;                        // 4-element groups per lane and chunk
constexpr int kChunk = NT * U * 4;          // 4096 elements
constexpr int kWords = SBG_DIFFAUG_WORDS;

struct Sample { float b, s, k; int tr, tc, r0, r1, c0, c1; };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ Sample load_sample(const int* __restrict__ table, int n, int H, int W, bool drop_b)
{
    const int* p = table + (int64_t)n * kWords;
    Sample a;
    a.b = drop_b ? 0.f : __int_as_float(p[0]);
    a.s = __int_as_float(p[1]);
    a.k = __int_as_float(p[2]);
    a.tr = clampi(p[3], -H, H);             // |t| >= the extent shifts everything out either way; clamped, i + t cannot overflow
    a.tc = clampi(p[4], -W, W);
    a.r0 = clampi(p[5], 0, H); a.r1 = clampi(p[6], 0, H);
    a.c0 = clampi(p[7], 0, W); a.c1 = clampi(p[8], 0, W);
    return a;
}

__device__ __forceinline__ bool inside(int i, int j, int H, int W) { return (unsigned)i < (unsigned)H && (unsigned)j < (unsigned)W; }
__device__ __forceinline__ bool cut(const Sample& a, int i, int j) { return i >= a.r0 && i < a.r1 && j >= a.c0 && j < a.c1; }

// elements e .. e + 3 of p[0, len), zeros behind the end.  VEC: len % 4 == 0 and p + e 16-byte aligned.
template <bool VEC>
__device__ __forceinline__ float4_t load4(const float* __restrict__ p, int e, int len)
{
    float4_t r = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {
        if (e < len) r = *reinterpret_cast<const float4_t*>(p + e);
    } else {
#pragma unroll
        for (int q = 0; q < 4; q++) if (e + q < len) r[q] = p[e + q];
    }
    return r;
}

template <bool VEC>
__device__ __forceinline__ void chunk_load(const float* __restrict__ xs, int e0, int len, float4_t (&r)[U])
{
#pragma unroll
    for (int u = 0; u < U; u++) r[u] = load4<VEC>(xs, e0 + 4 * (u * NT + (int)threadIdx.x), len);
}

// the chunk's sum in the order of the header; ADJ: only the elements of g at live output pixels take part (+ 0.0f is exact)
template <bool ADJ, bool VEC>
__device__ __forceinline__ float chunk_reduce(const float4_t (&r)[U], int e0, int len, int H, int W, const Sample& a, float* red)
{
    const int HW = H * W;
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int e = e0 + 4 * (u * NT + (int)threadIdx.x);
        float4_t v = r[u];
        if (ADJ && e < len) {
            if (VEC) {                      // the four elements share a row
                const int rem = e % HW, i = rem / W, j = rem - i * W;
#pragma unroll
                for (int q = 0; q < 4; q++) if (cut(a, i, j + q) || !inside(i + a.tr, j + q + a.tc, H, W)) v[q] = 0.f;
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (e + q < len) {
                        const int rem = (e + q) % HW, i = rem / W, j = rem - i * W;
                        if (cut(a, i, j) || !inside(i + a.tr, j + a.tc, H, W)) v[q] = 0.f;
                    }
                }
            }
        }
        acc += v[0]; acc += v[1]; acc += v[2]; acc += v[3];
    }
    return block_sum<NT>(acc, red);
}

template <int C>
__device__ __forceinline__ void fwd_pixel(float (&v)[C], const Sample& a, float M)
{
    float m = 0.f;
#pragma unroll
    for (int c = 0; c < C; c++) { v[c] += a.b; m = c == 0 ? v[0] : m + v[c]; }
    if (C > 1) m = m / (float)C;
    const float sm = (1.f - a.s) * m, km = (1.f - a.k) * M;
#pragma unroll
    for (int c = 0; c < C; c++) v[c] = a.k * (a.s * v[c] + sm) + km;
}

template <int C>
__device__ __forceinline__ void adj_pixel(float (&u)[C], const Sample& a, float S)
{
    const float ks = (1.f - a.k) * S;
    float m = 0.f;
#pragma unroll
    for (int c = 0; c < C; c++) { u[c] = a.k * u[c] + ks; m = c == 0 ? u[0] : m + u[c]; }
    if (C > 1) m = m / (float)C;
    const float sm = (1.f - a.s) * m;
#pragma unroll
    for (int c = 0; c < C; c++) u[c] = a.s * u[c] + sm;
}

// PX consecutive pixels of one row, all channels: pixels pix .. pix + PX - 1 of the sample (PX = 4: W % 4 == 0, 16-byte stores).
// `src` is the sample of the input tensor (x, or g for the adjoint) in HBM or LDS; every index into it is predicated.
// `mean` = M (forward) or S (adjoint).
template <int C, bool ADJ, int PX>
__device__ __forceinline__ void do_pixels(const float* __restrict__ src, float* __restrict__ ys, int pix, int H, int W, const Sample& a, float mean)
{
    const int HW = H * W;
    const int i = pix / W, j0 = pix - i * W;
    const int ri = ADJ ? i - a.tr : i + a.tr;               // row read from `src`
    float v[PX][C];
    bool ok[PX];
#pragma unroll
    for (int e = 0; e < PX; e++) {
        const int j = j0 + e;
        const int rj = ADJ ? j - a.tc : j + a.tc;
        // the output pixel of the pair: (i, j) forward, (ri, rj) for the adjoint
        ok[e] = inside(ri, rj, H, W) && !(ADJ ? cut(a, ri, rj) : cut(a, i, j));
#pragma unroll
        for (int c = 0; c < C; c++) v[e][c] = ok[e] ? src[c * HW + ri * W + rj] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < PX; e++) {
        if (ADJ) {
            adj_pixel<C>(v[e], a, mean);
        } else {
            fwd_pixel<C>(v[e], a, mean);
            if (!ok[e]) {
#pragma unroll
                for (int c = 0; c < C; c++) v[e][c] = 0.f;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < C; c++) {
        if (PX == 4) {
            const float4_t o = {v[0][c], v[1][c], v[2][c], v[3][c]};
            *reinterpret_cast<float4_t*>(ys + c * HW + pix) = o;
        } else {
#pragma unroll
            for (int e = 0; e < PX; e++) ys[c * HW + pix + e] = v[e][c];
        }
    }
}

// one workgroup per chunk: partials[n * chunks + chunk] = the chunk's sum
template <bool ADJ, bool VEC>
__global__ __launch_bounds__(NT) void diffaug_sum_kernel(const float* __restrict__ x, const int* __restrict__ table, float* __restrict__ partials,
                                                         int H, int W, int len, int chunks)
{
    __shared__ float red[NT / 64];
    const int n = (int)blockIdx.x / chunks, ch = (int)blockIdx.x - n * chunks;
    const Sample a = load_sample(table, n, H, W, false);
    const float* xs = x + (int64_t)n * len;
    float4_t r[U];
    chunk_load<VEC>(xs, ch * kChunk, len, r);
    const float s = chunk_reduce<ADJ, VEC>(r, ch * kChunk, len, H, W, a, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// `bps` workgroups per sample, one work-item per PX pixels
template <int C, bool ADJ, int PX>
__global__ __launch_bounds__(NT) void diffaug_apply_kernel(const float* __restrict__ x, const int* __restrict__ table, const float* __restrict__ partials,
                                                           float* __restrict__ y, int H, int W, int chunks, int bps, int drop_b)
{
    __shared__ float red[NT / 64];
    const int n = (int)blockIdx.x / bps, blk = (int)blockIdx.x - n * bps;
    const int len = C * H * W;
    const Sample a = load_sample(table, n, H, W, drop_b != 0);
    float acc = 0.f;
    for (int r = threadIdx.x; r < chunks; r += NT) acc += partials[(int64_t)n * chunks + r];
    const float total = block_sum<NT>(acc, red);
    const float mean = total / (float)len;
    const int g = blk * NT + (int)threadIdx.x;
    if (g >= H * W / PX) return;
    do_pixels<C, ADJ, PX>(x + (int64_t)n * len, y + (int64_t)n * len, g * PX, H, W, a, ADJ ? mean : mean + a.b);
}

// C H W <= kChunk: one workgroup per sample, the sample staged in LDS
template <int C, bool ADJ, bool VEC>
__global__ __launch_bounds__(NT) void diffaug_single_kernel(const float* __restrict__ x, const int* __restrict__ table, float* __restrict__ y,
                                                            int H, int W, int drop_b)
{
    __shared__ float4_t stage[kChunk / 4];
    __shared__ float red[NT / 64];
    constexpr int PX = VEC ? 4 : 1;
    const int n = blockIdx.x;
    const int len = C * H * W;
    const Sample a = load_sample(table, n, H, W, drop_b != 0);
    float4_t r[U];
    chunk_load<VEC>(x + (int64_t)n * len, 0, len, r);
#pragma unroll
    for (int u = 0; u < U; u++) stage[u * NT + threadIdx.x] = r[u];
    // its barriers also publish `stage`.  One chunk: the apply kernel's sum over chunk sums would add zeros to it, the same bits
    const float total = chunk_reduce<ADJ, VEC>(r, 0, len, H, W, a, red);
    const float mean = total / (float)len;
    const float* src = reinterpret_cast<const float*>(stage);
    for (int g = threadIdx.x; g < H * W / PX; g += NT)
        do_pixels<C, ADJ, PX>(src, y + (int64_t)n * len, g * PX, H, W, a, ADJ ? mean : mean + a.b);
}

int run(bool adj, const float* x, const int32_t* table, float* y, float* workspace, int N, int C, int H, int W, int drop_b, sbg_stream_t stream)
{
    SBG_CHECK(N >= 0 && H >= 1 && W >= 1, "diffaug: bad sizes N=%d H=%d W=%d", N, H, W);
    SBG_CHECK(C >= 1 && C <= 4, "diffaug: C = %d, 1..4 channels are supported", C);
    const int64_t len64 = (int64_t)C * H * W;
    SBG_CHECK(len64 <= INT32_MAX - 2 * kChunk, "diffaug: a sample of %lld values is too large", (long long)len64);
    if (N == 0) return SBG_OK;
    SBG_CHECK(x && table && y, "diffaug: null pointer");
    SBG_CHECK(x != y, "diffaug: in-place operation is not supported");
    SBG_CHECK(sbg_aligned(x, 4) && sbg_aligned(y, 4) && sbg_aligned(table, 4), "diffaug: pointers must be 4-byte aligned");
    const int len = (int)len64;
    const bool vec = W % 4 == 0 && sbg_aligned16(x) && sbg_aligned16(y);
    const int access = vec ? 1 : 2;
    hipStream_t s = (hipStream_t)stream;
    const double tbytes = (double)N * kWords * 4;

#define SBG_DA_C(KERN, A, B, ...) do { switch (C) { \
        case 1: SBG_LAUNCH((KERN<1, A, B>), __VA_ARGS__); break; case 2: SBG_LAUNCH((KERN<2, A, B>), __VA_ARGS__); break; \
        case 3: SBG_LAUNCH((KERN<3, A, B>), __VA_ARGS__); break; default: SBG_LAUNCH((KERN<4, A, B>), __VA_ARGS__); break; } } while (0)

    if (len <= kChunk) {
        SbgProfScope prof(s, SBG_K_DIFFAUG, 0.0, 8.0 * N * (double)len + tbytes, {adj ? kAdjSingle : kSingle, N, C, H, W, access});
        const dim3 grid((unsigned)N), block(NT);
        if (adj) { if (vec) SBG_DA_C(diffaug_single_kernel, true, true, grid, block, 0, s, x, table, y, H, W, drop_b);
                   else     SBG_DA_C(diffaug_single_kernel, true, false, grid, block, 0, s, x, table, y, H, W, drop_b); }
        else     { if (vec) SBG_DA_C(diffaug_single_kernel, false, true, grid, block, 0, s, x, table, y, H, W, drop_b);
                   else     SBG_DA_C(diffaug_single_kernel, false, false, grid, block, 0, s, x, table, y, H, W, drop_b); }
        SBG_HIP_LAUNCH_CHECK();
        return SBG_OK;
    }

    SBG_CHECK(workspace != nullptr && sbg_aligned(workspace, 4), "diffaug: the workspace must be a 4-byte aligned device pointer");
    const int chunks = (len + kChunk - 1) / kChunk;
    const int groups = H * W / (vec ? 4 : 1);
    const int bps = (groups + NT - 1) / NT;
    SBG_CHECK((int64_t)N * chunks <= INT32_MAX && (int64_t)N * bps <= INT32_MAX, "diffaug: the batch is too large (N=%d)", N);
    {
        SbgProfScope prof(s, SBG_K_DIFFAUG, 0.0, 4.0 * N * (double)len + 4.0 * N * chunks + tbytes, {adj ? kAdjSum : kSum, N, C, H, W, access});
        const dim3 grid((unsigned)(N * chunks)), block(NT);
        if (adj) { if (vec) SBG_LAUNCH((diffaug_sum_kernel<true, true>), grid, block, 0, s, x, table, workspace, H, W, len, chunks);
                   else     SBG_LAUNCH((diffaug_sum_kernel<true, false>), grid, block, 0, s, x, table, workspace, H, W, len, chunks); }
        else     { if (vec) SBG_LAUNCH((diffaug_sum_kernel<false, true>), grid, block, 0, s, x, table, workspace, H, W, len, chunks);
                   else     SBG_LAUNCH((diffaug_sum_kernel<false, false>), grid, block, 0, s, x, table, workspace, H, W, len, chunks); }
        SBG_HIP_LAUNCH_CHECK();
    }
    {
        SbgProfScope prof(s, SBG_K_DIFFAUG, 0.0, 8.0 * N * (double)len + tbytes, {adj ? kAdjApply : kApply, N, C, H, W, access});
        const dim3 grid((unsigned)(N * bps)), block(NT);
        if (adj) { if (vec) SBG_DA_C(diffaug_apply_kernel, true, 4, grid, block, 0, s, x, table, workspace, y, H, W, chunks, bps, drop_b);
                   else     SBG_DA_C(diffaug_apply_kernel, true, 1, grid, block, 0, s, x, table, workspace, y, H, W, chunks, bps, drop_b); }
        else     { if (vec) SBG_DA_C(diffaug_apply_kernel, false, 4, grid, block, 0, s, x, table, workspace, y, H, W, chunks, bps, drop_b);
                   else     SBG_DA_C(diffaug_apply_kernel, false, 1, grid, block, 0, s, x, table, workspace, y, H, W, chunks, bps, drop_b); }
        SBG_HIP_LAUNCH_CHECK();
    }
#undef SBG_DA_C
    return SBG_OK;
}

} // namespace

extern "C" int64_t sbg_diffaug_workspace(int N, int C, int H, int W)
{
    if (N < 0 || C < 1 || C > 4 || H < 1 || W < 1) return -1;
    const int64_t len = (int64_t)C * H * W;
    if (len > INT32_MAX - 2 * kChunk) return -1;
    if (len <= kChunk) return 0;
    return 4 * (int64_t)N * ((len + kChunk - 1) / kChunk);
}

extern "C" int sbg_diffaug_fwd(const float* x, const int32_t* table, float* y, float* workspace, int N, int C, int H, int W, int drop_b, sbg_stream_t stream)
{
    return run(false, x, table, y, workspace, N, C, H, W, drop_b, stream);
}

extern "C" int sbg_diffaug_adj(const float* g, const int32_t* table, float* dx, float* workspace, int N, int C, int H, int W, sbg_stream_t stream)
{
    return run(true, g, table, dx, workspace, N, C, H, W, 0, stream);
}
