// projector.hip -- the arithmetic around the generator and the detector in one step of the latent projector (stylegan2ada/projector.py
// of the reference, `project()` :25-131).  The reference spells each of these as a chain of tensor ops per noise buffer and per pyramid
// level; at sg2ada 256x256 that is 13 buffers and 43 levels, ~1 500 small ops for the regulariser's forward and backward and ~120 for
// the renormalisation, every step.  Here the whole set of buffers is one call:
//   noise_reg:       pool (every pyramid level of every buffer) -> products (per-level, per-chunk partials) -> final (means, reg)
//   noise_reg_bwd:   one pass: d reg / d buf for every element of every buffer, all levels summed in a fixed order
//   noise_normalize: per-chunk sums -> one workgroup per buffer: mean, centre, mean of squares, scale (in place)
//   sqdist:          sum_f (t[f] - s[f])^2, two stages, fixed order;  sqdist_bwd: ds = 2 g (s - t)
// No float atomics and every sum has a fixed order: two runs on the same inputs give the same bits.
// Launch-log key: kind SBG_K_PROJECTOR, one record per launch, dims[0] = variant (0 reg, 1 reg_bwd, 2 normalize, 3 sqdist,
// 4 sqdist_bwd), dims[1] = stage within the variant, then the shape.
#include "sbg_common.h"
#include "reduce.h"
#include "sqdist.h"

namespace {

constexpr int kProjReg = 0, kProjRegBwd = 1, kProjNorm = 2, kProjSqdist = 3, kProjSqdistBwd = 4;
constexpr int kMaxBufs = 32;
constexpr int kThreads = 256;
constexpr int kPoolTile = 128;          // level-0 side of one pooling workgroup's tile: its pyramid reaches side 8 for R <= 1024
constexpr int kProdElems = 4096;        // elements of one level per products workgroup
constexpr int kNormChunk = kThreads * 4 * 4;    // elements per first-stage normalisation workgroup: 4 float4 per work-item
constexpr int kNormThreads = 1024;

// The buffer set, passed by value as a kernel argument.  Buffer b is [R_b, R_b], R_b = 1 << log2r[b].
struct BufTable {
    float* buf[kMaxBufs];
    float* out[kMaxBufs];               // noise_reg_bwd: the gradient of each buffer
    int log2r[kMaxBufs];
    int level_off[kMaxBufs];            // index of the buffer's level 0 in the flat level list (buffer-major)
    int part_off[kMaxBufs];             // index of the buffer's first partial (pair) in the partials area
    int block_off[kMaxBufs + 1];        // first workgroup of each buffer in the current launch
    int64_t pyr_off[kMaxBufs];          // floats: where the buffer's levels 1.. start in the pyramid area
    int nbuf, nlevels;
};

// levels of an R x R buffer: R, R/2, ... down to the first side <= 8 (the reference's `while True: ...; if side <= 8: break`)
__host__ __device__ __forceinline__ int num_levels(int log2r) { return log2r <= 3 ? 1 : log2r - 2; }
__host__ __device__ __forceinline__ int64_t level_offset(int log2r, int k)      // floats of levels 1..k-1 of the buffer's pyramid
{
    int64_t o = 0;
    for (int j = 1; j < k; j++) o += (int64_t)1 << (2 * (log2r - j));
    return o;
}
__host__ __device__ __forceinline__ int prod_chunks(int log2n)                     // products workgroups of a level of side n
{
    const int64_t e = (int64_t)1 << (2 * log2n);
    return e <= kProdElems ? 1 : (int)(e / kProdElems);
}

__device__ __forceinline__ int find_buffer(const BufTable& T, int block)
{
    int b = 0;
    while (b + 1 < T.nbuf && block >= T.block_off[b + 1]) b++;
    return b;
}

__device__ __forceinline__ const float* level_ptr(const BufTable& T, const float* pyr, int b, int k)
{
    return k == 0 ? T.buf[b] : pyr + T.pyr_off[b] + level_offset(T.log2r[b], k);
}

// ---------------------------------------------------------------------------------------------------------------- regulariser forward
// Stage 1: workgroup (buffer, tile) pools its T x T tile of level 0 (T = min(R, 128)) down through every level the buffer has, in
// LDS, and writes levels 1.. to the pyramid.  One output = ((a + b) + c + d) * 0.25 over its 2 x 2 box in row-major order, the
// arithmetic of avg_pool2d(kernel_size=2).
__global__ __launch_bounds__(kThreads) void proj_pool_kernel(BufTable T, float* __restrict__ pyr)
{
#pragma clang fp contract(off)
    __shared__ float lds_a[(kPoolTile / 2) * (kPoolTile / 2)];
    __shared__ float lds_b[(kPoolTile / 4) * (kPoolTile / 4)];
    const int b = find_buffer(T, blockIdx.x);
    const int lr = T.log2r[b], R = 1 << lr, L = num_levels(lr);
    const int tile = R < kPoolTile ? R : kPoolTile;
    const int tiles_x = R / tile, t = blockIdx.x - T.block_off[b];
    const int ty = t / tiles_x, tx = t % tiles_x;
    const float* src = T.buf[b];

    int h = tile / 2;                   // side of the tile's part of level 1
    for (int e = threadIdx.x; e < h * h; e += kThreads) {
        const int i = e / h, j = e % h;
        const int64_t gy = (int64_t)ty * tile + 2 * i, gx = (int64_t)tx * tile + 2 * j;
        const float2 top = *reinterpret_cast<const float2*>(src + gy * R + gx);
        const float2 bot = *reinterpret_cast<const float2*>(src + (gy + 1) * R + gx);
        const float v = (((top.x + top.y) + bot.x) + bot.y) * 0.25f;
        lds_a[e] = v;
        pyr[T.pyr_off[b] + (int64_t)(ty * h + i) * (R >> 1) + tx * h + j] = v;
    }
    float* prev = lds_a;
    float* next = lds_b;
    for (int k = 2; k < L; k++) {
        __syncthreads();
        const int hp = h;
        h >>= 1;
        const int64_t base = T.pyr_off[b] + level_offset(lr, k);
        for (int e = threadIdx.x; e < h * h; e += kThreads) {
            const int i = e / h, j = e % h;
            const float* p = prev + (2 * i) * hp + 2 * j;
            const float v = (((p[0] + p[1]) + p[hp]) + p[hp + 1]) * 0.25f;
            next[e] = v;
            pyr[base + (int64_t)(ty * h + i) * (R >> k) + tx * h + j] = v;
        }
        float* tmp = prev; prev = next; next = tmp;
    }
}

// Stage 2: workgroup (buffer, level, chunk) sums P[i, j] * P[i, j - 1] and P[i, j] * P[i - 1, j] (indices wrap: torch.roll by 1 along W,
// then H) over a band of rows of the level -> one (x, y) partial pair.  Each product is rounded before it is added, as the reference's
// separate multiply and mean do.
__global__ __launch_bounds__(kThreads) void proj_products_kernel(BufTable T, const float* __restrict__ pyr, float* __restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ float red[kThreads / 64];
    const int b = find_buffer(T, blockIdx.x);
    const int lr = T.log2r[b];
    int c = blockIdx.x - T.block_off[b], k = 0, pidx = T.part_off[b];
    while (c >= prod_chunks(lr - k)) { c -= prod_chunks(lr - k); pidx += prod_chunks(lr - k); k++; }
    const int ln = lr - k, n = 1 << ln, nc = prod_chunks(ln);
    const int rows = n / nc;
    const float* P = level_ptr(T, pyr, b, k);
    const int quads = rows * n / 4;     // n >= 4: a row is whole float4s
    float sx = 0.f, sy = 0.f;
    for (int q = threadIdx.x; q < quads; q += kThreads) {
        const int i = c * rows + (4 * q) / n, j = (4 * q) % n;
        const float* row = P + (int64_t)i * n;
        const float4_t v = *reinterpret_cast<const float4_t*>(row + j);
        const float4_t u = *reinterpret_cast<const float4_t*>(P + (int64_t)((i - 1) & (n - 1)) * n + j);
        const float left = row[(j - 1) & (n - 1)];
        const float px0 = v[0] * left, px1 = v[1] * v[0], px2 = v[2] * v[1], px3 = v[3] * v[2];
        const float py0 = v[0] * u[0], py1 = v[1] * u[1], py2 = v[2] * u[2], py3 = v[3] * u[3];
        sx += px0; sx += px1; sx += px2; sx += px3;
        sy += py0; sy += py1; sy += py2; sy += py3;
    }
    const float tx = block_sum<kThreads>(sx, red);
    const float ty = block_sum<kThreads>(sy, red);
    if (threadIdx.x == 0) {
        float2 o; o.x = tx; o.y = ty;
        reinterpret_cast<float2*>(part)[pidx + c] = o;
    }
}

// Stage 3: one workgroup.  Level l's means m_x, m_y = (sum of its partials in chunk order) / n^2 -> means[2l], means[2l + 1]; then
// reg = sum of every m^2 in the reference's order (buffer, level, x before y), one work-item, sequentially.
__global__ __launch_bounds__(kThreads) void proj_reg_final_kernel(BufTable T, const float* __restrict__ part, float* __restrict__ means,
                                                                  float* __restrict__ reg)
{
#pragma clang fp contract(off)
    __shared__ float m[2 * kMaxBufs * 8];
    for (int l = threadIdx.x; l < T.nlevels; l += kThreads) {
        int b = 0;
        while (b + 1 < T.nbuf && l >= T.level_off[b + 1]) b++;
        const int k = l - T.level_off[b], lr = T.log2r[b];
        int pidx = T.part_off[b];
        for (int j = 0; j < k; j++) pidx += prod_chunks(lr - j);
        const int ln = lr - k, nc = prod_chunks(ln);
        float sx = 0.f, sy = 0.f;
        for (int q = 0; q < nc; q++) {
            const float2 p = reinterpret_cast<const float2*>(part)[pidx + q];
            sx += p.x; sy += p.y;
        }
        const float area = (float)((int64_t)1 << (2 * ln));
        const float mx = sx / area, my = sy / area;
        m[2 * l] = mx; m[2 * l + 1] = my;
        float2 o; o.x = mx; o.y = my;
        reinterpret_cast<float2*>(means)[l] = o;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = 0.f;
        for (int i = 0; i < 2 * T.nlevels; i++) { const float sq = m[i] * m[i]; r += sq; }
        reg[0] = r;
    }
}

// ---------------------------------------------------------------------------------------------------------------- regulariser backward
// One pass.  Work-item (buffer, y, x0..x0+3): for every level k of side n, deepest first,
//   G_k[i, j] = 2 (m_x (P[i, j-1] + P[i, j+1]) + m_y (P[i-1, j] + P[i+1, j])) / n^2   at (i, j) = (y >> k, x >> k), indices wrap,
//   acc = G_k + acc / 4   (so acc = sum_k G_k / 4^k at level 0, the pooling's backward chained from the deepest level),
// then dbuf = g * acc.
__global__ __launch_bounds__(kThreads) void proj_reg_bwd_kernel(BufTable T, const float* __restrict__ pyr, const float* __restrict__ means,
                                                                const float* __restrict__ gptr)
{
#pragma clang fp contract(off)
    const int b = find_buffer(T, blockIdx.x);
    const int lr = T.log2r[b], R = 1 << lr, L = num_levels(lr);
    const int64_t e = ((int64_t)(blockIdx.x - T.block_off[b]) * kThreads + threadIdx.x) * 4;
    if (e >= ((int64_t)R << lr)) return;
    const int y = (int)(e >> lr), x0 = (int)(e & (R - 1));
    const float g = gptr[0];
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = L - 1; k >= 0; k--) {
        const int ln = lr - k, n = 1 << ln;
        const float* P = level_ptr(T, pyr, b, k);
        const float2 mm = reinterpret_cast<const float2*>(means)[T.level_off[b] + k];
        const float area = (float)((int64_t)1 << (2 * ln));
        const int i = y >> k;
        const float* row = P + (int64_t)i * n;
        const float* up = P + (int64_t)((i - 1) & (n - 1)) * n;
        const float* dn = P + (int64_t)((i + 1) & (n - 1)) * n;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int j = (x0 + q) >> k;
            const float hx = row[(j - 1) & (n - 1)] + row[(j + 1) & (n - 1)];
            const float hy = up[j] + dn[j];
            const float tx = mm.x * hx, ty = mm.y * hy;
            const float G = (2.0f * (tx + ty)) / area;
            acc[q] = k == L - 1 ? G : G + acc[q] * 0.25f;
        }
    }
    float4_t o;
#pragma unroll
    for (int q = 0; q < 4; q++) o[q] = g * acc[q];
    *reinterpret_cast<float4_t*>(T.out[b] + e) = o;
}

// ---------------------------------------------------------------------------------------------------------------- renormalisation
// Stage 1: workgroup (buffer, chunk) sums its kNormChunk elements in a fixed order -> part[part_off[b] + chunk].
__global__ __launch_bounds__(kThreads) void proj_norm_partial_kernel(BufTable T, float* __restrict__ part)
{
    __shared__ float red[kThreads / 64];
    const int b = find_buffer(T, blockIdx.x);
    const int lr = T.log2r[b];
    const int64_t total = (int64_t)1 << (2 * lr);
    const int c = blockIdx.x - T.block_off[b];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int64_t e = (int64_t)c * kNormChunk + 4 * ((int64_t)k * kThreads + threadIdx.x);
        if (e < total) {
            const float4_t v = *reinterpret_cast<const float4_t*>(T.buf[b] + e);
            s += v[0]; s += v[1]; s += v[2]; s += v[3];
        }
    }
    const float tot = block_sum<kThreads>(s, red);
    if (threadIdx.x == 0) part[T.part_off[b] + c] = tot;
}

// Stage 2: one workgroup per buffer.  mean = (sum of the partials in order) / R^2; c = buf - mean (rounded, as `buf -= buf.mean()`
// stores it); v = (sum of c^2) / R^2; buf = c * rsqrt(v).
__global__ __launch_bounds__(kNormThreads) void proj_norm_apply_kernel(BufTable T, const float* __restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ float red[kNormThreads / 64];
    __shared__ float bcast;
    const int b = blockIdx.x;
    const int lr = T.log2r[b];
    const int64_t total = (int64_t)1 << (2 * lr);
    const int nc = (int)((total + kNormChunk - 1) / kNormChunk);
    const float area = (float)total;
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int q = 0; q < nc; q++) s += part[T.part_off[b] + q];
        bcast = s / area;
    }
    __syncthreads();
    const float mean = bcast;
    float* p = T.buf[b];
    float ss = 0.f;
    for (int64_t e = 4 * (int64_t)threadIdx.x; e < total; e += 4 * kNormThreads) {
        const float4_t v = *reinterpret_cast<const float4_t*>(p + e);
#pragma unroll
        for (int q = 0; q < 4; q++) { const float c = v[q] - mean; const float c2 = c * c; ss += c2; }
    }
    const float scale = rsqrtf(block_sum<kNormThreads>(ss, red) / area);
    for (int64_t e = 4 * (int64_t)threadIdx.x; e < total; e += 4 * kNormThreads) {
        const float4_t v = *reinterpret_cast<const float4_t*>(p + e);
        float4_t o;
#pragma unroll
        for (int q = 0; q < 4; q++) o[q] = (v[q] - mean) * scale;
        *reinterpret_cast<float4_t*>(p + e) = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------- LPIPS distance
// The forward value is the shared kernel pair of sqdist.h on one row.

// ds[f] = (2 (s[f] - t[f])) * g: the value autograd gives the reference's (t - s).square().sum() for s (pow backward, then the negation)
__global__ __launch_bounds__(kThreads) void proj_sqdist_bwd_kernel(const float* __restrict__ t, const float* __restrict__ s,
                                                                   const float* __restrict__ gptr, float* __restrict__ ds, int64_t F, int vec4)
{
#pragma clang fp contract(off)
    const float g = gptr[0];
    const int64_t items = vec4 ? F / 4 : F;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        if (vec4) {
            const float4_t a = *reinterpret_cast<const float4_t*>(t + 4 * i), c = *reinterpret_cast<const float4_t*>(s + 4 * i);
            float4_t o;
#pragma unroll
            for (int q = 0; q < 4; q++) o[q] = (2.0f * (c[q] - a[q])) * g;
            *reinterpret_cast<float4_t*>(ds + 4 * i) = o;
        } else {
            ds[i] = (2.0f * (s[i] - t[i])) * g;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
int log2_exact(int r)
{
    if (r < 4 || r > 1024 || (r & (r - 1))) return -1;
    int l = 0;
    while ((1 << l) < r) l++;
    return l;
}

// Fills the table's shape fields from res[]; returns false (with the error status set) for an unsupported set.
bool fill_table(BufTable& T, const int* res, int nbuf, const char* what)
{
    if (!res || nbuf < 1 || nbuf > kMaxBufs) {
        sbg_fail(SBG_ERR_INVALID, "%s: %d buffers (1 .. %d supported)", what, nbuf, kMaxBufs);
        return false;
    }
    T = BufTable{};
    T.nbuf = nbuf;
    int levels = 0, parts = 0;
    int64_t pyr = 0;
    for (int b = 0; b < nbuf; b++) {
        const int lr = log2_exact(res[b]);
        if (lr < 0) {
            sbg_fail(SBG_ERR_INVALID, "%s: buffer %d is %d x %d; the side must be a power of two in [4, 1024]", what, b, res[b], res[b]);
            return false;
        }
        T.log2r[b] = lr;
        T.level_off[b] = levels;
        T.part_off[b] = parts;
        T.pyr_off[b] = pyr;
        const int L = num_levels(lr);
        levels += L;
        for (int k = 0; k < L; k++) parts += prod_chunks(lr - k);
        pyr += level_offset(lr, L);
    }
    T.nlevels = levels;
    return true;
}

struct RegLayout { int64_t pyr_floats, part_pairs; };
RegLayout reg_layout(const BufTable& T)
{
    RegLayout l{0, 0};
    const int b = T.nbuf - 1;
    l.pyr_floats = T.pyr_off[b] + level_offset(T.log2r[b], num_levels(T.log2r[b]));
    l.part_pairs = T.part_off[b];
    for (int k = 0; k < num_levels(T.log2r[b]); k++) l.part_pairs += prod_chunks(T.log2r[b] - k);
    return l;
}
int64_t pyr_bytes_aligned(const RegLayout& l) { return (l.pyr_floats * 4 + 255) / 256 * 256; }

int64_t norm_chunks(int lr) { return (((int64_t)1 << (2 * lr)) + kNormChunk - 1) / kNormChunk; }

} // namespace

extern "C" int64_t sbg_proj_noise_reg_workspace(const int* res, int nbuf)
{
    BufTable T;
    if (!fill_table(T, res, nbuf, "proj_noise_reg_workspace")) return -1;
    const RegLayout l = reg_layout(T);
    return pyr_bytes_aligned(l) + l.part_pairs * 8;
}

extern "C" int sbg_proj_noise_reg(const float* const* bufs, const int* res, int nbuf, float* means, float* reg, void* workspace,
                                  sbg_stream_t stream)
{
    BufTable T;
    if (!fill_table(T, res, nbuf, "proj_noise_reg")) return SBG_ERR_INVALID;
    SBG_CHECK(bufs && means && reg && workspace && sbg_aligned16(workspace) && sbg_aligned(means, 8), "proj_noise_reg: null or misaligned pointer");
    for (int b = 0; b < nbuf; b++) {
        SBG_CHECK(bufs[b] && sbg_aligned16(bufs[b]), "proj_noise_reg: buffer %d is null or not 16-byte aligned", b);
        T.buf[b] = const_cast<float*>(bufs[b]);
    }
    const RegLayout l = reg_layout(T);
    float* pyr = (float*)workspace;
    float* part = (float*)((char*)workspace + pyr_bytes_aligned(l));
    hipStream_t s = (hipStream_t)stream;
    int64_t elems = 0;
    for (int b = 0; b < nbuf; b++) elems += (int64_t)1 << (2 * T.log2r[b]);

    int blocks = 0;                     // pooling: (R / tile)^2 workgroups per buffer with more than one level
    for (int b = 0; b < nbuf; b++) {
        T.block_off[b] = blocks;
        const int lr = T.log2r[b], R = 1 << lr, tile = R < kPoolTile ? R : kPoolTile;
        if (num_levels(lr) > 1) blocks += (R / tile) * (R / tile);
    }
    T.block_off[nbuf] = blocks;
    if (blocks > 0) {
        SbgProfScope prof(s, SBG_K_PROJECTOR, 0.0, 4.0 * (elems + l.pyr_floats), {kProjReg, 0, nbuf, T.nlevels});
        SBG_LAUNCH(proj_pool_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, T, pyr);
    }
    blocks = 0;                         // products: one workgroup per (level, band of rows)
    for (int b = 0; b < nbuf; b++) {
        T.block_off[b] = blocks;
        for (int k = 0; k < num_levels(T.log2r[b]); k++) blocks += prod_chunks(T.log2r[b] - k);
    }
    T.block_off[nbuf] = blocks;
    {
        SbgProfScope prof(s, SBG_K_PROJECTOR, 4.0 * (elems + l.pyr_floats), 8.0 * (elems + l.pyr_floats) + 8.0 * l.part_pairs,
                          {kProjReg, 1, nbuf, T.nlevels});
        SBG_LAUNCH(proj_products_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, T, (const float*)pyr, part);
    }
    {
        SbgProfScope prof(s, SBG_K_PROJECTOR, 0.0, 8.0 * l.part_pairs + 8.0 * T.nlevels + 4.0, {kProjReg, 2, nbuf, T.nlevels});
        SBG_LAUNCH(proj_reg_final_kernel, dim3(1), dim3(kThreads), 0, s, T, (const float*)part, means, reg);
    }
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int sbg_proj_noise_reg_bwd(const float* const* bufs, float* const* grads, const int* res, int nbuf, const float* means,
                                      const float* g, const void* workspace, sbg_stream_t stream)
{
    BufTable T;
    if (!fill_table(T, res, nbuf, "proj_noise_reg_bwd")) return SBG_ERR_INVALID;
    SBG_CHECK(bufs && grads && means && g && workspace && sbg_aligned16(workspace) && sbg_aligned(means, 8),
              "proj_noise_reg_bwd: null or misaligned pointer");
    int blocks = 0;
    int64_t elems = 0;
    for (int b = 0; b < nbuf; b++) {
        SBG_CHECK(bufs[b] && grads[b] && sbg_aligned16(grads[b]), "proj_noise_reg_bwd: buffer %d is null or not 16-byte aligned", b);
        T.buf[b] = const_cast<float*>(bufs[b]);
        T.out[b] = grads[b];
        T.block_off[b] = blocks;
        const int64_t e = (int64_t)1 << (2 * T.log2r[b]);
        elems += e;
        blocks += (int)((e / 4 + kThreads - 1) / kThreads);
    }
    T.block_off[nbuf] = blocks;
    hipStream_t s = (hipStream_t)stream;
    SbgProfScope prof(s, SBG_K_PROJECTOR, 12.0 * elems, 8.0 * elems + 4.0 * reg_layout(T).pyr_floats, {kProjRegBwd, 0, nbuf, T.nlevels});
    SBG_LAUNCH(proj_reg_bwd_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, T, (const float*)workspace, means, g);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int64_t sbg_proj_noise_normalize_workspace(const int* res, int nbuf)
{
    BufTable T;
    if (!fill_table(T, res, nbuf, "proj_noise_normalize_workspace")) return -1;
    int64_t n = 0;
    for (int b = 0; b < nbuf; b++) n += norm_chunks(T.log2r[b]);
    return n * 4;
}

extern "C" int sbg_proj_noise_normalize(float* const* bufs, const int* res, int nbuf, void* workspace, sbg_stream_t stream)
{
    BufTable T;
    if (!fill_table(T, res, nbuf, "proj_noise_normalize")) return SBG_ERR_INVALID;
    SBG_CHECK(bufs && workspace, "proj_noise_normalize: null pointer");
    int blocks = 0;
    int64_t elems = 0;
    for (int b = 0; b < nbuf; b++) {
        SBG_CHECK(bufs[b] && sbg_aligned16(bufs[b]), "proj_noise_normalize: buffer %d is null or not 16-byte aligned", b);
        T.buf[b] = bufs[b];
        T.part_off[b] = blocks;         // one partial per first-stage workgroup
        T.block_off[b] = blocks;
        blocks += (int)norm_chunks(T.log2r[b]);
        elems += (int64_t)1 << (2 * T.log2r[b]);
    }
    T.block_off[nbuf] = blocks;
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)workspace;
    {
        SbgProfScope prof(s, SBG_K_PROJECTOR, 1.0 * elems, 4.0 * (elems + blocks), {kProjNorm, 0, nbuf});
        SBG_LAUNCH(proj_norm_partial_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, T, part);
    }
    {
        SbgProfScope prof(s, SBG_K_PROJECTOR, 5.0 * elems, 4.0 * (3 * elems + blocks), {kProjNorm, 1, nbuf});
        SBG_LAUNCH(proj_norm_apply_kernel, dim3((unsigned)nbuf), dim3(kNormThreads), 0, s, T, (const float*)part);
    }
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int64_t sbg_proj_sqdist_workspace(int64_t F)
{
    if (F < 1) return -1;
    return dist_chunks(F) * (int64_t)sizeof(float);
}

extern "C" int sbg_proj_sqdist(const float* t, const float* s_, float* dist, void* workspace, int64_t F, sbg_stream_t stream)
{
    SBG_CHECK(t && s_ && dist && workspace, "proj_sqdist: null pointer");
    SBG_CHECK(F >= 1, "proj_sqdist: bad size F=%lld", (long long)F);
    const int64_t nchunk = dist_chunks(F);
    SBG_CHECK(nchunk <= (1 << 30), "proj_sqdist: F=%lld too large", (long long)F);
    hipStream_t s = (hipStream_t)stream;
    const int vec4 = (F % 4 == 0) && sbg_aligned16(t) && sbg_aligned16(s_);
    {
        SbgProfScope prof(s, SBG_K_PROJECTOR, 3.0 * F, 8.0 * F + 4.0 * nchunk, {kProjSqdist, 0, (int)(F >> 10), (int)(F & 1023), vec4});
        SBG_LAUNCH(sqdist_partial_kernel<false>, dim3((unsigned)nchunk, 1), dim3(kDistThreads), 0, s, t, s_, (float*)workspace, F, (int)nchunk, vec4);
    }
    SbgProfScope prof(s, SBG_K_PROJECTOR, 1.0 * nchunk, 4.0 * nchunk + 4.0, {kProjSqdist, 1, (int)(F >> 10), (int)(F & 1023), vec4});
    return merge_partials<float>((const float*)workspace, dist, 1, (int)nchunk, 1.0f, s);
}

extern "C" int sbg_proj_sqdist_bwd(const float* t, const float* s_, const float* g, float* ds, int64_t F, sbg_stream_t stream)
{
    SBG_CHECK(t && s_ && g && ds, "proj_sqdist_bwd: null pointer");
    SBG_CHECK(F >= 1, "proj_sqdist_bwd: bad size F=%lld", (long long)F);
    hipStream_t s = (hipStream_t)stream;
    const int vec4 = (F % 4 == 0) && sbg_aligned16(t) && sbg_aligned16(s_) && sbg_aligned16(ds);
    const int64_t items = vec4 ? F / 4 : F;
    SbgProfScope prof(s, SBG_K_PROJECTOR, 3.0 * F, 12.0 * F + 4.0, {kProjSqdistBwd, 0, (int)(F >> 10), (int)(F & 1023), vec4});
    SBG_LAUNCH(proj_sqdist_bwd_kernel, dim3(sbg_stream_grid(items, kThreads)), dim3(kThreads), 0, s, t, s_, g, ds, F, vec4);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}
