// msssim.hip -- the per-level terms of multi-scale structural similarity between two image batches (Wang, Simoncelli, Bovik, "Multi-scale
// structural similarity for image quality assessment", Asilomar 2003; the pairwise diversity tool diversity.py).
// Images are fp32 or uint8 byte values [BC, S, S], S a power of two >= 16; every moment, map value and sum is float64.
//
// Per image-channel, with the 11-tap window g (float64, computed on the host, one table for both devices) and n = S - 10:
//   the five images x, y, x x, y y, x y (the products of two fp32 values are exact in float64) are filtered "valid", along x first, then along
//   y; a 1-D pass is  acc = 0; for k = 0..10: acc = acc + g[k] v[k],  the product and the sum each rounded once;
//   s11 = Fxx - m1 m1,  s22 = Fyy - m2 m2,  s12 = Fxy - m1 m2,
//   cs = (2 s12 + C2) / ((s11 + s22) + C2),   l = (2 (m1 m2) + C1) / ((m1 m1 + m2 m2) + C1),   ssim = l cs,
//   every operation rounded on its own: the pragma below keeps the compiler from contracting a product into a sum (the _rn intrinsics do
//   not on this toolchain, see spectrum.hip).  out[bc] = {mean of cs, mean of ssim} over the n x n map.
// torch_utils/ops/msssim.py states the same graph and the same sum order with torch / numpy for CPU tensors; both devices give the same bits.
// level: one workgroup of 256 owns a tile of 16 rows x 32 columns of one image-channel's map.  It stages the 26 x 42 source pixels of both
//  images in LDS as fp32 (pixels past the image edge as 0: they feed map entries outside the map only), runs the row pass of the five
//  moments into a float64 LDS array [5][26][32], then the column pass from there: lane t owns the map entries (t / 32 + 8 i, t mod 32),
//  i = 0, 1, evaluates cs and ssim in registers and adds them in that order from 0, an entry outside the map as 0.  block_sum (reduce.h)
//  adds the lanes; the workgroup writes one pair of tile partials.  A half wave reads 32 consecutive float64 of one row (all 64 banks
//  once) at every step of the column walk, and 32 consecutive fp32 in the row pass: no pitch padding is needed.  A map smaller than the
//  tile takes the same path.  LDS: 2 x 26 x 42 x 4 + 5 x 26 x 32 x 8 + 32 = 42048 bytes.
// merge: the shared merge kernel (merge.h) adds the tile partials of one (image-channel, term), tiles in row-major order, and divides the
//  sum by n n.  No atomics; the order depends on S alone.
// down: y[i, j] = ((a + b) + (c + d)) * 0.25f in fp32, a b the upper left and right pixels of the 2 x 2 block, c d the lower ones.
// Launch-log key: kind SBG_K_MSSSIM, dims = {0 level | 1 down | 2 merge, BC clipped to INT32_MAX, S}.
#pragma clang fp contract(off)
#include "sbg_common.h"
#include "reduce.h"
#include "merge.h"

namespace {

constexpr int kLevel = 0, kDown = 1, kMerge = 2;
constexpr int NT = 256;
constexpr int kTaps = 11, kHalo = kTaps - 1;
constexpr int TW = 32, TH = 16;                         // map tile of one workgroup
constexpr int IW = TW + kHalo, IH = TH + kHalo;         // its source pixels
constexpr int kMaxSide = 16384;
constexpr int64_t kMaxGrid = (int64_t)1 << 24;          // workgroups of one launch: 2^32 work-items

template <class T>
__global__ __launch_bounds__(NT) void msssim_level_kernel(const T* __restrict__ x, const T* __restrict__ y, const double* __restrict__ g,
                                                          double* __restrict__ partial, int S, int n, int tiles_x, int tiles, double C1, double C2)
{
    __shared__ float xs[IH * IW], ys[IH * IW];
    __shared__ double mom[5][IH][TW];
    __shared__ double red[NT / 64];
    const int tid = threadIdx.x;
    const int64_t bc = blockIdx.x / (unsigned)tiles;
    const int tile = (int)(blockIdx.x % (unsigned)tiles);
    const int oy0 = (tile / tiles_x) * TH, ox0 = (tile % tiles_x) * TW;
    const T* xp = x + bc * S * S;
    const T* yp = y + bc * S * S;
    double w[kTaps];
#pragma unroll
    for (int k = 0; k < kTaps; k++) w[k] = g[k];

    for (int idx = tid; idx < IH * IW; idx += NT) {
        const int r = idx / IW, c = idx - r * IW;
        const int iy = oy0 + r, ix = ox0 + c;
        const bool ok = iy < S && ix < S;
        xs[idx] = ok ? sbg_pixel(xp[(int64_t)iy * S + ix]) : 0.f;
        ys[idx] = ok ? sbg_pixel(yp[(int64_t)iy * S + ix]) : 0.f;
    }
    __syncthreads();

    for (int idx = tid; idx < IH * TW; idx += NT) {     // the row pass: along x
        const int r = idx / TW, c = idx - r * TW;
        double ax = 0.0, ay = 0.0, axx = 0.0, ayy = 0.0, axy = 0.0;
#pragma unroll
        for (int k = 0; k < kTaps; k++) {
            const double a = (double)xs[r * IW + c + k], b = (double)ys[r * IW + c + k];
            ax = ax + w[k] * a;
            ay = ay + w[k] * b;
            axx = axx + w[k] * (a * a);
            ayy = ayy + w[k] * (b * b);
            axy = axy + w[k] * (a * b);
        }
        mom[0][r][c] = ax; mom[1][r][c] = ay; mom[2][r][c] = axx; mom[3][r][c] = ayy; mom[4][r][c] = axy;
    }
    __syncthreads();

    double sum_cs = 0.0, sum_ssim = 0.0;
    const int c = tid % TW;
#pragma unroll
    for (int i = 0; i < TH * TW / NT; i++) {            // the column pass: along y
        const int r = tid / TW + i * (NT / TW);
        double m1 = 0.0, m2 = 0.0, fxx = 0.0, fyy = 0.0, fxy = 0.0;
#pragma unroll
        for (int k = 0; k < kTaps; k++) {
            m1 = m1 + w[k] * mom[0][r + k][c];
            m2 = m2 + w[k] * mom[1][r + k][c];
            fxx = fxx + w[k] * mom[2][r + k][c];
            fyy = fyy + w[k] * mom[3][r + k][c];
            fxy = fxy + w[k] * mom[4][r + k][c];
        }
        const double m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
        const double s11 = fxx - m11, s22 = fyy - m22, s12 = fxy - m12;
        const double cs = (2.0 * s12 + C2) / ((s11 + s22) + C2);
        const double l = (2.0 * m12 + C1) / ((m11 + m22) + C1);
        const double ssim = l * cs;
        const bool in = oy0 + r < n && ox0 + c < n;
        sum_cs = sum_cs + (in ? cs : 0.0);
        sum_ssim = sum_ssim + (in ? ssim : 0.0);
    }
    sum_cs = block_sum<NT>(sum_cs, red);
    sum_ssim = block_sum<NT>(sum_ssim, red);
    if (tid == 0) {
        partial[(2 * bc) * tiles + tile] = sum_cs;
        partial[(2 * bc + 1) * tiles + tile] = sum_ssim;
    }
}

template <class T>
__global__ __launch_bounds__(NT) void msssim_down_kernel(const T* __restrict__ x, float* __restrict__ y, int64_t total, int S, int logH)
{
    const int H = S / 2;                                // a power of two
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
        const int ox = (int)(i & (H - 1)), oy = (int)((i >> logH) & (H - 1));
        const int64_t plane = i >> (2 * logH);
        const T* p = x + (plane * S + 2 * oy) * S + 2 * ox;
        const float a = sbg_pixel(p[0]), b = sbg_pixel(p[1]), c = sbg_pixel(p[S]), d = sbg_pixel(p[S + 1]);
        y[i] = ((a + b) + (c + d)) * 0.25f;
    }
}

inline int tiles_of(int S, int* tiles_x)
{
    const int n = S - kHalo, tx = (n + TW - 1) / TW, ty = (n + TH - 1) / TH;
    if (tiles_x) *tiles_x = tx;
    return tx * ty;
}

} // namespace

extern "C" int64_t sbg_msssim_workspace(int64_t BC, int S)
{
    if (BC < 1 || !sbg_pow2_in(S, 16, kMaxSide)) return -1;
    const int64_t tiles = tiles_of(S, nullptr);
    if (BC > kMaxGrid / tiles) return -1;
    return 8 * 2 * BC * tiles;
}

extern "C" int sbg_msssim_level(const void* x, const void* y, int is_u8, const double* window, double C1, double C2, double* out, void* workspace,
                                int64_t BC, int S, sbg_stream_t stream)
{
    SBG_CHECK(sbg_msssim_workspace(BC, S) >= 0, "msssim_level: bad sizes BC=%lld S=%d (S a power of two in [16, %d], BC x tiles <= 2^24)",
              (long long)BC, S, kMaxSide);
    SBG_CHECK(x && y && window && out && workspace && sbg_aligned(x, is_u8 ? 1 : 4) && sbg_aligned(y, is_u8 ? 1 : 4) && sbg_aligned(window, 8) && sbg_aligned(out, 8)
              && sbg_aligned(workspace, 8), "msssim_level: null or misaligned pointer");
    SBG_CHECK(C1 > 0.0 && C2 > 0.0, "msssim_level: the constants C1=%g and C2=%g must be positive", C1, C2);
    int tiles_x = 0;
    const int tiles = tiles_of(S, &tiles_x), n = S - kHalo;
    static_assert(sizeof(float) * 2 * IH * IW + sizeof(double) * (5 * IH * TW + NT / 64) < 64 * 1024, "the level kernel's LDS");
    static_assert(TH * TW % NT == 0 && NT % TW == 0, "whole map rows per lane step");
    hipStream_t st = (hipStream_t)stream;
    const double px = (double)BC * S * S;
    {
        SbgProfScope prof(st, SBG_K_MSSSIM, 2.0 * 5 * kTaps * 2 * px, (is_u8 ? 2.0 : 8.0) * px + 16.0 * (double)BC * tiles, {kLevel, sbg_clip31(BC), S});
        if (is_u8)
            SBG_LAUNCH(msssim_level_kernel<unsigned char>, dim3((unsigned)(BC * tiles)), dim3(NT), 0, st, (const unsigned char*)x, (const unsigned char*)y,
                       window, (double*)workspace, S, n, tiles_x, tiles, C1, C2);
        else
            SBG_LAUNCH(msssim_level_kernel<float>, dim3((unsigned)(BC * tiles)), dim3(NT), 0, st, (const float*)x, (const float*)y, window,
                       (double*)workspace, S, n, tiles_x, tiles, C1, C2);
        SBG_HIP_LAUNCH_CHECK();
    }
    SbgProfScope prof(st, SBG_K_MSSSIM, 0.0, 16.0 * (double)BC * tiles + 16.0 * (double)BC, {kMerge, sbg_clip31(BC), S});
    return merge_partials<double>((const double*)workspace, out, 2 * BC, tiles, (double)n * (double)n, st);
}

extern "C" int sbg_msssim_down(const void* x, int is_u8, float* y, int64_t BC, int S, sbg_stream_t stream)
{
    SBG_CHECK(BC >= 0 && BC <= ((int64_t)1 << 40), "msssim_down: bad size BC=%lld", (long long)BC);
    SBG_CHECK(sbg_pow2_in(S, 2, kMaxSide), "msssim_down: side %d, a power of two in [2, %d] is supported", S, kMaxSide);
    if (BC == 0) return SBG_OK;
    SBG_CHECK(x && y && (const void*)x != (const void*)y && sbg_aligned(x, is_u8 ? 1 : 4) && sbg_aligned(y, 4), "msssim_down: x and y must be distinct aligned device pointers");
    const int64_t total = BC * (S / 2) * (S / 2);
    hipStream_t st = (hipStream_t)stream;
    SbgProfScope prof(st, SBG_K_MSSSIM, 0.0, (is_u8 ? 4.0 : 16.0) * total + 4.0 * total, {kDown, sbg_clip31(BC), S});
    int logH = 0;
    while ((2 << logH) < S) logH++;
    if (is_u8)
        SBG_LAUNCH(msssim_down_kernel<unsigned char>, dim3(sbg_stream_grid(total, NT)), dim3(NT), 0, st, (const unsigned char*)x, y, total, S, logH);
    else
        SBG_LAUNCH(msssim_down_kernel<float>, dim3(sbg_stream_grid(total, NT)), dim3(NT), 0, st, (const float*)x, y, total, S, logH);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}
