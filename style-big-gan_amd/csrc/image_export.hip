// image_export.hip -- the arithmetic of the image writers: float images -> bytes in a grid canvas, and the latent table of the style matrix.
//   quantize_tile:  fp32 [N, C, H, W] (any strides) -> uint8 HWC canvas [gh * H, gw * W, C], image n in cell cell0 + n.  The reference spells this
//                   as subtract, multiply, rint, clip, cast, reshape, transpose, reshape on the host (`save_image_grid`, train_parts/trainers.py:
//                   102-112) or permute, multiply, add, clamp, cast on the device (stylegan2ada/generate.py:98,120); here it is one pass.
//   truncate_mix:   [S, L, D] mapped latents -> [R * Cn, L, D] truncated and style-mixed rows (stylegan2ada/style_mixing.py:74, 85-86), so the
//                   style matrix can be synthesised in batches.
// Both are streaming kernels: every input element is read once and every output element written once.
// Launch-log key: kind SBG_K_IMAGE_EXPORT, dims[0] = variant (0 quantize_tile, 1 truncate_mix), then the shape and the kernel variant.
#include "sbg_common.h"

namespace {

constexpr int kVarQuantize = 0, kVarMix = 1;
constexpr int kPlanar4 = 1, kMinor4 = 2, kPixel = 3;     // quantize_tile: how a work-item reads its pixels

// One value -> one byte.  Each arithmetic step rounds on its own (the reference's are separate array operations), so no contraction.
// fmaxf(NaN, 0) is 0: a NaN writes 0; +-inf clamp.
template <int RULE> __device__ __forceinline__ unsigned quantize(float x, float lo, float scale)
{
#pragma clang fp contract(off)
    float v;
    if (RULE == SBG_QUANT_GRID) {
        v = x - lo;
        v = v * scale;
        v = rintf(v);                       // round half to even, like np.rint
    } else {
        v = x * 127.5f;
        v = v + 128.0f;
    }
    v = fminf(fmaxf(v, 0.0f), 255.0f);
    return (unsigned)(int)v;                // the clamp rule truncates here; the grid rule's value is already integral
}

// MODE kPlanar4 / kMinor4: one work-item per four consecutive pixels of a row (W % 4 == 0, rows 16-byte aligned).  Planar reads one float4 per
// channel plane, channel-minor (C = 3, sc = 1, sw = 3) reads the twelve interleaved floats as three float4.  The 4 * C bytes start at a
// multiple of 4 * C bytes of the canvas and leave as C aligned dwords.  MODE kPixel: one work-item per pixel, C strided reads, C byte writes.
template <int RULE, int C, int MODE>
__global__ __launch_bounds__(256) void quantize_tile_kernel(const float* __restrict__ img, uint8_t* __restrict__ canvas, int N, int H, int W,
                                                            int64_t sn, int64_t sc, int64_t sh, int64_t sw, int gw, int cell0, float lo, float scale)
{
    constexpr int P = MODE == kPixel ? 1 : 4;
    const int WP = W / P;
    const int64_t total = (int64_t)N * H * WP;
    const int64_t row_bytes = (int64_t)gw * W * C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % WP) * P;
        const int y = (int)((i / WP) % H);
        const int n = (int)(i / ((int64_t)WP * H));
        const int cell = cell0 + n, gy = cell / gw, gx = cell - gy * gw;
        const float* src = img + n * sn + y * sh + x * sw;
        uint8_t* dst = canvas + ((int64_t)gy * H + y) * row_bytes + ((int64_t)gx * W + x) * C;
        if (MODE == kPixel) {
#pragma unroll
            for (int c = 0; c < C; c++) dst[c] = (uint8_t)quantize<RULE>(src[c * sc], lo, scale);
        } else {
            unsigned b[4 * C];              // bytes in canvas order: pixel-major, channel-minor
            if (MODE == kPlanar4) {
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const float4_t v = *reinterpret_cast<const float4_t*>(src + c * sc);
#pragma unroll
                    for (int p = 0; p < 4; p++) b[p * C + c] = quantize<RULE>(v[p], lo, scale);
                }
            } else {
#pragma unroll
                for (int q = 0; q < C; q++) {
                    const float4_t v = *reinterpret_cast<const float4_t*>(src + 4 * q);
#pragma unroll
                    for (int k = 0; k < 4; k++) b[4 * q + k] = quantize<RULE>(v[k], lo, scale);
                }
            }
            unsigned* d32 = reinterpret_cast<unsigned*>(dst);
#pragma unroll
            for (int q = 0; q < C; q++) d32[q] = b[4 * q] | (b[4 * q + 1] << 8) | (b[4 * q + 2] << 16) | (b[4 * q + 3] << 24);
        }
    }
}

template <int RULE, int C>
int launch_quantize(int mode, unsigned grid, hipStream_t s, const float* img, uint8_t* canvas, int N, int H, int W, int64_t sn, int64_t sc, int64_t sh,
                    int64_t sw, int gw, int cell0, float lo, float scale)
{
    if (mode == kPlanar4)     SBG_LAUNCH((quantize_tile_kernel<RULE, C, kPlanar4>), dim3(grid), dim3(256), 0, s, img, canvas, N, H, W, sn, sc, sh, sw, gw, cell0, lo, scale);
    else if (mode == kMinor4) SBG_LAUNCH((quantize_tile_kernel<RULE, C, kMinor4>), dim3(grid), dim3(256), 0, s, img, canvas, N, H, W, sn, sc, sh, sw, gw, cell0, lo, scale);
    else                      SBG_LAUNCH((quantize_tile_kernel<RULE, C, kPixel>), dim3(grid), dim3(256), 0, s, img, canvas, N, H, W, sn, sc, sh, sw, gw, cell0, lo, scale);
    return SBG_OK;
}

// One work-item per element (or float4) of out [M = R * Cn, L, D]: pick the source row by the layer's mask, then w_avg + (w - w_avg) * psi in
// that order, three rounded operations.  An index outside [0, S) is not dereferenced; its output is NaN.
template <int VEC>
__global__ __launch_bounds__(256) void truncate_mix_kernel(const float* __restrict__ w, const float* __restrict__ w_avg, float psi,
                                                           const int* __restrict__ rows, const int* __restrict__ cols, const int* __restrict__ mask,
                                                           float* __restrict__ out, int S, int L, int D, int M, int Cn)
{
#pragma clang fp contract(off)
    const int DV = D / VEC;
    const int64_t total = (int64_t)M * L * DV;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int d = (int)(i % DV) * VEC;
        const int l = (int)((i / DV) % L);
        const int m = (int)(i / ((int64_t)DV * L));
        const int r = m / Cn, c = m - r * Cn;
        const int src = mask[l] ? cols[c] : rows[r];
        const bool ok = src >= 0 && src < S;
        const float* pw = w + ((int64_t)(ok ? src : 0) * L + l) * D + d;
        float* po = out + ((int64_t)m * L + l) * D + d;
        if (VEC == 4) {
            const float4_t a = *reinterpret_cast<const float4_t*>(w_avg + d);
            const float4_t v = *reinterpret_cast<const float4_t*>(pw);
            float4_t o;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                float t = v[k] - a[k];
                t = t * psi;
                o[k] = ok ? a[k] + t : __builtin_nanf("");
            }
            *reinterpret_cast<float4_t*>(po) = o;
        } else {
            float t = pw[0] - w_avg[d];
            t = t * psi;
            po[0] = ok ? w_avg[d] + t : __builtin_nanf("");
        }
    }
}

} // namespace

extern "C" int sbg_img_quantize_tile(const float* img, uint8_t* canvas, int N, int C, int H, int W, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                                     int gw, int gh, int cell0, int rule, float lo, float scale, sbg_stream_t stream)
{
    SBG_CHECK(img && canvas, "img_quantize_tile: null pointer");
    SBG_CHECK(C == 1 || C == 3, "img_quantize_tile: C must be 1 or 3, got %d", C);
    SBG_CHECK(N >= 1 && H >= 1 && W >= 1 && gw >= 1 && gh >= 1, "img_quantize_tile: bad sizes N=%d H=%d W=%d grid=%dx%d", N, H, W, gw, gh);
    SBG_CHECK(sn >= 0 && sc >= 0 && sh >= 0 && sw >= 0, "img_quantize_tile: negative stride");
    SBG_CHECK(cell0 >= 0 && (int64_t)cell0 + N <= (int64_t)gw * gh, "img_quantize_tile: cells [%d, %lld) outside the %dx%d grid", cell0,
              (long long)cell0 + N, gw, gh);
    SBG_CHECK((int64_t)gw * W <= (1 << 30) && (int64_t)gh * H <= (1 << 30), "img_quantize_tile: canvas too large");
    SBG_CHECK(rule == SBG_QUANT_GRID || rule == SBG_QUANT_CLAMP, "img_quantize_tile: unknown rule %d", rule);
    hipStream_t s = (hipStream_t)stream;
    // four pixels per work-item: whole groups per row, 16-byte aligned loads, 4-byte aligned stores (4 * C bytes per group from an aligned base)
    const bool rows16 = W % 4 == 0 && sbg_aligned16(img) && sn % 4 == 0 && sh % 4 == 0 && sbg_aligned(canvas, 4);
    int mode = kPixel;
    if (rows16 && sw == 1 && (C == 1 || sc % 4 == 0)) mode = kPlanar4;
    else if (rows16 && C == 3 && sc == 1 && sw == 3) mode = kMinor4;
    const int64_t items = (int64_t)N * H * (mode == kPixel ? W : W / 4);
    const unsigned grid = sbg_stream_grid(items, 256);
    SbgProfScope prof(s, SBG_K_IMAGE_EXPORT, 0.0, 5.0 * N * C * (double)H * W, {kVarQuantize, N, C, H, W, rule, mode});
    int st;
    if (rule == SBG_QUANT_GRID) st = C == 3 ? launch_quantize<SBG_QUANT_GRID, 3>(mode, grid, s, img, canvas, N, H, W, sn, sc, sh, sw, gw, cell0, lo, scale)
                                            : launch_quantize<SBG_QUANT_GRID, 1>(mode, grid, s, img, canvas, N, H, W, sn, sc, sh, sw, gw, cell0, lo, scale);
    else                        st = C == 3 ? launch_quantize<SBG_QUANT_CLAMP, 3>(mode, grid, s, img, canvas, N, H, W, sn, sc, sh, sw, gw, cell0, lo, scale)
                                            : launch_quantize<SBG_QUANT_CLAMP, 1>(mode, grid, s, img, canvas, N, H, W, sn, sc, sh, sw, gw, cell0, lo, scale);
    if (st != SBG_OK) return st;
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int sbg_ws_truncate_mix(const float* W, const float* w_avg, float psi, const int* rows, const int* cols, const int* mask, float* out,
                                   int S, int L, int D, int R, int Cn, sbg_stream_t stream)
{
    SBG_CHECK(W && w_avg && rows && cols && mask && out, "ws_truncate_mix: null pointer");
    SBG_CHECK(S >= 1 && L >= 1 && D >= 1 && R >= 1 && Cn >= 1 && (int64_t)R * Cn <= (1 << 30), "ws_truncate_mix: bad sizes S=%d L=%d D=%d R=%d Cn=%d",
              S, L, D, R, Cn);
    hipStream_t s = (hipStream_t)stream;
    const int M = R * Cn;
    const int vec4 = D % 4 == 0 && sbg_aligned16(W) && sbg_aligned16(w_avg) && sbg_aligned16(out);
    const int64_t items = (int64_t)M * L * (vec4 ? D / 4 : D);
    SbgProfScope prof(s, SBG_K_IMAGE_EXPORT, 3.0 * M * L * (double)D, 4.0 * (2.0 * M * L * (double)D + D), {kVarMix, M, L, D, vec4 ? 1 : 2});
    if (vec4) SBG_LAUNCH(truncate_mix_kernel<4>, dim3(sbg_stream_grid(items, 256)), dim3(256), 0, s, W, w_avg, psi, rows, cols, mask, out, S, L, D, M, Cn);
    else      SBG_LAUNCH(truncate_mix_kernel<1>, dim3(sbg_stream_grid(items, 256)), dim3(256), 0, s, W, w_avg, psi, rows, cols, mask, out, S, L, D, M, Cn);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}
