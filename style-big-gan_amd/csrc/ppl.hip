// ppl.hip -- the arithmetic around the generator and the detector in the perceptual-path-length sampler
// (metrics/perceptual_path_length.py:23-94 of the reference, `slerp` and `PPLSampler.forward`).  The reference spells each of these
// steps as a chain of tensor ops (norms, divides, acos / cos / sin, lerp, crop view, reshape + mean, add, multiply, repeat, subtract,
// square, sum, divide); the registered metrics run 25 000 batch-of-2 iterations of it, so the chains are launch latency.  Here:
//   endpoints:  one launch writes the [2B, ...] synthesis batch (rows 0..B-1 at t, rows B..2B-1 at t + eps), z space (slerp) or w space (lerp)
//   prep:       one pass from the synthesis output (any strides) to the detector input [2B, 3 | C, S, S] fp32 dense
//   dist:       [2B, F] -> [B] = sum_f (x[b, f] - x[B + b, f])^2 / eps^2: the shared two-launch kernel pair of sqdist.h on rows b and B + b
// Launch-log key: kind SBG_K_PPL, dims[0] = variant (0 slerp, 1 lerp, 2 prep, 3 dist), then the shape.
#include "sbg_common.h"
#include "reduce.h"
#include "sqdist.h"

namespace {

constexpr int kPplSlerp = 0, kPplLerp = 1, kPplPrep = 2, kPplDist = 3;

// One wave per output row r = side * B + b: the reference's slerp(z0[b], z1[b], t_side) with t_0 = t[b], t_1 = t[b] + eps (fp32 add, like
// `t.unsqueeze(1) + self.epsilon`).  Every norm and dot product is a lane-strided sum followed by a butterfly over the wave.
__global__ __launch_bounds__(64) void ppl_slerp_kernel(const float* __restrict__ z0, const float* __restrict__ z1, const float* __restrict__ t,
                                                       float eps, float* __restrict__ out, int B, int D)
{
    const int r = blockIdx.x, b = r % B, lane = threadIdx.x;
    const float tt = r < B ? t[b] : t[b] + eps;
    const float* pa = z0 + (int64_t)b * D;
    const float* pb = z1 + (int64_t)b * D;
    float* po = out + (int64_t)r * D;

    float sa = 0.f, sb = 0.f;
    for (int i = lane; i < D; i += 64) { const float x = pa[i], y = pb[i]; sa += x * x; sb += y * y; }
    const float na = sqrtf(wave_sum(sa)), nb = sqrtf(wave_sum(sb));
    float sd = 0.f;
    for (int i = lane; i < D; i += 64) sd += (pa[i] / na) * (pb[i] / nb);
    const float d = wave_sum(sd);                                   // a . b
    const float p = tt * acosf(d);
    float sc = 0.f;
    for (int i = lane; i < D; i += 64) { const float c = pb[i] / nb - d * (pa[i] / na); sc += c * c; }
    const float nc = sqrtf(wave_sum(sc));
    const float cp = cosf(p), sp = sinf(p);
    float so = 0.f;
    for (int i = lane; i < D; i += 64) {
        const float o = (pa[i] / na) * cp + ((pb[i] / nb - d * (pa[i] / na)) / nc) * sp;
        po[i] = o;                                                  // un-normalised; rescaled below by the same lane
        so += o * o;
    }
    const float no = sqrtf(wave_sum(so));
    for (int i = lane; i < D; i += 64) po[i] = po[i] / no;
}

// out[r, l] = lerp(w0[b, l], w1[b, l], weight_r) with torch.lerp's two branches (ATen/native/Lerp.h): the same expression, so the same
// rounding (and the same contraction) as the framework's device kernel.
__device__ __forceinline__ float torch_lerp(float s, float e, float w)
{
    return fabsf(w) < 0.5f ? s + w * (e - s) : e - (e - s) * (1.0f - w);
}

__global__ __launch_bounds__(256) void ppl_lerp_kernel(const float* __restrict__ w0, const float* __restrict__ w1, const float* __restrict__ t,
                                                       float eps, float* __restrict__ out, int B, int64_t L, int vec4)
{
    const int64_t per_row = vec4 ? L / 4 : L;
    const int64_t total = 2 * (int64_t)B * per_row;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / per_row), b = r % B;
        const int64_t j = i - (int64_t)r * per_row;
        const float w = r < B ? t[b] : t[b] + eps;
        if (vec4) {
            const float4_t s = *reinterpret_cast<const float4_t*>(w0 + (int64_t)b * L + 4 * j);
            const float4_t e = *reinterpret_cast<const float4_t*>(w1 + (int64_t)b * L + 4 * j);
            float4_t o;
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = torch_lerp(s[k], e[k], w);
            *reinterpret_cast<float4_t*>(out + (int64_t)r * L + 4 * j) = o;
        } else {
            out[(int64_t)r * L + j] = torch_lerp(w0[(int64_t)b * L + j], w1[(int64_t)b * L + j], w);
        }
    }
}

// One work-item per output pixel (n, oy, ox): for every input channel the f x f box mean of the (cropped) window, then (m + 1) * 127.5,
// written to channel c -- or to channels 0..2 when the input is grey.  Mean and scale round separately, as the reference's two ops do.
__global__ __launch_bounds__(256) void ppl_prep_kernel(const float* __restrict__ img, float* __restrict__ out, int N, int C, int Co, int y0, int x0,
                                                       int OH, int OW, int f, int64_t sn, int64_t sc, int64_t sh, int64_t sw)
{
#pragma clang fp contract(off)
    const int64_t total = (int64_t)N * OH * OW;
    const float inv = 1.0f / (float)(f * f);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int ox = (int)(i % OW);
        const int oy = (int)((i / OW) % OH);
        const int n = (int)(i / ((int64_t)OW * OH));
        const float* base = img + n * sn + (int64_t)(y0 + oy * f) * sh + (int64_t)(x0 + ox * f) * sw;
        float* ob = out + (int64_t)n * Co * OH * OW + (int64_t)oy * OW + ox;
        for (int c = 0; c < C; c++) {
            const float* p = base + c * sc;
            float m;
            if (f == 1) {
                m = p[0];
            } else {
                float s = 0.f;
                for (int dy = 0; dy < f; dy++)
                    for (int dx = 0; dx < f; dx++) s += p[dy * sh + dx * sw];
                m = s * inv;
            }
            const float v = (m + 1.0f) * 127.5f;
            if (C == 1) {
                ob[0] = v; ob[(int64_t)OH * OW] = v; ob[2 * (int64_t)OH * OW] = v;
            } else {
                ob[(int64_t)c * OH * OW] = v;
            }
        }
    }
}

} // namespace

extern "C" int sbg_ppl_slerp_endpoints(const float* z0, const float* z1, const float* t, float eps, float* out, int B, int D, sbg_stream_t stream)
{
    SBG_CHECK(z0 && z1 && t && out, "ppl_slerp_endpoints: null pointer");
    SBG_CHECK(B >= 1 && D >= 1 && B <= 32768, "ppl_slerp_endpoints: bad sizes B=%d D=%d", B, D);
    hipStream_t s = (hipStream_t)stream;
    SbgProfScope prof(s, SBG_K_PPL, 0.0, 4.0 * (4.0 * B * (double)D + B + 2.0 * B * (double)D), {kPplSlerp, B, D});
    SBG_LAUNCH(ppl_slerp_kernel, dim3((unsigned)(2 * B)), dim3(64), 0, s, z0, z1, t, eps, out, B, D);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int sbg_ppl_lerp_endpoints(const float* w0, const float* w1, const float* t, float eps, float* out, int B, int64_t L, sbg_stream_t stream)
{
    SBG_CHECK(w0 && w1 && t && out, "ppl_lerp_endpoints: null pointer");
    SBG_CHECK(B >= 1 && L >= 1, "ppl_lerp_endpoints: bad sizes B=%d L=%lld", B, (long long)L);
    hipStream_t s = (hipStream_t)stream;
    const int vec4 = (L % 4 == 0) && sbg_aligned16(w0) && sbg_aligned16(w1) && sbg_aligned16(out);
    const int64_t items = 2 * (int64_t)B * (vec4 ? L / 4 : L);
    SbgProfScope prof(s, SBG_K_PPL, 0.0, 4.0 * (4.0 * B * (double)L + B), {kPplLerp, B, (int)L, vec4});
    SBG_LAUNCH(ppl_lerp_kernel, dim3(sbg_stream_grid(items, 256)), dim3(256), 0, s, w0, w1, t, eps, out, B, L, vec4);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int sbg_ppl_prep_images(const float* img, float* out, int N, int C, int H, int W, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                                   int crop, int factor, sbg_stream_t stream)
{
    SBG_CHECK(img && out, "ppl_prep_images: null pointer");
    SBG_CHECK(N >= 1 && C >= 1 && H >= 1 && W >= 1 && factor >= 1, "ppl_prep_images: bad sizes N=%d C=%d H=%d W=%d factor=%d", N, C, H, W, factor);
    SBG_CHECK(!crop || H == W, "ppl_prep_images: the centre crop needs a square image (H=%d W=%d)", H, W);
    const int c8 = H / 8;
    const int y0 = crop ? 3 * c8 : 0, x0 = crop ? 2 * c8 : 0;
    const int hh = crop ? 4 * c8 : H, ww = crop ? 4 * c8 : W;
    SBG_CHECK(hh >= factor && ww >= factor && hh % factor == 0 && ww % factor == 0,
              "ppl_prep_images: the %dx%d window does not split into %dx%d boxes", hh, ww, factor, factor);
    const int OH = hh / factor, OW = ww / factor, Co = C == 1 ? 3 : C;
    hipStream_t s = (hipStream_t)stream;
    const int64_t items = (int64_t)N * OH * OW;
    SbgProfScope prof(s, SBG_K_PPL, 0.0, 4.0 * ((double)N * C * hh * ww + (double)N * Co * OH * OW), {kPplPrep, N, C, H, crop, factor});
    SBG_LAUNCH(ppl_prep_kernel, dim3(sbg_stream_grid(items, 256)), dim3(256), 0, s, img, out, N, C, Co, y0, x0, OH, OW, factor, sn, sc, sh, sw);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int64_t sbg_ppl_dist_workspace(int B, int64_t F)
{
    if (B < 1 || F < 1) return -1;
    return (int64_t)B * dist_chunks(F) * (int64_t)sizeof(float);
}

extern "C" int sbg_ppl_dist(const float* feats, float* dist, void* workspace, int B, int64_t F, float eps2, sbg_stream_t stream)
{
    SBG_CHECK(feats && dist && workspace, "ppl_dist: null pointer");
    SBG_CHECK(B >= 1 && B <= 65535 && F >= 1, "ppl_dist: bad sizes B=%d F=%lld", B, (long long)F);
    const int64_t nchunk = dist_chunks(F);
    SBG_CHECK(nchunk <= (1 << 30), "ppl_dist: F=%lld too large", (long long)F);
    hipStream_t s = (hipStream_t)stream;
    const int vec4 = (F % 4 == 0) && sbg_aligned16(feats);
    SbgProfScope prof(s, SBG_K_PPL, 3.0 * B * (double)F, 4.0 * (2.0 * B * (double)F + 2.0 * B * nchunk + B), {kPplDist, B, (int)(F >> 10), (int)(F & 1023), vec4});
    SBG_LAUNCH(sqdist_partial_kernel<true>, dim3((unsigned)nchunk, (unsigned)B), dim3(kDistThreads), 0, s, feats, feats + (int64_t)B * F, (float*)workspace,
               F, (int)nchunk, vec4);
    return merge_partials<float>((const float*)workspace, dist, B, (int)nchunk, eps2, s);
}
