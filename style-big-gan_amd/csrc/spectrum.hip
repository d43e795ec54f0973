// spectrum.hip -- the average 2-D power spectrum of an image set (avg_spectra.py; Karras et al., "Alias-Free Generative Adversarial
// Networks", NeurIPS 2021, appendix: avg_spectra.py of their code).  fp32 transforms, a float64 power accumulator.
//
// Sizes: R image side, a power of two in [16, 1024]; S = P R the spectrum side, P in {1, 2, 4}; BC image-channels of one call.
// Per image-channel, x the pixel (uint8 or fp32):  v = fmaf(x, s, t);  a[y, x] = v * window[x];  row transform of length S (imaginary part 0,
// samples >= R zero), kx = 0 .. S/2 kept;  c[y, kx] = A[y, kx] * window[y] (both components);  column transform of length S;
// p[ky, kx] = (double)re (double)re + (double)im (double)im;  acc[kx, ky] += p, image-channels in ascending order.
// The 1-D transform is the radix-2 decimation-in-time value graph: bit-reversed input, stages of half-span h = 1, 2, .., S/2; the butterfly of
// a = z[i], b = z[i + h] with W = twiddle[j S / (2 h)], j = i mod h:
//     t_re = fmaf(b_re, w_re, -(b_im * w_im)),  t_im = fmaf(b_re, w_im, b_im * w_re),  z[i] = a + t,  z[i + h] = a - t,
// every plain product and sum rounded on its own: the pragma below keeps the compiler from contracting them (the _rn intrinsics do not on
// this toolchain), and what the definition fuses is written as fmaf.  torch_utils/ops/spectrum.py states the same graph in numpy for CPU
// tensors; both devices give the same bits.
// Schedule (it changes no value but the sign of a zero, which the power does not see):
//  * in-place stages in LDS, element i of a line stored at i ^ (31 when bit 5 of i is set): the a and b reads of the stages h < 32, which
//    otherwise put lanes l and l + 16 of a 32-lane group on one 8-byte bank, become conflict-free, and the stages h >= 32 stay so;
//  * the zero padding is never transformed: the non-zero samples sit at the bit-reversed positions that are multiples of P, the stages
//    h < P only add and subtract products with zero, so a line starts as every sample P times and the stages start at h = P;
//  * the twiddles come as one stage-major table, entry h - 1 + j = twiddle[j S / (2 h)], so a stage reads consecutive entries.
// rows: a workgroup owns RW = G x passes rows of one image-channel: G lines transformed side by side in LDS, one or two passes, the kept half
//  of an earlier pass parked in LDS, so that the store of one kx is RW consecutive float2.  The intermediate is [BC, S/2 + 1, R] with the R
//  axis in BIT-REVERSED row order (entry q holds row bitrev(q)): the column pass reads a column as R consecutive values that are already in
//  the order its first stage wants; the workgroup of rows q0 .. q0 + RW - 1 reads the image rows bitrev(q).
// cols: one workgroup per kx.  Lane t holds acc[kx, t + i NT] in registers over the whole loop over the image-channels (ascending: one
//  sequential float64 chain per entry, no atomics), stores the row once.  The next column is fetched while the current one is transformed.
// Launch-log key: kind SBG_K_SPECTRUM, dims = {0 rows | 1 cols, BC, R, S}.
#pragma clang fp contract(off)
#include "sbg_common.h"

namespace {

constexpr int kRows = 0, kCols = 1;
constexpr int NT = 256;
constexpr int kMaxOwn = 16;             // accumulator entries per lane of the column pass: 4096 / 256
constexpr int kMaxCol = 4;              // column samples per lane: 1024 / 256

__device__ __forceinline__ int sw(int i) { return i ^ (-((i >> 5) & 1) & 31); }
__device__ __forceinline__ int bitrev(int v, int bits) { return (int)(__brev((unsigned)v) >> (32 - bits)); }

// the stages h0, 2 h0, .., S/2 of `lines` lines of S complex values at `pitch`, all work-items of the workgroup; ends behind a barrier
__device__ __forceinline__ void fft_stages(float2* buf, const float2* __restrict__ tw, int S, int logS, int h0, int lines, int pitch, int tid, int nt)
{
    const int half = S >> 1, total = lines * half;
    for (int h = h0; h < S; h <<= 1) {
        __syncthreads();
        const float2* w_h = tw + (h - 1);
        for (int k = tid; k < total; k += nt) {
            const int line = k >> (logS - 1), kk = k & (half - 1);
            const int j = kk & (h - 1), i = ((kk - j) << 1) + j;
            float2* z = buf + line * pitch;
            const float2 a = z[sw(i)], b = z[sw(i + h)], w = w_h[j];
            const float pr = b.y * w.y, pi = b.y * w.x;
            const float tr = fmaf(b.x, w.x, -pr), ti = fmaf(b.x, w.y, pi);
            z[sw(i)] = make_float2(a.x + tr, a.y + ti);
            z[sw(i + h)] = make_float2(a.x - tr, a.y - ti);
        }
    }
    __syncthreads();
}

struct RowPlan { int G, passes, pad; };
inline RowPlan row_plan(int S)
{
    RowPlan p;
    p.G = 4096 / S < 1 ? 1 : (4096 / S > 16 ? 16 : 4096 / S);      // lines side by side: at most 32 KB
    p.passes = S >= 1024 ? 2 : 1;
    p.pad = p.G > 1 ? 32 / p.G : 0;         // the G lines of one kx on different banks for the final read
    return p;
}
inline size_t row_lds(int S) { const RowPlan p = row_plan(S); return 8 * ((size_t)p.G * (S + p.pad) + (size_t)(p.passes - 1) * p.G * (S / 2 + 1)); }

template <class T>
__global__ __launch_bounds__(NT) void spectrum_rows_kernel(const T* __restrict__ x, const float* __restrict__ window, const float2* __restrict__ tw,
                                                           float2* __restrict__ ws, float s, float t, int R, int logR, int S, int logS, int G, int passes, int pad)
{
    extern __shared__ float2 spectrum_lds[];
    const int tid = threadIdx.x, half = S >> 1, logP = logS - logR, P = 1 << logP;
    const int pitch = S + pad, RW = G * passes, groups = R / RW;
    float2* buf = spectrum_lds;
    float2* stash = spectrum_lds + G * pitch;               // the kept half of the rows of the earlier passes, pitch S/2 + 1
    const int64_t bc = blockIdx.x / groups;
    const int q0 = (int)(blockIdx.x % groups) * RW;
    const T* img = x + bc * R * R;

    for (int p = 0; p < passes; p++) {
        for (int idx = tid; idx < G * R; idx += NT) {       // line gl, position block qx: sample n = bitrev(qx) of row bitrev(q0 + p G + gl)
            const int gl = idx >> logR, qx = idx & (R - 1);
            const int n = bitrev(qx, logR), y = bitrev(q0 + p * G + gl, logR);
            const float v = fmaf(sbg_pixel(img[(int64_t)y * R + n]), s, t);
            const float2 a = make_float2(v * window[n], 0.f);
            for (int r = 0; r < P; r++) buf[gl * pitch + sw((qx << logP) + r)] = a;
        }
        fft_stages(buf, tw, S, logS, P, G, pitch, tid, NT);
        if (p + 1 < passes) {
            for (int idx = tid; idx < G * (half + 1); idx += NT) {
                const int gl = idx / (half + 1), kx = idx - gl * (half + 1);
                stash[(p * G + gl) * (half + 1) + kx] = buf[gl * pitch + sw(kx)];
            }
            __syncthreads();                                // the lines are free for the next pass
        }
    }
    const int parked = (passes - 1) * G;
    float2* out = ws + bc * (half + 1) * R + q0;
    for (int idx = tid; idx < (half + 1) * RW; idx += NT) { // RW consecutive float2 per kx
        const int l = idx & (RW - 1), kx = idx / RW;
        out[(int64_t)kx * R + l] = l < parked ? stash[l * (half + 1) + kx] : buf[(l - parked) * pitch + sw(kx)];
    }
}

__global__ __launch_bounds__(NT) void spectrum_cols_kernel(const float2* __restrict__ ws, const float* __restrict__ window, const float2* __restrict__ tw,
                                                           double* __restrict__ acc, int BC, int R, int logR, int S, int logS)
{
    extern __shared__ float2 spectrum_lds[];
    const int tid = threadIdx.x, nt = blockDim.x, half = S >> 1, logP = logS - logR, P = 1 << logP;
    const int kx = blockIdx.x;
    double* arow = acc + (int64_t)kx * S;
    double own[kMaxOwn];
#pragma unroll
    for (int i = 0; i < kMaxOwn; i++) { const int ky = tid + i * nt; own[i] = ky < S ? arow[ky] : 0.0; }
    float wq[kMaxCol];
    float2 cur[kMaxCol], nxt[kMaxCol];
    const float2* col = ws + (int64_t)kx * R;               // + bc (S/2 + 1) R
    const int64_t step = (int64_t)(half + 1) * R;
#pragma unroll
    for (int i = 0; i < kMaxCol; i++) {
        const int q = tid + i * nt;
        wq[i] = q < R ? window[bitrev(q, logR)] : 0.f;
        cur[i] = q < R ? col[q] : make_float2(0.f, 0.f);
        nxt[i] = make_float2(0.f, 0.f);
    }
    for (int bc = 0; bc < BC; bc++) {
#pragma unroll
        for (int i = 0; i < kMaxCol; i++) {
            const int q = tid + i * nt;
            if (q < R) {
                const float2 c = make_float2(cur[i].x * wq[i], cur[i].y * wq[i]);
                for (int r = 0; r < P; r++) spectrum_lds[sw((q << logP) + r)] = c;
            }
        }
        if (bc + 1 < BC) {
#pragma unroll
            for (int i = 0; i < kMaxCol; i++) { const int q = tid + i * nt; if (q < R) nxt[i] = col[(bc + 1) * step + q]; }
        }
        fft_stages(spectrum_lds, tw, S, logS, P, 1, S, tid, nt);
#pragma unroll
        for (int i = 0; i < kMaxOwn; i++) {
            const int ky = tid + i * nt;
            if (ky < S) { const float2 z = spectrum_lds[sw(ky)]; own[i] += (double)z.x * (double)z.x + (double)z.y * (double)z.y; }
        }
        __syncthreads();                                    // the line is read: the next column may overwrite it
#pragma unroll
        for (int i = 0; i < kMaxCol; i++) cur[i] = nxt[i];
    }
#pragma unroll
    for (int i = 0; i < kMaxOwn; i++) { const int ky = tid + i * nt; if (ky < S) arow[ky] = own[i]; }
}

inline int log2i(int v) { int l = 0; while ((1 << l) < v) l++; return l; }
inline bool sizes_ok(int R, int S)
{
    if (R < 16 || R > 1024 || (R & (R - 1))) return false;
    return S == R || S == 2 * R || S == 4 * R;
}
inline int cols_nt(int S) { return S / 2 < 64 ? 64 : (S / 2 > NT ? NT : S / 2); }

} // namespace

extern "C" int64_t sbg_spectrum_workspace(int64_t BC, int R, int S)
{
    if (BC < 1 || !sizes_ok(R, S)) return -1;
    const RowPlan p = row_plan(S);
    if (BC * (R / (p.G * p.passes)) > INT32_MAX) return -1;             // the row pass's grid
    return 8 * BC * (S / 2 + 1) * R;
}

extern "C" int sbg_spectrum_rows(const void* images, int is_u8, const float* window, const float* stages, float s, float t, void* workspace,
                                 int64_t BC, int R, int S, sbg_stream_t stream)
{
    SBG_CHECK(sbg_spectrum_workspace(BC, R, S) >= 0, "spectrum_rows: bad sizes BC=%lld R=%d S=%d (R a power of two in [16, 1024], S = R, 2 R or 4 R)",
              (long long)BC, R, S);
    SBG_CHECK(images && window && stages && workspace && sbg_aligned(images, is_u8 ? 1 : 4) && sbg_aligned(window, 4) && sbg_aligned(stages, 8) && sbg_aligned(workspace, 8),
              "spectrum_rows: null or misaligned pointer");
    const RowPlan p = row_plan(S);
    const size_t lds = row_lds(S);
    SBG_CHECK(lds < 64 * 1024, "spectrum_rows: %zu bytes of LDS for S=%d", lds, S);
    const int64_t grid = BC * (R / (p.G * p.passes));
    hipStream_t st = (hipStream_t)stream;
    const double px = (double)BC * R * R;
    SbgProfScope prof(st, SBG_K_SPECTRUM, 5.0 * px * S / R * log2i(S), (is_u8 ? 1.0 : 4.0) * px + 8.0 * (double)BC * (S / 2 + 1) * R,
                      {kRows, sbg_clip31(BC), R, S});
    if (is_u8)
        SBG_LAUNCH(spectrum_rows_kernel<unsigned char>, dim3((unsigned)grid), dim3(NT), lds, st, (const unsigned char*)images, window, (const float2*)stages,
                   (float2*)workspace, s, t, R, log2i(R), S, log2i(S), p.G, p.passes, p.pad);
    else
        SBG_LAUNCH(spectrum_rows_kernel<float>, dim3((unsigned)grid), dim3(NT), lds, st, (const float*)images, window, (const float2*)stages,
                   (float2*)workspace, s, t, R, log2i(R), S, log2i(S), p.G, p.passes, p.pad);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int sbg_spectrum_cols(const void* workspace, const float* window, const float* stages, double* acc, int64_t BC, int R, int S, sbg_stream_t stream)
{
    SBG_CHECK(sbg_spectrum_workspace(BC, R, S) >= 0, "spectrum_cols: bad sizes BC=%lld R=%d S=%d (R a power of two in [16, 1024], S = R, 2 R or 4 R)",
              (long long)BC, R, S);
    SBG_CHECK(workspace && window && stages && acc && sbg_aligned(workspace, 8) && sbg_aligned(window, 4) && sbg_aligned(stages, 8) && sbg_aligned(acc, 8),
              "spectrum_cols: null or misaligned pointer");
    static_assert(kMaxOwn * NT >= 4096 && kMaxCol * NT >= 1024, "a lane's registers hold the largest line");
    const int nt = cols_nt(S);
    SBG_CHECK(kMaxOwn * nt >= S && kMaxCol * nt >= R, "spectrum_cols: S=%d R=%d do not fit %d work-items", S, R, nt);
    hipStream_t st = (hipStream_t)stream;
    const double lines = (double)BC * (S / 2 + 1);
    SbgProfScope prof(st, SBG_K_SPECTRUM, 5.0 * lines * S * log2i(S), 8.0 * lines * R + 16.0 * (S / 2 + 1) * S,
                      {kCols, sbg_clip31(BC), R, S});
    SBG_LAUNCH(spectrum_cols_kernel, dim3((unsigned)(S / 2 + 1)), dim3(nt), (size_t)8 * S, st, (const float2*)workspace, window, (const float2*)stages, acc,
               (int)BC, R, log2i(R), S, log2i(S));
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}
