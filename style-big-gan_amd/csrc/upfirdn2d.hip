// upfirdn2d.hip -- pad -> zero-insert upsample -> 2-D FIR -> decimate, any up/down/pad/filter/strides.
//
// Semantics: stylegan2ada/torch_utils/ops/upfirdn2d.py:120-208 (`upfirdn2d`, `_upfirdn2d_ref`) and the output-size
// rule of upfirdn2d.cpp:32-33.  Per axis, with u the zero-inserted + padded signal,
//     y[o] = gain * sum_k u[o*down + k] * g[k],   g = f (flip_filter) or reversed f (default: true convolution)
// and u[X] is x[(X - pad0) / up] when (X - pad0) is a non-negative multiple of `up` inside the input, else 0; so only
// taps k == (pad0 - o*down) mod up contribute and the kernels below visit exactly those (no multiplies by inserted zeros).
//
// gfx950 design: HBM-bound streaming op (algorithmic bytes = (numel_in + numel_out) * sizeof(T)).
//  * channel-minor activations (the layout the conv kernels produce): one lane = 8 channels (16 B) of one output pixel,
//    consecutive lanes walk channels then x, so every tap is a fully coalesced 16-B-per-lane load and the 4x4 / 2x2
//    effective footprint is re-used out of L1/L2 (each input line is touched by <= fh*fw/(up*up) neighbouring lanes).
//  * planar (NCHW) activations: one lane = one output pixel of one channel, lanes walk x (coalesced along rows).
//  * the filter lives in LDS (<= 1024 taps) and is read with wave-uniform addresses (broadcast, conflict-free).
// Three kernels, most general first, and one dispatch (launch_upfirdn):
//   upfirdn2d_kernel<T,VEC>            any configuration; 8 channels per lane on channel-minor tensors, else one element
//   upfirdn2d_fir_kernel<T,FH,FW>      up == down == 1, channel-minor: register-blocked patch per lane; 4 x 4 at compile time or any size up to 8 x 8
//   upfirdn2d_fir_slide_kernel<T,BT>   the 4 x 4 low-pass on the matrix cores with the fused forward / backward tails; fir_mfma_accepts() is the one
//                                      statement of which launches it takes, asked by the dispatch, both probe entry points and the entry point's checks
#include "sbg_common.h"
#include "lds_asm.h"
#include <cstdlib>

namespace {

struct UpfirdnArgs {
    const void* x; const float* f; void* y;
    int upx, upy, downx, downy, padx0, pady0, flip; float gain;
    int inW, inH, C, N; int64_t isx, isy, isc, isn;
    int fw, fh, fsx, fsy;
    int outW, outH; int64_t osx, osy, osc, osn;
    int64_t total;    // number of lane work items
    // fused tail (matrix-core FIR only): y = clamp(act(fir * gain * oscale[n, c] + noise[n, pixel] + bias[c]) * act_gain)
    const float* oscale; const float* noise; int64_t noise_sn; const float* bias;
    int tail; float alpha, act_gain, clamp;
    // backward tail (sliding-window matrix-core FIR only; tail == 2): the result is the gradient w.r.t. the OUTPUT y of a bias_act (`dact_y`, saved,
    // same geometry as this launch's output); the kernel multiplies by the activation's slope at y -- dact_gpos for y > 0, dact_gneg below, zero on the
    // clamp rails |y| >= dact_rail -- and adds up the result per channel (the bias gradient): dact_part[workgroup][64]
    const void* dact_y; float* dact_part; float dact_gpos, dact_gneg, dact_rail;
    const float* post;      // forward tail only: the finished value is multiplied by post[n, c] (the style modulation of the layer that reads it next)
};

#define SBG_UPFIRDN_MAX_LDS_TAPS 1024

static __device__ __forceinline__ int pos_mod(int a, int m) { int r = a % m; return r < 0 ? r + m : r; }

template <class T, int VEC>
__global__ __launch_bounds__(256) void upfirdn2d_kernel(UpfirdnArgs p)
{
    __shared__ float sf[SBG_UPFIRDN_MAX_LDS_TAPS];
    const int ntaps = p.fw * p.fh;
    const bool f_lds = ntaps <= SBG_UPFIRDN_MAX_LDS_TAPS;
    if (f_lds) {
        // stage the filter in visiting order: sf[ky*fw + kx] multiplies u[.. + ky][.. + kx]
        for (int t = threadIdx.x; t < ntaps; t += blockDim.x) {
            int ky = t / p.fw, kx = t - ky * p.fw;
            int fy = p.flip ? ky : p.fh - 1 - ky, fx = p.flip ? kx : p.fw - 1 - kx;
            sf[t] = p.f[fy * p.fsy + fx * p.fsx];
        }
        __syncthreads();
    }
    const T* px = (const T*)p.x; T* py = (T*)p.y;
    const int cvecs = (VEC == 8) ? (p.C >> 3) : p.C;
    const bool cminor = (VEC == 8) || (p.isc == 1 && p.C > 1);
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        // decompose the work item: channel-minor -> (c fastest, then x, y, n); planar -> (x fastest, then y, c, n)
        int c, ox, oy, n;
        int64_t r = idx;
        if (cminor) { c = (int)(r % cvecs); r /= cvecs; ox = (int)(r % p.outW); r /= p.outW; oy = (int)(r % p.outH); n = (int)(r / p.outH); }
        else        { ox = (int)(r % p.outW); r /= p.outW; oy = (int)(r % p.outH); r /= p.outH; c = (int)(r % cvecs); n = (int)(r / cvecs); }
        if (VEC == 8) c <<= 3;

        const int baseX = ox * p.downx - p.padx0, baseY = oy * p.downy - p.pady0;   // u-coordinate of tap 0, in input*up units
        const int kx0 = pos_mod(-baseX, p.upx), ky0 = pos_mod(-baseY, p.upy);
        float acc[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++) acc[j] = 0.f;
        const T* xin = px + n * p.isn + c * p.isc;
        for (int ky = ky0; ky < p.fh; ky += p.upy) {
            const int iy = (baseY + ky) / p.upy;       // exact: (baseY + ky) is a multiple of upy
            if (iy < 0 || iy >= p.inH) continue;
            for (int kx = kx0; kx < p.fw; kx += p.upx) {
                const int ix = (baseX + kx) / p.upx;
                if (ix < 0 || ix >= p.inW) continue;
                float fv;
                if (f_lds) fv = sf[ky * p.fw + kx];
                else { int fy = p.flip ? ky : p.fh - 1 - ky, fx = p.flip ? kx : p.fw - 1 - kx; fv = p.f[fy * p.fsy + fx * p.fsx]; }
                const T* src = xin + iy * p.isy + ix * p.isx;
                if (VEC == 8) {
                    float v[8];
                    Vec8<T>::ld(src, v);
#pragma unroll
                    for (int j = 0; j < 8; j++) acc[j] += v[j] * fv;
                } else {
                    acc[0] += Elem<T>::ld(src) * fv;
                }
            }
        }
        T* dst = py + n * p.osn + c * p.osc + oy * p.osy + ox * p.osx;
        if (VEC == 8) {
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; j++) o[j] = acc[j] * p.gain;
            Vec8<T>::st(dst, o);
        } else {
            Elem<T>::st(dst, acc[0] * p.gain);
        }
    }
}


// Register-blocked FIR for the hot case: up == down == 1 (the 4x4 low-pass after every transposed / before every strided
// convolution, and their gradients), channel-minor, 8 channels per lane.  Each lane produces a TY x TX patch of output
// pixels from a (TY + fh - 1) x (TX + fw - 1) input window held in registers: for the 4x4 filter that is 35 16-B loads per 8
// outputs (4.4 per output instead of 16; an 8-wide patch measured slower), every load 256-B-contiguous across the 16 lanes that share a pixel.
// FH x FW is the filter size at compile time (4 x 4: the [1, 3, 3, 1] low-pass of every up / down layer) -- the window loops unroll, the
// taps live in registers and the tap-range tests fold away -- or 0 x 0 for any size up to FIR_MAXF read from p.fh / p.fw, taps in LDS.
// The bounds tests stay branches around each load, which also keeps the loads in program order (bounded live set).
#define FIR_TX 4
#define FIR_TY 2
#define FIR_MAXF 8
template <class T, int FH, int FW>
__global__ __launch_bounds__(256) void upfirdn2d_fir_kernel(UpfirdnArgs p, int xblocks, int yblocks)
{
    constexpr bool FIXED = FH > 0;
    constexpr int UNROLL_Y = FIXED ? FIR_TY + FH - 1 : 1, UNROLL_X = FIXED ? FIR_TX + FW - 1 : 1;        // 1 = leave the run-time loops rolled
    const int fh = FIXED ? FH : p.fh, fw = FIXED ? FW : p.fw;
    // taps in visiting order, gain folded in: [ky][kx] multiplies the window pixel (.. + ky, .. + kx)
    __shared__ float sf[FIR_MAXF * FIR_MAXF];
    float fv[FIXED ? FH : 1][FIXED ? FW : 1];
    if constexpr (FIXED) {
#pragma unroll
        for (int ky = 0; ky < FH; ky++)
#pragma unroll
            for (int kx = 0; kx < FW; kx++) {
                const int fy = p.flip ? ky : FH - 1 - ky, fx = p.flip ? kx : FW - 1 - kx;
                fv[ky][kx] = p.f[fy * p.fsy + fx * p.fsx] * p.gain;
            }
    } else {
        const int ntaps = p.fw * p.fh;
        for (int t = threadIdx.x; t < ntaps; t += blockDim.x) {
            int ky = t / p.fw, kx = t - ky * p.fw;
            int fy = p.flip ? ky : p.fh - 1 - ky, fx = p.flip ? kx : p.fw - 1 - kx;
            sf[t] = p.f[fy * p.fsy + fx * p.fsx] * p.gain;
        }
        __syncthreads();
    }
    auto tap = [&](int ky, int kx) { if constexpr (FIXED) return fv[ky][kx]; else return sf[ky * fw + kx]; };
    const T* px = (const T*)p.x; T* py = (T*)p.y;
    const int cvecs = p.C >> 3;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += step) {
        int64_t r = idx;
        const int c = (int)(r % cvecs) << 3; r /= cvecs;
        const int xb = (int)(r % xblocks); r /= xblocks;
        const int yb = (int)(r % yblocks); const int n = (int)(r / yblocks);
        const int ox0 = xb * FIR_TX, oy0 = yb * FIR_TY;
        float acc[FIR_TY][FIR_TX][8];
#pragma unroll
        for (int a = 0; a < FIR_TY; a++)
#pragma unroll
            for (int b = 0; b < FIR_TX; b++)
#pragma unroll
                for (int e = 0; e < 8; e++) acc[a][b][e] = 0.f;
        const T* xin = px + n * p.isn + c;
#pragma unroll UNROLL_Y
        for (int wy = 0; wy < FIR_TY + fh - 1; wy++) {           // input window rows
            const int iy = oy0 + wy - p.pady0;
            if ((unsigned)iy >= (unsigned)p.inH) continue;
#pragma unroll UNROLL_X
            for (int wx = 0; wx < FIR_TX + fw - 1; wx++) {
                const int ix = ox0 + wx - p.padx0;
                if ((unsigned)ix >= (unsigned)p.inW) continue;
                float v[8];
                Vec8<T>::ld(xin + iy * p.isy + ix * p.isx, v);
#pragma unroll
                for (int a = 0; a < FIR_TY; a++) {
                    const int ky = wy - a;
                    if (ky < 0 || ky >= fh) continue;
#pragma unroll
                    for (int b = 0; b < FIR_TX; b++) {
                        const int kx = wx - b;
                        if (kx < 0 || kx >= fw) continue;
#pragma unroll
                        for (int e = 0; e < 8; e++) acc[a][b][e] += v[e] * tap(ky, kx);
                    }
                }
            }
        }
#pragma unroll
        for (int a = 0; a < FIR_TY; a++) {
            const int oy = oy0 + a;
            if (oy >= p.outH) continue;
#pragma unroll
            for (int b = 0; b < FIR_TX; b++) {
                const int ox = ox0 + b;
                if (ox >= p.outW) continue;
                Vec8<T>::st(py + n * p.osn + c + oy * p.osy + ox * p.osx, acc[a][b]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Matrix-core FIR for the hot case (up == down == 1, 4 x 4 taps, 16-bit channel-minor tensors, C % 64 == 0, taps exactly
// representable in the tensor dtype: fir_mfma_accepts() below is the whole rule).  The register-blocked kernel above is VALU-bound
// (16 fp32 FMAs + unpacking per output element: 2.5 TB/s); here a row of 16 output pixels x 16 channels is ONE accumulator tile,
//     D[c][ox] += sum_ix  In[iy = oy + ky][ix][c] * T_ky[ix][ox],      T_ky[ix][ox] = f[ky][ix - ox]  (Toeplitz, 32 x 16)
// i.e. four v_mfma_f32_16x16x32 per tile (one per filter row, ky = 0..3 in that order into a cleared fp32 accumulator), 0.4 % of the
// chip's matrix rate, and the VALU only converts and stores.  The input window of 32 output columns x 64 channels (40 pixels per row) is
// staged by LDS-DMA in whole 128-B lines; the A operand (channel x 32 consecutive pixels) is read with the transposing ds_read_b64_tr_b16.
// Zero-padding = out-of-range DMA offsets; LDS pixels 40..47 of each row are only ever multiplied by zero taps and are
// cleared once so that they stay finite.  `gain` is applied in fp32 on the accumulator.
typedef __attribute__((address_space(3))) void* fir_lds_ptr;
typedef __attribute__((address_space(3))) short4_t* fir_lds_s4_ptr;
#define SBG_FIR_OOB 0x80000000u

template <class T> struct FirMfma;
template <> struct FirMfma<bf16_s> {
    static __device__ __forceinline__ float4_t run(short8_t a, short8_t b, float4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ short bits(float v) { return (short)f32_to_bf16_bits(v); }
    static __device__ __forceinline__ float from_bits(unsigned short b) { return bf16_bits_to_f32(b); }
};
template <> struct FirMfma<f16_s> {
    static __device__ __forceinline__ float4_t run(short8_t a, short8_t b, float4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ short bits(float v) { return (short)f32_to_f16_bits(v); }
    static __device__ __forceinline__ float from_bits(unsigned short b) { return f16_bits_to_f32(b); }
};

// The kernel is a sliding window: a workgroup owns a strip of 32 output columns x 64 channels and WALKS DOWN it, four output rows per
// step (one per wave; rows past the segment are masked DMA offsets and masked stores, so any height runs).  The window rows live in a
// 12-row ring in LDS (row r of the strip's window in slot r % 12); a step needs the seven rows [4s, 4s + 7), of which only the last four
// are new, and those are fetched by LDS-DMA one step ahead while the matrix cores work on the current rows.  The vertical overlap is read
// once per strip segment and the horizontal one is 35 / 32 (a kernel of independent 8 x 32 tiles, retired, re-read three of every eleven
// window rows: 1.72x the input bytes), and the loads of step s + 1, the MFMAs of step s and the stores of step s - 1 are in flight
// together (two workgroups per CU: 72 KB of LDS each).
// Order inside a step: issue the prefetch -> compute from LDS -> wait for the prefetch (the stores of the previous step, issued a whole step
// ago, have drained by then) -> barrier (every wave is done with the rows the NEXT prefetch overwrites, and sees the new rows) -> store.
// BT (backward tail): see UpfirdnArgs::dact_y -- the transposed low-pass in the backward of `bias_act -> low-pass` (D's conv0 -> the filter in front of the
// strided conv1) hands its result straight to the activation gradient, so the gradient w.r.t. the activation's output is never written or re-read.
template <class T, bool BT>
__global__ __launch_bounds__(256, 2) void upfirdn2d_fir_slide_kernel(UpfirdnArgs p, unsigned x_bytes, int tiles_x, int cblocks, int ysegs, int seg_rows)
{
    constexpr int TX = 32, FH = 4, FW = 4, SR = 4;      // SR = output rows per step (one per wave)
    constexpr int RING = 12, WXL = 48, PPR = 5;
    extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int b = blockIdx.x;
    const int cb0 = b % cblocks; b /= cblocks;
    const int tx = b % tiles_x; b /= tiles_x;
    const int ys = b % ysegs; const int n = b / ysegs;
    const int ox0 = tx * TX;
    const int oy_begin = ys * seg_rows;
    const int oy_end = (oy_begin + seg_rows < p.outH) ? oy_begin + seg_rows : p.outH;
    const int nsteps = (oy_end - oy_begin + SR - 1) / SR;
    if (nsteps <= 0) return;

    for (int i = tid; i < RING * 64; i += 256) {        // pixels 40..47 of every ring row only ever meet zero taps: keep them finite
        const int r = i >> 6, c = i & 63;
        *reinterpret_cast<float4_t*>(fsm + ((r * WXL + 40) * 128) + c * 16) = float4_t{0.f, 0.f, 0.f, 0.f};
    }
    __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)x_bytes, 0x00020000);
    const int drow = lane >> 3, dchunk = lane & 7;
    // window row w (0 = the first row behind output row oy_begin) -> ring slot w % RING; rows [w0, w1) are dealt to the waves piece by piece
    auto fetch_rows = [&](int w0, int w1) {
        for (int piece = wave + (w0 * PPR); piece < w1 * PPR; piece += 4) {
            const int w = piece / PPR, j = piece - w * PPR;
            const int slot = w % RING;
            const int R = slot * WXL + j * 8 + drow;
            const int sc = (((dchunk >> 1) ^ ((R >> 1) & 3)) << 1) | (dchunk & 1);
            const int iy = oy_begin - p.pady0 + w, ix = ox0 - p.padx0 + j * 8 + drow;
            const unsigned okm = 0u - (unsigned)(((unsigned)iy < (unsigned)p.inH) & ((unsigned)ix < (unsigned)p.inW) & (j * 8 + drow < TX + FW - 1));
            const unsigned real = (unsigned)(n * (int)p.isn + iy * (int)p.isy + ix * (int)p.isx + cb0 * 64 + sc * 8) * 2u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (fir_lds_ptr)(fsm + (slot * WXL + j * 8) * 128), 16, (real & okm) | (SBG_FIR_OOB & ~okm), 0, 0, 0);
        }
    };
    fetch_rows(0, SR + FH - 1);

    const int fi = lane & 15, fg = lane >> 4, fq = fi >> 2, fp = fi & 3;
    const unsigned lds_base = (unsigned)(uintptr_t)((fir_lds_ptr)fsm);
    short8_t bt[FH];
    {   // the sixteen taps first (uniform addresses, all in flight together), then the per-lane band matrix by selection: written as a load
        // under the lane's own condition this was 32 dependent load -> wait round trips at the head of every workgroup
        float taps[FH][FW];
#pragma unroll
        for (int ky = 0; ky < FH; ky++)
#pragma unroll
            for (int kx = 0; kx < FW; kx++) taps[ky][kx] = p.f[(p.flip ? ky : FH - 1 - ky) * p.fsy + (p.flip ? kx : FW - 1 - kx) * p.fsx];
#pragma unroll
        for (int ky = 0; ky < FH; ky++)
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int kpix = j < 4 ? 4 * fg + j : 16 + 4 * fg + (j - 4);
                const int kx = kpix - fi;
                float v = 0.f;
#pragma unroll
                for (int q = 0; q < FW; q++) v = (kx == q) ? taps[ky][q] : v;
                bt[ky][j] = FirMfma<T>::bits(v);
            }
    }
    // the swizzle of an LDS row depends on (R >> 1) & 3 with R = slot * 48 + pixel: 48 is a multiple of 8, so the offsets are slot-independent
    int offA[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int Rrel = 4 * fg + fq, chunk = ((c * 16) >> 3) + (fp >> 1);
        const int sw = (((chunk >> 1) ^ ((Rrel >> 1) & 3)) << 1) | (chunk & 1);
        offA[c] = Rrel * 128 + sw * 16 + (fp & 1) * 8;
    }
    T* yb = (T*)p.y + n * p.osn + cb0 * 64 + (fg & 1) * 16 + (fg >> 1) * 8;
    float4_t t_scale[4], t_bias[4];
    const float t_alpha = p.tail ? p.alpha : 1.f, t_gain = p.tail ? p.act_gain : 1.f, t_cl = (p.tail && p.clamp >= 0.f) ? p.clamp : __builtin_inff();
#pragma unroll
    for (int c = 0; c < 4; c++) { t_scale[c] = float4_t{p.gain, p.gain, p.gain, p.gain}; t_bias[c] = float4_t{0.f, 0.f, 0.f, 0.f}; }
    if (p.tail && p.oscale) {           // (one branch per tensor: its four loads are in flight together)
#pragma unroll
        for (int c = 0; c < 4; c++) t_scale[c] *= *reinterpret_cast<const float4_t*>(p.oscale + (int64_t)n * p.C + cb0 * 64 + c * 16 + 4 * fg);
    }
    if (p.tail && p.bias) {
#pragma unroll
        for (int c = 0; c < 4; c++) t_bias[c] = *reinterpret_cast<const float4_t*>(p.bias + cb0 * 64 + c * 16 + 4 * fg);
    }
    float4_t t_post[4];
#pragma unroll
    for (int c = 0; c < 4; c++) t_post[c] = float4_t{1.f, 1.f, 1.f, 1.f};
    if (p.tail == 1 && p.post) {
#pragma unroll
        for (int c = 0; c < 4; c++) t_post[c] = *reinterpret_cast<const float4_t*>(p.post + (int64_t)n * p.C + cb0 * 64 + c * 16 + 4 * fg);
    }
    typedef __attribute__((ext_vector_type(4))) unsigned uint4_t;
    const T* ysv = BT ? (const T*)p.dact_y + n * p.osn + cb0 * 64 + (fg & 1) * 16 + (fg >> 1) * 8 : nullptr;      // the store layout of this lane (see below)
    const float d_gpos = p.dact_gpos, d_gneg = p.dact_gneg, d_rail = p.dact_rail;
    float4_t dbacc[4];
#pragma unroll
    for (int c = 0; c < 4; c++) dbacc[c] = float4_t{0.f, 0.f, 0.f, 0.f};
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int s = 0; s < nsteps; s++) {
        uint4_t ysave[2][2];
        if (BT) {       // the saved activations of this step's outputs, in the (coalesced, 16 B per lane) layout the stores use; issued ahead of the prefetch
            const int oy_ = oy_begin + SR * s + wave;
#pragma unroll
            for (int sg = 0; sg < 2; sg++) {
                const int ox_ = ox0 + sg * 16 + fi;
                const bool ok_ = oy_ < oy_end && ox_ < p.outW;
                const T* src = ysv + (ok_ ? oy_ * p.osy + ox_ * p.osx : 0);
#pragma unroll
                for (int h = 0; h < 2; h++) ysave[sg][h] = *reinterpret_cast<const uint4_t*>(src + h * 32);
            }
        }
        if (s + 1 < nsteps) fetch_rows(SR * (s + 1) + FH - 1, SR * (s + 2) + FH - 1);       // the four new rows of the next window
        float4_t acc[2][4];
#pragma unroll
        for (int sg = 0; sg < 2; sg++)
#pragma unroll
            for (int c = 0; c < 4; c++) acc[sg][c] = float4_t{0.f, 0.f, 0.f, 0.f};
        // Reads by inline assembly (lds_asm.h): behind the LDS-DMA prefetch just issued, builtin reads get a compiler-inserted vmcnt(0) and the
        // prefetch would be waited for before the first MFMA of the step.  Eight groups (filter row ky, pixel half sg) of eight reads, the next
        // group in flight while the current one multiplies.
        unsigned rowa[FH];
#pragma unroll
        for (int ky = 0; ky < FH; ky++) rowa[ky] = lds_base + (unsigned)((((SR * s + wave + ky) % RING) * WXL) * 128);
        short4_t lo[2][4], hi[2][4];
        auto issue_grp = [&](auto gt) {
            constexpr int g = decltype(gt)::value, ky = g >> 1, sg = g & 1;
            sbg_static_for<4>([&](auto ct) {
                constexpr int c = decltype(ct)::value;
                lds_tr_issue<sg * 16 * 128>(lo[g & 1][c], rowa[ky] + (unsigned)offA[c]);
                lds_tr_issue<sg * 16 * 128 + 16 * 128>(hi[g & 1][c], rowa[ky] + (unsigned)offA[c]);
            });
        };
        issue_grp(std::integral_constant<int, 0>{});
        sbg_static_for<8>([&](auto gt) {
            constexpr int g = decltype(gt)::value, ky = g >> 1, sg = g & 1;
            if constexpr (g + 1 < 8) issue_grp(std::integral_constant<int, g + 1>{});
            lds_wait<(g + 1 < 8 ? 8 : 0)>(lo[g & 1], hi[g & 1]);
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const short8_t fa = {lo[g & 1][c][0], lo[g & 1][c][1], lo[g & 1][c][2], lo[g & 1][c][3], hi[g & 1][c][0], hi[g & 1][c][1], hi[g & 1][c][2], hi[g & 1][c][3]};
                acc[sg][c] = FirMfma<T>::run(fa, bt[ky], acc[sg][c]);
            }
        });
        const int oy = oy_begin + SR * s + wave;
        // fused tail in fp32, then pack to 16-bit pairs
        unsigned pk[2][4][2];
#pragma unroll
        for (int sg = 0; sg < 2; sg++) {
            const int ox = ox0 + sg * 16 + fi;
            const bool okp = oy < oy_end && ox < p.outW;
            if constexpr (BT) {
                // undo the store permutation on the saved activations: swapping is its own inverse, so the pair (c, c + 1) comes back from the same instruction
                unsigned yk[4][2];
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const auto q0 = __builtin_amdgcn_permlane16_swap(ysave[sg][h][0], ysave[sg][h][2], false, false);
                    const auto q1 = __builtin_amdgcn_permlane16_swap(ysave[sg][h][1], ysave[sg][h][3], false, false);
                    yk[2 * h][0] = q0[0]; yk[2 * h + 1][0] = q0[1]; yk[2 * h][1] = q1[0]; yk[2 * h + 1][1] = q1[1];
                }
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    float4_t v = acc[sg][c] * t_scale[c];
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const float yv = FirMfma<T>::from_bits((unsigned short)(yk[c][e >> 1] >> ((e & 1) * 16)));
                        const float slope = (fabsf(yv) < d_rail) ? (yv > 0.f ? d_gpos : d_gneg) : 0.f;
                        v[e] *= slope;
                        dbacc[c][e] += okp ? v[e] : 0.f;
                    }
                    pk[sg][c][0] = (unsigned)(unsigned short)FirMfma<T>::bits(v[0]) | ((unsigned)(unsigned short)FirMfma<T>::bits(v[1]) << 16);
                    pk[sg][c][1] = (unsigned)(unsigned short)FirMfma<T>::bits(v[2]) | ((unsigned)(unsigned short)FirMfma<T>::bits(v[3]) << 16);
                }
            } else {
            const float nz = (p.tail && p.noise && okp) ? p.noise[n * p.noise_sn + (int64_t)oy * p.outW + ox] : 0.f;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                float4_t v = acc[sg][c] * t_scale[c] + (t_bias[c] + nz);
#pragma unroll
                for (int e = 0; e < 4; e++) { float u = v[e]; u = (u > 0.f) ? u : u * t_alpha; v[e] = __builtin_amdgcn_fmed3f(u * t_gain, -t_cl, t_cl) * t_post[c][e]; }
                pk[sg][c][0] = (unsigned)(unsigned short)FirMfma<T>::bits(v[0]) | ((unsigned)(unsigned short)FirMfma<T>::bits(v[1]) << 16);
                pk[sg][c][1] = (unsigned)(unsigned short)FirMfma<T>::bits(v[2]) | ((unsigned)(unsigned short)FirMfma<T>::bits(v[3]) << 16);
            }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's share of the prefetch has landed (and the previous step's stores drained)
        __syncthreads();
#pragma unroll
        for (int sg = 0; sg < 2; sg++) {
            const int ox = ox0 + sg * 16 + fi;
            const bool ok = oy < oy_end && ox < p.outW;
            T* dst = yb + oy * p.osy + ox * p.osx;
#pragma unroll
            for (int c = 0; c < 4; c += 2) {
                const auto r0 = __builtin_amdgcn_permlane16_swap(pk[sg][c][0], pk[sg][c + 1][0], false, false);
                const auto r1 = __builtin_amdgcn_permlane16_swap(pk[sg][c][1], pk[sg][c + 1][1], false, false);
                typedef __attribute__((ext_vector_type(4))) unsigned uint4_t;
                const uint4_t o = {r0[0], r1[0], r0[1], r1[1]};
                if (ok) *reinterpret_cast<uint4_t*>(dst + c * 16) = o;
            }
        }
    }
    if constexpr (BT) {
        // per-channel sums of this workgroup (fixed order): over the 16 pixel lanes of a row by DPP rotates, then over the four waves through LDS
        __syncthreads();                                 // the ring is no longer read
        float* red = reinterpret_cast<float*>(fsm);      // [4 waves][64 channels]
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                float a = dbacc[c][e];
                a += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, a), 0x128, 0xf, 0xf, false));    // row_ror:8
                a += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, a), 0x124, 0xf, 0xf, false));    // row_ror:4
                a += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, a), 0x122, 0xf, 0xf, false));    // row_ror:2
                a += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, a), 0x121, 0xf, 0xf, false));    // row_ror:1
                if (fi == 0) red[wave * 64 + c * 16 + 4 * fg + e] = a;
            }
        __syncthreads();
        if (tid < 64) p.dact_part[(int64_t)blockIdx.x * 64 + tid] = (red[tid] + red[64 + tid]) + (red[128 + tid] + red[192 + tid]);
    }
}

// Strip / segment geometry of a sliding-window launch, and the extent of its buffer resource.
struct FirSlidePlan { unsigned x_bytes; int tiles_x, cblocks, ysegs, seg_rows; int64_t nblk; };

// THE rule "the matrix-core FIR takes this launch"; every caller asks here.  On top of it a launch needs the 8-channel vector layout
// (`vec8` of the entry point: pointer and stride alignment).
//  FIR_RULE_SHAPE   dtype, filter, sizes and channel-minor layout only: the answer of sbg_upfirdn2d_tail_supported(), which the Python
//                   layer probes before it has a launch to describe -- it never looked at the operand's extent or the stride signs
//  FIR_RULE_LAUNCH  the whole rule; *plan (if given) then describes the launch
enum FirRule { FIR_RULE_SHAPE, FIR_RULE_LAUNCH };
static bool fir_mfma_accepts(const UpfirdnArgs& a, bool exact16, size_t elem_size, FirRule rule, FirSlidePlan* plan = nullptr)
{
    if (elem_size != 2 || !exact16 || a.upx != 1 || a.upy != 1 || a.downx != 1 || a.downy != 1 || a.fw != 4 || a.fh != 4) return false;
    if ((a.C % 64) != 0 || a.outW < 16 || a.outH < 8 || a.isc != 1 || a.osc != 1) return false;   // smaller images stay with the register-blocked kernel
    if (rule == FIR_RULE_SHAPE) return true;
    if (a.tail == 2 && a.outH < 16) return false;       // the backward tail's domain (sbg_upfirdn2d_dact_rows)
    // the window is fetched through a buffer resource with 32-bit offsets; bit 31 marks the padding
    const int64_t x_bytes = 2 * ((int64_t)(a.N - 1) * a.isn + (int64_t)(a.inH - 1) * a.isy + (int64_t)(a.inW - 1) * a.isx + a.C);
    if (x_bytes >= (int64_t)SBG_FIR_OOB || a.isn < 0 || a.isy < 0 || a.isx < 0) return false;
    FirSlidePlan g;
    g.x_bytes = (unsigned)x_bytes;
    g.tiles_x = (a.outW + 31) / 32; g.cblocks = a.C / 64;
    const int64_t strips = (int64_t)a.N * g.tiles_x * g.cblocks;
    // vertical segments: enough workgroups for two per CU on every CU, but at least 16 output rows per segment (3 overlap rows are re-read per segment)
    g.ysegs = 1;
    while (strips * g.ysegs < 1024 && a.outH / (g.ysegs * 2) >= 16) g.ysegs *= 2;
    g.seg_rows = (((a.outH + g.ysegs - 1) / g.ysegs) + 3) & ~3;
    g.ysegs = (a.outH + g.seg_rows - 1) / g.seg_rows;
    g.nblk = strips * g.ysegs;
    if (g.nblk > INT32_MAX || g.nblk <= 0) return false;
    if (plan) *plan = g;
    return true;
}

template <class T, bool BT>
static bool launch_fir_slide(const UpfirdnArgs& a, const FirSlidePlan& g, hipStream_t stream)
{
    constexpr int lds = 12 * 48 * 128;
    auto kern = upfirdn2d_fir_slide_kernel<T, BT>;
    if (!SBG_RAISE_LDS_ONCE(kern, lds)) return false;
    SBG_LAUNCH_OR(return false, kern, dim3((unsigned)g.nblk), dim3(256), lds, stream, a, g.x_bytes, g.tiles_x, g.cblocks, g.ysegs, g.seg_rows);
    return true;
}

// Kernel that served an upfirdn2d launch: the launch log records 10000 * variant + 16 * upx + downx in dims[6] (listed in sbg_hip.h).
// 2 and 4 were the tile kernel's (alone / with edge columns) and stay retired: committed profiles carry them.
enum FirVariant { FIR_V_NONE = 0, FIR_V_SLIDE = 1, FIR_V_SLIDE_EDGE = 3, FIR_V_FIXED44 = 5, FIR_V_GENERIC = 6, FIR_V_VEC8 = 7, FIR_V_SCALAR = 8 };

template <class T>
static int launch_upfirdn(const UpfirdnArgs& a0, bool vec8, bool exact16, hipStream_t stream)
{
    UpfirdnArgs a = a0;
    const double es = sizeof(T) == 4 ? 4 : 2;
    SbgProfScope prof(stream, SBG_K_UPFIRDN2D, 0.0,
                      es * ((double)a.N * a.C * a.inH * a.inW + (double)a.N * a.C * a.outH * a.outW),
                      {a.N, a.C, a.inH, a.inW, a.outH, a.outW, a.upx * 16 + a.downx});      // dims[6] gains the variant digit below
    auto try_fir_mfma = [&](const UpfirdnArgs& b) -> bool {
        if constexpr (sizeof(T) == 2) {
            FirSlidePlan g;
            if (!vec8 || !fir_mfma_accepts(b, exact16, sizeof(T), FIR_RULE_LAUNCH, &g)) return false;
            return b.tail == 2 ? launch_fir_slide<T, true>(b, g, stream) : launch_fir_slide<T, false>(b, g, stream);
        } else {
            return false;
        }
    };
    // A few columns beyond a multiple of the 32-column strips (the 2 res + 1 wide outputs of the discriminator's low-pass in front of a strided
    // convolution: 257 = 8 strips + 1) would cost a whole strip of matrix-core work (9 strips for 257 columns: 11 % idle, 33 columns: 48 %): the
    // strips take the multiple of 32 and the register-blocked kernel the remaining columns, as a launch over the shifted sub-rectangle.
    const int rem = a.outW % 32;
    const int code = a.upx * 16 + a.downx;
    if (!a.tail && rem >= 1 && rem <= 4 && a.outW > 32) {
        UpfirdnArgs m = a, e = a;
        m.outW = a.outW - rem;
        e.outW = rem; e.padx0 = a.padx0 - m.outW; e.y = (void*)((T*)a.y + (int64_t)m.outW * a.osx);
        if (try_fir_mfma(m)) {
            const int xblocks = (e.outW + FIR_TX - 1) / FIR_TX, yblocks = (e.outH + FIR_TY - 1) / FIR_TY;
            e.total = (int64_t)e.N * yblocks * xblocks * (e.C >> 3);
            SBG_LAUNCH((upfirdn2d_fir_kernel<T, 4, 4>), dim3(sbg_stream_grid(e.total, 256)), dim3(256), 0, stream, e, xblocks, yblocks);
            SBG_HIP_LAUNCH_CHECK();
            prof.set_dim(6, 10000 * FIR_V_SLIDE_EDGE + code);
            return SBG_OK;
        }
    }
    int variant = try_fir_mfma(a) ? FIR_V_SLIDE : FIR_V_NONE;
    if (variant != FIR_V_NONE) {
        // matrix-core FIR
    } else if (a.tail) {
        return sbg_fail(SBG_ERR_UNSUPPORTED, "upfirdn2d: fused tail requested but the matrix-core FIR path does not take this launch");
    } else if (vec8 && a.upx == 1 && a.upy == 1 && a.downx == 1 && a.downy == 1 && a.fw <= FIR_MAXF && a.fh <= FIR_MAXF && a.fw * a.fh > 1) {
        const int xblocks = (a.outW + FIR_TX - 1) / FIR_TX, yblocks = (a.outH + FIR_TY - 1) / FIR_TY;
        a.total = (int64_t)a.N * yblocks * xblocks * (a.C >> 3);
        if (a.fw == 4 && a.fh == 4) {
            variant = FIR_V_FIXED44;
            SBG_LAUNCH((upfirdn2d_fir_kernel<T, 4, 4>), dim3(sbg_stream_grid(a.total, 256)), dim3(256), 0, stream, a, xblocks, yblocks);
        } else {
            variant = FIR_V_GENERIC;
            SBG_LAUNCH((upfirdn2d_fir_kernel<T, 0, 0>), dim3(sbg_stream_grid(a.total, 256)), dim3(256), 0, stream, a, xblocks, yblocks);
        }
    } else if (vec8) {
        variant = FIR_V_VEC8;
        a.total = (int64_t)a.N * a.outH * a.outW * (a.C >> 3);
        SBG_LAUNCH((upfirdn2d_kernel<T, 8>), dim3(sbg_stream_grid(a.total, 256)), dim3(256), 0, stream, a);
    } else {
        variant = FIR_V_SCALAR;
        a.total = (int64_t)a.N * a.outH * a.outW * a.C;
        SBG_LAUNCH((upfirdn2d_kernel<T, 1>), dim3(sbg_stream_grid(a.total, 256)), dim3(256), 0, stream, a);
    }
    SBG_HIP_LAUNCH_CHECK();
    prof.set_dim(6, 10000 * variant + code);
    return SBG_OK;
}

// the kernels' view of a parameter block (copies only; the entry point validates)
static void fill_args(const sbg_upfirdn2d_params* q, UpfirdnArgs& a)
{
    a.x = q->x; a.f = q->f; a.y = q->y;
    a.upx = q->upx; a.upy = q->upy; a.downx = q->downx; a.downy = q->downy; a.padx0 = q->padx0; a.pady0 = q->pady0;
    a.flip = q->flip ? 1 : 0; a.gain = q->gain;
    a.inW = q->inSize[0]; a.inH = q->inSize[1]; a.C = q->inSize[2]; a.N = q->inSize[3];
    a.isx = q->inStride[0]; a.isy = q->inStride[1]; a.isc = q->inStride[2]; a.isn = q->inStride[3];
    a.fw = q->filterSize[0]; a.fh = q->filterSize[1]; a.fsx = q->filterStride[0]; a.fsy = q->filterStride[1];
    a.outW = q->outSize[0]; a.outH = q->outSize[1];
    a.osx = q->outStride[0]; a.osy = q->outStride[1]; a.osc = q->outStride[2]; a.osn = q->outStride[3];
    a.total = 0;
    a.oscale = q->oscale; a.noise = q->noise; a.noise_sn = q->noise_stride_n; a.bias = q->bias;
    a.tail = q->dact_y ? 2 : (q->act != 0 ? 1 : 0);
    a.alpha = q->act == SBG_ACT_LRELU ? q->alpha : (q->act == SBG_ACT_RELU ? 0.f : 1.f); a.act_gain = q->act_gain; a.clamp = q->clamp;
    a.post = q->post_scale;
    // backward tail: slope of clamp(act(.) * gain) at the saved output (same tests as sbg_modconv_bwd)
    a.dact_y = q->dact_y; a.dact_part = q->dact_y ? q->dact_partial : nullptr;
    a.dact_gpos = q->dact_y ? q->dact_gain : 1.f;
    a.dact_gneg = !q->dact_y ? 1.f : (q->dact_act == SBG_ACT_LRELU ? q->dact_gain * q->dact_alpha : (q->dact_act == SBG_ACT_RELU ? 0.f : q->dact_gain));
    a.dact_rail = (q->dact_y && q->dact_clamp >= 0.f) ? q->dact_clamp : __builtin_inff();
}

} // namespace

extern "C" int sbg_upfirdn2d_tail_supported(const sbg_upfirdn2d_params* q)
{
    if (!q) return 0;
    UpfirdnArgs a;
    fill_args(q, a);
    return fir_mfma_accepts(a, q->filter_exact16 != 0, q->dtype == SBG_BF16 || q->dtype == SBG_F16 ? 2 : 0, FIR_RULE_SHAPE);
}

// Rows of `dact_partial` (= workgroups of the sliding-window launch) for a launch with a backward tail, or -1 when that kernel does not take it.
extern "C" int64_t sbg_upfirdn2d_dact_rows(const sbg_upfirdn2d_params* q)
{
    if (!q) return -1;
    UpfirdnArgs a;
    fill_args(q, a);
    a.tail = 2;         // whether or not dact_y is set yet: the caller sizes dact_partial from this answer
    FirSlidePlan g;
    return fir_mfma_accepts(a, q->filter_exact16 != 0, q->dtype == SBG_BF16 || q->dtype == SBG_F16 ? 2 : 0, FIR_RULE_LAUNCH, &g) ? g.nblk : -1;
}

extern "C" int sbg_upfirdn2d(const sbg_upfirdn2d_params* q, sbg_stream_t stream)
{
    SBG_CHECK(q != nullptr && q->x != nullptr && q->f != nullptr && q->y != nullptr, "upfirdn2d: null pointer");
    SBG_CHECK(q->dtype == SBG_F32 || q->dtype == SBG_F16 || q->dtype == SBG_BF16, "upfirdn2d: unsupported dtype %d", q->dtype);
    SBG_CHECK(q->filterSize[0] >= 1 && q->filterSize[1] >= 1, "upfirdn2d: f must be at least 1x1");
    SBG_CHECK(q->upx >= 1 && q->upy >= 1, "upfirdn2d: upsampling factor must be at least 1");
    SBG_CHECK(q->downx >= 1 && q->downy >= 1, "upfirdn2d: downsampling factor must be at least 1");
    SBG_CHECK(q->outSize[0] >= 1 && q->outSize[1] >= 1, "upfirdn2d: output must be at least 1x1");
    SBG_CHECK(q->outSize[2] == q->inSize[2] && q->outSize[3] == q->inSize[3], "upfirdn2d: channel/batch size mismatch");
    const int64_t in_numel  = (int64_t)q->inSize[0] * q->inSize[1] * q->inSize[2] * q->inSize[3];
    const int64_t out_numel = (int64_t)q->outSize[0] * q->outSize[1] * q->outSize[2] * q->outSize[3];
    SBG_CHECK(in_numel <= INT32_MAX, "upfirdn2d: x is too large");
    SBG_CHECK(out_numel <= INT32_MAX, "upfirdn2d: output is too large");
    if (out_numel == 0) return SBG_OK;

    UpfirdnArgs a;
    fill_args(q, a);
    SBG_CHECK(!q->post_scale || (q->act != 0 && sbg_aligned16(q->post_scale)), "upfirdn2d: post_scale belongs to the forward tail (act != 0) and must be 16-byte aligned");
    if (a.tail == 2) {
        SBG_CHECK(q->act == 0, "upfirdn2d: forward and backward tails exclude each other");
        SBG_CHECK(q->dact_partial != nullptr, "upfirdn2d: the backward tail needs dact_partial (sbg_upfirdn2d_dact_rows() x 64 floats)");
        SBG_CHECK(q->dact_act == SBG_ACT_LINEAR || q->dact_act == SBG_ACT_RELU || q->dact_act == SBG_ACT_LRELU, "upfirdn2d: backward-tail activation must be linear, relu or lrelu");
        SBG_CHECK(q->dact_gain > 0.f && sbg_aligned16(q->dact_y), "upfirdn2d: backward tail: gain must be positive, dact_y 16-byte aligned");
    }

    // 8-channel vector path: channel-minor on both sides, every pixel start 16-B aligned.
    const int es = sbg_dtype_size(q->dtype);
    auto mult8 = [&](int64_t s) { return ((s * es) % 16) == 0; };
    bool vec8 = a.isc == 1 && a.osc == 1 && (a.C % 8) == 0 && sbg_aligned16(a.x) && sbg_aligned16(a.y) &&
                mult8(a.isx) && mult8(a.isy) && mult8(a.isn) && mult8(a.osx) && mult8(a.osy) && mult8(a.osn) &&
                (es == 2 || ((a.isx | a.isy | a.isn | a.osx | a.osy | a.osn) % 4) == 0);
    hipStream_t s = (hipStream_t)stream;
    const bool exact16 = q->filter_exact16 != 0;
    if (a.tail == 2) {
        SBG_CHECK(vec8 && fir_mfma_accepts(a, exact16, es, FIR_RULE_LAUNCH), "upfirdn2d: the backward tail needs the sliding-window matrix-core FIR (sbg_upfirdn2d_dact_rows)");
    } else if (a.tail) {
        SBG_CHECK(q->act == SBG_ACT_LINEAR || q->act == SBG_ACT_RELU || q->act == SBG_ACT_LRELU, "upfirdn2d: fused activation must be linear, relu or lrelu");
        SBG_CHECK(vec8 && fir_mfma_accepts(a, exact16, es, FIR_RULE_SHAPE), "upfirdn2d: the fused tail needs the matrix-core FIR path (sbg_upfirdn2d_tail_supported)");
        SBG_CHECK((!q->oscale || sbg_aligned16(q->oscale)) && (!q->bias || sbg_aligned16(q->bias)), "upfirdn2d: oscale / bias must be 16-byte aligned");
    }
    if (q->dtype == SBG_F32) return launch_upfirdn<float>(a, vec8, false, s);
    if (q->dtype == SBG_F16) return launch_upfirdn<f16_s>(a, vec8, exact16, s);
    return launch_upfirdn<bf16_s>(a, vec8, exact16, s);
}
