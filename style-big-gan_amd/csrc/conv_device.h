// conv_device.h -- device-side pieces shared by the convolution kernels (conv_k64.hip, conv_up2.hip, conv_igemm.hip, conv_thin.hip):
// the LDS image conventions of the K-step-64 kernels (DMA lane coordinates, channel permutation, fragment offsets), the MFMA step,
// the scalar tail of the fused epilogue and the 8-channel epilogue of conv_k64.hip.  Everything is inlined into its kernel.
// A piece lives here only where the kernels that use it still compile to the instructions they had with the piece written in place;
// what did not pass that test stays in its kernel (weight-row offsets, accumulator clear, fragment reads, conv_k64_kernel's MFMA loop).
#pragma once
#include "conv_common.h"
#include "lds_asm.h"

namespace sbgconv {

// LDS row R of the weight tile holds output channel c0 + chmap(R): inside a 32-row block, MFMA row m of the even / odd
// 16-row tile maps to channel 8 (m / 4) + 4 (tile & 1) + (m % 4), so accumulator tiles (2h, 2h + 1) of a lane hold
// channels 32 h + 8 fg + {0..3} and {4..7}.
static __device__ __forceinline__ int chmap(int R) { return (R & ~31) + 8 * ((R & 15) >> 2) + 4 * ((R >> 4) & 1) + (R & 3); }

template <int N> static __device__ __forceinline__ void wait_vmcnt_const() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }

// XCD-aware tile order: workgroups b and b + 8 share an XCD (L2); give each XCD a contiguous run of tiles
static __device__ __forceinline__ int xcd_tile_order(int bid, int nwg)
{
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, k = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

// DMA lane coordinates of a piece (8 rows x 128 B): lane -> (row = 8 piece + dma_lrow, slot = lane & 7), source k-slot = slot ^ (row & 7);
// dma_src_k = the channel offset of that k-slot inside the 64-channel slice
static __device__ __forceinline__ int dma_lrow(int lane)  { return lane >> 3; }
static __device__ __forceinline__ int dma_src_k(int lane, int lrow) { return ((lane & 7) ^ lrow) * 8; }

// MFMA fragments of lane (fr = lane & 15, fg = lane >> 4): byte offset of k-sub 0 inside a 16-row block; k-sub 1 = ^ 64
static __device__ __forceinline__ int frag_off(int fr, int fg) { return fr * 128 + ((fg ^ (fr & 7)) << 4); }

// one K-step (two 32-deep k-subs) of the wave tile
template <class MF, int TC, int TP>
static __device__ __forceinline__ void mma_step(float4_t (&acc)[TC][TP], const short8_t (&fa)[2][TC], const short8_t (&fb)[2][TP])
{
#pragma unroll
    for (int ks = 0; ks < 2; ks++)
#pragma unroll
        for (int i = 0; i < TC; i++)
#pragma unroll
            for (int j = 0; j < TP; j++) acc[i][j] = Mfma<MF>::run(fa[ks][i], fb[ks][j], acc[i][j]);
}

// Scalar tail of the fused epilogue: clamp(act(u * oscale[si] + add) * gain), add = noise + bias.  (The vectorised fast path below has its
// own med3 form, and the slow path of conv_epilogue8 restates this one: see there.)
static __device__ __forceinline__ float tail(const ConvArgs& p, float u, int64_t si, float add)
{
    if (p.oscale) u *= p.oscale[si];
    u += add;
    if (p.act == SBG_ACT_LRELU) u = (u > 0.f) ? u : u * p.alpha;
    else if (p.act == SBG_ACT_RELU) u = (u > 0.f) ? u : 0.f;
    u *= p.gain;
    if (p.clamp >= 0.f) u = (u > -p.clamp && u < p.clamp) ? u : (u >= 0.f ? p.clamp : -p.clamp);
    return u;
}

// Straight-line fast path of the epilogue (layout of the accumulators: see conv_epilogue8 below): the output dtype and "no epilogue math" are template parameters, every 8-channel group of the
// wave is in range and 16-B aligned (checked by the caller), so the loops below carry no per-element guards and no dtype
// branches: leaky ReLU with alpha 0 / 1 covers ReLU / linear, clamp = med3 with an infinite bound when disabled.
// `lp`: the tile's epilogue parameters staged in LDS by a loader wave (halo kernel: [noise of the TH x TW tile, row-major | bias of the 128 tile
// channels | demodulation coefficients of (image, 128 tile channels)], 1 KiB each, fp32) -- the loads below then come from LDS (~100 cycles)
// instead of L2 / HBM (a round trip of 1-2 us under load, paid by both compute groups at every tile boundary); lp_c = channel offset of this wave
// inside the tile, lp_pix(j) = the pixel's index inside the tile.
typedef __attribute__((address_space(3))) const float lds_cfloat;
typedef __attribute__((address_space(3))) const float4_t lds_cfloat4;
struct LdsParams { lds_cfloat* base; int c; int tw; };
template <int TC, int TP, int YDT, bool PLAIN, bool NUNI, bool LP = false, class PixFn>
static __device__ __forceinline__ void conv_epilogue_fast(const ConvArgs& p, float4_t (&acc)[TC][TP], int cbase, int fg, PixFn pix, int64_t ybase,
                                                          const LdsParams* lp = nullptr, int y0 = 0, int x0 = 0)
{
    // NUNI: every pixel of the wave lies in one image (halo kernel), so the demodulation coefficients are per-h constants.
    // Every parameter load (noise per pixel, bias and demodulation coefficients per channel group) is issued up front and UNCONDITIONALLY -- an
    // absent term reads a valid dummy address (the first 16 bytes of x) and is replaced by a select -- so the wave waits for ONE round trip.
    // (With `if (p.noise) nz = p.noise[...]` per pixel the compiler emitted load, s_waitcnt vmcnt(0), branch join four times over, plus two
    // more waits for bias and coefficients: six exposed L2 / HBM latencies per tile, more than the arithmetic.)
    constexpr int TH2 = TC / 2;
    const float alpha = (p.act == SBG_ACT_LRELU) ? p.alpha : (p.act == SBG_ACT_RELU ? 0.f : 1.f);
    const float lsel = alpha <= 1.f ? __builtin_inff() : -__builtin_inff();      // leaky ReLU = med3(u, alpha u, +inf) = max for alpha <= 1, min (-inf) above
    const float cl = p.clamp >= 0.f ? p.clamp : __builtin_inff();
    const float gain = p.gain;
    const float* const dummy = reinterpret_cast<const float*>(p.x);
    const bool has_nz = !PLAIN && p.noise != nullptr, has_b = !PLAIN && p.bias != nullptr, has_s = !PLAIN && p.oscale != nullptr;
    int64_t yoff[TP]; float nz[TP]; bool ok[TP]; int nn[TP];
#pragma unroll
    for (int j = 0; j < TP; j++) {
        int n, oy, ox;
        ok[j] = pix(j, n, oy, ox);                      // (an out-of-range pixel still decodes to valid coordinates)
        nn[j] = n;
        yoff[j] = ybase + (int64_t)blockIdx.y * p.y_split_stride + (int64_t)n * p.ys_n + (int64_t)oy * p.ys_h + (int64_t)ox * p.ys_w + cbase + 8 * fg;
        nz[j] = 0.f;
        if (!PLAIN) {
            if constexpr (LP) nz[j] = lp->base[(oy - y0) * lp->tw + (ox - x0)];
            else              nz[j] = *(has_nz ? p.noise + ((int64_t)n * p.noise_sn + (int64_t)oy * p.OW + ox) : dummy);
        }
    }
    float4_t b_lo[TH2], b_hi[TH2], s_lo[TH2], s_hi[TH2];
#pragma unroll
    for (int h = 0; h < TH2; h++) {
        b_lo[h] = b_hi[h] = float4_t{0.f, 0.f, 0.f, 0.f};
        s_lo[h] = s_hi[h] = float4_t{1.f, 1.f, 1.f, 1.f};
        if (!PLAIN) {
            if constexpr (LP) {
                lds_cfloat* b = lp->base + 256 + lp->c + 32 * h + 8 * fg;
                b_lo[h] = *(lds_cfloat4*)b; b_hi[h] = *(lds_cfloat4*)(b + 4);
                if (NUNI) { s_lo[h] = *(lds_cfloat4*)(b + 256); s_hi[h] = *(lds_cfloat4*)(b + 260); }
            } else {
            const float* b = has_b ? p.bias + cbase + 32 * h + 8 * fg : dummy;
            b_lo[h] = *reinterpret_cast<const float4_t*>(b); b_hi[h] = *reinterpret_cast<const float4_t*>(has_b ? b + 4 : dummy);
            if (NUNI) {
                const float* sc = has_s ? p.oscale + (int64_t)nn[0] * p.Cout + cbase + 32 * h + 8 * fg : dummy;
                s_lo[h] = *reinterpret_cast<const float4_t*>(sc); s_hi[h] = *reinterpret_cast<const float4_t*>(has_s ? sc + 4 : dummy);
            }
            }
        }
    }
    if (!PLAIN) {
#pragma unroll
        for (int j = 0; j < TP; j++) nz[j] = has_nz ? nz[j] : 0.f;
#pragma unroll
        for (int h = 0; h < TH2; h++) {
            if (!has_b) { b_lo[h] = float4_t{0.f, 0.f, 0.f, 0.f}; b_hi[h] = b_lo[h]; }
            if (!NUNI || !has_s) { s_lo[h] = float4_t{1.f, 1.f, 1.f, 1.f}; s_hi[h] = s_lo[h]; }
        }
    }
#pragma unroll
    for (int h = 0; h < TH2; h++) {
#pragma unroll
        for (int j = 0; j < TP; j++) {
            if (!ok[j]) continue;
            float4_t lo = acc[2 * h][j], hi = acc[2 * h + 1][j];
            if (!PLAIN) {
                float4_t sl = s_lo[h], sh = s_hi[h];
                if (!NUNI && has_s) {
                    const float* sc = p.oscale + (int64_t)nn[j] * p.Cout + cbase + 32 * h + 8 * fg;
                    sl = *reinterpret_cast<const float4_t*>(sc); sh = *reinterpret_cast<const float4_t*>(sc + 4);
                }
                lo = lo * sl + (nz[j] + b_lo[h]);
                hi = hi * sh + (nz[j] + b_hi[h]);
                const float4_t tl = lo * alpha, th = hi * alpha;       // vector forms: v_pk_mul_f32
#pragma unroll
                for (int e = 0; e < 4; e++) { lo[e] = __builtin_amdgcn_fmed3f(lo[e], tl[e], lsel); hi[e] = __builtin_amdgcn_fmed3f(hi[e], th[e], lsel); }
                lo = lo * gain; hi = hi * gain;
#pragma unroll
                for (int e = 0; e < 4; e++) { lo[e] = __builtin_amdgcn_fmed3f(lo[e], -cl, cl); hi[e] = __builtin_amdgcn_fmed3f(hi[e], -cl, cl); }
            }
            if (YDT == SBG_F32) {
                float* dst = (float*)p.y + yoff[j] + 32 * h;
                if (p.accumulate) { lo += *reinterpret_cast<float4_t*>(dst); hi += *reinterpret_cast<float4_t*>(dst + 4); }
                *reinterpret_cast<float4_t*>(dst) = lo;
                *reinterpret_cast<float4_t*>(dst + 4) = hi;
            } else {
                short8_t o;
#pragma unroll
                for (int e = 0; e < 4; e++) { o[e] = (short)f32_to_bf16_bits(lo[e]); o[4 + e] = (short)f32_to_bf16_bits(hi[e]); }
                *reinterpret_cast<short8_t*>((unsigned short*)p.y + yoff[j] + 32 * h) = o;
            }
        }
    }
}


// Epilogue: lane (fr, fg) holds, for the pixel of fragment column fr in segment j, channels cbase + 32 h + 8 fg + e with
// e = 0..3 in acc[2h][j] and e = 4..7 in acc[2h + 1][j].  pix(j, n, oy, ox) -> in range?
template <int TC, int TP, bool NUNI = false, class PixFn>
static __device__ __forceinline__ void conv_epilogue8(const ConvArgs& p, float4_t (&acc)[TC][TP], int cbase, int fg, PixFn pix, int64_t ybase = 0,
                                                      const LdsParams* lp = nullptr, int y0 = 0, int x0 = 0)
{
    constexpr int TH2 = TC / 2;
    const bool plain = conv_is_plain(p);
    // fast path: the wave's whole channel range is valid, rows and per-channel vectors 16-B aligned, bf16 / fp32 output
    const bool fast = (cbase + 16 * TC <= p.Cout) && ((p.Cout & 7) == 0) && ((((uintptr_t)p.y) & 15) == 0) && (((p.ys_n | p.ys_h | p.ys_w) & 7) == 0)
                      && ((((uintptr_t)p.oscale) & 15) == 0) && ((((uintptr_t)p.bias) & 15) == 0) && p.ydtype != SBG_F16;
    if (fast) {
        if (p.ydtype == SBG_BF16) {
            if (plain) conv_epilogue_fast<TC, TP, SBG_BF16, true, NUNI>(p, acc, cbase, fg, pix, ybase);
            else if (lp) conv_epilogue_fast<TC, TP, SBG_BF16, false, NUNI, true>(p, acc, cbase, fg, pix, ybase, lp, y0, x0);
            else       conv_epilogue_fast<TC, TP, SBG_BF16, false, NUNI>(p, acc, cbase, fg, pix, ybase);
        } else {
            if (plain) conv_epilogue_fast<TC, TP, SBG_F32, true, NUNI>(p, acc, cbase, fg, pix, ybase);
            else if (lp) conv_epilogue_fast<TC, TP, SBG_F32, false, NUNI, true>(p, acc, cbase, fg, pix, ybase, lp, y0, x0);
            else       conv_epilogue_fast<TC, TP, SBG_F32, false, NUNI>(p, acc, cbase, fg, pix, ybase);
        }
        return;
    }
    float bias8[TH2][8];
#pragma unroll
    for (int h = 0; h < TH2; h++) {
        const int co = cbase + 32 * h + 8 * fg;
#pragma unroll
        for (int e = 0; e < 8; e++) bias8[h][e] = (p.bias && co + e < p.Cout) ? p.bias[co + e] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < TP; j++) {
        int n, oy, ox;
        if (!pix(j, n, oy, ox)) continue;
        const int64_t yoff = ybase + (int64_t)blockIdx.y * p.y_split_stride + (int64_t)n * p.ys_n + (int64_t)oy * p.ys_h + (int64_t)ox * p.ys_w;
        const float nz = (!plain && p.noise) ? p.noise[(int64_t)n * p.noise_sn + (int64_t)oy * p.OW + ox] : 0.f;
#pragma unroll
        for (int h = 0; h < TH2; h++) {
            const int co = cbase + 32 * h + 8 * fg;
            if (co >= p.Cout) continue;
            float v[8];
#pragma unroll
            for (int e = 0; e < 4; e++) { v[e] = acc[2 * h][j][e]; v[4 + e] = acc[2 * h + 1][j][e]; }
#pragma unroll 1
            for (int e = 0; e < 8; e++) {            // rolled: this path serves odd channel counts (ToRGB, tails), not the flops
                if (co + e >= p.Cout) break;
                float u = v[e];
                if (!plain) {                        // tail() written out: through the helper conv_k64_kernel compiles to different instructions
                    if (p.oscale) u *= p.oscale[(int64_t)n * p.Cout + co + e];
                    u += nz + bias8[h][e];
                    if (p.act == SBG_ACT_LRELU) u = (u > 0.f) ? u : u * p.alpha;
                    else if (p.act == SBG_ACT_RELU) u = (u > 0.f) ? u : 0.f;
                    u *= p.gain;
                    if (p.clamp >= 0.f) u = (u > -p.clamp && u < p.clamp) ? u : (u >= 0.f ? p.clamp : -p.clamp);
                }
                if (p.ydtype == SBG_F32) {
                    float* dst = (float*)p.y + yoff + co + e;
                    *dst = p.accumulate ? *dst + u : u;
                } else {
                    ((unsigned short*)p.y)[yoff + co + e] = (p.ydtype == SBG_BF16) ? f32_to_bf16_bits(u) : f32_to_f16_bits(u);
                }
            }
        }
    }
}

} // namespace sbgconv
