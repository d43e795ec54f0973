// conv_common.h -- what the convolution kernels (conv_k64.hip, conv_up2.hip, conv_igemm.hip, conv_thin.hip, conv_wgrad.hip) share on the
// host side: the LDS-DMA sentinel, the MFMA wrappers, the one launch function launch_as (these three are all conv_wgrad.hip takes: it has
// its own argument block and byte model), the kernel argument block ConvArgs, the forward launch layer (conv_is_plain, conv_prof_bytes,
// conv_launch) and the entry points of the per-file dispatchers.  The device-side pieces are in conv_device.h.
#pragma once
#include "sbg_common.h"
#include <cstdlib>

// Byte offset that is out of range for every buffer descriptor the kernels build (tensors < 2 GiB): an LDS-DMA load from it writes zeros.
#define SBG_OOB_OFFSET 0x80000000u

namespace sbgconv {

typedef __attribute__((address_space(3))) void* lds_void_ptr;

struct bf16_mfma { static constexpr int dtype = SBG_BF16; };
struct f16_mfma  { static constexpr int dtype = SBG_F16;  };

template <class MF> struct Mfma;
template <> struct Mfma<bf16_mfma> {
    static __device__ __forceinline__ float4_t run(short8_t a, short8_t b, float4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ unsigned short cvt(float v) { return f32_to_bf16_bits(v); }
};
template <> struct Mfma<f16_mfma> {
    static __device__ __forceinline__ float4_t run(short8_t a, short8_t b, float4_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ unsigned short cvt(float v) { return f32_to_f16_bits(v); }
};

struct ConvArgs {
    const unsigned short* x; const unsigned short* w; void* y; const float* oscale;
    const float* bias; const float* noise; int64_t noise_sn; int act; float alpha, gain, clamp;
    int ydtype;
    int N, IH, IW, Cin, Cout, OH, OW;
    int64_t xs_n, xs_h, xs_w, ys_n, ys_h, ys_w, ws_slab, ws_co;
    int stride, ntaps;
    int tap_dy[SBG_MAX_TAPS], tap_dx[SBG_MAX_TAPS], tap_slab[SBG_MAX_TAPS];
    int accumulate;
    int P;            // N * OH * OW output pixels of this launch
    int ptiles, ctiles;
    // phases (conv_gather_ld_kernel): up to four output sub-grids of one launch (the s x s phases of a transposed convolution), each
    // with its own run of taps [ph_tap0, ph_tap0 + ph_ntaps), grid ph_OH x ph_OW, pixel count ph_P and y offset; nphase == 1: the whole launch
    int nphase, ph_rot_div;   // phase of tile r = (r % nphase + (r / nphase) / ph_rot_div) % nphase: a persistent workgroup cycles through the phases
    int ph_tap0[4], ph_ntaps[4], ph_OH[4], ph_OW[4], ph_P[4];
    int64_t ph_yoff[4];
    int ksplit;               // gather kernel: the K-steps are split over gridDim.y workgroups, each writing its own fp32 slab
    int64_t y_split_stride;   // elements between the slabs (0 when ksplit == 1)
    int lds_params;   // halo kernel: a loader wave stages each tile's epilogue parameters (noise / bias / demodulation coefficients) in LDS
};

// no fused epilogue: the accumulators are stored as they are.  (The macro form is for conv_thin_kernel alone, which compiles to different
// instructions when the test goes through a function.)
#define SBG_CONV_IS_PLAIN(a) (((a).act <= SBG_ACT_LINEAR) && (a).gain == 1.f && (a).clamp < 0.f && !(a).bias && !(a).noise && !(a).oscale)
static __host__ __device__ __forceinline__ bool conv_is_plain(const ConvArgs& a) { return SBG_CONV_IS_PLAIN(a); }
// the same for the caller's parameter block, where act 0 and gain 0 stand for "not set"
static inline bool conv_is_plain(const sbg_conv_params& q)
{
    return (q.act == 0 || q.act == SBG_ACT_LINEAR) && (q.gain == 1.f || q.gain == 0.f) && q.clamp < 0.f && !q.bias && !q.noise && !q.oscale;
}

// bytes a launch moves, as the profiler counts them: the input once, the weights once, `outpix` output pixels (read back when accumulating)
static inline double conv_prof_bytes(const ConvArgs& a, double outpix)
{
    const double ys = a.ydtype == SBG_F32 ? 4.0 : 2.0;
    return 2.0 * a.N * a.IH * a.IW * (double)a.Cin + 2.0 * a.ntaps * a.Cout * (double)a.Cin + ys * outpix * (double)a.Cout * (a.accumulate ? 2 : 1);
}

// One launch of a kernel of the family: grid bound, dynamic-LDS limit (raised once per kernel), profiler scope, launch, error check.
// kind = the profiler's kernel kind, who = the entry point named in the error texts.
// dims = the profiler's shape key; its last entry is the code that names the kernel (bench.py, profiles/summarize.py, tests read it).
template <auto Kern, class... Args>
static int launch_as(int kind, const char* who, int64_t nblk, unsigned grid_y, unsigned block, int lds, hipStream_t stream, double flops,
                     double bytes, std::initializer_list<int> dims, const Args&... args)
{
    if (nblk > INT32_MAX || nblk < 1) return sbg_fail(SBG_ERR_INVALID, "%s: grid too large", who);
    if (lds > 64 * 1024 && !SBG_RAISE_LDS_ONCE(Kern, lds))
        return sbg_fail(SBG_ERR_LAUNCH, "%s: cannot raise the dynamic LDS limit to %d bytes", who, lds);
    SbgProfScope prof(stream, kind, flops, bytes, dims);
    SBG_LAUNCH(Kern, dim3((unsigned)nblk, grid_y), dim3(block), lds, stream, args...);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}
// the forward / data-gradient convolutions (conv_wgrad.hip calls launch_as with its own kinds)
template <auto Kern, class... Args>
static int conv_launch(int64_t nblk, unsigned grid_y, unsigned block, int lds, hipStream_t stream, double flops, double bytes,
                       std::initializer_list<int> dims, const Args&... args)
{
    return launch_as<Kern>(SBG_K_CONV_IGEMM, "conv2d_igemm", nblk, grid_y, block, lds, stream, flops, bytes, dims, args...);
}

} // namespace sbgconv

// conv_k64.hip: K-step-64 LDS-DMA kernels (gather and halo-staged).  Returns SBG_OK / an error, or -1 when the launch does not
// fit these kernels (the caller then uses the kernels of conv_igemm.hip).
int sbg_conv_k64_dispatch(sbgconv::ConvArgs& a, bool bf16, int64_t x_bytes, int64_t w_bytes, void* workspace, int ksplit, hipStream_t stream);
// conv_thin.hip: few-channel convolutions (Cin, Cout <= 64, one of them <= 32) as a streaming kernel with the reduction axis packed
// over (tap, channel).  Returns SBG_OK / an error, or -1 when the launch is not a thin one.
int sbg_conv_thin_dispatch(sbgconv::ConvArgs& a, bool bf16, hipStream_t stream);
// conv_up2.hip: puts the taps of a 4 / 2 / 2 / 1-tap stride-2 transposed convolution in canonical order (inside every phase by (dy, dx)), all of them
// or none; false when the launch is not of that form.  Called before any kernel is offered the launch, so every kernel sums a phase in one order.
bool sbg_conv_up2_canonical_taps(sbgconv::ConvArgs& a, int64_t x_bytes, int64_t w_bytes);
// conv_up2.hip: all four phases of a stride-2 3x3 transposed convolution from one staged input halo.  Returns SBG_OK / an error, or -1 when the
// launch is not of that form; on SBG_OK `border` describes the remaining last row / column rectangles as an ordinary phased launch.
int sbg_conv_up2_dispatch(sbgconv::ConvArgs& a, bool bf16, int64_t x_bytes, int64_t w_bytes, sbg_conv_params* border, const sbg_conv_params* q, hipStream_t stream);
