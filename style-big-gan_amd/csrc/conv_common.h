// conv_common.h -- what the convolution kernels (conv_k64.hip, conv_up2.hip, conv_igemm.hip, conv_thin.hip, conv_wgrad.hip) share on the
// host side: the LDS-DMA sentinel, the MFMA wrappers, the one launch function launch_as (these three are all conv_wgrad.hip takes: it has
// its own argument block and byte model), the kernel argument block ConvArgs, the forward launch layer (conv_is_plain, the planned launch
// ConvLaunch / ConvPlan, the profiler model conv_prof, conv_launch) and the per-file fit / launch functions the plan of conv_igemm.hip calls.
// The device-side pieces are in conv_device.h.
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

// ---- the forward / data-gradient launch plan (conv_wgrad.hip has its own) ------------------------------------------------------------
// One kernel launch as conv_plan (conv_igemm.hip) decided it: the kernel family and tile, the launch geometry, the kernel's argument block and
// the profiler's record.  The per-file *_fit functions fill it (pure host arithmetic), the per-file *_launch functions launch it as it stands.
enum ConvFamily { CONV_THIN, CONV_UP2, CONV_GATHER, CONV_HALO, CONV_K64, CONV_GENERIC };
struct ConvLaunch {
    ConvFamily family;
    int bc, bp;                                  // tile: BC x BP (k64, generic), TH x TW (halo), 16-channel fragments x 1 (thin)
    int64_t grid_x; unsigned grid_y, block; int lds;
    ConvArgs a;
    unsigned x_bytes, w_bytes;                   // operand extents, for the buffer descriptors of the LDS-DMA kernels
    int pitch;                                   // thin: LDS row pitch of the weights
    int tiles_y, tiles_x, dymin, dxmin;          // up2: 8 x 32 tiles of the common phase grid, origin of the 2 x 2 tap window
    double flops, bytes; int dims[7];            // the profiler's figures and shape key
};
// A call = up to five launches (up2 + four border rectangles, or four phases), then the slab reduction when K was split.
struct ConvPlan {
    int nlaunch; ConvLaunch launch[5];
    ConvArgs call;                               // the call as the caller described it (what the slab reduction finishes)
    int ksplit; bool reduce_epi;                 // K split of launch[0] (1 = none); the reduction applies the fused epilogue / output cast
    int64_t workspace_bytes;
};

// The profiler's model of a forward launch, every family: 2 flops per multiply-add (macs = output pixels x taps, per channel pair); bytes = the
// input once, the weights once, `outpix` output pixels (read back when accumulating); shape key {pixels, Cout, Cin, taps, stride, rows, kernel code}.
static inline void conv_prof(ConvLaunch& l, double macs, double outpix, int ntaps, int stride, int rows, int code)
{
    const ConvArgs& a = l.a;
    const double ys = a.ydtype == SBG_F32 ? 4.0 : 2.0;
    l.flops = 2.0 * macs * a.Cout * (double)a.Cin;
    l.bytes = 2.0 * a.N * a.IH * a.IW * (double)a.Cin + 2.0 * ntaps * a.Cout * (double)a.Cin + ys * outpix * (double)a.Cout * (a.accumulate ? 2 : 1);
    const int dims[7] = {(int)outpix, a.Cout, a.Cin, ntaps, stride, rows, code};
    for (int i = 0; i < 7; i++) l.dims[i] = dims[i];
}
// ... of a launch whose phases (or whose one grid) each run their own taps
static inline void conv_prof_phases(ConvLaunch& l, int code)
{
    const ConvArgs& a = l.a;
    double macs = (double)a.P * a.ntaps, outpix = a.P;
    if (a.nphase > 1) {
        macs = outpix = 0.0;
        for (int i = 0; i < a.nphase; i++) { macs += (double)a.ph_P[i] * a.ph_ntaps[i]; outpix += a.ph_P[i]; }
    }
    conv_prof(l, macs, outpix, a.ntaps, a.stride, a.OH, code);
}

template <auto Kern, class... Extra>
static int conv_launch(const ConvLaunch& l, hipStream_t stream, const Extra&... extra)
{
    const int* d = l.dims;
    return launch_as<Kern>(SBG_K_CONV_IGEMM, "conv2d_igemm", l.grid_x, l.grid_y, l.block, l.lds, stream, l.flops, l.bytes,
                           {d[0], d[1], d[2], d[3], d[4], d[5], d[6]}, l.a, extra...);
}

} // namespace sbgconv

// Per file: *_fit = does this launch (l.a, l.x_bytes, l.w_bytes set by the plan) fit the file's kernels, and with what parameters -- no HIP call;
// *_launch = launch a leaf that *_fit filled.
// conv_thin.hip: few-channel convolutions (Cin, Cout <= 64, one of them <= 32), single or phased; false when the launch is not a thin one.
bool sbg_conv_thin_fit(sbgconv::ConvLaunch& l);
int  sbg_conv_thin_launch(const sbgconv::ConvLaunch& l, bool bf16, hipStream_t stream);
// conv_up2.hip: all four phases of a stride-2 3x3 transposed convolution from one staged input halo.  A launch of that form (4 / 2 / 2 / 1 taps in
// one 2 x 2 window) gets its taps put in canonical order, inside every phase by (dy, dx), whichever kernel then runs it, so every kernel sums a
// phase in one order.  UP2_FITS: the kernel covers [0, Hm) x [0, Wm) of every phase grid and `border` describes the remaining last row / column
// rectangles as an ordinary phased call (nphase 0: none).
enum Up2Fit { UP2_OTHER_FORM, UP2_ORDERED, UP2_FITS };
Up2Fit sbg_conv_up2_fit(sbgconv::ConvLaunch& l, const sbg_conv_params& q, sbg_conv_params& border);
int    sbg_conv_up2_launch(const sbgconv::ConvLaunch& l, bool bf16, hipStream_t stream);
// conv_k64.hip: the K-step-64 LDS-DMA kernels take every launch whose operands a buffer descriptor can address; _fit chooses the kernel and tile.
// sbg_conv_ksplit_reduce sums the k fp32 slabs of a K-split launch into the call's y (reduce_epi: with the fused epilogue and the output cast).
void sbg_conv_k64_fit(sbgconv::ConvLaunch& l);
int  sbg_conv_k64_launch(const sbgconv::ConvLaunch& l, bool bf16, hipStream_t stream);
int  sbg_conv_ksplit_reduce(const sbgconv::ConvArgs& call, const void* workspace, int ksplit, bool reduce_epi, hipStream_t stream);
