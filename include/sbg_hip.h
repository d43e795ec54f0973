/*
 * sbg_hip.h -- C ABI of libsbg_hip.so, the MI355X (gfx950) hot path of the
 * Style-Big-GAN custom-op layer.
 *
 * Every entry point is `extern "C"`, takes plain device pointers, sizes and a
 * hipStream_t (passed as void*), never blocks the host, never allocates, and
 * returns 0 on success or a non-zero sbg_status; sbg_last_error() returns a
 * thread-local human readable message for the last failing call of the calling
 * thread.  Inputs are borrowed and never written; outputs are caller-allocated.
 * Entry points are re-entrant (autograd worker threads call them concurrently).
 *
 * Each declaration cites the reference interface it replaces
 * (paths relative to the reference checkout).
 */
#ifndef SBG_HIP_H
#define SBG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sbg_stream_t;            /* hipStream_t */

enum sbg_status {
    SBG_OK = 0,
    SBG_ERR_INVALID = 1,               /* argument validation failed (reference: TORCH_CHECK) */
    SBG_ERR_UNSUPPORTED = 2,           /* valid but not implemented by this build            */
    SBG_ERR_LAUNCH = 3                 /* hipLaunchKernel / runtime error                     */
};

enum sbg_dtype { SBG_F32 = 0, SBG_F16 = 1, SBG_BF16 = 2 };

/* activation ids follow the reference's `cuda_idx`
 * (stylegan2ada/torch_utils/ops/bias_act.py:23-33). */
enum sbg_act {
    SBG_ACT_LINEAR = 1, SBG_ACT_RELU = 2, SBG_ACT_LRELU = 3, SBG_ACT_TANH = 4, SBG_ACT_SIGMOID = 5,
    SBG_ACT_ELU = 6, SBG_ACT_SELU = 7, SBG_ACT_SOFTPLUS = 8, SBG_ACT_SWISH = 9
};

int         sbg_version(void);
const char* sbg_last_error(void);

/* ------------------------------------------------------------------------------------------
 * bias_act: y = clamp(act(x + b[(i / stepB) % sizeB]) * gain)  and its 1st / 2nd derivative forms.
 * Replaces the pybind entry `bias_act(x, b, xref, yref, dy, grad, dim, act, alpha, gain, clamp)`
 * (stylegan2ada/torch_utils/ops/bias_act.cpp:32-90) with the fields of `bias_act_kernel_params`
 * (stylegan2ada/torch_utils/ops/bias_act.h:12-31) minus the launch-tuning ones.
 * NULL pointer == "absent" (the reference passes an empty tensor).  All tensors share x's dense
 * layout; `dtype` applies to x, b, xref, yref, dy, y.  clamp < 0 disables clamping. */
int sbg_bias_act(const void* x, const void* b, const void* xref, const void* yref, const void* dy,
                 void* y, int dtype, int grad, int act, float alpha, float gain, float clamp,
                 int64_t sizeX, int sizeB, int64_t stepB, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * upfirdn2d: pad -> zero-insert upsample -> 2-D FIR -> decimate.
 * Replaces the pybind entry `upfirdn2d(x, f, upx, upy, downx, downy, padx0, padx1, pady0, pady1,
 * flip, gain)` (stylegan2ada/torch_utils/ops/upfirdn2d.cpp:16-94) with the fields of
 * `upfirdn2d_kernel_params` (stylegan2ada/torch_utils/ops/upfirdn2d.h:14-40).
 * Sizes/strides are [W, H, C, N] in elements like the reference's int4 fields; the filter is
 * float32 [fh, fw] with element strides; padx1/pady1 are implied by the output size. */
typedef struct sbg_upfirdn2d_params {
    const void*  x;
    const float* f;
    void*        y;
    int dtype;
    int upx, upy, downx, downy, padx0, pady0;
    int flip;
    float gain;
    int     inSize[4];      int64_t inStride[4];
    int     filterSize[2];  int     filterStride[2];      /* [W, H] */
    int     outSize[4];     int64_t outStride[4];
    /* Optional fused tail (the `fma(x, dcoefs, noise)` + `bias_act` that follow the low-pass of an up-sampling synthesis layer,
     * train_parts/generators.py:84-88,328):  y = clamp(act(fir * gain * oscale[n*C + c] + noise[n*noise_stride_n + oy*outW + ox] + bias[c]) * act_gain).
     * fp32 arrays, each may be NULL; act in {0 = no tail, linear, relu, lrelu}; clamp < 0 disables.  Only the matrix-core FIR path
     * (16-bit channel-minor tensors, up = down = 1, 4x4 exact taps, C % 64 == 0) applies it: sbg_upfirdn2d_tail_supported(). */
    const float* oscale; const float* noise; int64_t noise_stride_n; const float* bias;
    int act; float alpha, act_gain, clamp;
    int     filter_exact16;  /* hint: every tap of f is exactly representable in `dtype` (bf16 / f16), so the filter may be fed to the
                                matrix cores without rounding ([1,3,3,1]-type filters are); 0 = unknown -> fp32 vector path */
    /* Optional backward tail (excludes the forward tail above).  In the backward of `bias_act -> low-pass` -- a discriminator block's conv0 followed by
     * the filter of its down-sampling conv1, train_parts/discriminators.py:286-291 -- this launch is the transposed low-pass and its result is the
     * gradient w.r.t. the bias_act's OUTPUT `dact_y` (saved; this launch's output geometry).  With dact_y != NULL the kernel multiplies that result by
     * the slope of clamp(act(.) * dact_gain) at dact_y (bias_act.py:159-210 for the piecewise-linear activations: dact_gain above zero,
     * dact_gain * dact_alpha below for lrelu, zero where |y| >= dact_clamp; dact_clamp < 0 disables) and accumulates it per channel -- the bias
     * gradient: dact_partial[r][64] for r < sbg_upfirdn2d_dact_rows(), row r = ((n * ysegs + s) * xstrips + x) * (C / 64) + channel block, to be summed
     * over everything but the channel block by the caller.  Sliding-window matrix-core FIR only: _dact_rows() returns -1 for other launches. */
    const void* dact_y; float* dact_partial; int dact_act; float dact_alpha, dact_gain, dact_clamp;
    /* Forward tail only: the finished value is multiplied by post_scale[n*C + c] -- the style modulation `x * styles` of the layer that reads this
     * output next (generators.py:79), for passes in which nothing else reads it (inference-mode generator passes).  NULL = none. */
    const float* post_scale;
} sbg_upfirdn2d_params;
int sbg_upfirdn2d_tail_supported(const sbg_upfirdn2d_params* p);
int64_t sbg_upfirdn2d_dact_rows(const sbg_upfirdn2d_params* p);
int sbg_upfirdn2d(const sbg_upfirdn2d_params* p, sbg_stream_t stream);

/* Separable filter (1-D `f` of `taps` taps applied along both axes) in one launch -- replaces the reference's two plugin calls
 * with sqrt(gain) each for a rank-1 filter (stylegan2ada/torch_utils/ops/upfirdn2d.py:236-240).  Dense planar fp32 planes
 * x [M, IH, IW] -> y [M, OH, OW]; up, down in {1, 2} on both axes; OH = (IH*up + pady0 + pady1 - taps) / down + 1 etc. is the
 * caller's to compute (as for sbg_upfirdn2d); `gain` is the total gain.  _supported() says whether (up, down, taps) fits. */
int sbg_upfirdn2d_separable_supported(int up, int down, int taps);
int sbg_upfirdn2d_separable(const float* x, const float* f, float* y, int M, int IH, int IW, int OH, int OW, int taps,
                            int up, int down, int padx0, int pady0, int flip, float gain, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution on MFMA (channels-last activations).
 * Replaces the aten/cuDNN calls behind `conv2d_gradfix.conv2d / conv_transpose2d`
 * (stylegan2ada/torch_utils/ops/conv2d_gradfix.py:35-45,107-118): forward, data-gradient and the
 * four sub-pixel phases of a stride-2 transposed convolution are all expressed as
 *
 *   y[n, oy*ysh + yoh, ox*ysw + yow, co] (+)= sum_{t < ntaps} sum_{ci}
 *        x[n, oy*stride + dy[t], ox*stride + dx[t], ci] * w[wslab[t]][co][ci]
 *
 * over the launch's output grid OH x OW (out-of-range input pixels read as zero).
 * x: [N, IH, IW, Cin] channel-minor (Cin % 8 == 0, pixel stride xs_w etc. in elements),
 * w: packed [nslabs][Cout][Cin] (same dtype as x), y: channel-minor, dtype `ydtype`.
 * Optional fused epilogue (every pointer may be NULL, act 0 / SBG_ACT_LINEAR with gain 1 and clamp < 0 = identity), the
 * demodulation + noise + bias_act tail of the reference's layers (train_parts/generators.py:84-88,328; ops/bias_act.py:94-123):
 *   y = clamp( act( acc * oscale[n*Cout + co] + noise[n*noise_stride_n + pixel] + bias[co] ) * gain )
 * with fp32 oscale / noise / bias, pixel = oy*OW + ox of the launch grid, act in {linear, relu, lrelu}.
 * `accumulate` adds into the existing y (fp32 y only, no epilogue).
 * Kernel choice is internal: one host-side plan per call (csrc/conv_igemm.hip: conv_plan).  Precedence: the thin streaming kernel (few
 * channels) -> for phased calls the one-pass up2 kernel plus its border, the multi-phase gather, or one launch per phase -> the K-step-64
 * kernels (halo-staged 3x3, 64x256 / 128x128 tiles, persistent gather, 256x256, 128x256), with the K split -> the generic kernel for operands
 * of 2 GiB or more and negative strides.  sbg_conv2d_igemm_plan() prints the plan of a block without touching a device. */
#define SBG_MAX_TAPS 16
typedef struct sbg_conv_params {
    const void* x; const void* w; void* y;
    const float* oscale;
    int xdtype, ydtype;
    int N, IH, IW, Cin, Cout, OH, OW;
    int64_t xs_n, xs_h, xs_w;
    int64_t ys_n, ys_h, ys_w;
    int64_t ws_slab, ws_co;
    int stride;
    int ntaps;
    int tap_dy[SBG_MAX_TAPS], tap_dx[SBG_MAX_TAPS], tap_slab[SBG_MAX_TAPS];
    int accumulate;
    const float* bias; const float* noise; int64_t noise_stride_n;
    int act; float alpha, gain, clamp;
    /* Optional split of the reduction (taps x channels) over `ksplit` workgroups per output tile, for launches with too few
     * output tiles to fill the chip (the 4x4 / 8x8 blocks): partial fp32 results go to `workspace`
     * (>= sbg_conv2d_igemm_workspace() bytes) and a second kernel sums them in a fixed order into y (bitwise reproducible).
     * Needs a dense channel-minor y; a fused epilogue and a 16-bit output are applied by that second kernel (then without `accumulate`,
     * Cout % 8 == 0, y 16-byte aligned).  Whether and how far to split is the library's decision (fewer than 128 output tiles of 128 x 128,
     * at least 16 K-steps of 64 channels, Cout > 64: about 256 workgroups of at least four K-steps): ksplit 0 = the library chooses, 1 = never,
     * k > 1 = at most k; workspace == NULL = no split.  sbg_conv2d_igemm_workspace() returns the bytes of the split sbg_conv2d_igemm() will
     * use for the block when given a workspace (0 = none, -1 = a refused block). */
    void* workspace; int ksplit;
    /* Optional phases: nphase in 2..4 makes ONE launch compute several output sub-grids of the same input -- the s x s phases of a
     * stride-s transposed convolution, whose tiles then share the input through L2 instead of streaming it from HBM once per phase.
     * Phase i uses the next ph_ntaps[i] taps of the tap list (sum <= ntaps), the output grid ph_oh[i] x ph_ow[i] (instead of OH x OW)
     * and writes at y + ph_yoff[i] elements with the common ys_* strides.  nphase <= 1 = off.  No fused epilogue with phases, and they never split. */
    int nphase; int ph_ntaps[4], ph_oh[4], ph_ow[4]; int64_t ph_yoff[4];
} sbg_conv_params;
int64_t sbg_conv2d_igemm_workspace(const sbg_conv_params* p);
int     sbg_conv2d_igemm(const sbg_conv_params* p, sbg_stream_t stream);
/* The plan of a call, host only: one record per kernel launch sbg_conv2d_igemm(p) would make, in order (at most five; the slab reduction of a
 * split call is not one), as many as fit `max`; returns their number, or -1 for a refused block (sbg_last_error).  dims / flops / bytes are
 * what the launch log records (dims[6] = the code of the kernel and tile). */
typedef struct sbg_conv_launch_info {
    int dims[7]; double flops, bytes;
    int64_t grid_x; int grid_y, block, lds;
} sbg_conv_launch_info;
int     sbg_conv2d_igemm_plan(const sbg_conv_params* p, sbg_conv_launch_info* out, int max);


/* ------------------------------------------------------------------------------------------
 * Weight gradient (replaces `aten::cudnn_convolution_backward_weight` /
 * `..._transpose_backward_weight`, conv2d_gradfix.py:140-147):
 *
 *   out[t][ca][cb] = sum_{n, py, px} a[n, py, px, ca] * b[n, py*stride + dy[t], px*stride + dx[t], cb]
 *
 * a: [N, PH, PW, Ca], b: [N, BH, BW, Cb], both channel-minor with Ca % 8 == Cb % 8 == 0, same dtype;
 * out: fp32 [ntaps][Ca][Cb].  The pixel sum is split over `nsplit` workgroups that write fp32
 * partial slabs into `workspace` (>= sbg_conv2d_wgrad_workspace() bytes) and a second kernel reduces
 * them in a fixed order (bitwise reproducible). `accumulate` adds into the existing out. */
typedef struct sbg_wgrad_params {
    const void* a; const void* b; float* out; void* workspace;
    int dtype;
    int N, PH, PW, Ca, BH, BW, Cb;
    int64_t as_n, as_h, as_w;
    int64_t bs_n, bs_h, bs_w;
    int stride;
    int ntaps;
    int tap_dy[SBG_MAX_TAPS], tap_dx[SBG_MAX_TAPS];
    int accumulate;
} sbg_wgrad_params;
int64_t sbg_conv2d_wgrad_workspace(const sbg_wgrad_params* p);
int     sbg_conv2d_wgrad(const sbg_wgrad_params* p, sbg_stream_t stream);


/* ------------------------------------------------------------------------------------------
 * Per-sample channel scaling with optional per-pixel addend (the modulation `x * styles`, the demodulation
 * + noise `fma(x, dcoefs, noise)` of train_parts/generators.py:79-88 and stylegan2ada/torch_utils/ops/fma.py:15):
 *   y[n,c,p] = x[n,c,p] * a[n*C + c] (+ z[n*z_stride_n + p])         a, z: fp32; p = pixel index in [0, HW)
 * layout: 0 = planar [N][C][HW], 1 = channel-minor [N][HW][C]; x and y dense in that layout. */
int sbg_scale_nc(const void* x, const float* a, const float* z, void* y, int dtype, int layout,
                 int N, int C, int64_t HW, int64_t z_stride_n, sbg_stream_t stream);
/* Same with a per-sample, per-channel addend (the normalise-and-modulate step of biggan/layers.py `ccbn` / `bn` / `fused_bn`
 * :173-187,306-325 once the statistics are known):  y[n,c,p] = x[n,c,p] * a[n*C + c] + b[n*C + c]. */
int sbg_scale_shift_nc(const void* x, const float* a, const float* b, void* y, int dtype, int layout,
                       int N, int C, int64_t HW, sbg_stream_t stream);

/* Per-sample, per-channel dot product over pixels (the gradient of the scaling above w.r.t. `a`, and -- with
 * v == NULL -- the bias gradient `dx.sum([2, 3])` of bias_act.py:172-173):
 *   partial[s][n*C + c] = sum_{p in split s} u[n,c,p] * (v ? v[n,c,p] : 1)        partial: fp32 [nsplit][N][C]
 * The caller sums `partial` over s (fixed order => reproducible).  sbg_dot_hw_splits() returns nsplit. */
int sbg_dot_hw_splits(int layout, int N, int C, int64_t HW);
int sbg_dot_hw(const void* u, const void* v, float* partial, int dtype, int layout,
               int N, int C, int64_t HW, sbg_stream_t stream);
/* r[0][n*C + c] = sum over the H*W plane of x, r[1][n*C + c] = sum of x^2 -- both moments of a PLANAR tensor [N, C, H*W] in one pass (fp32
 * accumulation, fixed order).  The batch statistics of BigGAN's normalisation layers (biggan/layers.py:188-205 `manual_bn`,
 * sync_batchnorm/batchnorm.py:71-79: `input_sum`, `input_ssum`).  r: fp32 [2, N*C]. */
int sbg_moments_hw(const void* x, float* r, int dtype, int N, int C, int64_t HW, sbg_stream_t stream);

/* Many small fp32 matrix products in one launch (csrc/grouped_gemm.hip): the per-layer affine maps of a synthesis network
 * (train_parts/generators.py:333 `styles = self.affine(w)` in every SynthesisLayer / ToRGBLayer; FullyConnectedLayer.forward :117-131:
 * `torch.addmm(b.unsqueeze(0), x, w.t())` with the gains folded in) and their gradients -- ~20 + ~60 separate GEMM / reduction launches per
 * pass in the reference.  Problem p:  C[m][n] = sum_{t < nterms} alpha_t * sum_k A_t[m][k] B_t[k][n]  (+ bias[n] * bias_scale),
 * every operand addressed by element strides (row stride, column stride), so transposes and slices of larger tensors cost nothing;
 * `rowsum` (optional): rowsum[m] = rowsum_scale * sum_k A_0[m][k]  (the bias gradient next to the weight gradient).
 * fp32, fixed summation order (ascending k, term 0 then term 1).  Outputs of different problems must not overlap.
 * Empty extents are served: a problem with M = 0 or N = 0 writes nothing, a term with K = 0 adds nothing (C is then the bias or zeros);
 * the pointers of such empty tensors may be NULL. */
typedef struct sbg_gg_problem {
    const float *a0, *b0, *a1, *b1;         /* term 1 is ignored when nterms == 1 */
    float* c; const float* bias; float* rowsum;
    int64_t a0_rs, a0_cs, b0_rs, b0_cs, a1_rs, a1_cs, b1_rs, b1_cs, c_rs, c_cs;
    int M, N, K0, K1, nterms;
    float alpha0, alpha1, bias_scale, rowsum_scale;
} sbg_gg_problem;
int sbg_grouped_gemm(const sbg_gg_problem* problems, int count, sbg_stream_t stream);

/* Both gradients of y = x * a[n, c] (the style modulation in front of a convolution, train_parts/generators.py:79; autograd's
 * `dy * a` and `(dy * x).sum([2, 3])`) in ONE pass over u = dy and v = x, channel-minor tensors with C / 8 dividing 256:
 *   y[n,p,c] = u[n,p,c] * scale[n*C + c]     and     partial[s][n*C + c] as sbg_dot_hw(u, v). */
int sbg_dot_hw_scale_supported(int C);
int sbg_dot_hw_scale(const void* u, const void* v, const float* scale, void* y, float* partial, int dtype,
                     int N, int C, int64_t HW, sbg_stream_t stream);


/* Backward head of the fused modulated-convolution layer (train_parts/generators.py:79-88 + :328, i.e. modulated_conv2d's
 * `fma(x, dcoefs, noise)` followed by bias_act): with y = clamp(act(c * dcoef[n,o] + noise[n,p] + bias[o]) * gain) saved,
 * one pass over (dy, y) writes
 *   d2[n,o,p]            = d1 * dcoef[n,o],  d1 = dy * gain * (y > 0 ? 1 : alpha) * [|y| < clamp]   (bias_act.py:159-210)
 *   partial[0][s][n][o]  = sum_p d1                         (bias gradient)
 *   partial[1][s][n][o]  = sum_p d1 * (pre - noise - bias)  (dcoef[n,o] * demodulation gradient; pre is recovered from y)
 *   dnoise[n,p]          = sum_o d1                         (optional, NULL to skip)
 * Channel-minor [N][HW][C] tensors, C / 8 a power of two <= 64; partial: fp32 [2][nsplit][N][C], nsplit = sbg_dot_hw_splits(1, N, C, HW).
 * act in {linear, relu, lrelu}; clamp < 0 disables. */
int sbg_modconv_bwd_supported(int C);
int sbg_modconv_bwd(const void* dy, const void* y, const float* dcoef, const float* noise, const float* bias,
                    void* d2, float* partial, float* dnoise, int dtype, int N, int C, int64_t HW, int64_t noise_stride_n,
                    int act, float alpha, float gain, float clamp, sbg_stream_t stream);
/* Same, for a y that feeds a style-modulated convolution and nothing else (a synthesis block's conv0 output into its conv1, generators.py:462-463):
 * `dy` is then the gradient w.r.t. y * prescale[n, c] (what that convolution's data gradient delivers); the pass also takes
 * partial3[s][n*C + c] = sum_p dy * y (the gradient of prescale) and continues with dy * prescale -- autograd's `dy * s`, `(dy * x).sum([2, 3])` and the
 * backward head above in one pass over (dy, y). */
int sbg_modconv_bwd_prescaled(const void* dy, const void* y, const float* prescale, const float* dcoef, const float* noise, const float* bias,
                              void* d2, float* partial, float* partial3, float* dnoise, int dtype, int N, int C, int64_t HW,
                              int64_t noise_stride_n, int act, float alpha, float gain, float clamp, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Spectral norm, one power iteration with one singular vector (biggan/layers.py `power_iteration` :28-50, `SN.W_` :87-99):
 *   v = normalize(u W), u' = normalize(v W^T), sigma = (v W^T) . u'        W: fp32 [rows, cols] row-major, u: fp32 [rows]
 * Writes v [cols], u_new [rows] (both normalised with F.normalize's max(norm, eps)) and sigma [1]; `workspace` holds
 * sbg_sn_workspace(rows, cols) bytes.  The caller decides whether u_new replaces the stored u (training) -- nothing is
 * updated in place.  d sigma / d W = outer(u_new, v) is applied by the host autograd Function. */
int64_t sbg_sn_workspace(int rows, int cols);
int sbg_sn_power_iteration(const float* W, const float* u, float* v, float* u_new, float* sigma, void* workspace,
                           int rows, int cols, float eps, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Minibatch standard deviation (train_parts/discriminators.py:313-328): x fp32 [N, C, H, W] dense, N = G * M (sample g*M + m is in group m),
 * C = F * c.  y fp32 [N, C + F, H, W]: y[:, :C] = x and y[g*M + m, C + f] = mean_{cc,h,w} sqrt(var_g x[g*M + m, f*c + cc, h, w] + 1e-8).
 * sbg_mbstd_bwd: first-order dx from (x, dy).  One launch each (the reference: ~10 + ~14 tensor ops on a 1 MB tensor). */
int64_t sbg_mbstd_workspace(int N, int C, int HW, int G, int F);      /* bytes of partial sums sbg_mbstd_fwd needs */
int sbg_mbstd_fwd(const float* x, float* y, void* workspace, int N, int C, int HW, int G, int F, sbg_stream_t stream);
int sbg_mbstd_bwd(const float* x, const float* dy, float* dx, int N, int C, int HW, int G, int F, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * fp32 operands for the bf16 matrix cores: hi / mid / lo bf16 split of x, the parts concatenated along one axis in one pass.
 *   x: fp32 [outer, C, inner] dense;  y: bf16 [outer, nseg * C, inner];  y[o, s*C + c, i] = part_{order[s]}(x[o, c, i]),
 *   part_0 = bf16(x), part_1 = bf16(x - part_0), part_2 = bf16(x - part_0 - part_1);  nseg <= 8, order[s] in {0, 1, 2}.
 * (No counterpart in the reference: its fp32 layers go to cuDNN / oneDNN; here they run as six bf16 MFMA products with fp32 accumulation.) */
int sbg_split_bf16_cat(const float* x, void* y, int64_t outer, int64_t C, int64_t inner, int nseg, const int* order, sbg_stream_t stream);
/* the same split of a strided 4-D fp32 view (extents `shape`, element strides `xstrides`), written DENSELY in the view's dimension order with
 * dimension `cat_dim` holding the nseg parts side by side: y[.., s * shape[cat_dim] + d_cat, ..] = part order[s] of x[d].  Replaces the
 * reference's w.permute(..).contiguous() of an fp32 conv weight ahead of the launch (torch_utils/ops/conv2d_gradfix.py:94-146 hands cuDNN
 * the strided tensor). */
int sbg_split_bf16_cat_nd(const float* x, const int64_t* shape, const int64_t* xstrides, int cat_dim, void* y, int nseg, const int* order, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Non-local self-attention core (biggan/layers.py `Attention.forward` :162-166): for every sample n
 *   out[n, q, :] = softmax_m( theta[n, q, :] . phi[n, m, :] ) @ g[n, m, :]
 * theta: fp32 [N, Q, D], phi: fp32 [N, M, D], g: fp32 [N, M, DV], out: fp32 [N, Q, DV], all row-major dense.
 * Exact-fp32 matrix-core kernel (v_mfma_f32_16x16x4_f32); the [Q, M] attention map never touches HBM.
 * M <= 256: the whole key strip of a wave's 16 queries is held at once (M / 16 in {1, 2, 4, 8, 16}).  M > 256: the keys are walked in chunks
 * with a running maximum, sum and output per row (online softmax), one division at the end; any M % 16 == 0.
 * Supported (sbg_attention_supported returns 1 for exactly the shapes sbg_attention_fwd serves): Q % 16 == 0, M % 16 == 0, D % 4 == 0,
 * DV % 16 == 0; for M <= 256, M / 16 in {1, 2, 4, 8, 16} (M = 48, 80, 96, ... 240 are refused); for M > 256, per-sample matrices of at most
 * 2^31 - 1 elements (M * max(D, DV), Q * max(D, DV)). */
int sbg_attention_supported(int Q, int M, int D, int DV);
int sbg_attention_fwd(const float* theta, const float* phi, const float* g, float* out, int N, int Q, int M, int D, int DV,
                      sbg_stream_t stream);
/* First-order gradients of the same expression (what autograd derives from the reference's bmm / softmax / bmm, layers.py:162-166):
 *   dg = P^T dout,  dS = P o (dout g^T - rowsum(dout o out)),  dtheta = dS phi,  dphi = dS^T theta,   P = softmax(theta phi^T)
 * recomputed from theta / phi / g in two passes (per query tile, per key tile); the [Q, M] map never touches HBM and every sum over
 * queries stays inside one wave (fixed order).  workspace: sbg_attention_bwd_workspace(N, Q) bytes of row statistics.
 * M > 256 takes three launches: the forward recomputed in registers for lse and delta = rowsum(dout o out) (nothing of the forward is saved),
 * dtheta streamed over the key chunks from those statistics, then the same per-key-tile pass as M <= 256.
 * Supported (sbg_attention_bwd_supported): the forward's shapes with ceil(D / 16) in {1, 2, 4} (D <= 16, 20 .. 32, 52 .. 64) and
 * DV / 16 in {1, 2, 4, 8, 16}. */
int sbg_attention_bwd_supported(int Q, int M, int D, int DV);
int64_t sbg_attention_bwd_workspace(int N, int Q);
int sbg_attention_bwd(const float* theta, const float* phi, const float* g, const float* dout, float* dtheta, float* dphi, float* dg,
                      void* workspace, int N, int Q, int M, int D, int DV, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * fp32 master weights <-> packed convolution operands.  Replaces the per-call framework chain `w = self.weight * weight_gain`,
 * `w.to(x.dtype)` (train_parts/generators.py:176-179, discriminators.py:115-118) + layout change, and its autograd mirror.
 *   sbg_pack_weight:  out[t][a][b] = cast(w[a*sA + b*sB + kh*sKH + kw*sKW] * gain), t = kh*KW + kw, b zero-padded to Bp; `out` is the
 *                     `w` operand of sbg_conv2d_igemm ([slab][Cout][Cin]); optional w2[a][b] = sum_t (w*gain)^2 (fp32 [A][B], the
 *                     demodulation's sum over taps, generators.py:71-76).
 *   sbg_unpack_wgrad: dw[a*sA + b*sB + kh*sKH + kw*sKW] = gain * dwp[t*tap_stride + a*row_stride + b]  (+ 2 gain^2 w[...] dw2[a][b]
 *                     when dw2 != NULL; dwp may then be NULL): sbg_conv2d_wgrad's fp32 result in the parameter's own layout. */
int sbg_pack_weight(const float* w, void* out, int out_dtype, int A, int B, int KH, int KW,
                    int64_t sA, int64_t sB, int64_t sKH, int64_t sKW, int Bp, float gain, float* w2, sbg_stream_t stream);
int sbg_unpack_wgrad(const float* dwp, int64_t dwp_tap_stride, int64_t dwp_row_stride, float* dw, const float* w, const float* dw2,
                     int A, int B, int KH, int KW, int64_t sA, int64_t sB, int64_t sKH, int64_t sKW, float gain, sbg_stream_t stream);

/* Demodulation coefficients of a modulated convolution from the tap-summed squared weights w2 [O][I] (sbg_pack_weight's by-product):
 *   dcoefs[n, o] = rsqrt(sum_i styles[n, i]^2 * w2[o, i] + eps)        (train_parts/generators.py:71-76: `(w * s).square().sum([2,3,4]) + 1e-8).rsqrt()`
 * and the first-order gradient: g = d loss / d dcoefs -> dstyles [N][I], dw2 [O][I] (either may be NULL).  All fp32, dense. */
int sbg_demod_coefs(const float* styles, const float* w2, float* dcoefs, int N, int O, int I, float eps, sbg_stream_t stream);
int sbg_demod_coefs_bwd(const float* g, const float* dcoefs, const float* styles, const float* w2, float* dstyles, float* dw2,
                        int N, int O, int I, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * ToRGB layer (train_parts/generators.py:344-348: modulated 1x1 convolution without demodulation to <= 4 channels + linear bias_act
 * with clamp) as streaming kernels over channel-minor 16-bit x [N, HW, C]:
 *   fwd: y[n, o, p] = clamp(sum_c x[n, p, c] * wmod[n, o, c] + bias[o])      y fp32 planar [N, O, HW]; wmod = w[o, c] * styles[n, c], fp32
 *   bwd: d1 = dy masked by the clamp (from the saved y);  dx[n, p, c] = sum_o d1 * wmod  (may be NULL);
 *        partial[n][blk][o * C + c] = per-workgroup sums of d1[o, p] * x[p, c], then O sums of d1 -- the caller adds the
 *        sbg_torgb_bwd_blocks(N, C, HW) slabs in a fixed order (reproducible) to get d wmod [N, O, C] and d bias.
 * C = 8 * 2^k <= 512, O <= 4 (sbg_torgb_supported).  clamp < 0 disables clamping. */
int sbg_torgb_supported(int C, int O);
int sbg_torgb_bwd_blocks(int N, int C, int64_t HW);
int sbg_torgb_fwd(const void* x, const float* wmod, const float* bias, float* y, int dtype, int N, int C, int O, int64_t HW,
                  float clamp, sbg_stream_t stream);
int sbg_torgb_bwd(const void* x, const float* wmod, const float* dy, const float* y, void* dx, float* partial, int dtype,
                  int N, int C, int O, int64_t HW, float clamp, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * fromRGB layer of the discriminator (train_parts/discriminators.py:270-277 -> Conv2dLayer :115-124: 1x1 convolution from <= 4 image
 * channels + bias + activation * gain + clamp) as streaming kernels.  img fp32 planar [N, Ci, HW]; w fp32 [Co][Ci] (weight * weight_gain);
 * y 16-bit channel-minor [N, HW, Co]; act in {linear, relu, lrelu}.
 *   fwd: y = clamp(act(sum_c img * w + bias) * gain)
 *   bwd: d1 = dy * d(clamp(act(.) * gain)) from the saved y;  partial[n][blk][co * Ci + c] = per-workgroup sums of d1 * img, then Co sums of
 *        d1 (the caller adds the sbg_fromrgb_bwd_blocks(N, HW) slabs in a fixed order);  dimg[n, c, p] = sum_co d1 * w (NULL = not wanted). */
int sbg_fromrgb_supported(int Ci, int Co, int act);
int sbg_fromrgb_bwd_blocks(int N, int64_t HW);
int sbg_fromrgb_fwd(const float* img, const float* w, const float* bias, void* y, int dtype, int N, int Ci, int Co, int64_t HW,
                    int act, float alpha, float gain, float clamp, sbg_stream_t stream);
int sbg_fromrgb_bwd(const float* img, const float* w, const void* dy, const void* y, float* dimg, float* partial, int dtype,
                    int N, int Ci, int Co, int64_t HW, int act, float alpha, float gain, float clamp, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * ADA augmentation pipe, device ops (train_parts/augmentations.py:121-433).
 *
 * grid_sample: bilinear, zero padding, align_corners = False -- the one mode of the reference's
 * `grid_sample_gradfix.grid_sample(input, grid)` (stylegan2ada/torch_utils/ops/grid_sample_gradfix.py:24-27,45), whose
 * backward is `aten::grid_sampler_2d_backward(grad_output, input, grid, 0, 0, False)` (:63-64).
 * fp32 planar tensors with element strides.  Sampling positions come from `grid` (fp32 [N, OH, OW, 2] dense, normalised
 * coordinates) or, when `grid` is NULL, from `theta` (fp32 [N, 2, 3]): the positions `F.affine_grid(theta, [N, C, OH, OW],
 * align_corners=False)` would produce (augmentations.py:299) are generated inside the kernel.
 *   sbg_grid_sample2d:      y[n, c, oy, ox]  = sum over the 4 neighbours of x weighted bilinearly (x, y required)
 *   sbg_grid_sample2d_bwd:  dx += scatter of dy (dx must be zeroed by the caller; fp32 atomics); if dgrid != NULL also
 *                           dgrid[n, oy, ox, 2] (needs x).  dy shares y's strides, dx shares x's. */
typedef struct sbg_grid_sample_params {
    const void* x; const float* grid; const float* theta; const void* dy;
    void* y; void* dx; float* dgrid;
    int N, C, IH, IW, OH, OW;
    int64_t xs_n, xs_c, xs_h, xs_w;
    int64_t ys_n, ys_c, ys_h, ys_w;
    const float* theta_host;            /* optional HOST copy of theta: lets _bwd pick the deterministic gather kernel */
} sbg_grid_sample_params;
int sbg_grid_sample2d(const sbg_grid_sample_params* p, sbg_stream_t stream);
int sbg_grid_sample2d_bwd(const sbg_grid_sample_params* p, sbg_stream_t stream);
/* 1 when _bwd will take the gather kernel for these parameters: affine positions (theta + theta_host, no grid, no dgrid, C <= 4)
 * whose per-pixel candidate box is small.  That kernel OVERWRITES every element of dx (no zero fill needed, no atomics, bitwise
 * reproducible); otherwise _bwd accumulates into a caller-zeroed dx with fp32 atomics. */
int sbg_grid_sample2d_bwd_overwrites(const sbg_grid_sample_params* p);

/* Per-sample colour transform of dense planar fp32 RGB images x [N, 3, HW]: y[n, c, :] = sum_c' M[n, c, c'] x[n, c', :] + M[n, c, 3]
 * with M fp32 [N, 3, 4] -- `C[:, :3, :3] @ images + C[:, :3, 3:]` (augmentations.py:352-354).  Its data gradient is the same call
 * with the transposed 3x3 block and a zero fourth column. */
int sbg_color_transform(const float* x, const float* M, float* y, int N, int64_t HW, sbg_stream_t stream);

/* Per-sample 1-D correlation of M dense fp32 planes [M, H, W] along W (axis 0) or H (axis 1):
 *   y[m, .., o] = sum_t x[m, .., o + t - pad] * taps[m / planes_per_filter][flip ? T-1-t : t]      (zeros outside)
 * = one of the two grouped convolutions of the image-space filter, `conv2d(images, Hz_prime.unsqueeze(2 or 3),
 * groups=batch*channels)` (augmentations.py:388-389); with flip = 1 and pad = T - 1 - pad_fwd it is their data gradient.
 * Output extent along the axis: L + 2*pad - T + 1. */
int sbg_filter1d_batch(const float* x, const float* taps, float* y, int M, int H, int W, int T, int axis, int pad,
                       int planes_per_filter, int flip, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Perceptual path length sampler arithmetic (metrics/perceptual_path_length.py of the reference), all fp32, dense rows.
 * Each writes the [2B, ...] synthesis / detector batch in one launch: rows 0..B-1 at t[b], rows B..2B-1 at t[b] + eps (fp32 add).
 *   sbg_ppl_slerp_endpoints: out[r] = slerp(z0[b], z1[b], t_r) for z0, z1 [B, D] -- `slerp` (:23-32): both inputs normalised, the
 *                            angle from acos of their dot product, the orthogonalised second axis normalised, the result renormalised;
 *                            one wave per row, every norm and dot product a wave reduction.  Replaces `slerp(z0, z1, t)` and
 *                            `slerp(z0, z1, t + eps)` (:64-65) and their `torch.cat`.
 *   sbg_ppl_lerp_endpoints:  out[r] = torch.lerp(w0[b], w1[b], t_r) over [B, L = num_ws * w_dim] with torch's two-branch formula
 *                            (|weight| < 0.5 ? s + w (e - s) : e - (e - s)(1 - w)) -- `w0.lerp(w1, t)` / `w0.lerp(w1, t + eps)` (:59-60). */
int sbg_ppl_slerp_endpoints(const float* z0, const float* z1, const float* t, float eps, float* out, int B, int D, sbg_stream_t stream);
int sbg_ppl_lerp_endpoints(const float* w0, const float* w1, const float* t, float eps, float* out, int B, int64_t L, sbg_stream_t stream);
/* Synthesis output -> detector input (:77-89): img fp32 [N, C, H, W] with element strides (any memory format) -> out fp32 dense
 * [N, C == 1 ? 3 : C, S, S]: the optional centre crop (rows [3c, 7c), columns [2c, 6c), c = H / 8; needs H == W), the area mean over
 * factor x factor boxes (`reshape(...).mean([3, 5])`, skipped for factor 1), then (x + 1) * 127.5 and the grey -> RGB repeat.
 * Mean and scale round separately, in the reference's order.  The window must split into whole boxes. */
int sbg_ppl_prep_images(const float* img, float* out, int N, int C, int H, int W, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                        int crop, int factor, sbg_stream_t stream);
/* Differential LPIPS distance (:92-93, `(lpips_t0 - lpips_t1).square().sum(1) / epsilon ** 2`): feats fp32 [2B, F] dense ->
 * dist[b] = (sum_f (feats[b, f] - feats[B + b, f])^2) / eps2, eps2 = the fp32 value of epsilon^2, one division at the end.
 * Two launches: per-(row, chunk) partial sums into `workspace` (sbg_ppl_dist_workspace(B, F) bytes), then a fixed-order sum per
 * row.  No float atomics: the result is the same on every run. */
int64_t sbg_ppl_dist_workspace(int B, int64_t F);
int sbg_ppl_dist(const float* feats, float* dist, void* workspace, int B, int64_t F, float eps2, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Latent projector arithmetic (stylegan2ada/projector.py of the reference, `project()` :25-131), all fp32.  No float atomics; every
 * sum has a fixed order, so two runs on the same inputs give the same bits.  No allocation or synchronisation inside: workspaces
 * come from the caller (sizes from the *_workspace queries, -1 for an unsupported input).
 * The noise entries take the whole set of noise buffers as a host table: bufs[b] -> dense, 16-byte aligned fp32 [res[b], res[b]],
 * res[b] a power of two in [4, 1024], 1 <= nbuf <= 32; any other set is an error.  Levels of a buffer: level 0 is the buffer, level
 * k + 1 = avg_pool2d(level k, 2), down to the first side <= 8 (the reference's loop, :104-113).
 *   sbg_proj_noise_reg:      means[2l], means[2l + 1] = mean(P * roll(P, 1, W)), mean(P * roll(P, 1, H)) of level l of the flat
 *                            (buffer, level) list; reg[0] = sum of every mean^2 in that order.  The pooled levels stay in
 *                            `workspace` for the backward.  3 launches.
 *   sbg_proj_noise_reg_bwd:  grads[b] = g[0] * sum_k G_k[y >> k, x >> k] / 4^k with G_k[i, j] = 2 (m_x (P[i, j-1] + P[i, j+1]) +
 *                            m_y (P[i-1, j] + P[i+1, j])) / n^2 (indices wrap); reads the forward's means and workspace.  1 launch.
 *   sbg_proj_noise_normalize: in place, buf -= mean(buf); buf *= rsqrt(mean(buf^2)) (:125-129).  2 launches.
 * sbg_proj_sqdist: dist[0] = sum_f (t[f] - s[f])^2 (the LPIPS term, :98), two stages.  sbg_proj_sqdist_bwd: ds = 2 g[0] (s - t). */
int64_t sbg_proj_noise_reg_workspace(const int* res, int nbuf);
int sbg_proj_noise_reg(const float* const* bufs, const int* res, int nbuf, float* means, float* reg, void* workspace, sbg_stream_t stream);
int sbg_proj_noise_reg_bwd(const float* const* bufs, float* const* grads, const int* res, int nbuf, const float* means, const float* g,
                           const void* workspace, sbg_stream_t stream);
int64_t sbg_proj_noise_normalize_workspace(const int* res, int nbuf);
int sbg_proj_noise_normalize(float* const* bufs, const int* res, int nbuf, void* workspace, sbg_stream_t stream);
int64_t sbg_proj_sqdist_workspace(int64_t F);
int sbg_proj_sqdist(const float* t, const float* s, float* dist, void* workspace, int64_t F, sbg_stream_t stream);
int sbg_proj_sqdist_bwd(const float* t, const float* s, const float* g, float* ds, int64_t F, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Image export: the float -> uint8 step and the grid layout of the reference's image writers, and the latent table of its style
 * matrix.  One launch each, no workspace.
 *
 * sbg_img_quantize_tile: img fp32 [N, C, H, W], C = 1 or 3, with element strides >= 0 (any memory format, slices) -> bytes in the
 * caller's HWC canvas uint8 [gh * H, gw * W, C].  Image n fills cell k = cell0 + n, rows [k / gw * H, +H), columns [k % gw * W, +W);
 * cell0 + N <= gw * gh, cells outside that run are not touched, so several calls fill one canvas.  Every float is read once and
 * every byte written once.  `rule` selects the quantisation:
 *   SBG_QUANT_GRID   `save_image_grid` (train_parts/trainers.py:102-106): v = (x - lo) * scale as two rounded fp32 operations,
 *                    round half to even, clip to [0, 255].  scale = 255 / (hi - lo), computed by the caller in double and rounded
 *                    to float (what numpy does with the Python scalar).
 *   SBG_QUANT_CLAMP  stylegan2ada/generate.py:98,120 and style_mixing.py:79,88: v = x * 127.5 + 128 as a rounded multiply and a
 *                    rounded add (no fused multiply-add), clamp to [0, 255], truncate.  lo and scale are ignored.
 * The two differ on ties.  Non-finite values, which the reference leaves undefined: a NaN (in x or in v) writes 0, +inf and -inf
 * clamp like any other value outside the range.
 * W % 4 == 0 with 16-byte aligned rows (planar, or channel-minor with C = 3) takes four pixels per work-item: 16-byte loads,
 * 4-byte stores; anything else takes one pixel per work-item.
 *
 * sbg_ws_truncate_mix: W fp32 [S, L, D] dense, w_avg fp32 [D] -> out fp32 [R * Cn, L, D] dense,
 *   out[r * Cn + c, l] = T[mask[l] ? cols[c] : rows[r], l],  T = w_avg + (W - w_avg) * psi
 * evaluated in that order as three rounded fp32 operations (style_mixing.py:74; not torch.lerp).  rows [R], cols [Cn] and mask [L]
 * are int32 arrays on the device; an index outside [0, S) is never dereferenced: its rows of `out` are filled with NaN.  With
 * rows = 0..S-1, Cn = 1 and a zero mask the result is T itself. */
enum sbg_quant_rule { SBG_QUANT_GRID = 0, SBG_QUANT_CLAMP = 1 };
int sbg_img_quantize_tile(const float* img, uint8_t* canvas, int N, int C, int H, int W, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                          int gw, int gh, int cell0, int rule, float lo, float scale, sbg_stream_t stream);
int sbg_ws_truncate_mix(const float* W, const float* w_avg, float psi, const int* rows, const int* cols, const int* mask, float* out,
                        int S, int L, int D, int R, int Cn, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Exact uint8 resampling: the two passes of PIL's `Image.resize` on 8-bit images (its `ImagingResampleHorizontal_8bpc` /
 * `ImagingResampleVertical_8bpc`), which is the arithmetic of the reference's stylegan2ada/dataset_tool.py (`make_transform`, :199-248:
 * `img.resize((w, h), LANCZOS | BOX)`).  Integer arithmetic only, so the result is the same bytes as PIL's.
 * Images are uint8 with interleaved channels, [N, rows, width, C], C = 1 or 3; image n starts at `+ n * img_stride`, row y at
 * `+ y * pitch` (bytes).  A crop box is the caller's pointer offset and extent: `src` may start at any byte.
 * Tables (int32, on the device), one window per output index i of the resampled axis: bounds[2 i] = first input index,
 * bounds[2 i + 1] = count <= ksize, and `count` coefficients with 22 fractional bits.
 *   out = clamp((2^21 + sum_k in[first + k] * coeff[k]) >> 22, 0, 255),  the sum in wrapping int32, the shift arithmetic.
 * A window that leaves the input extent (a table that does not belong to these sizes) is clipped, never dereferenced.
 *
 * sbg_u8_resample_h: every row of [N, rows, in_w, C] -> [N, rows, out_w, C].  `coeffs_t` is tap-major, int32 [ksize, out_w].  A
 * workgroup stages the input span of `strip` consecutive output pixels of a row in LDS (dword loads, bytes at the unaligned ends) and
 * each work-item sums one output pixel from it; `strip` is a power of two in [16, 256] and `span` the largest number of input pixels
 * any strip's windows cover, both chosen by the caller from the table (the span must fit 60 KiB of LDS).  `dst` may have any pitch.
 * sbg_u8_resample_v: every column of [N, in_h, row_bytes] -> [N, out_h, row_bytes], a row being a flat array of row_bytes = width * C
 * bytes.  `coeffs` is int32 [out_h, ksize].  A work-item owns one dword of an output row: `dst`, `dst_pitch` and `dst_img_stride` must
 * be multiples of 4 and dst_pitch >= row_bytes rounded up to 4 (the pad bytes of a row are written, with unspecified values).  `src`
 * is read as dwords when its base, pitch and image stride are multiples of 4 and the pitch covers the rounded row (then up to 3 bytes
 * behind the end of a row are read, the last row's included: they lie inside the row's pitch), else as guarded bytes. */
int sbg_u8_resample_h(const uint8_t* src, int64_t src_img_stride, int64_t src_pitch, uint8_t* dst, int64_t dst_img_stride, int64_t dst_pitch,
                      int N, int rows, int in_w, int out_w, int C, const int* bounds, const int* coeffs_t, int ksize, int strip, int span,
                      sbg_stream_t stream);
int sbg_u8_resample_v(const uint8_t* src, int64_t src_img_stride, int64_t src_pitch, uint8_t* dst, int64_t dst_img_stride, int64_t dst_pitch,
                      int N, int row_bytes, int in_h, int out_h, const int* bounds, const int* coeffs, int ksize, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * k-nearest-neighbour arithmetic of the precision / recall metric (metrics/precision_recall.py of the reference) over fp16 feature
 * matrices, dense rows of F elements, as an implicit rows x manifold GEMM on the matrix cores; the [R, C] distance matrix is never
 * written.  n(x) = sum x_f^2 and s(x, y) = sum x_f y_f are fp32 sums of fp16 products, d2 = max((n(x) + n(y)) - 2 s, 0) in fp32,
 * d = fp16_rn(sqrt_f32(d2)); selection and comparison happen on these fp16 values.
 *   sbg_knn_kth_radius:  out[i] (fp16 [R]) = the (k + 1)-th smallest d(rows[i], manifold[j]) over j -- `dist.kthvalue(nhood_size + 1)`;
 *                        when `rows` is a slice of `manifold` the self-distance takes part, as in the reference.
 *   sbg_knn_in_manifold: out[i] (uint8 [P]) = 1 when d(probes[i], manifold[j]) <= radius[j] (fp16 [C]) for some j -- `(dist <= kth).any(dim=1)`.
 *   sbg_knn_probe:       count[i] (int32 [P]) = the number of j with d(probes[i], manifold[j]) <= radius[j], nearest[i] (fp16 [P]) =
 *                        min_j d(probes[i], manifold[j]) (the minimum is taken on d2 and rounded once): the pass behind density and
 *                        coverage (Naeem et al., "Reliable Fidelity and Diversity Metrics for Generative Models", ICML 2020), whose
 *                        `count > 0` is sbg_knn_in_manifold's flag.  Comparisons are `<=` as above; the published code compares with
 *                        `<`, which differs on exact ties only.  Argument rules of sbg_knn_in_manifold; workspace of
 *                        sbg_knn_probe_workspace(P, C) bytes: up16(4 P) + up16(4 C) + (runs > 1 ? 8 P runs : 0), one {int32 count,
 *                        float d2} pair per (run, row).
 * k + 1 <= 8, C >= k + 1, F a multiple of 8, features and workspace 16-byte aligned; anything else is an error.  The manifold columns
 * are split over workgroups when the rows alone do not fill the chip; partial results go through `workspace`
 * (sbg_knn_workspace(R, C, k, membership) bytes, -1 for unsupported sizes: the norms, R + C floats, and per (row, run) a list of 4 | 8
 * floats for the radius or one byte for the membership, where k is ignored) and are merged by a second launch in a fixed order.  No
 * atomics: two runs give the same bits. */
int64_t sbg_knn_workspace(int R, int C, int k, int membership);
int sbg_knn_kth_radius(const void* rows, const void* manifold, int R, int C, int64_t F, int k, void* out, void* workspace, sbg_stream_t stream);
int sbg_knn_in_manifold(const void* probes, const void* manifold, const void* radius, int P, int C, int64_t F, uint8_t* out, void* workspace,
                        sbg_stream_t stream);
int64_t sbg_knn_probe_workspace(int P, int C);
int sbg_knn_probe(const void* probes, const void* manifold, const void* radius, int P, int C, int64_t F, int32_t* count, void* nearest,
                  void* workspace, sbg_stream_t stream);
/* Nearest manifold rows in feature space (the --space=vgg16 search of nearest_neighbors.py), same kernels and arithmetic: for query q
 * the k rows j with the smallest d2(q, j), ascending by (d2, j) so a tie goes to the lower row: d2 fp32 [Q, k] (the fp32 value itself,
 * nothing is rounded to fp16), index int32 [Q, k].  Row exclude[q] (int32 [Q] on the device, or NULL) is skipped when it lies in
 * [0, M); it is the only row skipped, a duplicate of it elsewhere is a hit.  1 <= k <= 8; M >= k, and M >= k + 1 when `exclude` is
 * given; Q, M <= 2^24; F a multiple of 8; dense 16-byte aligned rows and workspace (sbg_knn_topk_workspace(Q, M, k) bytes, -1 for
 * unsupported sizes: the norms and, when the manifold is split, per (row, run) a list of 1 | 4 | 8 64-bit keys bits(d2) << 32 | row).
 * Anything else is an error.  Non-finite features are outside the definition (a NaN d2 becomes 0).  No atomics, and keys of distinct
 * rows are distinct: two calls give the same bits. */
int64_t sbg_knn_topk_workspace(int Q, int M, int k);
int sbg_knn_topk(const void* queries, const void* manifold, int Q, int M, int64_t F, int k, const int32_t* exclude, float* d2, int32_t* index,
                 void* workspace, sbg_stream_t stream);
/* Per-probe realism score (Kynkaanniemi et al., "Improved Precision and Recall Metric for Assessing Generative Models", NeurIPS 2019,
 * section 5; the reference has no such pass), same kernels and arithmetic, on the fp16 d of the membership test.  With radius fp16 [C]
 * (negative: the point is pruned and takes no part) and exclude int32 [P] on the device or NULL (a manifold index, or -1 for none):
 *   eligible(i, j) = radius[j] >= 0 and j != exclude[i]
 *   q(i, j) = +inf when d(i, j) == 0 (also at radius 0), else float(radius[j]) / float(d(i, j)): one IEEE fp32 division (a radius of -0
 *             counts as +0)
 *   score[i] (fp32 [P]) = max of q(i, j) over the eligible j, 0 when there is none;
 *   index[i] (int32 [P]) = the lowest eligible j attaining it, -1 when there is none.
 * Without `exclude`, score >= 1 is exactly sbg_knn_in_manifold's flag.  P, C in [1, 2^24]; F a multiple of 8; dense 16-byte aligned rows
 * and workspace; only `exclude` may be NULL; anything else is SBG_ERR_INVALID and launches nothing.  Workspace of
 * sbg_knn_realism_workspace(P, C) bytes (-1 for unsupported sizes): up16(4 P) + up16(4 C) + (runs > 1 ? 8 P runs : 0), one 64-bit key
 * bits(score) << 32 | ~j per (run, row), merged by an unsigned maximum.  No atomics, and keys of distinct columns are distinct: any
 * split and any two calls give the same bits. */
int64_t sbg_knn_realism_workspace(int P, int C);
int sbg_knn_realism(const void* probes, const void* manifold, const void* radius, int P, int C, int64_t F, const int32_t* exclude, float* score,
                    int32_t* index, void* workspace, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * End of a training phase over a flat fp32 gradient bucket: the reference's per-parameter loop `misc.nan_to_num(param.grad, nan=0,
 * posinf=1e5, neginf=-1e5, out=param.grad)` (train_parts/trainers.py:745-747), the 1/world averaging of a data-parallel exchange and
 * the gradient-health statistics of the run log, in one pass over the bucket.  For flat[0..n) and a scale s:
 *   y = x * s (one fp32 multiply, skipped when s == 1.0f);  z = isnan(y) ? +0 : y == +inf ? 1e5f : y == -inf ? -1e5f : y;  flat[i] = z;
 *   count = #{i : y_i not finite},  sumsq = sum (double)z_i * (double)z_i,  absmax = max |z_i|.
 * Every workgroup owns a contiguous chunk whose length depends on n alone, never on the device (4096 * ceil(n / 2^24) elements, so
 * at most 4096 chunks), and writes one float64 record [count, sumsq, absmax] to `partials`; the sums inside a workgroup follow
 * csrc/reduce.h.
 *   sbg_grad_finish_records (trainers.py:745-747): host only; the number of records a sweep over n elements writes
 *                           (ceil(n / chunk); 0 for n == 0, -1 for n < 0).  The largest n with one record is the chunk length of every n <= 2^24.
 *   sbg_grad_finish_sweep   (trainers.py:745-747): the pass above.  `flat` must be 16-byte aligned (an error otherwise, never a slower
 *                           path), `partials` holds 3 * records doubles.
 *   sbg_grad_finish_merge   (trainers.py:745-747): one workgroup adds `records` consecutive records into result[0..3) (count and
 *                           sumsq added, absmax maximised) in an order fixed by `records` alone: lane t of its 256 adds records t, t + 256, ...
 *                           in ascending order, the lanes are added as in csrc/reduce.h.  The records of several sweeps laid out back to back are merged
 *                           by one call; records == 0 gives zeros.
 * No atomics, two launches instead of an in-kernel finish: two runs give the same bits. */
int64_t sbg_grad_finish_records(int64_t n);
int sbg_grad_finish_sweep(float* flat, int64_t n, float scale, double* partials, sbg_stream_t stream);
int sbg_grad_finish_merge(const double* partials, int64_t records, double* result, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A training batch out of a device-resident uint8 image store.  Replaces, per step, the reference's host input path: the item read of
 * train_parts/datasets.py `Dataset.__getitem__` (:78-83; `image[:, :, ::-1]` for a mirrored item), the stock DataLoader's collate and
 * PCIe copy, and the normalisation `img.to(torch.float32) / 127.5 - 1` of train_parts/trainers.py:716.
 * `store` is dense uint8 [S, C, H, W]; `slot` int32 [B]; `flip` uint8 [B] or NULL (nothing mirrored).
 *   out_f32 = 0:  out uint8 [B, C, H, W],  out[b, c, y, x] = store[slot[b], c, y, flip[b] ? W - 1 - x : x]
 *   out_f32 = 1:  out fp32  [B, C, H, W],  lut[that byte], `lut` being 256 floats on the device (ignored for uint8 output)
 * The kernel does no floating-point arithmetic: the caller supplies the 256 values, evaluated by whatever expression and on whatever
 * device the consumer would have used, so the result has that expression's bits (the table sits in LDS).  Image offsets are 64-bit.
 * A slot outside [0, S) is never dereferenced: that image of `out` is NaN (fp32) or 0 (uint8), as for the row indices of the
 * truncate-mix kernel above.  With W % 4 == 0, `store` 4-byte aligned and `out` 16-byte aligned (4-byte for uint8) a work-item moves
 * 4 pixels of a row (one dword load, byte-reversed from column W - 4 - x when mirrored; one 16-byte or dword store); otherwise one
 * pixel with byte loads.  An fp32 `out` must be 4-byte aligned in either case; C * H * W may be at most 2^31 - 257. */
int sbg_u8_gather_images(const uint8_t* store, int64_t S, int C, int H, int W, const int32_t* slot, const uint8_t* flip, int B, void* out,
                         int out_f32, const float* lut, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Exact nearest stored images of uint8 queries (the search behind nearest_neighbors.py; the reference has no counterpart).
 * `queries` uint8 [Q, F], `store` uint8 [M, F], dense 16-byte aligned rows.  For query q: the k rows j with the smallest
 *   d2(q, j) = sum_f (queries[q, f] - store[j, f])^2,   an exact integer,
 * sorted ascending by (d2, j), so ties go to the lower j: d2 int64 [Q, k], index int32 [Q, k].  Row exclude[q] (int32 [Q] on the device,
 * or NULL) is skipped when it lies in [0, M); it is the only row skipped, a duplicate of it elsewhere in the store is a hit.
 * Arithmetic: bytes are re-centred (a - 128) and multiplied on the i8 matrix cores with i32 accumulators whose upper 16 bits are moved
 * into a second sum before they can overflow; the norms and d2 = n(q) + n(x) - 2 s are int64.  The result is exact for every input inside the limits:
 * 1 <= k <= 8; M >= k, and M >= k + 1 when `exclude` is given; Q, M <= 2^24; F a multiple of 16 in [16, 3 * 2^20].  Anything else is an
 * error, never another path.  The store's tiles are split over workgroups when the queries alone do not fill the chip; the partial
 * lists go through `workspace` (sbg_u8_nn_workspace(Q, M, k) bytes, 16-byte aligned; -1 for unsupported sizes) and are merged by a
 * second launch in index order.  The split is a function of the shape alone and there are no atomics: two calls give the same bits. */
int64_t sbg_u8_nn_workspace(int Q, int M, int k);
int sbg_u8_nn_topk(const uint8_t* queries, const uint8_t* store, int Q, int M, int64_t F, int k, const int32_t* exclude, int64_t* d2,
                   int32_t* index, void* workspace, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * DiffAugment (Zhao et al., "Differentiable Augmentation for Data-Efficient GAN Training", NeurIPS 2020: colour, translation, cutout)
 * in front of the discriminator, fused: fp32 dense [N, C, H, W], C = 1..4, rows are axis 2 and columns axis 3.
 * `table` is the packed per-sample parameter table, int32 [N, SBG_DIFFAUG_WORDS] on the device, 4-byte aligned; words of sample n:
 *   0 b   1 s   2 k        brightness, saturation, contrast: the bit patterns of three fp32 values
 *   3 t_row   4 t_col      translation, int32:  y[i, j] = x[i + t_row, j + t_col]
 *   5 r0  6 r1  7 c0  8 c1 cutout rectangle, int32, half-open: rows [r0, r1) x columns [c0, c1) of the OUTPUT are zeroed
 *   9..11                  unused (a sample's entry is 48 bytes)
 * Any integers are safe: a shift of the extent or more gives zeros, a rectangle is clipped to the image, r1 <= r0 or c1 <= c0 is empty.
 * Forward, with M = mean(x[n]) + b: an output pixel (i, j) outside the rectangle whose source (p, q) = (i + t_row, j + t_col) is inside
 * the image is   v = x[:, p, q] + b;  v <- s v + (1 - s) mean_c(v);  y[:, i, j] = k v + (1 - k) M;   every other pixel is 0.  With
 * b = 0, s = k = 1, t = 0 and an empty rectangle y is x bit for bit.  `drop_b` != 0 evaluates the same with b = 0: the adjoint's adjoint.
 * Adjoint (g = dL/dy -> dx = dL/dx): u[:, p, q] = g[:, p - t_row, q - t_col] where that output pixel exists and is not cut, else 0;
 *   S = sum(u) / (C H W);  w = k u + (1 - k) S;  dx = s w + (1 - s) mean_c(w).
 * The per-sample sums are fixed-order (csrc/reduce.h inside chunks of 4096 elements, the chunk sums in ascending order): no atomics,
 * a sample's bits depend on neither N, its place in the batch nor the run.  C H W <= 4096: one launch, the sample staged in LDS;
 * larger: a sum launch and an apply launch, with sbg_diffaug_workspace(N, C, H, W) bytes of `workspace` (0: none needed, may be NULL;
 * -1: unsupported sizes).  x and y (g and dx) must not overlap.  W % 4 == 0 and 16-byte aligned tensors take 16-byte accesses. */
#define SBG_DIFFAUG_WORDS 12
int64_t sbg_diffaug_workspace(int N, int C, int H, int W);
int sbg_diffaug_fwd(const float* x, const int32_t* table, float* y, float* workspace, int N, int C, int H, int W, int drop_b, sbg_stream_t stream);
int sbg_diffaug_adj(const float* g, const int32_t* table, float* dx, float* workspace, int N, int C, int H, int W, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Sliced Wasserstein distance on Laplacian-pyramid patches (Karras et al., "Progressive Growing of GANs", ICLR 2018, section 5: `swd-16k`
 * of their metrics/sliced_wasserstein.py; the reference has no counterpart).  The definition and every fixed order are stated in
 * csrc/swd.hip and DESIGN.md section 21.  fp32 dense tensors, 4-byte aligned (float64 outputs and workspaces 8-byte aligned); no atomics:
 * two calls give the same bits.
 *   sbg_swd_pyr_down: x [B, C, S, S] -> y [B, C, S/2, S/2]: the separable [1,4,6,4,1]/16 filter, mirrored boundaries (no repeat of the edge
 *                     sample), even rows and columns kept.  S a power of two in [4, 16384].
 *   sbg_swd_pyr_lap:  out = fine [B, C, S, S] - up(coarse [B, C, S/2, S/2]), up = zero insertion (samples at even positions) and the
 *                     separable [1,4,6,4,1]/8 filter with the same boundaries.  `out` may be `fine`.
 *   sbg_swd_gather:   rows row_offset + b P + p of desc [M, 49 C] = the 7 x 7 x C patch of level [B, C, S, S] around centres[b, p] = (y, x)
 *                     (int32 [B, P, 2] on the device), in (c, dy, dx) order; a centre outside [3, S - 4] writes a row of NaN.  C = 1..4.
 *   sbg_swd_moments:  out (float64 [C, 2]) = sum and sum of squares of every channel of desc [M, 49 C], float64 accumulation in an order fixed
 *                     by M alone; sbg_swd_moments_workspace(M, C) bytes of workspace (-1: unsupported sizes).  Two launches.
 *   sbg_swd_project:  out[d, m] (fp32 [D, M], direction-major) = the fp32 chain over k = 0 .. 49 C - 1 from 0 of
 *                     acc = fmaf(fmaf(desc[m, k], s[k / 49], t[k / 49]), dirs[k * dirs_ld + d], acc)  on v_mfma_f32_32x32x2_f32 (that chain bit
 *                     for bit).  s, t: fp32 [C] on the device; dirs: fp32 [49 C, >= D] with row pitch dirs_ld (a column slice costs nothing).
 *   sbg_swd_l1:       out[d] (float64 [D]) = sum_m |a[d, m] - b[d, m]| of two fp32 [D, M] arrays, the difference and the sum in float64 in an
 *                     order fixed by M alone; sbg_swd_l1_workspace(D, M) bytes of workspace (-1: unsupported sizes).  Two launches. */
int sbg_swd_pyr_down(const float* x, float* y, int B, int C, int S, sbg_stream_t stream);
int sbg_swd_pyr_lap(const float* fine, const float* coarse, float* out, int B, int C, int S, sbg_stream_t stream);
int sbg_swd_gather(const float* level, const int32_t* centres, float* desc, int B, int C, int S, int P, int64_t row_offset, int64_t M,
                   sbg_stream_t stream);
int64_t sbg_swd_moments_workspace(int64_t M, int C);
int sbg_swd_moments(const float* desc, double* out, void* workspace, int64_t M, int C, sbg_stream_t stream);
int sbg_swd_project(const float* desc, const float* s, const float* t, const float* dirs, float* out, int64_t M, int C, int D, int64_t dirs_ld,
                    sbg_stream_t stream);
int64_t sbg_swd_l1_workspace(int D, int64_t M);
int sbg_swd_l1(const float* a, const float* b, double* out, void* workspace, int D, int64_t M, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Average 2-D power spectrum of an image set (avg_spectra.py of Karras et al., "Alias-Free Generative Adversarial Networks", NeurIPS 2021;
 * the reference has no counterpart).  The definition -- a windowed, zero-padded fp32 radix-2 transform whose every rounding is stated, and a
 * float64 power accumulator with one sequential chain per entry -- is in csrc/spectrum.hip and DESIGN.md section 22; torch_utils/ops/spectrum.py
 * evaluates it for CPU tensors to the same bits.  R: image side, a power of two in [16, 1024]; S = R, 2 R or 4 R: spectrum side; BC image-channels.
 *   window:  fp32 [R].   stages: fp32 [S - 1, 2], the twiddles stage-major: entry h - 1 + j = twiddle[j S / (2 h)] = (cos, -sin)(2 pi j / (2 h)) for
 *            the half-spans h = 1, 2, .., S/2 and j < h (the op layer gathers it from twiddle[S/2]).   s, t: the normalisation v = fmaf(x, s, t).
 *   sbg_spectrum_workspace: bytes of the intermediate [BC, S/2 + 1, R] float2 (its R axis in bit-reversed row order), -1 for unsupported sizes.
 *   sbg_spectrum_rows: images (uint8 when is_u8, else fp32) [BC, R, R] -> the windowed row transforms, kx = 0 .. S/2, into the workspace.
 *   sbg_spectrum_cols: acc[kx, ky] (float64 [S/2 + 1, S], read and written in place) += the power of the windowed column transforms of the
 *                      BC image-channels, in ascending order; one workgroup per kx, no atomics: two runs give the same bits. */
int64_t sbg_spectrum_workspace(int64_t BC, int R, int S);
int sbg_spectrum_rows(const void* images, int is_u8, const float* window, const float* stages, float s, float t, void* workspace, int64_t BC, int R, int S,
                      sbg_stream_t stream);
int sbg_spectrum_cols(const void* workspace, const float* window, const float* stages, double* acc, int64_t BC, int R, int S, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Multi-scale structural similarity between two image batches (Wang, Simoncelli, Bovik 2003; the pairwise diversity tool diversity.py; the
 * reference has no counterpart).  The definition -- float64 moments under a separable 11-tap window whose every rounding is stated, the SSIM
 * map and fixed-order float64 means -- is in csrc/msssim.hip and DESIGN.md section 23; torch_utils/ops/msssim.py evaluates it for CPU tensors
 * to the same bits.  Images are byte values, uint8 when is_u8, else fp32, [BC, S, S] (BC image-channels).
 *   sbg_msssim_workspace: bytes of the tile partials of one level call (S a power of two in [16, 16384]), -1 for unsupported sizes.
 *   sbg_msssim_level: out[bc] = {mean of cs, mean of ssim} (float64 [BC, 2]) over the (S - 10)^2 map of x[bc] against y[bc]; window: float64
 *                     [11]; C1, C2: the stabilising constants.  Two launches (tiles, merge), no atomics: two runs give the same bits.
 *   sbg_msssim_down:  y (fp32 [BC, S/2, S/2]) = the 2 x 2 box mean ((a + b) + (c + d)) * 0.25f of x; S a power of two in [2, 16384]. */
int64_t sbg_msssim_workspace(int64_t BC, int S);
int sbg_msssim_level(const void* x, const void* y, int is_u8, const double* window, double C1, double C2, double* out, void* workspace, int64_t BC, int S,
                     sbg_stream_t stream);
int sbg_msssim_down(const void* x, int is_u8, float* y, int64_t BC, int S, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Latent directions (directions.py: GANSpace, Harkonen et al., NeurIPS 2020, and SeFa, Shen & Zhou, CVPR 2021; the reference has no
 * counterpart): the column mean and the Gram matrix of a table of latents x fp32 [N, D], and the table of edited latents.  The orders are
 * stated in csrc/directions.hip and DESIGN.md section 25; torch_utils/ops/directions.py evaluates them for CPU tensors to the same bits.
 * Dense tensors, fp32 4-byte and float64 8-byte aligned; N >= 1, 1 <= D <= 1024; no atomics: two runs give the same bits.
 *   sbg_directions_mean:  out (float64 [D]) = the float64 column sums of x in an order fixed by N alone, divided once by N;
 *                         sbg_directions_mean_workspace(N, D) bytes of workspace (-1: unsupported sizes).  Two launches.
 *   sbg_directions_gram:  out (float64 [D, D]) = c^T c of c = x - mean (one fp32 subtraction; mean NULL: c = x): fp32 fmaf chains over chunks
 *                         of 256 rows on the matrix cores, float64 sums of 16 chunks in registers, the group sums added by the merge kernel;
 *                         symmetric bit for bit.  sbg_directions_gram_workspace(N, D) bytes = 8 * groups * D * D (-1: unsupported sizes).
 *                         Two launches.
 *   sbg_directions_edit:  out (fp32 [S K T, L, D]), row (s K + k) T + t = ws[s] (fp32 [S, L, D]) with fmaf(sigmas[t] * scale[k], comps[k, d],
 *                         ws[s, l, d]) on the layers whose layer_mask (int32 [L]) entry is nonzero, a copy on the others.  One launch;
 *                         S K T = 0 writes nothing. */
int64_t sbg_directions_mean_workspace(int64_t N, int D);
int sbg_directions_mean(const float* x, double* out, void* workspace, int64_t N, int D, sbg_stream_t stream);
int64_t sbg_directions_gram_workspace(int64_t N, int D);
int sbg_directions_gram(const float* x, const float* mean, double* out, void* workspace, int64_t N, int D, sbg_stream_t stream);
int sbg_directions_edit(const float* ws, const float* comps, const float* scale, const float* sigmas, const int32_t* layer_mask, float* out,
                        int S, int L, int D, int K, int T, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * k-means centroid update on uint8 rows (modes.py: the number of statistically different bins, Richardson & Weiss, NeurIPS 2018; the
 * reference has no counterpart; csrc/kmeans_u8.hip).  points uint8 [N, F], labels int32 [N], old_centroids and
 * centroids uint8 [K, F], sums int64 [K, F], counts int64 [K], all dense:
 *   counts[k] = the number of rows with labels[n] == k;  sums[k, f] = the int64 sum of points[n, f] over those rows;
 *   centroids[k, f] = (2 sums[k, f] + counts[k]) / (2 counts[k]) in integer division (the mean rounded half up); an empty cluster keeps
 *   old_centroids[k] and has a sums row of 0.  A row whose label lies outside [0, K) is skipped (the caller's error; nothing is written
 *   out of bounds for it).  Integer arithmetic only: the result depends on the inputs alone; no floating point, no global atomics.
 * Limits: 1 <= N <= 2^24, 1 <= K <= 256, F a multiple of 16 and at most 3 * 2^20; points, old_centroids, centroids, sums and workspace
 * 16-byte aligned, counts 8, labels 4.  A refused call (bad sizes, a null or misaligned pointer) launches nothing, returns
 * SBG_ERR_INVALID and names the shape in sbg_last_error().  sbg_kmeans_u8_update_workspace(N, F, K) bytes of workspace = 4 * chunks * K * (F + 1)
 * for the i32 partial sums and counts of the row chunks (-1: unsupported sizes); chunks is chosen so that column tiles x chunks fills the
 * chip and is 1 once F / tile alone does (100 MB at N = 2^17, F = 196608, K = 128).  Two launches: accumulate, finish. */
int64_t sbg_kmeans_u8_update_workspace(int64_t N, int64_t F, int K);
int sbg_kmeans_u8_update(const uint8_t* points, const int32_t* labels, const uint8_t* old_centroids, uint8_t* centroids, int64_t* sums,
                         int64_t* counts, void* workspace, int64_t N, int64_t F, int K, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Latent walks (interpolate.py; the reference has no counterpart; csrc/walk.hip).  torch_utils/ops/walk.py evaluates
 * both for CPU tensors to the same bits.  Dense tensors; no atomics: two runs give the same bits.
 *   sbg_walk_blend:   keys fp32 [K, L, D], index int32 [T, 4], weight fp32 [T, 4] -> out fp32 [T, L, D].  On a layer whose layer_mask (int32 [L])
 *                     entry is nonzero (layer_mask NULL: every layer) out[t, l, d] is the fp32 chain acc = weight[t, 0] * keys[index[t, 0], l, d]
 *                     (one rounded product), acc = fmaf(weight[t, j], keys[index[t, j], l, d], acc) for j = 1, 2, 3 in this order; on the other
 *                     layers it is a copy of keys[hold[t], l, d] (hold int32 [T], needed with a mask).  K >= 1, L >= 1, 1 <= D <= 1024,
 *                     T L D < 2^31; pointers 4-byte aligned.  The CALLER checks that every index and hold value lies in [0, K); an element whose
 *                     index lies outside is skipped, never read.  One launch; T = 0 launches nothing.
 *   sbg_walk_sqdiff:  a, b uint8 [N, F], rows F bytes apart, any alignment (they may be slices of one tensor) -> out int64 [N],
 *                     out[n] = sum_f (a[n, f] - b[n, f])^2, exact.  1 <= N <= 2^24, 1 <= F <= 2^26; out and workspace 8-byte aligned.  Rows are
 *                     cut into sbg_walk_sqdiff_splits(N, F) = ceil(F / 16384) chunks (-1: unsupported sizes); with more than one, the chunks' int64
 *                     partials go to sbg_walk_sqdiff_workspace(N, F) = 8 N splits bytes (0 with one split, -1 unsupported) and a second launch
 *                     adds them.  A refused call launches nothing, returns SBG_ERR_INVALID and names the shape in sbg_last_error(). */
int sbg_walk_blend(const float* keys, const int32_t* index, const float* weight, const int32_t* layer_mask, const int32_t* hold, float* out,
                   int K, int T, int L, int D, sbg_stream_t stream);
int64_t sbg_walk_sqdiff_splits(int64_t N, int64_t F);
int64_t sbg_walk_sqdiff_workspace(int64_t N, int64_t F);
int sbg_walk_sqdiff(const uint8_t* a, const uint8_t* b, int64_t* out, void* workspace, int64_t N, int64_t F, sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Moments of uint8 images (variation.py: per-pixel variance by generator input, figures 4 and 5 of the StyleGAN paper; the reference has no
 * counterpart; csrc/moments_u8.hip).  torch_utils/ops/moments_u8.py evaluates all three for CPU tensors (numpy int64) to
 * the same bits.  Integers only; no atomics: the results depend on the inputs alone.  A refused call (bad sizes, a null or misaligned pointer)
 * launches nothing, returns SBG_ERR_INVALID and names the shape in sbg_last_error().
 *   sbg_moments_accumulate: images uint8 [G, N, F]; image (g, n) starts at images + g * group_stride + n * row_stride bytes, any base alignment
 *                     (a slice of a larger batch), row_stride >= F, group_stride >= (N - 1) row_stride + F (ignored when G = 1).  sum, sumsq int64
 *                     [G, F] dense, 8-byte aligned, RUNNING: sum[g, f] += sum_n images[g, n, f], sumsq[g, f] += sum_n images[g, n, f]^2.
 *                     1 <= G <= 65535, 1 <= F <= 2^26, 0 <= N <= sbg_moments_accumulate_max_n() = 32768 per call (N = 0 launches nothing): a
 *                     work-item adds the bytes of its columns into uint32 partials, which cannot overflow while 255^2 N < 2^32 (N <= 66051); 32768
 *                     leaves a factor of two.  The caller splits a larger N into several calls.
 *                     THE SPLIT RULE.  The kernel is a byte stream and G * ceil(F / 4096) workgroups (256 work-items of 16 bytes) do not fill the
 *                     chip at low resolution, so N is split over workgroups: with tiles = ceil(F / 4096),
 *                         want = max(1, min(ceil(1024 / (G tiles)), ceil(N / 16))),  rows = ceil(N / want),  splits = ceil(N / rows)
 *                     = sbg_moments_accumulate_splits(G, N, F) (0 for N = 0, -1 for unsupported sizes).  With one split the kernel adds into sum
 *                     and sumsq itself; otherwise it stores int64 partials [splits, G, 2, F] to sbg_moments_accumulate_workspace(G, N, F) =
 *                     16 splits G F bytes (0 with one split, -1 unsupported; 8-byte aligned) and a second launch adds them in split order.  The
 *                     load width W is 16 bytes when row_stride (and, for G > 1, group_stride) is a multiple of 16, 4 when a multiple of 4, else 1.
 *   sbg_moments_numerator:  sum, sumsq int64 [G, C, P], the count n -> num int64 [G, P], num[g, p] = sum_c (n sumsq[g, c, p] - sum[g, c, p]^2):
 *                     exact, never negative for the moments of n bytes; num / (C n (n - 1)) is the channel mean of the unbiased variance.  Every
 *                     term is at most 65025 n^2, so int64 cannot overflow while n^2 * 65025 * C < 2^63: the largest such n is
 *                     sbg_moments_numerator_max_n(C) (11 909 805 at C = 1, 6 876 129 at C = 3; -1 for C outside [1, 1024]) and a larger n is
 *                     refused.  1 <= G <= 65535, 1 <= P <= 2^26, G C P <= 2^40.  One launch.
 *   sbg_moments_render:     num int64 [G, P], thresholds int64 [255], table uint8 [256, 3] -> heat uint8 [G, 3, P], heat[g, :, p] = table[level]
 *                     with level = the number of thresholds <= num[g, p] (an integer comparison; ascending thresholds make it a scale), and
 *                     dominant uint8 [P] = the g of the largest num[g, p], ties to the lower g, 255 where every group is <= 0.  1 <= G <= 255,
 *                     1 <= P <= 2^26.  One launch. */
int64_t sbg_moments_accumulate_max_n(void);
int64_t sbg_moments_accumulate_splits(int64_t G, int64_t N, int64_t F);
int64_t sbg_moments_accumulate_workspace(int64_t G, int64_t N, int64_t F);
int sbg_moments_accumulate(const uint8_t* images, int64_t row_stride, int64_t group_stride, int64_t* sum, int64_t* sumsq, void* workspace,
                           int64_t G, int64_t N, int64_t F, sbg_stream_t stream);
int64_t sbg_moments_numerator_max_n(int64_t C);
int sbg_moments_numerator(const int64_t* sum, const int64_t* sumsq, int64_t* num, int64_t G, int64_t C, int64_t P, int64_t n, sbg_stream_t stream);
int sbg_moments_render(const int64_t* num, const int64_t* thresholds, const uint8_t* table, uint8_t* heat, uint8_t* dominant, int64_t G, int64_t P,
                       sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Activation statistics (network_summary.py: the per-layer, per-channel numerics columns of the network summary; the reference has no
 * counterpart; csrc/act_stats.hip).  torch_utils/ops/act_stats.py evaluates both entry points for CPU tensors in numpy to
 * the same bits.  No global atomics; no result depends on the launch geometry or on how samples were batched.  A refused call (bad sizes, a null
 * or misaligned pointer) launches nothing, returns SBG_ERR_INVALID and names the shape in sbg_last_error().
 *   sbg_act_stats_planes:  x is logically [N, C, P] of `dtype` (SBG_F32 / SBG_F16 / SBG_BF16); element (n, c, p) sits at x + n sn + c sc + p sp
 *                     ELEMENTS.  Dense NCHW is (C P, P, 1), channels_last (P C, 1, C), a 2-D [N, F] tensor C = F, P = 1, a batch slice has a
 *                     larger sn.  The planes must not overlap (the caller's check).  x need only be aligned to its element: a misaligned base or
 *                     stride takes a narrower load, never an error.  1 <= P < 2^31 - 4096, N C < 2^31 - 256, strides in [1, 2^40] wherever the
 *                     size is above 1.  One launch.  Every element is converted exactly to fp32; one record per plane (n, c):
 *                     counts int64 [N, C, SBG_ACT_STATS_COUNTS = 70], 8-byte aligned, dense:
 *                       [0] n = P     [1] n_zero (x == 0, either sign)     [2] n_nan     [3] n_posinf     [4] n_neginf
 *                       [5] n_peak: the number of finite elements with |x| == peak, peak the largest finite |x| of the plane; 0 when the plane
 *                           has no finite element.  (A clamped layer shows as many elements on one peak, whatever clamp and gain produced it.)
 *                       [6 .. 69] hist[64]: the exponent histogram of the finite non-zero elements: with e = floor(log2 |x|) of the fp32 value,
 *                           bin = min(max(e, -32), 31) + 32; fp32 subnormals land in bin 0.
 *                     values float64 [N, C, SBG_ACT_STATS_VALUES = 4], 8-byte aligned, dense:
 *                       [0] sum, [1] sumsq over the finite elements: (double)x and (double)x * (double)x are both exact and are added IN THE
 *                           PROJECT'S FIXED ORDER over the logical pixel index p, in every layout: lane t of 256 adds p = t, t + 256, ... in
 *                           ascending order from +0.0, then block_sum<256> of csrc/reduce.h (_exact_common.strided_sum_np of the float64 plane
 *                           with the non-finite elements replaced by 0).
 *                       [2] min, [3] max over the finite elements, as the float64 of the fp32 value, a zero of either sign counting as +0.0
 *                           (so the two do not depend on which zero is met first); +inf and -inf when the plane has no finite element.
 *                     sbg_act_stats_path (host only) names the mapping a call takes -- 1 staged (P > 64, sp == 1: 16-byte loads along P through
 *                     LDS), 2 cminor (P > 64, sc == 1, C a multiple of V = 16 / element bytes, x 16-byte aligned, sn and sp multiples of V: a
 *                     16-byte vector of V channels per work-item), 3 group (P <= 64: several planes per workgroup), 4 strided (the rest: scalar
 *                     loads) -- or -1 for a shape sbg_act_stats_planes refuses.  The bits are the same on every mapping.
 *   sbg_act_stats_fold:    records counts [N, C, 70] / values [N, C, 4] are added into the RUNNING records run_counts [C, 70] / run_values [C, 4]
 *                     (dense, 8-byte aligned; an empty running record is all zeros with min = +inf and max = -inf), one work-item per
 *                     (c, field), n ascending: counts add; sum and sumsq add in sample order, so the result does not depend on how the samples
 *                     were batched; min and max combine; n_peak follows the larger peak max(|min|, |max|) and adds on equal peaks.  N = 0
 *                     launches nothing.  One launch. */
#define SBG_ACT_STATS_COUNTS 70
#define SBG_ACT_STATS_VALUES 4
int sbg_act_stats_path(const void* x, int dtype, int64_t N, int64_t C, int64_t P, int64_t sn, int64_t sc, int64_t sp);
int sbg_act_stats_planes(const void* x, int dtype, int64_t N, int64_t C, int64_t P, int64_t sn, int64_t sc, int64_t sp, int64_t* counts,
                         double* values, sbg_stream_t stream);
int sbg_act_stats_fold(const int64_t* counts, const double* values, int64_t* run_counts, double* run_values, int64_t N, int64_t C,
                       sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-parameter gradient and update health of the run log (layers.jsonl; the reference has no counterpart; csrc/layer_health.hip, DESIGN.md
 * section 30).  torch_utils/ops/layer_health.py builds the tables and restates the three entry points in numpy to the same bits.  Nothing
 * but `out` / `running` is written; no atomics; every order of additions is a function of the segment sizes alone.
 * A parameter is a SEGMENT of n fp32 elements, 4-byte aligned, cut into ceil(n / SBG_LAYER_HEALTH_CHUNK) chunks counted from its own first
 * element.  All tables are dense device memory built by the caller, and the kernels trust them:
 *   wg        int32 [records, 2]: workgroup b reads chunk wg[b][1] of segment wg[b][0]; segment-major, chunks ascending, so the records of
 *             segment p are rec_start[p] .. rec_start[p + 1)
 *   rec_start int64 [P + 1]: the running sum of the chunk counts
 *   total_n   the sum of the sizes (launch log and sanity only)
 *   sbg_layer_health_grads:    segs int64 [P, 2] = {address of the first element, n}.  Per element, with the scale s, the definition of
 *                     sbg_grad_finish_sweep without the store: y = x * s (skipped when s == 1.0f); z = isnan(y) ? +0 : y == +inf ? 1e5f :
 *                     y == -inf ? -1e5f : y.  out[b] = float64 [count of y not finite, sum (double)z * (double)z, max |z|] of chunk b.
 *   sbg_layer_health_updates:  segs int64 [P, 4] = {address of w, of exp_avg, of exp_avg_sq, n}: three fp32 arrays read in memory order.
 *                     Per element in float64: d = lr * (m / bc1) / (sqrt(v / bc2) + eps), IEEE division and square root, every operation
 *                     rounded once.  out[b] = float64 [sum w * w, max |w|, sum d * d] of chunk b.  0 < bc1, bc2 <= 1, eps >= 0.
 *   Inside a chunk, vector v holds the elements 4 v .. 4 v + 3; lane t of 256 adds the elements of its vectors t, t + 256, t + 512, t + 768 in
 *   ascending order from +0.0; the lanes are added as in csrc/reduce.h.
 *   sbg_layer_health_fold:     one workgroup per parameter adds its records (lane t the records t, t + 256, ... of the parameter in ascending
 *                     order, the lanes as in csrc/reduce.h) into running float64 [P, SBG_LAYER_HEALTH_FIELDS]:
 *                       [0] steps  [1] steps_with_nonfinite  [2] nonfinite  [3] grad_sumsq  [4] grad_absmax  [5] weight_sumsq  [6] weight_absmax
 *                       [7] update_sumsq
 *                     mode 0 (records of _grads):  [0] += 1, [1] += count > 0, [2] += count, [3] += sumsq, [4] = max([4], absmax);
 *                     mode 1 (records of _updates): [5] = sum w * w, [6] = max |w|, [7] += sum d * d.  A parameter without records (n == 0)
 *                     contributes zeros.  P == 0 launches nothing. */
#define SBG_LAYER_HEALTH_CHUNK 4096
#define SBG_LAYER_HEALTH_FIELDS 8
int sbg_layer_health_grads(const int64_t* segs, const int32_t* wg, int64_t records, int64_t total_n, float scale, double* out, sbg_stream_t stream);
int sbg_layer_health_updates(const int64_t* segs, const int32_t* wg, int64_t records, int64_t total_n, double lr, double eps, double bc1, double bc2,
                             double* out, sbg_stream_t stream);
int sbg_layer_health_fold(const double* records, const int64_t* rec_start, int64_t P, int64_t nrecords, int mode, double* running,
                          sbg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * In-process launch timing (measurement only; bench.py's roofline figures come from here).
 * While enabled, every kernel launch of this library is bracketed by two hipEvents recorded on the launch stream
 * and logged with its algorithmic flops / bytes.  sbg_prof_fetch() synchronises the logged events, writes up to `max`
 * records (oldest first) with their measured duration, clears the log and returns the number written
 * (or the number pending when out == NULL). */
enum sbg_kernel_kind {
    SBG_K_BIAS_ACT = 1, SBG_K_UPFIRDN2D = 2, SBG_K_CONV_IGEMM = 3, SBG_K_CONV_WGRAD = 4, SBG_K_WGRAD_REDUCE = 5,
    SBG_K_SCALE_NC = 6, SBG_K_DOT_HW = 7, SBG_K_SN_POWER = 9, SBG_K_ATTENTION = 10, SBG_K_GRID_SAMPLE = 11, SBG_K_FILTER1D = 12, SBG_K_COLOR = 13, SBG_K_WEIGHT_PREP = 14, SBG_K_TORGB = 15, SBG_K_FROMRGB = 16,
    SBG_K_GROUPED_GEMM = 17, SBG_K_PPL = 18,    /* SBG_K_PPL: dims[0] = variant: 0 slerp / 1 lerp endpoints, 2 image prep, 3 distance */
    SBG_K_PROJECTOR = 19,       /* one record per launch; dims[0] = variant: 0 reg / 1 reg_bwd / 2 normalize / 3 sqdist / 4 sqdist_bwd, dims[1] = stage */
    SBG_K_IMAGE_EXPORT = 20,    /* dims[0] = variant: 0 quantize_tile (N, C, H, W, rule, dims[6] = 1 four planar pixels / 2 four channel-minor
                                 * pixels / 3 one pixel per work-item), 1 truncate_mix (R * Cn, L, D, dims[4] = 1 vec4 / 2 scalar) */
    SBG_K_RESAMPLE = 21,        /* dims[0] = variant: 0 h (N, rows, in_w, out_w, C, dims[6] = strip), 1 v (N, row_bytes, in_h, out_h, ksize,
                                 * dims[6] = 1 dword / 2 byte loads) */
    SBG_K_PR = 22,              /* dims[0] = variant: 0 single / 1 split (the tile kernel, one / several column runs per row tile), 2 merge,
                                 * 3 norms; then R, C, F, k, runs, dims[6] = 0 radius / 1 membership / 2 probe / 3 top-k / 4 realism */
    SBG_K_GRAD_FINISH = 23,     /* dims[0] = variant: 0 sweep (records, n clipped to INT32_MAX, dims[3] = 1 when the scale is applied),
                                 * 1 merge (records) */
    SBG_K_RESIDENT = 24,        /* dims = B, C, H, W, out_f32, 0, dims[6] = 1 dword path (4 pixels per work-item) / 2 byte path */
    SBG_K_DIFFAUG = 25,         /* dims[0] = variant: 0 sum / 1 apply / 2 adjoint sum / 3 adjoint apply (the two launches of C H W > 4096),
                                 * 4 single-pass forward / 5 single-pass adjoint (C H W <= 4096); then N, C, H, W, dims[5] = 1 16-byte / 2 dword accesses */
    SBG_K_NN_U8 = 26,           /* dims[0] = variant: 0 norms (Q or M rows, the other 0) / 1 single / 2 split (the tile kernel, one / several
                                 * store runs per query tile) / 3 merge; then Q, M, F clipped to INT32_MAX, k, runs */
    SBG_K_SWD = 27,             /* dims[0] = variant: 0 pyr_down (B, C, S) / 1 pyr_lap (B, C, S) / 2 gather (B, C, S, P) / 3 moments (M, C, chunks) /
                                 * 4 project (M, K, D) / 5 l1 (D, M, chunks) / 6 merge of the float64 partials (values, chunks); M clipped to INT32_MAX */
    SBG_K_SPECTRUM = 28,        /* dims[0] = variant: 0 rows / 1 cols; then BC (image-channels of the call), R, S */
    SBG_K_MSSSIM = 29,          /* dims[0] = variant: 0 level / 1 down / 2 merge; then BC (image-channels of the call, clipped to INT32_MAX), S */
    SBG_K_DIRECTIONS = 30,      /* dims[0] = variant: 0 mean (N, D, chunks) / 1 gram (N, D, groups) / 2 merge (N, D, chunks or groups: the launch
                                 * it finishes) / 3 edit (S, K, T, L, D); N clipped to INT32_MAX */
    SBG_K_KMEANS_U8 = 31,       /* dims[0] = variant: 0 accumulate / 1 finish; then N, F (both clipped to INT32_MAX), K, row chunks, lanes per row */
    SBG_K_WALK = 32,            /* dims[0] = variant: 0 blend (T, L, D, 1 with a layer mask) / 1 sqdiff (N, F, splits) / 2 merge (N, F, splits: the
                                 * second launch of a split sqdiff); N, F clipped to INT32_MAX */
    SBG_K_MOMENTS = 33,         /* dims[0] = variant: 0 accumulate (G, N, F, splits, load width W) / 1 merge (G, N, F, splits: the second launch of a
                                 * split accumulate) / 2 numerator (G, C, P) / 3 render (G, P); F, P clipped to INT32_MAX */
    SBG_K_ACT_STATS = 34,       /* dims[0] = variant: 0 planes (N, C, P, mapping 1 staged / 2 cminor / 3 group / 4 strided, dtype) / 1 fold (N, C);
                                 * N, C, P clipped to INT32_MAX */
    SBG_K_LAYER_HEALTH = 35     /* dims[0] = variant: 0 grads (records, n clipped to INT32_MAX, dims[3] = 1 when the scale is applied) /
                                 * 1 updates (records, n) / 2 fold (P, records, dims[3] = 0 grads / 1 updates) */
};
/* Kernel-variant codes in the records of the streaming kernels (which kernel served the launch):
 *   bias_act     dims[4] = 1 vec8 / 2 scalar,  dims[5] = bias mode (0 none, 1 channel-minor vector, 2 one per 8-vector, 3 generic)
 *   scale_nc     dims[4] = 1 vec8 / 2 scalar
 *   upfirdn2d    dims[6] = 10000 * variant + 16 * upx + downx: 1 sliding-window matrix-core FIR / 3 the same plus the register-blocked kernel
 *                on 1..4 edge columns / 5 register-blocked 4x4 / 6 register-blocked, any size up to 8x8 / 7 generic, 8 channels per lane /
 *                8 generic, scalar.  2 and 4 (the tile matrix-core kernel alone / with edge columns) are retired and not reused: logs
 *                recorded before its removal carry them; those launches (8..15 output rows) now log 1 and 3
 *   dot_hw       dims[4] = 1 generic / 2 lane per channel vector / 3 serial channel vectors,  dims[5] = pixel splits
 *                (dims[3] = layout, 3 dot_hw_scale, 2 modconv_bwd, 4 modconv_bwd_prescaled, 5 moments_hw: dims[4] = 1 vec8 / 2 scalar)
 *   weight_prep  pack (dims[3] = 0): dims[4] = 1 transposing LDS tiles / 2 one lane per (row, column)
 *   torgb        forward (dims[4] = 0): dims[5] = 1 matrix cores / 2 streaming, 3 outputs / 3 streaming, 4 outputs
 *   fromrgb      backward (dims[4] = 1): dims[5] = image channels unrolled (3, or 4 for any), dims[6] = 1 with the image gradient
 *   attention    (N, Q, M, D, DV), dims[5] = 0 forward / 1 backward, dims[6] = 0 single (M <= 256; the backward is one record for both
 *                passes) / 1 stream (forward) / 2 stream_stats / 3 stream_dq / 4 stream_dkv (the three launches of the streamed backward) */
typedef struct sbg_prof_record {
    int    kind;            /* enum sbg_kernel_kind */
    int    dims[7];         /* kernel specific shape key (see each kernel's source) */
    double flops;           /* algorithmic floating point operations of the launch (2 x MACs) */
    double bytes;           /* algorithmic HBM bytes of the launch */
    float  ms;              /* measured duration */
    int    pad;
} sbg_prof_record;
int sbg_prof_enable(int on);
int sbg_prof_fetch(sbg_prof_record* out, int max);

#ifdef __cplusplus
}
#endif
#endif /* SBG_HIP_H */
