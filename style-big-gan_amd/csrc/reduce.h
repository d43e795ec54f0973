// reduce.h -- the one definition of the fixed-order sums behind the tool kernels' reproducibility claims (ppl.hip, projector.hip,
// knn_manifold.hip, diffaug.hip, mbstd.hip, grad_finish.hip, swd.hip, msssim.hip, sqdist.h, merge.h).  The ORDER IS PART OF THE CONTRACT:
// the bit-for-bit tests and DESIGN.md rest on it.  merge.h adds the partials of a split sum with it; torch_utils/ops/_exact_common.py
// states the same order in numpy.
//   wave_sum:   the 64-lane xor butterfly, offsets 32, 16, ... 1; every lane ends with the same value.
//   block_sum:  wave_sum in each wave, then the NT / 64 per-wave values added LEFT TO RIGHT IN WAVE ORDER,
//               ((red[0] + red[1]) + red[2]) + ...; every work-item ends with the same value.
// The step's hot kernels keep their own in-wave sums (shared only where the instructions stay the same).
#pragma once
#include <hip/hip_runtime.h>

static __device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// NT = workgroup size; `red` holds NT / 64 floats of LDS.  Every work-item of the workgroup must call it.  The leading barrier lets a
// kernel call it again with the same `red` (a previous call's reads are over before the next call's writes).
template <int NT>
static __device__ __forceinline__ float block_sum(float v, float* red)
{
    static_assert(NT % 64 == 0 && NT >= 64 && NT <= 1024, "block_sum: whole waves only");
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = red[0];
#pragma unroll
    for (int w = 1; w < NT / 64; w++) s += red[w];
    return s;
}

// The float64 forms (grad_finish.hip, swd.hip, msssim.hip, merge.h): the same butterfly and the same wave order; `red` holds NT / 64 doubles.
static __device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int NT>
static __device__ __forceinline__ double block_sum(double v, double* red)
{
    static_assert(NT % 64 == 0 && NT >= 64 && NT <= 1024, "block_sum: whole waves only");
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < NT / 64; w++) s += red[w];
    return s;
}
