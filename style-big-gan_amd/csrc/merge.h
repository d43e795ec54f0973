// merge.h -- the one second stage of the tool kernels' split sums: out[v] = (sum of partial[v * count .. + count)) / div, for the partials
// that swd_moments / swd_l1 (swd.hip), msssim_level (msssim.hip) and sqdist_partial (sqdist.h: ppl.hip, projector.hip) write.
// One workgroup of 256 per output value: lane t adds the partials t, t + 256, ... in ascending order from 0, block_sum (reduce.h) adds
// the lanes, work-item 0 divides once.  div = 1 is the plain sum (x / 1 is x, for NaN, the infinities and the signed zeros too).  The order
// depends on `count` alone: no atomics, the same bits on every run.  torch_utils/ops/_exact_common.py `strided_sum_np` is the same order
// in numpy.  The callers own the launch-log scopes; nothing here logs.
#pragma once
#include "sbg_common.h"
#include "reduce.h"

namespace {

constexpr int kMergeThreads = 256;

template <class T>
__global__ __launch_bounds__(kMergeThreads) void partials_merge_kernel(const T* __restrict__ partial, T* __restrict__ out, int count, T div)
{
    __shared__ T red[kMergeThreads / 64];
    const T* p = partial + (int64_t)blockIdx.x * count;
    T s = 0;
    for (int i = threadIdx.x; i < count; i += kMergeThreads) s = s + p[i];
    s = block_sum<kMergeThreads>(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s / div;
}

// values >= 1 workgroups; the caller has checked the pointers and that values fits a grid dimension
template <class T>
int merge_partials(const T* partial, T* out, int64_t values, int count, T div, hipStream_t s)
{
    SBG_LAUNCH(partials_merge_kernel<T>, dim3((unsigned)values), dim3(kMergeThreads), 0, s, partial, out, count, div);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

} // namespace
