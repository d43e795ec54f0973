// sqdist.h -- the LPIPS squared distance dist[r] = (sum_f (a[r, f] - b[r, f])^2) / div for B rows of F features, shared by
// ppl.hip (B rows, div = eps^2) and projector.hip (one row, div = 1).  Two launches, no float atomics:
//   partial:  grid (nchunk, B); workgroup (chunk, r) sums its kDistChunk features of row r -> part[r, chunk]
//   final:    the shared merge kernel (merge.h) adds the nchunk partials of row r and divides once
// Every work-item's share is summed in index order, then block_sum (reduce.h): the same bits on every run.  Each square is rounded
// before it is added.  The callers own the launch-log scopes; nothing here logs.
#pragma once
#include "sbg_common.h"
#include "reduce.h"
#include "merge.h"

namespace {

constexpr int kDistThreads = 256;
constexpr int kDistChunk = kDistThreads * 4 * 8;      // elements of one row per workgroup: 8 float4 per work-item

int64_t dist_chunks(int64_t F) { return (F + kDistChunk - 1) / kDistChunk; }

// FMA_TAIL exists only to keep the path-length metric's historical rounding: its scalar path (F % 4 != 0 or unaligned rows) was
// compiled to fused multiply-adds, its float4 path was not.  New callers pass false.
template <bool FMA_TAIL>
__global__ __launch_bounds__(kDistThreads) void sqdist_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                      float* __restrict__ part, int64_t F, int nchunk, int vec4)
{
#pragma clang fp contract(off)
    __shared__ float red[kDistThreads / 64];
    const int chunk = blockIdx.x, r = blockIdx.y;
    const float* pa = a + (int64_t)r * F;
    const float* pb = b + (int64_t)r * F;
    const int64_t f0 = (int64_t)chunk * kDistChunk;
    float s = 0.f;
    if (vec4) {         // F % 4 == 0 and 16-byte aligned rows: a float4 is wholly inside or wholly outside the row
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int64_t f = f0 + 4 * ((int64_t)k * kDistThreads + threadIdx.x);
            if (f < F) {
                const float4_t x = *reinterpret_cast<const float4_t*>(pa + f), y = *reinterpret_cast<const float4_t*>(pb + f);
#pragma unroll
                for (int q = 0; q < 4; q++) { const float d = x[q] - y[q]; const float d2 = d * d; s += d2; }
            }
        }
    } else {
        for (int k = 0; k < 32; k++) {
            const int64_t f = f0 + (int64_t)k * kDistThreads + threadIdx.x;
            if (f < F) {
                const float d = pa[f] - pb[f];
                if (FMA_TAIL) s = fmaf(d, d, s);
                else { const float d2 = d * d; s += d2; }
            }
        }
    }
    const float tot = block_sum<kDistThreads>(s, red);
    if (threadIdx.x == 0) part[(int64_t)r * nchunk + chunk] = tot;
}

} // namespace
