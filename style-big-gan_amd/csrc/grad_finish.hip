// grad_finish.hip -- the end of a training phase over a flat fp32 gradient bucket in one pass: the 1/world scale of a data-parallel
// exchange, the reference's nan_to_num(nan=0, posinf=1e5, neginf=-1e5) (train_parts/trainers.py:745-747) and, from the same read, the
// gradient-health statistics of the run log.  Per element, with the scale s:
//   y = x * s            one fp32 multiply, skipped when s == 1.0f
//   z = isnan(y) ? +0.0f : y == +inf ? 1e5f : y == -inf ? -1e5f : y          stored back in place
//   count += y is not finite;   sumsq += (double)z * (double)z;   absmax = max(absmax, |z|)
// The squares are float64 products of fp32 values (exact) summed in float64: finite gradients near 1e30 do not overflow the norm.
//
// Sweep: a streaming kernel, 16-B loads and stores, 4 of them in flight per lane, a scalar tail for n % 4 in the last chunk.  Workgroup b
// owns the contiguous chunk [b * chunk, (b + 1) * chunk) with chunk = 4096 * ceil(n / 2^24): a function of n alone, never of the CU
// count, so the partial sums and with them the bits of the result are the same on every device.  A lane adds its elements in ascending
// order, the lanes are added by block_sum (reduce.h), lane 0 writes the record [count, sumsq, absmax] as float64.
// Merge: one workgroup; lane t adds records t, t + 256, ... in ascending order, block_sum adds the lanes: an order that depends on the
// number of records alone.  A second launch, not a last-workgroup counter inside the sweep; no atomics: two runs give the same bits.
// HBM-bound: algorithmic bytes = 8 n (one read, one write).
// Launch-log key: kind SBG_K_GRAD_FINISH, dims = {0 sweep, records, n, scale applied} / {1 merge, records}.
#include "sbg_common.h"
#include "reduce.h"

namespace {

constexpr int kSweep = 0, kMerge = 1;
constexpr int NT = 256;                     // sweep workgroup
constexpr int U = 4;                        // 16-B vectors in flight per lane
constexpr int64_t kChunk0 = 4096;           // NT * U * 4: the chunk of every n <= kChunk0 * kMaxRecords
constexpr int64_t kMaxRecords = 4096;
constexpr int MT = 256;                     // merge workgroup

static_assert(kChunk0 == (int64_t)NT * U * 4, "one batch of the sweep covers the base chunk");

int64_t chunk_len(int64_t n)
{
    const int64_t span = kChunk0 * kMaxRecords;
    const int64_t k = n <= span ? 1 : (n + span - 1) / span;
    return kChunk0 * k;
}

struct Health { unsigned count; double sumsq; float absmax; };

constexpr int kNotFinite = 0x207;           // v_cmp_class mask: signalling NaN, quiet NaN, -inf, +inf

__device__ __forceinline__ float sanitise(float y, unsigned& count)
{
    if (!__builtin_amdgcn_classf(y, kNotFinite)) return y;
    count++;
    return (y != y) ? 0.f : (y > 0.f ? 1e5f : -1e5f);
}

__device__ __forceinline__ void account(float z, Health& h)
{
    const double zd = (double)z;
    h.sumsq += zd * zd;
    h.absmax = fmaxf(h.absmax, fabsf(z));
}

// U vectors per lane, NT apart, from vector v0 on: every load is issued before the first value is used.  GUARD: vectors at or beyond nvec
// are skipped (the last chunk, and the chunks of n > 2^24 that take several batches); the lane's order of additions is the same either way.
template <bool SCALE, bool GUARD>
__device__ __forceinline__ void sweep_batch(float* __restrict__ p, int64_t v0, int64_t nvec, float s, Health& h)
{
    float4_t r[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int64_t v = v0 + (int64_t)u * NT;
        if (!GUARD || v < nvec) r[u] = *reinterpret_cast<const float4_t*>(p + 4 * v);
        __builtin_amdgcn_sched_barrier(0);  // loads leave in the order they are used: vector u is worked on while u + 1 ... are in flight
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int64_t v = v0 + (int64_t)u * NT;
        if (!GUARD || v < nvec) {
            float4_t y = r[u];
            if (SCALE) y *= s;
            // a wave whose 256 values are all finite, the common case, stores them back as they are: one class test per value and a
            // wave-uniform branch around the selects
            const bool bad = __builtin_amdgcn_classf(y[0], kNotFinite) | __builtin_amdgcn_classf(y[1], kNotFinite) |
                             __builtin_amdgcn_classf(y[2], kNotFinite) | __builtin_amdgcn_classf(y[3], kNotFinite);
            if (__builtin_amdgcn_ballot_w64(bad) != 0) {
#pragma unroll
                for (int e = 0; e < 4; e++) y[e] = sanitise(y[e], h.count);
            }
#pragma unroll
            for (int e = 0; e < 4; e++) account(y[e], h);
            *reinterpret_cast<float4_t*>(p + 4 * v) = y;
        }
    }
}

template <bool SCALE>
__global__ __launch_bounds__(NT) void grad_finish_sweep_kernel(float* __restrict__ flat, int64_t n, float s, int64_t chunk, double* __restrict__ partials)
{
    __shared__ double red[NT / 64];
    __shared__ float redmax[NT / 64];
    const int tid = threadIdx.x;
    const int64_t begin = (int64_t)blockIdx.x * chunk;
    const int64_t left = n - begin;
    const int64_t len = left < chunk ? left : chunk;        // the host launches ceil(n / chunk) workgroups: len >= 1
    float* const p = flat + begin;                          // 16-B aligned: the base is, and chunk % 4 == 0
    const int64_t nvec = len >> 2;

    Health h = {0u, 0.0, 0.f};
    if (len == kChunk0) {                                   // one unguarded batch is the whole chunk: NT * U * 4 == kChunk0
        sweep_batch<SCALE, false>(p, tid, nvec, s, h);
    } else {
        for (int64_t v0 = tid; v0 < nvec; v0 += (int64_t)NT * U) sweep_batch<SCALE, true>(p, v0, nvec, s, h);
        const int64_t t = (nvec << 2) + tid;                // n % 4 elements behind the last whole vector of the last chunk
        if (t < len) {
            const float z = sanitise(SCALE ? p[t] * s : p[t], h.count);
            account(z, h);
            p[t] = z;
        }
    }

    const double c = block_sum<NT>((double)h.count, red);
    const double q = block_sum<NT>(h.sumsq, red);
    float absmax = h.absmax;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) absmax = fmaxf(absmax, __shfl_xor(absmax, off, 64));
    if ((tid & 63) == 0) redmax[tid >> 6] = absmax;
    __syncthreads();
    if (tid == 0) {
        float m = redmax[0];
#pragma unroll
        for (int w = 1; w < NT / 64; w++) m = fmaxf(m, redmax[w]);
        double* rec = partials + 3 * (int64_t)blockIdx.x;
        rec[0] = c; rec[1] = q; rec[2] = (double)m;
    }
}

// result = [sum of the counts, sum of the sumsq, max of the absmax] over `records` records, in an order that depends on `records` alone:
// lane t of the MT adds records t, t + MT, t + 2 MT, ... in ascending order, block_sum (reduce.h) adds the lanes.  The maximum has no order.
__global__ __launch_bounds__(MT) void grad_finish_merge_kernel(const double* __restrict__ partials, int64_t records, double* __restrict__ result)
{
    __shared__ double red[MT / 64];
    const int tid = threadIdx.x;
    double count = 0.0, sumsq = 0.0, absmax = 0.0;
    for (int64_t r0 = tid; r0 < records; r0 += 4 * MT) {
        double v[4][3];
#pragma unroll
        for (int j = 0; j < 4; j++) {                       // four records in flight; + 0.0 and max with 0 are exact
            const int64_t r = r0 + (int64_t)j * MT;
#pragma unroll
            for (int k = 0; k < 3; k++) v[j][k] = r < records ? partials[3 * r + k] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) { count += v[j][0]; sumsq += v[j][1]; absmax = fmax(absmax, v[j][2]); }
    }
    count = block_sum<MT>(count, red);
    sumsq = block_sum<MT>(sumsq, red);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) absmax = fmax(absmax, __shfl_xor(absmax, off, 64));
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = absmax;
    __syncthreads();
    if (tid == 0) {
        double m = red[0];
#pragma unroll
        for (int w = 1; w < MT / 64; w++) m = fmax(m, red[w]);
        result[0] = count; result[1] = sumsq; result[2] = m;
    }
}

} // namespace

extern "C" int64_t sbg_grad_finish_records(int64_t n)
{
    if (n < 0) return -1;
    const int64_t chunk = chunk_len(n);
    return (n + chunk - 1) / chunk;
}

extern "C" int sbg_grad_finish_sweep(float* flat, int64_t n, float scale, double* partials, sbg_stream_t stream)
{
    SBG_CHECK(n >= 0, "grad_finish: n = %lld", (long long)n);
    if (n == 0) return SBG_OK;
    SBG_CHECK(flat != nullptr && partials != nullptr, "grad_finish: flat and partials must be device pointers");
    SBG_CHECK(sbg_aligned16(flat), "grad_finish: the buffer must be 16-byte aligned (pass the whole flat bucket, not a view into it)");
    SBG_CHECK((reinterpret_cast<uintptr_t>(partials) & 7) == 0, "grad_finish: partials must be 8-byte aligned");
    SBG_CHECK(scale == scale, "grad_finish: the scale is NaN");
    const int64_t chunk = chunk_len(n);
    const int64_t records = (n + chunk - 1) / chunk;
    const bool scaled = scale != 1.0f;
    hipStream_t s = (hipStream_t)stream;
    SbgProfScope prof(s, SBG_K_GRAD_FINISH, 0.0, 8.0 * (double)n, {kSweep, (int)records, (int)(n < INT32_MAX ? n : INT32_MAX), scaled ? 1 : 0});
    if (scaled) SBG_LAUNCH(grad_finish_sweep_kernel<true>, dim3((unsigned)records), dim3(NT), 0, s, flat, n, scale, chunk, partials);
    else        SBG_LAUNCH(grad_finish_sweep_kernel<false>, dim3((unsigned)records), dim3(NT), 0, s, flat, n, scale, chunk, partials);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int sbg_grad_finish_merge(const double* partials, int64_t records, double* result, sbg_stream_t stream)
{
    SBG_CHECK(records >= 0, "grad_finish_merge: records = %lld", (long long)records);
    SBG_CHECK(result != nullptr && (records == 0 || partials != nullptr), "grad_finish_merge: partials and result must be device pointers");
    SBG_CHECK((reinterpret_cast<uintptr_t>(partials) & 7) == 0 && (reinterpret_cast<uintptr_t>(result) & 7) == 0,
              "grad_finish_merge: partials and result must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    SbgProfScope prof(s, SBG_K_GRAD_FINISH, 0.0, 24.0 * (double)records + 24.0, {kMerge, (int)(records < INT32_MAX ? records : INT32_MAX)});
    SBG_LAUNCH(grad_finish_merge_kernel, dim3(1), dim3(MT), 0, s, partials, records, result);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}
