// layer_health.hip -- per-parameter gradient and update health of the run log (layers.jsonl; the reference has no
// counterpart).  Two read-only streaming passes over tables of segments (one segment = one parameter) and a fold into a running table.
//
// Gradient pass, per element of a segment and a scale s -- the definition of grad_finish.hip, nothing stored:
//   y = x * s            one fp32 multiply, skipped when s == 1.0f
//   z = isnan(y) ? +0.0f : y == +inf ? 1e5f : y == -inf ? -1e5f : y
//   record = [count of y not finite, sum (double)z * (double)z, max |z|]
// Update pass, per element, in float64 from the fp32 weight w and Adam moments m, v, with lr, eps, bc1 = 1 - beta1^t, bc2 = 1 - beta2^t:
//   d = lr * (m / bc1) / (sqrt(v / bc2) + eps)           IEEE division and square root, no contraction
//   record = [sum w * w, max |w|, sum d * d]
//
// Chunking: a segment of n elements is cut into ceil(n / 4096) chunks COUNTED FROM ITS OWN FIRST ELEMENT; one workgroup of 256 per chunk,
// named by the host-built table wg[b] = (segment, chunk).  Inside a chunk of len <= 4096 elements, vector v holds the elements 4v .. 4v + 3
// (those at or beyond len do not exist); lane t owns the vectors t, t + 256, t + 512, t + 768 and adds their elements in ascending order
// from +0.0; the lanes are added by block_sum (reduce.h); lane 0 writes the record as three float64.  Every order is a function of n alone:
// the segment starts are only 4-byte aligned and the 16-byte loads are issued at that alignment (global memory takes them), the one partial
// vector of a segment's last chunk is read element by element.
// Fold: one workgroup per parameter; lane t adds that parameter's records t, t + 256, ... in ascending order, block_sum adds the lanes,
// lane 0 updates the parameter's row of the running float64 table [P, SBG_LAYER_HEALTH_FIELDS].  A second launch, not a last-workgroup
// counter; no atomics: two runs give the same bits.
// HBM-bound: algorithmic bytes = 4 n (gradient pass), 12 n (update pass).
// Launch-log key: kind SBG_K_LAYER_HEALTH, dims = {0 grads, records, n, scale applied} / {1 updates, records, n} / {2 fold, P, records, mode}.
#include "sbg_common.h"
#include "reduce.h"

#pragma clang fp contract(off)              // d * d and the sums round once each, as the host restatement does

namespace {

constexpr int kGrads = 0, kUpdates = 1, kFold = 2;
constexpr int NT = 256;
constexpr int U = 4;                        // 16-B vectors per lane
constexpr int kChunk = SBG_LAYER_HEALTH_CHUNK;
constexpr int kNotFinite = 0x207;           // v_cmp_class mask: signalling NaN, quiet NaN, -inf, +inf

static_assert(kChunk == NT * U * 4, "one batch of vectors covers a chunk");

typedef float float4_a4 __attribute__((ext_vector_type(4), aligned(4)));    // a 16-byte load from a 4-byte aligned address
typedef const __attribute__((address_space(1))) float* gfloat_p;            // the segments are global memory: global_load, not flat_load
typedef const __attribute__((address_space(1))) float4_a4* gfloat4_p;

__device__ __forceinline__ gfloat_p global_floats(int64_t address) { return (gfloat_p)(uintptr_t)address; }

struct Chunk { int64_t seg; int64_t begin; int len; };

__device__ __forceinline__ Chunk chunk_of(const int32_t* __restrict__ wg, const int64_t* __restrict__ segs, int stride)
{
    Chunk c;
    c.seg = wg[2 * (int64_t)blockIdx.x];
    c.begin = (int64_t)wg[2 * (int64_t)blockIdx.x + 1] * kChunk;
    const int64_t left = segs[c.seg * stride + stride - 1] - c.begin;       // the host builds wg from the same sizes: left >= 1
    c.len = (int)(left < kChunk ? left : kChunk);
    return c;
}

// the chunk's vectors of this lane: whole ones by one 16-byte load, the partial one of a last chunk element by element, absent ones +0.0
// (present[u] = number of elements of vector u that exist)
__device__ __forceinline__ void load_lane(gfloat_p p, int len, float4_t (&r)[U], int (&present)[U])
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int e0 = 4 * (tid + u * NT);
        const int have = len - e0;
        present[u] = have >= 4 ? 4 : (have > 0 ? have : 0);
        r[u] = float4_t{0.f, 0.f, 0.f, 0.f};
        if (have >= 4) {
            r[u] = *(gfloat4_p)(p + e0);
        } else {
#pragma unroll
            for (int e = 0; e < 3; e++)
                if (e < have) r[u][e] = p[e0 + e];
        }
    }
}

__device__ __forceinline__ float block_max(float v, float* redmax)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) redmax[threadIdx.x >> 6] = v;
    __syncthreads();
    float m = redmax[0];
#pragma unroll
    for (int w = 1; w < NT / 64; w++) m = fmaxf(m, redmax[w]);
    return m;
}

template <bool SCALE>
__global__ __launch_bounds__(NT) void layer_health_grads_kernel(const int64_t* __restrict__ segs, const int32_t* __restrict__ wg, float s,
                                                                double* __restrict__ records)
{
    __shared__ double red[NT / 64];
    __shared__ float redmax[NT / 64];
    const Chunk c = chunk_of(wg, segs, 2);
    const gfloat_p p = global_floats(segs[2 * c.seg]) + c.begin;

    float4_t r[U];
    int present[U];
    load_lane(p, c.len, r, present);

    unsigned count = 0;
    double sumsq = 0.0;
    float absmax = 0.f;
#pragma unroll
    for (int u = 0; u < U; u++) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (e < present[u]) {
                float y = r[u][e];
                if (SCALE) y *= s;
                if (__builtin_amdgcn_classf(y, kNotFinite)) {
                    count++;
                    y = (y != y) ? 0.f : (y > 0.f ? 1e5f : -1e5f);
                }
                const double zd = (double)y;
                sumsq += zd * zd;
                absmax = fmaxf(absmax, fabsf(y));
            }
        }
    }

    const double cnt = block_sum<NT>((double)count, red);
    const double q = block_sum<NT>(sumsq, red);
    const float m = block_max(absmax, redmax);
    if (threadIdx.x == 0) {
        double* rec = records + 3 * (int64_t)blockIdx.x;
        rec[0] = cnt; rec[1] = q; rec[2] = (double)m;
    }
}

__global__ __launch_bounds__(NT) void layer_health_updates_kernel(const int64_t* __restrict__ segs, const int32_t* __restrict__ wg, double lr, double eps,
                                                                  double bc1, double bc2, double* __restrict__ records)
{
    __shared__ double red[NT / 64];
    __shared__ float redmax[NT / 64];
    const Chunk c = chunk_of(wg, segs, 4);
    const gfloat_p pw = global_floats(segs[4 * c.seg + 0]) + c.begin;
    const gfloat_p pm = global_floats(segs[4 * c.seg + 1]) + c.begin;
    const gfloat_p pv = global_floats(segs[4 * c.seg + 2]) + c.begin;

    float4_t w[U], m[U], v[U];
    int present[U];
    load_lane(pw, c.len, w, present);
    load_lane(pm, c.len, m, present);
    load_lane(pv, c.len, v, present);

    double wsq = 0.0, dsq = 0.0;
    float wmax = 0.f;
#pragma unroll
    for (int u = 0; u < U; u++) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (e < present[u]) {
                const double wd = (double)w[u][e];
                wsq += wd * wd;
                wmax = fmaxf(wmax, fabsf(w[u][e]));
                const double d = lr * ((double)m[u][e] / bc1) / (__dsqrt_rn((double)v[u][e] / bc2) + eps);
                dsq += d * d;
            }
        }
    }

    const double a = block_sum<NT>(wsq, red);
    const double b = block_sum<NT>(dsq, red);
    const float mx = block_max(wmax, redmax);
    if (threadIdx.x == 0) {
        double* rec = records + 3 * (int64_t)blockIdx.x;
        rec[0] = a; rec[1] = (double)mx; rec[2] = b;
    }
}

// running[p] takes the records rec_start[p] .. rec_start[p + 1) of parameter p = blockIdx.x.  Lane t adds the records t, t + NT, ... in ascending
// order, block_sum (reduce.h) adds the lanes; the maximum has no order.  Fields: 0 steps, 1 steps_with_nonfinite, 2 nonfinite, 3 grad_sumsq,
// 4 grad_absmax, 5 weight_sumsq, 6 weight_absmax, 7 update_sumsq.
template <int MODE>
__global__ __launch_bounds__(NT) void layer_health_fold_kernel(const double* __restrict__ records, const int64_t* __restrict__ rec_start,
                                                               double* __restrict__ running)
{
    __shared__ double red[NT / 64];
    const int tid = threadIdx.x;
    const int64_t r0 = rec_start[blockIdx.x], r1 = rec_start[blockIdx.x + 1];
    double a = 0.0, b = 0.0, mx = 0.0;                      // the two sums and the maximum of the three values of a record
    for (int64_t r = r0 + tid; r < r1; r += NT) {
        const double v0 = records[3 * r], v1 = records[3 * r + 1], v2 = records[3 * r + 2];
        if (MODE == kGrads) { a += v0; b += v1; mx = fmax(mx, v2); }
        else                { a += v0; b += v2; mx = fmax(mx, v1); }
    }
    a = block_sum<NT>(a, red);
    b = block_sum<NT>(b, red);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) {
        double m = red[0];
#pragma unroll
        for (int w = 1; w < NT / 64; w++) m = fmax(m, red[w]);
        double* row = running + SBG_LAYER_HEALTH_FIELDS * (int64_t)blockIdx.x;
        if (MODE == kGrads) {
            row[0] += 1.0;
            row[1] += a > 0.0 ? 1.0 : 0.0;
            row[2] += a;
            row[3] += b;
            row[4] = fmax(row[4], m);
        } else {
            row[5] = a;
            row[6] = m;
            row[7] += b;
        }
    }
}

int check_tables(const char* what, const void* segs, const void* wg, int64_t records, int64_t total_n, const void* out)
{
    SBG_CHECK(records >= 0 && total_n >= 0 && records <= total_n && records < INT32_MAX, "%s: records = %lld, n = %lld", what, (long long)records,
              (long long)total_n);
    if (records == 0) return SBG_OK;
    SBG_CHECK(segs != nullptr && wg != nullptr && out != nullptr, "%s: the tables and the records must be device pointers", what);
    SBG_CHECK(sbg_aligned(segs, 8) && sbg_aligned(wg, 4) && sbg_aligned(out, 8), "%s: misaligned table or records", what);
    return SBG_OK;
}

} // namespace

extern "C" int sbg_layer_health_grads(const int64_t* segs, const int32_t* wg, int64_t records, int64_t total_n, float scale, double* out,
                                      sbg_stream_t stream)
{
    const int st = check_tables("layer_health_grads", segs, wg, records, total_n, out);
    if (st != SBG_OK || records == 0) return st;
    SBG_CHECK(scale == scale, "layer_health_grads: the scale is NaN");
    const bool scaled = scale != 1.0f;
    hipStream_t s = (hipStream_t)stream;
    SbgProfScope prof(s, SBG_K_LAYER_HEALTH, 0.0, 4.0 * (double)total_n, {kGrads, (int)records, sbg_clip31(total_n), scaled ? 1 : 0});
    if (scaled) SBG_LAUNCH(layer_health_grads_kernel<true>, dim3((unsigned)records), dim3(NT), 0, s, segs, wg, scale, out);
    else        SBG_LAUNCH(layer_health_grads_kernel<false>, dim3((unsigned)records), dim3(NT), 0, s, segs, wg, scale, out);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int sbg_layer_health_updates(const int64_t* segs, const int32_t* wg, int64_t records, int64_t total_n, double lr, double eps, double bc1,
                                        double bc2, double* out, sbg_stream_t stream)
{
    const int st = check_tables("layer_health_updates", segs, wg, records, total_n, out);
    if (st != SBG_OK || records == 0) return st;
    SBG_CHECK(lr == lr && eps >= 0.0 && bc1 > 0.0 && bc1 <= 1.0 && bc2 > 0.0 && bc2 <= 1.0,
              "layer_health_updates: lr = %g, eps = %g, bc1 = %g, bc2 = %g", lr, eps, bc1, bc2);
    hipStream_t s = (hipStream_t)stream;
    SbgProfScope prof(s, SBG_K_LAYER_HEALTH, 0.0, 12.0 * (double)total_n, {kUpdates, (int)records, sbg_clip31(total_n)});
    SBG_LAUNCH(layer_health_updates_kernel, dim3((unsigned)records), dim3(NT), 0, s, segs, wg, lr, eps, bc1, bc2, out);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int sbg_layer_health_fold(const double* records, const int64_t* rec_start, int64_t P, int64_t nrecords, int mode, double* running,
                                     sbg_stream_t stream)
{
    SBG_CHECK(P >= 0 && P < INT32_MAX && nrecords >= 0, "layer_health_fold: P = %lld, records = %lld", (long long)P, (long long)nrecords);
    SBG_CHECK(mode == kGrads || mode == kUpdates, "layer_health_fold: mode = %d (0 grads, 1 updates)", mode);
    if (P == 0) return SBG_OK;
    SBG_CHECK(rec_start != nullptr && running != nullptr && (nrecords == 0 || records != nullptr), "layer_health_fold: the tables must be device pointers");
    SBG_CHECK(sbg_aligned(records, 8) && sbg_aligned(rec_start, 8) && sbg_aligned(running, 8), "layer_health_fold: misaligned table");
    hipStream_t s = (hipStream_t)stream;
    SbgProfScope prof(s, SBG_K_LAYER_HEALTH, 0.0, 24.0 * (double)nrecords + 16.0 * 8.0 * (double)P, {kFold, sbg_clip31(P), sbg_clip31(nrecords), mode});
    if (mode == kGrads) SBG_LAUNCH(layer_health_fold_kernel<kGrads>, dim3((unsigned)P), dim3(NT), 0, s, records, rec_start, running);
    else                SBG_LAUNCH(layer_health_fold_kernel<kUpdates>, dim3((unsigned)P), dim3(NT), 0, s, records, rec_start, running);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}
