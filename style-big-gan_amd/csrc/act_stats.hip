// act_stats.hip -- device arithmetic of the network summary tool (network_summary.py): one record of counts and sums per
// (sample, channel) plane of an activation tensor, and the fold of such records into running per-channel records.  torch_utils/ops/act_stats.py
// states the same value graph for CPU tensors in numpy (built from _exact_common), so both devices give the same bits.  The full contract (the
// record, the order of the two float sums) is in include/sbg_hip.h; this file decides only how planes are mapped to workgroups.
//
// planes.  x is logically [N, C, P] with element strides (sn, sc, sp), fp16 / bf16 / fp32; every element is converted exactly to fp32.  The two
//   float64 sums of a plane are DEFINED over 256 virtual lanes: lane t adds p = t, t + 256, ... in ascending order from +0.0, then
//   block_sum<256> (reduce.h).  Everything else in the record is a count, a minimum or a maximum and does not depend on the order.  Four mappings,
//   chosen on the host by act_stats_path():
//   1 staged   P > 64, sp == 1 (dense NCHW, any base alignment).  One workgroup per plane; work-item L loads the 16-byte vector L of a chunk of
//              256 vectors, cut at the 16-byte boundaries of the ADDRESS (the first and last vector of a plane may be partial and are read
//              element by element, never outside the plane), stores it to LDS, and work-item t reads back the elements of virtual lane t in
//              ascending p.  The next chunk's load is issued before the current chunk is added.
//   2 cminor   P > 64, sc == 1, C a multiple of the vector width V (8 for 16 bits, 4 for fp32), base 16-byte aligned, sn and sp multiples of V
//              (channels_last).  One workgroup per (n, V consecutive channels); work-item t IS virtual lane t and loads the 16-byte channel
//              vector of the pixels t, t + 256, ...; V records are finished per workgroup.
//   3 group    P <= 64, any strides.  G = the power of two >= P lanes per plane, 256 / G planes per workgroup, one element per lane.  The lanes
//              above P hold +0.0, so the 64-lane butterfly of the definition reduces to its last log2 G steps and the other three waves add
//              +0.0: the same bits.  Counts are ballots; no LDS.
//   4 strided  everything else (a channel-minor tensor whose C, base or strides do not allow the vector): mapping 1 with scalar loads at stride sp.
//   Exponent bins are integer adds in LDS (mappings 1, 2, 4), into one of several copies of the histogram chosen by the work-item so that the
//   lanes of a wave that hit one binade spread over banks.  No global atomics; no float sum depends on the launch geometry.
// fold.  records [N, C, 70] / [N, C, 4] -> running [C, 70] / [C, 4], one work-item per (c, field), n ascending.  The work-item of n_peak also owns
//   min and max (the peak is read from them), so no field is read by one work-item while another writes it.
// Launch-log key: kind SBG_K_ACT_STATS, dims = {variant, ...}: 0 planes (N, C, P, mapping, dtype) / 1 fold (N, C); N, C, P clipped to INT32_MAX.
#include "sbg_common.h"
#include "reduce.h"
#include <hip/hip_fp16.h>

namespace {

constexpr int kPlanes = 0, kFold = 1;
constexpr int kStaged = 1, kCminor = 2, kGroup = 3, kStrided = 4;
constexpr int NT = 256;
constexpr int kCounts = SBG_ACT_STATS_COUNTS, kValues = SBG_ACT_STATS_VALUES, kBins = 64, kHist0 = 6;
constexpr int kPitch = kBins + 1;               // a histogram copy's pitch in LDS words: copy k, bin b sits in bank (k + b) mod 64
constexpr int kCopies = 32;                     // histogram copies of a one-plane workgroup
constexpr int kCopiesV = 8;                     // copies per channel of a channel-vector workgroup
constexpr int64_t kMaxP = ((int64_t)1 << 31) - 1 - 4096, kMaxPlanes = ((int64_t)1 << 31) - 1 - NT, kMaxStride = (int64_t)1 << 40;

template <int DT> struct Elem;
template <> struct Elem<SBG_F32> {
    typedef float raw;
    static constexpr int V = 4;
    static __device__ __forceinline__ float f32(float v) { return v; }
};
template <> struct Elem<SBG_F16> {
    typedef uint16_t raw;
    static constexpr int V = 8;
    static __device__ __forceinline__ float f32(uint16_t v) { return __half2float(__ushort_as_half(v)); }
};
template <> struct Elem<SBG_BF16> {
    typedef uint16_t raw;
    static constexpr int V = 8;
    static __device__ __forceinline__ float f32(uint16_t v) { return __uint_as_float((unsigned)v << 16); }
};

// what a lane knows of the elements it has seen: pk < 0 means no finite element yet
struct Acc {
    double s, q;
    float mn, mx, pk;
    unsigned npk, nz, nn, npi, nni;
};

static __device__ __forceinline__ void acc_init(Acc& a)
{
    a.s = a.q = 0.0;
    a.mn = INFINITY;
    a.mx = -INFINITY;
    a.pk = -1.0f;
    a.npk = a.nz = a.nn = a.npi = a.nni = 0;
}

static __device__ __forceinline__ int exponent_bin(unsigned mag)        // mag: the bits of a finite non-zero |x|; subnormals have field 0 -> bin 0
{
    const int e = (int)(mag >> 23) - 127;
    return (e < -32 ? -32 : e > 31 ? 31 : e) + 32;
}

// hist: this lane's histogram copy in LDS
static __device__ __forceinline__ void acc_add(Acc& a, float x, unsigned* hist)
{
    const unsigned bits = __float_as_uint(x), mag = bits & 0x7fffffffu;
    if (mag > 0x7f800000u) { a.nn++; return; }
    if (mag == 0x7f800000u) { if (bits >> 31) a.nni++; else a.npi++; return; }
    const double d = (double)x;
    a.s += d;
    a.q += d * d;
    float xz = x;                                                       // min and max see every zero as +0.0
    if (mag == 0) { a.nz++; xz = 0.0f; }
    else atomicAdd(hist + exponent_bin(mag), 1u);
    a.mn = xz < a.mn ? xz : a.mn;
    a.mx = xz > a.mx ? xz : a.mx;
    const float ax = __uint_as_float(mag);
    if (ax > a.pk) { a.pk = ax; a.npk = 1; }
    else if (ax == a.pk) a.npk++;
}

struct Part { float mn, mx, pk; unsigned nz, nn, npi, nni, npk; };

static __device__ __forceinline__ float wave_min(float v) { for (int o = 32; o >= 1; o >>= 1) { const float w = __shfl_xor(v, o, 64); v = w < v ? w : v; } return v; }
static __device__ __forceinline__ float wave_max(float v) { for (int o = 32; o >= 1; o >>= 1) { const float w = __shfl_xor(v, o, 64); v = w > v ? w : v; } return v; }
static __device__ __forceinline__ unsigned wave_add(unsigned v) { for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64); return v; }

// Every work-item of the 256 calls it with the lane state of ONE plane; `hist` holds `copies` histogram copies of that plane.  Writes the record.
static __device__ __forceinline__ void finish_plane(const Acc& a, const unsigned* hist, int copies, double* redd, Part* parts, int64_t P,
                                                    int64_t* __restrict__ counts, double* __restrict__ values)
{
    const int t = threadIdx.x, wave = t >> 6;
    const double S = block_sum<NT>(a.s, redd);
    const double Q = block_sum<NT>(a.q, redd);
    {
        const float mn = wave_min(a.mn), mx = wave_max(a.mx), pk = wave_max(a.pk);
        const unsigned nz = wave_add(a.nz), nn = wave_add(a.nn), npi = wave_add(a.npi), nni = wave_add(a.nni);
        if ((t & 63) == 0) {
            Part& w = parts[wave];
            w.mn = mn; w.mx = mx; w.pk = pk; w.nz = nz; w.nn = nn; w.npi = npi; w.nni = nni;
        }
    }
    __syncthreads();
    float mn = parts[0].mn, mx = parts[0].mx, pk = parts[0].pk;
    unsigned nz = parts[0].nz, nn = parts[0].nn, npi = parts[0].npi, nni = parts[0].nni;
#pragma unroll
    for (int w = 1; w < NT / 64; w++) {
        mn = parts[w].mn < mn ? parts[w].mn : mn;
        mx = parts[w].mx > mx ? parts[w].mx : mx;
        pk = parts[w].pk > pk ? parts[w].pk : pk;
        nz += parts[w].nz; nn += parts[w].nn; npi += parts[w].npi; nni += parts[w].nni;
    }
    const unsigned mine = (pk >= 0.0f && a.pk == pk) ? a.npk : 0u;
    const unsigned wnpk = wave_add(mine);
    if ((t & 63) == 0) parts[wave].npk = wnpk;
    __syncthreads();
    if (t == 0) {
        counts[0] = P;
        counts[1] = nz;
        counts[2] = nn;
        counts[3] = npi;
        counts[4] = nni;
        counts[5] = (int64_t)parts[0].npk + parts[1].npk + parts[2].npk + parts[3].npk;
        values[0] = S;
        values[1] = Q;
        values[2] = (double)mn;
        values[3] = (double)mx;
    }
    if (t < kBins) {
        unsigned h = 0;
        for (int k = 0; k < copies; k++) h += hist[k * kPitch + t];
        counts[kHist0 + t] = h;
    }
}

// Mappings 1 (STAGED, sp == 1) and 4 (scalar loads at stride sp): one workgroup per plane.
template <int DT, bool STAGED>
__global__ __launch_bounds__(NT) void act_stats_plane_kernel(const void* __restrict__ xv, int64_t C, int64_t P, int64_t sn, int64_t sc, int64_t sp,
                                                             int64_t* __restrict__ counts, double* __restrict__ values)
{
    typedef Elem<DT> E;
    typedef typename E::raw R;
    constexpr int V = E::V, EPC = NT * V;                               // elements per vector and per chunk
    __shared__ unsigned hist[kCopies * kPitch];
    __shared__ double redd[NT / 64];
    __shared__ Part parts[NT / 64];
    __shared__ uint4 stage[STAGED ? NT : 1];
    const int t = threadIdx.x;
    const int64_t plane = blockIdx.x, n = plane / C, c = plane - n * C;
    const R* base = static_cast<const R*>(xv) + n * sn + c * sc;
    for (int i = t; i < kCopies * kPitch; i += NT) hist[i] = 0;
    __syncthreads();
    unsigned* mine = hist + (t & (kCopies - 1)) * kPitch;
    Acc a;
    acc_init(a);
    if constexpr (STAGED) {
        const int shift = (int)((reinterpret_cast<uintptr_t>(base) & 15) / sizeof(R));      // elements between the 16-byte boundary below and the plane
        const R* aligned = base - shift;                                                    // never dereferenced below `base`
        const int64_t chunks = (shift + P + EPC - 1) / EPC;
        const int i0 = (t + shift) & (NT - 1);                          // chunk index i holds p = k EPC - shift + i: lane t owns i = i0 + 256 j
        auto load = [&](int64_t k) -> uint4 {
            const int64_t e0 = k * EPC + (int64_t)t * V - shift;        // the p of this vector's first element
            if (e0 >= 0 && e0 + V <= P) return *reinterpret_cast<const uint4*>(aligned + k * EPC + t * V);
            union { uint4 v; R r[V]; } u;
            u.v = make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int j = 0; j < V; j++)
                if (e0 + j >= 0 && e0 + j < P) u.r[j] = base[e0 + j];
            return u.v;
        };
        uint4 v = load(0);
        const R* st = reinterpret_cast<const R*>(stage);
        for (int64_t k = 0; k < chunks; k++) {
            __syncthreads();                                            // the previous chunk has been read
            stage[t] = v;
            __syncthreads();
            if (k + 1 < chunks) v = load(k + 1);
            const int64_t lo = k * EPC - shift;
#pragma unroll
            for (int j = 0; j < V; j++) {
                const int i = i0 + NT * j;
                const int64_t p = lo + i;
                if (p >= 0 && p < P) acc_add(a, E::f32(st[i]), mine);
            }
        }
    } else {
#pragma unroll 4
        for (int64_t p = t; p < P; p += NT) acc_add(a, E::f32(base[p * sp]), mine);
    }
    finish_plane(a, hist, kCopies, redd, parts, P, counts + plane * kCounts, values + plane * kValues);
}

// Mapping 2: one workgroup per (n, V consecutive channels); work-item t is virtual lane t of all V planes.
template <int DT>
__global__ __launch_bounds__(NT) void act_stats_cminor_kernel(const void* __restrict__ xv, int64_t C, int64_t P, int64_t sn, int64_t sp,
                                                              int64_t* __restrict__ counts, double* __restrict__ values)
{
    typedef Elem<DT> E;
    typedef typename E::raw R;
    constexpr int V = E::V;
    __shared__ unsigned hist[V * kCopiesV * kPitch];
    __shared__ double redd[NT / 64];
    __shared__ Part parts[NT / 64];
    const int t = threadIdx.x;
    const int64_t vectors = C / V, n = blockIdx.x / vectors, c0 = (blockIdx.x - n * vectors) * V;
    const R* base = static_cast<const R*>(xv) + n * sn + c0;
    for (int i = t; i < V * kCopiesV * kPitch; i += NT) hist[i] = 0;
    __syncthreads();
    unsigned* mine = hist + (t & (kCopiesV - 1)) * kPitch;
    Acc a[V];
#pragma unroll
    for (int j = 0; j < V; j++) acc_init(a[j]);
    union Vec { uint4 v; R r[V]; };
    int64_t p = t;
    for (; p + NT < P; p += 2 * NT) {                                   // two loads in flight
        Vec u0, u1;
        u0.v = *reinterpret_cast<const uint4*>(base + p * sp);
        u1.v = *reinterpret_cast<const uint4*>(base + (p + NT) * sp);
#pragma unroll
        for (int j = 0; j < V; j++) acc_add(a[j], E::f32(u0.r[j]), mine + j * kCopiesV * kPitch);
#pragma unroll
        for (int j = 0; j < V; j++) acc_add(a[j], E::f32(u1.r[j]), mine + j * kCopiesV * kPitch);
    }
    if (p < P) {
        Vec u0;
        u0.v = *reinterpret_cast<const uint4*>(base + p * sp);
#pragma unroll
        for (int j = 0; j < V; j++) acc_add(a[j], E::f32(u0.r[j]), mine + j * kCopiesV * kPitch);
    }
    const int64_t plane = n * C + c0;
#pragma unroll
    for (int j = 0; j < V; j++)
        finish_plane(a[j], hist + j * kCopiesV * kPitch, kCopiesV, redd, parts, P, counts + (plane + j) * kCounts, values + (plane + j) * kValues);
}

// Mapping 3: G = 1 << lg lanes per plane (P <= G <= 64), one element per lane, ballots for the counts.
template <int DT>
__global__ __launch_bounds__(NT) void act_stats_group_kernel(const void* __restrict__ xv, int64_t planes, int64_t C, int P, int64_t sn, int64_t sc,
                                                             int64_t sp, int lg, int64_t* __restrict__ counts, double* __restrict__ values)
{
    typedef Elem<DT> E;
    typedef typename E::raw R;
    const int G = 1 << lg;
    const int64_t gid = (int64_t)blockIdx.x * NT + threadIdx.x, plane = gid >> lg;
    const int p = (int)(gid & (G - 1)), lane = threadIdx.x & 63;
    const bool live = plane < planes, valid = live && p < P;
    float x = 0.0f;
    if (valid) {
        const int64_t n = plane / C, c = plane - n * C;
        x = E::f32(static_cast<const R*>(xv)[n * sn + c * sc + (int64_t)p * sp]);
    }
    const unsigned bits = __float_as_uint(x), mag = bits & 0x7fffffffu;
    const bool finite = valid && mag < 0x7f800000u, nonzero = finite && mag != 0;
    const unsigned long long gmask = (G == 64 ? ~0ull : ((1ull << G) - 1)) << (lane & ~(G - 1));
    auto count = [&](bool flag) -> int64_t { return (int64_t)__popcll(__ballot(flag) & gmask); };
    const double d = finite ? (double)x : 0.0;
    double s = 0.0 + d, q = d * d;                                      // the lane's sum from +0.0; the lanes above P hold +0.0
    float mn = finite ? (mag == 0 ? 0.0f : x) : INFINITY, mx = finite ? (mag == 0 ? 0.0f : x) : -INFINITY, pk = finite ? __uint_as_float(mag) : -1.0f;
    for (int o = G >> 1; o >= 1; o >>= 1) {                             // the last lg steps of wave_sum; the first 6 - lg add +0.0
        s += __shfl_xor(s, o, 64);
        q += __shfl_xor(q, o, 64);
        const float a = __shfl_xor(mn, o, 64), b = __shfl_xor(mx, o, 64), k = __shfl_xor(pk, o, 64);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
        pk = k > pk ? k : pk;
    }
    const int64_t nz = count(finite && mag == 0), nn = count(valid && mag > 0x7f800000u);
    const int64_t npi = count(valid && mag == 0x7f800000u && !(bits >> 31)), nni = count(valid && mag == 0x7f800000u && (bits >> 31));
    const int64_t npk = count(finite && __uint_as_float(mag) == pk);
    const int bin = nonzero ? exponent_bin(mag) : -1;
    int64_t* cr = counts + (live ? plane : 0) * kCounts;
    for (int b = 0; b < kBins; b++) {
        const int64_t h = count(bin == b);
        if (live && p == (b & (G - 1))) cr[kHist0 + b] = h;
    }
    if (live && p == 0) {
        cr[0] = P;
        cr[1] = nz;
        cr[2] = nn;
        cr[3] = npi;
        cr[4] = nni;
        cr[5] = npk;
        double* vr = values + plane * kValues;
        vr[0] = s;
        vr[1] = q;
        vr[2] = (double)mn;
        vr[3] = (double)mx;
    }
}

static __device__ __forceinline__ double record_peak(double mn, double mx) { return mn <= mx ? fmax(fabs(mn), fabs(mx)) : -1.0; }

// one work-item per (c, field): fields 0 .. 69 the counts, 70 .. 73 the values.  Field 5 (n_peak) also folds min and max; fields 72, 73 are idle.
__global__ __launch_bounds__(NT) void act_stats_fold_kernel(const int64_t* __restrict__ counts, const double* __restrict__ values,
                                                            int64_t* __restrict__ run_counts, double* __restrict__ run_values, int64_t N, int64_t C)
{
    constexpr int F = kCounts + kValues;
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= C * F) return;
    const int64_t c = i / F;
    const int f = (int)(i - c * F);
    if (f == 5) {
        double mn = run_values[c * kValues + 2], mx = run_values[c * kValues + 3];
        int64_t npk = run_counts[c * kCounts + 5];
        for (int64_t n = 0; n < N; n++) {
            const double rmn = values[(n * C + c) * kValues + 2], rmx = values[(n * C + c) * kValues + 3];
            const double have = record_peak(mn, mx), got = record_peak(rmn, rmx);
            const int64_t rn = counts[(n * C + c) * kCounts + 5];
            npk = got > have ? rn : got == have ? npk + rn : npk;
            mn = rmn < mn ? rmn : mn;
            mx = rmx > mx ? rmx : mx;
        }
        run_counts[c * kCounts + 5] = npk;
        run_values[c * kValues + 2] = mn;
        run_values[c * kValues + 3] = mx;
    } else if (f < kCounts) {
        int64_t v = run_counts[c * kCounts + f];
        for (int64_t n = 0; n < N; n++) v += counts[(n * C + c) * kCounts + f];
        run_counts[c * kCounts + f] = v;
    } else if (f < kCounts + 2) {
        const int k = f - kCounts;
        double v = run_values[c * kValues + k];
        for (int64_t n = 0; n < N; n++) v += values[(n * C + c) * kValues + k];
        run_values[c * kValues + k] = v;
    }
}

bool shape_ok(int dtype, int64_t N, int64_t C, int64_t P, int64_t sn, int64_t sc, int64_t sp)
{
    if (dtype != SBG_F32 && dtype != SBG_F16 && dtype != SBG_BF16) return false;
    if (N < 1 || C < 1 || P < 1 || P > kMaxP || N > kMaxPlanes || C > kMaxPlanes || N * C > kMaxPlanes) return false;
    if (sn < 0 || sc < 0 || sp < 0 || sn > kMaxStride || sc > kMaxStride || sp > kMaxStride) return false;
    return (N == 1 || sn >= 1) && (C == 1 || sc >= 1) && (P == 1 || sp >= 1);
}

int path_of(int dtype, int64_t C, int64_t P, int64_t sn, int64_t sc, int64_t sp, uintptr_t base, int64_t N)
{
    const int V = dtype == SBG_F32 ? 4 : 8;
    if (P <= 64) return kGroup;
    if (sp == 1) return kStaged;
    if ((sc == 1 || C == 1) && C % V == 0 && (base & 15) == 0 && (N == 1 || sn % V == 0) && sp % V == 0) return kCminor;
    return kStrided;
}

template <int DT>
int launch_planes(int path, const void* x, int64_t N, int64_t C, int64_t P, int64_t sn, int64_t sc, int64_t sp, int64_t* counts, double* values,
                  hipStream_t s)
{
    const int64_t planes = N * C;
    if (path == kStaged)
        SBG_LAUNCH((act_stats_plane_kernel<DT, true>), dim3((unsigned)planes), dim3(NT), 0, s, x, C, P, sn, sc, sp, counts, values);
    else if (path == kStrided)
        SBG_LAUNCH((act_stats_plane_kernel<DT, false>), dim3((unsigned)planes), dim3(NT), 0, s, x, C, P, sn, sc, sp, counts, values);
    else if (path == kCminor)
        SBG_LAUNCH((act_stats_cminor_kernel<DT>), dim3((unsigned)(N * (C / Elem<DT>::V))), dim3(NT), 0, s, x, C, P, sn, sp, counts, values);
    else {
        int lg = 0;
        while ((1 << lg) < P) lg++;
        const int64_t blocks = ((planes << lg) + NT - 1) / NT;
        SBG_LAUNCH((act_stats_group_kernel<DT>), dim3((unsigned)blocks), dim3(NT), 0, s, x, planes, C, (int)P, sn, sc, sp, lg, counts, values);
    }
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

} // namespace

extern "C" int sbg_act_stats_path(const void* x, int dtype, int64_t N, int64_t C, int64_t P, int64_t sn, int64_t sc, int64_t sp)
{
    if (!shape_ok(dtype, N, C, P, sn, sc, sp)) return -1;
    return path_of(dtype, C, P, sn, sc, sp, reinterpret_cast<uintptr_t>(x), N);
}

extern "C" int sbg_act_stats_planes(const void* x, int dtype, int64_t N, int64_t C, int64_t P, int64_t sn, int64_t sc, int64_t sp, int64_t* counts,
                                    double* values, sbg_stream_t stream)
{
    SBG_CHECK(shape_ok(dtype, N, C, P, sn, sc, sp), "act_stats_planes: bad input: dtype %d, [N, C, P] = [%lld, %lld, %lld], strides (%lld, %lld, %lld) "
              "(fp32 / fp16 / bf16; 1 <= P < 2^31 - 4096; N C < 2^31 - 256; strides in [1, 2^40] wherever the size is above 1)", dtype, (long long)N,
              (long long)C, (long long)P, (long long)sn, (long long)sc, (long long)sp);
    const uintptr_t esize = dtype == SBG_F32 ? 4 : 2;
    SBG_CHECK(x && counts && values && sbg_aligned(x, esize) && sbg_aligned(counts, 8) && sbg_aligned(values, 8),
              "act_stats_planes: null or misaligned pointer for [%lld, %lld, %lld]", (long long)N, (long long)C, (long long)P);
    hipStream_t s = (hipStream_t)stream;
    const int path = path_of(dtype, C, P, sn, sc, sp, reinterpret_cast<uintptr_t>(x), N);
    SbgProfScope prof(s, SBG_K_ACT_STATS, 0.0, (double)N * C * ((double)P * esize + 8.0 * (kCounts + kValues)),
                      {kPlanes, sbg_clip31(N), sbg_clip31(C), sbg_clip31(P), path, dtype});
    return dtype == SBG_F32 ? launch_planes<SBG_F32>(path, x, N, C, P, sn, sc, sp, counts, values, s)
         : dtype == SBG_F16 ? launch_planes<SBG_F16>(path, x, N, C, P, sn, sc, sp, counts, values, s)
                            : launch_planes<SBG_BF16>(path, x, N, C, P, sn, sc, sp, counts, values, s);
}

extern "C" int sbg_act_stats_fold(const int64_t* counts, const double* values, int64_t* run_counts, double* run_values, int64_t N, int64_t C,
                                  sbg_stream_t stream)
{
    SBG_CHECK(N >= 0 && C >= 1 && N <= kMaxPlanes && C <= kMaxPlanes / (kCounts + kValues) && (N == 0 || N * C <= kMaxPlanes),
              "act_stats_fold: bad shape [N, C] = [%lld, %lld] (0 <= N, 1 <= C, N C < 2^31 - 256, 74 C < 2^31 - 256)", (long long)N, (long long)C);
    if (N == 0) return SBG_OK;
    SBG_CHECK(counts && values && run_counts && run_values && sbg_aligned(counts, 8) && sbg_aligned(values, 8) && sbg_aligned(run_counts, 8) &&
              sbg_aligned(run_values, 8), "act_stats_fold: null or misaligned pointer for [%lld, %lld]", (long long)N, (long long)C);
    hipStream_t s = (hipStream_t)stream;
    const int64_t items = C * (kCounts + kValues);
    SbgProfScope prof(s, SBG_K_ACT_STATS, 0.0, 8.0 * (kCounts + kValues) * (double)C * (double)(N + 2), {kFold, sbg_clip31(N), sbg_clip31(C)});
    SBG_LAUNCH(act_stats_fold_kernel, dim3((unsigned)((items + NT - 1) / NT)), dim3(NT), 0, s, counts, values, run_counts, run_values, N, C);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}
