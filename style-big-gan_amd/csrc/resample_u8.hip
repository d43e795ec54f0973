// resample_u8.hip -- the two passes of PIL's `Image.resize` on 8-bit images, the arithmetic of the reference's data set tool
// (stylegan2ada/dataset_tool.py:199-248, `img.resize((w, h), LANCZOS | BOX)`), in integers and therefore bit for bit:
//   out = clamp((2^21 + sum_k in[first + k] * coeff[k]) >> 22, 0, 255),  wrapping int32 sum, arithmetic shift,
// with one window (first, count) and `count` 22-bit fixed-point coefficients per output index, computed on the host.  The horizontal pass
// runs first and its result is rounded to uint8 before the vertical pass, as in PIL; the op layer skips a pass that does not change its extent.
//   resample_h:  a workgroup stages the input span of `strip` output pixels of R rows in LDS (coalesced dwords, bytes at the unaligned head
//                and tail: a crop box may start at any byte), then a work-item sums one output pixel, all channels, from LDS.  The table is
//                tap-major so that the lanes of a wave read consecutive coefficients.
//   resample_v:  a row is a flat array of width * C bytes; a work-item owns one dword of an output row and walks the taps down the input rows.
//                A wave covers 64 consecutive dwords of one row, so its window and coefficients are uniform.  No LDS.
// Every window is clipped to the staged span / the input extent before it is used: a table that does not fit the sizes gives wrong
// bytes, never an access outside the images.
// Launch-log key: kind SBG_K_RESAMPLE, dims[0] = variant (0 h, 1 v), then the shape and the kernel variant.
#include "sbg_common.h"

namespace {

constexpr int kVarH = 0, kVarV = 1;
constexpr int kPrecisionBits = 22;                          // 32 - 8 - 2, PIL's PRECISION_BITS
constexpr unsigned kHalf = 1u << (kPrecisionBits - 1);
constexpr int kLdsBudget = 60 * 1024;

// The sum is kept unsigned (wrapping is defined) and read as int32.  clamp(acc >> 22, 0, 255) is written as the clamp of acc to
// [0, 2^30 - 1] followed by a logical shift, which is the same value.  The shift-then-clamp spelling is kept out on purpose: hipcc
// matches two neighbouring bytes of it to v_ashr_pk_u8_i32 and ORs the other two bytes into that instruction's destination, and the
// vertical kernel built that way wrote wrong bytes 2 and 3 in every output dword on an MI355X while bytes 0 and 1 were right -- what
// one sees if the instruction leaves bits 31:16 of its destination as they were and the compiler takes them to be zero.
__device__ __forceinline__ unsigned clip8(unsigned acc)
{
    constexpr int kTop = (256 << kPrecisionBits) - 1;
    int v = (int)acc;
    v = v < 0 ? 0 : v > kTop ? kTop : v;
    return (unsigned)v >> kPrecisionBits;
}

// Block = strip x R work-items.  Workgroup (s, g, n): output pixels [s * strip, +strip) of rows [g * R, +R) of image n.
// LDS row r holds the bytes [a_al, a1) of input row g * R + r, a_al = the span's first byte rounded down to a dword: lds_row bytes each.
template <int C>
__global__ __launch_bounds__(256) void resample_h_kernel(const uint8_t* __restrict__ src, int64_t src_img_stride, int64_t src_pitch,
                                                         uint8_t* __restrict__ dst, int64_t dst_img_stride, int64_t dst_pitch, int rows, int in_w,
                                                         int out_w, const int* __restrict__ bounds, const int* __restrict__ coeffs_t, int ksize,
                                                         int strip, int R, int span, int lds_row, int nstrips, int ngroups)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, nthreads = blockDim.x;
    int b = blockIdx.x;
    const int s = b % nstrips;  b /= nstrips;
    const int g = b % ngroups;
    const int n = b / ngroups;
    const int x0 = s * strip;
    int first0 = bounds[2 * x0];
    first0 = first0 < 0 ? 0 : first0 > in_w ? in_w : first0;
    const int end = first0 + span < in_w ? first0 + span : in_w;         // the staged span: input pixels [first0, end)
    const uint8_t* img = src + n * src_img_stride;

    for (int r = 0; r < R; r++) {
        const int y = g * R + r;
        if (y >= rows) break;
        const uint8_t* row = img + y * src_pitch;
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(row + (int64_t)first0 * C), a1 = reinterpret_cast<uintptr_t>(row + (int64_t)end * C);
        const uintptr_t a_al = a0 & ~(uintptr_t)3;
        const int ndw = (int)((a1 - a_al + 3) >> 2);                      // <= lds_row / 4: a1 - a_al <= 3 + span * C
        uint8_t* l8 = lds + r * lds_row;
        for (int d = tid; d < ndw; d += nthreads) {
            const uintptr_t ga = a_al + 4 * (uintptr_t)d;
            if (ga >= a0 && ga + 4 <= a1) {
                reinterpret_cast<unsigned*>(l8)[d] = *reinterpret_cast<const unsigned*>(ga);
            } else {                                                     // the dwords that hold the span's first and last bytes
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (ga + k >= a0 && ga + k < a1) l8[4 * d + k] = *reinterpret_cast<const uint8_t*>(ga + k);
            }
        }
    }
    __syncthreads();

    const int tx = tid & (strip - 1), ty = tid / strip;
    const int x = x0 + tx, y = g * R + ty;
    if (x >= out_w || y >= rows) return;
    int first = bounds[2 * x], cnt = bounds[2 * x + 1];
    if (first < 0 || first > in_w) { first = first0; cnt = 0; }
    cnt = cnt < ksize ? cnt : ksize;
    const int k0 = first < first0 ? first0 - first : 0;                  // taps in front of the span (a foreign table): not read
    const int k1 = cnt < end - first ? cnt : end - first;
    const int head = (int)(reinterpret_cast<uintptr_t>(img + y * src_pitch + (int64_t)first0 * C) & 3);
    const uint8_t* p = lds + ty * lds_row + head + (first - first0) * C;
    unsigned acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = kHalf;
    for (int k = k0; k < k1; k++) {
        const unsigned w = (unsigned)coeffs_t[(int64_t)k * out_w + x];
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] += p[k * C + c] * w;
    }
    uint8_t* o = dst + n * dst_img_stride + y * dst_pitch + (int64_t)x * C;
#pragma unroll
    for (int c = 0; c < C; c++) o[c] = (uint8_t)clip8(acc[c]);
}

// Block = 64 dwords x 4 output rows.  DWORD: the source rows are dword aligned and padded to whole dwords; else four guarded byte loads.
template <bool DWORD>
__global__ __launch_bounds__(256) void resample_v_kernel(const uint8_t* __restrict__ src, int64_t src_img_stride, int64_t src_pitch,
                                                         uint8_t* __restrict__ dst, int64_t dst_img_stride, int64_t dst_pitch, int row_bytes, int in_h,
                                                         int out_h, const int* __restrict__ bounds, const int* __restrict__ coeffs, int ksize,
                                                         int ncols, int ngroups)
{
    int b = blockIdx.x;
    const int cb = b % ncols;  b /= ncols;
    const int g = b % ngroups;
    const int n = b / ngroups;
    const int j = cb * 64 + (threadIdx.x & 63), y = g * 4 + (threadIdx.x >> 6);
    if (4 * (int64_t)j >= row_bytes || y >= out_h) return;
    int first = bounds[2 * y], cnt = bounds[2 * y + 1];
    if (first < 0 || first > in_h) { first = 0; cnt = 0; }
    cnt = cnt < ksize ? cnt : ksize;
    cnt = cnt < in_h - first ? cnt : in_h - first;
    const uint8_t* p = src + n * src_img_stride + first * src_pitch + 4 * (int64_t)j;
    const int* w = coeffs + (int64_t)y * ksize;
    const int valid = row_bytes - 4 * j;                                 // bytes of this dword inside the row (>= 4 except at the row's end)
    unsigned acc[4] = {kHalf, kHalf, kHalf, kHalf};
    for (int k = 0; k < cnt; k++) {
        const unsigned wk = (unsigned)w[k];
        const uint8_t* q = p + k * src_pitch;
        unsigned v;
        if (DWORD) {
            v = *reinterpret_cast<const unsigned*>(q);
        } else {
            v = 0;
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (i < valid) v |= (unsigned)q[i] << (8 * i);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) acc[i] += ((v >> (8 * i)) & 255u) * wk;
    }
    *reinterpret_cast<unsigned*>(dst + n * dst_img_stride + y * dst_pitch + 4 * (int64_t)j) =
        clip8(acc[0]) | (clip8(acc[1]) << 8) | (clip8(acc[2]) << 16) | (clip8(acc[3]) << 24);
}

inline bool mult4(int64_t v) { return (v & 3) == 0; }

} // namespace

extern "C" int sbg_u8_resample_h(const uint8_t* src, int64_t src_img_stride, int64_t src_pitch, uint8_t* dst, int64_t dst_img_stride, int64_t dst_pitch,
                                 int N, int rows, int in_w, int out_w, int C, const int* bounds, const int* coeffs_t, int ksize, int strip, int span,
                                 sbg_stream_t stream)
{
    SBG_CHECK(src && dst && bounds && coeffs_t, "u8_resample_h: null pointer");
    SBG_CHECK(C == 1 || C == 3, "u8_resample_h: C must be 1 or 3, got %d", C);
    SBG_CHECK(N >= 1 && rows >= 1 && in_w >= 1 && out_w >= 1 && ksize >= 1, "u8_resample_h: bad sizes N=%d rows=%d in_w=%d out_w=%d ksize=%d", N, rows,
              in_w, out_w, ksize);
    SBG_CHECK((int64_t)in_w * C <= (1 << 30) && (int64_t)out_w * C <= (1 << 30), "u8_resample_h: rows too long");
    SBG_CHECK(src_pitch >= (int64_t)in_w * C && dst_pitch >= (int64_t)out_w * C, "u8_resample_h: a pitch is shorter than its row");
    SBG_CHECK(src_img_stride >= 0 && (N == 1 || dst_img_stride >= (int64_t)(rows - 1) * dst_pitch + (int64_t)out_w * C),
              "u8_resample_h: bad image stride");
    SBG_CHECK(strip >= 16 && strip <= 256 && (strip & (strip - 1)) == 0, "u8_resample_h: strip must be a power of two in [16, 256], got %d", strip);
    SBG_CHECK(span >= 1 && span <= in_w, "u8_resample_h: span %d outside [1, in_w = %d]", span, in_w);
    const int64_t lds_row = ((int64_t)span * C + 3 + 3) / 4 * 4;
    SBG_CHECK(lds_row <= kLdsBudget, "u8_resample_h: the span of one strip (%d pixels x %d channels) does not fit the %d bytes of LDS", span, C,
              kLdsBudget);
    int R = 256 / strip;
    while (R > 1 && (R * lds_row > kLdsBudget || R / 2 >= rows)) R /= 2;
    const int nstrips = (out_w + strip - 1) / strip, ngroups = (rows + R - 1) / R;
    const int64_t blocks = (int64_t)nstrips * ngroups * N;
    SBG_CHECK(blocks <= 0x7fffffff, "u8_resample_h: too many workgroups");
    hipStream_t s = (hipStream_t)stream;
    SbgProfScope prof(s, SBG_K_RESAMPLE, 0.0, (double)N * rows * ((double)in_w + out_w) * C, {kVarH, N, rows, in_w, out_w, C, strip});
    const dim3 grid((unsigned)blocks), block((unsigned)(strip * R));
    const size_t lds = (size_t)(R * lds_row);
    if (C == 3) SBG_LAUNCH(resample_h_kernel<3>, grid, block, lds, s, src, src_img_stride, src_pitch, dst, dst_img_stride, dst_pitch, rows, in_w, out_w,
                           bounds, coeffs_t, ksize, strip, R, span, (int)lds_row, nstrips, ngroups);
    else        SBG_LAUNCH(resample_h_kernel<1>, grid, block, lds, s, src, src_img_stride, src_pitch, dst, dst_img_stride, dst_pitch, rows, in_w, out_w,
                           bounds, coeffs_t, ksize, strip, R, span, (int)lds_row, nstrips, ngroups);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}

extern "C" int sbg_u8_resample_v(const uint8_t* src, int64_t src_img_stride, int64_t src_pitch, uint8_t* dst, int64_t dst_img_stride, int64_t dst_pitch,
                                 int N, int row_bytes, int in_h, int out_h, const int* bounds, const int* coeffs, int ksize, sbg_stream_t stream)
{
    SBG_CHECK(src && dst && bounds && coeffs, "u8_resample_v: null pointer");
    SBG_CHECK(N >= 1 && row_bytes >= 1 && in_h >= 1 && out_h >= 1 && ksize >= 1, "u8_resample_v: bad sizes N=%d row_bytes=%d in_h=%d out_h=%d ksize=%d", N,
              row_bytes, in_h, out_h, ksize);
    SBG_CHECK(row_bytes <= (1 << 30), "u8_resample_v: rows too long");
    const int64_t padded = ((int64_t)row_bytes + 3) / 4 * 4;
    SBG_CHECK(src_pitch >= row_bytes && src_img_stride >= 0, "u8_resample_v: the source pitch is shorter than a row, or a negative image stride");
    SBG_CHECK(sbg_aligned(dst, 4) && mult4(dst_pitch) && mult4(dst_img_stride) && dst_pitch >= padded,
              "u8_resample_v: dst, dst_pitch and dst_img_stride must be multiples of 4 and dst_pitch >= %lld", (long long)padded);
    SBG_CHECK(N == 1 || dst_img_stride >= (int64_t)out_h * dst_pitch, "u8_resample_v: bad image stride");
    const bool dword = sbg_aligned(src, 4) && mult4(src_pitch) && mult4(src_img_stride) && src_pitch >= padded;
    const int ncols = (int)((padded / 4 + 63) / 64), ngroups = (out_h + 3) / 4;
    const int64_t blocks = (int64_t)ncols * ngroups * N;
    SBG_CHECK(blocks <= 0x7fffffff, "u8_resample_v: too many workgroups");
    hipStream_t s = (hipStream_t)stream;
    SbgProfScope prof(s, SBG_K_RESAMPLE, 0.0, (double)N * row_bytes * ((double)in_h + out_h), {kVarV, N, row_bytes, in_h, out_h, ksize, dword ? 1 : 2});
    const dim3 grid((unsigned)blocks), block(256);
    if (dword) SBG_LAUNCH(resample_v_kernel<true>, grid, block, 0, s, src, src_img_stride, src_pitch, dst, dst_img_stride, dst_pitch, row_bytes, in_h, out_h,
                          bounds, coeffs, ksize, ncols, ngroups);
    else       SBG_LAUNCH(resample_v_kernel<false>, grid, block, 0, s, src, src_img_stride, src_pitch, dst, dst_img_stride, dst_pitch, row_bytes, in_h, out_h,
                          bounds, coeffs, ksize, ncols, ngroups);
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}
