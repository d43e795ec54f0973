// resident_set.hip -- one training batch out of a device-resident uint8 image store: gather by slot, mirror, normalise through a table.
// Replaces, per step, the reference's host path: `Dataset.__getitem__` (train_parts/datasets.py:78-83: load, `image[:, :, ::-1]` when the
// item is a mirrored one), the collate and PCIe copy of the stock DataLoader, and `img.to(torch.float32) / 127.5 - 1`
// (train_parts/trainers.py:716).
//   out[b, c, y, x] = T(store[slot[b], c, y, flip[b] ? W - 1 - x : x]),   T = identity (uint8 out) or lut[.] (fp32 out)
// The kernel does no floating-point arithmetic: the caller supplies the 256 fp32 values a byte can become (the op layer evaluates the
// trainer's own expression over 0..255 on the training device), so the result is bit for bit what that expression gives.
//   dword path:  W % 4 == 0, `store` 4-byte aligned, `out` 16-byte (fp32) / 4-byte (uint8) aligned.  A work-item owns 4 consecutive output
//                pixels of a row: one dword load from column x, or from column W - 4 - x with its bytes reversed when the image is
//                mirrored, four table look-ups in LDS, one 16-byte store (one dword store for uint8).
//   byte path:   anything else; one pixel per work-item, byte loads.
// A workgroup works on 256 consecutive work-items of ONE image, so slot[b] and flip[b] are uniform in it; workgroups stride over
// (image, chunk) pairs.  The table is copied to LDS (1 KiB) once per workgroup.  Image offsets are 64-bit (FFHQ at 256^2 is 13.8 GB).
// A slot outside [0, S) is never dereferenced: that image of `out` is NaN (fp32) or 0 (uint8), as in ws_truncate_mix.
// Launch-log key: kind SBG_K_RESIDENT, dims = {B, C, H, W, out_f32, 0, path (1 dword, 2 byte)}.
#include "sbg_common.h"

namespace {

constexpr int kPathDword = 1, kPathByte = 2;
constexpr int kBlock = 256;

// DWORD: 4 pixels per work-item, else 1.  `per_image` = work-items per image, `chunks` = ceil(per_image / 256), `wq` = work-items per row.
template <bool F32, bool DWORD>
__global__ __launch_bounds__(kBlock) void gather_images_kernel(const uint8_t* __restrict__ store, int64_t S, int64_t image_bytes, int W,
                                                               const int* __restrict__ slot, const uint8_t* __restrict__ flip, void* __restrict__ out,
                                                               const float* __restrict__ lut, int per_image, int wq, int chunks, int64_t nblocks)
{
    __shared__ float table[256];
    if (F32) {
        table[threadIdx.x] = lut[threadIdx.x];
        __syncthreads();
    }
    for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const int b = (int)(blk / chunks);
        const int r = (int)(blk - (int64_t)b * chunks) * kBlock + (int)threadIdx.x;      // work-item inside image b
        if (r >= per_image) continue;
        const int64_t s = slot[b];
        const bool ok = s >= 0 && s < S;
        const bool mirror = flip != nullptr && flip[b] != 0;
        const int row = r / wq, q = r - row * wq;                                         // row = c * H + y
        if (DWORD) {
            const int64_t o = (int64_t)b * image_bytes + 4 * (int64_t)r;                  // first of this work-item's 4 output pixels
            unsigned v = 0;
            if (ok) {
                const int col = mirror ? W - 4 - 4 * q : 4 * q;
                v = *reinterpret_cast<const unsigned*>(store + s * image_bytes + (int64_t)row * W + col);
                if (mirror) v = __builtin_bswap32(v);
            }
            if (F32) {
                float4_t f;
                if (ok) {
                    f[0] = table[v & 255u]; f[1] = table[(v >> 8) & 255u]; f[2] = table[(v >> 16) & 255u]; f[3] = table[v >> 24];
                } else {
                    f[0] = f[1] = f[2] = f[3] = __builtin_nanf("");
                }
                *reinterpret_cast<float4_t*>(static_cast<float*>(out) + o) = f;
            } else {
                *reinterpret_cast<unsigned*>(static_cast<uint8_t*>(out) + o) = v;
            }
        } else {
            const int64_t o = (int64_t)b * image_bytes + r;
            unsigned v = 0;
            if (ok) v = store[s * image_bytes + (int64_t)row * W + (mirror ? W - 1 - q : q)];
            if (F32) static_cast<float*>(out)[o] = ok ? table[v] : __builtin_nanf("");
            else     static_cast<uint8_t*>(out)[o] = (uint8_t)v;
        }
    }
}


// the one place that decides the path
inline int gather_path(const uint8_t* store, int W, const void* out, int out_f32)
{
    return (W % 4 == 0 && sbg_aligned(store, 4) && sbg_aligned(out, out_f32 ? 16 : 4)) ? kPathDword : kPathByte;
}

} // namespace

extern "C" int sbg_u8_gather_images(const uint8_t* store, int64_t S, int C, int H, int W, const int32_t* slot, const uint8_t* flip, int B, void* out,
                                    int out_f32, const float* lut, sbg_stream_t stream)
{
    SBG_CHECK(store && slot && out, "u8_gather_images: null pointer");
    SBG_CHECK(out_f32 == 0 || out_f32 == 1, "u8_gather_images: out_f32 must be 0 or 1, got %d", out_f32);
    SBG_CHECK(!out_f32 || lut, "u8_gather_images: fp32 output needs the table of 256 values");
    SBG_CHECK(S >= 1 && C >= 1 && H >= 1 && W >= 1 && B >= 1, "u8_gather_images: bad sizes S=%lld C=%d H=%d W=%d B=%d", (long long)S, C, H, W, B);
    const int64_t image_bytes = (int64_t)C * H * W;
    SBG_CHECK(image_bytes <= 0x7fffffff - kBlock, "u8_gather_images: an image of %lld values is too large", (long long)image_bytes);   // chunks * 256 stays an int
    SBG_CHECK(S <= INT64_MAX / image_bytes, "u8_gather_images: the store's size overflows");
    SBG_CHECK(sbg_aligned(slot, 4) && (!out_f32 || (sbg_aligned(out, 4) && sbg_aligned(lut, 4))), "u8_gather_images: slot, lut and an fp32 out must be 4-byte aligned");
    const int path = gather_path(store, W, out, out_f32);
    const bool dword = path == kPathDword;
    const int wq = dword ? W / 4 : W;
    const int per_image = (int)(dword ? image_bytes / 4 : image_bytes);
    const int chunks = (per_image + kBlock - 1) / kBlock;
    const int64_t nblocks = (int64_t)B * chunks;
    hipStream_t s = (hipStream_t)stream;
    const double bytes = (double)B * image_bytes * (out_f32 ? 5.0 : 2.0) + (double)B * (flip ? 5.0 : 4.0) + (out_f32 ? 1024.0 : 0.0);
    SbgProfScope prof(s, SBG_K_RESIDENT, 0.0, bytes, {B, C, H, W, out_f32, 0, path});
    const dim3 grid((unsigned)(nblocks < 256 * 8 ? nblocks : 256 * 8)), block(kBlock);
#define SBG_GATHER_LAUNCH(F32, DW) SBG_LAUNCH((gather_images_kernel<F32, DW>), grid, block, 0, s, store, S, image_bytes, W, slot, flip, out, lut, per_image, \
                                              wq, chunks, nblocks)
    if (out_f32) { if (dword) SBG_GATHER_LAUNCH(true, true); else SBG_GATHER_LAUNCH(true, false); }
    else         { if (dword) SBG_GATHER_LAUNCH(false, true); else SBG_GATHER_LAUNCH(false, false); }
#undef SBG_GATHER_LAUNCH
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}
