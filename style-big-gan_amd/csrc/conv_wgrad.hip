// conv_wgrad.hip -- convolution weight gradient on the gfx950 matrix cores.
//
//   out[t][ca][cb] = sum_{n,py,px} a[n,py,px,ca] * b[n, py*stride + dy[t], px*stride + dx[t], cb]
//
// replaces aten::cudnn_convolution_backward_weight / ..._transpose_backward_weight
// (stylegan2ada/torch_utils/ops/conv2d_gradfix.py:140-147).  `a` is the tensor living on the coarse grid (grad_output
// for a forward conv, the input for a transposed conv), `b` the one on the fine grid.
//
// GEMM view per tap: D[ca][cb] = sum_pix A[ca][pix] * B[pix][cb]; the reduction index is the pixel, which is the SLOW
// axis of both channel-minor operands, so both MFMA fragments are read from pixel-major LDS tiles with the hardware
// transposing read ds_read_b64_tr_b16.  The k order inside a 32-pixel chunk is a free permutation (both operands use the
// same one): 16-lane group g takes pixels {4g..4g+3} and {16+4g..16+4g+3}, which with a row stride of (channels*2 + 32)
// bytes keeps each 32-lane half on 8 distinct 32-B bank slots (conflict-free).
//
// Workgroup = 256 lanes (2 x 2 waves), tile BCA x BCB channels for ALL taps of the launch (<= NT accumulator sets in
// registers), walking its share of the pixel axis in 32-pixel chunks: the a-tile is staged once per chunk and re-used by
// every tap, only the gathered b-tiles change.  The pixel axis is split over gridDim.z workgroups that write fp32
// partial slabs; a second kernel sums the slabs in a fixed order (bitwise reproducible, no float atomics).
#include "conv_common.h"
#include "lds_asm.h"

namespace {

using sbgconv::bf16_mfma; using sbgconv::f16_mfma; using sbgconv::Mfma;

struct WgradArgs {
    const unsigned short* a; const unsigned short* b; float* out; float* ws;
    int N, PH, PW, Ca, BH, BW, Cb;
    int64_t as_n, as_h, as_w, bs_n, bs_h, bs_w;
    int stride, ntaps;
    int tap_dy[SBG_MAX_TAPS], tap_dx[SBG_MAX_TAPS];
    int accumulate;
    int64_t P;              // N * PH * PW pixels on the coarse grid
    int nchunks;            // ceil(P / 32)
    int nsplit, chunks_per_split;
    int atiles, btiles;
    int tap0;               // first tap handled by this launch (out slab offset)
    int ntaps_total;
};

// Workgroup -> (a tile, b tile, pixel split).  Workgroups are dealt round-robin to the eight XCDs, each with its own L2: all channel
// tiles of one pixel split are therefore placed on ONE XCD, back to back, so the split's a / b pixels come from HBM once and the
// other tiles hit that L2 (with a plain (x, y, z) grid the tiles of a split land on all eight L2s and the 256-channel layers
// measured 3x their algorithmic HBM bytes: profiles/r01j_traffic.json, FETCH_SIZE).  Returns false for the padding workgroups.
static __device__ __forceinline__ bool wgrad_decode_block(const WgradArgs& p, int& ta, int& tb, int& split)
{
    const int T = p.atiles * p.btiles;
    const int L = blockIdx.x, xcd = L & 7, j = L >> 3;
    const int tile = j % T;
    split = (j / T) * 8 + xcd;
    ta = tile % p.atiles; tb = tile / p.atiles;
    return split < p.nsplit;
}

typedef __attribute__((address_space(3))) short4_t* lds_s4_ptr;

// transposing LDS read: lane (16-lane group, 4q+p) passes the address of row q, columns 4p..4p+3; lane i gets column i of
// the 4 rows.
static __device__ __forceinline__ short4_t lds_tr_read(const unsigned char* p)
{
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_ptr)(p));
}

template <class MF, int BCA, int BCB, int NT>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgradArgs p)
{
    constexpr int WA = BCA / 2, WB = BCB / 2;          // wave tile (2 x 2 waves)
    constexpr int TA = WA / 16, TB = WB / 16;
    constexpr int RSA = BCA * 2 + 32, RSB = BCB * 2 + 32;   // LDS row strides (bytes), padded by 32 B
    constexpr int A_BYTES = 32 * RSA, B_BYTES = 32 * RSB;
    constexpr int CHA = BCA / 8, CHB = BCB / 8;        // 16-B chunks per pixel row
    constexpr int LA = (32 * CHA) / 256, LB = (32 * CHB) / 256;   // staging loads per lane per tile
    static_assert(LA >= 1 && LB >= 1, "tile too small");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sA = smem;
    unsigned char* sB = smem + A_BYTES;                 // NT tiles

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int ta_, tb_, split;
    if (!wgrad_decode_block(p, ta_, tb_, split)) return;       // (uniform per workgroup, before any barrier)
    const int ca0 = ta_ * BCA, cb0 = tb_ * BCB;
    const int chunk_begin = split * p.chunks_per_split;
    int chunk_end = chunk_begin + p.chunks_per_split;
    if (chunk_end > p.nchunks) chunk_end = p.nchunks;

    const int wa = (wave >> 1) * WA, wb = (wave & 1) * WB;
    const int fi = lane & 15, fg = lane >> 4, fq = fi >> 2, fp = fi & 3;

    float4_t acc[NT][TA][TB];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int i = 0; i < TA; i++)
#pragma unroll
            for (int j = 0; j < TB; j++) acc[t][i][j] = float4_t{0.f, 0.f, 0.f, 0.f};

    short8_t ra[LA], rb[NT][LB];
    auto issue_loads = [&](int chunk) {
        const int64_t pix0 = (int64_t)chunk * 32;
#pragma unroll
        for (int l = 0; l < LA; l++) {
            const int idx = tid + 256 * l, row = idx / CHA, ch = idx % CHA;
            const int64_t pix = pix0 + row;
            const int c = ca0 + ch * 8;
            short8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (pix < p.P && c < p.Ca) {
                const int px = (int)(pix % p.PW); const int64_t r = pix / p.PW; const int py = (int)(r % p.PH); const int n = (int)(r / p.PH);
                v = *reinterpret_cast<const short8_t*>(p.a + n * p.as_n + py * p.as_h + px * p.as_w + c);
            }
            ra[l] = v;
        }
#pragma unroll
        for (int l = 0; l < LB; l++) {
            const int idx = tid + 256 * l, row = idx / CHB, ch = idx % CHB;
            const int64_t pix = pix0 + row;
            const int c = cb0 + ch * 8;
            const bool ok = pix < p.P && c < p.Cb;
            int px = 0, py = 0, n = 0;
            if (ok) { px = (int)(pix % p.PW); const int64_t r = pix / p.PW; py = (int)(r % p.PH); n = (int)(r / p.PH); }
            const unsigned short* base = p.b + n * p.bs_n + c;
#pragma unroll
            for (int t = 0; t < NT; t++) {
                short8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
                if (t < p.ntaps && ok) {
                    const int by = py * p.stride + p.tap_dy[t], bx = px * p.stride + p.tap_dx[t];
                    if ((unsigned)by < (unsigned)p.BH && (unsigned)bx < (unsigned)p.BW)
                        v = *reinterpret_cast<const short8_t*>(base + (int64_t)by * p.bs_h + (int64_t)bx * p.bs_w);
                }
                rb[t][l] = v;
            }
        }
    };
    auto write_tiles = [&]() {
#pragma unroll
        for (int l = 0; l < LA; l++) {
            const int idx = tid + 256 * l, row = idx / CHA, ch = idx % CHA;
            *reinterpret_cast<short8_t*>(sA + row * RSA + ch * 16) = ra[l];
        }
#pragma unroll
        for (int l = 0; l < LB; l++) {
            const int idx = tid + 256 * l, row = idx / CHB, ch = idx % CHB;
#pragma unroll
            for (int t = 0; t < NT; t++)
                if (t < p.ntaps) *reinterpret_cast<short8_t*>(sB + t * B_BYTES + row * RSB + ch * 16) = rb[t][l];
        }
    };
    // fragment for 16 channels starting at column `col` of a pixel-major tile: k = {4g+q} and {16+4g+q}
    auto read_frag = [&](const unsigned char* tile, int rs, int col) -> short8_t {
        const unsigned char* r0 = tile + (4 * fg + fq) * rs + (col + 4 * fp) * 2;
        short4_t lo = lds_tr_read(r0), hi = lds_tr_read(r0 + 16 * rs);
        return short8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    };

    if (chunk_begin < chunk_end) {
        issue_loads(chunk_begin);
        for (int c = chunk_begin; c < chunk_end; c++) {
            write_tiles();
            __syncthreads();
            if (c + 1 < chunk_end) issue_loads(c + 1);
            short8_t fa[TA];
#pragma unroll
            for (int i = 0; i < TA; i++) fa[i] = read_frag(sA, RSA, wa + 16 * i);
#pragma unroll
            for (int t = 0; t < NT; t++) {
                if (t < p.ntaps) {
                    short8_t fb[TB];
#pragma unroll
                    for (int j = 0; j < TB; j++) fb[j] = read_frag(sB + t * B_BYTES, RSB, wb + 16 * j);
#pragma unroll
                    for (int i = 0; i < TA; i++)
#pragma unroll
                        for (int j = 0; j < TB; j++) acc[t][i][j] = Mfma<MF>::run(fa[i], fb[j], acc[t][i][j]);
                }
            }
            __syncthreads();
        }
    }

    // ---- store: lane holds rows ca = .. + 4*fg + e, column cb = .. + fi ------------------------------------------------
    const bool direct = (p.nsplit == 1);
    float* dst_base = direct ? p.out : p.ws + (int64_t)split * p.ntaps_total * p.Ca * p.Cb;
#pragma unroll
    for (int t = 0; t < NT; t++) {
        if (t >= p.ntaps) continue;
        float* slab = dst_base + (int64_t)(p.tap0 + t) * p.Ca * p.Cb;
#pragma unroll
        for (int i = 0; i < TA; i++)
#pragma unroll
            for (int j = 0; j < TB; j++) {
                const int cb = cb0 + wb + 16 * j + fi;
                if (cb >= p.Cb) continue;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int ca = ca0 + wa + 16 * i + 4 * fg + e;
                    if (ca >= p.Ca) continue;
                    float* d = slab + (int64_t)ca * p.Cb + cb;
                    const float v = acc[t][i][j][e];
                    *d = (direct && p.accumulate) ? *d + v : v;
                }
            }
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// Row-chunk LDS-DMA kernel: stride 1, |tap offset| <= 1, PW % 32 == 0 (every 3x3 / 1x1 pad-same layer from 32x32 up).
// A K-chunk is 32 consecutive pixels of ONE image row; the b operand of all nine taps is the 3-row x 34-pixel halo of that
// chunk, staged ONCE (15 KB instead of nine gathered 4 KB tiles) next to the 4 KB a-tile.  Stages are filled by
// `buffer_load_dwordx4 ... lds` (out-of-image pixels -> out-of-range offset -> zeros), three stages deep with two chunks of
// loads in flight behind a counted s_waitcnt vmcnt and one raw s_barrier per chunk (the register-staged kernel above keeps
// one chunk in flight and spends most of its wave cycles in s_waitcnt).
// LDS rows are 128 B (64 channels) and cannot be padded under LDS-DMA, so the 16-B chunk pairs of row R are XOR-swizzled by
// (R >> 1) & 3 on the source side and in the transposing reads: any 8 consecutive rows then cover 8 distinct 32-B bank slots.

using sbgconv::lds_void_ptr;      // (and SBG_OOB_OFFSET: conv_common.h)

template <class MF, int S, int BCA, int NSTAGE>
__global__ __launch_bounds__(512) void conv_wgrad_rows_kernel(WgradArgs p, unsigned a_bytes, unsigned b_bytes)
{
    // 8 waves = 2 (ca) x 4 (cb), wave tile (BCA / 2) x 16 channels for all nine taps: two waves per SIMD overlap one wave's
    // barrier / transposing LDS reads with the other's MFMAs.  BCA = 128 (144 accumulator registers) halves the bytes staged per
    // MFMA against BCA = 64 -- the L2 -> LDS stream, not the matrix pipe, bounds this kernel, most of all at stride 2 where the
    // b patch of a 32-pixel chunk is 65 columns wide.
    // S = stride between the coarse (a) and fine (b) grids: b pixel = S * a pixel + tap, taps = (dy0 + i, dx0 + j), i, j in 0..2
    static_assert(BCA == 64 || BCA == 128, "a tile of 64 or 128 channels");
    static_assert(NSTAGE >= 2 && NSTAGE <= 6, "2..6 stages (the wait ladder covers five chunks in flight)");
    constexpr int BCB = 64, NT = 9, DEPTH = NSTAGE - 1;     // NSTAGE = 2 (one chunk of loads in flight) lets two workgroups share a CU where three stages would not fit twice
    constexpr int TA = BCA / 32;                               // 16-channel a fragments per wave
    constexpr int APIECES = BCA / 16;                          // a-tile = BCA / 64 sub-tiles of [32 pixels][64 channels], 4 pieces each
    constexpr int PCOLS = S * 31 + 3;                          // b columns needed by a 32-pixel chunk
    constexpr int PPR = (PCOLS + 7) / 8;                       // 8-pixel DMA pieces per patch row
    constexpr int PROW = PPR * 8;                              // patch row pitch in pixels
    constexpr int NWAVE = 8;
    constexpr int NPIECE = ((APIECES + 3 * PPR + NWAVE - 1) / NWAVE) * NWAVE;   // a-tile + patch pieces, padded with spares
    constexpr int PIECES = NPIECE / NWAVE;                     // DMA instructions per wave per stage
    constexpr int NREAL = APIECES + 3 * PPR;                   // pieces that carry data; the spares (equal DMA counts on every wave) all land in one dump KiB behind the stages
    constexpr int A_BYTES = APIECES * 1024, STAGE = NREAL * 1024, DUMP = NSTAGE * STAGE;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int ta_, tb_, split;
    if (!wgrad_decode_block(p, ta_, tb_, split)) return;       // (uniform per workgroup, before any barrier)
    const int ca0 = ta_ * BCA, cb0 = tb_ * BCB;
    const int chunk_begin = split * p.chunks_per_split;
    int chunk_end = chunk_begin + p.chunks_per_split;
    if (chunk_end > p.nchunks) chunk_end = p.nchunks;
    const int nloc = chunk_end - chunk_begin;
    const int xblocks = p.PW >> 5;
    const int dy0 = p.tap_dy[0], dx0 = p.tap_dx[0];

    __amdgpu_buffer_rsrc_t ar = __builtin_amdgcn_make_buffer_rsrc((void*)p.a, 0, (int)a_bytes, 0x00020000);
    __amdgpu_buffer_rsrc_t br = __builtin_amdgcn_make_buffer_rsrc((void*)p.b, 0, (int)b_bytes, 0x00020000);

    // ---- DMA lane coordinates: piece = 8 rows x 8 chunks of 16 B; lane -> (row = lane / 8, LDS chunk = lane % 8)
    const int drow = lane >> 3, dchunk = lane & 7;
    auto src_chunk = [&](int R) { return (((dchunk >> 1) ^ ((R >> 1) & 3)) << 1) | (dchunk & 1); };   // swizzled source chunk for LDS row R

    // coordinates of chunk `loc` (wave-uniform), then its DMA pieces i = 0 .. PIECES - 1 of this wave
    struct ChunkC { int py, n, px0; unsigned char* st; };
    auto chunk_coords = [&](int loc) -> ChunkC {
        const int c = chunk_begin + loc;
        const int xb = c % xblocks, rowid = c / xblocks;
        ChunkC r; r.py = rowid % p.PH; r.n = rowid / p.PH; r.px0 = xb << 5; r.st = smem + (loc % NSTAGE) * STAGE;
        return r;
    };
    auto issue_piece = [&](const ChunkC& cc, int i) {
        const int py = cc.py, n = cc.n, px0 = cc.px0;
        unsigned char* st = cc.st;
        {
            const int piece = wave + NWAVE * i;                // wave-uniform
            if (piece < APIECES) {                             // a sub-tile piece >> 2, pixel rows 8 * (piece & 3) ..
                const int R = (piece & 3) * 8 + drow;
                const int ch = ca0 + (piece >> 2) * 64 + src_chunk(R) * 8;
                const unsigned okm = 0u - (unsigned)(ch < p.Ca);
                const unsigned real = (unsigned)(n * (int)p.as_n + py * (int)p.as_h + (px0 + R) * (int)p.as_w + ch) * 2u;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(ar, (lds_void_ptr)(st + piece * 1024), 16, (real & okm) | (SBG_OOB_OFFSET & ~okm), 0, 0, 0);
            } else {
                const int q = piece - APIECES;                 // patch piece; q >= 3 * PPR are spares (zeros)
                const int r = q / PPR, jb = q - r * PPR;
                const int R = r * PROW + jb * 8 + drow;        // LDS row inside the patch
                // stride 2: the patch row is stored de-interleaved -- its 33 even columns in LDS rows 0..39, the 32 odd ones in rows 40..71 -- so
                // that the 32 pixels a tap reads (columns dx + 2 p) are CONSECUTIVE LDS rows, like at stride 1.  Interleaved, the eight rows of a
                // transposing read all had one parity, i.e. one 32-bank half: two-way conflicts on every b read (SQ_LDS_BANK_CONFLICT 41 % of
                // the LDS cycles, profiles/r02d_sq_counters.json).
                constexpr int NEVEN = (PCOLS + 1) / 2, EVROWS = ((NEVEN + 7) / 8) * 8;
                const int pcol = (S == 1) ? jb * 8 + drow : (jb * 8 < EVROWS ? 2 * (jb * 8 + drow) : 2 * (jb * 8 - EVROWS + drow) + 1);
                const int by = S * py + dy0 + r, bx = S * px0 + dx0 + pcol;
                const int ch = cb0 + src_chunk(R) * 8;
                const unsigned okm = 0u - (unsigned)((q < 3 * PPR) & (pcol < PCOLS) & ((unsigned)by < (unsigned)p.BH) & ((unsigned)bx < (unsigned)p.BW) & (ch < p.Cb));
                const unsigned real = (unsigned)(n * (int)p.bs_n + by * (int)p.bs_h + bx * (int)p.bs_w + ch) * 2u;
                unsigned char* dst = (q < 3 * PPR) ? st + A_BYTES + q * 1024 : smem + DUMP;      // (wave-uniform)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(br, (lds_void_ptr)dst, 16, (real & okm) | (SBG_OOB_OFFSET & ~okm), 0, 0, 0);
            }
        }
    };
    auto issue = [&](int loc) {
        const ChunkC cc = chunk_coords(loc);
#pragma unroll
        for (int i = 0; i < PIECES; i++) issue_piece(cc, i);
    };
    // `late`: the DMA instructions of chunk s + DEPTH go out spread over the tap loop, each behind a tap's MFMAs, instead of together right
    // behind the barrier (where all eight waves issued them at once and the matrix pipe waited).  Measured (one device,
    // interleaved rounds, 64 images): 128 x 128 @ 256^2 1060 -> 1135 TF, 256 x 256 @ 128^2 1149 -> 1227, 512 x 512 @ 64^2 1204 -> 1285,
    // stride 2: 256 x 128 917 -> 1016, 512 x 256 966 -> 1081.  
    constexpr bool late = true;

    const int wa = (wave >> 2) * (BCA / 2), wb = (wave & 3) * 16;
    const int fi = lane & 15, fg = lane >> 4, fq = fi >> 2, fp = fi & 3;
    const unsigned lds_base = (unsigned)(uintptr_t)((lds_void_ptr)smem);
    float4_t acc[NT][TA];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int i = 0; i < TA; i++) acc[t][i] = float4_t{0.f, 0.f, 0.f, 0.f};

    // Per-lane LDS byte offsets of the transposing reads, computed once.  The tap order is fixed (t = 3 i + j), so inside the
    // chunk loop every read is `per-lane base (one of 3 column-tap variants) + compile-time constant`.
    // The 32 pixels of tap column j are the consecutive patch rows PROW*i + base(j) + p (stride 2: columns de-interleaved, base(j) = 40 (j & 1)
    // + (j >> 1)), so the swizzle term (R >> 1) & 3 depends on j only (PROW and 40 are multiples of 8).
    auto frag_off = [&](int Rrel, int col) {
        const int chunk = (col >> 3) + (fp >> 1);
        const int sw = (((chunk >> 1) ^ ((Rrel >> 1) & 3)) << 1) | (chunk & 1);
        return Rrel * 128 + sw * 16 + (fp & 1) * 8;
    };
    int offA[TA], offB[3];
#pragma unroll
    for (int i = 0; i < TA; i++) {
        const int col = wa + 16 * i;                           // channel offset inside the a tile -> (sub-tile, column)
        offA[i] = (col >> 6) * 4096 + frag_off(4 * fg + fq, col & 63);
    }
#pragma unroll
    for (int d = 0; d < 3; d++) {
        constexpr int EVROWS_ = (((PCOLS + 1) / 2 + 7) / 8) * 8;
        offB[d] = frag_off((S == 1 ? d : (d & 1) * EVROWS_ + (d >> 1)) + 4 * fg + fq, wb);      // stride 2: de-interleaved columns (see issue())
    }
    auto read_frag = [&](const unsigned char* base, int off, int hi_off) -> short8_t {
        short4_t lo = lds_tr_read(base + off), hi = lds_tr_read(base + off + hi_off);
        return short8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    };

#pragma unroll
    for (int s = 0; s < DEPTH; s++) if (s < nloc) issue(s);
    for (int s = 0; s < nloc; s++) {
        {   // chunk s has landed once at most the loads of the (up to DEPTH - 1) chunks issued after it are outstanding
            const int later = nloc - 1 - s;
            if (DEPTH >= 2 && later >= DEPTH - 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"((DEPTH - 1) * PIECES) : "memory");
            else if (DEPTH >= 3 && later == DEPTH - 2) asm volatile("s_waitcnt vmcnt(%0)" :: "n"((DEPTH >= 3 ? DEPTH - 2 : 0) * PIECES) : "memory");
            else if (DEPTH >= 4 && later == DEPTH - 3) asm volatile("s_waitcnt vmcnt(%0)" :: "n"((DEPTH >= 4 ? DEPTH - 3 : 0) * PIECES) : "memory");
            else if (DEPTH >= 5 && later == DEPTH - 4) asm volatile("s_waitcnt vmcnt(%0)" :: "n"((DEPTH >= 5 ? DEPTH - 4 : 0) * PIECES) : "memory");
            else                                       asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        const bool more = s + DEPTH < nloc;
        ChunkC nxt = chunk_coords(more ? s + DEPTH : s);
        if (more && !late) {
#pragma unroll
            for (int i = 0; i < PIECES; i++) issue_piece(nxt, i);
        }
        // The transposing reads are issued as inline assembly with hand-counted lgkmcnt waits.  Written with the builtin, the compiler sees LDS
        // reads behind LDS-DMA writes it cannot tell apart and guards the first read of every chunk with s_waitcnt vmcnt(0) -- the wave then
        // waits for the loads it has just issued for chunk s + DEPTH, and the whole L2 -> LDS stream is exposed (ablation: 806 us, 532 us
        // without the loads, 325 us MFMA only).  The explicit vmcnt(PIECES) + barrier above is the real dependence.
        const unsigned stage = lds_base + (unsigned)((s % NSTAGE) * STAGE);
        short4_t alo[TA], ahi[TA], blo[3], bhi[3];
        sbg_static_for<TA>([&](auto it) {
            constexpr int i = decltype(it)::value;
            lds_tr_issue<0>(alo[i], stage + (unsigned)offA[i]);
            lds_tr_issue<16 * 128>(ahi[i], stage + (unsigned)offA[i]);
        });
        unsigned pb[3];
#pragma unroll
        for (int d = 0; d < 3; d++) pb[d] = stage + (unsigned)offB[d];
        auto issue_b = [&](auto tt) {
            constexpr int t = decltype(tt)::value, dyi = t / 3, dxi = t % 3, OFF = A_BYTES + dyi * PROW * 128;
            lds_tr_issue<OFF>(blo[t % 3], pb[dxi]);
            lds_tr_issue<OFF + 16 * 128>(bhi[t % 3], pb[dxi]);
        };
        issue_b(std::integral_constant<int, 0>{});
        issue_b(std::integral_constant<int, 1>{});
        sbg_static_for<9>([&](auto tt) {
            constexpr int t = decltype(tt)::value;
            if constexpr (t + 2 < 9) issue_b(std::integral_constant<int, t + 2>{});
            lds_wait<(t + 2 < 9 ? 4 : t + 1 < 9 ? 2 : 0)>(blo[t % 3], bhi[t % 3]);      // the reads of taps t + 1 and t + 2 may still be in flight
            // (the a reads precede tap 0's and LDS returns in order: they have landed)
            const short8_t fb = short8_t{blo[t % 3][0], blo[t % 3][1], blo[t % 3][2], blo[t % 3][3], bhi[t % 3][0], bhi[t % 3][1], bhi[t % 3][2], bhi[t % 3][3]};
#pragma unroll
            for (int i = 0; i < TA; i++) {
                const short8_t fa_i = short8_t{alo[i][0], alo[i][1], alo[i][2], alo[i][3], ahi[i][0], ahi[i][1], ahi[i][2], ahi[i][3]};
                acc[t][i] = Mfma<MF>::run(fa_i, fb, acc[t][i]);
            }
            if (more && late) {      // pieces i with i * 9 / PIECES == t: spread evenly over the nine taps
                sbg_static_for<PIECES>([&](auto pt) {
                    constexpr int i = decltype(pt)::value;
                    if constexpr (i * 9 / PIECES == t) issue_piece(nxt, i);
                });
            }
        });
    }

    const bool direct = (p.nsplit == 1);
    float* dst_base = direct ? p.out : p.ws + (int64_t)split * p.ntaps_total * p.Ca * p.Cb;
    const int cb = cb0 + wb + fi;
#pragma unroll
    for (int t = 0; t < NT; t++) {
        if (t >= p.ntaps || cb >= p.Cb) continue;
        float* slab = dst_base + (int64_t)(p.tap0 + t) * p.Ca * p.Cb;
#pragma unroll
        for (int i = 0; i < TA; i++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int ca = ca0 + wa + 16 * i + 4 * fg + e;
                if (ca >= p.Ca) continue;
                float* d = slab + (int64_t)ca * p.Cb + cb;
                const float v = acc[t][i][e];
                *d = (direct && p.accumulate) ? *d + v : v;
            }
    }
}

// out[i] (+)= sum_s ws[s][i], fixed order.  LANES lanes share an output element (slabs s, s + LANES, ...) and finish with a
// shuffle tree, so a small output with many slabs (the fromrgb layer: 1024 elements x 1024 slabs) is not one serial chain per lane.
template <int LANES>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* ws, float* out, int64_t n, int nsplit, int accumulate)
{
    const int sub = threadIdx.x % LANES;
    const int64_t step = (int64_t)gridDim.x * (256 / LANES);
    for (int64_t i = (int64_t)blockIdx.x * (256 / LANES) + threadIdx.x / LANES; i < n; i += step) {
        float s = 0.f;
        int k = sub;
        for (; k + 7 * LANES < nsplit; k += 8 * LANES) {         // eight independent loads in flight; the sum keeps its fixed order
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = ws[(int64_t)(k + u * LANES) * n + i];
#pragma unroll
            for (int u = 0; u < 8; u++) s += v[u];
        }
        for (; k < nsplit; k += LANES) s += ws[(int64_t)k * n + i];
#pragma unroll
        for (int m = LANES >> 1; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
        if (sub == 0) out[i] = accumulate ? out[i] + s : s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Thin weight gradient: Ca, Cb <= 32 (the 16 / 32-channel layers of the 512^2 / 1024^2 blocks, configs/ffhq_sg2.yaml).  The kernels above
// tile 64 x 64 channels; at 16 x 16 fifteen sixteenths of their MFMAs multiply padding (62 TFLOP/s, 870 GB/s on tensors that stream in a
// sixth of the time).  Here every WAVE works alone: a K-step is 32 pixels of one image row, staged per wave in LDS as they lie in memory
// ([pixel][channel]: the a row segment and the RY x PCOLS patch of b behind all taps), and the MFMA operands -- eight pixels of ONE channel
// per lane -- are gathered with 16-bit LDS reads (any stride, any tap window up to 3 rows).  Each wave writes its own fp32 slab; the
// fixed-order slab reduction above finishes (bitwise reproducible).  Measured (ffhq_sg2 shapes): 16 x 16 @1024^2 2468 -> 1995 us, 32 x 16 stride 2
// 1264 -> 1127 us; at 32 x 32 the 64 x 64 rows kernel is faster (684 vs 2147 us: the 16-bit gathers dominate), so Ca * Cb <= 512 only.
template <class MF, int TA, int TB>      // 16-channel fragments of a and b
__global__ __launch_bounds__(256) void conv_wgrad_thin_kernel(WgradArgs p, int dymin, int dxmin, int RY, int PCOLS, int wave_lds)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned short* la = reinterpret_cast<unsigned short*>(smem + wave * wave_lds);     // [32 pixels][Ca]
    unsigned short* lb = la + 32 * p.Ca;                                                  // [RY][PCOLS][Cb]
    const int slab = blockIdx.x * 4 + wave;                                               // one output slab per wave
    const int nwaves = gridDim.x * 4;
    const int xblocks = (p.PW + 31) >> 5;
    const int nchunks = p.N * p.PH * xblocks;
    const int fi = lane & 15, fg = lane >> 4;
    const int ca8 = p.Ca >> 3, cb8 = p.Cb >> 3;
    float4_t acc[9][TA][TB];
#pragma unroll
    for (int t = 0; t < 9; t++)
#pragma unroll
        for (int i = 0; i < TA; i++)
#pragma unroll
            for (int j = 0; j < TB; j++) acc[t][i][j] = float4_t{0.f, 0.f, 0.f, 0.f};
    int tdy[9], tdx[9];
#pragma unroll
    for (int t = 0; t < 9; t++) { tdy[t] = (t < p.ntaps ? p.tap_dy[t] : 0) - dymin; tdx[t] = (t < p.ntaps ? p.tap_dx[t] : 0) - dxmin; }

    for (int c = slab; c < nchunks; c += nwaves) {
        const int xb = c % xblocks, rowid = c / xblocks;
        const int py = rowid % p.PH, n = rowid / p.PH;
        const int px0 = xb << 5;
        // ---- stage a: 32 pixels x Ca channels (pixels beyond the row end = zeros)
        for (int piece = lane; piece < 32 * ca8; piece += 64) {
            const int px = piece / ca8, ch = (piece - px * ca8) * 8;
            short8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (px0 + px < p.PW) v = *reinterpret_cast<const short8_t*>(p.a + (int64_t)n * p.as_n + (int64_t)py * p.as_h + (int64_t)(px0 + px) * p.as_w + ch);
            *reinterpret_cast<short8_t*>(la + piece * 8) = v;
        }
        // ---- stage the b patch: rows S*py + dymin + r, columns S*px0 + dxmin + col
        const int npieces = RY * PCOLS * cb8;
        for (int piece = lane; piece < npieces; piece += 64) {
            const int ch = (piece % cb8) * 8, pc = piece / cb8;
            const int col = pc % PCOLS, r = pc / PCOLS;
            const int by = p.stride * py + dymin + r, bx = p.stride * px0 + dxmin + col;
            short8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
            if ((unsigned)by < (unsigned)p.BH && (unsigned)bx < (unsigned)p.BW)
                v = *reinterpret_cast<const short8_t*>(p.b + (int64_t)n * p.bs_n + (int64_t)by * p.bs_h + (int64_t)bx * p.bs_w + ch);
            *reinterpret_cast<short8_t*>(lb + piece * 8) = v;
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);              // this wave's LDS writes are visible to its own reads
        __builtin_amdgcn_wave_barrier();
        // ---- operands: lane (channel fi of fragment, k-group fg) holds pixels 8 fg + j
        short8_t fa[TA];
#pragma unroll
        for (int i = 0; i < TA; i++)
#pragma unroll
            for (int j = 0; j < 8; j++) fa[i][j] = (short)la[(8 * fg + j) * p.Ca + 16 * i + fi];
#pragma unroll
        for (int t = 0; t < 9; t++) {
            if (t < p.ntaps) {                           // (a predicate, not a break: the tap loop must unroll so that acc[] stays in registers)
                const unsigned short* row = lb + (tdy[t] * PCOLS + tdx[t]) * p.Cb;
#pragma unroll
                for (int jb = 0; jb < TB; jb++) {
                    short8_t fb;
#pragma unroll
                    for (int j = 0; j < 8; j++) fb[j] = (short)row[(p.stride * (8 * fg + j)) * p.Cb + 16 * jb + fi];
#pragma unroll
                    for (int i = 0; i < TA; i++) acc[t][i][jb] = Mfma<MF>::run(fa[i], fb, acc[t][i][jb]);
                }
            }
        }
        __builtin_amdgcn_wave_barrier();                 // the next chunk overwrites the buffers this wave has just read
    }
    // ---- this wave's slab: out[t][ca][cb], lane holds rows (ca) 16 i + 4 fg + e of column (cb) 16 jb + fi
    float* dst = p.ws + (int64_t)slab * p.ntaps_total * p.Ca * p.Cb;
#pragma unroll
    for (int t = 0; t < 9; t++) {
        if (t < p.ntaps) {
#pragma unroll
            for (int i = 0; i < TA; i++)
#pragma unroll
                for (int jb = 0; jb < TB; jb++)
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const int ca = 16 * i + 4 * fg + e, cb = 16 * jb + fi;
                        if (ca < p.Ca && cb < p.Cb) dst[((int64_t)(p.tap0 + t) * p.Ca + ca) * p.Cb + cb] = acc[t][i][jb][e];
                    }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side.  wgrad_plan decides everything about a call, once, from the validated parameter block alone (no HIP calls): the kernel
// that serves it, its tiles and pixel splits, launch geometry, launch-record code and the profiler's figures.  Both entry points read it.

enum WgradFamily { WG_EMPTY, WG_THIN, WG_ROWS, WG_BIG, WG_TAPS };      // no pixels | thin | rows | conv_wgrad_kernel 128 x 128, one tap | 64 x 64, groups of nine taps

struct WgradPlan {
    WgradFamily family;
    int bca, bcb;                                       // channels per workgroup tile (thin: 16-channel fragments per wave)
    int atiles, btiles, nchunks, nsplit, chunks_per_split;
    int64_t grid; int block, lds;
    int code;                                           // dims[6] of the launch record
    unsigned a_bytes, b_bytes;                          // rows kernel: byte extents of the operands
    int dymin, dxmin, RY, PCOLS, wave_lds;              // thin kernel: tap window origin, patch rows x columns, LDS bytes per wave (grid = workgroups of four waves)
    double flops_per_tap, bytes_ab, bytes_out_per_tap;  // profiler: a launch over t taps does flops_per_tap * t and moves bytes_ab + bytes_out_per_tap * t
};

static bool thin_plan(const sbg_wgrad_params& q, WgradPlan& pl)
{
    if (q.Ca > 32 || q.Cb > 32 || q.Ca * q.Cb > 512 || q.ntaps > 9 || q.stride > 2) return false;
    int dy0 = q.tap_dy[0], dy1 = dy0, dx0 = q.tap_dx[0], dx1 = dx0;
    for (int i = 1; i < q.ntaps; i++) {
        if (q.tap_dy[i] < dy0) dy0 = q.tap_dy[i]; if (q.tap_dy[i] > dy1) dy1 = q.tap_dy[i];
        if (q.tap_dx[i] < dx0) dx0 = q.tap_dx[i]; if (q.tap_dx[i] > dx1) dx1 = q.tap_dx[i];
    }
    const int64_t nchunks = (int64_t)q.N * q.PH * ((q.PW + 31) / 32);
    if (dy1 - dy0 > 2 || dx1 - dx0 > 2 || nchunks >= INT32_MAX) return false;
    pl.dymin = dy0; pl.dxmin = dx0; pl.RY = dy1 - dy0 + 1; pl.PCOLS = q.stride * 31 + (dx1 - dx0) + 1;
    pl.wave_lds = ((32 * q.Ca + pl.RY * pl.PCOLS * q.Cb) * 2 + 15) & ~15;
    pl.grid = (nchunks + 15) / 16;                       // at least four chunks per wave
    if (pl.grid > 2048) pl.grid = 2048;
    return true;
}

static bool rows_kernel_ok(const sbg_wgrad_params& q, WgradPlan& pl)
{
    if (q.stride > 2 || (q.PW % 32) != 0 || q.ntaps != 9) return false;
    for (int t = 0; t < 9; t++)          // the kernel hard-codes a row-major 3x3 tap window starting at (dy[0], dx[0])
        if (q.tap_dy[t] != q.tap_dy[0] + t / 3 || q.tap_dx[t] != q.tap_dx[0] + t % 3) return false;
    if (q.as_n < 0 || q.as_h < 0 || q.as_w < 0 || q.bs_n < 0 || q.bs_h < 0 || q.bs_w < 0) return false;
    auto extent = [&](int h, int w, int c, int64_t s_n, int64_t s_h, int64_t s_w) { return 2 * ((int64_t)(q.N - 1) * s_n + (int64_t)(h - 1) * s_h + (int64_t)(w - 1) * s_w + c); };
    const int64_t ab = extent(q.PH, q.PW, q.Ca, q.as_n, q.as_h, q.as_w), bb = extent(q.BH, q.BW, q.Cb, q.bs_n, q.bs_h, q.bs_w);
    pl.a_bytes = (unsigned)ab; pl.b_bytes = (unsigned)bb;
    return ab < (int64_t)SBG_OOB_OFFSET && bb < (int64_t)SBG_OOB_OFFSET;
}

// Stages of the rows kernel (LDS: stages x (a + patch pieces) + 1 KiB).  Measured flat from 2 to 6 stages at one workgroup per CU (the L2 -> LDS
// stream is not latency bound); what matters is that two workgroups still fit where registers allow two.
static constexpr int rows_nstage(int stride, int bca)
{
    if (bca == 128) return 4;                 // 4 x 23 + 1 = 93 KB (stride 1) / 4 x 35 + 1 = 141 KB (stride 2): one workgroup per CU (195 VGPRs)
    return stride == 1 ? 4 : 2;               // 4 x 19 + 1 = 77 KB / 2 x 31 + 1 = 63 KB: two per CU
}

static void plan_split(WgradPlan& pl, const sbg_wgrad_params& q, int bca, int bcb, int target)     // target = workgroups aimed for (tiles x pixel splits)
{
    pl.bca = bca; pl.bcb = bcb;
    pl.atiles = (q.Ca + bca - 1) / bca;
    pl.btiles = (q.Cb + bcb - 1) / bcb;
    const int tiles = pl.atiles * pl.btiles;
    int want = (target + tiles - 1) / tiles;             // ~target workgroups in total
    int maxsplit = pl.nchunks / 8; if (maxsplit < 1) maxsplit = 1;   // at least 8 chunks of work per workgroup
    if (want > maxsplit) want = maxsplit;
    if (want < 1) want = 1;
    pl.chunks_per_split = (pl.nchunks + want - 1) / want;
    pl.nsplit = (pl.nchunks + pl.chunks_per_split - 1) / pl.chunks_per_split;
    pl.grid = 8 * (int64_t)tiles * ((pl.nsplit + 7) / 8);          // the splits padded to the eight XCDs (wgrad_decode_block)
}

static WgradPlan wgrad_plan(const sbg_wgrad_params& q)
{
    WgradPlan pl = {};
    const int64_t P = (int64_t)q.N * q.PH * q.PW;
    pl.family = WG_EMPTY; pl.nsplit = 1;
    if (P == 0) return pl;                               // an empty batch: decided before anything divides
    pl.nchunks = (int)((P + 31) / 32);
    pl.block = 256;
    if (thin_plan(q, pl)) {
        pl.family = WG_THIN;
        pl.bca = (q.Ca + 15) / 16; pl.bcb = (q.Cb + 15) / 16;
        pl.atiles = pl.btiles = 1; pl.nsplit = 4 * (int)pl.grid; pl.chunks_per_split = 0;      // one slab per wave
        pl.lds = 4 * pl.wave_lds;
        pl.code = 3000000 + pl.bca * 10 + pl.bcb;
    } else if (rows_kernel_ok(q, pl)) {
        pl.family = WG_ROWS;
        // a tile of 128 wherever there are 128 a channels: half the staged bytes and 0.72 instead of 1.22 fragment reads per MFMA.  (While the compiler still
        // guarded the fragment reads with vmcnt(0), the wide tile lost 7-10 % at stride 1 up to 512 channels: one workgroup per CU, nothing overlapped.)
        plan_split(pl, q, q.Ca >= 128 ? 128 : 64, 64, 512);      // one resident workgroup per CU: two waves of workgroups, half the slab traffic
        // stage = a pieces + 3 x patch pieces, 1 KiB each; one more KiB behind the stages takes the spare pieces
        const int stage_kib = pl.bca / 16 + 3 * ((q.stride * 31 + 3 + 7) / 8);
        pl.block = 512;
        pl.lds = (rows_nstage(q.stride, pl.bca) * stage_kib + 1) * 1024;
        pl.code = 1000000 + pl.bca * 1000 + 64;          // 1xxxxxx = rows kernel (profiles/summarize.py joins the launch log with the kernel trace on this)
    } else {
        pl.family = q.ntaps == 1 ? WG_BIG : WG_TAPS;
        const int tile = pl.family == WG_BIG ? 128 : 64, nt = pl.family == WG_BIG ? 1 : 9;
        plan_split(pl, q, tile, tile, 1024);
        pl.lds = (1 + nt) * 32 * (tile * 2 + 32);        // one a tile and nt b tiles of 32 pixels, rows padded by 32 B
        pl.code = tile * 1000 + tile;
    }
    pl.flops_per_tap = 2.0 * (double)P * q.Ca * (double)q.Cb;
    pl.bytes_ab = 2.0 * (double)P * q.Ca + 2.0 * (double)q.N * q.BH * q.BW * q.Cb;
    pl.bytes_out_per_tap = 4.0 * (double)q.Ca * q.Cb * (pl.nsplit > 1 ? pl.nsplit : 1);
    return pl;
}

static int fill_args(const sbg_wgrad_params* q, WgradPlan& pl, WgradArgs& a)
{
    SBG_CHECK(q && q->a && q->b && q->out, "conv2d_wgrad: null pointer");
    SBG_CHECK(q->dtype == SBG_BF16 || q->dtype == SBG_F16, "conv2d_wgrad: a/b must be bf16 or f16 (fp32 inputs are split by the host)");
    SBG_CHECK(q->N >= 0 && q->PH >= 1 && q->PW >= 1 && q->BH >= 1 && q->BW >= 1, "conv2d_wgrad: bad sizes");
    SBG_CHECK(q->Ca >= 8 && q->Cb >= 8 && (q->Ca % 8) == 0 && (q->Cb % 8) == 0, "conv2d_wgrad: channel counts must be multiples of 8 (pad on the host)");
    SBG_CHECK(q->ntaps >= 1 && q->ntaps <= SBG_MAX_TAPS, "conv2d_wgrad: 1..%d taps", SBG_MAX_TAPS);
    SBG_CHECK(q->stride >= 1, "conv2d_wgrad: stride must be >= 1");
    SBG_CHECK(sbg_aligned16(q->a) && sbg_aligned16(q->b), "conv2d_wgrad: a and b must be 16-byte aligned");
    SBG_CHECK((q->as_n % 8) == 0 && (q->as_h % 8) == 0 && (q->as_w % 8) == 0 && (q->bs_n % 8) == 0 && (q->bs_h % 8) == 0 && (q->bs_w % 8) == 0,
              "conv2d_wgrad: pixel / row strides must be multiples of 8 elements");
    pl = wgrad_plan(*q);
    a.a = (const unsigned short*)q->a; a.b = (const unsigned short*)q->b; a.out = q->out; a.ws = (float*)q->workspace;
    a.N = q->N; a.PH = q->PH; a.PW = q->PW; a.Ca = q->Ca; a.BH = q->BH; a.BW = q->BW; a.Cb = q->Cb;
    a.as_n = q->as_n; a.as_h = q->as_h; a.as_w = q->as_w; a.bs_n = q->bs_n; a.bs_h = q->bs_h; a.bs_w = q->bs_w;
    a.stride = q->stride; a.ntaps = q->ntaps; a.accumulate = q->accumulate;
    for (int t = 0; t < SBG_MAX_TAPS; t++) { a.tap_dy[t] = q->tap_dy[t]; a.tap_dx[t] = q->tap_dx[t]; }
    a.P = (int64_t)q->N * q->PH * q->PW;
    a.tap0 = 0; a.ntaps_total = q->ntaps;
    a.nchunks = pl.nchunks; a.nsplit = pl.nsplit; a.chunks_per_split = pl.chunks_per_split; a.atiles = pl.atiles; a.btiles = pl.btiles;
    return SBG_OK;
}

// One kernel launch of the plan over the taps of `g`: the whole call, or one of its tap groups.
template <auto Kern, class... Extra>
static int launch(const WgradPlan& pl, const WgradArgs& g, hipStream_t s, const Extra&... extra)
{
    return sbgconv::launch_as<Kern>(SBG_K_CONV_WGRAD, "conv2d_wgrad", pl.grid, 1, pl.block, pl.lds, s,
                                    pl.flops_per_tap * g.ntaps, pl.bytes_ab + pl.bytes_out_per_tap * g.ntaps,
                                    {(int)(g.P > INT32_MAX ? INT32_MAX : g.P), g.Ca, g.Cb, g.ntaps, g.stride, g.nsplit, pl.code}, g, extra...);
}

template <class MF, int TA, int TB>
static int thin(const WgradPlan& pl, const WgradArgs& a, hipStream_t s) { return launch<conv_wgrad_thin_kernel<MF, TA, TB>>(pl, a, s, pl.dymin, pl.dxmin, pl.RY, pl.PCOLS, pl.wave_lds); }
template <class MF, int S, int BCA>
static int rows(const WgradPlan& pl, const WgradArgs& a, hipStream_t s) { return launch<conv_wgrad_rows_kernel<MF, S, BCA, rows_nstage(S, BCA)>>(pl, a, s, pl.a_bytes, pl.b_bytes); }

// out (+)= the slabs of the workspace, summed in slab order, LANES lanes per element
template <int LANES>
static int reduce_slabs(const WgradArgs& a, int64_t n, hipStream_t s)
{
    return sbgconv::launch_as<wgrad_reduce_kernel<LANES>>(SBG_K_WGRAD_REDUCE, "conv2d_wgrad", sbg_stream_grid(n * LANES, 256), 1, 256, 0, s, 0.0,
                                                          4.0 * n * (a.nsplit + 1), {(int)n, a.nsplit}, a.ws, a.out, n, a.nsplit, a.accumulate);
}
static int reduce_slabs(const WgradArgs& a, hipStream_t s)
{
    const int64_t n = (int64_t)a.ntaps_total * a.Ca * a.Cb;
    if (n >= (1 << 18) || a.nsplit < 16) return reduce_slabs<1>(a, n, s);      // plenty of elements: one lane each, coalesced across lanes
    return n >= (1 << 14) ? reduce_slabs<4>(a, n, s) : reduce_slabs<64>(a, n, s);
}

template <class MF>
static int run(const WgradPlan& pl, const WgradArgs& a, hipStream_t s)
{
    int rc = SBG_OK;
    if (pl.family == WG_THIN)
        rc = pl.bca == 1 ? (pl.bcb == 1 ? thin<MF, 1, 1>(pl, a, s) : thin<MF, 1, 2>(pl, a, s)) : (pl.bcb == 1 ? thin<MF, 2, 1>(pl, a, s) : thin<MF, 2, 2>(pl, a, s));
    else if (pl.family == WG_ROWS)
        rc = a.stride == 1 ? (pl.bca == 64 ? rows<MF, 1, 64>(pl, a, s) : rows<MF, 1, 128>(pl, a, s)) : (pl.bca == 64 ? rows<MF, 2, 64>(pl, a, s) : rows<MF, 2, 128>(pl, a, s));
    else if (pl.family == WG_BIG)
        rc = launch<conv_wgrad_kernel<MF, 128, 128, 1>>(pl, a, s);
    else
        for (int t0 = 0; t0 < a.ntaps && rc == SBG_OK; t0 += 9) {      // taps in groups of 9 accumulator sets
            WgradArgs g = a;
            g.tap0 = t0; g.ntaps = (a.ntaps - t0 < 9) ? a.ntaps - t0 : 9;
            for (int t = 0; t < g.ntaps; t++) { g.tap_dy[t] = a.tap_dy[t0 + t]; g.tap_dx[t] = a.tap_dx[t0 + t]; }
            rc = launch<conv_wgrad_kernel<MF, 64, 64, 9>>(pl, g, s);
        }
    return rc != SBG_OK || pl.nsplit == 1 ? rc : reduce_slabs(a, s);
}

} // namespace

extern "C" int64_t sbg_conv2d_wgrad_workspace(const sbg_wgrad_params* q)
{
    WgradPlan pl; WgradArgs a;
    if (fill_args(q, pl, a) != SBG_OK) return -1;
    if (pl.nsplit <= 1) return 0;
    return (int64_t)pl.nsplit * q->ntaps * q->Ca * q->Cb * (int64_t)sizeof(float);
}

extern "C" int sbg_conv2d_wgrad(const sbg_wgrad_params* q, sbg_stream_t stream)
{
    WgradPlan pl; WgradArgs a;
    const int rc = fill_args(q, pl, a);
    if (rc != SBG_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (pl.family == WG_EMPTY) {                         // no pixels: the sum is zero
        if (!a.accumulate && hipMemsetAsync(a.out, 0, (size_t)a.ntaps_total * a.Ca * a.Cb * sizeof(float), s) != hipSuccess)
            return sbg_fail(SBG_ERR_LAUNCH, "conv2d_wgrad: memset failed");
        return SBG_OK;
    }
    SBG_CHECK(pl.nsplit == 1 || a.ws != nullptr, "conv2d_wgrad: workspace required (%d pixel splits)", pl.nsplit);
    return q->dtype == SBG_BF16 ? run<bf16_mfma>(pl, a, s) : run<f16_mfma>(pl, a, s);
}
