// conv_k64.hip -- implicit-GEMM convolution on the gfx950 matrix cores, K-step 64, LDS-DMA staging in full 128-B lines.
//
// Same launch contract as conv_igemm.hip (tap list, see include/sbg_hip.h); this file holds the kernels that carry the
// flops of the StyleGAN2 step.  Design points (measured with rocprofv3 / ablation builds):
//   * The 128 x 128 x 32 kernel of conv_igemm.hip was bound by the L2 -> LDS stream (64-B row pieces = half a cache line
//     per request, 15.6 B per kflop).  Here a K-step is 64 channels deep, so every staged row is one whole 128-B line
//     (8 rows x 128 B per wave instruction) and the tile is 128 output channels x 256 pixels.
//   * conv_halo_ld_kernel (3x3 / stride 1 / output grid == input grid): a workgroup owns a TH x TW patch of one image; per
//     64-channel slice the (TH + 2) x (TW + 2) input halo is staged ONCE and all nine taps read shifted windows of it, so
//     a K-step fetches its 16 KB weight tile plus a ninth of the 43 KB halo: 5 B per kflop.  Persistent (one workgroup
//     per CU walks its tiles, the pipeline runs through tile boundaries) with dedicated loader waves.
//   * conv_k64_kernel (everything else: strided, transposed phases, 1x1): im2col on the fly, every wave stages its share.
//   * Compute waves run as two groups in ping-pong (one wave of each per SIMD): while one group reads its MFMA fragments
//     from LDS the other owns the matrix pipe; per-step control flow is compile-time (unrolled taps) or two-way scalar.
//   * Output channels are permuted inside each 32-channel block so that a lane ends up with 8 CONSECUTIVE channels of a
//     pixel: the epilogue stores 16 B (bf16) per lane, straight-line code specialised on dtype / fused tail.
//
// LDS images are [row][8 slots x 16 B] (128 B per row = 64 channels of one tap), written lane-linearly by
// `buffer_load_dwordx4 ... lds` (lane -> row = lane >> 3, slot = lane & 7).  The k-slot -> slot XOR swizzle
// slot = kslot ^ (row & 7) is applied on the SOURCE address and on the fragment reads: ds_read_b128 of 16 consecutive
// rows is conflict-free at any row alignment (SQ_LDS_BANK_CONFLICT = 0 measured), which the shifted halo windows need.
//
// Host side: sbg_conv_k64_fit holds the tile precedence (halo 8x32 / 16x16, 64x256, 128x128, persistent gather, 256x256, 128x256) and fills the
// planned launch; sbg_conv_k64_launch launches that record; sbg_conv_ksplit_reduce finishes a K-split call.  Whether a launch comes here, and
// whether K is split, is decided by conv_plan in conv_igemm.hip.
#include "conv_device.h"
#include <type_traits>

using namespace sbgconv;

namespace {


// Gather (im2col-on-the-fly) kernel: any tap list and stride; one 128 (or 64) x 256 (or 128) tile per workgroup, 8 waves, three LDS
// stages -- or one 256 x 256 tile with two stages (wave tile 128 x 64; the pipeline of that form is derived at its loop below).
template <class MF, int BC, int BP, int WGC, int WGP, int NSTAGE = 3>
__global__ __launch_bounds__(512, 2) void conv_k64_kernel(ConvArgs p, unsigned x_bytes, unsigned w_bytes)
{
    constexpr int NW = 8;
    static_assert(WGC * WGP == NW, "8 waves per workgroup");
    constexpr int WC = BC / WGC, WP = BP / WGP;        // wave tile
    constexpr int TC = WC / 16,  TP = WP / 16;         // 16 x 16 MFMA tiles per wave
    static_assert(WC % 32 == 0 && WP % 16 == 0 && BC % 64 == 0 && BP % 64 == 0, "tile shape");
    constexpr int IA = BC / 64;                        // weight pieces (8 rows x 128 B) per wave per K-step
    constexpr int IB = BP / 64;                        // gathered pixel pieces per wave per K-step
    constexpr int LEAD = NSTAGE - 1;                   // LDS stages: NSTAGE; the loads of step s + LEAD are issued in step s
    static_assert(NSTAGE == 2 || NSTAGE == 3, "gather pipeline: one or two steps of loads in flight");
    constexpr int A_BYTES = BC * 128, B_BYTES = BP * 128, STAGE = A_BYTES + B_BYTES;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool grpY = wave >= 4;
    const int bid = xcd_tile_order(blockIdx.x, gridDim.x);
    const int c0 = (bid % p.ctiles) * BC, p0 = (bid / p.ctiles) * BP;     // one tile per workgroup

    __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)x_bytes, 0x00020000);
    __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (int)w_bytes, 0x00020000);

    const int lrow = dma_lrow(lane);
    const int src_k = dma_src_k(lane, lrow);      // DMA lane coordinates
    unsigned a_base[IA];                                // byte offset of (channel row, src_k) in a weight slab, or out of range
#pragma unroll
    for (int i = 0; i < IA; i++) {
        const int co = c0 + chmap((wave * IA + i) * 8 + lrow);
        a_base[i] = (co < p.Cout) ? (unsigned)(co * (int)p.ws_co + src_k) * 2u : SBG_OOB_OFFSET;
    }
    const int kchunks = (p.Cin + 63) >> 6;
    const int nsteps_all = p.ntaps * kchunks;
    int nsteps = nsteps_all;
    // per-tap constants live in lane t of a VGPR and are fetched with v_readlane (no scalar-memory latency inside the K loop)
    const int tl = lane < p.ntaps ? lane : 0;
    const int tbl_dy = p.tap_dy[tl], tbl_dx = p.tap_dx[tl];
    const int tbl_wtap = p.tap_slab[tl] * (int)p.ws_slab * 2;

    // weights of (tap t, slice chunk) -> stage `stage`
    auto issue_w = [&](int t, int chunk, int stage) {
        unsigned char* st = smem + stage * STAGE;
        // the step's (tap, slab) offset is a scalar and rides in the instruction's scalar offset: a piece is the DMA alone.  Only the last slab of a
        // ragged Cin masks lanes (a masked-off lane reads out of range -> zeros; skipping it would leave stale bytes in LDS)
        const int wtap = __builtin_amdgcn_readlane(tbl_wtap, t) + chunk * 128;
        const bool ragged = chunk * 64 + 64 > p.Cin;          // (wave-uniform)
#pragma unroll
        for (int i = 0; i < IA; i++) {
            unsigned off = a_base[i];
            if (ragged) off = (chunk * 64 + src_k < p.Cin) ? off : SBG_OOB_OFFSET;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (lds_void_ptr)(st + (wave * IA + i) * 1024), 16, off, wtap, 0, 0);
        }
    };

    // ---- MFMA coordinates -------------------------------------------------------------------------------------------
    const int wci = wave / WGP, wpi = wave % WGP;
    const int wc = wci * WC, wp = wpi * WP;
    const int fr = lane & 15, fg = lane >> 4;
    const int foff = frag_off(fr, fg);
    float4_t acc[TC][TP];
#pragma unroll
    for (int i = 0; i < TC; i++)
#pragma unroll
        for (int j = 0; j < TP; j++) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};
    short8_t fa[2][TC], fb[2][TP];

    auto read_a = [&](int stage) {
        const unsigned char* sa = smem + stage * STAGE + wc * 128;
#pragma unroll
        for (int ks = 0; ks < 2; ks++)
#pragma unroll
            for (int i = 0; i < TC; i++) fa[ks][i] = *reinterpret_cast<const short8_t*>(sa + i * 16 * 128 + (foff ^ (ks * 64)));
    };
    auto mma = [&]() {
#pragma unroll
        for (int ks = 0; ks < 2; ks++)
#pragma unroll
            for (int i = 0; i < TC; i++)
#pragma unroll
                for (int j = 0; j < TP; j++) acc[i][j] = Mfma<MF>::run(fa[ks][i], fb[ks][j], acc[i][j]);
    };

    // Ping-pong schedule: waves 0-3 (X) and 4-7 (Y) -- one of each per SIMD -- run half a K-step apart, separated by two
    // barriers per step: while one group issues its LDS reads and DMAs the other owns the matrix pipe.  Global barrier index:
    // X: B_a(s) = 2s, B_b(s) = 2s + 1;  Y: one extra barrier first, B_a(s) = 2s + 1, B_b(s) = 2s + 2.  With three stages (two steps of
    // loads in flight; the two-stage form is derived at its loop):
    //   RAW: every wave's counted vmcnt wait for step s precedes a barrier with index <= 2s (X: before B_a(s); Y: before
    //        B_b(s - 1)), and a stage is read only behind B_a(s).
    //   WAR: reads of step s are retired (lgkmcnt(0)) before B_b(s) <= 2s + 2; stage s % NSTAGE is refilled by the loads of
    //        step s + NSTAGE, issued behind B_a(s + 1) >= 2s + 2.
    // Everything that decides a vmcnt count is a compile-time constant (unrolled taps) or a two-way scalar branch.

    {
        int b_iy0[IB], b_ix0[IB]; unsigned b_base[IB];
#pragma unroll
        for (int i = 0; i < IB; i++) {
            const int pix = p0 + (wave * IB + i) * 8 + lrow;
            const bool ok = pix < p.P;
            const int pp = ok ? pix : 0;
            const int ox = pp % p.OW, t = pp / p.OW, oy = t % p.OH, n = t / p.OH;
            b_iy0[i] = ok ? oy * p.stride : -(1 << 28);            // invalid rows fail every range test below
            b_ix0[i] = ox * p.stride;
            b_base[i] = (unsigned)(n * (int)p.xs_n + src_k) * 2u;
        }
        // Steps are tap-major, so the gathered pixel of a lane (and whether it lies in the image) changes only once per kchunks steps: its byte offset
        // is worked out when the tap changes (x_off[], ~12 vector instructions per piece) and the slab within the tap rides in the instruction's scalar
        // offset.  These waves issue the MFMAs too; at Cin = 512 seven of eight steps now issue their four pixel pieces with no arithmetic at all.
        unsigned x_off[IB]; int x_tap = -1;
        auto issue_x = [&](int t, int chunk, int stage) {          // gathered pixels of (tap t, slice chunk) -> stage
            unsigned char* st = smem + stage * STAGE + A_BYTES;
            if (t != x_tap) {                                      // (wave-uniform)
                x_tap = t;
                const int dy = __builtin_amdgcn_readlane(tbl_dy, t), dx = __builtin_amdgcn_readlane(tbl_dx, t);
#pragma unroll
                for (int i = 0; i < IB; i++) {
                    const int iy = b_iy0[i] + dy, ix = b_ix0[i] + dx;
                    const bool ok = ((unsigned)iy < (unsigned)p.IH) & ((unsigned)ix < (unsigned)p.IW);
                    x_off[i] = ok ? b_base[i] + (unsigned)(iy * (int)p.xs_h + ix * (int)p.xs_w) * 2u : SBG_OOB_OFFSET;
                }
            }
            const bool ragged = chunk * 64 + 64 > p.Cin;           // (wave-uniform)
#pragma unroll
            for (int i = 0; i < IB; i++) {
                unsigned off = x_off[i];
                if (ragged) off = (chunk * 64 + src_k < p.Cin) ? off : SBG_OOB_OFFSET;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_void_ptr)(st + (wave * IB + i) * 1024), 16, off, chunk * 128, 0, 0);
            }
        };
        auto read_b = [&](int stage) {
            const unsigned char* sb = smem + stage * STAGE + A_BYTES + wp * 128;
#pragma unroll
            for (int ks = 0; ks < 2; ks++)
#pragma unroll
                for (int j = 0; j < TP; j++) fb[ks][j] = *reinterpret_cast<const short8_t*>(sb + j * 16 * 128 + (foff ^ (ks * 64)));
        };
        constexpr int C = IA + IB;                       // DMA instructions per wave per step
        // steps are tap-major: step = t * kchunks + chunk; (it, ic) = coordinates of the step whose loads are issued next
        // split K: workgroup blockIdx.y of gridDim.y takes steps [s_begin, s_begin + nsteps)
        int s_begin = 0;
        if (p.ksplit > 1) {
            const int per = (nsteps_all + p.ksplit - 1) / p.ksplit;
            s_begin = blockIdx.y * per;
            nsteps = nsteps_all - s_begin < per ? nsteps_all - s_begin : per;
            if (nsteps < 0) nsteps = 0;
        }
        int it = s_begin / kchunks, ic = s_begin - it * kchunks, wstage = 0;
        auto issue_next = [&]() {
            issue_w(it, ic, wstage); issue_x(it, ic, wstage);
            wstage = wstage == NSTAGE - 1 ? 0 : wstage + 1;
            if (++ic == kchunks) { ic = 0; it++; }
        };
        if constexpr (LEAD == 2) {
        if (nsteps > 0) issue_next();
        if (nsteps > 1) { issue_next(); wait_vmcnt_const<C>(); } else wait_vmcnt_const<0>();
        if (grpY) __builtin_amdgcn_s_barrier();
        int stage = 0;
        for (int s = 0; s < nsteps; s++) {
            if (!grpY) { if (s + 1 < nsteps) wait_vmcnt_const<C>(); else wait_vmcnt_const<0>(); }     // step s; step s + 1 may be in flight
            __builtin_amdgcn_s_barrier();                // B_a
            read_a(stage); read_b(stage);
            if (s + LEAD < nsteps) issue_next();
            if (grpY) { if (s + 2 < nsteps) wait_vmcnt_const<C>(); else wait_vmcnt_const<0>(); }      // step s + 1; step s + 2 may be in flight
            __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0)
            __builtin_amdgcn_s_barrier();                // B_b
            __builtin_amdgcn_sched_barrier(0);
            mma();
            __builtin_amdgcn_sched_barrier(0);
            stage = stage == NSTAGE - 1 ? 0 : stage + 1;
        }
        if (!grpY) __builtin_amdgcn_s_barrier();
        } else {
        // Two stages, ONE step of loads in flight.  Barrier indices as above.  Stage s % 2 is read by X between barriers 2s and 2s + 1
        // and by Y between 2s + 1 and 2s + 2 (each group's reads retired, lgkmcnt(0), before its B_b(s)), so it is free from global
        // barrier 2s + 2 on and takes the loads of step s + 2; said for step s + 1: they may be issued behind global barrier 2s.
        //   X: 2s is its B_a(s) -- it issues step s + 1 beside its fragment reads of step s, as the three-stage form does.
        //   Y: 2s is its B_b(s - 1).  Behind its B_a(s) = 2s + 1 it would have to wait for the same loads before its B_b(s) of that
        //      iteration (X reads them behind 2s + 2) and would expose the whole load latency, so Y issues step s + 2 behind its
        //      B_b(s), one piece behind every eighth of the 64 MFMAs of step s.  (All eight pieces in front of the MFMAs: 4-5 % slower on
        //      every shape; all behind them: the same within 1 %, 1-3 % slower at Cin 512.  DESIGN.md section 4.)
        //   RAW: a wave's loads of step s + 1 go out behind global barrier 2s and are waited for (vmcnt(0): nothing newer is in
        //        flight) in front of global barrier 2s + 2 -- X at the top of iteration s + 1, before B_a(s + 1); Y in iteration s,
        //        before B_b(s) -- a full step later; stage (s + 1) % 2 is first read behind 2s + 2 (X's B_a(s + 1)).
        //   WAR: stage (s + 1) % 2 held step s - 1, whose reads are retired before X's B_b(s - 1) = 2s - 1 and Y's B_b(s - 1) = 2s.
        //   Start: everybody issues step 0; Y issues step 1 too (its "B_b(-1)" is the extra barrier 0, the stages are empty) and
        //   waits for its step 0 in front of barrier 0; X waits for its step 0 in front of its B_a(0) = 0.
        // Every wait is vmcnt(0) or a compile-time count; the two groups run separate loops, and Y's last two steps (nothing left to
        // issue) are peeled, so the only branch between its B_b and its MFMAs is the tap change of the step it issues.
        static_assert(NSTAGE == 2 && LEAD == 1, "two stages");
        // Registers: 128 accumulators and 96 fragment registers leave 32 of the 256 for everything else, so a pixel piece keeps TWO values
        // (the three-stage form keeps three): the byte offset of its tap-(0, 0) input pixel and its (row, column) packed in 16 + 16 bits for the
        // range test (the launcher admits output grids whose rows and columns stay below 32768 only; an invalid pixel has row -16384); the tap's byte shift is a scalar.  The tap
        // table packs (dy, dx) the same way.  The wave's IA weight pieces are rows of ONE 32-row block: chmap() puts piece k at channel
        // 16 (k & 1) + 4 (k >> 1) of piece 0's, a scalar that rides in the DMA's scalar offset beside (tap, slab) -- one register for the four
        // (the block is in range or out as a whole: the launcher admits Cout % 256 == 0 only).
        static_assert(IA == 4, "weight pieces of a wave = one 32-row block");
        const int tbl_dyx = tbl_dy * 65536 | (tbl_dx & 0xffff);
        unsigned b_org[IB]; int b_yx[IB];
#pragma unroll
        for (int i = 0; i < IB; i++) {
            const int pix = p0 + (wave * IB + i) * 8 + lrow;
            const bool ok = pix < p.P;
            const int pp = ok ? pix : 0;
            const int ox = pp % p.OW, t = pp / p.OW, oy = t % p.OH, n = t / p.OH;
            b_yx[i] = ((ok ? oy * p.stride : -16384) * 65536) | (ox * p.stride);
            b_org[i] = (unsigned)(n * (int)p.xs_n + oy * p.stride * (int)p.xs_h + ox * p.stride * (int)p.xs_w + src_k) * 2u;
        }
        auto tap_prep = [&](int t) {                     // issue_x's per-tap part
            if (t != x_tap) {                            // (wave-uniform)
                x_tap = t;
                const int dyx = __builtin_amdgcn_readlane(tbl_dyx, t), dy = dyx >> 16, dx = (int)(short)(dyx & 0xffff);
                const unsigned shift = (unsigned)(dy * (int)p.xs_h + dx * (int)p.xs_w) * 2u;
#pragma unroll
                for (int i = 0; i < IB; i++) {
                    const int iy = (b_yx[i] >> 16) + dy, ix = (b_yx[i] & 0xffff) + dx;
                    const bool ok = ((unsigned)iy < (unsigned)p.IH) & ((unsigned)ix < (unsigned)p.IW);
                    x_off[i] = ok ? b_org[i] + shift : SBG_OOB_OFFSET;
                }
            }
        };
        auto issue_piece = [&](auto k_tag, int t, int chunk, int stg) {      // piece k of the wave's C: weight pieces first, then pixel pieces
            constexpr int k = decltype(k_tag)::value;
            unsigned char* st = smem + stg * STAGE;
            const bool ragged = chunk * 64 + 64 > p.Cin;          // (wave-uniform)
            if constexpr (k < IA) {
                const int wtap = __builtin_amdgcn_readlane(tbl_wtap, t) + chunk * 128 + (16 * (k & 1) + 4 * (k >> 1)) * (int)p.ws_co * 2;
                unsigned off = a_base[0];
                if (ragged) off = (chunk * 64 + src_k < p.Cin) ? off : SBG_OOB_OFFSET;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (lds_void_ptr)(st + (wave * IA + k) * 1024), 16, off, wtap, 0, 0);
            } else {
                constexpr int i = k - IA;
                unsigned off = x_off[i];
                if (ragged) off = (chunk * 64 + src_k < p.Cin) ? off : SBG_OOB_OFFSET;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_void_ptr)(st + A_BYTES + (wave * IB + i) * 1024), 16, off, chunk * 128, 0, 0);
            }
        };
        auto issue_advance = [&]() {
            wstage ^= 1;
            if (++ic == kchunks) { ic = 0; it++; }
        };
        auto issue_all = [&]() {                         // all C pieces of the next step
            tap_prep(it);
            sbg_static_for<C>([&](auto k_tag) { issue_piece(k_tag, it, ic, wstage); });
            issue_advance();
        };
        constexpr int NG = 2 * TC, GPP = NG / C;        // MFMA groups (TP MFMAs each) of a step; groups per DMA piece
        static_assert(NG % C == 0, "pieces spread evenly over the MFMA groups");
        auto mma_issue = [&]() {                         // Y: the MFMAs of step s with the loads of step s + 2 spread between them
            tap_prep(it);
            sbg_static_for<NG>([&](auto q_tag) {
                constexpr int q = decltype(q_tag)::value, ks = q / TC, i = q % TC;
#pragma unroll
                for (int j = 0; j < TP; j++) acc[i][j] = Mfma<MF>::run(fa[ks][i], fb[ks][j], acc[i][j]);
                if constexpr ((q + 1) % GPP == 0) {
                    __builtin_amdgcn_sched_barrier(0);
                    issue_piece(std::integral_constant<int, (q + 1) / GPP - 1>{}, it, ic, wstage);
                    __builtin_amdgcn_sched_barrier(0);
                }
            });
            issue_advance();
        };
        if (nsteps > 0) issue_all();
        int stage = 0;
        if (!grpY) {
            for (int s = 0; s < nsteps; s++) {
                wait_vmcnt_const<0>();                       // this wave's loads of step s
                __builtin_amdgcn_s_barrier();                // B_a
                read_a(stage); read_b(stage);
                if (s + 1 < nsteps) issue_all();
                __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0)
                __builtin_amdgcn_s_barrier();                // B_b
                __builtin_amdgcn_sched_barrier(0);
                mma();
                __builtin_amdgcn_sched_barrier(0);
                stage ^= 1;
            }
            __builtin_amdgcn_s_barrier();
        } else {
            if (nsteps > 1) { issue_all(); wait_vmcnt_const<C>(); } else wait_vmcnt_const<0>();
            __builtin_amdgcn_s_barrier();                    // 0
            auto y_step = [&](auto more_tag) {
                constexpr bool more = decltype(more_tag)::value;      // step s + 2 exists
                __builtin_amdgcn_s_barrier();                // B_a
                read_a(stage); read_b(stage);
                wait_vmcnt_const<0>();                       // this wave's loads of step s + 1
                __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0)
                __builtin_amdgcn_s_barrier();                // B_b
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (more) mma_issue(); else mma();
                __builtin_amdgcn_sched_barrier(0);
                stage ^= 1;
            };
            int s = 0;
            for (; s + 2 < nsteps; s++) y_step(std::true_type{});
            for (; s < nsteps; s++) y_step(std::false_type{});
        }
        }
    }

    // ---- epilogue ---------------------------------------------------------------------------------------------------
    conv_epilogue8<TC, TP>(p, acc, c0 + wc, fg, [&](int j, int& n, int& oy, int& ox) {
        const int pix = p0 + wp + 16 * j + fr;
        const int pp = pix < p.P ? pix : 0;
        ox = pp % p.OW; const int t = pp / p.OW; oy = t % p.OH; n = t / p.OH;
        return pix < p.P;
    });
}

// ---------------------------------------------------------------------------------------------------------------------
// Halo kernel with loader waves.  12 waves: 0-3 (X) and 4-7 (Y) compute in ping-pong as above but issue NO vector-memory
// instruction inside the K loop; waves 8-9 stream the weight tiles, waves 10-11 the halo.  Why: (1) a compute wave's
// non-MFMA phase shrinks to `barrier, 16 ds_read_b128, barrier`; (2) vmcnt retires in order, so in the 8-wave kernel a halo
// piece that misses L2 (537 MB activations do not fit the 256 MB Infinity Cache) stalled the weight stream queued behind it --
// here the halo loaders have a whole slice (nine K-steps) of lead and the weight loaders never wait for HBM.
// Every wave executes exactly 2 S + 1 workgroup barriers (S = K-steps of all tiles of this workgroup), index g = 0 .. 2S:
//   X: B_a(s) = 2s, B_b(s) = 2s + 1, final 2S;   Y: first 0, B_a(s) = 2s + 1, B_b(s) = 2s + 2;
//   weight loader: per step { wait W(s) landed; 2s; issue W(s + 3) into the stage step s - 1 used (its reads retired before
//                  2s); 2s + 1 }, final 2S;      halo loader: per slice c { vmcnt(0): halo(c) landed; 18c; issue halo(c + 1) into
//                  the buffer slice c - 1 used; 18c + 1 .. 18c + 17 }, final 2S.
template <class MF, int TH, int TW>
__global__ __launch_bounds__(768, 3) void conv_halo_ld_kernel(ConvArgs p, unsigned x_bytes, unsigned w_bytes)
{
    constexpr int BC = 128, BP = 256, WGP = 4;
    constexpr int WC = 64, WP = 64, TC = 4, TP = 4;
    static_assert(TH * TW == BP, "halo tile = TH x TW pixels");
    constexpr int NSTAGE = 4, STAGE = BC * 128;        // weight stages: the loads of step s + 3 are issued while step s computes
    constexpr int PW = TW + 2, PH = TH + 2, NPIX = PW * PH;
    constexpr int HPIECES = (NPIX + 7) / 8, HALO_BYTES = HPIECES * 1024;
    constexpr int NT = 9, SEG = TW / 16;
    constexpr int WPIECES = BC / 8 / 2;                // weight pieces per weight loader per step
    constexpr int HPL = (HPIECES + 1) / 2;             // halo pieces per halo loader per slice

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const sH = smem + NSTAGE * STAGE;
    unsigned char* const sP = sH + 2 * HALO_BYTES;     // epilogue parameters of the tile being computed: two buffers (tile parity) of 3 KiB
    constexpr int PARAM_BYTES = 3072;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bid = xcd_tile_order(blockIdx.x, gridDim.x);
    const int tiles_x = p.OW / TW, tiles_y = p.OH / TH;
    const int ntiles = p.ptiles * p.ctiles, G = gridDim.x;
    const int my_tiles = (ntiles - bid + G - 1) / G;                  // tiles bid, bid + G, ...  (the grid never exceeds ntiles)
    const int kchunks = (p.Cin + 63) >> 6;
    const int nslices = my_tiles * kchunks;                            // slice = one 64-channel slab of one tile = nine K-steps
    struct TileC { int c0, tn, y0, x0; };
    auto decode = [&](int tile) -> TileC {
        TileC r;
        const int ct_ = tile % p.ctiles; int pt_ = tile / p.ctiles;
        const int tx = pt_ % tiles_x; pt_ /= tiles_x;
        const int ty = pt_ % tiles_y;
        r.c0 = ct_ * BC; r.tn = pt_ / tiles_y; r.y0 = ty * TH; r.x0 = tx * TW;
        return r;
    };
    // tile + G without divisions: G in the mixed radix (ctiles, tiles_x, tiles_y), added with carries.  (decode()'s four scalar divisions are
    // ~1000 cycles; the compute waves ran them between a tile's last MFMA and the barrier their partner group was waiting at.)
    const TileC gstep = decode(G);                       // digits of G, scaled like the coordinates
    auto advance = [&](TileC t_) -> TileC {
        t_.c0 += gstep.c0; int carry = t_.c0 >= p.ctiles * BC; t_.c0 -= carry ? p.ctiles * BC : 0;
        t_.x0 += gstep.x0 + (carry ? TW : 0); carry = t_.x0 >= tiles_x * TW; t_.x0 -= carry ? tiles_x * TW : 0;
        t_.y0 += gstep.y0 + (carry ? TH : 0); carry = t_.y0 >= tiles_y * TH; t_.y0 -= carry ? tiles_y * TH : 0;
        t_.tn += gstep.tn + carry;
        return t_;
    };
    const int lrow = dma_lrow(lane);
    const int src_k = dma_src_k(lane, lrow);      // DMA lane coordinates

    if (wave >= 10) {
        // ---------------------------------------------------------------- halo loader (waves 10, 11) ----------------------
        const int lh = wave - 10;
        __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)x_bytes, 0x00020000);
        // epilogue parameters of tile `t_` -> parameter buffer `buf` (wave 10 only): the noise of the TH x TW tile (one 16-B piece per lane, row-major),
        // the bias of the tile's 128 channels and the demodulation coefficients of (image, those channels) (lanes 0-31).  Issued during the tile's LAST
        // slice; this wave's vmcnt(0) in front of the next slice's first barrier covers them, and the tile's epilogue runs behind that barrier.
        auto issue_params = [&](int t_, int buf) {
            const TileC pc = decode(t_);
            unsigned char* dst = sP + buf * PARAM_BYTES;
            if (p.noise) {
                __amdgpu_buffer_rsrc_t nr = __builtin_amdgcn_make_buffer_rsrc((void*)p.noise, 0, 0x7fffffff, 0x00020000);
                constexpr int LPR = TW / 4;
                const int r = lane / LPR, cx = (lane - r * LPR) * 4;
                const unsigned off = (unsigned)(pc.tn * (int)p.noise_sn + (pc.y0 + r) * p.OW + pc.x0 + cx) * 4u;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(nr, (lds_void_ptr)dst, 16, off, 0, 0, 0);
            }
            const int co = pc.c0 + 4 * lane;
            const unsigned okm = 0u - (unsigned)((lane < 32) & (co < p.Cout));
            if (p.bias) {
                __amdgpu_buffer_rsrc_t br_ = __builtin_amdgcn_make_buffer_rsrc((void*)p.bias, 0, 0x7fffffff, 0x00020000);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(br_, (lds_void_ptr)(dst + 1024), 16, (((unsigned)co * 4u) & okm) | (SBG_OOB_OFFSET & ~okm), 0, 0, 0);
            }
            if (p.oscale) {
                __amdgpu_buffer_rsrc_t sr = __builtin_amdgcn_make_buffer_rsrc((void*)p.oscale, 0, 0x7fffffff, 0x00020000);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(sr, (lds_void_ptr)(dst + 2048), 16, (((unsigned)(pc.tn * p.Cout + co) * 4u) & okm) | (SBG_OOB_OFFSET & ~okm), 0, 0, 0);
            }
        };
        // The loader's HPL pieces of a slice with everything per-lane worked out ONCE: rel[i] = byte offset of piece i's halo pixel (py, px) and k-slot from the halo's
        // origin, flag bits {py == 0, py == PH - 1, px == 0, px == PW - 1, no pixel} (5 per piece, 6 pieces per word).  Per slice the origin's byte offset
        // and the tile's edge mask are scalars, so an issue is ~5 vector instructions instead of ~25 (a division by PW, two range tests, three multiplies).
        // The loader waves share their SIMDs with the compute waves and were the last to arrive at every second barrier (clock stamps at every barrier):
        // +3 .. 4.5 %.
        int rel[HPL]; unsigned ef[(HPL + 5) / 6];
#pragma unroll
        for (int w_ = 0; w_ < (HPL + 5) / 6; w_++) ef[w_] = 0;
#pragma unroll
        for (int i = 0; i < HPL; i++) {
            const int piece = lh * HPL + i, pp = piece * 8 + lrow;
            const int py = pp / PW, px = pp - py * PW;
            rel[i] = (py * (int)p.xs_h + px * (int)p.xs_w + src_k) * 2;
            const unsigned f = (unsigned)(py == 0) | ((unsigned)(py == PH - 1) << 1) | ((unsigned)(px == 0) << 2) | ((unsigned)(px == PW - 1) << 3)
                             | ((unsigned)((piece >= HPIECES) | (pp >= NPIX)) << 4);
            ef[i / 6] |= f << (5 * (i % 6));
        }
        auto issue_halo = [&](auto i_tag, int hbase, unsigned emask, bool kok, int buf) {
            constexpr int i = decltype(i_tag)::value;
            const int piece = lh * HPL + i;
            if (piece >= HPIECES) return;                // (wave-uniform)
            const bool bad = (((ef[i / 6] >> (5 * (i % 6))) & emask) != 0u) | !kok;
            const unsigned off = bad ? SBG_OOB_OFFSET : (unsigned)(rel[i] + hbase);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_void_ptr)(sH + buf * HALO_BYTES + piece * 1024), 16, off, 0, 0, 0);
        };
        auto halo_base = [&](const TileC& t_, int chunk_) { return (t_.tn * (int)p.xs_n + (t_.y0 - 1) * (int)p.xs_h + (t_.x0 - 1) * (int)p.xs_w + chunk_ * 64) * 2; };
        auto edge_mask = [&](const TileC& t_) {
            const unsigned m = (unsigned)(t_.y0 == 0) | ((unsigned)(t_.y0 + TH == p.IH) << 1) | ((unsigned)(t_.x0 == 0) << 2) | ((unsigned)(t_.x0 + TW == p.IW) << 3) | 16u;
            return (unsigned)__builtin_amdgcn_readfirstlane((int)m);
        };
        int ctile = bid, cchunk = 0, cpar = 0;          // tile / chunk of the slice being computed, parity of that tile's ordinal
        int tile = bid, chunk = 0;
        TileC tc = decode(tile);
        {
            const int hbase = halo_base(tc, 0); const unsigned emask = edge_mask(tc);
            sbg_static_for<HPL>([&](auto it_) { issue_halo(it_, hbase, emask, src_k < p.Cin, 0); });
        }
        // The 22 pieces of the next slice go out TWO per half-step (behind each of the slice's first eleven barriers), not as one burst behind
        // the first: an LDS-DMA instruction costs its wave ~100+ cycles beside the compute waves' fragment reads, every wave of the workgroup
        // meets at the next barrier, and a burst of 22 made that one half-step ~4x as long as the 32 MFMAs it should hide behind.  Measured
        // (interleaved rounds on one device, [64, C, R, R] (*) [C, C, 3, 3]): C = 128 @ 256^2 1070 -> 1160 TF,
        // 256 @ 128^2 1154 -> 1300, 512 @ 64^2 1214 -> 1389, 512 @ 32^2 1273 -> 1390; three or four per half-step 1090-1110 / 1220-1250 /
        // 1280-1310.  (One piece behind each of the later barriers instead of two behind the first eleven: no difference.)
        constexpr int per = 2;                           // pieces per half-step
        for (int c = 0; c < nslices; c++) {
            wait_vmcnt_const<0>();                       // halo(c) has landed
            __builtin_amdgcn_s_barrier();                // 18c
            const bool more = c + 1 < nslices;
            if (more) {
                if (++chunk == kchunks) { chunk = 0; tile += G; tc = advance(tc); }
            }
            const int hbase = halo_base(tc, chunk); const unsigned emask = edge_mask(tc);
            const bool kok = chunk * 64 + src_k < p.Cin;
            sbg_static_for<17>([&](auto it_) {
                constexpr int i = decltype(it_)::value;
                if (more) {
                    if constexpr (per * i < HPL)     issue_halo(std::integral_constant<int, (per * i < HPL ? per * i : 0)>{}, hbase, emask, kok, (c + 1) & 1);
                    if constexpr (per * i + 1 < HPL) issue_halo(std::integral_constant<int, (per * i + 1 < HPL ? per * i + 1 : 0)>{}, hbase, emask, kok, (c + 1) & 1);
                }
                if (i == 12 && lh == 0 && p.lds_params && cchunk == kchunks - 1) issue_params(ctile, cpar);
                if (i == 16 && p.lds_params && c + 1 == nslices) wait_vmcnt_const<0>();      // the LAST tile's parameters have no later slice whose first barrier would cover them
                __builtin_amdgcn_s_barrier();
            });
            if (++cchunk == kchunks) { cchunk = 0; ctile += G; cpar ^= 1; }
        }
        __builtin_amdgcn_s_barrier();                    // 2S
        return;
    }
    if (wave >= 8) {
        // ---------------------------------------------------------------- weight loader (waves 8, 9) ----------------------
        const int lw = wave - 8;
        __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (int)w_bytes, 0x00020000);
        const int tl = lane < p.ntaps ? lane : 0;
        const int tbl_wtap = p.tap_slab[tl] * (int)p.ws_slab * 2;
        unsigned a_base[WPIECES];
        auto weight_rows = [&](int c0_) {
#pragma unroll
            for (int i = 0; i < WPIECES; i++) {
                const int co = c0_ + chmap((lw * WPIECES + i) * 8 + lrow);
                a_base[i] = (co < p.Cout) ? (unsigned)(co * (int)p.ws_co + src_k) * 2u : SBG_OOB_OFFSET;
            }
        };
        // (it, ichunk, itile, istage): coordinates of the step whose weights are issued next
        int it = 0, ichunk = 0, itile = bid, istage = 0;
        weight_rows(decode(itile).c0);
        unsigned char* st = nullptr; unsigned kokm = 0, wtap = 0;
        auto issue_prep = [&]() {
            st = smem + istage * STAGE + lw * WPIECES * 1024;
            kokm = 0u - (unsigned)(ichunk * 64 + src_k < p.Cin);
            wtap = (unsigned)(__builtin_amdgcn_readlane(tbl_wtap, it) + ichunk * 128);
        };
        // Whole 64-channel slabs (Cin % 64 == 0): the step's (tap, slab) offset is a scalar and rides in the instruction's scalar offset, so a piece
        // is the DMA and nothing else (a_base[i] stays 0x80000000 for a row past Cout: out of range with or without the scalar part).  The six vector
        // instructions per piece this removes (48 per step, in waves that share their SIMDs with the compute waves) were worth +7 .. 9 %:
        // [64, C, R, R] (*) [C, C, 3, 3], interleaved rounds: C = 128 @ 256^2 1187 -> 1270 TF, 256 @ 128^2 1321 -> 1439, 512 @ 64^2 1401 -> 1526.
        const bool whole_k = (p.Cin & 63) == 0;
        auto issue_part = [&](int lo, int hi) {
            if (whole_k) {
#pragma unroll
                for (int i = 0; i < WPIECES; i++)
                    if (i >= lo && i < hi) __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (lds_void_ptr)(st + i * 1024), 16, a_base[i], wtap, 0, 0);
                return;
            }
#pragma unroll
            for (int i = 0; i < WPIECES; i++) {
                if (i < lo || i >= hi) continue;
                const unsigned okm = kokm & (0u - (unsigned)(a_base[i] != SBG_OOB_OFFSET));
                const unsigned off = ((a_base[i] + wtap) & okm) | (SBG_OOB_OFFSET & ~okm);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (lds_void_ptr)(st + i * 1024), 16, off, 0, 0, 0);
            }
        };
        auto issue_done = [&]() {
            istage = (istage + 1) & (NSTAGE - 1);
            if (++it == NT) {
                it = 0;
                if (++ichunk == kchunks) { ichunk = 0; itile += G; if (itile < ntiles) weight_rows(decode(itile).c0); }
            }
        };
        auto issue_next = [&]() { issue_prep(); issue_part(0, WPIECES); issue_done(); };
        constexpr bool split = false;                    // (half of a step's pieces behind each of its two barriers: +2..4 % alone, none beside the spread halo loads)
        const int S = nslices * NT;
        int issued = 0;                                  // steps issued so far
        for (; issued < 4 && issued < S; issued++) issue_next();
        for (int s = 0; s < S; s++) {
            // W(s) has landed once at most the steps issued after it are outstanding
            const int newer = issued - 1 - s;            // 0 .. 3
            if (newer >= 3) wait_vmcnt_const<3 * WPIECES>();
            else if (newer == 2) wait_vmcnt_const<2 * WPIECES>();
            else if (newer == 1) wait_vmcnt_const<1 * WPIECES>();
            else wait_vmcnt_const<0>();
            __builtin_amdgcn_s_barrier();                // 2s
            const bool go = s >= 1 && issued < S;      // step s + 3 -> the stage step s - 1 was read from
            if (go) { issue_prep(); issue_part(0, split ? WPIECES / 2 : WPIECES); }
            __builtin_amdgcn_s_barrier();                // 2s + 1
            if (go) { if (split) issue_part(WPIECES / 2, WPIECES); issue_done(); issued++; }
            else if (s >= 1 && issued < S) issued++;
        }
        __builtin_amdgcn_s_barrier();                    // 2S
        return;
    }

    // -------------------------------------------------------------------- compute waves (0-7) ----------------------------
    const bool grpY = wave >= 4;
    const int wci = wave >> 2, wpi = wave & 3;           // waves 0-3 and 4-7 each cover both channel halves? no: wave = wci * 4 + wpi
    const int wc = wci * WC;
    const int fr = lane & 15, fg = lane >> 4;
    const int foff = frag_off(fr, fg);
    const int tl = lane < p.ntaps ? lane : 0;
    const int tbl_shift = p.tap_dy[tl] * PW + p.tap_dx[tl];
    float4_t acc[TC][TP];
#pragma unroll
    for (int i = 0; i < TC; i++)
#pragma unroll
        for (int j = 0; j < TP; j++) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};
    short8_t fa[2][TC], fb[2][TP];
    int seg_pp[TP];                                      // patch pixel of (segment j, lane fr) for tap (0, 0)
#pragma unroll
    for (int j = 0; j < TP; j++) {
        const int sg = wpi * TP + j, r = sg / SEG, cseg = (sg - r * SEG) * 16;
        seg_pp[j] = (r + 1) * PW + cseg + fr + 1;
    }
    int stage = 0, par = 0, chunk = 0, tile = bid;
    TileC cur = decode(tile);
    // The epilogue of a finished tile is deferred into the first step of the next tile, behind that step's B_a: there it runs
    // beside the partner group's MFMA phase instead of holding both groups at a barrier (the stores are the exposed part of a
    // short-K tile: 18 K-steps at Cin = 128).
    bool pend = false;
    TileC done = cur;
    int tpar = 0, done_par = 0;                          // parity of the current / finished tile's ordinal: its parameter buffer
    auto epilogue = [&](const TileC& tc) __attribute__((always_inline)) {
        const LdsParams lp{(lds_cfloat*)(sP + done_par * PARAM_BYTES), wc, TW};
        conv_epilogue8<TC, TP, true>(p, acc, tc.c0 + wc, fg, [&](int j, int& n, int& oy, int& ox) {
            const int sg = wpi * TP + j, r = sg / SEG, cseg = (sg - r * SEG) * 16;
            n = tc.tn; oy = tc.y0 + r; ox = tc.x0 + cseg + fr;
            return true;
        }, 0, p.lds_params ? &lp : nullptr, tc.y0, tc.x0);
#pragma unroll
        for (int i = 0; i < TC; i++)
#pragma unroll
            for (int j = 0; j < TP; j++) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};
    };
    if (grpY) __builtin_amdgcn_s_barrier();              // 0
    for (int c = 0; c < nslices; c++) {
        const unsigned char* hb = sH + par * HALO_BYTES;
        sbg_static_for<NT>([&](auto tap_tag) {
            constexpr int t = decltype(tap_tag)::value;
            const int shift = __builtin_amdgcn_readlane(tbl_shift, t);
            const unsigned char* sa = smem + stage * STAGE + wc * 128;
            __builtin_amdgcn_s_barrier();                // B_a: the stage and the halo buffer of this step have landed
            if (t == 0 && pend) { epilogue(done); pend = false; }
#pragma unroll
            for (int ks = 0; ks < 2; ks++)
#pragma unroll
                for (int i = 0; i < TC; i++) fa[ks][i] = *reinterpret_cast<const short8_t*>(sa + i * 16 * 128 + (foff ^ (ks * 64)));
#pragma unroll
            for (int j = 0; j < TP; j++) {
                const int pp = seg_pp[j] + shift;
                const int o = pp * 128 + ((fg ^ (pp & 7)) << 4);
#pragma unroll
                for (int ks = 0; ks < 2; ks++) fb[ks][j] = *reinterpret_cast<const short8_t*>(hb + (o ^ (ks * 64)));
            }
            __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0): fragments are in registers, this wave no longer reads the stage
            __builtin_amdgcn_s_barrier();                // B_b
            __builtin_amdgcn_sched_barrier(0);
            mma_step<MF>(acc, fa, fb);
            __builtin_amdgcn_sched_barrier(0);
            stage = (stage + 1) & (NSTAGE - 1);
        });
        par ^= 1;
        if (++chunk < kchunks) continue;
        done = cur; done_par = tpar; tpar ^= 1;
        // X defers its epilogue behind the next step's B_a (Y is then in its last MFMA phase).  With a fused tail (its arithmetic makes the epilogue
        // ~40 % longer) Y runs its own right away, behind its last MFMA, in the interval in which X runs X's: the two groups' tail arithmetic and
        // stores side by side take less than one after the other (deferred like X's, Y's epilogue filled a second ~3850-cycle interval while X
        // waited at the next barrier; clock stamps).  Measured, interleaved rounds: with tail +3 / +1.7 / +1 % (128 / 256 / 512 channels),
        // plain stores -1 % -- a plain launch keeps both deferred.
        if (grpY && p.lds_params) epilogue(done); else pend = true;
        chunk = 0; tile += G;
        if (tile < ntiles) cur = advance(cur);
    }
    if (pend) epilogue(done);
    if (!grpY) __builtin_amdgcn_s_barrier();             // 2S
}

// ---------------------------------------------------------------------------------------------------------------------
// Gather kernel with loader waves: the 128 x 256 tile of conv_k64_kernel in the persistent 12-wave structure of
// conv_halo_ld_kernel.  Waves 8-9 stream the weight tile, waves 10-11 gather the 256 pixel rows of the tap (im2col on the
// fly, out-of-image rows at an out-of-range offset); three 48 KB stages, the loads of step s + 2 are issued while step s
// computes.  Tiles bid, bid + G, ... run through one pipeline, the epilogue of a tile is deferred into the next tile's first
// step.  Transposed-convolution phases and strided convolutions have 2-36 K-steps per tile, so the per-tile prologue /
// epilogue of the one-tile-per-workgroup kernel was a third of their time.
// Barrier indices as in conv_halo_ld_kernel; every loader: per step { wait step s landed; 2s; issue step s + 2 into the stage
// step s - 1 used (its reads retired before 2s); 2s + 1 }, final 2S.
template <class MF>
__global__ __launch_bounds__(768, 3) void conv_gather_ld_kernel(ConvArgs p, unsigned x_bytes, unsigned w_bytes)
{
    constexpr int BC = 128, BP = 256, WGP = 4;
    constexpr int WC = 64, WP = 64, TC = 4, TP = 4;
    constexpr int NSTAGE = 3, A_BYTES = BC * 128, B_BYTES = BP * 128, STAGE = A_BYTES + B_BYTES;
    constexpr int WPIECES = BC / 8 / 2;                // weight pieces per weight loader per step (8)
    constexpr int XPIECES = BP / 8 / 2;                // pixel pieces per pixel loader per step (16)

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bid = xcd_tile_order(blockIdx.x, gridDim.x);
    const int ntiles = p.ptiles * p.ctiles, G = gridDim.x;
    const int my_tiles = (ntiles - bid + G - 1) / G;                  // tiles bid, bid + G, ...  (the grid never exceeds ntiles)
    const int kchunks = (p.Cin + 63) >> 6;
    // tile -> (channel tile, phase, pixel tile): the phases of one pixel tile are neighbours in the tile order, so they run at the same
    // time on CUs of one XCD and share the input rows through its L2.  K-steps of a tile, tap-major: step = t * kchunks + chunk.
    // The phases have different K lengths (4 / 2 / 2 / 1 taps), and tile + G keeps r % nphase, so the phase is rotated with the pixel
    // tile: every workgroup then walks all phases in turn (equal work) -- still a bijection on (pixel tile, phase).
    auto tile_phase = [&](int tile) { const int r = tile / p.ctiles; return (r % p.nphase + (r / p.nphase) / p.ph_rot_div) % p.nphase; };
    int S = 0;
    for (int t_ = bid; t_ < ntiles; t_ += G) S += p.ph_ntaps[tile_phase(t_)] * kchunks;
    const int lrow = dma_lrow(lane);
    const int src_k = dma_src_k(lane, lrow);      // DMA lane coordinates
    const int tl = lane < p.ntaps ? lane : 0;

    if (wave >= 8) {
        // ---------------------------------------------------------------- loader waves -----------------------------------
        const bool xload = wave >= 10;                  // waves 10, 11 gather pixels; 8, 9 stream weights
        const int lw = (wave - 8) & 1;
        __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)x_bytes, 0x00020000);
        __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (int)w_bytes, 0x00020000);
        const int tbl_dy = p.tap_dy[tl], tbl_dx = p.tap_dx[tl];
        const int tbl_wtap = p.tap_slab[tl] * (int)p.ws_slab * 2;
        unsigned a_base[WPIECES];
        int b_iy0[XPIECES], b_ix0[XPIECES]; unsigned b_base[XPIECES];
        int ph_t0 = 0, ph_nt = 1;                       // taps of the issue tile's phase
        auto tile_state = [&](int tile) {
            const int ph = tile_phase(tile);
            const int c0 = (tile % p.ctiles) * BC, p0 = (tile / p.ctiles / p.nphase) * BP;
            const int OW_ = p.ph_OW[ph], OH_ = p.ph_OH[ph], P_ = p.ph_P[ph];
            ph_t0 = p.ph_tap0[ph]; ph_nt = p.ph_ntaps[ph];
            if (!xload) {
#pragma unroll
                for (int i = 0; i < WPIECES; i++) {
                    const int co = c0 + chmap((lw * WPIECES + i) * 8 + lrow);
                    a_base[i] = (co < p.Cout) ? (unsigned)(co * (int)p.ws_co + src_k) * 2u : SBG_OOB_OFFSET;
                }
            } else {
#pragma unroll
                for (int i = 0; i < XPIECES; i++) {
                    const int pix = p0 + (lw * XPIECES + i) * 8 + lrow;
                    const bool ok = pix < P_;
                    const int pp = ok ? pix : 0;
                    const int ox = pp % OW_, t = pp / OW_, oy = t % OH_, n = t / OH_;
                    b_iy0[i] = ok ? oy * p.stride : -(1 << 28);            // invalid rows fail every range test below
                    b_ix0[i] = ox * p.stride;
                    b_base[i] = (unsigned)(n * (int)p.xs_n + src_k) * 2u;
                }
            }
        };
        // (it, ic, itile, istage): coordinates of the step whose loads are issued next
        int it = 0, ic = 0, itile = bid, istage = 0;
        tile_state(itile);
        // the loads of one step in two parts (half = 0, 1; half < 0: everything): the two halves go behind the step's two barriers
        auto issue_part = [&](int half) {
            const unsigned kokm = 0u - (unsigned)(ic * 64 + src_k < p.Cin);
            if (!xload) {
                unsigned char* st = smem + istage * STAGE + lw * WPIECES * 1024;
                const unsigned wtap = (unsigned)(__builtin_amdgcn_readlane(tbl_wtap, ph_t0 + it) + ic * 128);
#pragma unroll
                for (int i = 0; i < WPIECES; i++) {
                    if (half >= 0 && (i >= WPIECES / 2) != (half == 1)) continue;
                    const unsigned okm = kokm & (0u - (unsigned)(a_base[i] != SBG_OOB_OFFSET));      // branch-free: a masked-off lane would leave stale LDS bytes
                    const unsigned off = ((a_base[i] + wtap) & okm) | (SBG_OOB_OFFSET & ~okm);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (lds_void_ptr)(st + i * 1024), 16, off, 0, 0, 0);
                }
            } else {
                unsigned char* st = smem + istage * STAGE + A_BYTES + lw * XPIECES * 1024;
                const int dy = __builtin_amdgcn_readlane(tbl_dy, ph_t0 + it), dx = __builtin_amdgcn_readlane(tbl_dx, ph_t0 + it);
#pragma unroll
                for (int i = 0; i < XPIECES; i++) {
                    if (half >= 0 && (i >= XPIECES / 2) != (half == 1)) continue;
                    const int iy = b_iy0[i] + dy, ix = b_ix0[i] + dx;
                    const unsigned okm = kokm & (0u - (unsigned)(((unsigned)iy < (unsigned)p.IH) & ((unsigned)ix < (unsigned)p.IW)));
                    const unsigned real = b_base[i] + (unsigned)(iy * (int)p.xs_h + ix * (int)p.xs_w + ic * 64) * 2u;
                    const unsigned off = (real & okm) | (SBG_OOB_OFFSET & ~okm);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_void_ptr)(st + i * 1024), 16, off, 0, 0, 0);
                }
            }
        };
        auto issue_done = [&]() {
            istage = istage == NSTAGE - 1 ? 0 : istage + 1;
            if (++ic == kchunks) {
                ic = 0;
                if (++it == ph_nt) { it = 0; itile += G; if (itile < ntiles) tile_state(itile); }
            }
        };
        auto issue_next = [&]() { issue_part(-1); issue_done(); };
        constexpr bool split = true;                     // half of a step's pieces behind each of its two barriers (+0.5..1 %)
        int issued = 0;                                  // steps issued so far
        for (; issued < NSTAGE && issued < S; issued++) issue_next();
        for (int s = 0; s < S; s++) {
            // step s has landed once at most the steps issued after it are outstanding (same instruction count per step)
            const int newer = issued - 1 - s;            // 0 .. 2
            if (xload) {
                if (newer >= 2) wait_vmcnt_const<2 * XPIECES>(); else if (newer == 1) wait_vmcnt_const<XPIECES>(); else wait_vmcnt_const<0>();
            } else {
                if (newer >= 2) wait_vmcnt_const<2 * WPIECES>(); else if (newer == 1) wait_vmcnt_const<WPIECES>(); else wait_vmcnt_const<0>();
            }
            __builtin_amdgcn_s_barrier();                // 2s
            const bool go = s >= 1 && issued < S;        // step s + 2 -> the stage step s - 1 was read from
            if (go) issue_part(split ? 0 : -1);
            __builtin_amdgcn_s_barrier();                // 2s + 1
            if (go) { if (split) issue_part(1); issue_done(); issued++; }
        }
        __builtin_amdgcn_s_barrier();                    // 2S
        return;
    }

    // -------------------------------------------------------------------- compute waves (0-7) ----------------------------
    const bool grpY = wave >= 4;
    const int wci = wave >> 2, wpi = wave & 3;
    const int wc = wci * WC, wp = wpi * WP;
    const int fr = lane & 15, fg = lane >> 4;
    const int foff = frag_off(fr, fg);
    float4_t acc[TC][TP];
#pragma unroll
    for (int i = 0; i < TC; i++)
#pragma unroll
        for (int j = 0; j < TP; j++) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};
    short8_t fa[2][TC], fb[2][TP];
    int stage = 0, tile = bid, left = p.ph_ntaps[tile_phase(bid)] * kchunks;      // steps left in the tile being computed
    bool pend = false;
    int done_tile = tile;
    auto epilogue = [&](int t_) __attribute__((always_inline)) {
        const int ph = tile_phase(t_);
        const int c0 = (t_ % p.ctiles) * BC, p0 = (t_ / p.ctiles / p.nphase) * BP;
        const int OW_ = p.ph_OW[ph], OH_ = p.ph_OH[ph], P_ = p.ph_P[ph];
        conv_epilogue8<TC, TP>(p, acc, c0 + wc, fg, [&](int j, int& n, int& oy, int& ox) {
            const int pix = p0 + wp + 16 * j + fr;
            const int pp = pix < P_ ? pix : 0;
            ox = pp % OW_; const int t = pp / OW_; oy = t % OH_; n = t / OH_;
            return pix < P_;
        }, p.ph_yoff[ph]);
#pragma unroll
        for (int i = 0; i < TC; i++)
#pragma unroll
            for (int j = 0; j < TP; j++) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};
    };
    if (grpY) __builtin_amdgcn_s_barrier();              // 0
    for (int s = 0; s < S; s++) {
        const unsigned char* sa = smem + stage * STAGE + wc * 128;
        const unsigned char* sb = smem + stage * STAGE + A_BYTES + wp * 128;
        __builtin_amdgcn_s_barrier();                    // B_a: the stage of this step has landed
        if (pend) { epilogue(done_tile); pend = false; } // previous tile's stores run beside the partner group's MFMA phase
#pragma unroll
        for (int ks = 0; ks < 2; ks++)
#pragma unroll
            for (int i = 0; i < TC; i++) fa[ks][i] = *reinterpret_cast<const short8_t*>(sa + i * 16 * 128 + (foff ^ (ks * 64)));
#pragma unroll
        for (int ks = 0; ks < 2; ks++)
#pragma unroll
            for (int j = 0; j < TP; j++) fb[ks][j] = *reinterpret_cast<const short8_t*>(sb + j * 16 * 128 + (foff ^ (ks * 64)));
        __builtin_amdgcn_s_waitcnt(0xC07F);              // lgkmcnt(0): fragments are in registers, this wave no longer reads the stage
        __builtin_amdgcn_s_barrier();                    // B_b
        __builtin_amdgcn_sched_barrier(0);
        mma_step<MF>(acc, fa, fb);
        __builtin_amdgcn_sched_barrier(0);
        stage = stage == NSTAGE - 1 ? 0 : stage + 1;
        if (--left == 0) { pend = true; done_tile = tile; tile += G; if (tile < ntiles) left = p.ph_ntaps[tile_phase(tile)] * kchunks; }
    }
    if (pend) epilogue(done_tile);
    if (!grpY) __builtin_amdgcn_s_barrier();             // 2S
}

constexpr int kGatherLds = 3 * (128 * 128 + 256 * 128);
constexpr int halo_lds(int TH, int TW) { return 4 * 128 * 128 + 2 * (((TH + 2) * (TW + 2) + 7) / 8) * 1024 + 2 * 3072; }
constexpr int k64_lds(int BC, int BP, int NSTAGE) { return NSTAGE * (BC * 128 + BP * 128); }
static_assert(kGatherLds <= 160 * 1024 && halo_lds(8, 32) <= 160 * 1024 && halo_lds(16, 16) <= 160 * 1024 && k64_lds(256, 256, 2) <= 160 * 1024
              && k64_lds(128, 256, 3) <= 160 * 1024, "LDS budget");

template <class MF>
static int launch_leaf(const ConvLaunch& l, hipStream_t stream)
{
    if (l.family == CONV_GATHER) return conv_launch<conv_gather_ld_kernel<MF>>(l, stream, l.x_bytes, l.w_bytes);
    if (l.family == CONV_HALO)
        return l.bc == 8 ? conv_launch<conv_halo_ld_kernel<MF, 8, 32>>(l, stream, l.x_bytes, l.w_bytes)
                         : conv_launch<conv_halo_ld_kernel<MF, 16, 16>>(l, stream, l.x_bytes, l.w_bytes);
    if (l.bc == 64)  return conv_launch<conv_k64_kernel<MF, 64, 256, 1, 8>>(l, stream, l.x_bytes, l.w_bytes);
    if (l.bp == 128) return conv_launch<conv_k64_kernel<MF, 128, 128, 2, 4>>(l, stream, l.x_bytes, l.w_bytes);
    if (l.bc == 256) return conv_launch<conv_k64_kernel<MF, 256, 256, 2, 4, 2>>(l, stream, l.x_bytes, l.w_bytes);
    return conv_launch<conv_k64_kernel<MF, 128, 256, 2, 4>>(l, stream, l.x_bytes, l.w_bytes);
}

// persistent kernels: one workgroup per CU, each walks tiles b, b + grid, ...  (More tiles than an int counts stay as they are: the launch refuses them.)
static int64_t persistent_grid(int64_t tiles) { return tiles <= INT32_MAX && tiles > sbg_cu_count() ? sbg_cu_count() : tiles; }

static void fit_gather(ConvLaunch& l)
{
    ConvArgs& a = l.a;
    a.ctiles = (a.Cout + 127) / 128;
    if (a.nphase <= 1) {            // the whole launch as one phase
        a.nphase = 1; a.ph_tap0[0] = 0; a.ph_ntaps[0] = a.ntaps; a.ph_OH[0] = a.OH; a.ph_OW[0] = a.OW; a.ph_P[0] = a.P; a.ph_yoff[0] = 0;
    }
    int pmax = 0;
    for (int i = 0; i < a.nphase; i++) if (a.ph_P[i] > pmax) pmax = a.ph_P[i];
    a.ptiles = ((pmax + 255) / 256) * a.nphase;      // every phase gets the pixel tiles of the largest one (the others' last tile may be empty)
    l.family = CONV_GATHER; l.bc = 128; l.bp = 256;
    l.grid_x = persistent_grid((int64_t)a.ptiles * a.ctiles); l.grid_y = 1; l.block = 768; l.lds = kGatherLds;
    a.ph_rot_div = (int)(l.grid_x / ((int64_t)a.ctiles * a.nphase)); if (a.ph_rot_div < 1) a.ph_rot_div = 1;
    conv_prof_phases(l, 4128256 + (a.nphase > 1 ? 1000000 * a.nphase : 0));
}

static void fit_halo(ConvLaunch& l, int TH, int TW)
{
    ConvArgs& a = l.a;
    {   // the epilogue parameters go through LDS when the epilogue's 16-B fast path applies and the noise rows are 16-B aligned
        const bool plain = conv_is_plain(a);
        const bool fast = ((a.Cout & 7) == 0) && ((((uintptr_t)a.y) & 15) == 0) && (((a.ys_n | a.ys_h | a.ys_w) & 7) == 0)
                          && ((((uintptr_t)a.oscale) & 15) == 0) && ((((uintptr_t)a.bias) & 15) == 0) && a.ydtype != SBG_F16;
        const bool nz_ok = !a.noise || (((((uintptr_t)a.noise) & 15) == 0) && (a.noise_sn & 3) == 0 && (a.OW & 3) == 0
                                        && (int64_t)a.N * (a.noise_sn > 0 ? a.noise_sn : 0) + (int64_t)a.OH * a.OW < (1ll << 28));
        a.lds_params = !plain && fast && nz_ok && (int64_t)a.N * a.Cout < (1ll << 28);
    }
    a.ctiles = (a.Cout + 127) / 128;
    a.ptiles = a.N * (a.OH / TH) * (a.OW / TW);
    l.family = CONV_HALO; l.bc = TH; l.bp = TW;
    l.grid_x = persistent_grid((int64_t)a.ptiles * a.ctiles); l.grid_y = 1; l.block = 768; l.lds = halo_lds(TH, TW);      // (the LDS footprint admits one workgroup per CU)
    conv_prof_phases(l, 3128256);
}

static void fit_tile(ConvLaunch& l, int BC, int BP, int NSTAGE = 3)
{
    ConvArgs& a = l.a;
    a.ctiles = (a.Cout + BC - 1) / BC;
    a.ptiles = (a.P + BP - 1) / BP;
    l.family = CONV_K64; l.bc = BC; l.bp = BP;
    l.grid_x = (int64_t)a.ptiles * a.ctiles; l.grid_y = (unsigned)(a.ksplit > 1 ? a.ksplit : 1); l.block = 512; l.lds = k64_lds(BC, BP, NSTAGE);
    conv_prof_phases(l, 1000000 + BC * 1000 + BP);
}

// y[i] (+)= sum_k ws[k][i] in a fixed order; 16 lanes share an output element (slabs k, k + 16, ...), then a shuffle tree.
__global__ __launch_bounds__(256) void conv_ksplit_reduce_kernel(const float* ws, float* y, int64_t n, int ksplit, int accumulate)
{
    const int sub = threadIdx.x & 15;
    const int64_t step = (int64_t)gridDim.x * 16;
    for (int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); i < n; i += step) {
        float s = 0.f;
        for (int k = sub; k < ksplit; k += 16) s += ws[(int64_t)k * n + i];
        for (int m = 8; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
        if (sub == 0) y[i] = accumulate ? y[i] + s : s;
    }
}

// Slab reduction with the fused epilogue: y[p][co] = clamp(act(sum_k ws[k][p][co] * oscale[n, co] + noise[n, pixel] + bias[co]) * gain), any output
// dtype, dense channel-minor y.  Lets the few-tile / long-K launches of the 16-bit 4x4 .. 8x8 blocks (16-64 workgroups for 72 K-steps) split K as
// well: 8 channels per lane, 16-B loads per slab.
__global__ __launch_bounds__(256) void conv_ksplit_reduce_epi_kernel(const float* ws, ConvArgs p, int64_t n, int ksplit)
{
    const int64_t groups = n >> 3;                      // n = P * Cout, Cout % 8 == 0
    const int hw = p.OH * p.OW;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        const int64_t i = g << 3;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < ksplit; k++) {
            float v[8];
            Vec8<float>::ld(ws + (int64_t)k * n + i, v);
#pragma unroll
            for (int e = 0; e < 8; e++) acc[e] += v[e];
        }
        const int64_t pix = i / p.Cout; const int co = (int)(i - pix * p.Cout);
        const int img = (int)(pix / hw), pp = (int)(pix - (int64_t)img * hw);
        const float nz = p.noise ? p.noise[(int64_t)img * p.noise_sn + pp] : 0.f;
#pragma unroll
        for (int e = 0; e < 8; e++) acc[e] = tail(p, acc[e], (int64_t)img * p.Cout + co + e, nz + (p.bias ? p.bias[co + e] : 0.f));
        if (p.ydtype == SBG_F32)       Vec8<float>::st((float*)p.y + i, acc);
        else if (p.ydtype == SBG_BF16) Vec8<bf16_s>::st((bf16_s*)p.y + i, acc);
        else                           Vec8<f16_s>::st((f16_s*)p.y + i, acc);
    }
}

} // namespace

// The kernel and tile of a launch, in order of precedence.
void sbg_conv_k64_fit(ConvLaunch& l)
{
    const ConvArgs& a = l.a;
    if (a.nphase > 1) return fit_gather(l);       // multi-phase launches exist only in the persistent gather kernel
    // halo kernel: stride 1, nine taps with |offset| <= 1, output grid == input grid, tile-aligned, enough tiles to fill the chip
    bool halo = a.stride == 1 && a.ntaps == 9 && a.OH == a.IH && a.OW == a.IW;
    for (int t = 0; halo && t < 9; t++) halo = a.tap_dy[t] >= -1 && a.tap_dy[t] <= 1 && a.tap_dx[t] >= -1 && a.tap_dx[t] <= 1;
    const int64_t tiles256 = (int64_t)((a.P + 255) / 256) * ((a.Cout + 127) / 128);
    if (halo && a.Cout > 64 && tiles256 >= 256) {
        if (a.OW % 32 == 0 && a.OH % 8 == 0)  return fit_halo(l, 8, 32);
        if (a.OW % 16 == 0 && a.OH % 16 == 0) return fit_halo(l, 16, 16);
    }
    if (a.Cout <= 64) return fit_tile(l, 64, 256);
    if (a.ksplit > 1) return fit_tile(l, 128, 128);        // the slab reduction follows this launch
    if (tiles256 < 256) return fit_tile(l, 128, 128);
    // short reductions (transposed-conv phases: 1-4 taps) gain from the persistent pipeline; measured: +4..10 % at <= 8 K-steps per tile,
    // -5 % at 18+ (the 8-wave kernel's in-wave DMA issue overlaps better there)
    const int ksteps = a.ntaps * ((a.Cin + 63) >> 6);
    if (ksteps >= 2 && ksteps <= 8) return fit_gather(l);      // 1 step: store-bound, the plain kernel wins
    // 256 x 256 tiles, two stages: 64 DMA pieces per K-step for twice the flops of the 48 below.  Stride-2 launches (D's conv1, the data
    // gradient of G's up-sampling layers) whose 256-channel tiles still give every CU one
    // (the kernel packs a pixel's input row and column into 16 + 16 bits)
    if (a.stride == 2 && a.Cout % 256 == 0 && (a.OH - 1) * 2 + 8 < 32768 && (a.OW - 1) * 2 + 8 < 32768 && (int64_t)((a.P + 255) / 256) * (a.Cout / 256) >= sbg_cu_count())
        return fit_tile(l, 256, 256, 2);
    return fit_tile(l, 128, 256);
}

int sbg_conv_k64_launch(const ConvLaunch& l, bool bf16, hipStream_t stream)
{
    return bf16 ? launch_leaf<bf16_mfma>(l, stream) : launch_leaf<f16_mfma>(l, stream);
}

int sbg_conv_ksplit_reduce(const ConvArgs& call, const void* workspace, int ksplit, bool reduce_epi, hipStream_t stream)
{
    const int64_t y_numel = (int64_t)call.P * call.Cout;
    if (!reduce_epi) {
        unsigned grid = (unsigned)((y_numel + 15) / 16); if (grid > 4096) grid = 4096;
        SBG_LAUNCH(conv_ksplit_reduce_kernel, dim3(grid), dim3(256), 0, stream, (const float*)workspace, (float*)call.y, y_numel, ksplit, call.accumulate);
    } else {
        unsigned grid = (unsigned)((y_numel / 8 + 255) / 256); if (grid > 4096) grid = 4096; if (grid < 1) grid = 1;
        SBG_LAUNCH(conv_ksplit_reduce_epi_kernel, dim3(grid), dim3(256), 0, stream, (const float*)workspace, call, y_numel, ksplit);
    }
    SBG_HIP_LAUNCH_CHECK();
    return SBG_OK;
}
