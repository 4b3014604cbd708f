// stripe_mm.inc -- batches on the stripe16 image: 5 <= M <= 128 rows of x through 16-row MFMA tiles (four schedules, below) and 129 .. 1024 rows
// through a 2-D tiled fused-dequantise GEMM (stripe_gemm_kernel, the end of this file); ONE bit width per translation unit
// (stripe_mm_b4.hip / stripe_mm_b8.hip define STRIPE_BITS).  Same arithmetic as matmul_248_kernel (reference
// quant/quant_linear.py:103-137) / fusedmatmul_248_kernel (quant/fused_mlp.py:128-168) for every M the reference's
// forward accepts (quant_linear.py:415-419); what is new is the schedule:
//
//  * a lane's packed word is the B fragment of v_mfma_f32_16x16x32_f16 (8 consecutive k of one column).  It is unpacked with the
//    fp16 magic-exponent trick (stripe_unpack.inc) and then made EXACT: one v_pk_add_f16 per pair subtracts (OFF + zero + 1), so
//    the matrix core multiplies x by the integer q - z (exact in fp16) and the group scale is applied to the fp32 accumulator
//    once per row block (y += s * acc): no fp16 rounding of weights, no x-sum corrections.  The unpack is paid ONCE per weight
//    and amortised over 16 TM rows (TM = 1..4 MFMA row tiles on the same B fragments);
//  * what bounds M = 16..64 is not HBM but how often x is re-read: a workgroup that owns c columns over a K span re-reads
//    M * span * 2 bytes of x, N M K / (8 c) bytes over the launch whatever the span is.  The first version of this kernel (one
//    stripe, whole K per workgroup, x streamed through LDS in chunks) moved 134 MB of x through L2 at M = 64 on 4096^2 and took
//    16 us.  So: a workgroup = 8 waves = 8 ADJACENT STRIPES (128 columns) x ONE K slice; its x slice [16 TM][span] is loaded into
//    LDS once (rows padded by 16 bytes: the 16-byte A-fragment reads are bank-conflict free) and every wave streams its own
//    stripe's row blocks of the slice, RD = 4 loads (4 KiB) in flight;
//  * the S K slices of a column group meet through fp32 partial tiles and a second, tiny kernel (sum in slice order:
//    bit-reproducible; SiLU pair / bias / rounding in its epilogue), not through per-element atomics.  An in-kernel hand-off
//    (write-through tiles, one counter increment per workgroup, last arriver adds) was measured first: +0.6 us per slice
//    (20 us at S = 16 on 4096^2) -- on this chip a kernel boundary (1.4 us) is the cheaper hand-off.  S = 1 stores straight from
//    the accumulators.  Linear block id = slice + S * group: the workgroups of one XCD (id % 8) read the same x slices.
//  * up to 32 rows on shapes that are ONE round of stripes over the 256 CUs keep a single launch instead (stripe_mm1_kernel /
//    stripe_mm2_kernel below: a stripe x whole K per workgroup, x streamed through LDS).  Their bound is what one CU pulls from
//    L2: ~45-50 GB/s (~1 KiB per 60-80 cycles) whether the bytes return to registers or land in LDS by DMA -- both are built.
// Eligibility: bits 4 / 8, group size a multiple of the row block (BK = 128 / 64 k) or one group.  Dispatch: the end of this file.

#include "gptq_device.h"
#include "gptq_internal.h"
#include "stripe_common.h"

namespace gptq {

namespace {

#include "stripe_unpack.inc"

typedef _Float16 mm_h8_t __attribute__((ext_vector_type(8)));

constexpr int MM_RD = 4;   // weight row blocks in flight per wave

struct MMArgs {
    const half_t *x;
    const uint32_t *R, *tab;
    half_t *y;
    const half_t *bias;   // ldb == 0: [N], added to every row; ldb != 0: a residual [M][ldb] (batched decode engine, round 5)
    float *partials;      // [groups][S][8 waves][NS][TM][64 lanes][4]
    int K, nrb, G, grp_shift, M, ldx, ldy, nstripes, S, span;
    int gq_shift;   // log2(groupsize / LK) (PS kernels: the group of a LANE block), -1 = one group
    int ldb;
    int MT;         // K slices of the 128-row tile GEMM over SEVERAL row tiles (round 5): row tiles of the launch; 0 / 1 = one
    int rowmajor;   // round 6 (one row tile, one set): the slices' partials as [S][16][N] fp32 rows -- the combine launch owns whole rows (slices_combine_norm_launch)
};

// -OFF of every offset class (stripe_unpack.inc), both halves: built once per kernel, ahead of the K loop
GPTQ_DEV void neg_offsets(half2_t (&negoff)[NOFFC]) {
#pragma unroll
    for (int o = 0; o < NOFFC; o++) negoff[o] = half2_t{(half_t)(-class_off(o)), (half_t)(-class_off(o))};
}

// THE dequantiser of this file: a lane's share of one row block (WPL packed words) -> its PPB B fragments of v_mfma_f32_16x16x32_f16, the exact
// integers q - z: one v_pk_add_f16 per pair subtracts OFF + zero + 1 (cz = negoff - zz, exact).  Returns the fp32 group scale of the table word
// {scale, zero + 1} for the accumulator, zero when !valid (a clamped re-read past K or past the slice).  (The prescale form -- every pair times the
// lane block's fp16 scale -- exists only at the hand-written sites of stripe_mm_kernel and stripe_gemm_kernel, see the note above mm_epilogue.)
template <typename WV>
GPTQ_DEV float dequant_block(const WV &w, uint32_t table_word, bool valid, const half2_t (&negoff)[NOFFC], const UnpackConsts &uc, mm_h8_t (&B)[PPB]) {
    const half2_t e = as_half2(table_word);
    const half2_t zz = {e[1], e[1]};
    half2_t cz[NOFFC];
#pragma unroll
    for (int o = 0; o < NOFFC; o++) cz[o] = negoff[o] - zz;   // -(OFF + zero + 1), exact
    uint32_t t[NPB], d[NPB];
    unpack_block(w, uc, t);
#pragma unroll
    for (int q = 0; q < NPB; q++) d[q] = as_u32(as_half2(t[q]) + cz[off_class(q)]);   // q - z, exact
#pragma unroll
    for (int b = 0; b < PPB; b++) B[b] = __builtin_bit_cast(mm_h8_t, u32x4{d[4 * b], d[4 * b + 1], d[4 * b + 2], d[4 * b + 3]});
    return valid ? (float)e[0] : 0.f;
}

// THE output epilogue of this file: one row tile of one stripe.  lane = column n = 16 stripe + col; rows row0 + 4 rq + r of the tile's fp32 sums
// (a float4 per weight set) -> SiLU(gate) * up for a pair -> fp16 -> + bias (ldb == 0) or + the residual row (ldb != 0) on the ROUNDED value
// -> y, rows below M only.
template <int NS>
GPTQ_DEV void finish_tile(const float4_t (&tot)[NS], const MMArgs &a, int stripe, int row0, int rq, int col) {
    const int n = stripe * 16 + col;
    const float bv = (a.bias && !a.ldb) ? (float)a.bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = row0 + 4 * rq + r;
        float v = tot[0][r];
        if constexpr (NS == 2) v = v * (1.0f / (1.0f + __expf(-v))) * tot[1][r];   // silu on the fp32 accumulator (fused_mlp.py:160-164)
        if (row < a.M) {
            half_t h = (half_t)v;
            if (a.bias) h = (half_t)((float)h + (a.ldb ? (float)a.bias[(size_t)row * a.ldb + n] : bv));
            a.y[(size_t)row * a.ldy + n] = h;
        }
    }
}

// Three kernels keep their HAND-WRITTEN dequantiser and epilogue, the text of dequant_block / finish_tile written out at the site: stripe_mm_kernel
// (with mm_epilogue, below), stripe_mm2_kernel and stripe_gemm_kernel.  Through the functions the compiler gave their K loops another schedule -- more
// waits in most instances, six v_perm_b32 in the 256-row tile GEMM, the occupancy line of seven kernels moved
// (profiles/stripe_dequant_once/README.md) -- and the rule of this file is that such a kernel keeps its site.  A change to the dequantiser or
// the epilogue is made in dequant_block / finish_tile AND at these three sites.

// the TM row tiles a wave of stripe_mm_kernel holds for one stripe: lane = column, rows 16 t + 4 rq + r (hand-written, see above)
template <int TM, int NS>
GPTQ_DEV void mm_epilogue(const float4_t (&yacc)[NS][TM], const MMArgs &a, int stripe, bool has, int rq, int col) {
    if (!has) return;
    const int n = stripe * 16 + col;
    const float bv = (a.bias && !a.ldb) ? (float)a.bias[n] : 0.f;
#pragma unroll
    for (int t = 0; t < TM; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = 16 * t + 4 * rq + r;
            float v = yacc[0][t][r];
            if constexpr (NS == 2) v = v * (1.0f / (1.0f + __expf(-v))) * yacc[1][t][r];   // silu on the fp32 accumulator (fused_mlp.py:160-164)
            if (row < a.M) {
                half_t h = (half_t)v;
                if (a.bias) h = (half_t)((float)h + (a.ldb ? (float)a.bias[(size_t)row * a.ldb + n] : bv));
                a.y[(size_t)row * a.ldy + n] = h;
            }
        }
}

// grp_shift = log2(groupsize / BK), -1 for one group; span = row blocks per K slice.
// PS ("prescale"): the group is smaller than a row block (or the width is 2-bit at g128: BK = 256), so the MFMA would sum across
// groups -- each lane multiplies its exact q - z by its own group's fp16 scale first (one rounding, the reference's own dequantisation,
// quant_linear.py:128) and the accumulator needs no per-row-block scale.  Any width with a stripe image runs here (2 / 3 / 4 / 8 bits).
template <int TM, int NS, bool PS>
__global__ void __launch_bounds__(STRIPE_NW * 64) stripe_mm_kernel(const MMArgs a) {
    typedef uint32_t wvec_t __attribute__((ext_vector_type(WPL)));
    constexpr int NW = STRIPE_NW, RD = MM_RD, ROWS = 16 * TM, RPW = ROWS / NW;   // RPW rows of x per wave while staging
    constexpr int TILE = NS * TM * 256;                                          // floats of one wave's accumulators (per stripe)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    half_t *xl = (half_t *)smem;   // [ROWS][XS]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = a.S, group = blockIdx.x / S, slice = blockIdx.x % S;
    const int rb0 = slice * a.span, rb1 = min(a.nrb, rb0 + a.span);
    const int kspan = a.span * BK, XS = kspan + 8, ppr = kspan / 8;
    const int rq = lane >> 4, col = lane & 15;
    const UnpackConsts uc = unpack_consts();

    // ---- the first RD row blocks of this wave's stripes (HBM: the longest latency goes first), then the x slice ----
    wvec_t w[RD][NS];
    uint32_t tw[RD][NS];
    const int stripe = group * NW + wave, sc = min(stripe, a.nstripes - 1);
    const uint32_t *wbase = a.R + ((size_t)sc * a.nrb * NS * 64 + lane) * WPL;
    const uint32_t *tbase = a.tab + (size_t)sc * NS * a.G * 16 + col;
    auto issue = [&](int slot, int u) {
        const int rb = min(rb0 + u, a.nrb - 1);   // past the slice: a valid address, the scale is zeroed below
        const int g = PS ? ((rb * 4 + rq) >> a.gq_shift) : (a.grp_shift >= 0 ? (rb >> a.grp_shift) : 0);
#pragma unroll
        for (int s = 0; s < NS; s++) {
            w[slot][s] = __builtin_nontemporal_load((const wvec_t *)(wbase + ((size_t)rb * NS + s) * (64 * WPL)));
            tw[slot][s] = tbase[((size_t)s * a.G + g) * 16];
        }
    };
#pragma unroll
    for (int u = 0; u < RD; u++) issue(u, u);
    __builtin_amdgcn_sched_barrier(0);
    {
        const half_t *xs = a.x + (size_t)rb0 * BK;
        for (int j0 = 0; j0 < ppr; j0 += 64) {
            const int pc = j0 + lane;
            const int k = min(pc * 8, a.K - 8 - rb0 * BK);   // ragged last slice: stay inside the row
            u32x4 v[RPW];
#pragma unroll
            for (int r = 0; r < RPW; r++) v[r] = *(const u32x4 *)(xs + (size_t)min(wave + NW * r, a.M - 1) * a.ldx + k);
            if (pc < ppr) {
#pragma unroll
                for (int r = 0; r < RPW; r++) *(u32x4 *)(xl + (size_t)(wave + NW * r) * XS + pc * 8) = v[r];
            }
        }
    }
    __syncthreads();

    float4_t yacc[NS][TM];
#pragma unroll
    for (int s = 0; s < NS; s++)
#pragma unroll
        for (int t = 0; t < TM; t++) yacc[s][t] = float4_t{0.f, 0.f, 0.f, 0.f};
    half2_t negoff[NOFFC];
#pragma unroll
    for (int o = 0; o < NOFFC; o++) negoff[o] = half2_t{(half_t)(-class_off(o)), (half_t)(-class_off(o))};

    auto step = [&](int i, int u, bool refill) {
        const bool valid = rb0 + u < rb1;
        const int kk = u * BK + LK * rq;   // this lane's k block inside the slice
        mm_h8_t B[NS][PPB];
        float scale[NS];
#pragma unroll
        for (int s = 0; s < NS; s++) {      // (hand-written dequant_block, with the prescale: see the note above mm_epilogue)
            const half2_t e = as_half2(tw[i][s]);
            scale[s] = valid ? (float)e[0] : 0.f;
            const half2_t zz = {e[1], e[1]};
            const half2_t s2 = valid ? half2_t{e[0], e[0]} : half2_t{(half_t)0.f, (half_t)0.f};
            half2_t cz[NOFFC];
#pragma unroll
            for (int o = 0; o < NOFFC; o++) cz[o] = negoff[o] - zz;   // -(OFF + zero + 1), exact
            uint32_t t[NPB], d[NPB];
            unpack_block(w[i][s], uc, t);
#pragma unroll
            for (int q = 0; q < NPB; q++) {
                half2_t v = as_half2(t[q]) + cz[off_class(q)];          // q - z, exact
                if constexpr (PS) v = v * s2;                              // ... times the lane block's own scale: one fp16 rounding
                d[q] = as_u32(v);
            }
#pragma unroll
            for (int b = 0; b < PPB; b++) B[s][b] = __builtin_bit_cast(mm_h8_t, u32x4{d[4 * b], d[4 * b + 1], d[4 * b + 2], d[4 * b + 3]});
        }
        if (refill) {
            issue(i, u + RD);   // the slot's words are unpacked: refill it before the math
            __builtin_amdgcn_sched_barrier(0);
        }
        const int kc = valid ? kk : LK * rq;   // past the slice: read inside the staged rows
        float4_t acc[NS][TM];
#pragma unroll
        for (int s = 0; s < NS; s++)
#pragma unroll
            for (int t = 0; t < TM; t++) acc[s][t] = PS ? yacc[s][t] : float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < PPB; b++) {
#pragma unroll
            for (int t = 0; t < TM; t++) {
                const mm_h8_t A = *(const mm_h8_t *)(xl + (size_t)(16 * t + col) * XS + kc + 8 * b);
#pragma unroll
                for (int s = 0; s < NS; s++) acc[s][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A, B[s][b], acc[s][t], 0, 0, 0);
            }
        }
#pragma unroll
        for (int s = 0; s < NS; s++)
#pragma unroll
            for (int t = 0; t < TM; t++) {
                if constexpr (PS) {
                    yacc[s][t] = acc[s][t];
                } else {
#pragma unroll
                    for (int r = 0; r < 4; r++) yacc[s][t][r] = fmaf(scale[s], acc[s][t][r], yacc[s][t][r]);
                }
            }
    };
    int u0 = 0;
    for (; u0 + RD < a.span; u0 += RD) {   // rounds that refill their slots
#pragma unroll
        for (int i = 0; i < RD; i++) step(i, u0 + i, true);
    }
#pragma unroll
    for (int i = 0; i < RD; i++) step(i, u0 + i, false);   // the last round (blocks past the slice carry a zero scale)

    if constexpr (TM == 1 && NS == 1) {
        if (S > 1 && a.rowmajor) {   // rows for the combine + norm launch: [slice][16][N], 64-byte runs per row and stripe
            if (stripe < a.nstripes) {
                float *pr = a.partials + ((size_t)slice * 16 + 4 * rq) * ((size_t)a.nstripes * 16) + (size_t)stripe * 16 + col;
#pragma unroll
                for (int r = 0; r < 4; r++) pr[(size_t)r * a.nstripes * 16] = yacc[0][0][r];
            }
            return;
        }
    }
    if (S > 1) {
        // ---- K slices meet in the reduce kernel: this wave's fp32 tile, [64 lanes][4] per (set, row tile): 1 KiB stores ----
        float *mine = a.partials + (((size_t)group * S + slice) * NW + wave) * TILE + lane * 4;
#pragma unroll
        for (int s = 0; s < NS; s++)
#pragma unroll
            for (int t = 0; t < TM; t++) *(float4_t *)(mine + (s * TM + t) * 256) = yacc[s][t];
    } else {
        mm_epilogue<TM, NS>(yacc, a, stripe, stripe < a.nstripes, rq, col);
    }
}

// slices -> y: one thread per (column group, stripe, lane), all S loads of a row tile in flight; slice order = bit-reproducible
template <int TM, int NS>
__global__ void __launch_bounds__(STRIPE_NW * 64) stripe_mm_reduce_kernel(const MMArgs a) {
    constexpr int NW = STRIPE_NW, TILE = NS * TM * 256;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // (a.MT > 1, round 5: the tile GEMM's slices over several 128-row tiles -- block group gm = row tile * groups + group, rows offset by 16 TM per tile)
    const int gm = blockIdx.x / TM, t = blockIdx.x % TM, S = a.S;
    const int ngr = (a.nstripes + NW - 1) / NW;
    const int group = a.MT > 1 ? gm % ngr : gm, row0 = a.MT > 1 ? (gm / ngr) * 16 * TM : 0;
    const int stripe = group * NW + wave;
    const float *first = a.partials + (((size_t)gm * S) * NW + wave) * TILE + t * 256 + lane * 4;
    float4_t acc[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) acc[s] = float4_t{0.f, 0.f, 0.f, 0.f};
    for (int sl0 = 0; sl0 < S; sl0 += 8) {
        float4_t v[8][NS];
#pragma unroll
        for (int q = 0; q < 8; q++)
#pragma unroll
            for (int s = 0; s < NS; s++) v[q][s] = *(const float4_t *)(first + (size_t)min(sl0 + q, S - 1) * NW * TILE + s * TM * 256);
#pragma unroll
        for (int q = 0; q < 8; q++)
            if (sl0 + q < S) {
#pragma unroll
                for (int s = 0; s < NS; s++) acc[s] += v[q][s];
            }
    }
    if (stripe >= a.nstripes) return;
    finish_tile<NS>(acc, a, stripe, row0 + 16 * t, lane >> 4, lane & 15);
}

// ---- single-launch variant: one stripe (16 columns) x WHOLE K per workgroup, x streamed through LDS ----
// No cross-workgroup combine at all (a second launch costs ~3 us, more than the whole budget at M <= 16).  The price is that every
// workgroup reads all of x (M K 2 bytes through L2 -> LDS), so the x path is pipelined as deep as the registers allow: chunks of
// 32 KB (ROWS x CK k, CK = NRB row blocks), PF = 2 chunks requested ahead into registers (PF = 4 costs 32 more VGPRs and the second
// workgroup per CU: 6.3 instead of 5.9 us at M = 16 on 4096^2, 15.8 instead of 12.0 at N = 12288), two LDS buffers, ONE barrier per chunk.
// The eight waves are NRB (k) x TG (row tiles): TM = 1: 8 x 1, TM = 2: 4 x 2, TM = 3 / 4: 2 x 4 -- every wave unpacks one row
// block per chunk (waves of different row tiles unpack the same block: VALU is idle anyway) and runs ONE row tile on the matrix core.
// PF = chunks of x requested ahead in registers: 4 (64 VGPRs, one workgroup per CU) or 2 (two workgroups per CU: shapes with more than one
// round of stripes over the CUs)
template <int TM, int NS, int PF>
__global__ void __launch_bounds__(STRIPE_NW * 64, PF == 2 ? 4 : 1) stripe_mm1_kernel(const MMArgs a) {
    constexpr int NW = STRIPE_NW, T = NW * 64, TG = TM == 1 ? 1 : (TM == 2 ? 2 : 4), NRB = NW / TG;
    constexpr int ROWS = 16 * TM, CK = NRB * BK, XS = CK + 8, CP = CK / 8, NPC = ROWS * CP, XPF = (NPC + T - 1) / T;
    constexpr int RD = 4, BUF = ROWS * XS;   // halves per LDS buffer
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    half_t *xl = (half_t *)smem;   // [2][ROWS][XS]; reused for the output partials
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kb = wave % NRB, tg = wave / NRB;
    const int stripe = blockIdx.x;
    const int rq = lane >> 4, col = lane & 15;
    const UnpackConsts uc = unpack_consts();
    const int nchunk = (a.nrb + NRB - 1) / NRB;

    u32x4 xpf[PF][XPF];
    auto xload = [&](int slot, int c) {
#pragma unroll
        for (int q = 0; q < XPF; q++) {
            const int p = min(tid + q * T, NPC - 1), row = min(p / CP, a.M - 1), k = min(c * CK + (p % CP) * 8, a.K - 8);
            xpf[slot][q] = *(const u32x4 *)(a.x + (size_t)row * a.ldx + k);
        }
    };
    auto xstore = [&](int slot, int buf) {
#pragma unroll
        for (int q = 0; q < XPF; q++) {
            const int p = tid + q * T;
            if (NPC % T == 0 || p < NPC) *(u32x4 *)(xl + buf * BUF + (p / CP) * XS + (p % CP) * 8) = xpf[slot][q];
        }
    };
    u32x4 w[RD][NS];
    uint32_t tw[RD][NS];
    const uint32_t *wbase = a.R + ((size_t)stripe * a.nrb * NS * 64 + lane) * 4;
    const uint32_t *tbase = a.tab + (size_t)stripe * NS * a.G * 16 + col;
    auto issue = [&](int slot, int c) {
        const int rb = min(c * NRB + kb, a.nrb - 1);
        const int g = a.grp_shift >= 0 ? (rb >> a.grp_shift) : 0;
#pragma unroll
        for (int s = 0; s < NS; s++) {
            if constexpr (TG == 1) w[slot][s] = __builtin_nontemporal_load((const u32x4 *)(wbase + ((size_t)rb * NS + s) * 256));
            else w[slot][s] = *(const u32x4 *)(wbase + ((size_t)rb * NS + s) * 256);   // TG waves read the same block: keep it cacheable
            tw[slot][s] = tbase[((size_t)s * a.G + g) * 16];
        }
    };
    // request order = consumption order: chunk 0 of x, block 0, chunk 1, block 1, ...
#pragma unroll
    for (int i = 0; i < RD; i++) {
        if (i < PF) xload(i, i);
        issue(i, i);
    }
    __builtin_amdgcn_sched_barrier(0);

    float4_t yacc[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) yacc[s] = float4_t{0.f, 0.f, 0.f, 0.f};
    half2_t negoff[NOFFC];
    neg_offsets(negoff);

    for (int c0 = 0; c0 < nchunk; c0 += RD) {
#pragma unroll
        for (int i = 0; i < RD; i++) {
            const int c = c0 + i, buf = i & 1;
            xstore(i % PF, buf);
            if (c + PF < nchunk) xload(i % PF, c + PF);   // wave-uniform
            __syncthreads();                         // chunk c is in LDS; everyone is done with chunk c - 1 (the other buffer)
            const bool valid = c * NRB + kb < a.nrb && tg < TM;
            mm_h8_t B[NS][PPB];
            float scale[NS];
#pragma unroll
            for (int s = 0; s < NS; s++) scale[s] = dequant_block(w[i][s], tw[i][s], valid, negoff, uc, B[s]);
            if (c + RD < nchunk) issue(i, c + RD);   // wave-uniform
            const half_t *xa = xl + buf * BUF + (16 * min(tg, TM - 1) + col) * XS + kb * BK + LK * rq;
            float4_t acc[NS];
#pragma unroll
            for (int s = 0; s < NS; s++) acc[s] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int b = 0; b < PPB; b++) {
                const mm_h8_t A = *(const mm_h8_t *)(xa + 8 * b);
#pragma unroll
                for (int s = 0; s < NS; s++) acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A, B[s][b], acc[s], 0, 0, 0);
            }
#pragma unroll
            for (int s = 0; s < NS; s++)
#pragma unroll
                for (int r = 0; r < 4; r++) yacc[s][r] = fmaf(scale[s], acc[s][r], yacc[s][r]);
        }
    }

    // ---- NRB k-waves of a row tile -> 1 through LDS ([wave][set][lane] float4: conflict-free), epilogue ----
    __syncthreads();
    float4_t *red = (float4_t *)smem;
#pragma unroll
    for (int s = 0; s < NS; s++) red[(wave * NS + s) * 64 + lane] = yacc[s];
    __syncthreads();
    if (kb == 0 && tg < TM) {
        float4_t tot[NS];
#pragma unroll
        for (int s = 0; s < NS; s++) {
            tot[s] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k2 = 0; k2 < NRB; k2++) tot[s] += red[((tg * NRB + k2) * NS + s) * 64 + lane];
        }
        finish_tile<NS>(tot, a, stripe, 16 * tg, rq, col);
    }
}

template <int TM, int NS, int PF = 4>
int stripe_mm1_launch(const StripeParams &p, int grp_shift, hipStream_t s) {
    auto kern = stripe_mm1_kernel<TM, NS, PF>;
    constexpr int TG = TM == 1 ? 1 : (TM == 2 ? 2 : 4), NRB = STRIPE_NW / TG;
    const size_t lds = (size_t)2 * 16 * TM * (NRB * BK + 8) * 2;
    static LdsOptIn opt_in;   // per instantiation; per device inside
    if (int rc = opt_in.ensure((const void *)kern, lds)) return rc;
    MMArgs a{};
    a.x = p.x; a.R = p.R; a.tab = p.tab; a.y = p.y; a.bias = p.bias; a.ldb = (int)p.ldb;
    a.K = p.K; a.nrb = p.K / BK; a.G = p.G; a.grp_shift = grp_shift; a.M = p.M; a.ldx = (int)p.ldx; a.ldy = (int)p.ldy;
    a.nstripes = p.N / 16; a.S = 1; a.span = a.nrb;
    hipLaunchKernelGGL(kern, dim3(p.N / 16), dim3(STRIPE_NW * 64), lds, s, a);
    return (int)hipGetLastError();
}

// ---- single-launch variant, all loads as LDS-DMA (global_load_lds_dwordx4): x AND weights AND the table land in LDS without
// passing through registers, three stages deep, counted vmcnt + raw s_barrier (a __syncthreads would drain the DMA queue).  The x
// image of a stage is lane-linear per 1 KiB DMA and XOR-swizzled on the SOURCE side (piece kp of row r sits at kp ^ (r & 15)), so the
// 16-byte A-fragment reads of 16 rows hit 16 different bank groups; a weight row block is lane-linear as stored (a lane reads back
// its own 16 bytes).  Waves = NRB (k) x TG (row tiles) as above; with TG > 1 the row block is fetched ONCE and unpacked by TG waves.
template <int TM, int NS>
__global__ void __launch_bounds__(STRIPE_NW * 64) stripe_mm2_kernel(const MMArgs a) {
    constexpr int NW = STRIPE_NW, TG = TM == 1 ? 1 : (TM == 2 ? 2 : 4), NRB = NW / TG;
    constexpr int ROWS = 16 * TM, CK = NRB * BK, CP = CK / 8, NPC = ROWS * CP;   // 16-byte pieces of x per stage
    constexpr int XG = (NPC / 64 + NW - 1) / NW;                                 // x DMAs per wave and stage (1 KiB each)
    constexpr int XBYTES = XG * NW * 1024, STAGE = XBYTES + NRB * NS * 1024, NSTG = 3;
    constexpr int NOFF = SB == 8 ? 1 : 2;
    typedef const __attribute__((address_space(1))) void *gptr_t;
    typedef __attribute__((address_space(3))) void *lptr_t;
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
    uint32_t *tabl = (uint32_t *)(smem + NSTG * STAGE);   // [NS][G][16] half2 {scale, zero + 1}
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kb = wave % NRB, tg = wave / NRB;
    const bool wloader = wave < NRB;   // tg == 0
    const int stripe = blockIdx.x;
    const int rq = lane >> 4, col = lane & 15;
    const UnpackConsts uc = unpack_consts();
    const int nchunk = (a.nrb + NRB - 1) / NRB;

    // table: 256-byte DMAs (4 bytes per lane), FIRST in the queue: they retire before stage 0
    {
        const uint32_t *tsrc = a.tab + (size_t)stripe * NS * a.G * 16;
        const int ntp = (NS * a.G * 16 + 63) / 64;
        for (int i = wave; i < ntp; i += NW)
            __builtin_amdgcn_global_load_lds((gptr_t)(tsrc + min(i * 64 + lane, NS * a.G * 16 - 1)), (lptr_t)(tabl + i * 64), 4, 0, 0);
    }
    // per-lane source of this wave's x pieces (chunk 0): LDS piece P = (wave XG + q) 64 + lane holds row P / CP, piece (P % CP) ^ (row & 15)
    uint32_t xoff[XG];
#pragma unroll
    for (int q = 0; q < XG; q++) {
        const int P = min((wave * XG + q) * 64 + lane, NPC - 1), row = P / CP, kp = (P % CP) ^ (row & 15);
        xoff[q] = (uint32_t)(min(row, a.M - 1) * a.ldx + kp * 8);
    }
    const uint32_t *wsrc = a.R + ((size_t)stripe * a.nrb * NS * 64 + lane) * 4;
    auto dma = [&](int stage, int c) {
        unsigned char *base = smem + stage * STAGE;
        const int kmax = a.K - 8 - c * CK;   // ragged last chunk: stay inside the row (those blocks carry a zero scale)
#pragma unroll
        for (int q = 0; q < XG; q++) {
            const half_t *src = a.x + (size_t)xoff[q] + (size_t)c * CK;
            if (kmax < CK - 8) {   // wave-uniform: only the last chunk of a ragged K
                const int P = min((wave * XG + q) * 64 + lane, NPC - 1), row = P / CP, kp = (P % CP) ^ (row & 15);
                src = a.x + (size_t)min(row, a.M - 1) * a.ldx + (size_t)c * CK + min(kp * 8, kmax);
            }
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(base + (wave * XG + q) * 1024), 16, 0, 0);
        }
        if (wloader) {
            const int rb = min(c * NRB + kb, a.nrb - 1);
#pragma unroll
            for (int s = 0; s < NS; s++)
                __builtin_amdgcn_global_load_lds((gptr_t)(wsrc + ((size_t)rb * NS + s) * 256), (lptr_t)(base + XBYTES + (kb * NS + s) * 1024), 16, 0, 2);
        }
    };
    auto wait_one_stage_in_flight = [&]() {   // everything but the most recent stage of THIS wave has landed
        if (wloader) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(XG + NS) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(XG) : "memory");
    };
    dma(0, 0);
    dma(1, min(1, nchunk - 1));
    wait_one_stage_in_flight();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);

    float4_t yacc[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) yacc[s] = float4_t{0.f, 0.f, 0.f, 0.f};
    half2_t negoff[NOFF];
#pragma unroll
    for (int o = 0; o < NOFF; o++) negoff[o] = half2_t{(half_t)(-pair_off(o)), (half_t)(-pair_off(o))};
    const int tile = min(tg, TM - 1);

    for (int c = 0; c < nchunk; c++) {
        dma((c + 2) % NSTG, min(c + 2, nchunk - 1));   // that stage was last read in iteration c - 1 (every wave has passed its barrier)
        __builtin_amdgcn_sched_barrier(0);
        const unsigned char *st = smem + (c % NSTG) * STAGE;
        const int rb = c * NRB + kb;
        const bool valid = rb < a.nrb && tg < TM;
        const int g = a.grp_shift >= 0 ? (min(rb, a.nrb - 1) >> a.grp_shift) : 0;
        mm_h8_t B[NS][PPB];
        float scale[NS];
#pragma unroll
        for (int s = 0; s < NS; s++) {
            const u32x4 wv = *(const u32x4 *)(st + XBYTES + (kb * NS + s) * 1024 + lane * 16);
            // (hand-written, in the WORD form this kernel was built in: see the note above mm_epilogue.  4 and 8 bits only -- WPL == 4, the class of pair q of a word is q & 1)
            const half2_t e = as_half2(tabl[(s * a.G + g) * 16 + col]);
            scale[s] = valid ? (float)e[0] : 0.f;
            const half2_t zz = {e[1], e[1]};
            half2_t cz[NOFF];
#pragma unroll
            for (int o = 0; o < NOFF; o++) cz[o] = negoff[o] - zz;
            uint32_t d[4 * NPAIR];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t t[NPAIR];
                unpack_word(wv[j], uc, t);
#pragma unroll
                for (int q = 0; q < NPAIR; q++) d[j * NPAIR + q] = as_u32(as_half2(t[q]) + cz[SB == 8 ? 0 : (q & 1)]);
            }
#pragma unroll
            for (int b = 0; b < PPB; b++) B[s][b] = __builtin_bit_cast(mm_h8_t, u32x4{d[4 * b], d[4 * b + 1], d[4 * b + 2], d[4 * b + 3]});
        }
        const unsigned char *xrow = st + (16 * tile + col) * (CK * 2);
        const int kp0 = (kb * BK + LK * rq) / 8;
        float4_t acc[NS];
#pragma unroll
        for (int s = 0; s < NS; s++) acc[s] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < PPB; b++) {
            const mm_h8_t A = *(const mm_h8_t *)(xrow + ((kp0 + b) ^ col) * 16);
#pragma unroll
            for (int s = 0; s < NS; s++) acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A, B[s][b], acc[s], 0, 0, 0);
        }
#pragma unroll
        for (int s = 0; s < NS; s++)
#pragma unroll
            for (int r = 0; r < 4; r++) yacc[s][r] = fmaf(scale[s], acc[s][r], yacc[s][r]);
        // stage c + 1 (requested one iteration ago) must have landed; stage c + 2 may stay in flight
        wait_one_stage_in_flight();
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // ---- NRB k-waves of a row tile -> 1 through LDS, epilogue ----
    float4_t *red = (float4_t *)smem;
#pragma unroll
    for (int s = 0; s < NS; s++) red[(wave * NS + s) * 64 + lane] = yacc[s];
    __syncthreads();
    if (kb == 0 && tg < TM) {
        float4_t tot[NS];
#pragma unroll
        for (int s = 0; s < NS; s++) {
            tot[s] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k2 = 0; k2 < NRB; k2++) tot[s] += red[((tg * NRB + k2) * NS + s) * 64 + lane];
        }
        const int n = stripe * 16 + col;
        const float bv = (a.bias && !a.ldb) ? (float)a.bias[n] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = 16 * tg + 4 * rq + r;
            float v = tot[0][r];
            if constexpr (NS == 2) v = v * (1.0f / (1.0f + __expf(-v))) * tot[1][r];
            if (row < a.M) {
                half_t h = (half_t)v;
                if (a.bias) h = (half_t)((float)h + (a.ldb ? (float)a.bias[(size_t)row * a.ldb + n] : bv));
                a.y[(size_t)row * a.ldy + n] = h;
            }
        }
    }
}

template <int TM, int NS>
int stripe_mm2_launch(const StripeParams &p, int grp_shift, hipStream_t s) {
    auto kern = stripe_mm2_kernel<TM, NS>;
    constexpr int TG = TM == 1 ? 1 : (TM == 2 ? 2 : 4), NRB = STRIPE_NW / TG, NPC = 16 * TM * NRB * BK / 8;
    constexpr int XG = (NPC / 64 + STRIPE_NW - 1) / STRIPE_NW;
    const size_t lds = (size_t)3 * (XG * STRIPE_NW * 1024 + NRB * NS * 1024) + (size_t)(NS * p.G * 16 + 63) / 64 * 256;
    if (lds > 160 * 1024 - 64) return GPTQ_E_VARIANT;
    static LdsOptIn opt_in;   // per instantiation; per device inside
    if (int rc = opt_in.ensure((const void *)kern, lds)) return rc;
    MMArgs a{};
    a.x = p.x; a.R = p.R; a.tab = p.tab; a.y = p.y; a.bias = p.bias; a.ldb = (int)p.ldb;
    a.K = p.K; a.nrb = p.K / BK; a.G = p.G; a.grp_shift = grp_shift; a.M = p.M; a.ldx = (int)p.ldx; a.ldy = (int)p.ldy;
    a.nstripes = p.N / 16; a.S = 1; a.span = a.nrb;
    hipLaunchKernelGGL(kern, dim3(p.N / 16), dim3(STRIPE_NW * 64), lds, s, a);
    return (int)hipGetLastError();
}

// ---- single-launch variant, round 3: x through WAVE-PRIVATE staging, plain loads, no workgroup barrier in the K loop ----
// What the kernels above ran into is not what a CU can pull out of L2: tools/l2ingest.hip (profiles/r3g_mid_m/l2ingest.txt) measures
// 140-160 GB/s per CU for plain 1-KiB wave loads of a buffer every workgroup shares -- against 45-63 GB/s for LDS-DMA (what
// stripe_mm2_kernel uses) and 40-50 GB/s for loads in MFMA-fragment order (16 rows x 64 B).  stripe_mm1_kernel uses plain loads but
// pays a workgroup barrier and an exposed LDS round trip per 32-KB chunk.  Here every wave owns a K range of a stripe for ALL row
// tiles, so its x bytes are needed by no other wave: it loads them row-contiguous (two 512-byte row segments per instruction), parks
// them in its own LDS ring (sub-slot = 16 rows x 256 k), reads them back in fragment order and feeds the matrix core -- in-order LDS
// execution inside a wave is the only synchronisation; PF sub-slots of loads stay in flight in registers.  The B fragments of the
// wave's 512 k (64 VGPRs per weight set) are unpacked once per segment and reused by every row tile.  Waves meet once, at the end.
// One stripe x whole K per workgroup, 1 <= TM <= 8 row tiles; groups of at least a row block (scale applied to the fp32 accumulator
// per row block, exactly like stripe_mm_kernel).
constexpr int MM3_SEGK = 512;                                // k per wave and segment
constexpr int MM3_SSK = BK;                                  // k per sub-slot: one row block (B fragments of ONE row block live at a time)
constexpr int MM3_XS = MM3_SSK + 16;                         // halves per staged row: 32 bytes of padding + piece p of row r at position p ^ (r & 3):
                                                             // conflict-free A-fragment reads (see SG_XS below; + 8 alone leaves a 2-way conflict)
constexpr int MM3_SLOT = 16 * MM3_XS;                        // halves per sub-slot
constexpr int MM3_NQ = MM3_SEGK / BK;                        // row blocks (sub-slots per row tile) per wave and segment: 2 / 4 / 4 / 8
constexpr size_t mm3_lds_bytes(int tm, int ns, int nw = STRIPE_NW) {      // ns = weight sets per wave (the pair's two, or C stripes)
    const size_t ring = (size_t)nw * 2 * MM3_SLOT * 2, red = (size_t)nw * ns * tm * 1024;
    return ring > red ? ring : red;
}

// Measured and dropped (profiles/r3g_mid_m/): a 16-wave instance (1024 threads, 128 VGPRs; the microbenchmark's load -> ds_write -> ds_read
// chain moves 130 GB/s per CU from 16 waves against 100 from 8): 2-5 % faster up to 48 rows, slower beyond, where 128 VGPRs no longer hold
// the accumulators (mm3_waves_8_vs_16.txt); and 2 / 3 ADJACENT STRIPES per workgroup on the same staged x for shapes with several rounds
// of stripes (packed words parked in LDS by DMA to make room): + 10-15 % at 16-48 rows on N = 8192, but three stripes x four row tiles do
// not fit 256 VGPRs and the spilling instances run 2 x slower than the K-slice kernel (mm3_multi_stripe.txt).
// C (round 4): ADJACENT stripes per workgroup on the SAME staged x -- shapes whose stripes need several rounds of workgroups (N = 11008,
// 12288: three per CU) pulled M K 2 bytes of x through every CU once per STRIPE; with C = 3 a CU stages x once.  Every wave keeps the B
// fragments of its row block for all C stripes (16 VGPRs each) next to C x TM accumulator tiles: C = 3 fits up to four row tiles (M <= 64)
// without spills -- round 3's attempt parked the packed words in LDS by DMA and spilled at three stripes x four row tiles; here the words
// stay in registers and the reduction buffer aliases the ring.  C > 1: single weight set only.
// NWV (round 4): waves per workgroup.  8 (two per SIMD: 256 registers each) or 4 (one per SIMD: 512 registers -- 256 architectural + 256
// accumulation registers the allocator spills into at one v_accvgpr move per access).  What bounds these kernels is the x ingest, and that is
// bytes IN FLIGHT per CU over the L2 latency (8 waves x 2 sub-slots x 4 KiB = 64 KiB ~ 90 GB/s): four waves with 8 sub-slots each keep 128 KiB
// in flight, and 512 registers hold three stripes x eight row tiles of accumulators next to them.
template <int TM, int NS, int PF, int C = 1, int NWV = STRIPE_NW>
__global__ void __launch_bounds__(NWV * 64) stripe_mm3_kernel(const MMArgs a) {
    typedef uint32_t wvec_t __attribute__((ext_vector_type(WPL)));
    constexpr int NW = NWV, NQ = MM3_NQ, NSUB = NQ * TM;
    constexpr int PCR = MM3_SSK / 8, RPI = 64 / PCR, NI = 16 / RPI;   // 16-byte pieces per staged row, rows per load instruction, instructions per sub-slot
    static_assert(NSUB % PF == 0, "the register slots rotate consistently across segments");   // (PF = 1: always)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    half_t *ring = (half_t *)smem + (size_t)wave * 2 * MM3_SLOT;
    const int stripe0 = blockIdx.x * C;                       // first stripe of this workgroup; stripes past the last one are clamped (and not stored)
    const int rq = lane >> 4, col = lane & 15;
    const UnpackConsts uc = unpack_consts();
    const int nseg = (a.nrb + NW * NQ - 1) / (NW * NQ);
    const uint32_t *wbase[C], *tbase[C];
#pragma unroll
    for (int c = 0; c < C; c++) {
        const int stripe = min(stripe0 + c, a.nstripes - 1);
        wbase[c] = a.R + ((size_t)stripe * a.nrb * NS * 64 + lane) * WPL;
        tbase[c] = a.tab + (size_t)stripe * NS * a.G * 16 + col;
    }

    // x: sub-slot j of a segment = row block j / TM, row tile j % TM of this wave's 512 k; instruction i covers RPI rows (BK * 2 bytes each).
    // Buffer loads: ONE per-lane byte offset per sub-slot + a wave-uniform row offset in an SGPR per instruction; rows past M - 1 are
    // out of the descriptor's range and read as zero (no clamps, no 64-bit address per load).
    u32x4 xr[PF][NI];
    const int xrow = lane / PCR, xpiece = lane % PCR;
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void *)a.x, 0, (int)(((size_t)(a.M - 1) * a.ldx + a.K) * 2), 0x00020000);
    int ldx2 = a.ldx * 2;   // bytes per row of x
    auto xload = [&](int slot, int seg, int j) {
        const int q = j / TM, t = j % TM;
        const int kk = min((seg * NW + wave) * MM3_SEGK + q * MM3_SSK + xpiece * 8, a.K - 8);   // past K: a valid address, the scale is zero
        const int voff = kk * 2 + xrow * ldx2;
#pragma unroll
        for (int i = 0; i < NI; i++)
            xr[slot][i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, voff, (16 * t + RPI * i) * ldx2, 0));
    };
    auto xstore = [&](int slot, int buf) {
#pragma unroll
        for (int i = 0; i < NI; i++) *(u32x4 *)(ring + buf * MM3_SLOT + (RPI * i + xrow) * MM3_XS + (xpiece ^ ((RPI * i + xrow) & 3)) * 8) = xr[slot][i];
    };

    constexpr int NSC = NS * C;                                // weight sets in flight per wave: the pair's two, or C stripes
    constexpr bool SPLIT = NS == 2 && C > 1;                   // the pair on C stripes: gate and up take turns (see the K loop)
    static_assert(!SPLIT || TM == 1, "the pair with several stripes per workgroup: one row tile");
    float4_t yacc[NSC][TM];
#pragma unroll
    for (int s = 0; s < NSC; s++)
#pragma unroll
        for (int t = 0; t < TM; t++) yacc[s][t] = float4_t{0.f, 0.f, 0.f, 0.f};
    half2_t negoff[NOFFC];
    neg_offsets(negoff);

    // the weights of segment 0 go first (HBM: the longest latency), then the first PF sub-slots of x
    // C == 1: the packed words of a whole segment (NQ row blocks) are requested at once, one segment ahead.  C > 1: a ring of WD = 2 row
    // blocks per stripe, refilled right after a row block is unpacked (C x NQ words per lane would not leave room for the accumulators).
    constexpr int WD = (C > 1 && NWV == STRIPE_NW) ? 2 : NQ;      // (four waves: registers for a whole segment of every stripe)
    static_assert(NQ % WD == 0, "ring slots stay aligned across segments");
    wvec_t w[WD][NSC];
    uint32_t tw[WD][NSC];
    auto wload1 = [&](int slot, int seg, int q) {     // one row block of every stripe; past the end: the last row block again (its scale is zeroed)
        const int rb = min((seg * NW + wave) * NQ + q, a.nrb - 1);
        const int g = a.grp_shift >= 0 ? (rb >> a.grp_shift) : 0;
#pragma unroll
        for (int c = 0; c < C; c++)
#pragma unroll
            for (int s = 0; s < NS; s++) {
                w[slot][c * NS + s] = __builtin_nontemporal_load((const wvec_t *)(wbase[c] + ((size_t)rb * NS + s) * (64 * WPL)));
                tw[slot][c * NS + s] = tbase[c][((size_t)s * a.G + g) * 16];
            }
    };
    auto wload = [&](int seg) {
#pragma unroll
        for (int u = 0; u < NQ; u++) {
            const int rb = min((seg * NW + wave) * NQ + u, a.nrb - 1);
            const int g = a.grp_shift >= 0 ? (rb >> a.grp_shift) : 0;
#pragma unroll
            for (int c = 0; c < C; c++)
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    w[u][c * NS + s] = __builtin_nontemporal_load((const wvec_t *)(wbase[c] + ((size_t)rb * NS + s) * (64 * WPL)));
                    tw[u][c * NS + s] = tbase[c][((size_t)s * a.G + g) * 16];
                }
        }
    };
    if constexpr (WD < NQ) {
#pragma unroll
        for (int u = 0; u < WD; u++) wload1(u, 0, u);
    } else {
        wload(0);
    }
#pragma unroll
    for (int i = 0; i < PF; i++) xload(i, 0, i);
    __builtin_amdgcn_sched_barrier(0);

    for (int seg = 0; seg < nseg; seg++) {
        asm volatile("" : "+s"(ldx2));   // keep the row offsets out of SGPRs that live across the loop: an s_mul per load is cheaper
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const bool valid = (seg * NW + wave) * NQ + q < a.nrb;
            // exact q - z fragments of weight set s of this row block + its scale (16 VGPRs per set)
            auto unpack_set = [&](int s, mm_h8_t (&Bs)[PPB]) __attribute__((always_inline)) -> float {
                return dequant_block(w[q % WD][s], tw[q % WD][s], valid, negoff, uc, Bs);
            };
            if constexpr (SPLIT) {
                // the PAIR with C stripes per workgroup (round 5): 2 C weight streams per wave -- their B fragments together (96 VGPRs at C = 3) spill,
                // so gate and up take turns on the same A fragments: C sets unpacked, C x PPB MFMAs, then the other C
                const int j = q;
                xstore(j % PF, j & 1);
                if (j + PF < NSUB) xload(j % PF, seg, j + PF);
                else if (seg + 1 < nseg) xload(j % PF, seg + 1, j + PF - NSUB);
                const half_t *xa = ring + (j & 1) * MM3_SLOT + col * MM3_XS;
#pragma unroll
                for (int h = 0; h < NS; h++) {
                    mm_h8_t Bh[C][PPB];
                    float sch[C];
#pragma unroll
                    for (int c = 0; c < C; c++) {
                        sch[c] = unpack_set(c * NS + h, Bh[c]);
                        __builtin_amdgcn_sched_barrier(0);   // one set's unpack temporaries at a time
                    }
                    float4_t acc[C];
#pragma unroll
                    for (int c = 0; c < C; c++) acc[c] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int b = 0; b < PPB; b++) {
                        const mm_h8_t A = *(const mm_h8_t *)(xa + 8 * ((rq * PPB + b) ^ (col & 3)));
#pragma unroll
                        for (int c = 0; c < C; c++) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A, Bh[c][b], acc[c], 0, 0, 0);
                    }
#pragma unroll
                    for (int c = 0; c < C; c++)
#pragma unroll
                        for (int r = 0; r < 4; r++) yacc[c * NS + h][0][r] = fmaf(sch[c], acc[c][r], yacc[c * NS + h][0][r]);
                    __builtin_amdgcn_sched_barrier(0);
                }
                // every word of the slot is unpacked: refill it
                if constexpr (WD < NQ) {
                    // the slot is free: row block q + WD of this segment, or the first ones of the next (branch-free; past the last segment the
                    // clamped address re-reads the last row block)
                    if (q + WD < NQ) wload1(q % WD, seg, q + WD);
                    else wload1(q % WD, seg + 1, q + WD - NQ);
                } else {
                    if (q == NQ - 1 && seg + 1 < nseg) wload(seg + 1);   // wave-uniform; every word of this segment is unpacked
                }
                __builtin_amdgcn_sched_barrier(0);
            } else {
            // ---- B fragments of this row block (16 VGPRs per weight set) ----
            mm_h8_t B[NSC][PPB];
            float scale[NSC];
#pragma unroll
            for (int s = 0; s < NSC; s++) {
                scale[s] = unpack_set(s, B[s]);
                if constexpr (C > 1) __builtin_amdgcn_sched_barrier(0);   // one stripe's unpack temporaries at a time (32 VGPRs each if interleaved)
            }
            if constexpr (WD < NQ) {
                // the slot is free: row block q + WD of this segment, or the first ones of the next (branch-free; past the last segment the
                // clamped address re-reads the last row block)
                if (q + WD < NQ) wload1(q % WD, seg, q + WD);
                else wload1(q % WD, seg + 1, q + WD - NQ);
            } else {
                if (q == NQ - 1 && seg + 1 < nseg) wload(seg + 1);   // wave-uniform; every word of this segment is unpacked
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < TM; t++) {
                const int j = q * TM + t;
                xstore(j % PF, j & 1);
                // the register slot is free again: request the sub-slot PF ahead (the next segment's first ones at the end of this one)
                if (j + PF < NSUB) xload(j % PF, seg, j + PF);
                else if (seg + 1 < nseg) xload(j % PF, seg + 1, j + PF - NSUB);
                const half_t *xa = ring + (j & 1) * MM3_SLOT + col * MM3_XS;
                float4_t acc[NSC];
#pragma unroll
                for (int s = 0; s < NSC; s++) acc[s] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int b = 0; b < PPB; b++) {
                    const mm_h8_t A = *(const mm_h8_t *)(xa + 8 * ((rq * PPB + b) ^ (col & 3)));
#pragma unroll
                    for (int s = 0; s < NSC; s++) acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A, B[s][b], acc[s], 0, 0, 0);
                }
#pragma unroll
                for (int s = 0; s < NSC; s++)
#pragma unroll
                    for (int r = 0; r < 4; r++) yacc[s][t][r] = fmaf(scale[s], acc[s][r], yacc[s][t][r]);
                __builtin_amdgcn_sched_barrier(0);
            }
            }   // !SPLIT
        }
    }

    // ---- 8 k-waves -> 1 through LDS ([wave][set][tile][lane] float4), wave t finishes row tile t ----
    __syncthreads();   // every wave is done with its ring
    float4_t *red = (float4_t *)smem;
#pragma unroll
    for (int s = 0; s < NSC; s++)
#pragma unroll
        for (int t = 0; t < TM; t++) red[((wave * NSC + s) * TM + t) * 64 + lane] = yacc[s][t];
    __syncthreads();
    // (row tile, stripe) pairs over the waves: wave j finishes pairs j, j + NW, ...
    for (int j = wave; j < TM * C; j += NW) {
        const int t = j % TM, c = j / TM;
        float4_t tot[NS];
#pragma unroll
        for (int s = 0; s < NS; s++) {
            tot[s] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k2 = 0; k2 < NW; k2++) tot[s] += red[((k2 * NSC + c * NS + s) * TM + t) * 64 + lane];
        }
        const int stripe = stripe0 + c;
        if (stripe >= a.nstripes) continue;     // (wave-uniform)
        finish_tile<NS>(tot, a, stripe, 16 * t, rq, col);
    }
}

template <int TM, int NS, int PF, int C = 1, int NWV = STRIPE_NW>
int stripe_mm3_launch(const StripeParams &p, int grp_shift, hipStream_t s) {
    auto kern = stripe_mm3_kernel<TM, NS, PF, C, NWV>;
    constexpr size_t lds = mm3_lds_bytes(TM, NS * C, NWV);
    static LdsOptIn opt_in;   // per instantiation; per device inside
    if (int rc = opt_in.ensure((const void *)kern, lds)) return rc;
    MMArgs a{};
    a.x = p.x; a.R = p.R; a.tab = p.tab; a.y = p.y; a.bias = p.bias; a.ldb = (int)p.ldb;
    a.K = p.K; a.nrb = p.K / BK; a.G = p.G; a.grp_shift = grp_shift; a.M = p.M; a.ldx = (int)p.ldx; a.ldy = (int)p.ldy;
    a.nstripes = p.N / 16; a.S = 1; a.span = a.nrb;
    hipLaunchKernelGGL(kern, dim3((a.nstripes + C - 1) / C), dim3(NWV * 64), lds, s, a);
    return (int)hipGetLastError();
}

// PF = sub-slots of x in flight in registers (one row block of 16 rows each: 4 KiB for 4 bits); it must divide NQ * TM
template <int NS>
int stripe_mm3_dispatch(int tm, const StripeParams &p, int grp_shift, hipStream_t s) {
    constexpr int PF = MM3_NQ % 4 == 0 ? 4 : 2, PFL = 2;   // PFL: the instances that would spill with four (kernel_resources)
    switch (tm) {
        case 1: return stripe_mm3_launch<1, NS, PF>(p, grp_shift, s);
        case 2: return stripe_mm3_launch<2, NS, NS == 2 ? PFL : PF>(p, grp_shift, s);
        case 3: if constexpr (NS == 1) return stripe_mm3_launch<3, NS, PF>(p, grp_shift, s);
        case 4: if constexpr (NS == 1) return stripe_mm3_launch<4, NS, PF>(p, grp_shift, s);
        case 5: if constexpr (NS == 1) return stripe_mm3_launch<5, NS, PF>(p, grp_shift, s);
        case 6: if constexpr (NS == 1) return stripe_mm3_launch<6, NS, PF>(p, grp_shift, s);
        case 7: if constexpr (NS == 1) return stripe_mm3_launch<7, NS, PFL>(p, grp_shift, s);
        case 8: if constexpr (NS == 1) return stripe_mm3_launch<8, NS, PFL>(p, grp_shift, s);
        default: return GPTQ_E_VARIANT;
    }
}

// several stripes per workgroup (round 4): 4-bit / 3-bit single sets, up to four row tiles.  C = ceil(stripes / 256): one workgroup per CU
// Instances: one and two row tiles (C = 3 holds 3 x 16 B-fragment registers next to 3 TM accumulator tiles: more row tiles spill; C = 2 fits
// four without spills but runs 24 us at 48 / 64 rows on 4096 x 8192 against 13.7 / 15.4 for the K-slice schedule).  Measured
// (profiles/r4f_mm3c/, us, this / the K-slice schedule): 4096 x 12288 M = 8 / 16 / 32: 9.1 / 9.6 / 12.1 against 11.5 / 12.1 / 13.4; 4096 x 11008:
// 9.0 / 9.2 / 11.8 against 11.1 / 11.6 / 12.9; 4096 x 8192 (C = 2): 7.8 / 8.0 / 10.1 against 8.3 / 8.9 / 11.8.
template <int C>
int stripe_mm3c_dispatch(int tm, const StripeParams &p, int grp_shift, hipStream_t s) {
    switch (tm) {
        case 1: return stripe_mm3_launch<1, 1, 2, C>(p, grp_shift, s);
        case 2: return stripe_mm3_launch<2, 1, 1, C>(p, grp_shift, s);
        default: return GPTQ_E_VARIANT;
    }
}
// round 5: the gate | up PAIR with C stripes per workgroup, one row tile (5 .. 16 rows of a decode batch): 2 C weight streams per wave on the
// same staged x, ONE sub-slot of x in flight (two measured no faster: DESIGN 3.8)
template <int C>
int stripe_mm3c_pair_dispatch(int tm, const StripeParams &p, int grp_shift, hipStream_t s) {
    if (tm == 1) return stripe_mm3_launch<1, 2, 1, C>(p, grp_shift, s);
    return GPTQ_E_VARIANT;
}

// four-wave instances (512 registers per wave).  Measured (profiles/r4l_w4/w4.txt, us, four waves / default) with SIX sub-slots of x in flight:
// they lose wherever the eight-wave kernel does not spill (4096^2: 8.1 .. 16.7 against 7.4 .. 14.6 at 32 .. 128 rows -- so the x ingest is NOT
// bound by bytes in flight, as hoped) and wherever they spill themselves, and win at three row tiles on the multi-round shapes.  The depth of the
// x prefetch was what made them spill (profiles/r4n_w4pf/w4pf.txt): with TWO sub-slots the C = 3 instance of three row tiles keeps its 53
// spilled registers (4096 x 12288 at 48 rows 19.3 -> 15.7 us, 4096 x 11008 18.4 -> 14.9), with ONE the four-row-tile instance nearly fits (9
// spilled: 49 .. 64 rows 23.7 -> 19.5 / 23.3 -> 19.0 us), and on two-round shapes (C = 2, N = 8192) nothing spills up to six row tiles: 49 .. 64 rows
// 15.8 -> 13.6 us, 65 .. 80 25.5 -> 18.2, 96 24.2 -> 20.4.  Seven and eight row tiles (C = 2) and five or six with C = 3 spill 44 .. 100 registers and
// lose to the K-sliced tile GEMM (29.7 / 32.7 against 23.7; 32 .. 40 against 27.5): not built.
template <int C>
int stripe_mm3w4_dispatch(int tm, const StripeParams &p, int grp_shift, hipStream_t s) {
    if (tm == 3) return stripe_mm3_launch<3, 1, 2, C, 4>(p, grp_shift, s);
    if constexpr (C == 2) {
        if (tm == 4) return stripe_mm3_launch<4, 1, 2, C, 4>(p, grp_shift, s);
        if (tm == 5) return stripe_mm3_launch<5, 1, 1, C, 4>(p, grp_shift, s);
        if (tm == 6) return stripe_mm3_launch<6, 1, 1, C, 4>(p, grp_shift, s);
    } else {
        if (tm == 4) return stripe_mm3_launch<4, 1, 1, C, 4>(p, grp_shift, s);
    }
    return GPTQ_E_VARIANT;
}

// ---- round 6: loader / consumer split (VERDICT r5 item 6) -- x through an LDS ring filled by LDS-DMA, consumers only ds_read + MFMA ----
// What bounds the wave-private kernel above at 17 .. 128 rows is neither HBM, nor the matrix core (13 % busy), nor LDS waits (4 %): it is the in-order
// chain x load -> ds_write -> ds_read -> MFMA inside every wave (DESIGN 3.3a, round 5 counters).  Here the chain is cut: NL loader waves move x --
// row-block-major chunks of 16 TM rows x 128 k, 1 KiB (4 rows) per `global_load_lds_dwordx4`, the XOR swizzle of the A-fragment reads applied on the
// SOURCE side -- into a ring of NSLOT chunks and never compute; NCW consumer waves own row blocks (k-split, like the wave-private kernel), request
// their packed words one row block ahead with plain loads, unpack them once and run 4 TM C MFMAs per row block on A fragments read out of the ring;
// they wait for nothing but the chunk's arrival.  Progress words in LDS: P[l] = chunks of loader l that have landed (counted vmcnt), done[w] = chunks
// consumer w has finished (a ring slot is refilled when the consumer of the chunk it held is done).  The loaders poll / publish through inline
// assembly (a wave with LDS-DMA in flight gets an s_waitcnt vmcnt(0) in front of every compiler-visible LDS instruction: tools/persistlab.hip).
// One weight set, C stripes per workgroup on the same x (C = ceil(stripes / 256): one workgroup per CU), 1 <= TM <= 4, groups of at least a row block.
// every wait inside the workgroup is bounded (a launch takes < 0.1 ms; 2^20 polls with s_sleep are > 20 ms): a wave that runs into the limit goes on with what
// is there -- a wrong result that the parity tests would see, never a hung device
constexpr int MMR_SPIN_LIMIT = 1 << 20;
constexpr int MMR_NL = 2, MMR_INF = 2;      // loader waves, chunks in flight per loader (2 / 3 / 4 and 1 / 2 / 3 measured within 5 % of each other: profiles/r6s_mmr/)
constexpr int MMR_NSLOT = 8;      // ring chunks (at most 64 rows x 128 k = 16 KiB each); six consumers hold one chunk each, the loaders fill the others
// NH = 2 (five to eight row tiles): the consumers split into two ROW HALVES -- consumer cw owns pass cw % 2 of the row blocks cw / 2, cw / 2 + 3, .. -- instead
// of running both passes on one set of B fragments: the sums of four row tiles per wave instead of eight (the eight-tile instance of three stripes spilled its
// prefetched weight words, 37 us against 28.9 for the sliced tile GEMM), at the price of unpacking every row block twice per workgroup.
// NS = 2: the gate | up pair -- per row block a consumer unpacks the C gate stripes, runs them on the chunk, then the C up stripes on the SAME chunk (the B
// fragment and chunk-sum registers take turns; only the sums per set are doubled), one set's packed words requested ahead; SiLU(gate) * up on the fp32 sums.
// SS = 1 (the pair): the consumers split by SET instead -- consumer cw runs set cw % 2 (its k lane: cw / 2) with the registers of the single-set instance
// and unpacks nothing twice; a chunk is released when the consumers of both sets are done with it.
template <int TM, int C, int NH = 1, int NS = 1, int SS = 0>      // row tiles, stripes per workgroup, row halves, weight sets, set split
__global__ void __launch_bounds__(STRIPE_NW * 64) stripe_mmr_kernel(const MMArgs a) {
    constexpr int MMR_NCW = STRIPE_NW - MMR_NL;
    typedef uint32_t wvec_t __attribute__((ext_vector_type(WPL)));
    typedef const __attribute__((address_space(1))) void *gptr_t;
    typedef __attribute__((address_space(3))) void *lptr_t;
    typedef __attribute__((address_space(3))) int lds_int;
    constexpr int NL = MMR_NL, NCW = MMR_NCW, NSLOT = MMR_NSLOT;
    // five to eight row tiles: a row block of x is TWO chunks (rows 0 .. 63, rows 64 ..), consumed one after the other on the SAME unpacked B fragments --
    // a 32-KiB chunk would leave four ring slots for six consumers (measured: 25.5 / 45 us at 80 / 128 rows against 15.9 at 64).  Chunk ch = rb NPASS + pass.
    constexpr int TH = TM <= 4 ? TM : 4, NPASS = (TM + TH - 1) / TH;
    constexpr int CHB = 16 * TH * BK * 2;                                     // bytes of a ring slot (BK = 128 k: 256 B per row)
    static_assert(NL + NCW == STRIPE_NW && BK == 128, "8 waves; a chunk row is 16 pieces of 16 bytes");
    static_assert(NL % NPASS == 0, "a loader wave always loads the same pass: its DMA instruction count per chunk is a constant for vmcnt");
    static_assert(4 * TH * (MMR_INF - 1) <= 63 && NL * MMR_INF <= NSLOT, "vmcnt is six bits wide; the chunks in flight fit the ring");
    static_assert(NH == 1 || (NH == NPASS && NCW % NH == 0), "row halves: one per pass");
    constexpr int NSS = SS ? NS : 1, NSW = NS / NSS;  // set roles among the consumers, sets a consumer runs
    constexpr int NR = NH * NSS;                      // consumer roles: cw -> role cw % NR = (set role) * NH + (row half), k lane cw / NR
    static_assert(NCW % NR == 0 && (SS == 0 || NS == 2), "roles divide the consumers");
    constexpr int NKW = NCW / NR;                     // consumers that split k (per role)
    constexpr int NPW = NPASS / NH;                   // passes a consumer runs per row block
    constexpr int TW = NPW * TH < TM ? NPW * TH : TM; // row tiles a consumer holds sums for
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
    lds_int *sync = (lds_int *)(smem + NSLOT * CHB);                          // P[NL] | done[NCW]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // K slices (a.S > 1: long K on shapes whose stripes fill one round): workgroup = (slice, group of C stripes); the slice's row blocks rb0 .. rb0 + nrbl - 1,
    // its fp32 sums go to a.partials [S][M][N] and a combine launch adds the slices in slice order
    const int ngroups = (a.nstripes + C - 1) / C;
    const int sl = blockIdx.x / ngroups;
    const int stripe0 = (blockIdx.x - sl * ngroups) * C;
    const int rb0 = sl * a.span, nrbl = min(a.span, a.nrb - rb0);
    if (tid < NL + NCW) sync[tid] = 0;
    __syncthreads();
    auto ld_raw = [](lds_int *p) {
        int v;
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"((uint32_t)(uintptr_t)p) : "memory");
        return v;
    };
    auto st_raw = [](lds_int *p, int v) { asm volatile("ds_write_b32 %0, %1" ::"v"((uint32_t)(uintptr_t)p), "v"(v) : "memory"); };

    float4_t yacc[NSW][C][TW];
#pragma unroll
    for (int st = 0; st < NSW; st++)
#pragma unroll
        for (int c = 0; c < C; c++)
#pragma unroll
            for (int t = 0; t < TW; t++) yacc[st][c][t] = float4_t{0.f, 0.f, 0.f, 0.f};
    const int rq = lane >> 4, col = lane & 15;

    if (wave < NL) {
        // =========================== LOADER ===========================
        // instruction j of a chunk: rows 4 j .. 4 j + 3, lane = (row in the four, position): the position holds piece (position ^ (row & 15))
        auto load_pass = [&](auto pass_c) {
            constexpr int PS = decltype(pass_c)::value;
            constexpr int NDI = 4 * (TM - PS * TH < TH ? TM - PS * TH : TH);       // DMA instructions of this pass's chunks (1 KiB = 4 rows each)
            const half_t *src[NDI];
#pragma unroll
            for (int j = 0; j < NDI; j++) {
                const int r = 4 * j + (lane >> 4), piece = (lane & 15) ^ (r & 15);
                src[j] = a.x + (size_t)min(PS * 16 * TH + r, a.M - 1) * a.ldx + piece * 8;
            }
            int i = 0;
            for (int ch = wave; ch < nrbl * NPASS; ch += NL, i++) {
                const int rb = ch / NPASS;
                if (ch >= NSLOT) {           // the slot held chunk ch - NSLOT: wait for its consumer
                    const int orb = (ch - NSLOT) / NPASS, ops = (ch - NSLOT) % NPASS;
                    const int need = NH == 1 ? (orb / NKW) * NPASS + ops : orb / NKW;
#pragma unroll
                    for (int sr = 0; sr < NSS; sr++) {      // (every set role's consumer of that chunk)
                        const int cw = (orb % NKW) * NR + sr * NH + (NH == 1 ? 0 : ops);
                        for (int spin = 0; ld_raw(sync + NL + cw) <= need && spin < MMR_SPIN_LIMIT; spin++) __builtin_amdgcn_s_sleep(1);
                    }
                }
                unsigned char *dst = smem + (ch % NSLOT) * CHB;
#pragma unroll
                for (int j = 0; j < NDI; j++) __builtin_amdgcn_global_load_lds((gptr_t)(src[j] + (size_t)(rb0 + rb) * BK), (lptr_t)(dst + j * 1024), 16, 0, 0);
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDI * (MMR_INF - 1)) : "memory");      // every chunk but the MMR_INF - 1 most recent has landed
                if (i >= MMR_INF - 1 && lane == 0) st_raw(sync + wave, i - (MMR_INF - 1) + 1);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == 0) st_raw(sync + wave, i);
        };
        if (NPASS == 1 || wave % NPASS == 0) load_pass(std::integral_constant<int, 0>{});
        else load_pass(std::integral_constant<int, NPASS - 1>{});
    } else {
        // =========================== CONSUMER ===========================
        const int cw = wave - NL;
        const UnpackConsts uc = unpack_consts();
        // wave-uniform bases (stripe, row block: SGPRs) + ONE per-lane offset each -- C pointer pairs per lane cost the largest instance its registers
        int stripe_of[C];
#pragma unroll
        for (int c = 0; c < C; c++) stripe_of[c] = min(stripe0 + c, a.nstripes - 1);
        const uint32_t woff = lane * WPL;
        half2_t negoff[NOFFC];
        neg_offsets(negoff);
        wvec_t wn[C];
        uint32_t twn[C];
        auto wload = [&](int rb, int st) {     // the image: [stripe][row block][set][64 lanes] words, [stripe][set][group][16] table entries
            const int rbc = min(rb0 + rb, a.nrb - 1);
            const int g = a.grp_shift >= 0 ? (rbc >> a.grp_shift) : 0;
#pragma unroll
            for (int c = 0; c < C; c++) {
                const wvec_t *wp = (const wvec_t *)(a.R + (((size_t)stripe_of[c] * a.nrb + rbc) * NS + st) * (64 * WPL) + woff);
                wn[c] = NH == 1 ? __builtin_nontemporal_load(wp) : *wp;          // (row halves: the CU's second reader of the row block should find it in the caches)
                twn[c] = (a.tab + (((size_t)stripe_of[c] * NS + st) * a.G + g) * 16)[col];
            }
        };
        // consumer cw: k lane kw of NKW, passes P0 .. P0 + NPW - 1 of the row blocks kw, kw + NKW, ..  (NH = 1: kw = cw, every pass)
        auto consume = [&](auto p0_c) {
            constexpr int P0 = decltype(p0_c)::value;
            const int kw = cw / NR, sr = (cw % NR) / NH;         // k lane, set role
            wload(kw, SS ? sr : 0);
            int i = 0, seen[NL];
#pragma unroll
            for (int l = 0; l < NL; l++) seen[l] = 0;
            for (int rb = kw; rb < nrbl; rb += NKW, i++) {
#pragma unroll
                for (int sw = 0; sw < NSW; sw++) {
                    const int st = SS ? sr : sw;
                    // exact q - z fragments of this row block's set (16 VGPRs per stripe) + scales, then the next set's / row block's words are requested
                    mm_h8_t B[C][PPB];
                    float scale[C];
#pragma unroll
                    for (int c = 0; c < C; c++) {
                        scale[c] = dequant_block(wn[c], twn[c], true, negoff, uc, B[c]);      // (rb < nrbl: every row block here is inside the slice)
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if (sw + 1 < NSW) wload(rb, st + 1);
                    else wload(rb + NKW, SS ? sr : 0);
                    __builtin_amdgcn_sched_barrier(0);
                    // every (stripe, tile) of a chunk has its OWN accumulator: C TH independent MFMA chains (a shared one made tile t + 1 wait for tile t's
                    // MFMA -> fma tail: 2.2 us per row tile, the slope of the wave-private kernel); the scales are applied once, after the chunk
#pragma unroll
                    for (int pw = 0; pw < NPW; pw++) {
                        const int ps = P0 + pw;
                        const int ch = rb * NPASS + ps;
                        {   // the chunk: loader ch % NL, its chunk number ch / NL
                            const int l = ch % NL, need = ch / NL;
                            int sv = 0;
#pragma unroll
                            for (int q = 0; q < NL; q++)
                                if (l == q) sv = seen[q];
                            for (int spin = 0; sv <= need && spin < MMR_SPIN_LIMIT; spin++) {
                                sv = __hip_atomic_load(sync + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                                if (sv <= need) __builtin_amdgcn_s_sleep(1);
                            }
#pragma unroll
                            for (int q = 0; q < NL; q++)
                                if (l == q) seen[q] = sv;
                            asm volatile("" ::: "memory");
                        }
                        const unsigned char *xa = smem + (ch % NSLOT) * CHB + col * (BK * 2);
                        float4_t acc[C][TH];
#pragma unroll
                        for (int c = 0; c < C; c++)
#pragma unroll
                            for (int t = 0; t < TH; t++) acc[c][t] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int t = 0; t < TH; t++) {
                            if ((P0 + pw) * TH + t >= TM) continue;
                            mm_h8_t A[PPB];
#pragma unroll
                            for (int b = 0; b < PPB; b++) A[b] = *(const mm_h8_t *)(xa + t * 16 * (BK * 2) + 16 * ((rq * PPB + b) ^ col));
#pragma unroll
                            for (int b = 0; b < PPB; b++)
#pragma unroll
                                for (int c = 0; c < C; c++) acc[c][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[b], B[c][b], acc[c][t], 0, 0, 0);
                        }
                        if (sw == NSW - 1) {
                            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // (this wave's reads of the chunk have returned)
                            if (lane == 0) __hip_atomic_store(sync + NL + cw, i * NPW + pw + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
#pragma unroll
                        for (int c = 0; c < C; c++)
#pragma unroll
                            for (int t = 0; t < TH; t++) {
                                if ((P0 + pw) * TH + t >= TM) continue;
#pragma unroll
                                for (int r = 0; r < 4; r++) yacc[sw][c][pw * TH + t][r] = fmaf(scale[c], acc[c][t][r], yacc[sw][c][pw * TH + t][r]);
                            }
                    }
                }
            }
        };
        if (NH == 1 || (cw % NR) % NH == 0) consume(std::integral_constant<int, 0>{});
        else consume(std::integral_constant<int, NH - 1>{});
    }

    // ---- the k-waves -> 1 through LDS ([consumer][set][stripe][tile of the consumer][lane] float4, over the ring), wave j finishes (stripe, tile) pairs j, j + 8, .. ----
    __syncthreads();
    float4_t *red = (float4_t *)smem;
    if (wave >= NL) {
#pragma unroll
        for (int st = 0; st < NSW; st++)
#pragma unroll
            for (int c = 0; c < C; c++)
#pragma unroll
                for (int t = 0; t < TW; t++) red[((((wave - NL) * NSW + st) * C + c) * TW + t) * 64 + lane] = yacc[st][c][t];
    }
    __syncthreads();
    for (int j = wave; j < TM * C; j += STRIPE_NW) {
        const int t = j % TM, c = j / TM;
        const int hh = NH == 1 ? 0 : t / TH, tl = NH == 1 ? t : t % TH;       // the row half that holds tile t, its index there
        float4_t tot[NS];
#pragma unroll
        for (int st = 0; st < NS; st++) {
            tot[st] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k2 = 0; k2 < NKW; k2++) tot[st] += red[((((k2 * NR + (SS ? st : 0) * NH + hh) * NSW + (SS ? 0 : st)) * C + c) * TW + tl) * 64 + lane];
        }
        const int stripe = stripe0 + c;
        if (stripe >= a.nstripes) continue;
        const int n = stripe * 16 + col;
        if constexpr (NS == 1) {
            if (a.S > 1) {      // this slice's fp32 sums (the combine launch rounds and adds the bias / residual)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int row = 16 * t + 4 * rq + r;
                    if (row < a.M) a.partials[((size_t)sl * a.M + row) * (a.nstripes * 16) + n] = tot[0][r];
                }
                continue;
            }
        }
        finish_tile<NS>(tot, a, stripe, 16 * t, rq, col);
    }
}

// the slices of stripe_mmr_kernel meet here: y = fp16(sum over the slices, in slice order) [+ bias / residual on the rounded sum, as every epilogue of this file];
// partials [S][M][N] fp32; one thread per 8 columns of a row, the loads of four slices in flight together
__global__ void __launch_bounds__(256) mmr_combine_kernel(const float *__restrict__ partials, int S, int M, int N, const half_t *__restrict__ add, int64_t ldb,
                                                          half_t *__restrict__ y, int64_t ldy) {
    const int row = blockIdx.y, c8 = blockIdx.x * 256 + threadIdx.x;
    if (c8 * 8 >= N) return;
    const float *first = partials + (size_t)row * N + (size_t)c8 * 8;
    float4_t lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
    for (int sl0 = 0; sl0 < S; sl0 += 4) {
        float4_t vl[4], vh[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float *src = first + (size_t)min(sl0 + q, S - 1) * M * N;
            vl[q] = *(const float4_t *)src;
            vh[q] = *(const float4_t *)(src + 4);
        }
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (sl0 + q < S) {
                lo += vl[q];
                hi += vh[q];
            }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        half_t hh = (half_t)(j < 4 ? lo[j & 3] : hi[j & 3]);
        const int n = c8 * 8 + j;
        if (add) hh = (half_t)((float)hh + (float)add[(ldb ? (size_t)row * ldb : (size_t)0) + n]);
        y[(size_t)row * ldy + n] = hh;
    }
}

template <int TM, int C, int NH = 1, int NS = 1, int SS = 0>
int stripe_mmr_launch(const StripeParams &p, int grp_shift, hipStream_t s, int S = 1, void *ws = nullptr, size_t ws_bytes = 0) {
    auto kern = stripe_mmr_kernel<TM, C, NH, NS, SS>;
    constexpr size_t ring = (size_t)MMR_NSLOT * 16 * (TM <= 4 ? TM : 4) * BK * 2, red = (size_t)(STRIPE_NW - MMR_NL) * (SS ? 1 : NS) * C * (NH == 2 ? 4 : TM) * 1024;
    constexpr size_t lds = (ring > red ? ring : red) + 256;
    static_assert(lds <= 160 * 1024 - 64, "LDS");
    static LdsOptIn opt_in;   // per instantiation; per device inside
    if (int rc = opt_in.ensure((const void *)kern, lds)) return rc;
    MMArgs a{};
    a.x = p.x; a.R = p.R; a.tab = p.tab; a.y = p.y; a.bias = p.bias; a.ldb = (int)p.ldb;
    a.K = p.K; a.nrb = p.K / BK; a.G = p.G; a.grp_shift = grp_shift; a.M = p.M; a.ldx = (int)p.ldx; a.ldy = (int)p.ldy;
    a.nstripes = p.N / 16; a.S = 1; a.span = a.nrb;
    if (S > 1) {
        if (NS != 1 || p.N % 8) return GPTQ_E_VARIANT;
        a.span = (a.nrb + S - 1) / S;
        a.S = (a.nrb + a.span - 1) / a.span;
        if ((size_t)a.S * p.M * p.N * 4 > ws_bytes || !ws) return GPTQ_E_WORKSPACE;
        a.partials = (float *)ws;
    }
    hipLaunchKernelGGL(kern, dim3((a.nstripes + C - 1) / C * a.S), dim3(STRIPE_NW * 64), lds, s, a);
    if (a.S > 1) hipLaunchKernelGGL(mmr_combine_kernel, dim3((p.N / 8 + 255) / 256, p.M), dim3(256), 0, s, a.partials, a.S, p.M, p.N, p.bias, p.ldb, p.y, p.ldy);
    return (int)hipGetLastError();
}
// K slices (long K, one round of stripes): four stripes per workgroup x S slices = one round of workgroups, a quarter of x per workgroup
int stripe_mmr_sliced_dispatch(int tm, int S, const StripeParams &p, int grp_shift, void *ws, size_t ws_bytes, hipStream_t s) {
    if constexpr (SB == 4) {      // (the loader / consumer kernel is built for 4 bits: BK = 128)
        constexpr int C = 4;
        switch (tm) {
            case 2: return stripe_mmr_launch<2, C>(p, grp_shift, s, S, ws, ws_bytes);
            case 3: return stripe_mmr_launch<3, C>(p, grp_shift, s, S, ws, ws_bytes);
            case 4: return stripe_mmr_launch<4, C>(p, grp_shift, s, S, ws, ws_bytes);
            case 5: return stripe_mmr_launch<5, C, 1>(p, grp_shift, s, S, ws, ws_bytes);
            case 6: return stripe_mmr_launch<6, C, 2>(p, grp_shift, s, S, ws, ws_bytes);      // (two passes spill from six row tiles on with four stripes)
            case 7: return stripe_mmr_launch<7, C, 2>(p, grp_shift, s, S, ws, ws_bytes);
            case 8: return stripe_mmr_launch<8, C, 2>(p, grp_shift, s, S, ws, ws_bytes);
            default: break;
        }
    }
    return GPTQ_E_VARIANT;
}
// the gate | up pair: the consumers split by set (SS = 1).  Measured (profiles/r6z_pair/, us, 2 x 4096 x 11008 at 32 / 48 / 64 / 80 / 96 / 112 / 128 rows): set split
// 16.2 / 19.2 / 21.9 / 26.1 / 28.7 / 31.0 / 51.0 (eight row tiles of three stripes spilled: not built), both sets per consumer (row halves from five row tiles on) 16.4 / 20.6 /
// 32.7 / 46.7 / 47.2 / 48.6 / 52.6 (spills from four row tiles on), the routes before 21.3 / 35.0 / 36.0 / 49.2 / 55.5 / 70.5 / 71.8
template <int C>
int stripe_mmr_pair_dispatch(int tm, const StripeParams &p, int grp_shift, hipStream_t s) {
    switch (tm) {
        case 2: return stripe_mmr_launch<2, C, 1, 2, 1>(p, grp_shift, s);
        case 3: return stripe_mmr_launch<3, C, 1, 2, 1>(p, grp_shift, s);
        case 4: return stripe_mmr_launch<4, C, 1, 2, 1>(p, grp_shift, s);
        case 5: return stripe_mmr_launch<5, C, 1, 2, 1>(p, grp_shift, s);
        case 6: return stripe_mmr_launch<6, C, 1, 2, 1>(p, grp_shift, s);
        case 7: return stripe_mmr_launch<7, C, 1, 2, 1>(p, grp_shift, s);
        case 8: if constexpr (C == 2) return stripe_mmr_launch<8, C, 1, 2, 1>(p, grp_shift, s);   // (three stripes: two launches of four row tiles, see the dispatcher)
        default: return GPTQ_E_VARIANT;
    }
}
// two to eight row tiles.  Five to seven run both passes per consumer (NH = 1), eight the row halves (NH = 2: its two-pass instance spilled) -- measured in
// profiles/r6y_mmr_halves/, the table in DESIGN 3.3a, round 6
template <int C>
int stripe_mmr_dispatch(int tm, const StripeParams &p, int grp_shift, hipStream_t s) {
    switch (tm) {
        case 2: return stripe_mmr_launch<2, C>(p, grp_shift, s);
        case 3: return stripe_mmr_launch<3, C>(p, grp_shift, s);
        case 4: return stripe_mmr_launch<4, C>(p, grp_shift, s);
        case 5: return stripe_mmr_launch<5, C>(p, grp_shift, s);
        case 6: return stripe_mmr_launch<6, C>(p, grp_shift, s);
        case 7: return stripe_mmr_launch<7, C>(p, grp_shift, s);
        case 8: return stripe_mmr_launch<8, C, 2>(p, grp_shift, s);
        default: return GPTQ_E_VARIANT;
    }
}

// K slices for a launch (profiles/r2c_mm/slices.txt): as many workgroups as fill the chip ONCE (256; 128 for four row tiles, whose x
// slices are the largest) -- a second, partial round of workgroups costs more than larger slices -- and never more x per workgroup
// than LDS holds.  Returns the row blocks per slice.
int mm_pick_slices(int tm, int nrb, int groups, int forced) {
    const int max_span_k = 135 * 1024 / (32 * tm) - 8;   // rows * (span + 8) * 2 bytes <= 135 KB
    const int target = tm >= 4 ? 128 : 256;
    int s = forced > 0 ? forced : target / groups;
    if (s > nrb) s = nrb;
    if (s < 1) s = 1;
    int span = (nrb + s - 1) / s;
    while (forced <= 0 && span * BK > max_span_k && span > 1) span--;   // (a forced S is taken literally: A/B sweeps)
    s = (nrb + span - 1) / span;
    return (nrb + s - 1) / s;   // equal slices: the longest one sets the time
}

template <int TM, int NS, bool PS>
int stripe_mm_launch(const StripeParams &p, int grp_shift, void *ws, size_t ws_bytes, int forced_slices, hipStream_t s) {
    auto kern = stripe_mm_kernel<TM, NS, PS>;
    const int nrb = p.K / BK, nstripes = p.N / 16, groups = (nstripes + STRIPE_NW - 1) / STRIPE_NW;
    const int span = mm_pick_slices(TM, nrb, groups, forced_slices);
    const int S = (nrb + span - 1) / span;
    const size_t lds = (size_t)16 * TM * (span * BK + 8) * 2;
    if (lds > 160 * 1024 - 256) return GPTQ_E_VARIANT;
    const size_t part_bytes = S > 1 ? (size_t)groups * S * STRIPE_NW * NS * TM * 256 * 4 : 0;
    if (S > 1 && (!ws || ws_bytes < part_bytes)) return GPTQ_E_WORKSPACE;
    static LdsOptIn opt_in;   // per instantiation; per device inside
    if (int rc = opt_in.ensure((const void *)kern, lds)) return rc;
    MMArgs a{};
    a.x = p.x; a.R = p.R; a.tab = p.tab; a.y = p.y; a.bias = p.bias; a.ldb = (int)p.ldb;
    a.partials = (float *)ws;
    a.K = p.K; a.nrb = nrb; a.G = p.G; a.grp_shift = grp_shift; a.M = p.M; a.ldx = (int)p.ldx; a.ldy = (int)p.ldy;
    a.nstripes = nstripes; a.S = S; a.span = span; a.gq_shift = p.gq_shift;
    if constexpr (TM == 1 && NS == 1) {
        // round 6: the caller wants h = rmsnorm(y) * w for the NEXT linear -- the combine launch owns whole rows and writes it too
        if (S > 1 && p.next_norm_w && p.h && p.next_norm_done && p.N / 8 <= 4096 && p.ldy % 8 == 0 && p.ldh % 8 == 0 && (!p.bias || p.ldb % 8 == 0) &&
            ((uintptr_t)p.y % 16 == 0) && ((uintptr_t)p.h % 16 == 0) && ((uintptr_t)p.next_norm_w % 16 == 0) && (!p.bias || (uintptr_t)p.bias % 16 == 0) &&
            (size_t)S * 16 * p.N * 4 <= ws_bytes) {
            a.rowmajor = 1;
            hipLaunchKernelGGL(kern, dim3(groups * S), dim3(STRIPE_NW * 64), lds, s, a);
            *p.next_norm_done = 1;
            return slices_combine_norm_launch((const float *)ws, S, p.M, p.N, p.bias, p.ldb, p.y, p.ldy, p.next_norm_w, p.next_norm_eps, p.h, p.ldh, s);
        }
    }
    hipLaunchKernelGGL(kern, dim3(groups * S), dim3(STRIPE_NW * 64), lds, s, a);
    if (S > 1) hipLaunchKernelGGL((stripe_mm_reduce_kernel<TM, NS>), dim3(groups * TM), dim3(STRIPE_NW * 64), 0, s, a);
    return (int)hipGetLastError();
}


// ---- batches above 128 rows on the stripe16 image: a 2-D tiled, fused-dequantise MFMA GEMM (round 3) ----
// The dense route (dequantise the layer per call + a tile GEMM on fp16 operands) pays a 10-20 us pass over the weights that is as long
// as the product itself below ~1000 rows, and its 256 x 256 tiles leave most of the chip idle there.  This kernel keeps the weights
// packed: workgroup tile = 128 rows x 128 columns (8 stripes; gate | up pair: 64 columns of both sets) x whole K, 8 waves = 2 row
// halves (64 rows = 4 MFMA row tiles) x 4 column quarters (2 weight slots: 2 stripes, or {gate, up} of one) -- the first version gave a wave
// 2 row tiles x 4 slots and was bound by the unpack VALU (650-690 TFLOP/s with the chip full).  Per row block (BK k):
//   x: the 128 x BK chunk is fetched by plain buffer loads (one per-lane offset for the whole kernel, row / k offsets in an SGPR; rows
//      past M are out of the descriptor's range and read as zero), parked in one of two LDS buffers by the SAME threads one iteration
//      ahead, ONE workgroup barrier per chunk; a wave reads its 4 x PPB A fragments once per chunk and reuses them for its slots;
//   W: a slot's packed words (one dwordx4 per lane and row block -- the B fragments of the chunk's PPB MFMAs) are requested PFW = 4
//      chunks ahead into registers, unpacked to the exact q - z (stripe_unpack.inc) once for the wave's 32 rows;
//   the group scale multiplies the fp32 accumulator once per row block (as in stripe_mm_kernel): no fp16 rounding of weights.
// Grid = column groups x row tiles of 128; linear id = row tile * groups + group.  Groups of at least a row block (no prescale mode).
constexpr int SG_PFW = 4, SG_NSW = 2;                  // chunks of weights in flight; weight slots per wave
// halves per staged row: 32 bytes of padding, and piece p (16 B) of row r sits at position p ^ (r & 3) -- with the lane groups ds_read_b128
// is served in ({0-3, 12-15, 20-27}, ...: 8 rows of one k quarter + the other 8 rows of the next) that makes every A-fragment read conflict-
// free; the plain 16-byte padding of the other kernels leaves a 2-way conflict on 4 of 16 lanes (PMC: 40 % of the LDS cycles of this kernel)
constexpr int SG_XS = BK + 16;
constexpr size_t sg_lds_bytes(int rt) { return (size_t)2 * (32 * rt) * SG_XS * 2; }

// RT = row tiles per wave: 4 (128-row workgroup tiles, exact q - z on the matrix core + fp32 group scale) or 8 (256-row tiles for the
// batches where one round of 256 x 128 tiles fills the chip: twice the MFMAs per unpacked word and per A fragment; PRESCALED operands --
// B = fp16((q - z) * scale), the reference's own dequantisation, quant_linear.py:128 -- so that the MFMAs accumulate straight into the 64
// result registers and no second accumulator set is needed).
// (Measured and dropped: two phases per chunk with the row halves of the waves one barrier apart -- the gemm8 stagger, so that the waves sharing
// a SIMD are in opposite phases: 830-920 TFLOP/s chip-full against 930-1040, profiles/r3g_mid_m/stripe_gemm_staggered_phases.txt; and
// 4-wave workgroups of 128 x 64, two per CU, to overlap one workgroup's MFMAs with the other's barrier / unpack phase --
// 680-750 TFLOP/s with the chip full against 800-900: twice the x staging per CU, half the reuse of an A fragment;
// profiles/r3g_mid_m/stripe_gemm_4wave_two_per_cu.txt.)
template <int NS, int RT>
__global__ void __launch_bounds__(STRIPE_NW * 64) stripe_gemm_kernel(const MMArgs a) {
    typedef uint32_t wvec_t __attribute__((ext_vector_type(WPL)));
    typedef float float2_t __attribute__((ext_vector_type(2)));
    constexpr bool PS = RT == 8;
    constexpr int TR = 32 * RT, PFW = SG_PFW, NSW = SG_NSW, XS = SG_XS, XBUF = TR * XS;
    constexpr int PCR = BK / 8, RPT = 512 / PCR, NXI = TR / RPT;   // 16-byte pieces per staged row, rows per 512-thread load, loads per chunk and thread
    constexpr int SPG = NS == 1 ? 8 : 4;                           // stripes per workgroup
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    half_t *xl = (half_t *)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;   // row half (16 RT rows) x column quarter (2 weight slots)
    const int ngroups = (a.nstripes + SPG - 1) / SPG;
    // K slices (round 4, a.S > 1: one row tile, batches of up to 128 rows whose column groups do not fill the chip): linear id = slice * groups
    // + group; the slice covers row blocks [cb, ce), a.span a multiple of PFW; its fp32 sums go to a.partials, stripe_mm_reduce_kernel adds them
    // (round 5: several row tiles per sliced launch -- linear id = (slice * MT + row tile) * groups + group)
    const int bg = blockIdx.x / ngroups, mtn = a.MT > 1 ? a.MT : 1;
    const int sl = a.S > 1 ? bg / mtn : 0;
    const int mt = a.S > 1 ? bg % mtn : bg, cg = blockIdx.x % ngroups, m0 = mt * TR;
    const int cb = sl * a.span, ce = min(cb + a.span, a.nrb);
    const int rq = lane >> 4, col = lane & 15;
    const UnpackConsts uc = unpack_consts();
    const int nrb = a.nrb;

    // weight slots of this wave: two stripes, or {gate, up} of one
    int sstripe[NSW];
    const uint32_t *wbase[NSW], *tbase[NSW];
#pragma unroll
    for (int i = 0; i < NSW; i++) {
        const int st = NS == 1 ? cg * 8 + wc * 2 + i : cg * 4 + wc, set = NS == 1 ? 0 : i;
        sstripe[i] = st;
        const int sc = min(st, a.nstripes - 1);   // a ragged last group re-reads the last stripe and does not store it
        wbase[i] = a.R + (((size_t)sc * nrb * NS + set) * 64 + lane) * WPL;
        tbase[i] = a.tab + ((size_t)sc * NS + set) * a.G * 16 + col;
    }
    wvec_t w[PFW][NSW];
    uint32_t tw[PFW][NSW];
    auto wload = [&](int slot, int c) {
        const int rb = min(c, ce - 1);
        const int g = a.grp_shift >= 0 ? (rb >> a.grp_shift) : 0;
#pragma unroll
        for (int i = 0; i < NSW; i++) {
            w[slot][i] = *(const wvec_t *)(wbase[i] + (size_t)rb * NS * (64 * WPL));   // cacheable: the other row tiles read the same words
            tw[slot][i] = tbase[i][(size_t)g * 16];
        }
    };

    // x: rows m0 .. m0 + 127 through a buffer descriptor that ends with row M - 1
    const __amdgpu_buffer_rsrc_t xrs =
        __builtin_amdgcn_make_buffer_rsrc((void *)(a.x + (size_t)m0 * a.ldx), 0, (int)(((size_t)(a.M - m0 - 1) * a.ldx + a.K) * 2), 0x00020000);
    int ldx2 = a.ldx * 2;
    const int xvoff = (tid / PCR) * ldx2 + (tid % PCR) * 16;
    u32x4 xr[NXI];
    auto xload = [&](int c) {   // (past the last chunk: the last one again -- the K loop below is branch-free so that the counted vmcnt waits stay exact)
        const int cc = min(c, ce - 1);
#pragma unroll
        for (int i = 0; i < NXI; i++) xr[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, xvoff, (RPT * i) * ldx2 + cc * (BK * 2), 0));
    };
    auto xstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NXI; i++) *(u32x4 *)(xl + buf * XBUF + (tid / PCR + RPT * i) * XS + ((tid % PCR) ^ ((tid / PCR) & 3)) * 8) = xr[i];
    };

    float4_t yacc[NSW][RT];
#pragma unroll
    for (int i = 0; i < NSW; i++)
#pragma unroll
        for (int t = 0; t < RT; t++) yacc[i][t] = float4_t{0.f, 0.f, 0.f, 0.f};
    half2_t negoff[NOFFC];
#pragma unroll
    for (int o = 0; o < NOFFC; o++) negoff[o] = half2_t{(half_t)(-class_off(o)), (half_t)(-class_off(o))};

    // ---- prologue: weights of the first PFW chunks, x chunk 0 into LDS, x chunk 1 into registers ----
    // B fragments + scales of one chunk from its packed words: exact q - z (VALU only)
    auto unpack = [&](int j, bool valid, mm_h8_t (&B)[NSW][PPB], float2_t (&scale)[NSW]) {
#pragma unroll
        for (int i = 0; i < NSW; i++) {      // (hand-written dequant_block, with the prescale: see the note above mm_epilogue)
            const half2_t e = as_half2(tw[j][i]);
            const float sc1 = valid ? (float)e[0] : 0.f;   // chunks past K (clamped loads) carry a zero scale
            scale[i] = float2_t{sc1, sc1};
            const half2_t zz = {e[1], e[1]};
            half2_t cz[NOFFC];
#pragma unroll
            for (int o = 0; o < NOFFC; o++) cz[o] = negoff[o] - zz;   // -(OFF + zero + 1), exact
            uint32_t t32[NPB], d[NPB];
            unpack_block(w[j][i], uc, t32);
#pragma unroll
            for (int q = 0; q < NPB; q++) {
                half2_t v = as_half2(t32[q]) + cz[off_class(q)];   // q - z, exact
                if constexpr (PS) v = v * half2_t{valid ? e[0] : (half_t)0.f, valid ? e[0] : (half_t)0.f};   // ... times the group scale: one fp16 rounding
                d[q] = as_u32(v);
            }
#pragma unroll
            for (int b = 0; b < PPB; b++) B[i][b] = __builtin_bit_cast(mm_h8_t, u32x4{d[4 * b], d[4 * b + 1], d[4 * b + 2], d[4 * b + 3]});
        }
    };

    // ---- prologue.  The order mirrors the loop's steady state (per chunk c: x of c + 2, then weights of c + 1 + PFW) so that the
    // compiler's counted vmcnt waits at the loop header are the same on the entry edge and on the back edge.
    // (round 4: the ORDER must also survive the scheduler -- without the sched_barriers below it moved xload(cb + 1) behind the last weight
    // loads of the prologue, the entry edge then needed vmcnt(0) for x, and the merged wait at the loop header made every round of PFW chunks
    // wait for the weight loads it had just issued: found in the disassembly, s_waitcnt vmcnt(3..0) at the loop header instead of 7..4.
    // Measured effect of the fix: none (35.7 .. 76 us at 129 .. 2048 rows on 4096^2, same as before) -- x is the longer wait there anyway.)
    static_assert(PFW == 4, "prologue order below");
    wload(0, cb);
    wload(1, cb + 1);
    wload(2, cb + 2);
    xload(cb);
    __builtin_amdgcn_sched_barrier(0);
    mm_h8_t B[NSW][PPB];
    float2_t scale[NSW];
    if constexpr (!PS) {   // 128-row tiles: the B fragments of chunk c + 1 are unpacked while the MFMAs of chunk c run (256-row tiles have no
        wload(3, cb + 3);  // registers for a second set: they unpack at the top of their own chunk, under the partner wave's MFMAs)
        __builtin_amdgcn_sched_barrier(0);
        xstore(0);
        xload(cb + 1);
        __builtin_amdgcn_sched_barrier(0);
        unpack(0, true, B, scale);
        wload(0, cb + 4);           // steady state at the top of a chunk: x of the next chunk, then ONE slot of weights behind it
    } else {
        xstore(0);
        xload(cb + 1);
        __builtin_amdgcn_sched_barrier(0);
        wload(3, cb + 3);           // the same steady state for the 256-row tiles (their loop refills slot j after xload(c + 2))
    }
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();

    // No branch inside a round of PFW chunks: every load is issued unconditionally (clamped addresses) and chunks past K carry a zero
    // scale -- with `if (c < nrb)` guards the compiler's vmcnt bookkeeping falls back to vmcnt(0) at every join, i.e. every chunk waits
    // for the loads it has just issued.  The B fragments of chunk c + 1 are unpacked (VALU) while the MFMAs of chunk c run.
    for (int c0 = cb; c0 < ce; c0 += PFW) {      // (cb is a multiple of PFW: the LDS buffer parity c & 1 is the slice-relative one)
        asm volatile("" : "+s"(ldx2));   // recompute the row offsets per round instead of keeping them in SGPRs across the loop
#pragma unroll
        for (int j = 0; j < PFW; j++) {
            const int c = c0 + j, buf = c & 1, jn = (j + 1) % PFW;
            xstore(buf ^ 1);     // chunk c + 1: its buffer was last read in iteration c - 1 (barrier below)
            xload(c + 2);
            mm_h8_t Bn[PS ? 1 : NSW][PPB];
            float2_t scalen[NSW];
            if constexpr (PS) {
                unpack(j, c < ce, B, scale);
                wload(j, c + PFW);        // the slot's words are unpacked: refill it (clamped past K)
            } else {
                unpack(jn, c + 1 < ce, Bn, scalen);
                wload(jn, c + 1 + PFW);
            }
            const half_t *xa = xl + buf * XBUF + (wr * 16 * RT + col) * XS;   // piece rq PPB + b of a row sits at position (rq PPB + b) ^ (row & 3); row & 3 == col & 3
            if constexpr (PS) {
#pragma unroll
                for (int b = 0; b < PPB; b++) {   // PPB rounds of {RT A fragments, 2 RT independent MFMAs} straight into the result registers
                    mm_h8_t A[RT];
#pragma unroll
                    for (int t = 0; t < RT; t++) A[t] = *(const mm_h8_t *)(xa + t * 16 * XS + 8 * ((rq * PPB + b) ^ (col & 3)));
#pragma unroll
                    for (int t = 0; t < RT; t++)
#pragma unroll
                        for (int i = 0; i < NSW; i++) yacc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[t], B[i][b], yacc[i][t], 0, 0, 0);
                }
            } else {
                float4_t acc[NSW][RT];
#pragma unroll
                for (int i = 0; i < NSW; i++)
#pragma unroll
                    for (int t = 0; t < RT; t++) acc[i][t] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int b = 0; b < PPB; b++) {   // PPB rounds of {RT A fragments, 2 RT independent MFMAs}
                    mm_h8_t A[RT];
#pragma unroll
                    for (int t = 0; t < RT; t++) A[t] = *(const mm_h8_t *)(xa + t * 16 * XS + 8 * ((rq * PPB + b) ^ (col & 3)));
#pragma unroll
                    for (int t = 0; t < RT; t++)
#pragma unroll
                        for (int i = 0; i < NSW; i++) acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[t], B[i][b], acc[i][t], 0, 0, 0);
                }
#pragma unroll
                for (int i = 0; i < NSW; i++)
#pragma unroll
                    for (int t = 0; t < RT; t++) {   // group scale on the fp32 accumulator (v_pk_fma_f32)
                        const float2_t lo = __builtin_elementwise_fma(scale[i], float2_t{acc[i][t][0], acc[i][t][1]}, float2_t{yacc[i][t][0], yacc[i][t][1]});
                        const float2_t hi = __builtin_elementwise_fma(scale[i], float2_t{acc[i][t][2], acc[i][t][3]}, float2_t{yacc[i][t][2], yacc[i][t][3]});
                        yacc[i][t] = float4_t{lo[0], lo[1], hi[0], hi[1]};
                    }
            }
            if constexpr (!PS) {
#pragma unroll
                for (int i = 0; i < NSW; i++) {
                    scale[i] = scalen[i];
#pragma unroll
                    for (int b = 0; b < PPB; b++) B[i][b] = Bn[i][b];
                }
            }
            __syncthreads();
            __builtin_amdgcn_sched_barrier(0);   // no code motion across chunks: longer live ranges spill, and a scratch reload waits with vmcnt(0)
        }
    }

    if (a.S > 1) {   // this slice's fp32 sums in the layout stripe_mm_reduce_kernel<2 RT, NS> reads: [row tile of 128][group][slice][stripe in group][set][row tile][lane][4]
        constexpr int TMW = 2 * RT, TILE = NS * TMW * 256;
#pragma unroll
        for (int i = 0; i < NSW; i++) {
            const int sig = NS == 1 ? wc * 2 + i : wc, set = NS == 1 ? 0 : i;
            float *dst = a.partials + (((size_t)(mt * ngroups + cg) * a.S + sl) * STRIPE_NW + sig) * TILE + (size_t)set * TMW * 256 + lane * 4;
#pragma unroll
            for (int t = 0; t < RT; t++) *(float4_t *)(dst + (wr * RT + t) * 256) = yacc[i][t];
        }
        return;
    }
    // ---- epilogue: lane = column, rows 4 rq + r of each row tile (hand-written finish_tile: see the note above mm_epilogue) ----
#pragma unroll
    for (int i = 0; i < (NS == 1 ? NSW : 1); i++) {
        if (sstripe[i] >= a.nstripes) continue;
        const int n = sstripe[i] * 16 + col;
        const float bv = (a.bias && !a.ldb) ? (float)a.bias[n] : 0.f;
#pragma unroll
        for (int t = 0; t < RT; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = m0 + wr * 16 * RT + 16 * t + 4 * rq + r;
                float v = yacc[i][t][r];
                if constexpr (NS == 2) {
                    const float u = yacc[1][t][r];
                    v = v * (1.0f / (1.0f + __expf(-v))) * u;   // silu on the fp32 accumulator (fused_mlp.py:160-164)
                }
                if (row < a.M) {
                    half_t h = (half_t)v;
                    if (a.bias) h = (half_t)((float)h + (a.ldb ? (float)a.bias[(size_t)row * a.ldb + n] : bv));
                    a.y[(size_t)row * a.ldy + n] = h;
                }
            }
    }
}

template <int NS, int RT>
int stripe_gemm_launch(const StripeParams &p, int grp_shift, hipStream_t s) {
    auto kern = stripe_gemm_kernel<NS, RT>;
    constexpr size_t lds = sg_lds_bytes(RT);
    static LdsOptIn opt_in;
    if (int rc = opt_in.ensure((const void *)kern, lds)) return rc;
    MMArgs a{};
    a.x = p.x; a.R = p.R; a.tab = p.tab; a.y = p.y; a.bias = p.bias; a.ldb = (int)p.ldb;
    a.K = p.K; a.nrb = p.K / BK; a.G = p.G; a.grp_shift = grp_shift; a.M = p.M; a.ldx = (int)p.ldx; a.ldy = (int)p.ldy;
    a.nstripes = p.N / 16; a.S = 1; a.span = a.nrb;
    const int spg = NS == 1 ? 8 : 4, ngroups = (a.nstripes + spg - 1) / spg, mtiles = (p.M + 32 * RT - 1) / (32 * RT);
    hipLaunchKernelGGL(kern, dim3(ngroups * mtiles), dim3(STRIPE_NW * 64), lds, s, a);
    return (int)hipGetLastError();
}

// Batches of up to 128 rows whose column groups (128 columns each) cover only a part of the chip: K slices of the 128-row tile GEMM, one
// round of workgroups, fp32 partial tiles + stripe_mm_reduce_kernel (summed in slice order: bit-reproducible).  Round 4: the K-slice kernel
// of the 16-row tiles stages its whole x slice in LDS, which forces 4 / 8 slices at 64 / 128 rows (768 workgroups + 50 MB of partials at
// 4096 x 12288: 24 / 41 us); here x streams through the 2 x 33 KB double buffer, so the slice count follows the chip, not LDS.
// (inside the anonymous namespace like every launcher of this file: the four bit-width translation units each need THEIR instance)
template <int NS>
int stripe_gemm_sliced_launch(const StripeParams &p, int grp_shift, void *ws, size_t ws_bytes, int forced_slices, hipStream_t s) {
    static_assert(NS == 1, "the reduce kernel's column group is 8 stripes of ONE set");
    constexpr int RT = 4, TMW = 2 * RT;
    auto kern = stripe_gemm_kernel<NS, RT>;
    constexpr size_t lds = sg_lds_bytes(RT);
    const int nrb = p.K / BK, nstripes = p.N / 16, spg = NS == 1 ? 8 : 4, ngroups = (nstripes + spg - 1) / spg;
    // round 5: batches of SEVERAL 128-row tiles whose tiles cover at most half the chip (N = 4096 up to 512 rows: 32 column groups x 4 row tiles) are
    // sliced too -- one launch, row tile x group x slice workgroups, the reduce kernel walks the row tiles; before, 256 x 4096 x 11008 ran 64 workgroups
    // over the whole K each (87.7 us against 81.9 for the library, the one cell of the prompt table below it: profiles/r5e_gemm8_tile/)
    const int mtiles = (p.M + 32 * RT - 1) / (32 * RT);
    // (the limit of 128 tiles was swept, profiles/r5e_gemm8_tile/image_route_k_slices_tile_limit_128_192_256.txt: with 129 .. 256 tiles two slices are
    // SLOWER than none -- 4096 x 12288 at 129 .. 256 rows 48-50 us against 39, 4096^2 at 640 rows 48 against 38)
    constexpr int mt_tiles = 128;
    if (nrb < 2 * SG_PFW || (mtiles > 1 && (mtiles * ngroups > mt_tiles || forced_slices > 0))) return GPTQ_E_VARIANT;
    int S = forced_slices > 0 ? forced_slices : std::max(2, 256 / (ngroups * mtiles));     // at most ONE round of workgroups (a partial second round costs a whole one)
    int span = ((nrb + S - 1) / S + SG_PFW - 1) / SG_PFW * SG_PFW;                                // whole rounds of PFW chunks per slice
    S = (nrb + span - 1) / span;
    if (S < 2) return GPTQ_E_VARIANT;
    const size_t part_bytes = (size_t)mtiles * ngroups * S * STRIPE_NW * NS * TMW * 256 * 4;
    if (!ws || ws_bytes < part_bytes) return GPTQ_E_WORKSPACE;
    static LdsOptIn opt_in;
    if (int rc = opt_in.ensure((const void *)kern, lds)) return rc;
    MMArgs a{};
    a.x = p.x; a.R = p.R; a.tab = p.tab; a.y = p.y; a.bias = p.bias; a.ldb = (int)p.ldb;
    a.partials = (float *)ws;
    a.K = p.K; a.nrb = nrb; a.G = p.G; a.grp_shift = grp_shift; a.M = p.M; a.ldx = (int)p.ldx; a.ldy = (int)p.ldy;
    a.nstripes = nstripes; a.S = S; a.span = span; a.MT = mtiles;
    hipLaunchKernelGGL(kern, dim3(mtiles * ngroups * S), dim3(STRIPE_NW * 64), lds, s, a);
    hipLaunchKernelGGL((stripe_mm_reduce_kernel<TMW, NS>), dim3(mtiles * ngroups * TMW), dim3(STRIPE_NW * 64), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace

#define STRIPE_CAT2(a, b) a##b
#define STRIPE_CAT(a, b) STRIPE_CAT2(a, b)
// any M >= 1 (meant for M > 128); GPTQ_E_VARIANT when the layer is not eligible: groups smaller than a row block, 2-bit (its 256-k row
// block does not fit two LDS buffers next to each other comfortably), batches whose addresses do not fit the 32-bit buffer offsets
int STRIPE_CAT(stripe_gemm_dispatch_b, STRIPE_BITS)(const StripeParams &p, void *ws, size_t ws_bytes, hipStream_t s) {
    if (p.M < 1 || p.norm_w || p.xperm || p.y32 || SB == 2) return GPTQ_E_VARIANT;
    if ((int64_t)p.M * p.ldx + p.K >= (int64_t)1 << 30) return GPTQ_E_VARIANT;
    int grp_shift = -1;
    if (p.gq_shift >= 0) {
        if (p.gq_shift < 2) return GPTQ_E_VARIANT;   // group smaller than a row block
        grp_shift = p.gq_shift - 2;
    }
    const int spg = p.NS == 1 ? 8 : 4, ngroups = (p.N / 16 + spg - 1) / spg;
    // K slices over several row tiles while the tiles cover at most half the chip (stripe_gemm_sliced_launch declines otherwise): profiles/r5e_gemm8_tile/
    if constexpr (SB != 2) {
        if (p.NS == 1 && p.M > 128 && ws) {
            const int rc = stripe_gemm_sliced_launch<1>(p, grp_shift, ws, ws_bytes, -1, s);
            if (rc != GPTQ_E_VARIANT && rc != GPTQ_E_WORKSPACE) return rc;
        }
    }
    // 256-row tiles where they need less time in whole rounds of workgroups over the 256 CUs: a 256-row tile costs 1.75 x a 128-row tile
    // (profiles/r3g_mid_m/stripe_gemm_tile_rows.txt: 66-70 us against 36-40 us per round at K = 4096)
    const int64_t r4 = ((int64_t)ngroups * ((p.M + 127) / 128) + 255) / 256, r8 = ((int64_t)ngroups * ((p.M + 255) / 256) + 255) / 256;
    if (7 * r8 < 4 * r4) return p.NS == 2 ? stripe_gemm_launch<2, 8>(p, grp_shift, s) : stripe_gemm_launch<1, 8>(p, grp_shift, s);
    // 128-row tiles: everything else
    return p.NS == 2 ? stripe_gemm_launch<2, 4>(p, grp_shift, s) : stripe_gemm_launch<1, 4>(p, grp_shift, s);
}


// 1 <= M <= 128 (65 .. 128 rows: round 3, six / eight row tiles on the same B fragments -- the weights are streamed and unpacked ONCE for
// all of them instead of once per 64-row pass); GPTQ_E_VARIANT when the shape is not eligible (the caller falls back), GPTQ_E_WORKSPACE when the partial tiles
// do not fit.  ws: scratch for the partial tiles (no state survives a launch).
int STRIPE_CAT(stripe_mm_dispatch_b, STRIPE_BITS)(const StripeParams &p, void *ws, size_t ws_bytes, int forced_slices, hipStream_t s) {
    if (p.M < 1 || p.M > 128 || p.norm_w || p.xperm || p.y32) return GPTQ_E_VARIANT;
    if ((int64_t)p.M * p.ldx + p.K >= (int64_t)1 << 30) return GPTQ_E_VARIANT;
    int grp_shift = -1;
    bool ps = false;
    if (p.gq_shift >= 0) {
        if (p.gq_shift < 2) ps = true;            // group smaller than a row block: prescale kernels
        else grp_shift = p.gq_shift - 2;          // BK = 4 LK
    }
    // the facts the routes share.  An ordered list: the first route whose predicate holds (and whose launcher does not decline) runs.
    // What each route was measured against, and the forms that were built and removed: DESIGN 3.3a.
    const int tm = (p.M + 15) / 16;                    // row tiles of 16
    const int cw = (p.N / 16 + 255) / 256;             // rounds of stripes over the 256 CUs = adjacent stripes per workgroup of the C-stripe kernels
    const bool auto_slices = forced_slices < 0;        // the caller pins no slice count (gptq_set_split_k)
    const bool x_aligned = p.K % BK == 0 && (uintptr_t)p.x % 16 == 0 && p.ldx % 8 == 0;      // LDS-DMA of whole 16-byte pieces of x
    const bool one_round_short_k = p.N / 16 <= 256 && p.K <= 6144;
    const bool c_stripes = !ps && auto_slices && p.K <= 6144 && (cw == 2 || cw == 3);         // what the C-stripes-per-workgroup routes share

    if constexpr (SB == 4) {
        // loader / consumer split, 17 .. 128 rows on shapes with two or three rounds of stripes, K <= 8192 (8192 x 8192 from 96 rows on loses: 6144 there).
        // profiles/r6s_mmr/, r6x_mmr_tm7/, r6y_mmr_halves/
        if (!ps && auto_slices && x_aligned && p.NS == 1 && tm >= 2 && tm <= 8 && (cw == 2 || cw == 3) && p.K <= (tm >= 6 ? 6144 : 8192))
            return cw == 2 ? stripe_mmr_dispatch<2>(tm, p, grp_shift, s) : stripe_mmr_dispatch<3>(tm, p, grp_shift, s);
        // the same kernel in four K slices of four stripes: one round of stripes with a long K (LLaMA-7B down_proj, 11008 x 4096).  profiles/r7g_mmr_kslices/
        const int nst = p.N / 16;
        if (!ps && auto_slices && x_aligned && p.NS == 1 && tm >= 2 && tm <= 8 && nst > 192 && nst <= 256 && p.K > 6144 && p.K <= 16384 && ws) {
            const int rc = stripe_mmr_sliced_dispatch(tm, 4, p, grp_shift, ws, ws_bytes, s);
            if (rc != GPTQ_E_VARIANT && rc != GPTQ_E_WORKSPACE) return rc;
        }
        // the gate | up pair on the loader / consumer kernel, 17 .. 128 rows.  Eight row tiles of three stripes would spill: rows 0 .. 63 and 64 .. M - 1 as TWO
        // launches of the four-tile instance (the second reads the weights out of the Infinity Cache).  profiles/r6z_pair/, r7e_pair_two_launches/
        if (c_stripes && x_aligned && p.NS == 2 && tm >= 2 && tm <= 8) {
            if (tm == 8 && cw == 3) {
                StripeParams lo = p, hi = p;
                lo.M = 64;
                hi.M = p.M - 64; hi.x = p.x + 64 * p.ldx; hi.y = p.y + 64 * p.ldy;
                if (p.bias && p.ldb) hi.bias = p.bias + 64 * p.ldb;
                const int rc = stripe_mmr_pair_dispatch<3>(4, lo, grp_shift, s);
                return rc ? rc : stripe_mmr_pair_dispatch<3>((hi.M + 15) / 16, hi, grp_shift, s);
            }
            return cw == 2 ? stripe_mmr_pair_dispatch<2>(tm, p, grp_shift, s) : stripe_mmr_pair_dispatch<3>(tm, p, grp_shift, s);
        }
    }
    if constexpr (SB == 4 || SB == 3) {
        // four-wave instances of the wave-private kernel (512 registers per wave): 33 .. 64 rows on shapes with two or three rounds of stripes, .. 96 rows with two.
        // profiles/r4l_w4/, r4n_w4pf/
        if (c_stripes && p.NS == 1 && ((cw == 2 && tm >= 3 && tm <= 6) || (cw == 3 && (tm == 3 || tm == 4))))
            return cw == 2 ? stripe_mm3w4_dispatch<2>(tm, p, grp_shift, s) : stripe_mm3w4_dispatch<3>(tm, p, grp_shift, s);
        // cw adjacent stripes per workgroup on the same staged x, one and two row tiles.  profiles/r4f_mm3c/
        if (c_stripes && p.NS == 1 && tm <= 2)
            return cw == 2 ? stripe_mm3c_dispatch<2>(tm, p, grp_shift, s) : stripe_mm3c_dispatch<3>(tm, p, grp_shift, s);
    }
    if constexpr (SB == 4) {
        // the gate | up pair at one row tile (5 .. 16 rows of a decode batch), cw stripes per workgroup: the single-launch pair kernel re-reads x per stripe.
        // DESIGN 3.8
        if (c_stripes && p.NS == 2 && tm == 1)
            return cw == 2 ? stripe_mm3c_pair_dispatch<2>(tm, p, grp_shift, s) : stripe_mm3c_pair_dispatch<3>(tm, p, grp_shift, s);
    }
    if constexpr (SB != 2) {
        // K slices of the 128-row fused tile GEMM from 65 rows on, where one round of stripes does not cover N or K is long (4096 x 4096 stays with the
        // wave-private kernel: 14.7 us at 128 rows); a forced slice count >= 1 is passed through.  profiles/r4g_sgs/
        if (!ps && p.NS == 1 && forced_slices != 0 && tm >= 5 && !one_round_short_k) {
            const int rc = stripe_gemm_sliced_launch<1>(p, grp_shift, ws, ws_bytes, forced_slices, s);
            if (rc != GPTQ_E_VARIANT && rc != GPTQ_E_WORKSPACE) return rc;
        }
    }
    // wave-private staging (stripe_mm3_kernel): it re-reads x once per stripe, so it runs where ONE round of workgroups covers N and K is short, and at
    // 65 .. 96 rows elsewhere.  8-bit: the instances beyond four row tiles / the pair beyond one would spill.  profiles/r3g_mid_m/mm3_ab.txt
    const bool mm3_can = !ps && auto_slices && (p.NS == 1 ? tm <= (SB == 8 ? 4 : 8) : tm <= (SB == 8 ? 1 : 2));
    if (mm3_can && (one_round_short_k || (p.NS == 1 && (tm == 5 || tm == 6) && SB != 8)))
        return p.NS == 2 ? stripe_mm3_dispatch<2>(tm, p, grp_shift, s) : stripe_mm3_dispatch<1>(tm, p, grp_shift, s);
    // one launch (a stripe x whole K per workgroup, x streamed through LDS) for up to 32 rows while that is one round of workgroups over the 256 CUs and K
    // is short, or when the caller asks for it (forced_slices == 0); 4 / 8 bits with groups of at least a row block.  profiles/r2c_mm/slices.txt
    constexpr bool has_single = SB == 4 || SB == 8;
    const bool single = has_single && !ps && (forced_slices == 0 || (auto_slices && p.K <= 6144 && ((tm == 1 && p.N / 16 <= 1024) || (tm == 2 && p.N / 16 <= 288))));
    if constexpr (has_single) {
        if (single) {
            int rc;
            if (p.NS == 2) {
                switch (tm) {
                    // (PF = 4, one workgroup per CU: the pair instance with PF = 2 spilled 208 B per lane, profiles/r2d_final/kernel_resources.txt)
                    case 1: rc = stripe_mm1_launch<1, 2, 4>(p, grp_shift, s); break;
                    case 2: rc = stripe_mm2_launch<2, 2>(p, grp_shift, s); break;
                    case 3: rc = stripe_mm2_launch<3, 2>(p, grp_shift, s); break;
                    default: rc = stripe_mm2_launch<4, 2>(p, grp_shift, s); break;
                }
            } else {
                switch (tm) {
                    case 1: rc = stripe_mm1_launch<1, 1, 2>(p, grp_shift, s); break;
                    case 2: rc = stripe_mm2_launch<2, 1>(p, grp_shift, s); break;
                    case 3: rc = stripe_mm2_launch<3, 1>(p, grp_shift, s); break;
                    default: rc = stripe_mm2_launch<4, 1>(p, grp_shift, s); break;
                }
            }
            if (rc != GPTQ_E_VARIANT || forced_slices == 0) return rc;   // a table too large for the LDS-DMA stages: K slices instead
        }
    }
    // everything else: K slices + the reduce kernel (forced_slices >= 1: that many)
    const int fs = forced_slices == 0 ? -1 : forced_slices;
#define MM_SPLIT(TMV, NSV) (ps ? stripe_mm_launch<TMV, NSV, true>(p, grp_shift, ws, ws_bytes, fs, s) : stripe_mm_launch<TMV, NSV, false>(p, grp_shift, ws, ws_bytes, fs, s))
    if (p.NS == 2) {
        switch (tm) {
            case 1: return MM_SPLIT(1, 2);
            case 2: return MM_SPLIT(2, 2);
            case 3: return MM_SPLIT(3, 2);
            case 4: return MM_SPLIT(4, 2);
            default: return GPTQ_E_WORKSPACE;   // the pair kernel with 6 / 8 row tiles spills (2 x 8 accumulator tiles + their per-row-block
                                                // twins): the caller runs 64-row passes
        }
    }
    switch (tm) {
        case 1: return MM_SPLIT(1, 1);
        case 2: return MM_SPLIT(2, 1);
        case 3: return MM_SPLIT(3, 1);
        case 4: return MM_SPLIT(4, 1);
        case 5: case 6: return MM_SPLIT(6, 1);
        default: return MM_SPLIT(8, 1);
    }
#undef MM_SPLIT
}

}  // namespace gptq
