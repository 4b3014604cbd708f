// stripe_kernel.inc -- the stripe16 decode kernel for ONE bit width; included by stripe_b2.hip / stripe_b4.hip / stripe_b8.hip with
// STRIPE_BITS defined (three translation units so that `make -j` builds the ~600 instantiations in parallel).
// Layout, schedule and measurements: stripe.hip (header) and DESIGN.md 3.1.
#include "attn_split.h"
#include "gptq_device.h"
#include "gptq_internal.h"
#include "stripe_common.h"

namespace gptq {

namespace {

#include "stripe_unpack.inc"

// NS = 2: y = silu(x Wg) * (x Wu) (fused_mlp.py:160-166).  NORM: x is RMS-normalised while it is staged.  XPERM: x is gathered through
// a permutation (act-order layer whose rows were sorted by group at load time).  MR = 4: up to four rows of x (M = 2..4), row
// stride ldx / ldy; MR = 8 / 16: two / four MFMA row groups on the same unpacked words (as long as MR rows of x fit in LDS);
// XPERM is an M = 1 feature, y32 serves M <= 4; NORM (one rstd per row) and a per-row residual (ldb != 0) serve every MR since round 5 (the
// batched decode engine).  gq_shift = log2(groupsize / LK), or -1 for a single group.
// ATT (round 6): x is not an fp16 row but the decode attention's split records -- {M, den} per (split, head) and fp32 numerators per (split, k),
// attn_split.h -- of up to ATT_MAX_SPLITS splits; this kernel (o_proj of a batch-1 decode step) merges them while it stages x: the kernel boundary is
// the attention's cross-workgroup hand-off, its ticket + last-arriver merge (5.5 us per layer from 129 tokens of context on) is gone.  The number of
// active splits follows from the row's position exactly as in the producer (attn_split); slots past it re-read the last record and get weight 0.
template <int NU, int NS, int DU, bool NORM, bool XPERM, int MR, bool ATT = false>
__global__ void __launch_bounds__(STRIPE_NW * 64) stripe_gemv_kernel(const half_t *__restrict__ x, const uint32_t *__restrict__ R,
                                                                     const uint32_t *__restrict__ tab, half_t *__restrict__ y, int K, int nrb, int G,
                                                                     int gq_shift, const half_t *__restrict__ bias, const half_t *__restrict__ nw,
                                                                     float eps, const uint16_t *__restrict__ xperm, float *__restrict__ y32, int M,
                                                                     int ldx, int ldy, uint32_t *progress, int ldb, const int32_t *__restrict__ yperm,
                                                                     const AttnMerge am) {
    static_assert(!ATT || (MR == 1 && NS == 1 && !NORM && !XPERM), "the record merge serves the plain one-row launch");
    typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
    constexpr int NW = STRIPE_NW, T = NW * 64;
    // progress tick (debug hook gptq_set_progress_counter): ONE fire-and-forget device-scope add per launch, before anything is in flight --
    // what the run-ahead prefetcher of tools/warmlab.hip paces itself on (a measured negative result, DESIGN 3.6); NULL in the product
    if (progress != nullptr && blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_fetch_add(progress, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    constexpr int XP = (NU * NW * BK / 8 + T - 1) / T;   // 16-byte pieces of one x row per thread (K <= NU * NW * BK)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int xstride = MR > 1 ? K + 8 : K;              // halves; MR > 1: 16 bytes of padding -> the four rows sit on different banks
    half_t *xl = (half_t *)smem;                                                              // [MR][xstride] (normalised) x
    float2 *xs4 = (float2 *)(smem + (size_t)MR * xstride * 2);                                // [MR][K / LK] {sum x OFF_k, sum x}
    float2 *tabf = xs4 + (size_t)MR * (K / LK);                                               // [NS][G][16] {s, -(z + 1) s}
    float *red = (float *)(tabf + (size_t)NS * G * 16);                                       // [NW][NS][MR][16], also the norm partials; XPERM: + raw x [K]
    half_t *xraw = (half_t *)(red + STRIPE_NW * NS * MR * 16);                                // XPERM only: (normalised) x in natural order
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int stripe = blockIdx.x;
    const half2_t ones = {(half_t)1.f, (half_t)1.f};
    const UnpackConsts uc = unpack_consts();
    const int npieces = K / 8, ntab = NS * G * 4;   // 16-byte pieces of an x row / of this stripe's table

    // ---- 1. x (+ norm weight) and the first table piece: requested BEFORE the weights (vector loads return in order) ----
    // XPW (round 3): act-order with 32 k per lane block (3 / 4 bits): the permutation does NOT gate the staging any more.  It is as cold as
    // the weights (8-22 KB per layer), vector loads return in order, and the cooperative gather + per-block sums (work that grows with K) used
    // to start only when that cold load had arrived: + 0.35 us at K = 4096, + 1.3 us at K = 11008 over the trivial-g_idx kernel
    // (tools/act_order_probe.py; the gather PATTERN is irrelevant).  Now x is parked raw, the indices of a wave's row blocks are requested
    // right behind x, and the wave gathers the 128 k' of a row block it owns inside the K loop, in consumption order.
    constexpr bool XPW = XPERM && LK == 32;
    u32x4 xv[MR][XP], nv[NORM ? XP : 1], pv[(XPERM && !XPW) ? XP : 1], tv0;   // pv: eight uint16 source indices per piece of x
    // ATT: the records of this thread's pieces -- per split two 16-byte loads of numerators and the {M, den} of the piece's head
    u32x4 an[ATT ? XP : 1][ATT ? ATT_MAX_SPLITS : 1];
    float2 amd[ATT ? XP : 1][ATT ? ATT_MAX_SPLITS : 1];
    int att_nsp = 1;
    bool att_idle = false;
    int64_t att_pos = 0;
    if constexpr (ATT) {
        // the row's position through the SCALAR cache (constant address space: nothing in this launch writes it, and a launch starts with the
        // scalar cache invalidated; as a plain load hipcc made it a vector load + vmcnt(0)).  Requested first, needed only for splits 1 .. 3 below.
        att_pos = *(const __attribute__((address_space(4))) int64_t *)am.pos;
    }
#pragma unroll
    for (int i = 0; i < XP; i++) {
        const int idx = min(tid + i * T, npieces - 1);   // clamped, not branched: a branch in the load phase costs a vmcnt(0)
        if constexpr (ATT) {
            // split 0 always exists: its record is requested without waiting for the position -- at a short context (one split) this launch
            // costs what the plain one does (the record IS the fp16 row, + {M, den} of the piece's head).  (Re-reading the last record for the
            // inactive slots was measured first, with fp32 records: L1 hits, but 48 KB more through the CU's 64 B / clk load path = + 0.45 us.)
            an[i][0] = *(const u32x4 *)(am.o16 + (size_t)idx * 8);
            amd[i][0] = *(const float2 *)(am.md + (size_t)(idx >> 4) * 2);
#pragma unroll
            for (int sp = 1; sp < ATT_MAX_SPLITS; sp++) {
                an[i][sp] = u32x4{0u, 0u, 0u, 0u};
                amd[i][sp] = float2{ATT_M_FLOOR, 0.f};
            }
        } else {
#pragma unroll
        for (int m = 0; m < MR; m++) xv[m][i] = *(const u32x4 *)(x + (size_t)min(m, M - 1) * ldx + (size_t)idx * 8);
        }
        if constexpr (NORM) nv[i] = *(const u32x4 *)(nw + (size_t)idx * 8);
        if constexpr (XPERM && !XPW) {
            pv[i] = *(const u32x4 *)(xperm + (size_t)idx * 8);
        }
    }
    // XPW: the source indices of this wave's row blocks -- k' = 128 rb + 2 lane, + 1: one dword per lane, 256 contiguous bytes per wave and
    // row block -- cold like the table and the weights, but FIRST in the return order
    uint32_t pw[XPW ? NU : 1];
    if constexpr (XPW) {
#pragma unroll
        for (int u = 0; u < NU; u++) pw[u] = *((const uint32_t *)xperm + (size_t)min(wave + STRIPE_NW * u, nrb - 1) * (BK / 2) + lane);
    }
    const uint32_t *tsrc = tab + (size_t)stripe * NS * G * 16;
    tv0 = *(const u32x4 *)(tsrc + (size_t)min(tid, ntab - 1) * 4);
    // the bias / residual of this thread's output column is requested NOW, ahead of the weight stream (loads return in order), not
    // in the epilogue where its L2 round trip (~0.7 us on the engine's o_proj / down_proj + residual launches) would be the last
    // thing the launch waits for.  No branch in the load phase: without a bias the address is x (always valid), the value unused.
    // ldb != 0 (round 5, batched decode): `bias` is a [M][ldb] residual -- thread (m, c) of the epilogue takes row m of it
    const half_t bias_pre = *((bias ? bias + (size_t)min(tid >> 4, M - 1) * ldb + (size_t)stripe * 16 : x) + (tid & 15));
    // yperm (round 5): the CONSUMER of y is an act-order layer whose image holds group-sorted rows -- column n of y is written where that layer's
    // sorted order wants it (its inverse permutation), so the consumer runs the trivial kernel instead of gathering x per launch.  Requested here,
    // ahead of the weight stream, like the bias.
    const int ycol = yperm ? yperm[stripe * 16 + (tid & 15)] : stripe * 16 + (tid & 15);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (ATT) {   // the records of the further splits of a long context (wave-uniform branches; the position has arrived under the loads above)
        att_idle = att_pos < 0;
        const int alen = (int)(att_pos < 0 ? 0 : (att_pos >= am.t_max ? am.t_max - 1 : att_pos)) + 1;
        att_nsp = attn_split(alen, am.S, am.tps).nsp;
#pragma unroll
        for (int sp = 1; sp < ATT_MAX_SPLITS; sp++) {
            if (sp < att_nsp) {
#pragma unroll
                for (int i = 0; i < XP; i++) {
                    const int idx = min(tid + i * T, npieces - 1);
                    an[i][sp] = *(const u32x4 *)(am.o16 + (size_t)sp * K + (size_t)idx * 8);
                    amd[i][sp] = *(const float2 *)(am.md + ((size_t)sp * am.heads + (idx >> 4)) * 2);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }

    // ---- 2. the first DU row blocks of this wave ----
    typedef uint32_t wvec_t __attribute__((ext_vector_type(WPL)));   // dwordx4, or dwordx3 for 3-bit
    wvec_t w[NU][NS];
    const uint32_t *wbase = R + ((size_t)stripe * nrb * NS * 64 + lane) * WPL;
    auto issue = [&](int u) {
        const int rb = min(wave + NW * u, nrb - 1);   // ragged tail: re-read the last block (its table entry is zeroed below)
#pragma unroll
        for (int s = 0; s < NS; s++) w[u][s] = __builtin_nontemporal_load((const wvec_t *)(wbase + ((size_t)rb * NS + s) * (64 * WPL)));
    };
#pragma unroll
    for (int u = 0; u < (DU < NU ? DU : NU); u++) issue(u);
    __builtin_amdgcn_sched_barrier(0);

    // ---- 3. stage x, the per-lane-block sums and the table in LDS ----
    if constexpr (ATT) {   // x = fp16(sum_s c_s o_s): the arithmetic of the in-kernel merge (attn_split.h), bit for bit
#pragma unroll
        for (int i = 0; i < XP; i++) {
            float m4[ATT_MAX_SPLITS], d4[ATT_MAX_SPLITS], c4[ATT_MAX_SPLITS];
#pragma unroll
            for (int sp = 0; sp < ATT_MAX_SPLITS; sp++) {
                m4[sp] = amd[i][sp].x;
                d4[sp] = amd[i][sp].y;
            }
            if (att_nsp > 1) {        // (wave-uniform; one split: its record is the row)
                attn_merge_coeffs(m4, d4, att_nsp, c4);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    half_t e[2];
#pragma unroll
                    for (int hh = 0; hh < 2; hh++) {
                        half_t o4[ATT_MAX_SPLITS];
#pragma unroll
                        for (int sp = 0; sp < ATT_MAX_SPLITS; sp++) {
                            const uint32_t word = an[i][sp][q];      // (through a scalar: see the note on __builtin_bit_cast below)
                            o4[sp] = as_half2(word)[hh];
                        }
                        e[hh] = attn_round_f16(attn_merge_value(o4, c4));
                    }
                    xv[0][i][q] = as_u32(half2_t{e[0], e[1]});
                }
            } else {
                xv[0][i] = an[i][0];
            }
            // an idle row of the batch (negative position): its records are stale -- x = 0, the result is nobody's
            if (att_idle) xv[0][i] = u32x4{0u, 0u, 0u, 0u};
            // (hipcc 7.2: __builtin_bit_cast applied DIRECTLY to a vector-element lvalue -- __builtin_bit_cast(float, v[i][j]) -- reads element 0
            // whatever the index; go through a scalar copy)
        }
    }
    if constexpr (NORM) {
        // one rstd per row of x (round 5: MR > 1 -- a decode batch keeps the norm fused; the arithmetic per row is rms_norm_fwd_fused's)
        float ss[MR];
#pragma unroll
        for (int m = 0; m < MR; m++) {
            ss[m] = 0.f;
#pragma unroll
            for (int i = 0; i < XP; i++) {
                if (tid + i * T < npieces) {
#pragma unroll
                    for (int q = 0; q < 4; q++) ss[m] = __builtin_amdgcn_fdot2(as_half2(xv[m][i][q]), as_half2(xv[m][i][q]), ss[m], false);
                }
            }
            ss[m] = wave_sum_all(ss[m]);
            if (lane == 0) red[wave * MR + m] = ss[m];
        }
        __syncthreads();
        // (no second barrier: red is written again only after the staging barrier below, which every wave reaches after these reads)
#pragma unroll
        for (int m = 0; m < MR; m++) {
            float tot = 0.f;
#pragma unroll
            for (int wv = 0; wv < NW; wv++) tot += red[wv * MR + m];
            const float rstd = 1.0f / sqrtf(tot / (float)K + eps);
#pragma unroll
            for (int i = 0; i < XP; i++) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const half2_t a = as_half2(xv[m][i][q]), b = as_half2(nv[i][q]);
                    const half2_t r = {(half_t)((float)a[0] * rstd * (float)b[0]), (half_t)((float)a[1] * rstd * (float)b[1])};
                    xv[m][i][q] = as_u32(r);
                }
            }
        }
    }
    if constexpr (XPERM) {
        // (normalised) x in natural order -> LDS; gathered through the permutation from there: random access stays on chip
#pragma unroll
        for (int i = 0; i < XP; i++) {
            const int idx = tid + i * T;
            if (idx < npieces) *(u32x4 *)(xraw + (size_t)idx * 8) = xv[0][i];
        }
        if constexpr (!XPW) {   // cooperative gather of the whole row before the K loop (widths whose lane block is not 32 k)
            __syncthreads();
#pragma unroll
            for (int i = 0; i < XP; i++) {
                half_t e[8];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    e[2 * q] = xraw[pv[i][q] & 0xFFFFu];
                    e[2 * q + 1] = xraw[pv[i][q] >> 16];
                }
#pragma unroll
                for (int q = 0; q < 4; q++) xv[0][i][q] = as_u32(half2_t{e[2 * q], e[2 * q + 1]});
            }
        }
    }
    if constexpr (!XPW) {   // (XPW: the K loop below stages what it needs; the barrier after the table covers the raw row)
#pragma unroll
    for (int i = 0; i < XP; i++) {
        const int idx = tid + i * T;
        // offsets of this piece's four pairs: pairs 4 idx .. 4 idx + 3 of the packed rows (2-bit: a row is two pieces)
        half2_t off[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float o = pair_off_block(4 * (idx % PPB) + q);   // pair 4 (piece in lane block) + q of the lane block
            off[q] = half2_t{(half_t)o, (half_t)o};
        }
#pragma unroll
        for (int m = 0; m < MR; m++) {
            const u32x4 xn = xv[m][i];
            float s8 = 0.f, o8 = 0.f;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                s8 = __builtin_amdgcn_fdot2(as_half2(xn[q]), ones, s8, false);
                o8 = __builtin_amdgcn_fdot2(as_half2(xn[q]), off[q], o8, false);
            }
            s8 = block_sum(s8);
            o8 = block_sum(o8);
            if (idx < npieces) {
                *(u32x4 *)(xl + (size_t)m * xstride + (size_t)idx * 8) = xn;
                if ((idx % PPB) == 0) xs4[(size_t)m * (K / LK) + idx / PPB] = float2{o8, s8};
            }
        }
    }
    }   // !XPW
    auto stage_tab = [&](int idx, const u32x4 tv) {
        if (idx < ntab) {
            float4_t a, b;
            const half2_t e0 = as_half2(tv[0]), e1 = as_half2(tv[1]), e2 = as_half2(tv[2]), e3 = as_half2(tv[3]);
            a[0] = (float)e0[0]; a[1] = -(float)e0[1] * (float)e0[0]; a[2] = (float)e1[0]; a[3] = -(float)e1[1] * (float)e1[0];
            b[0] = (float)e2[0]; b[1] = -(float)e2[1] * (float)e2[0]; b[2] = (float)e3[0]; b[3] = -(float)e3[1] * (float)e3[0];
            *(float4_t *)(tabf + (size_t)idx * 4) = a;
            *(float4_t *)(tabf + (size_t)idx * 4 + 2) = b;
        }
    };
    stage_tab(tid, tv0);
    if (ntab > T) {   // more than 512 table pieces (small groups on a long K): the rest, blocking (rare)
        for (int idx = tid + T; idx < ntab; idx += T) stage_tab(idx, *(const u32x4 *)(tsrc + (size_t)idx * 4));
    }
    __syncthreads();

    // ---- 4. row blocks in arrival order; the next request goes out before the math of the current one ----
    const int rq = lane >> 4, col = lane & 15;
    constexpr int RG = (MR + 3) / 4;            // MFMA row groups: one v_mfma_f32_4x4x4 computes four rows of x
    const int arow = MR > 1 ? (lane & 3) : 0;   // lane l supplies row l % 4 (+ 4 per row group) of A (= of x)
    float yv[NS][MR];
#pragma unroll
    for (int s = 0; s < NS; s++)
#pragma unroll
        for (int m = 0; m < MR; m++) yv[s][m] = 0.f;
#pragma unroll
    for (int u = 0; u < NU; u++) {
        if (u + DU < NU) {
            issue(u + DU);
            __builtin_amdgcn_sched_barrier(0);
        }
        const bool valid = wave + NW * u < nrb;
        const int rb = min(wave + NW * u, nrb - 1);
        const int qd = rb * 4 + rq;                              // lane block (LK consecutive k) of this lane
        const int g = gq_shift >= 0 ? (qd >> gq_shift) : 0;
        float2 xsw = float2{0.f, 0.f};
        if constexpr (XPW) {
            // this wave owns row block rb: lane l gathers k' = 128 rb + 2 l, + 1 from the raw row, parks the pair where the fragment reads below
            // expect it (in-order LDS execution inside the wave: no barrier), and the 16 lanes of a lane block add up its {sum x OFF, sum x}
            const uint32_t pr = pw[u];
            const half2_t xg = {xraw[pr & 0xFFFFu], xraw[pr >> 16]};
            *(uint32_t *)(xl + (size_t)rb * BK + 2 * lane) = as_u32(xg);
            asm volatile("" ::: "memory");                         // (compiler order only: the fragment reads below must follow this store)
            const float of = pair_off_block(col);                // pair col of the lane block (both elements carry the same magic offset)
            float s8 = __builtin_amdgcn_fdot2(xg, ones, 0.f, false);
            float o8 = __builtin_amdgcn_fdot2(xg, half2_t{(half_t)of, (half_t)of}, 0.f, false);
            s8 += dpp_f<0xB1>(s8); o8 += dpp_f<0xB1>(o8);        // the 16 lanes of a DPP row = the 16 pairs of one lane block
            s8 += dpp_f<0x4E>(s8); o8 += dpp_f<0x4E>(o8);
            s8 += dpp_f<0x141>(s8); o8 += dpp_f<0x141>(o8);
            s8 += dpp_f<0x140>(s8); o8 += dpp_f<0x140>(o8);
            xsw = float2{o8, s8};
        }
        uint32_t X[RG][PPB * 4];
#pragma unroll
        for (int r = 0; r < RG; r++) {
            const u32x4 *xp = (const u32x4 *)(xl + (size_t)(4 * r + arow) * xstride + (size_t)qd * LK);
#pragma unroll
            for (int j = 0; j < PPB; j++) {
                const u32x4 v = xp[j];
                X[r][4 * j] = v[0]; X[r][4 * j + 1] = v[1]; X[r][4 * j + 2] = v[2]; X[r][4 * j + 3] = v[3];
            }
        }
        float2 xs[MR];
#pragma unroll
        for (int m = 0; m < MR; m++) xs[m] = XPW ? xsw : xs4[(size_t)m * (K / LK) + qd];
#pragma unroll
        for (int s = 0; s < NS; s++) {
            float4_t acc[RG];
#pragma unroll
            for (int r = 0; r < RG; r++) acc[r] = float4_t{0.f, 0.f, 0.f, 0.f};
            uint32_t t[NPB];
            unpack_block(w[u][s], uc, t);
#pragma unroll
            for (int q = 0; q < NPB / 2; q++) {
                const h4_t B = __builtin_bit_cast(h4_t, u32x2{t[2 * q], t[2 * q + 1]});
#pragma unroll
                for (int r = 0; r < RG; r++) {
                    const h4_t A = __builtin_bit_cast(h4_t, u32x2{X[r][2 * q], X[r][2 * q + 1]});
                    acc[r] = __builtin_amdgcn_mfma_f32_4x4x4f16(A, B, acc[r], 0, 0, 0);
                }
            }
            float2 e = tabf[((size_t)s * G + g) * 16 + col];
            if (!valid) e = float2{0.f, 0.f};
#pragma unroll
            for (int m = 0; m < MR; m++) {
                yv[s][m] = fmaf(e.x, acc[m / 4][m % 4] - xs[m].x, yv[s][m]);
                yv[s][m] = fmaf(e.y, xs[m].y, yv[s][m]);
            }
        }
    }

    // ---- 5. 4 row lanes -> 1 (permlane swaps), 8 waves -> 1 (LDS), epilogue, store ----
#pragma unroll
    for (int s = 0; s < NS; s++)
#pragma unroll
        for (int m = 0; m < MR; m++) yv[s][m] = fold_rows(yv[s][m]);
    if (lane < 16) {
#pragma unroll
        for (int s = 0; s < NS; s++)
#pragma unroll
            for (int m = 0; m < MR; m++) red[((wave * NS + s) * MR + m) * 16 + lane] = yv[s][m];
    }
    __syncthreads();
    if (tid < 16 * MR) {
        const int m = tid >> 4, c = tid & 15;
        float a[NS];
#pragma unroll
        for (int s = 0; s < NS; s++) {
            a[s] = 0.f;
#pragma unroll
            for (int wv = 0; wv < NW; wv++) a[s] += red[((wv * NS + s) * MR + m) * 16 + c];
        }
        float v = a[0];
        if constexpr (NS == 2) v = a[0] * (1.0f / (1.0f + __expf(-a[0]))) * a[1];   // silu on the fp32 accumulator (fused_mlp.py:160-164)
        const int n = stripe * 16 + c;
        if (y32) {           // K-shard of a row-sharded layer: the partial sums leave in fp32 (rounded once, after the all-reduce);
            if (m < M) {     // [M][NS][N]: gate and up separately -- SiLU needs the complete sums
                const size_t Nn = (size_t)gridDim.x * 16;
                y32[(size_t)m * NS * Nn + n] = a[0];
                if constexpr (NS == 2) y32[(size_t)m * NS * Nn + Nn + n] = a[1];
            }
        } else if (m < M) {
            half_t h = (half_t)v;
            if (bias) h = (half_t)((float)h + (float)bias_pre);
            y[(size_t)m * ldy + ycol] = h;     // (ycol = n, or the consumer's sorted position of column n)
        }
    }
}

// ---- 5 .. 8 rows on a LONG K (round 5): x staged in two K halves ----
// The row groups above keep all MR rows of x in LDS for the whole launch: 8 rows x 11008 k (LLaMA-7B down_proj) are 176 KB, so 5 .. 8 rows of
// that layer fell to the 16-row tiles + reduce launch (12.2 us where four rows cost 7.7 -- the hole a decode batch of 5 .. 8 sequences hits
// once per layer).  A wave's row blocks are wave + 8 u: the first NU0 of them cover a PREFIX of K, so the launch runs in two phases on one
// LDS region of MR x KP halves: stage x[:, :KP] -> blocks u < NU0 -> barrier -> stage x[:, KP:] (requested into registers before the phase-0
// math: L2 hits that arrive under it) -> the rest.  The weight stream is requested progressively across the phase boundary, exactly as above.
// Plain rows only: no fused norm, no act-order gather, no fp32 partials (down_proj needs none of them).
// X2P_EARLY = 1 would request the second half of x one block ahead of its staging; with its 64 registers next to a block's working set the
// NU = 11 instance (K = 11008) spills 28 VGPRs (tools/kernel_usage.py), without it fits exactly: the half is requested at the phase boundary
// (one exposed L2 round trip per launch; the weight stream stays DU blocks ahead across it)
#ifndef X2P_EARLY
#define X2P_EARLY 0
#endif
template <int NU, int NS, int DU, bool MF = false>
__global__ void __launch_bounds__(STRIPE_NW * 64) stripe_gemv2p_kernel(const half_t *__restrict__ x, const uint32_t *__restrict__ R,
                                                                       const uint32_t *__restrict__ tab, half_t *__restrict__ y, int K, int nrb, int G,
                                                                       int gq_shift, const half_t *__restrict__ bias, int M, int ldx, int ldy, int ldb) {
    typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
    constexpr int MR = 8, RG = MF ? 1 : 2, NW = STRIPE_NW, T = NW * 64;   // MF: v_mfma_f32_16x16x16_f16 (see stripe_gemvc_kernel)
    // (round 6: the MF instances hold 16 fragment registers per block instead of 32, so with them the early request fits without spills -- NU = 11:
    // 198 VGPRs -- and was measured: 11.3-11.4 us against 11.0-11.1 at 5 / 8 rows of 11008 x 4096, engine 3489 / 5478 against 3516 / 5509 tok/s at
    // B = 5 / 8, profiles/r6m_x2p_early: the round trip at the phase boundary is not what these launches wait for.  Stays off.)
    constexpr bool EARLY = X2P_EARLY;
    constexpr int NU0 = (NU + 1) / 2;                    // row blocks per wave in phase 0 (phase 1: the other NU - NU0)
    constexpr int KP = NU0 * NW * BK;                    // k staged per phase
    constexpr int XP = (KP / 8 + T - 1) / T;             // 16-byte pieces per thread, row and phase
    constexpr int XS = KP + 8;                           // halves per staged row (16 bytes of padding: the rows sit on different banks)
    constexpr int QP = KP / LK;                          // lane blocks per phase
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    half_t *xl = (half_t *)smem;                                           // [MR][XS]
    float2 *xs4 = (float2 *)(smem + (size_t)MR * XS * 2);                  // [MR][QP] {sum x OFF_k, sum x}
    float2 *tabf = xs4 + (size_t)MR * QP;                                  // [NS][G][16] {s, -(z + 1) s}
    float *red = (float *)(tabf + (size_t)NS * G * 16);                    // [NW][NS][MR][16]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int stripe = blockIdx.x;
    const half2_t ones = {(half_t)1.f, (half_t)1.f};
    const UnpackConsts uc = unpack_consts();
    const int npieces = K / 8, ntab = NS * G * 4;

    u32x4 xv[MR][XP], tv0;
    auto load_x = [&](int phase) {
#pragma unroll
        for (int i = 0; i < XP; i++) {
            const int idx = min(phase * (KP / 8) + tid + i * T, npieces - 1);   // clamped, not branched
#pragma unroll
            for (int m = 0; m < MR; m++) xv[m][i] = *(const u32x4 *)(x + (size_t)min(m, M - 1) * ldx + (size_t)idx * 8);
        }
    };
    load_x(0);
    const uint32_t *tsrc = tab + (size_t)stripe * NS * G * 16;
    tv0 = *(const u32x4 *)(tsrc + (size_t)min(tid, ntab - 1) * 4);
    const half_t bias_pre = *((bias ? bias + (size_t)min(tid >> 4, M - 1) * ldb + (size_t)stripe * 16 : x) + (tid & 15));
    __builtin_amdgcn_sched_barrier(0);

    typedef uint32_t wvec_t __attribute__((ext_vector_type(WPL)));
    wvec_t w[NU][NS];
    const uint32_t *wbase = R + ((size_t)stripe * nrb * NS * 64 + lane) * WPL;
    auto issue = [&](int u) {
        const int rb = min(wave + NW * u, nrb - 1);
#pragma unroll
        for (int s = 0; s < NS; s++) w[u][s] = __builtin_nontemporal_load((const wvec_t *)(wbase + ((size_t)rb * NS + s) * (64 * WPL)));
    };
#pragma unroll
    for (int u = 0; u < (DU < NU ? DU : NU); u++) issue(u);
    __builtin_amdgcn_sched_barrier(0);

    auto stage_x = [&](int phase) {
#pragma unroll
        for (int i = 0; i < XP; i++) {
            const int idl = tid + i * T, idg = phase * (KP / 8) + idl;     // piece inside the phase / inside the row
            half2_t off[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float o = pair_off_block(4 * (idl % PPB) + q);
                off[q] = half2_t{(half_t)o, (half_t)o};
            }
#pragma unroll
            for (int m = 0; m < MR; m++) {
                const u32x4 xn = xv[m][i];
                float s8 = 0.f, o8 = 0.f;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    s8 = __builtin_amdgcn_fdot2(as_half2(xn[q]), ones, s8, false);
                    o8 = __builtin_amdgcn_fdot2(as_half2(xn[q]), off[q], o8, false);
                }
                s8 = block_sum(s8);
                o8 = block_sum(o8);
                if constexpr (MF) {   // ... on to the sums of the ROW BLOCK (BK / 8 adjacent lanes of one DPP row)
                    if constexpr (PPB < 4) { s8 += dpp_f<0x4E>(s8); o8 += dpp_f<0x4E>(o8); }
                    if constexpr (PPB < 8 && BK / 8 >= 8) { s8 += dpp_f<0x141>(s8); o8 += dpp_f<0x141>(o8); }
                    if constexpr (BK / 8 >= 16) { s8 += dpp_f<0x140>(s8); o8 += dpp_f<0x140>(o8); }
                }
                if (idl < KP / 8 && idg < npieces) {
                    *(u32x4 *)(xl + (size_t)m * XS + (size_t)idl * 8) = xn;
                    if constexpr (MF) {
                        if ((idl % (BK / 8)) == 0) xs4[(size_t)(idl / (BK / 8)) * MR + m] = float2{o8, s8};   // [row block of the phase][row]
                    } else {
                        if ((idl % PPB) == 0) xs4[(size_t)m * QP + idl / PPB] = float2{o8, s8};
                    }
                }
            }
        }
    };
    stage_x(0);
    for (int idx = tid; idx < ntab; idx += T) {
        const u32x4 tv = idx == tid ? tv0 : *(const u32x4 *)(tsrc + (size_t)idx * 4);
        float4_t a, b;
        const half2_t e0 = as_half2(tv[0]), e1 = as_half2(tv[1]), e2 = as_half2(tv[2]), e3 = as_half2(tv[3]);
        a[0] = (float)e0[0]; a[1] = -(float)e0[1] * (float)e0[0]; a[2] = (float)e1[0]; a[3] = -(float)e1[1] * (float)e1[0];
        b[0] = (float)e2[0]; b[1] = -(float)e2[1] * (float)e2[0]; b[2] = (float)e3[0]; b[3] = -(float)e3[1] * (float)e3[0];
        *(float4_t *)(tabf + (size_t)idx * 4) = a;
        *(float4_t *)(tabf + (size_t)idx * 4 + 2) = b;
    }
    __syncthreads();

    const int rq = lane >> 4, col = lane & 15;
    const int arow = MF ? (lane & (MR - 1)) : (lane & 3);
    float yv[NS][MR];
#pragma unroll
    for (int s = 0; s < NS; s++)
#pragma unroll
        for (int m = 0; m < MR; m++) yv[s][m] = 0.f;
    auto block = [&](int u, int phase) {
        if (u + DU < NU) {
            issue(u + DU);
            __builtin_amdgcn_sched_barrier(0);
        }
        const bool valid = wave + NW * u < nrb;
        const int rb = min(wave + NW * u, nrb - 1);
        const int qd = rb * 4 + rq;                              // lane block (LK consecutive k) of this lane, in the row
        const int qdl = min(max(qd - phase * QP, 0), QP - 1);   // ... in the staged half (a clamped tail block reads finite rows; its scale is zero)
        const int g = gq_shift >= 0 ? ((MF ? rb * 4 : qd) >> gq_shift) : 0;
        uint32_t X[RG][PPB * 4];
#pragma unroll
        for (int r = 0; r < RG; r++) {
            const u32x4 *xp = (const u32x4 *)(xl + (size_t)(4 * r + arow) * XS + (size_t)qdl * LK);
#pragma unroll
            for (int j = 0; j < PPB; j++) {
                const u32x4 v = xp[j];
                X[r][4 * j] = v[0]; X[r][4 * j + 1] = v[1]; X[r][4 * j + 2] = v[2]; X[r][4 * j + 3] = v[3];
            }
        }
        float2 xs[MR];
        if constexpr (MF) {
            const int rbl = qdl >> 2;                             // row block inside the staged half
#pragma unroll
            for (int i = 0; i < 4; i++) xs[i] = xs4[(size_t)rbl * MR + ((4 * rq) & (MR - 1)) + i];
        } else {
#pragma unroll
        for (int m = 0; m < MR; m++) xs[m] = xs4[(size_t)m * QP + qdl];
        }
#pragma unroll
        for (int s = 0; s < NS; s++) {
            float4_t acc[RG];
#pragma unroll
            for (int r = 0; r < RG; r++) acc[r] = float4_t{0.f, 0.f, 0.f, 0.f};
            uint32_t t[NPB];
            unpack_block(w[u][s], uc, t);
#pragma unroll
            for (int q = 0; q < NPB / 2; q++) {
                const h4_t B = __builtin_bit_cast(h4_t, u32x2{t[2 * q], t[2 * q + 1]});
#pragma unroll
                for (int r = 0; r < RG; r++) {
                    const h4_t A = __builtin_bit_cast(h4_t, u32x2{X[r][2 * q], X[r][2 * q + 1]});
                    if constexpr (MF) acc[r] = __builtin_amdgcn_mfma_f32_16x16x16f16(A, B, acc[r], 0, 0, 0);
                    else acc[r] = __builtin_amdgcn_mfma_f32_4x4x4f16(A, B, acc[r], 0, 0, 0);
                }
            }
            float2 e = tabf[((size_t)s * G + g) * 16 + col];
            if (!valid) e = float2{0.f, 0.f};
            if constexpr (MF) {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    yv[s][i] = fmaf(e.x, acc[0][i] - xs[i].x, yv[s][i]);
                    yv[s][i] = fmaf(e.y, xs[i].y, yv[s][i]);
                }
            } else {
#pragma unroll
            for (int m = 0; m < MR; m++) {
                yv[s][m] = fmaf(e.x, acc[m / 4][m % 4] - xs[m].x, yv[s][m]);
                yv[s][m] = fmaf(e.y, xs[m].y, yv[s][m]);
            }
            }
        }
    };
#pragma unroll
    for (int u = 0; u < NU0; u++) {
        if (u == NU0 - 1 && EARLY) {          // the second half of x (L2 hits): requested one block ahead of its staging -- 64 registers that would not fit next to
            load_x(1);               // the whole first phase (the instance spilled 28), and the last block's math covers most of the round trip
            __builtin_amdgcn_sched_barrier(0);
        }
        block(u, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();                 // every wave is done with the first half of x
    if (!EARLY) load_x(1);
    stage_x(1);
    __syncthreads();
#pragma unroll
    for (int u = NU0; u < NU; u++) {
        block(u, 1);
        __builtin_amdgcn_sched_barrier(0);
    }

    if constexpr (MF) {
        if (rq < MR / 4) {
#pragma unroll
            for (int s = 0; s < NS; s++)
#pragma unroll
                for (int i = 0; i < 4; i++) red[((wave * NS + s) * MR + 4 * rq + i) * 16 + col] = yv[s][i];
        }
    } else {
#pragma unroll
    for (int s = 0; s < NS; s++)
#pragma unroll
        for (int m = 0; m < MR; m++) yv[s][m] = fold_rows(yv[s][m]);
    if (lane < 16) {
#pragma unroll
        for (int s = 0; s < NS; s++)
#pragma unroll
            for (int m = 0; m < MR; m++) red[((wave * NS + s) * MR + m) * 16 + lane] = yv[s][m];
    }
    }
    __syncthreads();
    if (tid < 16 * MR) {
        const int m = tid >> 4, c = tid & 15;
        float a[NS];
#pragma unroll
        for (int s = 0; s < NS; s++) {
            a[s] = 0.f;
#pragma unroll
            for (int wv = 0; wv < NW; wv++) a[s] += red[((wv * NS + s) * MR + m) * 16 + c];
        }
        float v = a[0];
        if constexpr (NS == 2) v = a[0] * (1.0f / (1.0f + __expf(-a[0]))) * a[1];
        if (m < M) {
            half_t h = (half_t)v;
            if (bias) h = (half_t)((float)h + (float)bias_pre);
            y[(size_t)m * ldy + stripe * 16 + c] = h;
        }
    }
}

template <int NU, int NS, bool MF = false>
int stripe_launch_2p(const StripeParams &p, hipStream_t s) {
    constexpr int DU = NS == 2 ? 1 : 3, NU0 = (NU + 1) / 2, KP = NU0 * STRIPE_NW * BK, MR = 8;
    auto kern = stripe_gemv2p_kernel<NU, NS, DU, MF>;
    const size_t lds = (size_t)MR * (KP + 8) * 2 + (size_t)MR * (KP / LK) * 8 + (size_t)NS * p.G * 16 * 8 + (size_t)STRIPE_NW * NS * MR * 16 * 4;
    if (lds > 160 * 1024 - 64) return GPTQ_E_VARIANT;
    static LdsOptIn opt_in;   // per instantiation; per device inside
    if (int rc = opt_in.ensure((const void *)kern, lds)) return rc;
    hipLaunchKernelGGL(kern, dim3(p.N / 16), dim3(STRIPE_NW * 64), lds, s, p.x, p.R, p.tab, p.y, p.K, p.K / BK, p.G, p.gq_shift, p.bias, p.M, (int)p.ldx,
                       (int)p.ldy, (int)p.ldb);
    return (int)hipGetLastError();
}

// bytes of the first LDS region of stripe_gemvc_kernel: MR rows of x; with the deferred epilogue (MR = 16) also the C stripes' partial sums
__host__ __device__ inline size_t stripe_c_region0_bytes(int K, int MR, int C, int NS, bool defer) {
    const size_t xb = (size_t)MR * (K + 8) * 2, rb = (size_t)C * STRIPE_NW * NS * MR * 16 * 4;
    return defer && rb > xb ? rb : xb;
}

// ---- decode batches of 2 .. 4 rows on WIDE layers (round 5): C consecutive stripes per workgroup ----
// The kernel above gives every 16-column stripe its own workgroup; a layer with more stripes than twice the CUs (qkv 768, gate | up 688 on LLaMA-7B)
// puts three workgroups on a CU, and each of them stages -- and with NORM normalises -- the SAME MR rows of x: at four rows that staging is the
// difference to the one-row launch (4096 x 12288: 6.9 -> 8.1 us plain, 7.5 -> 10.5 with the norm; profiles/r5a_batch/layer_decode_default.txt).
// Here ONE workgroup stages x once and walks C stripes: the weight stream is one sequence of C x NU row blocks per wave, requested DU ahead ACROSS
// the stripe boundaries; a stripe's epilogue (4 row lanes -> 1, 8 waves -> 1 through one of two `red` buffers, store) runs under the next stripe's
// loads -- its barrier waits for LDS only (s_waitcnt lgkmcnt(0) + s_barrier; __syncthreads() would drain the prefetched weights).  The tables of
// the C stripes are contiguous in the image and staged together.  Plain / NORM, residual, yperm; no act-order gather, no fp32 partials.
// MF (round 6, MR = 8): 5 .. 8 rows through v_mfma_f32_16x16x16_f16 instead of two 4x4x4 row groups.  The stripe layout IS that instruction's B
// operand -- lane l holds four consecutive k of column l % 16, the lane groups l / 16 are its four k quads -- so one MFMA per k quad of the lane
// block multiplies the SAME unpacked pair registers by 16 rows of x (A: lane l supplies row l % 16 -- the staged rows, repeated -- of its own k quad)
// and sums the four lane groups on the way: the MFMA count and the LDS fragment bytes of the FOUR-row launch (the 4x4x4 row groups double both
// at eight rows: 4096 x 12288 + norm 11.6 us against 7.9 at four rows, gpurun_out r6e), no fold across the lane groups.  The sums of x a lane block
// needs for the magic offsets become sums per ROW BLOCK, so the group must span the row block (gq_shift >= 2 or one group; not 2-bit: its
// row block is 32 pieces, wider than a DPP row).
template <int NU, int NS, int DU, bool NORM, int MR, int C, bool MF = false>
__global__ void __launch_bounds__(STRIPE_NW * 64) stripe_gemvc_kernel(const half_t *__restrict__ x, const uint32_t *__restrict__ R,
                                                                      const uint32_t *__restrict__ tab, half_t *__restrict__ y, int K, int nrb, int G,
                                                                      int gq_shift, const half_t *__restrict__ bias, const half_t *__restrict__ nw,
                                                                      float eps, int M, int ldx, int ldy, int ldb, const int32_t *__restrict__ yperm,
                                                                      int nstripes) {
    typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
    static_assert(!MF || ((MR == 8 || MR == 16) && SB != 2), "the 16x16x16 inner product serves the eight- and sixteen-row instances");
    constexpr int NW = STRIPE_NW, T = NW * 64;
    constexpr int XP = (NU * NW * BK / 8 + T - 1) / T;   // 16-byte pieces of one x row per thread (K <= NU * NW * BK)
    constexpr int RED = NW * NS * MR * 16;               // floats per `red` buffer
    // DEFER (MR = 16): sixteen rows of x fill LDS (K = 4096: 128 KB), so there is no room for the two `red` buffers of the pipelined epilogue --
    // every stripe keeps its four sums per lane in registers (yv[C][NS][4]) and ONE epilogue at the end reduces all C stripes through the region
    // x occupied; the norm partials get 512 bytes of their own
    constexpr bool DEFER = MF && MR == 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int xstride = K + 8;
    const size_t xbytes = stripe_c_region0_bytes(K, MR, C, NS, DEFER);
    half_t *xl = (half_t *)smem;                                                              // [MR][xstride] (normalised) x
    float2 *xs4 = (float2 *)(smem + xbytes);                                                  // [MR][K / LK] {sum x OFF_k, sum x}; MF: [K / BK][MR]
    float2 *tabf = xs4 + (size_t)MR * (MF ? K / BK : K / LK);                                 // [C][NS][G][16] {s, -(z + 1) s}
    float *red = DEFER ? (float *)smem : (float *)(tabf + (size_t)C * NS * G * 16);           // [2][NW][NS][MR][16]; DEFER: [C][NW][NS][MR][16] over x
    float *nrm = DEFER ? (float *)(tabf + (size_t)C * NS * G * 16) : red;                     // [NW][MR] norm partials
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int stripe0 = blockIdx.x * C;
    const int cvalid = min(C, nstripes - stripe0);       // stripes of this workgroup that exist (the last workgroup of a ragged N)
    const half2_t ones = {(half_t)1.f, (half_t)1.f};
    const UnpackConsts uc = unpack_consts();
    const int npieces = K / 8, ntab = NS * G * 4, ntabc = cvalid * ntab;   // 16-byte pieces of an x row / of a stripe's table / of this workgroup's tables

    // ---- 1. x (+ norm weight), the first table piece, the residual and the output columns: requested BEFORE the weights ----
    u32x4 xv[MR][XP], nv[NORM ? XP : 1], tv0, tv1;
#pragma unroll
    for (int i = 0; i < XP; i++) {
        const int idx = min(tid + i * T, npieces - 1);   // clamped, not branched
#pragma unroll
        for (int m = 0; m < MR; m++) xv[m][i] = *(const u32x4 *)(x + (size_t)min(m, M - 1) * ldx + (size_t)idx * 8);
        if constexpr (NORM) nv[i] = *(const u32x4 *)(nw + (size_t)idx * 8);
    }
    const uint32_t *tsrc = tab + (size_t)stripe0 * NS * G * 16;
    tv0 = *(const u32x4 *)(tsrc + (size_t)min(tid, ntabc - 1) * 4);
    tv1 = *(const u32x4 *)(tsrc + (size_t)min(tid + T, ntabc - 1) * 4);   // (pair: 2 sets x 32 groups x 3 stripes = 768 pieces)
    half_t bias_pre[C];
    int ycol[C];
#pragma unroll
    for (int c = 0; c < C; c++) {
        const int st = min(stripe0 + c, nstripes - 1);
        bias_pre[c] = *((bias ? bias + (size_t)min(tid >> 4, M - 1) * ldb + (size_t)st * 16 : x) + (tid & 15));
        ycol[c] = yperm ? yperm[st * 16 + (tid & 15)] : st * 16 + (tid & 15);
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- 2. the first DU row blocks of this wave's sequence (stripe c = g / NU, row block wave + NW (g % NU)) ----
    typedef uint32_t wvec_t __attribute__((ext_vector_type(WPL)));
    wvec_t w[C * NU][NS];
    const uint32_t *wlane = R + (size_t)lane * WPL;
    auto issue = [&](int g) {
        const int c = g / NU, u = g % NU;
        const int st = min(stripe0 + c, nstripes - 1);        // a stripe past the end re-reads the last one (never stored)
        const int rb = min(wave + NW * u, nrb - 1);           // ragged tail: re-read the last block (its table entry is zeroed below)
#pragma unroll
        for (int s = 0; s < NS; s++)
            w[g][s] = __builtin_nontemporal_load((const wvec_t *)(wlane + (((size_t)st * nrb + rb) * NS + s) * (64 * WPL)));
    };
#pragma unroll
    for (int g = 0; g < (DU < C * NU ? DU : C * NU); g++) issue(g);
    __builtin_amdgcn_sched_barrier(0);

    // ---- 3. stage x, the per-lane-block sums and the tables in LDS (as in stripe_gemv_kernel) ----
    if constexpr (NORM) {
        float ss[MR];
#pragma unroll
        for (int m = 0; m < MR; m++) {
            ss[m] = 0.f;
#pragma unroll
            for (int i = 0; i < XP; i++) {
                if (tid + i * T < npieces) {
#pragma unroll
                    for (int q = 0; q < 4; q++) ss[m] = __builtin_amdgcn_fdot2(as_half2(xv[m][i][q]), as_half2(xv[m][i][q]), ss[m], false);
                }
            }
            ss[m] = wave_sum_all(ss[m]);
            if (lane == 0) nrm[wave * MR + m] = ss[m];
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < MR; m++) {
            float tot = 0.f;
#pragma unroll
            for (int wv = 0; wv < NW; wv++) tot += nrm[wv * MR + m];
            const float rstd = 1.0f / sqrtf(tot / (float)K + eps);
#pragma unroll
            for (int i = 0; i < XP; i++) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const half2_t a = as_half2(xv[m][i][q]), b = as_half2(nv[i][q]);
                    const half2_t r = {(half_t)((float)a[0] * rstd * (float)b[0]), (half_t)((float)a[1] * rstd * (float)b[1])};
                    xv[m][i][q] = as_u32(r);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < XP; i++) {
        const int idx = tid + i * T;
        half2_t off[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float o = pair_off_block(4 * (idx % PPB) + q);
            off[q] = half2_t{(half_t)o, (half_t)o};
        }
#pragma unroll
        for (int m = 0; m < MR; m++) {
            const u32x4 xn = xv[m][i];
            float s8 = 0.f, o8 = 0.f;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                s8 = __builtin_amdgcn_fdot2(as_half2(xn[q]), ones, s8, false);
                o8 = __builtin_amdgcn_fdot2(as_half2(xn[q]), off[q], o8, false);
            }
            s8 = block_sum(s8);
            o8 = block_sum(o8);
            if constexpr (MF) {   // ... on to the sums of the ROW BLOCK: its BK / 8 pieces are BK / 8 adjacent lanes of one DPP row
                if constexpr (BK / 8 > PPB) {
                    if constexpr (PPB < 4) { s8 += dpp_f<0x4E>(s8); o8 += dpp_f<0x4E>(o8); }
                    if constexpr (PPB < 8 && BK / 8 >= 8) { s8 += dpp_f<0x141>(s8); o8 += dpp_f<0x141>(o8); }
                    if constexpr (BK / 8 >= 16) { s8 += dpp_f<0x140>(s8); o8 += dpp_f<0x140>(o8); }
                }
            }
            if (idx < npieces) {
                *(u32x4 *)(xl + (size_t)m * xstride + (size_t)idx * 8) = xn;
                if constexpr (MF) {
                    if ((idx % (BK / 8)) == 0) xs4[(size_t)(idx / (BK / 8)) * MR + m] = float2{o8, s8};   // [row block][row]
                } else {
                    if ((idx % PPB) == 0) xs4[(size_t)m * (K / LK) + idx / PPB] = float2{o8, s8};
                }
            }
        }
    }
    auto stage_tab = [&](int idx, const u32x4 tv) {
        if (idx >= ntabc) return;
        float4_t a, b;
        const half2_t e0 = as_half2(tv[0]), e1 = as_half2(tv[1]), e2 = as_half2(tv[2]), e3 = as_half2(tv[3]);
        a[0] = (float)e0[0]; a[1] = -(float)e0[1] * (float)e0[0]; a[2] = (float)e1[0]; a[3] = -(float)e1[1] * (float)e1[0];
        b[0] = (float)e2[0]; b[1] = -(float)e2[1] * (float)e2[0]; b[2] = (float)e3[0]; b[3] = -(float)e3[1] * (float)e3[0];
        *(float4_t *)(tabf + (size_t)idx * 4) = a;
        *(float4_t *)(tabf + (size_t)idx * 4 + 2) = b;
    };
    stage_tab(tid, tv0);
    stage_tab(tid + T, tv1);
    if (ntabc > 2 * T) {   // more than 1024 table pieces (small groups): the rest, blocking (rare)
        for (int idx = tid + 2 * T; idx < ntabc; idx += T) stage_tab(idx, *(const u32x4 *)(tsrc + (size_t)idx * 4));
    }
    __syncthreads();

    // ---- 4. the sequence of C x NU row blocks; after the last block of a stripe its epilogue ----
    const int rq = lane >> 4, col = lane & 15;
    constexpr int RG = MF ? 1 : (MR + 3) / 4;
    const int arow = MF ? (lane & (MR - 1)) : (MR > 1 ? (lane & 3) : 0);   // MF: lane l supplies row l % 16 of A: the eight staged rows, twice
    constexpr int YC = DEFER ? C : 1, YR = MF ? 4 : MR;
    float yv[YC][NS][YR];
#pragma unroll
    for (int c = 0; c < YC; c++)
#pragma unroll
        for (int s = 0; s < NS; s++)
#pragma unroll
            for (int m = 0; m < YR; m++) yv[c][s][m] = 0.f;
#pragma unroll
    for (int g = 0; g < C * NU; g++) {
        const int c = g / NU, u = g % NU;
        const int yc = DEFER ? c : 0;
        if (g + DU < C * NU) {
            issue(g + DU);
            __builtin_amdgcn_sched_barrier(0);
        }
        const bool valid = wave + NW * u < nrb;
        const int rb = min(wave + NW * u, nrb - 1);
        const int qd = rb * 4 + rq;
        const int gi = gq_shift >= 0 ? ((MF ? rb * 4 : qd) >> gq_shift) : 0;   // (MF: the row block's group -- it spans the block)
        uint32_t X[RG][PPB * 4];
#pragma unroll
        for (int r = 0; r < RG; r++) {
            const u32x4 *xp = (const u32x4 *)(xl + (size_t)(4 * r + arow) * xstride + (size_t)qd * LK);
#pragma unroll
            for (int j = 0; j < PPB; j++) {
                const u32x4 v = xp[j];
                X[r][4 * j] = v[0]; X[r][4 * j + 1] = v[1]; X[r][4 * j + 2] = v[2]; X[r][4 * j + 3] = v[3];
            }
        }
        float2 xs[MR];
        if constexpr (MF) {   // the lane's four result rows 4 (l / 16) .. + 3 (rows 8 .. 15 repeat 0 .. 7): sums of x over the row block
#pragma unroll
            for (int i = 0; i < 4; i++) xs[i] = xs4[(size_t)rb * MR + ((4 * rq) & (MR - 1)) + i];
        } else {
#pragma unroll
            for (int m = 0; m < MR; m++) xs[m] = xs4[(size_t)m * (K / LK) + qd];
        }
#pragma unroll
        for (int s = 0; s < NS; s++) {
            float4_t acc[RG];
#pragma unroll
            for (int r = 0; r < RG; r++) acc[r] = float4_t{0.f, 0.f, 0.f, 0.f};
            uint32_t t[NPB];
            unpack_block(w[g][s], uc, t);
#pragma unroll
            for (int q = 0; q < NPB / 2; q++) {
                const h4_t B = __builtin_bit_cast(h4_t, u32x2{t[2 * q], t[2 * q + 1]});
#pragma unroll
                for (int r = 0; r < RG; r++) {
                    const h4_t A = __builtin_bit_cast(h4_t, u32x2{X[r][2 * q], X[r][2 * q + 1]});
                    if constexpr (MF) acc[r] = __builtin_amdgcn_mfma_f32_16x16x16f16(A, B, acc[r], 0, 0, 0);
                    else acc[r] = __builtin_amdgcn_mfma_f32_4x4x4f16(A, B, acc[r], 0, 0, 0);
                }
            }
            float2 e = tabf[(((size_t)min(c, cvalid - 1) * NS + s) * G + gi) * 16 + col];
            if (!valid) e = float2{0.f, 0.f};
            if constexpr (MF) {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    yv[yc][s][i] = fmaf(e.x, acc[0][i] - xs[i].x, yv[yc][s][i]);
                    yv[yc][s][i] = fmaf(e.y, xs[i].y, yv[yc][s][i]);
                }
            } else {
#pragma unroll
            for (int m = 0; m < MR; m++) {
                yv[0][s][m] = fmaf(e.x, acc[m / 4][m % 4] - xs[m].x, yv[0][s][m]);
                yv[0][s][m] = fmaf(e.y, xs[m].y, yv[0][s][m]);
            }
            }
        }
        if constexpr (!DEFER)
        if (u == NU - 1) {   // ---- 5. stripe c is complete: 4 row lanes -> 1, 8 waves -> 1 (LDS, buffer c % 2), epilogue, store ----
            float *rbuf = red + (c & 1) * RED;
            if constexpr (MF) {   // the matrix core summed the lane groups already: lane (g, col) holds rows 4 g .. + 3 (g < 2: the eight rows)
                if (rq < MR / 4) {
#pragma unroll
                    for (int s = 0; s < NS; s++)
#pragma unroll
                        for (int i = 0; i < 4; i++) rbuf[((wave * NS + s) * MR + 4 * rq + i) * 16 + col] = yv[0][s][i];
                }
            } else {
#pragma unroll
            for (int s = 0; s < NS; s++)
#pragma unroll
                for (int m = 0; m < MR; m++) yv[0][s][m] = fold_rows(yv[0][s][m]);
            if (lane < 16) {
#pragma unroll
                for (int s = 0; s < NS; s++)
#pragma unroll
                    for (int m = 0; m < MR; m++) rbuf[((wave * NS + s) * MR + m) * 16 + lane] = yv[0][s][m];
            }
            }
            // LDS-only barrier: the weight loads of the next stripe stay in flight.  (Buffer c % 2 is written again for stripe c + 2, i.e. after the
            // barrier of stripe c + 1, which every wave reaches after its reads below.)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (tid < 16 * MR) {
                const int m = tid >> 4, cc = tid & 15;
                float a[NS];
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    a[s] = 0.f;
#pragma unroll
                    for (int wv = 0; wv < NW; wv++) a[s] += rbuf[((wv * NS + s) * MR + m) * 16 + cc];
                }
                float v = a[0];
                if constexpr (NS == 2) v = a[0] * (1.0f / (1.0f + __expf(-a[0]))) * a[1];   // silu on the fp32 accumulator (fused_mlp.py:160-164)
                if (m < M && c < cvalid) {
                    half_t h = (half_t)v;
                    if (bias) h = (half_t)((float)h + (float)bias_pre[c]);
                    y[(size_t)m * ldy + ycol[c]] = h;
                }
            }
#pragma unroll
            for (int s = 0; s < NS; s++)
#pragma unroll
                for (int m = 0; m < YR; m++) yv[0][s][m] = 0.f;
        }
    }
    if constexpr (DEFER) {   // ---- 5'. all C stripes at once: 8 waves -> 1 through the region x occupied, epilogue, store ----
        __syncthreads();     // every wave is done with x
#pragma unroll
        for (int c = 0; c < C; c++)
#pragma unroll
            for (int s = 0; s < NS; s++)
#pragma unroll
                for (int i = 0; i < 4; i++) red[(size_t)c * RED + ((wave * NS + s) * MR + 4 * rq + i) * 16 + col] = yv[c][s][i];
        __syncthreads();
        if (tid < 16 * MR) {
            const int m = tid >> 4, cc = tid & 15;
#pragma unroll
            for (int c = 0; c < C; c++) {
                float a[NS];
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    a[s] = 0.f;
#pragma unroll
                    for (int wv = 0; wv < NW; wv++) a[s] += red[(size_t)c * RED + ((wv * NS + s) * MR + m) * 16 + cc];
                }
                float v = a[0];
                if constexpr (NS == 2) v = a[0] * (1.0f / (1.0f + __expf(-a[0]))) * a[1];   // silu on the fp32 accumulator (fused_mlp.py:160-164)
                if (m < M && c < cvalid) {
                    half_t h = (half_t)v;
                    if (bias) h = (half_t)((float)h + (float)bias_pre[c]);
                    y[(size_t)m * ldy + ycol[c]] = h;
                }
            }
        }
    }
}

size_t stripe_lds_bytes(int K, int G, int NS, bool xperm, int MR) {
    const size_t xstride = MR > 1 ? K + 8 : K;
    return (size_t)MR * xstride * 2 + (size_t)MR * (K / LK) * 8 + (size_t)NS * G * 16 * 8 + (size_t)STRIPE_NW * NS * MR * 16 * 4 +
           (xperm ? (size_t)K * 2 : 0);
}

template <int NU, int NS, int DU, bool NORM, bool XPERM, int MR, bool ATT = false>
int stripe_launch_du(const StripeParams &p, hipStream_t s) {
    auto kern = stripe_gemv_kernel<NU, NS, DU, NORM, XPERM, MR, ATT>;
    const size_t lds = stripe_lds_bytes(p.K, p.G, NS, XPERM, MR);
    if (lds > 160 * 1024 - 64) return GPTQ_E_VARIANT;
    static LdsOptIn opt_in;   // per instantiation; per device inside
    if (int rc = opt_in.ensure((const void *)kern, lds)) return rc;
    hipLaunchKernelGGL(kern, dim3(p.N / 16), dim3(STRIPE_NW * 64), lds, s, p.x, p.R, p.tab, p.y, p.K, p.K / BK, p.G, p.gq_shift, p.bias,
                       p.norm_w, p.norm_eps, p.xperm, p.y32, p.M, (int)p.ldx, (int)p.ldy, p.progress, (int)p.ldb, p.yperm, p.att);
    return (int)hipGetLastError();
}

template <int NU, int NS, bool NORM, bool XPERM, int MR>
int stripe_launch_one(const StripeParams &p, hipStream_t s) {
    // row blocks of weights requested ahead.  (Round 5, measured and lost: for a decode batch -- MR > 1, a long staging phase, with NORM one rstd per
    // row behind a barrier -- EVERY row block of a short K (NU <= 4) requested before the staging instead of DU of them; no spills (111 VGPRs for the
    // pair with NORM at MR = 4), and slower: gate | up pair at 4 rows 13.75 against 12.42 us plain, 15.3 against 14.2 with the norm, qkv 8.42 against
    // 8.08; engine at B = 4 2756 against 2824 tok/s -- profiles/r5g_du_deep/.  And on the long K of LLaMA-7B's down_proj (NU = 11, one workgroup per
    // CU, 24 KB in flight per CU at DU = 3) deeper is monotonically SLOWER at one row: DU = 3 / 5 / 8 / 11: 6.22 / 6.45 / 7.08 / 8.17 us with the residual
    // -- profiles/r5k_du_long/.)
    constexpr int DU = NS == 2 ? 1 : (NU > 4 ? 3 : 2);
    return stripe_launch_du<NU, NS, DU, NORM, XPERM, MR>(p, s);
}

// C stripes per workgroup (stripe_gemvc_kernel) on layers with more than two stripes per CU.  Measured (profiles/r5i_c_stripes/, us per launch, LLaMA-7B
// qkv / gate | up pair, this kernel against one stripe per workgroup): 2 .. 4 rows -- 8.2 / 11.9 against 10.7 / 14.5 with the fused norm, 7.9 / 11.4
// against 8.2 / 12.3 plain: every variant; ONE row -- 6.9 / 10.5 against 7.2 / 10.8 with the norm, but 7.0 / 10.8 against 6.7 / 10.4 plain: NORM only;
// 5 .. 8 rows (against the 16-row tiles + a norm launch) -- the pair 15.6 / 16.2 against 16.4 / 17.4, qkv a tie (11.7 / 11.3 against 11.7 / 11.5) and
// slower plain: the pair only (capi.hip decode_rows_max).  Engine: 955 against 922 tok/s at B = 1, 3134 against 2851 at B = 4, 4694 against 4547 at B = 8.
template <int NU, int NS, bool NORM, int C, int MR, int DU, bool MF = false>
int stripe_launch_cdu(const StripeParams &p, hipStream_t s) {
    auto kern = stripe_gemvc_kernel<NU, NS, DU, NORM, MR, C, MF>;
    constexpr bool DEFER = MF && MR == 16;
    const size_t lds = stripe_c_region0_bytes(p.K, MR, C, NS, DEFER) + (size_t)MR * (MF ? p.K / BK : p.K / LK) * 8 + (size_t)C * NS * p.G * 16 * 8 +
                       (DEFER ? (size_t)STRIPE_NW * MR * 4 : (size_t)2 * STRIPE_NW * NS * MR * 16 * 4);
    if (lds > 160 * 1024 - 64) return GPTQ_E_VARIANT;
    static LdsOptIn opt_in;   // per instantiation; per device inside
    if (int rc = opt_in.ensure((const void *)kern, lds)) return rc;
    const int nstripes = p.N / 16;
    hipLaunchKernelGGL(kern, dim3((nstripes + C - 1) / C), dim3(STRIPE_NW * 64), lds, s, p.x, p.R, p.tab, p.y, p.K, p.K / BK, p.G, p.gq_shift, p.bias,
                       p.norm_w, p.norm_eps, p.M, (int)p.ldx, (int)p.ldy, (int)p.ldb, p.yperm, nstripes);
    return (int)hipGetLastError();
}

template <int NU, int NS, bool NORM, int C, int MR>
int stripe_launch_c(const StripeParams &p, hipStream_t s) {
    // row blocks in flight per wave across the stripe boundaries: swept on qkv / the pair at one and four rows (the sweep in
    // profiles/r5i_c_stripes/, us with the fused norm at 1 / 4 rows): single set 2 / 3 / 4 / 6 / 8 blocks: 6.81 / 6.86 / 6.79 / 7.02 /
    // 7.28 and 8.63 / 8.36 / 7.99 / 8.15 / 8.98; pair 2 / 3 / 4: 10.6 / 11.0 / 11.5 and 11.7 / 12.1 / 12.2 -- deeper is slower here too (r5k_du_long)
    return stripe_launch_cdu<NU, NS, NORM, C, MR, (NS == 2 ? 2 : 4)>(p, s);
}

template <int NU, int NS, int MR, int C>
int stripe_launch_c_norm(const StripeParams &p, hipStream_t s) {
    if (p.norm_w) return stripe_launch_c<NU, NS, true, C, MR>(p, s);
    if constexpr (MR == 1) return GPTQ_E_VARIANT;   // one row: the fused-norm launches only (plain, again with 4 / 2 blocks in flight: 6.94 / 10.6-10.8 us
    else return stripe_launch_c<NU, NS, false, C, MR>(p, s);   // against 6.7-6.8 / 10.4-10.5, the driver-contract pass 4126 against 4124 GB/s: plain_one_row_through_c_stripes_ab.txt)
}

template <int NU, int NS, int MR>
int stripe_launch_c_pick(const StripeParams &p, hipStream_t s) {
    if constexpr (NU > 5 || SB == 2 || (MR == 8 && NS == 1)) {
        return GPTQ_E_VARIANT;
    } else {
        // more than two stripes per CU; with the fused norm already more than ONE (x is normalised once per workgroup: 5120 x 5120 at four rows 7.9
        // against 9.2 us, 4096 x 6144 6.7 against 7.2, 4096 x 8192 7.2 against 7.6; plain launches of those shapes are a tie)
        const int nstripes = p.N / 16, min_stripes = p.norm_w ? 256 : 512;
        if (nstripes <= min_stripes) return GPTQ_E_VARIANT;
        const int c = (nstripes + 255) / 256;
        if (c == 2) return stripe_launch_c_norm<NU, NS, MR, 2>(p, s);
        if (c == 3) return stripe_launch_c_norm<NU, NS, MR, 3>(p, s);
        if (c == 4) return stripe_launch_c_norm<NU, NS, MR, 4>(p, s);
        return GPTQ_E_VARIANT;
    }
}

// 5 .. 8 rows through the 16x16x16 inner product (stripe_gemvc_kernel / stripe_gemv2p_kernel, MF): any number of stripes per workgroup (C = 1 on
// one-round shapes), with or without the fused norm.  Everything else keeps the 4x4x4 row groups / 16-row tiles of round 5.
inline bool stripe_mf8_ok(const StripeParams &p) {
    return SB != 2 && (p.gq_shift == -1 || p.gq_shift >= 2) && !p.y32 && !p.xperm && p.M > 4 && p.M <= 16;
}
template <int NU, int NS, int C, int MR>
int stripe_launch_mf8_c(const StripeParams &p, hipStream_t s) {
    constexpr int DU = NS == 2 ? 2 : 4;
    return p.norm_w ? stripe_launch_cdu<NU, NS, true, C, MR, DU, true>(p, s) : stripe_launch_cdu<NU, NS, false, C, MR, DU, true>(p, s);
}
// MR = 16 (round 6: 9 .. 16 rows): the same inner product with all sixteen A rows distinct -- K <= 4096 (one 16-byte piece of every row per thread:
// 64 registers of x in flight; sixteen rows of a longer K do not fit LDS either), one epilogue for all C stripes at the end (DEFER, see the kernel)
template <int NU, int NS, int MR = 8>
int stripe_launch_mf8(const StripeParams &p, hipStream_t s) {
    if constexpr (SB == 2 || NU > 8 || (MR == 16 && NU * STRIPE_NW * BK > 4096)) {
        return GPTQ_E_VARIANT;
    } else {
        const int c = (p.N / 16 + 255) / 256;
        if (c <= 1) return stripe_launch_mf8_c<NU, NS, 1, MR>(p, s);
        if constexpr (NU <= 5) {
            if (c == 2) return stripe_launch_mf8_c<NU, NS, 2, MR>(p, s);
            if (c == 3) return stripe_launch_mf8_c<NU, NS, 3, MR>(p, s);
            if (c == 4) return stripe_launch_mf8_c<NU, NS, 4, MR>(p, s);
        }
        return GPTQ_E_VARIANT;
    }
}

template <int NU, int NS>
int stripe_launch_variant(const StripeParams &p, hipStream_t s) {
    const bool norm = p.norm_w != nullptr, perm = p.xperm != nullptr;
    if (p.att.o16) {   // round 6: x comes as the decode attention's split records (the plain one-row launch of o_proj)
        if constexpr (NS == 1) {
            if (p.M == 1 && !norm && !perm && !p.y32 && !p.yperm) return stripe_launch_du<NU, 1, (NU > 4 ? 3 : 2), false, false, 1, true>(p, s);
        }
        return GPTQ_E_VARIANT;
    }
    if (p.M > 1) {
        if (perm || (p.y32 && (p.M > 4 || norm))) return GPTQ_E_VARIANT;
        if (p.M <= 4) {
            if (!p.y32) {   // wide layers: C stripes per workgroup, x staged (and normalised) once per CU instead of once per stripe
                const int rc = stripe_launch_c_pick<NU, NS, 4>(p, s);
                if (rc != GPTQ_E_VARIANT) return rc;
            }
            return norm ? stripe_launch_one<NU, NS, true, false, 4>(p, s) : stripe_launch_one<NU, NS, false, false, 4>(p, s);
        }
        if (stripe_mf8_ok(p) && p.M > 8) {   // round 6: 9 .. 16 rows, K <= 4096; declines when the tables do not fit LDS next to sixteen rows of x
            const int rc = stripe_launch_mf8<NU, NS, 16>(p, s);
            if (rc != GPTQ_E_VARIANT) return rc;
        } else if (stripe_mf8_ok(p)) {   // round 6: 5 .. 8 rows at the cost of four (16x16x16 inner product); declines when 8 rows of x do not fit LDS
            const int rc = stripe_launch_mf8<NU, NS>(p, s);
            if (rc != GPTQ_E_VARIANT) return rc;
            if constexpr (SB != 2 && NU * STRIPE_NW * BK > 9216 && NU * STRIPE_NW * BK <= 12288 && NS == 1) {
                if (!norm && !p.yperm && !p.progress) return stripe_launch_2p<NU, NS, true>(p, s);     // long K: x in two halves
            }
        }
        // 8 / 16 rows of x must fit in LDS next to the tables (checked again at launch): K <= ~9200 / ~4600
        if constexpr (NU * STRIPE_NW * BK <= 9216) {
            if (p.M <= 8) {
                if (!p.y32) {
                    const int rc = stripe_launch_c_pick<NU, NS, 8>(p, s);
                    if (rc != GPTQ_E_VARIANT) return rc;
                }
                return norm ? stripe_launch_one<NU, NS, true, false, 8>(p, s) : stripe_launch_one<NU, NS, false, false, 8>(p, s);
            }
        } else if constexpr (NU * STRIPE_NW * BK <= 12288 && NS == 1) {      // (NU = 13 .. 16 would fit LDS but spill 25 .. 48 registers)
            // long K: x in two halves (LLaMA-7B down_proj at 5 .. 8 rows); its epilogue stores natural columns and ticks nothing (ADVICE r5)
            if (p.M <= 8 && !norm && !p.y32 && !p.yperm && !p.progress) return stripe_launch_2p<NU, NS>(p, s);
        }
        if constexpr (NU * STRIPE_NW * BK <= 5120) {
            if (p.M <= 16) {
                // (the fused norm keeps 16 rows x XP pieces of x in registers: with XP = 2 -- K > 4096 -- the instance spills 41-48 VGPRs
                // (tools/kernel_usage.py); the caller then runs the norm as its own launch)
                if constexpr (NU * STRIPE_NW * BK <= 4096) {
                    if (norm) return stripe_launch_one<NU, NS, true, false, 16>(p, s);
                }
                if (norm) return GPTQ_E_VARIANT;
                return stripe_launch_one<NU, NS, false, false, 16>(p, s);
            }
        }
        return GPTQ_E_VARIANT;
    }
    if (norm && !perm && !p.y32 && !p.progress) {   // round 5: wide layers with the fused norm -- C stripes per workgroup, x normalised once per CU
        const int rc = stripe_launch_c_pick<NU, NS, 1>(p, s);
        if (rc != GPTQ_E_VARIANT) return rc;
    }
    if (norm) return perm ? stripe_launch_one<NU, NS, true, true, 1>(p, s) : stripe_launch_one<NU, NS, true, false, 1>(p, s);
    return perm ? stripe_launch_one<NU, NS, false, true, 1>(p, s) : stripe_launch_one<NU, NS, false, false, 1>(p, s);
}

template <int NU>
int stripe_launch_nu(int nu, const StripeParams &p, hipStream_t s) {
    if constexpr (NU > stripe_max_nu(SB)) {
        return GPTQ_E_VARIANT;
    } else {
        if (nu == NU) return p.NS == 2 ? stripe_launch_variant<NU, 2>(p, s) : stripe_launch_variant<NU, 1>(p, s);
        return stripe_launch_nu<NU + 1>(nu, p, s);
    }
}

}  // namespace

#define STRIPE_CAT2(a, b) a##b
#define STRIPE_CAT(a, b) STRIPE_CAT2(a, b)
int STRIPE_CAT(stripe_gemv_dispatch_b, STRIPE_BITS)(const StripeParams &p, hipStream_t s) {
    const int nu = (p.K / BK + STRIPE_NW - 1) / STRIPE_NW;
    if (nu < 1) return GPTQ_E_VARIANT;
    return stripe_launch_nu<1>(nu, p, s);
}

}  // namespace gptq
