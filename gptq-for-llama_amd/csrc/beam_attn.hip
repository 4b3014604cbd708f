// beam_attn.hip -- attention of the N running beams of ONE beam search (N = 2 .. 16), the histories read through an ancestry table instead of being
// copied between cache rows (include/gptq_mi355x.h "beam cache indirection"; the table's update is gptq_beam_src_update_u8 in beam.hip).
//
// src uint8 [N][t_max]: src[b][t] = the cache slot that physically holds position t of beam b's history.  All beams sit at ONE position p (device
// memory); `common` (device memory) says that columns t < common are the same in every row of the table: the trunk of the hypothesis tree.
// Two launches:
//   1. beam_rope_kv_kernel, grid (N, heads): the shared RoPE + append of attn_device.h per (beam, head) -- cache row (slot b, p) gets the bits a
//      token-by-token feed writes --, the rotated q goes to the workspace, src[b][p] = b, the arrival tickets of launch 2 are cleared.
//   2. beam_attn_kernel, grid (heads, S): ONE workgroup of four waves serves all N beams of a head for its range of keys; [0, p + 1) is cut by
//      attn_split() at run time.  Inside a split:
//        trunk  keys t < common: streamed ONCE for all beams.  A wave walks tiles of 32 keys: S^T = K Q^T and O^T += V^T P^T on
//               v_mfma_f32_16x16x32_f16 with the beams as the (padded) 16 query columns -- chunk_attn.hip's tile without the causal mask: K from
//               global memory in the A layout, V through the wave's own swizzled LDS image and ds_read_b64_tr_b16, online softmax per beam in the
//               log2 domain, the next tile in flight while this one is computed.  Consecutive trunk keys may live in different slots: the 32 slot
//               bytes of a tile are ONE byte load per lane, requested a tile ahead of the K / V loads that need them, and handed to the lanes by
//               ds_bpermute -- so K / V addresses never wait for a dependent load.
//        tail   keys common <= t <= p differ per beam: the waves take the beams in turn (beam = wave, wave + 4, ..), 16 lanes per key row, four rows
//               per pass, fp32 fma dot products as the streaming decode kernel does, the row (src[b][t], t) gathered per key; two register sets.
//      The four waves' trunk states and the beams' tail states {M, l, acc} meet once in LDS and give the split's record per beam; one active
//      split: that IS the output row; several: the records / ticket / last-arriver merge of attn_device.h.  Every sum has a fixed order and the
//      ticket only decides who merges: same inputs, same bits.
// A `common` below the true common prefix only moves keys from the trunk to the tail.  Slot bytes are clamped to N - 1 before they address the
// cache: whatever the table holds, nothing outside the N slots is read.  p < 0 or p >= t_max: nothing is read or written.
#include <algorithm>

#include "attn_device.h"
#include "gptq_internal.h"

namespace gptq {

constexpr int BA_HD = 128;     // head_dim served
constexpr int BA_NW = 4;       // waves per workgroup
constexpr int BA_KT = 32;      // trunk keys per wave tile (two 16-key MFMA blocks)
constexpr int BA_QR = 16;      // query columns of the MFMA: the beams, padded
constexpr int BA_TP = 4;       // tail passes per step: 4 passes x 4 key rows = 16 keys of one beam per wave step
constexpr int BA_TPS = 256;    // tokens a split owns at least (chunk_attn.hip's cut: 8 splits from 1793 tokens on)

__global__ void __launch_bounds__(64) beam_rope_kv_kernel(const half_t *__restrict__ qkv, int64_t ldq, const int64_t *__restrict__ pos_ptr,
                                                          half_t *__restrict__ kc, half_t *__restrict__ vc, int64_t slot_stride,
                                                          uint8_t *__restrict__ src, half_t *__restrict__ qrot, unsigned *__restrict__ tickets,
                                                          int heads, int t_max, float inv_base, const float2 *__restrict__ tab) {
    const int b = blockIdx.x, h = blockIdx.y, c = threadIdx.x, half = BA_HD / 2;
    if (b == 0 && c == 0) tickets[h] = 0u;
    const int64_t p = pos_ptr[0];
    if (p < 0 || p >= t_max) return;
    if (h == 0 && c == 0) src[(size_t)b * t_max + p] = (uint8_t)b;
    float cs, sn;
    rope_cos_sin(tab, p, c, half, inv_base, cs, sn);
    const int hd = heads * BA_HD;
    const half_t *q = qkv + (size_t)b * ldq + (size_t)h * BA_HD + c;
    half_t *qd = qrot + (size_t)b * hd + (size_t)h * BA_HD + c;
    half_t *kd = kc + (size_t)b * slot_stride + (size_t)p * hd + (size_t)h * BA_HD + c;
    half_t *vd = vc + (size_t)b * slot_stride + (size_t)p * hd + (size_t)h * BA_HD + c;
    rope_kv_row(q, q + hd, q + 2 * hd, qd, kd, vd, half, cs, sn);
}

struct BeamAttnArgs {
    const half_t *q;             // rotated q [N][heads * 128]
    const int64_t *pos;          // [1]
    const int32_t *common;       // [1]
    const uint8_t *src;          // [N][t_max]
    const half_t *kc, *vc;       // N slots [t_max][heads * 128], slot_stride elements apart
    half_t *out;                 // [N] rows, ldo apart
    const int32_t *out_perm;     // NULL or [heads * 128]: the column element k of a row is stored at
    uint32_t *o16;               // records: [S][N][heads * 128] fp16 partial outputs (as pairs)
    float *md;                   //          [S][heads][N] {M, den}
    unsigned *tickets;           //          [heads]
    int heads, beams, t_max;
    int64_t ldo, slot_stride;
    float scale2;                // softmax scale x log2(e)
};

__global__ void __launch_bounds__(BA_NW * 64) beam_attn_kernel(const BeamAttnArgs a) {
    // the waves' V tiles [32 keys][128] fp16; at the end the waves' trunk O [16 beams][128] fp32 (the same 8 KB each)
    __shared__ __attribute__((aligned(16))) half_t vs[BA_NW][BA_KT * BA_HD];
    __shared__ __attribute__((aligned(16))) float ta[BA_QR][BA_HD];      // the beams' tail O
    __shared__ float mw[BA_NW + 1][BA_QR], lw[BA_NW + 1][BA_QR];         // row BA_NW: the tails
    __shared__ int last_flag;
    const int h = blockIdx.x, s = blockIdx.y, S = gridDim.y;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, qi = lane & 15;               // 16-lane row of the wave, column (= beam of the MFMA)
    const int hd = a.heads * BA_HD, N = a.beams;
    const int64_t p64 = ((const __attribute__((address_space(4))) int64_t *)a.pos)[0];
    if (p64 < 0 || p64 >= a.t_max) return;
    const int p = (int)p64, len = p + 1;
    const int common = min(max(((const __attribute__((address_space(4))) int32_t *)a.common)[0], 0), p);   // position p is never shared
    const AttnSplit sp = attn_split(len, S, BA_TPS);
    if (s >= sp.nsp) return;
    const int t0 = s * sp.chunk;
    const int t_end = min(t0 + sp.chunk, len);             // this split attends to keys [t0, t_end):
    const int k_end = min(t_end, common);                  //   [t0, k_end) on the shared path (empty when k_end <= t0),
    const int l0 = max(t0, common);                        //   [l0, t_end) gathered per beam
    const int ntiles = k_end > t0 ? (k_end - t0 + BA_KT - 1) / BA_KT : 0;
    const half_t *const kc = a.kc + (size_t)h * BA_HD, *const vc = a.vc + (size_t)h * BA_HD;

    // ================================================ trunk ================================================
    // Q^T fragments (B operand of K Q^T): lane = beam, element j of k-step ks = dim 32 g + 8 ks + j (K's fragments use the same map)
    half8_t qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
        qf[ks] = half8_t{0, 0, 0, 0, 0, 0, 0, 0};
        if (qi < N) qf[ks] = *(const half8_t *)(a.q + (size_t)qi * hd + (size_t)h * BA_HD + 32 * g + 8 * ks);
    }
    // A row m of a 16-key block is key 8 ((m >> 2) & 1) + 4 (m >> 3) + (m & 3) of the block: accumulator register r of lane row g holds key
    // 8 (g & 1) + 4 (g >> 1) + r (chunk_attn.hip: the two 4-row blocks a 32-lane half reads through the transposed read lie 8 rows apart)
    const int krow = 8 * ((qi >> 2) & 1) + 4 * (qi >> 3) + (qi & 3);
    const int kreg0 = 8 * (g & 1) + 4 * (g >> 1);
    const int vrow = lane >> 4, vch = lane & 15;           // V staging: chunk vch of tile rows vrow + 4 i

    // the slots of a tile's 32 keys: lane j (and j + 32) asks for key tb + j of row 0 of the table
    auto slots_of = [&](int tb) {
        const int key = tb + (lane & 31);
        int sl = 0;
        if (key < k_end) sl = a.src[key];
        return sl;
    };
    u32x4 kA[2][4], vA[8], kB[2][4], vB[8];
    auto request = [&](u32x4 (&K)[2][4], u32x4 (&V)[8], int tb, int slots) {
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const int key = tb + 16 * b + krow;
            const int sl = min(__shfl(slots, 16 * b + krow, 64), N - 1);
            const half_t *row = kc + (size_t)sl * a.slot_stride + (size_t)key * hd + 32 * g;
#pragma unroll
            for (int ks = 0; ks < 4; ks++) {
                K[b][ks] = u32x4{0u, 0u, 0u, 0u};
                if (key < k_end) K[b][ks] = *(const u32x4 *)(row + 8 * ks);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int key = tb + vrow + 4 * i;
            const int sl = min(__shfl(slots, vrow + 4 * i, 64), N - 1);
            V[i] = u32x4{0u, 0u, 0u, 0u};
            if (key < k_end) V[i] = *(const u32x4 *)(vc + (size_t)sl * a.slot_stride + (size_t)key * hd + vch * 8);
        }
    };
    half_t *const img = vs[wave];

    // running state of the lane's beam: M (log2 domain, the same in the four lanes of a column), l (this lane's keys), O^T[dim][beam]
    float M = ATT_M_FLOOR, l = 0.f;
    float4_t acc[8];
#pragma unroll
    for (int d = 0; d < 8; d++) acc[d] = float4_t{0.f, 0.f, 0.f, 0.f};

    auto tile = [&](const u32x4 (&K)[2][4], const u32x4 (&V)[8], int tb) {
#pragma unroll
        for (int i = 0; i < 8; i++) *(ATTN_LDS u32x4 *)((ATTN_LDS char *)img + attn_lds_off(vrow + 4 * i, vch)) = V[i];
        float4_t sc[2];
#pragma unroll
        for (int b = 0; b < 2; b++) {
            sc[b] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ks++)
                sc[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8_t, K[b][ks]), qf[ks], sc[b], 0, 0, 0);
        }
        float mt = -INFINITY;
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int key = tb + 16 * b + kreg0 + r;
                float v = sc[b][r] * a.scale2;
                if (key >= k_end) v = -INFINITY;           // every beam sees the whole trunk: the only mask is the end of the range
                sc[b][r] = v;
                mt = fmaxf(mt, v);
            }
        mt = rows_max(mt);
        const float Mn = fmaxf(M, mt);                     // finite: M starts at the floor
        const float alpha = __builtin_amdgcn_exp2f(M - Mn);
        M = Mn;
        float ps = 0.f;
        half8_t pf;
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float e = __builtin_amdgcn_exp2f(sc[b][r] - Mn);   // masked slots hold -inf: 0
                ps += e;
                pf[4 * b + r] = (half_t)e;
            }
        l = __builtin_fmaf(l, alpha, ps);
#pragma unroll
        for (int d = 0; d < 8; d++) acc[d] *= alpha;
        // O^T[dim][beam] += V^T P^T: element j of lane row g is key 16 (j >> 2) + kreg0 + (j & 3) -- what pf holds -- so V^T comes as two transposed
        // 4-key blocks, 16 keys apart; lane 4 q + pp of a 16-lane group supplies row q, columns 4 pp .. 4 pp + 3 of the block
#pragma unroll
        for (int d = 0; d < 8; d++) {
            const int r0 = kreg0 + (qi >> 2), ch = 2 * d + ((qi & 3) >> 1), sub = 8 * (qi & 1);
            const half4_t lo = attn_tr_read(img, attn_lds_off(r0, ch) + sub);
            const half4_t up = attn_tr_read(img, attn_lds_off(r0 + 16, ch) + sub);
            const half8_t vf = half8_t{lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
            acc[d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, acc[d], 0, 0, 0);
        }
    };

    // the wave's tiles: wave, wave + 4, ... (wave-uniform control flow: EXEC is full at every transposed read and every ds_bpermute).  The slot
    // bytes of a tile are requested one K / V request ahead of the request that uses them.
    if (wave < ntiles) {
        int sA = slots_of(t0 + wave * BA_KT), sB = slots_of(t0 + (wave + BA_NW) * BA_KT);
        request(kA, vA, t0 + wave * BA_KT, sA);
        for (int i = wave; i < ntiles; i += 2 * BA_NW) {
            const bool more = i + BA_NW < ntiles;
            sA = slots_of(t0 + (i + 2 * BA_NW) * BA_KT);
            if (more) request(kB, vB, t0 + (i + BA_NW) * BA_KT, sB);
            tile(kA, vA, t0 + i * BA_KT);
            if (more) {
                sB = slots_of(t0 + (i + 3 * BA_NW) * BA_KT);
                if (i + 2 * BA_NW < ntiles) request(kA, vA, t0 + (i + 2 * BA_NW) * BA_KT, sA);
                tile(kB, vB, t0 + (i + BA_NW) * BA_KT);
            }
        }
    }
    // the lane rows of a column -> one; the wave's trunk state goes to LDS (the wave is done with its own V image)
    l = rows_sum(l);
    float *const ow = (float *)img;                        // [16 beams][128 dims] fp32
#pragma unroll
    for (int d = 0; d < 8; d++) *(ATTN_LDS float4_t *)((ATTN_LDS float *)ow + qi * BA_HD + 16 * d + 4 * g) = acc[d];
    if (g == 0) {
        mw[wave][qi] = M;
        lw[wave][qi] = l;
    }

    // ================================================ tail ================================================
    // beam b = wave, wave + 4, ..: key row tsub of a pass, eight dims per lane; rows of beams >= N and empty tails leave {floor, 0, 0}
    const int tsub = lane >> 4, d8 = lane & 15;
    for (int b = wave; b < BA_QR; b += BA_NW) {
        float Mt = ATT_M_FLOOR, lt = 0.f, av[8];
#pragma unroll
        for (int j = 0; j < 8; j++) av[j] = 0.f;
        if (b < N && l0 < t_end) {
            const uint8_t *const sb = a.src + (size_t)b * a.t_max;
            const half8_t q8 = *(const half8_t *)(a.q + (size_t)b * hd + (size_t)h * BA_HD + d8 * 8);
            float qv[8];
#pragma unroll
            for (int j = 0; j < 8; j++) qv[j] = (float)q8[j];
            u32x4 KA[BA_TP], VA[BA_TP], KB[BA_TP], VB[BA_TP];
            auto treq = [&](u32x4 (&K)[BA_TP], u32x4 (&V)[BA_TP], int tb) {
#pragma unroll
                for (int it = 0; it < BA_TP; it++) {
                    const int key = tb + 4 * it + tsub;
                    K[it] = u32x4{0u, 0u, 0u, 0u};
                    V[it] = u32x4{0u, 0u, 0u, 0u};
                    if (key < t_end) {
                        const int sl = min((int)sb[key], N - 1);
                        const size_t off = (size_t)sl * a.slot_stride + (size_t)key * hd + d8 * 8;
                        K[it] = *(const u32x4 *)(kc + off);
                        V[it] = *(const u32x4 *)(vc + off);
                    }
                }
            };
            auto tstep = [&](const u32x4 (&K)[BA_TP], const u32x4 (&V)[BA_TP], int tb) {
                float sc[BA_TP], mt = -INFINITY;
#pragma unroll
                for (int it = 0; it < BA_TP; it++) {
                    const half8_t k8 = __builtin_bit_cast(half8_t, K[it]);
                    float dot = 0.f;
#pragma unroll
                    for (int j = 0; j < 8; j++) dot = __builtin_fmaf(qv[j], (float)k8[j], dot);
                    const float v = row_sum16(dot) * a.scale2;
                    sc[it] = tb + 4 * it + tsub < t_end ? v : -INFINITY;
                    mt = fmaxf(mt, sc[it]);
                }
                mt = rows_max(mt);                                   // the wave's four key rows: Mt stays wave-uniform
                const float Mn = fmaxf(Mt, mt), alpha = __builtin_amdgcn_exp2f(Mt - Mn);
                Mt = Mn;
                float pr[BA_TP], ps = 0.f;
#pragma unroll
                for (int it = 0; it < BA_TP; it++) {
                    pr[it] = __builtin_amdgcn_exp2f(sc[it] - Mn);    // masked slots hold -inf: 0
                    ps += pr[it];
                }
                lt = __builtin_fmaf(lt, alpha, ps);
#pragma unroll
                for (int j = 0; j < 8; j++) av[j] *= alpha;
#pragma unroll
                for (int it = 0; it < BA_TP; it++) {
                    const half8_t v8 = __builtin_bit_cast(half8_t, V[it]);
#pragma unroll
                    for (int j = 0; j < 8; j++) av[j] = __builtin_fmaf(pr[it], (float)v8[j], av[j]);
                }
            };
            constexpr int STEP = 4 * BA_TP;
            treq(KA, VA, l0);
            for (int tb = l0; tb < t_end; tb += 2 * STEP) {
                const bool more = tb + STEP < t_end;
                if (more) treq(KB, VB, tb + STEP);
                tstep(KA, VA, tb);
                if (more) {
                    if (tb + 2 * STEP < t_end) treq(KA, VA, tb + 2 * STEP);
                    tstep(KB, VB, tb + STEP);
                }
            }
#pragma unroll
            for (int j = 0; j < 8; j++) av[j] = rows_sum(av[j]);
            lt = rows_sum(lt);                                       // the four key rows -> one: every lane holds the beam's {Mt, lt}
        }
        if (lane < 16) {
            *(float4_t *)(&ta[b][lane * 8]) = float4_t{av[0], av[1], av[2], av[3]};
            *(float4_t *)(&ta[b][lane * 8 + 4]) = float4_t{av[4], av[5], av[6], av[7]};
        }
        if (lane == 0) {
            mw[BA_NW][b] = Mt;
            lw[BA_NW][b] = lt;
        }
    }
    __syncthreads();

    // ================================ the four trunk states and the tail of a beam -> {Mx, den, o} of the split ================================
    const int qq = tid >> 4, d0 = (tid & 15) * 8;          // this thread's beam and its eight dims
    float Mx, den;                                         // (den = 0 only for the padding rows qq >= N)
    half_t o[8];
    attn_waves_meet<BA_NW + 1, 8>(&mw[0][qq], &lw[0][qq], BA_QR,
                                        [&](int w) { return (w < BA_NW ? (const float *)vs[w] + qq * BA_HD : &ta[qq][0]) + d0; }, Mx, den, o);
    half_t *const orow = a.out + (size_t)qq * a.ldo;
    auto store = [&](const half_t (&r)[8]) {               // out_perm: element k of the row goes to column out_perm[k] (the batch entry's map)
        if (a.out_perm) {
#pragma unroll
            for (int j = 0; j < 8; j++) orow[a.out_perm[h * BA_HD + d0 + j]] = r[j];
        } else {
            *(half8_t *)(orow + (size_t)h * BA_HD + d0) = half8_t{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
        }
    };
    const size_t rstride = (size_t)N * hd / 2;             // uint32 words per split
    const size_t mstride = (size_t)a.heads * N * 2;
    uint32_t *const ro = a.o16 + ((size_t)qq * hd + (size_t)h * BA_HD + d0) / 2;
    float *const rmd = a.md + ((size_t)h * N + qq) * 2;
    attn_split_finish(o, Mx, den, ro, rstride, rmd, mstride, a.tickets + h, &last_flag, sp.nsp, s, qq < N, (tid & 15) == 0, store);
}

// the workspace is the chunk attention's for one sequence of N rows (attn_split.h): rotated q | records | {M, den} | tickets; S of the grid likewise
size_t beam_attn_ws_bytes(int beams, int heads, int t_max) { return chunk_attn_ws(1, beams, heads, t_max).bytes; }

// active splits of a call whose beams attend to `len` = p + 1 keys: what attn_split() gives the kernel
int beam_attn_active_splits(int heads, int t_max, int len) { return attn_split(len, chunk_attn_grid_splits(heads, t_max), BA_TPS).nsp; }

int beam_attn_launch(const half_t *qkv, int64_t ldq, int beams, const int64_t *pos, half_t *kc, half_t *vc, int64_t slot_stride, uint8_t *src,
                     const int32_t *common, half_t *out, int64_t ldo, const int32_t *out_perm, void *ws, int heads, int t_max, float base,
                     float scale, const float *rope_table, hipStream_t s) {
    const ChunkAttnWs w = chunk_attn_ws(1, beams, heads, t_max);
    half_t *qrot = (half_t *)((char *)ws + w.qrot);
    BeamAttnArgs a{};
    a.o16 = (uint32_t *)((char *)ws + w.o16);
    a.md = (float *)((char *)ws + w.md);
    a.tickets = (unsigned *)((char *)ws + w.tickets);
    hipLaunchKernelGGL(beam_rope_kv_kernel, dim3(beams, heads), dim3(BA_HD / 2), 0, s, qkv, ldq, pos, kc, vc, slot_stride, src, qrot, a.tickets, heads,
                       t_max, rope_inv_base(base, BA_HD), (const float2 *)rope_table);
    a.q = qrot; a.pos = pos; a.common = common; a.src = src; a.kc = kc; a.vc = vc; a.out = out; a.out_perm = out_perm;
    a.heads = heads; a.beams = beams; a.t_max = t_max; a.ldo = ldo; a.slot_stride = slot_stride;
    a.scale2 = scale * 1.44269504088896340736f;
    hipLaunchKernelGGL(beam_attn_kernel, dim3(heads, w.S), dim3(BA_NW * 64), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace gptq
