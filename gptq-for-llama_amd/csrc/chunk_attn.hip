// chunk_attn.hip -- attention of a handful of CONSECUTIVE tokens of one sequence over a long history, with the position in device memory: the
// verify step of speculative decoding (the last accepted token and its drafts go through the model together, one pass over the weights).
// Reference: what HF generate's one-token loop does R times behind llama_inference.py:109-115 -- triton_rotate_half_, torch.cat onto the past and
// F.scaled_dot_product_attention (quant/fused_attn.py:126-158) -- for R rows at once.
//
// rows (1..16, a host value: it shapes the grid) tokens sit at positions p .. p + rows - 1, p = *position read on the device, so a captured graph
// replays the call at any position.  Two launches:
//   1. chunk_rope_kv_kernel, grid (rows, heads): the shared RoPE + append of attn_device.h (rope_cos_sin, rope_kv_row) per (row, head) -- the
//      instructions and flags of every other entry, so cache rows p + r get the bits a token-by-token feed writes; the rotated q
//      goes to the workspace, qkv is never written.  It also clears the arrival tickets of launch 2 (no state is asked of the caller's workspace).
//      The kernel boundary orders the append against every read of launch 2.
//   2. chunk_attn_kernel, grid (heads, S): the key range [0, p + rows) is cut into splits by attn_split() from its length at run time, as the decode
//      attention does (attn_split.h; CA_TPS tokens per split at least, at most S <= ATT_MAX_SPLITS) -- ONE cut for all rows: a split streams its
//      keys and values once and serves every row with them.  A split is a workgroup of four waves; a wave walks tiles of 32 keys with an online
//      softmax (log2 domain) per query row, the query rows padded to 16:
//        S^T[key][query] = K Q^T   v_mfma_f32_16x16x32_f16, K straight from global memory in the A layout (lane = key, 64 contiguous bytes per
//                                  lane), Q^T fragments in registers for the whole walk;
//        O^T[dim][query] += V^T P^T  the accumulator layout of the first product is the B operand of the second (P rounded to fp16 in registers);
//                                  V^T comes through ds_read_b64_tr_b16 from the wave's own LDS image of the V tile (the swizzled
//                                  256-byte rows of attn_device.h; the key order of a 16-key block is permuted so that the two 4-row blocks a
//                                  32-lane half reads lie 8 rows apart: conflict-free).
//      The next tile's K / V are requested into registers before the current one is computed.  No workgroup barrier inside the walk: the LDS image
//      is private to the wave.  The four waves meet once (LDS), giving the split's {M, den, o = num / den in fp16} per row.  One active split: that
//      IS the output row.  Several: the split hand-off of attn_device.h (system-scope records, attn_ticket_last, attn_merge_records), as in the decode
//      attention -- the ticket decides who merges, never what is computed: same inputs, same bits.
// Bounds: keys at and beyond min(p + rows, t_max) are never loaded (their slots of a tile are zeros); for row r everything above p + r is masked by a
// select before the maximum.  p < 0 or p >= t_max: nothing is read or written.  A row whose position is >= t_max is skipped.
// Several sequences (batched speculative decoding): both grids get the sequence b as blockIdx.z -- its packed rows b rows .. of qkv / out, its cache
// slot, its position pos[b], its part of the workspace, its tickets -- and nothing else changes: per sequence the same instructions on the same
// values as a single-sequence call (which is the seqs = 1 case), hence the same bits; still two launches for any number of sequences.
#include <algorithm>

#include "attn_device.h"
#include "gptq_internal.h"

namespace gptq {

constexpr int CA_HD = 128;     // head_dim served
constexpr int CA_NW = 4;       // waves per workgroup
constexpr int CA_KT = 32;      // keys per wave tile (two 16-key MFMA blocks)
constexpr int CA_QR = 16;      // query rows of the MFMA (rows padded to it)
constexpr int CA_TPS = 256;    // tokens a split owns at least: 8 splits from 1793 tokens on (32 heads x 8 = one workgroup per CU at 2047)

__global__ void __launch_bounds__(64) chunk_rope_kv_kernel(const half_t *__restrict__ qkv, int64_t ldq, const int64_t *__restrict__ pos_ptr,
                                                           half_t *__restrict__ kc, half_t *__restrict__ vc, int64_t slot_stride,
                                                           half_t *__restrict__ qrot, unsigned *__restrict__ tickets, int heads, int t_max,
                                                           float inv_base, const float2 *__restrict__ tab) {
    const int h = blockIdx.y, c = threadIdx.x, half = CA_HD / 2;
    const int r = blockIdx.x, b = blockIdx.z, rows = gridDim.x;      // sequence b: packed rows b rows .., cache slot b, position pos_ptr[b]
    if (r == 0 && c == 0) tickets[(size_t)b * heads + h] = 0u;
    const int64_t p = pos_ptr[b];
    if (p < 0 || p >= t_max) return;                              // (before the sum: p + r cannot wrap for any position value)
    const int64_t pos = p + r;
    if (pos >= t_max) return;
    float cs, sn;
    rope_cos_sin(tab, pos, c, half, inv_base, cs, sn);
    const int hd = heads * CA_HD;
    const half_t *q = qkv + ((size_t)b * rows + r) * ldq + (size_t)h * CA_HD + c;
    half_t *qd = qrot + ((size_t)b * rows + r) * hd + (size_t)h * CA_HD + c;
    half_t *kd = kc + (size_t)b * slot_stride + (size_t)pos * hd + (size_t)h * CA_HD + c;
    half_t *vd = vc + (size_t)b * slot_stride + (size_t)pos * hd + (size_t)h * CA_HD + c;
    rope_kv_row(q, q + hd, q + 2 * hd, qd, kd, vd, half, cs, sn);
}

struct ChunkAttnArgs {
    const half_t *q;             // rotated q [seqs][rows][heads * 128]
    const int64_t *pos;          // [seqs]
    const half_t *kc, *vc;       // [seqs] slots [t_max][heads * 128], slot_stride elements apart
    half_t *out;                 // [seqs * rows] rows, ldo apart
    uint32_t *o16;               // records: [seqs][S][rows][heads * 128] fp16 partial outputs (as pairs)
    float *md;                   //          [seqs][S][heads][rows] {M, den}
    unsigned *tickets;           //          [seqs][heads]
    int heads, rows, t_max;
    int64_t ldo, slot_stride;
    float scale2;                // softmax scale x log2(e)
};

__global__ void __launch_bounds__(CA_NW * 64) chunk_attn_kernel(const ChunkAttnArgs a) {
    // the waves' V tiles [32 keys][128] fp16; at the end the waves' O [16 rows][128] fp32 (the same 8 KB each)
    __shared__ __attribute__((aligned(16))) half_t vs[CA_NW][CA_KT * CA_HD];
    __shared__ float mw[CA_NW][CA_QR], lw[CA_NW][CA_QR];
    __shared__ int last_flag;
    const int h = blockIdx.x, s = blockIdx.y, S = gridDim.y, b = blockIdx.z;   // head, split, splits of the grid, sequence
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, qi = lane & 15;               // 16-lane row of the wave, column (= query row of the MFMA)
    const int hd = a.heads * CA_HD;
    const int64_t p64 = ((const __attribute__((address_space(4))) int64_t *)a.pos)[b];
    if (p64 < 0 || p64 >= a.t_max) return;
    const int p = (int)p64;
    const int nr = min(a.rows, a.t_max - p);               // rows that fit the cache
    const int len = p + nr;                                // keys of the launch: [0, len)
    const AttnSplit sp = attn_split(len, S, CA_TPS);
    if (s >= sp.nsp) return;
    const int t0 = s * sp.chunk;
    const int t_end = min(t0 + sp.chunk, len);             // this split attends to keys [t0, t_end)
    const int ntiles = (t_end - t0 + CA_KT - 1) / CA_KT;   // >= 1
    const half_t *const kc = a.kc + (size_t)b * a.slot_stride + (size_t)h * CA_HD, *const vc = a.vc + (size_t)b * a.slot_stride + (size_t)h * CA_HD;
    const half_t *const qb = a.q + (size_t)b * a.rows * hd;           // this sequence's rotated q rows

    // ---- Q^T fragments (B operand of K Q^T): lane = query, element j of k-step ks = dim 32 g + 8 ks + j (K's fragments use the same map) ----
    half8_t qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
        qf[ks] = half8_t{0, 0, 0, 0, 0, 0, 0, 0};
        if (qi < nr) qf[ks] = *(const half8_t *)(qb + (size_t)qi * hd + (size_t)h * CA_HD + 32 * g + 8 * ks);
    }
    // A row m of a 16-key block is key ca_key(m) of the block: accumulator register r of lane row g holds key 8 (g & 1) + 4 (g >> 1) + r
    const int krow = 8 * ((qi >> 2) & 1) + 4 * (qi >> 3) + (qi & 3);
    const int kreg0 = 8 * (g & 1) + 4 * (g >> 1);
    const int vrow = lane >> 4, vch = lane & 15;           // V staging: chunk vch of tile rows vrow + 4 i

    u32x4 kA[2][4], vA[8], kB[2][4], vB[8];
    auto request = [&](u32x4 (&K)[2][4], u32x4 (&V)[8], int tb) {
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const int key = tb + 16 * b + krow;
#pragma unroll
            for (int ks = 0; ks < 4; ks++) {
                K[b][ks] = u32x4{0u, 0u, 0u, 0u};
                if (key < t_end) K[b][ks] = *(const u32x4 *)(kc + (size_t)key * hd + 32 * g + 8 * ks);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int key = tb + vrow + 4 * i;
            V[i] = u32x4{0u, 0u, 0u, 0u};
            if (key < t_end) V[i] = *(const u32x4 *)(vc + (size_t)key * hd + vch * 8);
        }
    };
    half_t *const img = vs[wave];

    // ---- running state of the lane's query row: M (log2 domain, the same in the four lanes of a column), l (this lane's keys), O^T[dim][query] ----
    float M = ATT_M_FLOOR, l = 0.f;
    float4_t acc[8];
#pragma unroll
    for (int d = 0; d < 8; d++) acc[d] = float4_t{0.f, 0.f, 0.f, 0.f};
    const int qpos = p + qi;                               // the last key this lane's query row sees

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
                if (key > qpos || key >= t_end) v = -INFINITY;
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
        // O^T[dim][query] += V^T P^T: element j of lane row g is key 16 (j >> 2) + kreg0 + (j & 3) -- what pf holds -- so V^T comes as two transposed
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

    // the wave's tiles: wave, wave + 4, ... (wave-uniform control flow: EXEC is full at every transposed read)
    if (wave < ntiles) {
        request(kA, vA, t0 + wave * CA_KT);
        for (int i = wave; i < ntiles; i += 2 * CA_NW) {
            const bool more = i + CA_NW < ntiles;
            if (more) request(kB, vB, t0 + (i + CA_NW) * CA_KT);
            tile(kA, vA, t0 + i * CA_KT);
            if (more) {
                if (i + 2 * CA_NW < ntiles) request(kA, vA, t0 + (i + 2 * CA_NW) * CA_KT);
                tile(kB, vB, t0 + (i + CA_NW) * CA_KT);
            }
        }
    }

    // ---- the lane rows of a column -> one, the waves -> one (LDS): {Mx, den, num} of the split per query row ----
    l = rows_sum(l);
    float *const ow = (float *)img;                        // [16 queries][128 dims] fp32: the wave is done with its own V image
#pragma unroll
    for (int d = 0; d < 8; d++) *(ATTN_LDS float4_t *)((ATTN_LDS float *)ow + qi * CA_HD + 16 * d + 4 * g) = acc[d];
    if (g == 0) {
        mw[wave][qi] = M;
        lw[wave][qi] = l;
    }
    __syncthreads();
    const int qq = tid >> 4, d0 = (tid & 15) * 8;          // this thread's query row and its eight dims
    float Mx = mw[0][qq];
#pragma unroll
    for (int w = 1; w < CA_NW; w++) Mx = fmaxf(Mx, mw[w][qq]);
    float num[8], den = 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++) num[j] = 0.f;
#pragma unroll
    for (int w = 0; w < CA_NW; w++) {
        const float e = __builtin_amdgcn_exp2f(mw[w][qq] - Mx);
        den = __builtin_fmaf(e, lw[w][qq], den);
        const float *src = (const float *)vs[w] + qq * CA_HD + d0;
#pragma unroll
        for (int j = 0; j < 8; j++) num[j] = __builtin_fmaf(e, src[j], num[j]);
    }
    // the split's normalised output; a row that saw no key of this split (den = 0: its keys end below t0) leaves zeros, which merge with weight 0
    const float rden = den > 0.f ? __builtin_amdgcn_rcpf(den) : 0.f;
    half8_t o;
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = attn_round_f16(num[j] * rden);
    half_t *const orow = a.out + ((size_t)b * a.rows + qq) * a.ldo + (size_t)h * CA_HD + d0;
    if (sp.nsp == 1) {       // this workgroup is the whole head
        if (qq < nr) *(half8_t *)orow = o;
        return;
    }
    // ---- several splits: system-scope records, arrival ticket, the last split merges them in split order ----
    const size_t rstride = (size_t)a.rows * hd / 2;        // uint32 words per split
    const size_t mstride = (size_t)a.heads * a.rows * 2;
    uint32_t *const ro = a.o16 + (size_t)b * S * rstride + ((size_t)qq * hd + (size_t)h * CA_HD + d0) / 2;
    float *const rmd = a.md + (size_t)b * S * mstride + ((size_t)h * a.rows + qq) * 2;
    if (qq < nr) {
        const u32x4 ow4 = __builtin_bit_cast(u32x4, o);
#pragma unroll
        for (int j = 0; j < 4; j++) __hip_atomic_store(ro + (size_t)s * rstride + j, ow4[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if ((tid & 15) == 0) {
            __hip_atomic_store(rmd + (size_t)s * mstride, Mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(rmd + (size_t)s * mstride + 1, den, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    if (!attn_ticket_last(a.tickets + (size_t)b * a.heads + h, sp.nsp, &last_flag) || qq >= nr) return;
    half_t res[8];
    attn_merge_records(rmd, mstride, ro, rstride, sp.nsp, res);
    *(half8_t *)orow = half8_t{res[0], res[1], res[2], res[3], res[4], res[5], res[6], res[7]};
}

// S of the launch's grid: as the decode attention of one row (heads x S <= 256 workgroups, at most ATT_MAX_SPLITS, one split per tile of tokens)
int chunk_attn_grid_splits(int heads, int t_max) { return decode_attn_grid_splits(heads, t_max, 1); }

// active splits of a call whose rows end at token `len` (= p + rows, capped at t_max): what attn_split() gives the kernel
int chunk_attn_active_splits(int heads, int t_max, int len) { return attn_split(len, chunk_attn_grid_splits(heads, t_max), CA_TPS).nsp; }

size_t chunk_attn_batch_ws_bytes(int seqs, int rows, int heads, int t_max) { return chunk_attn_ws(seqs, rows, heads, t_max).bytes; }

size_t chunk_attn_ws_bytes(int rows, int heads, int t_max) { return chunk_attn_batch_ws_bytes(1, rows, heads, t_max); }

// seqs sequences of `rows` rows each -- packed rows b rows .. b rows + rows - 1 of qkv / out, cache slot b (slot_stride elements apart), position
// pos[b] on the device -- in the same two launches: the sequence is blockIdx.z of both kernels, everything else is per sequence what it is for one
// (the same attn_split() cut from the same grid split count S, tickets per (sequence, head))
int chunk_attn_batch_launch(const half_t *qkv, int64_t ldq, int seqs, int rows, const int64_t *pos, half_t *kc, half_t *vc, int64_t slot_stride,
                            half_t *out, int64_t ldo, void *ws, int heads, int t_max, float base, float scale, const float *rope_table,
                            hipStream_t s) {
    const ChunkAttnWs w = chunk_attn_ws(seqs, rows, heads, t_max);
    half_t *qrot = (half_t *)((char *)ws + w.qrot);
    ChunkAttnArgs a{};
    a.o16 = (uint32_t *)((char *)ws + w.o16);
    a.md = (float *)((char *)ws + w.md);
    a.tickets = (unsigned *)((char *)ws + w.tickets);
    hipLaunchKernelGGL(chunk_rope_kv_kernel, dim3(rows, heads, seqs), dim3(CA_HD / 2), 0, s, qkv, ldq, pos, kc, vc, slot_stride, qrot, a.tickets, heads,
                       t_max, rope_inv_base(base, CA_HD), (const float2 *)rope_table);
    a.q = qrot; a.pos = pos; a.kc = kc; a.vc = vc; a.out = out;
    a.heads = heads; a.rows = rows; a.t_max = t_max; a.ldo = ldo; a.slot_stride = slot_stride;
    a.scale2 = scale * 1.44269504088896340736f;
    hipLaunchKernelGGL(chunk_attn_kernel, dim3(heads, w.S, seqs), dim3(CA_NW * 64), 0, s, a);
    return (int)hipGetLastError();
}

int chunk_attn_launch(const half_t *qkv, int64_t ldq, int rows, const int64_t *pos, half_t *kc, half_t *vc, half_t *out, int64_t ldo, void *ws,
                      int heads, int t_max, float base, float scale, const float *rope_table, hipStream_t s) {
    return chunk_attn_batch_launch(qkv, ldq, 1, rows, pos, kc, vc, 0, out, ldo, ws, heads, t_max, base, scale, rope_table, s);
}

}  // namespace gptq
