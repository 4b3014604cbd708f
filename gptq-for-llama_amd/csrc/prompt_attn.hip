// prompt_attn.hip -- causal multi-row attention of a PROMPT chunk over the decode engine's own K/V cache: what
// F.scaled_dot_product_attention does for a prompt between the reference's Triton kernels (quant/fused_attn.py:126-158), with the
// RoPE (triton_rotate_half_ :126) and the cache append (torch.cat :142-143) of all rows in front of it.
//
// A SEGMENT is `rows` consecutive tokens of one sequence at positions start .. start + rows - 1; a call serves a table of up to 16 of them
// (gptq_prompt_seg_t: packed rows row0 .. row0 + rows - 1 of one qkv / out matrix, cache slice `slot` of one allocation) in two launches,
// however many segments there are -- the table travels BY VALUE in the launch arguments (256 bytes: nothing is allocated or copied, the
// caller's array is free at once), and a workgroup finds its segment with a scan of scalars (blockIdx and the table: wave-uniform).
// gptq_prompt_attn_f16 is the table of one segment: one kernel body, the same bits.
//   1. prompt_rope_kv_kernel: the shared RoPE + append of attn_device.h (rope_cos_sin, rope_kv_row) per (row, head) -- rotated k and
//      v go to cache rows start + r (bit-identical to a token-by-token feed: the instructions and flags of every other entry), the
//      rotated q to a workspace copy; qkv itself is never written.
//   2. prompt_attn_kernel: flash-style attention, grid = (q tiles of all segments, head); the host sorts the table by start + rows
//      (longest key range first), within a segment the q tiles are issued last (longest) first.  A workgroup is four
//      waves x 32 query rows; it walks the keys [0, last position of the tile] in tiles of 64 with an online softmax (log2 domain).
//      Q fragments live in registers; the K / V tile is requested into registers BEFORE the current tile is computed and written to
//      LDS behind the barrier that ends it.  Both LDS images are the swizzled 256-byte rows of attn_device.h
//      (attn_lds_off): conflict-free for the ds_read_b128 row reads of K and for the ds_read_b64_tr_b16
//      transposed reads of V.  S^T = K Q^T (v_mfma_f32_32x32x16_f16, keys on the registers, the query on the lane: a lane owns half a
//      score row, its partner lane ^ 32 the other half -> max / sum are in-lane plus one permlane32 swap), P is rounded to fp16 in
//      registers and IS the B operand of O^T = V^T P^T (the accumulator layout of the first product is the operand layout of the
//      second, with V^T taken through the transposed read in the same permuted key order).  fp32 accumulation, one fp16 rounding at
//      the store.  No atomics, no scores in memory.
// Masking is a select (-inf before the maximum); cache rows at and beyond start + rows are never loaded (their slots of a tile are
// zeros: 0 * NaN would poison P V).
#include <algorithm>

#include "attn_device.h"
#include "gptq_internal.h"

namespace gptq {

constexpr int PA_HD = 128;    // head_dim served
constexpr int PA_NW = 4;      // waves per workgroup
constexpr int PA_QT = 32 * PA_NW;   // query rows per workgroup (32 per wave: one 32x32 MFMA column block)
constexpr int PA_KT = 64;     // keys per tile

struct PromptSegTable {      // by value in the launch arguments
    gptq_prompt_seg_t seg[GPTQ_PROMPT_ATTN_MAX_SEQS];
    int nseq;
};

// The segment that unit u of a launch falls into, a segment holding ceil(rows / UNIT) units (UNIT = 1: rows, PA_QT: q tiles); u becomes the
// unit within the segment.  u < sum of the units (the grid): the last segment needs no test.  Scalars only.
template <int UNIT>
GPTQ_DEV int pa_find_seg(const PromptSegTable &t, int &u) {
    int si = 0;
    for (; si + 1 < t.nseq; si++) {
        const int n = (t.seg[si].rows + UNIT - 1) / UNIT;
        if (u < n) break;
        u -= n;
    }
    return si;
}

__global__ void __launch_bounds__(64) prompt_rope_kv_kernel(const half_t *__restrict__ qkv, int64_t ldq, const PromptSegTable t,
                                                            half_t *__restrict__ kc, half_t *__restrict__ vc, int64_t slot_stride,
                                                            half_t *__restrict__ qrot, int heads, float inv_base, const float2 *__restrict__ tab) {
    const int h = blockIdx.y, c = threadIdx.x, half = PA_HD / 2;
    int r = blockIdx.x;                                    // r-th row of all segments -> row r of segment si
    const gptq_prompt_seg_t sg = t.seg[pa_find_seg<1>(t, r)];
    const int64_t pos = (int64_t)sg.start + r, row = (int64_t)sg.row0 + r;   // cache row, packed row
    kc += (int64_t)sg.slot * slot_stride;
    vc += (int64_t)sg.slot * slot_stride;
    float cs, sn;
    rope_cos_sin(tab, pos, c, half, inv_base, cs, sn);
    const int hd = heads * PA_HD;
    const half_t *q = qkv + (size_t)row * ldq + (size_t)h * PA_HD + c;
    half_t *qd = qrot + (size_t)row * hd + (size_t)h * PA_HD + c;
    half_t *kd = kc + (size_t)pos * hd + (size_t)h * PA_HD + c;
    half_t *vd = vc + (size_t)pos * hd + (size_t)h * PA_HD + c;
    rope_kv_row(q, q + hd, q + 2 * hd, qd, kd, vd, half, cs, sn);
}

struct PromptAttnArgs {
    const half_t *q;             // rotated q [total rows][heads * 128], packed as qkv
    const half_t *kc, *vc;       // slot s: [t_max][heads * 128] at s * slot_stride; rows [0, start + rows) of a segment's slot are read
    half_t *out;
    int heads;
    int64_t ldo, slot_stride;
    float scale2;                // softmax scale x log2(e)
    PromptSegTable t;            // sorted by start + rows, longest first
};

__global__ void __launch_bounds__(PA_NW * 64) prompt_attn_kernel(const PromptAttnArgs a) {
    __shared__ __attribute__((aligned(16))) half_t ks[PA_KT * PA_HD];
    __shared__ __attribute__((aligned(16))) half_t vs[PA_KT * PA_HD];
    int bid = blockIdx.x;                                  // bid-th q tile of all segments -> tile bid of segment sg
    const gptq_prompt_seg_t sg = a.t.seg[pa_find_seg<PA_QT>(a.t, bid)];
    const int rows = sg.rows, start = sg.start;
    const int qt = (rows + PA_QT - 1) / PA_QT - 1 - bid;   // the last q tile has the longest key range: first
    const half_t *const qs = a.q + (int64_t)sg.row0 * (a.heads * PA_HD);
    const half_t *const kc = a.kc + (int64_t)sg.slot * a.slot_stride, *const vc = a.vc + (int64_t)sg.slot * a.slot_stride;
    half_t *const out = a.out + (int64_t)sg.row0 * a.ldo;
    const int h = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const int hd = a.heads * PA_HD;
    const int q0 = qt * PA_QT;
    const int qrow = q0 + wave * 32 + l31;                 // this lane's query row of the segment (its partner lane ^ 32 has the same)
    const int qpos = start + qrow;
    const int kv_end = start + min(q0 + PA_QT, rows);      // keys the workgroup reads: [0, kv_end)
    const int ntiles = (kv_end + PA_KT - 1) / PA_KT;
    const int wq_min = start + q0 + wave * 32, wq_max = wq_min + 31;   // positions of the wave's rows
    const bool wave_active = q0 + wave * 32 < rows;        // (wave-uniform) a wave of padding rows only stages tiles

    // ---- Q^T fragments (B operand of K Q^T): lane = query, element j of k-step s = dim 16 s + 8 hi + j --------------------------
    half8_t qf[8];
#pragma unroll
    for (int s = 0; s < 8; s++) {
        qf[s] = half8_t{0, 0, 0, 0, 0, 0, 0, 0};
        if (qrow < rows) qf[s] = *(const half8_t *)(qs + (size_t)qrow * hd + (size_t)h * PA_HD + 16 * s + 8 * hi);
    }

    // ---- staging: 1024 16-byte chunks per image and tile, four per thread (16 lanes = one 256-byte head row) ----------------------
    const int srow = tid >> 4, sch = tid & 15;             // chunk i of this thread: row srow + 16 i, chunk sch
    u32x4 kreg[4], vreg[4];
    auto request = [&](int kb) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int key = kb + srow + 16 * i;
            kreg[i] = u32x4{0u, 0u, 0u, 0u};
            vreg[i] = u32x4{0u, 0u, 0u, 0u};
            if (key < kv_end) {
                const size_t g = (size_t)key * hd + (size_t)h * PA_HD + sch * 8;
                kreg[i] = *(const u32x4 *)(kc + g);
                vreg[i] = *(const u32x4 *)(vc + g);
            }
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int off = attn_lds_off(srow + 16 * i, sch);
            *(ATTN_LDS u32x4 *)((ATTN_LDS char *)ks + off) = kreg[i];
            *(ATTN_LDS u32x4 *)((ATTN_LDS char *)vs + off) = vreg[i];
        }
    };

    // ---- running state of the lane's query row: m (log2 domain), l (this lane's half of the keys), O^T[dim][query] ---------------
    float m = -INFINITY, l = 0.f;
    float16_t acc[4];
#pragma unroll
    for (int d = 0; d < 4; d++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[d][r] = 0.f;

    const int g16 = lane & 15, tq = g16 >> 2, tp = g16 & 3, g1 = (lane >> 4) & 1;   // transposed read: row tq of the block, columns 4 tp .. 4 tp + 3

    request(0);
    commit();
    __syncthreads();
    for (int t = 0; t < ntiles; t++) {
        const int kb = t * PA_KT;
        if (t + 1 < ntiles) request(kb + PA_KT);           // in flight under the products of this tile
        if (wave_active && kb <= wq_max) {                 // (wave-uniform) tiles above the wave's diagonal are skipped
            // S^T[key][query] = K Q^T: two blocks of 32 keys
            float16_t sc[2];
#pragma unroll
            for (int b = 0; b < 2; b++) {
#pragma unroll
                for (int r = 0; r < 16; r++) sc[b][r] = 0.f;
#pragma unroll
                for (int s = 0; s < 8; s++) {
                    const half8_t kf = attn_row_read(ks, attn_lds_off(32 * b + l31, 2 * s + hi));
                    sc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s], sc[b], 0, 0, 0);
                }
            }
            // scale into the log2 domain, causal mask (a select), tile maximum of the row
            const bool diag = kb + PA_KT - 1 > wq_min;     // (wave-uniform) the tile reaches past the wave's first row
            float mt = -INFINITY;
#pragma unroll
            for (int b = 0; b < 2; b++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int key = kb + 32 * b + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    float v = sc[b][r] * a.scale2;
                    if (diag && key > qpos) v = -INFINITY;
                    sc[b][r] = v;
                    mt = fmaxf(mt, v);
                }
            mt = halves_max(mt);
            const float mn = fmaxf(m, mt);
            const float msub = mn == -INFINITY ? 0.f : mn;   // a row with nothing unmasked so far: exp2(-inf - 0) = 0, never -inf - -inf
            const float alpha = __builtin_amdgcn_exp2f(m - msub);
            m = mn;
            float ps = 0.f;
            half8_t pf[2][2];
#pragma unroll
            for (int b = 0; b < 2; b++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const float p = __builtin_amdgcn_exp2f(sc[b][r] - msub);
                    ps += p;
                    pf[b][r >> 3][r & 7] = (half_t)p;
                }
            l = __builtin_fmaf(l, alpha, ps);
#pragma unroll
            for (int d = 0; d < 4; d++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[d][r] *= alpha;
            // O^T[dim][query] += V^T P^T.  k-step s of key block b: element j of lane half hi is key 32 b + 16 s + 8 (j >> 2) + 4 hi + (j & 3)
            // -- the order the accumulator registers 8 s .. 8 s + 7 of S^T hold -- so V^T comes as two transposed 4-key blocks, 8 keys apart.
#pragma unroll
            for (int d = 0; d < 4; d++)
#pragma unroll
                for (int b = 0; b < 2; b++)
#pragma unroll
                    for (int s = 0; s < 2; s++) {
                        const int r0 = 32 * b + 16 * s + 4 * hi + tq;
                        const int ch = 4 * d + 2 * g1 + (tp >> 1);
                        const half4_t lo = attn_tr_read(vs, attn_lds_off(r0, ch) + 8 * (tp & 1));
                        const half4_t up = attn_tr_read(vs, attn_lds_off(r0 + 8, ch) + 8 * (tp & 1));
                        const half8_t vf = half8_t{lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
                        acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[b][s], acc[d], 0, 0, 0);
                    }
        }
        __syncthreads();                                   // every wave is done with the tile
        if (t + 1 < ntiles) {
            commit();
            __syncthreads();
        }
    }

    // ---- out[query][32 d + 8 g + 4 hi + (0..3)] = O^T / l: four dims per register quad, one fp16 rounding ----------------------
    l = halves_sum(l);
    if (qrow < rows) {
        const float inv = 1.0f / l;
        half_t *o = out + (size_t)qrow * a.ldo + (size_t)h * PA_HD + 4 * hi;
#pragma unroll
        for (int d = 0; d < 4; d++)
#pragma unroll
            for (int g = 0; g < 4; g++) {
                half4_t v;
#pragma unroll
                for (int j = 0; j < 4; j++) v[j] = (half_t)(acc[d][4 * g + j] * inv);
                *(half4_t *)(o + 32 * d + 8 * g) = v;
            }
    }
}

size_t prompt_attn_ws_bytes(int rows, int heads) { return ((size_t)rows * heads * PA_HD * sizeof(half_t) + 255) & ~(size_t)255; }

int prompt_attn_batch_launch(const half_t *qkv, int64_t ldq, const gptq_prompt_seg_t *segs, int nseq, half_t *kc, half_t *vc, int64_t slot_stride,
                             half_t *out, int64_t ldo, half_t *ws, int heads, float base, float scale, const float *rope_table, hipStream_t s) {
    PromptAttnArgs a{};
    std::copy(segs, segs + nseq, a.t.seg);
    a.t.nseq = nseq;
    // long key ranges first (stable: a table already in that order is launched as it came)
    std::stable_sort(a.t.seg, a.t.seg + nseq,
                     [](const gptq_prompt_seg_t &x, const gptq_prompt_seg_t &y) { return x.start + x.rows > y.start + y.rows; });
    int rows = 0, tiles = 0;
    for (int i = 0; i < nseq; i++) {
        rows += segs[i].rows;
        tiles += (segs[i].rows + PA_QT - 1) / PA_QT;
    }
    hipLaunchKernelGGL(prompt_rope_kv_kernel, dim3(rows, heads), dim3(PA_HD / 2), 0, s, qkv, ldq, a.t, kc, vc, slot_stride, ws, heads,
                       rope_inv_base(base, PA_HD), (const float2 *)rope_table);
    a.q = ws; a.kc = kc; a.vc = vc; a.out = out;
    a.heads = heads; a.ldo = ldo; a.slot_stride = slot_stride;
    a.scale2 = scale * 1.44269504088896340736f;
    hipLaunchKernelGGL(prompt_attn_kernel, dim3(tiles, heads), dim3(PA_NW * 64), 0, s, a);
    return (int)hipGetLastError();
}

int prompt_attn_launch(const half_t *qkv, int64_t ldq, int rows, int64_t start, half_t *kc, half_t *vc, half_t *out, int64_t ldo, half_t *ws,
                       int heads, int t_max, float base, float scale, const float *rope_table, hipStream_t s) {
    const gptq_prompt_seg_t one{0, rows, (int32_t)start, 0};    // the table of one segment
    return prompt_attn_batch_launch(qkv, ldq, &one, 1, kc, vc, 0, out, ldo, ws, heads, base, scale, rope_table, s);
}

}  // namespace gptq
