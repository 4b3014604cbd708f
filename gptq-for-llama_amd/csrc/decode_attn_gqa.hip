// decode_attn_gqa.hip -- the batch decode attention for GROUPED-QUERY models: `heads` query heads share `kv_heads` K/V heads, G = heads / kv_heads
// query heads per K/V head (2 .. 16, any integer: Qwen2-7B has 7).  Reference: what HF's repeat_kv + F.scaled_dot_product_attention compute for
// one new token per row (quant/fused_attn.py:126-158 with the K/V heads repeated G times) -- here WITHOUT the repeat: one workgroup streams a
// K/V head's history once and serves the G query heads of its group with it.  The streaming kernel of decode_attn.hip on a repeated cache
// reads G times the bytes.
//
// Layouts: a qkv row is [heads 128 q | kv_heads 128 k | kv_heads 128 v]; a cache slice is [t_max][kv_heads 128]; out is [heads 128].
// Two launches, as the chunk entry (chunk_attn.hip):
//   1. gqa_rope_kv_kernel, grid (heads + kv_heads, batch): the shared RoPE of attn_device.h.  Blocks x < heads rotate one query head into the
//      workspace (qkv is never written); blocks x >= heads rotate one K head into the cache row p, copy its V row -- ONCE per K/V head -- and
//      clear the head's arrival ticket.  The kernel boundary orders the append against every read of launch 2: the tile that holds position p
//      reads the appended row from the cache like any other.
//   2. gqa_attn_kernel, grid (kv_heads, S, batch): the unit of work is (row, K/V head, split); the key range [0, p] is cut by attn_split() at
//      run time.  A split is a workgroup of four waves; a wave walks tiles of 32 keys with an online softmax (log2 domain) per query column.
//      The G rotated queries are the 16 query columns of the chunk kernel's tile (columns >= G are zero and never stored):
//        S^T[key][query] = K Q^T     v_mfma_f32_16x16x32_f16, K from global memory in the A layout (lane = key, 64 contiguous bytes per lane),
//                                    Q^T fragments in registers for the whole walk; the softmax scale multiplies the fp32 product (a query
//                                    scaled in fp16 would carry a rounding of its own into every logit);
//        O^T[dim][query] += V^T P^T  the accumulator layout of the first product is the B operand of the second; V^T comes through
//                                    ds_read_b64_tr_b16 from the wave's own swizzled LDS image of the V tile (attn_device.h).  P goes in as TWO
//                                    fp16 terms, hi = fp16(p) and lo = fp16(p - hi), two MFMAs into the same accumulator: the output is held
//                                    to the bar of the streaming kernel, which keeps p in fp32 -- a single fp16 p would cost 2^-11 of
//                                    sum w |v|.  The second MFMA is free: the walk waits on memory.
//      There is no causal mask between the columns: all of them sit at position p.  The next tile's K / V are requested into registers before
//      the current one is computed; no workgroup barrier inside the walk.  The four waves meet once (attn_waves_meet); one active split stores
//      the rows, several go through the split hand-off of attn_device.h (system-scope records, attn_ticket_last, attn_merge_records) -- the only
//      global atomics.  The ticket decides who merges, never what is computed: same inputs, same bits.
// Bounds: keys beyond p are never loaded (their slots of a tile are zeros and masked before the maximum).  A position < 0 or >= t_max idles the
// row in both launches: nothing of qkv or the caches is read, neither the caches nor out are written.
#include <algorithm>

#include "attn_device.h"
#include "gptq_internal.h"

namespace gptq {

constexpr int GA_HD = 128;     // head_dim served
constexpr int GA_NW = 4;       // waves per workgroup
constexpr int GA_KT = 32;      // keys per wave tile (two 16-key MFMA blocks)
constexpr int GA_QC = 16;      // query columns of the MFMA (the group padded to it)
constexpr int GA_TPS = 128;    // tokens a split owns at least: the grid has kv_heads x batch units before it is cut, G times fewer than the
                               // streaming kernel's, so a row is cut as soon as a further split has a full tile for each of its waves
constexpr int GA_MAX_BATCH = 16;

// S of the launch's grid (and of the workspace layout): the decode attention's rule on the units of this kernel
static int gqa_grid_splits(int kv_heads, int t_max, int batch) { return decode_attn_grid_splits(kv_heads, t_max, batch); }

// workspace: rotated q [batch][heads 128] fp16 | records [batch][S][heads 128] fp16 | {M, den} [batch][S][heads] fp32 x 2 | tickets
// [batch][kv_heads], each part rounded up to 256 bytes
struct GqaAttnWs {
    int S;
    size_t qrot, o16, md, tickets, bytes;
};
static GqaAttnWs gqa_attn_ws(int batch, int heads, int kv_heads, int t_max) {
    const auto align = [](size_t n) { return (n + 255) & ~(size_t)255; };
    GqaAttnWs w{};
    w.S = gqa_grid_splits(kv_heads, t_max, batch);
    const size_t n = (size_t)batch, hd = (size_t)heads * GA_HD;
    w.qrot = 0;
    w.o16 = w.qrot + align(n * hd * sizeof(_Float16));
    w.md = w.o16 + align(n * w.S * hd * sizeof(_Float16));
    w.tickets = w.md + align(n * w.S * heads * 2 * sizeof(float));
    w.bytes = w.tickets + align(n * kv_heads * sizeof(unsigned));
    return w;
}

__global__ void __launch_bounds__(64) gqa_rope_kv_kernel(const half_t *__restrict__ qkv, int64_t ldq, const int64_t *__restrict__ pos_ptr,
                                                         half_t *__restrict__ kc, half_t *__restrict__ vc, half_t *__restrict__ qrot,
                                                         unsigned *__restrict__ tickets, int heads, int kv_heads, int t_max, float inv_base,
                                                         const float2 *__restrict__ tab) {
    const int x = blockIdx.x, b = blockIdx.y, c = threadIdx.x, half = GA_HD / 2;
    const bool is_q = x < heads;
    if (!is_q && c == 0) tickets[(size_t)b * kv_heads + (x - heads)] = 0u;
    const int64_t pos = pos_ptr[b];
    if (pos < 0 || pos >= t_max) return;
    float cs, sn;
    rope_cos_sin(tab, pos, c, half, inv_base, cs, sn);
    const half_t *row = qkv + (size_t)b * ldq;
    if (is_q) {
        rope_rotate(row + (size_t)x * GA_HD + c, qrot + ((size_t)b * heads + x) * GA_HD + c, half, cs, sn);
        return;
    }
    const int j = x - heads, kvd = kv_heads * GA_HD;
    const half_t *k = row + (size_t)heads * GA_HD + (size_t)j * GA_HD + c, *v = k + kvd;
    const size_t at = ((size_t)b * t_max + (size_t)pos) * kvd + (size_t)j * GA_HD + c;
    rope_rotate(k, kc + at, half, cs, sn);
    vc[at] = v[0];
    vc[at + half] = v[half];
}

struct GqaAttnArgs {
    const half_t *q;             // rotated q [batch][heads * 128]
    const int64_t *pos;          // [batch]
    const half_t *kc, *vc;       // [batch][t_max][kv_heads * 128]
    half_t *out;                 // [batch] rows, ldo apart
    const int32_t *out_perm;     // NULL or [heads * 128]: element n of a row is stored at column out_perm[n]
    uint32_t *o16;               // records: [batch][S][heads * 128] fp16 partial outputs (as pairs)
    float *md;                   //          [batch][S][heads] {M, den}
    unsigned *tickets;           //          [batch][kv_heads]
    int heads, kv_heads, group, t_max;
    int64_t ldo;
    float scale2;                // softmax scale x log2(e)
};

__global__ void __launch_bounds__(GA_NW * 64) gqa_attn_kernel(const GqaAttnArgs a) {
    // the waves' V tiles [32 keys][128] fp16; at the end the waves' O [16 queries][128] fp32 (the same 8 KB each)
    __shared__ __attribute__((aligned(16))) half_t vs[GA_NW][GA_KT * GA_HD];
    __shared__ float mw[GA_NW][GA_QC], lw[GA_NW][GA_QC];
    __shared__ int last_flag;
    const int kvh = blockIdx.x, s = blockIdx.y, S = gridDim.y, b = blockIdx.z;   // K/V head, split, splits of the grid, row of the batch
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, qi = lane & 15;               // 16-lane row of the wave, column (= query head of the group)
    const int G = a.group, hd = a.heads * GA_HD, kvd = a.kv_heads * GA_HD;
    const int64_t p64 = ((const __attribute__((address_space(4))) int64_t *)a.pos)[b];
    if (p64 < 0 || p64 >= a.t_max) return;
    const int len = (int)p64 + 1;                          // keys of the row: [0, len), the appended one included
    const AttnSplit sp = attn_split(len, S, GA_TPS);
    if (s >= sp.nsp) return;
    const int t0 = s * sp.chunk;
    const int t_end = min(t0 + sp.chunk, len);             // this split attends to keys [t0, t_end)
    const int ntiles = (t_end - t0 + GA_KT - 1) / GA_KT;   // >= 1
    const half_t *const kc = a.kc + (size_t)b * a.t_max * kvd + (size_t)kvh * GA_HD, *const vc = a.vc + (size_t)b * a.t_max * kvd + (size_t)kvh * GA_HD;
    const int h0 = kvh * G;                                // first query head of the group

    // ---- Q^T fragments (B operand of K Q^T): lane = query head, element j of k-step ks = dim 32 g + 8 ks + j (K's fragments use the same map) ----
    half8_t qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
        qf[ks] = half8_t{0, 0, 0, 0, 0, 0, 0, 0};
        if (qi < G) qf[ks] = *(const half8_t *)(a.q + (size_t)b * hd + (size_t)(h0 + qi) * GA_HD + 32 * g + 8 * ks);
    }
    // A row m of a 16-key block is key 8 ((m >> 2) & 1) + 4 (m >> 3) + (m & 3) of the block: accumulator register r of lane row g then holds
    // key 8 (g & 1) + 4 (g >> 1) + r, and the two 4-row blocks a 32-lane half reads transposed lie 8 rows apart (conflict-free)
    const int krow = 8 * ((qi >> 2) & 1) + 4 * (qi >> 3) + (qi & 3);
    const int kreg0 = 8 * (g & 1) + 4 * (g >> 1);
    const int vrow = lane >> 4, vch = lane & 15;           // V staging: chunk vch of tile rows vrow + 4 i

    u32x4 kA[2][4], vA[8], kB[2][4], vB[8];
    auto request = [&](u32x4 (&K)[2][4], u32x4 (&V)[8], int tb) {
#pragma unroll
        for (int blk = 0; blk < 2; blk++) {
            const int key = tb + 16 * blk + krow;
#pragma unroll
            for (int ks = 0; ks < 4; ks++) {
                K[blk][ks] = u32x4{0u, 0u, 0u, 0u};
                if (key < t_end) K[blk][ks] = *(const u32x4 *)(kc + (size_t)key * kvd + 32 * g + 8 * ks);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int key = tb + vrow + 4 * i;
            V[i] = u32x4{0u, 0u, 0u, 0u};
            if (key < t_end) V[i] = *(const u32x4 *)(vc + (size_t)key * kvd + vch * 8);
        }
    };
    half_t *const img = vs[wave];

    // ---- running state of the lane's query column: M (log2 domain, the same in the four lanes of a column), l (this lane's keys), O^T[dim][query] ----
    float M = ATT_M_FLOOR, l = 0.f;
    float4_t acc[8];
#pragma unroll
    for (int d = 0; d < 8; d++) acc[d] = float4_t{0.f, 0.f, 0.f, 0.f};

    auto tile = [&](const u32x4 (&K)[2][4], const u32x4 (&V)[8], int tb) {
#pragma unroll
        for (int i = 0; i < 8; i++) *(ATTN_LDS u32x4 *)((ATTN_LDS char *)img + attn_lds_off(vrow + 4 * i, vch)) = V[i];
        float4_t sc[2];
#pragma unroll
        for (int blk = 0; blk < 2; blk++) {
            sc[blk] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ks++)
                sc[blk] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8_t, K[blk][ks]), qf[ks], sc[blk], 0, 0, 0);
        }
        float mt = -INFINITY;
#pragma unroll
        for (int blk = 0; blk < 2; blk++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int key = tb + 16 * blk + kreg0 + r;
                float v = sc[blk][r] * a.scale2;
                if (key >= t_end) v = -INFINITY;           // the only mask: every column sits at position p
                sc[blk][r] = v;
                mt = fmaxf(mt, v);
            }
        mt = rows_max(mt);
        const float Mn = fmaxf(M, mt);                     // finite: M starts at the floor
        const float alpha = __builtin_amdgcn_exp2f(M - Mn);
        M = Mn;
        float ps = 0.f;
        half8_t phi, plo;
#pragma unroll
        for (int blk = 0; blk < 2; blk++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float e = __builtin_amdgcn_exp2f(sc[blk][r] - Mn);   // masked slots hold -inf: 0
                ps += e;
                const half_t hi = (half_t)e;
                phi[4 * blk + r] = hi;
                plo[4 * blk + r] = (half_t)(e - (float)hi);               // the difference is exact in fp32
            }
        l = __builtin_fmaf(l, alpha, ps);
#pragma unroll
        for (int d = 0; d < 8; d++) acc[d] *= alpha;
        // O^T[dim][query] += V^T P^T: element j of lane row g is key 16 (j >> 2) + kreg0 + (j & 3) -- what phi / plo hold -- so V^T comes as two
        // transposed 4-key blocks, 16 keys apart; lane 4 q + pp of a 16-lane group supplies row q, columns 4 pp .. 4 pp + 3 of the block
#pragma unroll
        for (int d = 0; d < 8; d++) {
            const int r0 = kreg0 + (qi >> 2), ch = 2 * d + ((qi & 3) >> 1), sub = 8 * (qi & 1);
            const half4_t lo = attn_tr_read(img, attn_lds_off(r0, ch) + sub);
            const half4_t up = attn_tr_read(img, attn_lds_off(r0 + 16, ch) + sub);
            const half8_t vf = half8_t{lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
            acc[d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, plo, acc[d], 0, 0, 0);
            acc[d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, phi, acc[d], 0, 0, 0);
        }
    };

    // the wave's tiles: wave, wave + 4, ... (wave-uniform control flow: EXEC is full at every transposed read)
    if (wave < ntiles) {
        request(kA, vA, t0 + wave * GA_KT);
        for (int i = wave; i < ntiles; i += 2 * GA_NW) {
            const bool more = i + GA_NW < ntiles;
            if (more) request(kB, vB, t0 + (i + GA_NW) * GA_KT);
            tile(kA, vA, t0 + i * GA_KT);
            if (more) {
                if (i + 2 * GA_NW < ntiles) request(kA, vA, t0 + (i + 2 * GA_NW) * GA_KT);
                tile(kB, vB, t0 + (i + GA_NW) * GA_KT);
            }
        }
    }

    // ---- the lane rows of a column -> one, the waves -> one (LDS): {Mx, den, num} of the split per query head ----
    l = rows_sum(l);
    float *const ow = (float *)img;                        // [16 queries][128 dims] fp32: the wave is done with its own V image
#pragma unroll
    for (int d = 0; d < 8; d++) *(ATTN_LDS float4_t *)((ATTN_LDS float *)ow + qi * GA_HD + 16 * d + 4 * g) = acc[d];
    if (g == 0) {
        mw[wave][qi] = M;
        lw[wave][qi] = l;
    }
    __syncthreads();
    const int qq = tid >> 4, d0 = (tid & 15) * 8;          // this thread's query head of the group and its eight dims
    const bool live = qq < G;
    const int h = h0 + (live ? qq : 0);                    // (a column past the group addresses the group's first head and never stores)
    float Mx, den;
    half_t o[8];
    attn_waves_meet<GA_NW, 8>(&mw[0][qq], &lw[0][qq], GA_QC, [&](int w) { return (const float *)vs[w] + qq * GA_HD + d0; }, Mx, den, o);
    half_t *const orow = a.out + (size_t)b * a.ldo;
    const int n0 = h * GA_HD + d0;                         // element of the output row
    const size_t rstride = (size_t)hd / 2;                 // uint32 words per split
    const size_t mstride = (size_t)a.heads * 2;
    uint32_t *const ro = a.o16 + (size_t)b * S * rstride + (size_t)n0 / 2;
    float *const rmd = a.md + (size_t)b * S * mstride + (size_t)h * 2;
    attn_split_finish(o, Mx, den, ro, rstride, rmd, mstride, a.tickets + (size_t)b * a.kv_heads + kvh, &last_flag, sp.nsp, s, live, (tid & 15) == 0,
                      [&](const half_t (&r)[8]) {
                          if (a.out_perm) {
#pragma unroll
                              for (int j = 0; j < 8; j++) orow[a.out_perm[n0 + j]] = r[j];
                          } else {
                              *(half8_t *)(orow + n0) = half8_t{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
                          }
                      });
}

static int gqa_attn_launch(const half_t *qkv, int64_t ldq, const int64_t *pos, half_t *kc, half_t *vc, half_t *out, int64_t ldo, void *ws, int batch,
                           int heads, int kv_heads, int t_max, float base, float scale, const float *rope_table, const int32_t *out_perm,
                           hipStream_t s) {
    const GqaAttnWs w = gqa_attn_ws(batch, heads, kv_heads, t_max);
    half_t *qrot = (half_t *)((char *)ws + w.qrot);
    GqaAttnArgs a{};
    a.o16 = (uint32_t *)((char *)ws + w.o16);
    a.md = (float *)((char *)ws + w.md);
    a.tickets = (unsigned *)((char *)ws + w.tickets);
    hipLaunchKernelGGL(gqa_rope_kv_kernel, dim3(heads + kv_heads, batch), dim3(GA_HD / 2), 0, s, qkv, ldq, pos, kc, vc, qrot, a.tickets, heads, kv_heads,
                       t_max, rope_inv_base(base, GA_HD), (const float2 *)rope_table);
    a.q = qrot; a.pos = pos; a.kc = kc; a.vc = vc; a.out = out; a.out_perm = out_perm;
    a.heads = heads; a.kv_heads = kv_heads; a.group = heads / kv_heads; a.t_max = t_max; a.ldo = ldo;
    a.scale2 = scale * 1.44269504088896340736f;
    hipLaunchKernelGGL(gqa_attn_kernel, dim3(kv_heads, w.S, batch), dim3(GA_NW * 64), 0, s, a);
    return (int)hipGetLastError();
}

// the shapes both entries serve: head_dim 128, 1 .. 16 rows, kv_heads dividing heads with 2 .. 16 query heads per K/V head (one query head per K/V
// head is gptq_decode_attn_batch_f16's case)
static bool gqa_shape_ok(int batch, int heads, int kv_heads, int head_dim, int t_max) {
    if (batch < 1 || batch > GA_MAX_BATCH || heads < 1 || kv_heads < 1 || head_dim != GA_HD || t_max < 1) return false;
    if (heads % kv_heads != 0) return false;
    const int G = heads / kv_heads;
    return G >= 2 && G <= GA_QC;
}

}  // namespace gptq

using namespace gptq;

size_t gptq_decode_attn_batch_gqa_workspace_bytes(int batch, int heads, int kv_heads, int head_dim, int t_max) {
    if (!gqa_shape_ok(batch, heads, kv_heads, head_dim, t_max)) return 0;
    return gqa_attn_ws(batch, heads, kv_heads, t_max).bytes;
}

int gptq_decode_attn_batch_gqa_f16(const void *qkv, int64_t ldq, const int64_t *positions, void *k_cache, void *v_cache, void *out, int64_t ldo,
                                   void *workspace, size_t workspace_bytes, int batch, int heads, int kv_heads, int head_dim, int t_max, float base,
                                   float scale, const float *rope_table, const int32_t *out_perm, gptq_stream_t stream) {
    if (!qkv || !k_cache || !v_cache || !positions || !out || !workspace) return GPTQ_E_NULL;
    if (!gqa_shape_ok(batch, heads, kv_heads, head_dim, t_max) || ldq < ((int64_t)heads + 2 * (int64_t)kv_heads) * head_dim ||
        ldo < (int64_t)heads * head_dim)
        return GPTQ_E_SHAPE;
    if (!aligned(qkv, 16) || !aligned(k_cache, 16) || !aligned(v_cache, 16) || !aligned(out, 16) || !aligned(workspace, 16) || !aligned(positions, 8) ||
        (rope_table && !aligned(rope_table, 8)) || (out_perm && !aligned(out_perm, 4)) || ldq % 8 != 0 || ldo % 8 != 0)
        return GPTQ_E_ALIGN;
    if (workspace_bytes < gqa_attn_ws(batch, heads, kv_heads, t_max).bytes) return GPTQ_E_WORKSPACE;
    return gqa_attn_launch((const half_t *)qkv, ldq, positions, (half_t *)k_cache, (half_t *)v_cache, (half_t *)out, ldo, workspace, batch, heads,
                           kv_heads, t_max, base, scale, rope_table, out_perm, (hipStream_t)stream);
}
