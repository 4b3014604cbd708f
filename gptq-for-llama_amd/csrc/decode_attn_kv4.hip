// decode_attn_kv4.hip -- the decode attention of decode_attn.hip (RoPE + KV append + single-query attention in one launch, run-time splits,
// per-wave online softmax, one LDS meeting, ticket merge) over a 4-BIT K/V cache, and the kernel that converts rows of an fp16 cache into that
// format (the prompt paths).  The format (include/gptq_mi355x.h "int4 KV cache"):
//   k4 / v4       uint8 [slot][t_max][heads * 64]     4-bit codes c, two per byte, 16 bytes per group of 32 consecutive values of a head row
//   kmeta / vmeta fp16  [slot][t_max][heads][4][2]    {d, m} per group: the stored value means m + d c
// kv4_quant_group below is the rule (every step one IEEE fp32 operation; this unit is built without contraction and without fast-math).
//
// The algebra.  Nothing in the inner loops touches d or m per element:
//   score = sum_g ( d_g sum_{i in g} q_i c_i + m_g sum_{i in g} q_i )        the group sums of q once per row, then q . codes and two scalars
//   out_i = sum_t (p_t d_tg) c_ti + sum_t p_t m_tg                            one more accumulator per group for the minimum term
// A nibble OR-ed into bits 6 .. 9 of the fp16 pattern of 16.0 is the fp16 value 16 + c (the magic offsets of stripe_unpack.inc), so a word of
// eight codes becomes four fp16 PAIRS by one shift and one v_and_or_b32 each; the nibble order of the format is chosen so that each pair is two
// NEIGHBOURING elements.  K: v_dot2_f32_f16 of the pair with the fp16 pair of q; V: two mixed-precision fmas.  The offset 16 moves into the scalars:
// d (q . (16 + c)) + (m - 16 d) sum q, and p d (16 + c) + p (m - 16 d).  It costs one bit (16 + c < 32 against c < 16), not the seven of 1024 + c.
//
// A 16-byte load is exactly one group: 4 lanes hold a head row, a lane OWNS a group -- its codes, its {d, m} (one 4-byte load per key), its 32
// output dims -- so the quantiser and the metadata need no cross-lane traffic at all.  A wave instruction covers 16 timesteps, a pass of the four
// waves 64, a tile of 8 passes 512: per lane the 8 + 8 loads of 16 bytes per tile, two tiles in flight, of the fp16 and fp8 kernels.
#include <algorithm>
#include <type_traits>

#include "attn_device.h"
#include "gptq_internal.h"

namespace gptq {

constexpr uint32_t KV4_MASK = 0x03C003C0u;    // bits 6 .. 9 of both halves: the top four mantissa bits of fp16
constexpr uint32_t KV4_MAGIC = 0x4C004C00u;   // fp16 16.0 in both halves: (field & MASK) | MAGIC = {16 + c, 16 + c'}
constexpr float KV4_OFF = 16.f;

// ---- the quantiser, written once for the attention's owner split and for the store kernel ---------------------------------------------------
// 32 consecutive fp16 values (one group) -> 16 bytes of codes and the group's {d, m} as one word (d in the low half).
// Word w of the codes holds elements 8w .. 8w + 7: nibble s (bits 4s ..) = element 8w + 2s, nibble 4 + s = element 8w + 2s + 1, s = 0 .. 3.
GPTQ_DEV u32x4 kv4_quant_group(const half8_t (&r)[4], uint32_t &meta) {
    float lo = (float)r[0][0], hi = lo;
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int i = 0; i < 8; i++) {
            lo = fminf(lo, (float)r[j][i]);
            hi = fmaxf(hi, (float)r[j][i]);
        }
    lo += 0.0f;                                              // a minimum or maximum of -0 counts as +0: the bytes do not depend on which zero
    hi += 0.0f;                                              // a min / max of mixed zeros returns
    const half_t d = (half_t)((hi - lo) / 15.0f);            // IEEE division, one rounding to fp16 (RNE)
    const float inv = 1.0f / (float)d;                       // (inf when d == 0: not used then)
    u32x4 q;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        uint32_t word = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const float c = fminf(fmaxf(__builtin_rintf(((float)r[w][i] - lo) * inv), 0.f), 15.f);
            word |= (uint32_t)(int)c << (4 * ((i >> 1) + 4 * (i & 1)));
        }
        q[w] = d == (half_t)0 ? 0u : word;
    }
    meta = (uint32_t)__builtin_bit_cast(uint16_t, d) | ((uint32_t)__builtin_bit_cast(uint16_t, (half_t)lo) << 16);
    return q;
}
// pair s (0 .. 3) of a word of codes: {16 + element 2s, 16 + element 2s + 1} as fp16
// (mask in an SGPR, magic in a VGPR: the and-or is ONE v_and_or_b32, which takes no literal on this target)
struct Kv4Consts {
    uint32_t mask, magic;
};
GPTQ_DEV Kv4Consts kv4_consts() { return Kv4Consts{sreg_const(KV4_MASK), vreg_const(KV4_MAGIC)}; }
template <int S>
GPTQ_DEV half2_t kv4_pair(uint32_t w, const Kv4Consts &c) {
    const uint32_t f = S == 0 ? w << 6 : (S == 1 ? w << 2 : (S == 2 ? w >> 2 : w >> 6));
    return as_half2((f & c.mask) | c.magic);
}
// {d, m} of a group -> the two scalars of the algebra above: d and m - 16 d
GPTQ_DEV void kv4_meta(uint32_t meta, float &d, float &mo) {
    const half2_t h = as_half2(meta);
    d = (float)h[0];
    mo = __builtin_fmaf(-KV4_OFF, d, (float)h[1]);
}

// ---------------------------------------------------------------------------------------
// The streaming decode attention over the int4 cache.  grid = (heads, rows of the decode batch, S splits), 256 threads; everything that is not
// about the cache format is the fp16 / fp8 kernel's: the split rule and the workspace of attn_split.h, an idle row (pos < 0 or >= t_max) reads
// and writes nothing, K / V rows by buffer loads whose descriptor ends at the split's last old row (lanes past it read zeros without a memory
// request), the next tile requested before the current one is used, scores in the log2 domain, one split stores the row itself, several go
// through the system-scope records and the arrival ticket of attn_device.h.
// The split that owns position `pos` rotates the new k, quantises k and v from LDS (every lane its own group), attends to the QUANTISED row
// -- a step is a function of the cache alone -- and appends codes and metadata at the end.
// ---------------------------------------------------------------------------------------
struct AttnKv4Args {
    const half_t *qkv;
    const int64_t *pos;
    uint8_t *k4, *v4;
    uint32_t *kmeta, *vmeta;     // {d, m} fp16 pairs as words
    half_t *out;
    half_t *o16;                 // records: [batch][S][heads * 128] fp16 partial outputs
    float *md;                   //          [batch][S][heads] {M, den}
    unsigned *tickets;
    const float2 *rope_tab;
    const int32_t *out_perm;
    int heads, t_max, ldq, ldo, tps;
    float inv_base, scale2;      // scale2 = softmax scale x log2(e)
};

GPTQ_DEV u32x4 kv4_load16(__amdgpu_buffer_rsrc_t r, int voff) {
    return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0));
}
GPTQ_DEV uint32_t kv4_load4(__amdgpu_buffer_rsrc_t r, int voff) { return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(r, voff, 0, 0); }

constexpr int KV4_NW = 4;                    // waves of a split
constexpr int KV4_GB = 16;                   // bytes of a group's codes: 4 lanes per timestep
constexpr int KV4_ROWB = ATT_HD / 2;         // bytes of a head row's codes
constexpr int KV4_RP = KV4_NW * 16;          // timesteps per pass of the workgroup (16 per wave instruction)
constexpr int KV4_NP = 8;                    // passes per tile = 16-byte K (and V) loads per lane and tile
constexpr int KV4_TILE = KV4_RP * KV4_NP;    // 512 timesteps: a multiple of ATT_TILE, the unit of a split's range
static_assert(KV4_TILE % ATT_TILE == 0, "a split's range is cut in units of ATT_TILE");

__global__ void __launch_bounds__(KV4_NW * 64) attn_stream_kv4_kernel(const AttnKv4Args a) {
    constexpr int NW = KV4_NW, RP = KV4_RP, NP = KV4_NP, TILE = KV4_TILE;
    __shared__ __attribute__((aligned(16))) half_t qh[ATT_HD];
    __shared__ __attribute__((aligned(16))) half_t knew[ATT_HD];
    __shared__ __attribute__((aligned(16))) half_t vnew[ATT_HD];
    __shared__ __attribute__((aligned(16))) float accs[NW][ATT_HD];
    __shared__ float mw[NW], lw[NW];
    __shared__ int last_flag;
    const int h = blockIdx.x, b = blockIdx.y, s = blockIdx.z, S = gridDim.z;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hd = a.heads * ATT_HD;
    const int ocol = tid < ATT_HD ? (a.out_perm ? a.out_perm[h * ATT_HD + tid] : h * ATT_HD + tid) : 0;
    // this row's q / k / v halves of the head, requested before the position is known (as attn_stream_kernel)
    const half_t *qrow = a.qkv + (size_t)b * a.ldq;
    half_t q0 = (half_t)0, q1 = (half_t)0, k0 = (half_t)0, k1 = (half_t)0, nv0 = (half_t)0, nv1 = (half_t)0;
    if (tid < ATT_HD / 2) {
        const half_t *q = qrow + (size_t)h * ATT_HD + tid;
        q0 = q[0]; q1 = q[ATT_HD / 2];
        k0 = q[hd]; k1 = q[hd + ATT_HD / 2];
        nv0 = q[2 * hd]; nv1 = q[2 * hd + ATT_HD / 2];
    }
    const int64_t pos64 = ((const __attribute__((address_space(4))) int64_t *)a.pos)[b];
    if (pos64 < 0 || pos64 >= a.t_max) return;
    const int pos = (int)pos64, len = pos + 1;
    const AttnSplit sp = attn_split(len, S, a.tps);
    if (s >= sp.nsp) return;
    const int t0 = s * sp.chunk;
    const int t_end = min(t0 + sp.chunk, len);   // this split attends to rows [t0, t_end)
    const bool owner = t_end == len;             // ... the last of which is the new token
    const int n_old = min(t_end, pos);           // cache rows of this split: [t0, n_old)
    const int ntiles = (t_end - t0 + TILE - 1) / TILE;   // >= 1
    const int g = tid & 3, tsub = tid >> 2;      // this lane: group g (dims [32 g, 32 g + 32)) of timestep tsub of a pass

    // descriptors over rows [0, n_old) of this (row, head), codes and metadata: anything past the split's last cache row reads as zero
    const int rowb = a.heads * KV4_ROWB, rowm = a.heads * 16;                // bytes between timesteps: codes, metadata
    const size_t slice = ((size_t)b * a.t_max) * rowb + (size_t)h * KV4_ROWB;
    const size_t mslice = ((size_t)b * a.t_max) * a.heads * 4 + (size_t)h * 4;    // in words
    const int nrec = n_old > 0 ? (n_old - 1) * rowb + KV4_ROWB : 0;
    const int nrec_m = n_old > 0 ? (n_old - 1) * rowm + 16 : 0;
    const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void *)(a.k4 + slice), 0, nrec, 0x00020000);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void *)(a.v4 + slice), 0, nrec, 0x00020000);
    const __amdgpu_buffer_rsrc_t rkm = __builtin_amdgcn_make_buffer_rsrc((void *)(a.kmeta + mslice), 0, nrec_m, 0x00020000);
    const __amdgpu_buffer_rsrc_t rvm = __builtin_amdgcn_make_buffer_rsrc((void *)(a.vmeta + mslice), 0, nrec_m, 0x00020000);
    struct Tile {
        u32x4 K[NP], V[NP];
        uint32_t MK[NP], MV[NP];
    };
    Tile A, B;
    auto load = [&](Tile &T, int tb) {
        const int vo = (tb + tsub) * rowb + g * KV4_GB, mo = (tb + tsub) * rowm + g * 4;
#pragma unroll
        for (int it = 0; it < NP; it++) T.MK[it] = kv4_load4(rkm, mo + it * RP * rowm);
#pragma unroll
        for (int it = 0; it < NP; it++) T.K[it] = kv4_load16(rk, vo + it * RP * rowb);
#pragma unroll
        for (int it = 0; it < NP; it++) T.MV[it] = kv4_load4(rvm, mo + it * RP * rowm);
#pragma unroll
        for (int it = 0; it < NP; it++) T.V[it] = kv4_load16(rv, vo + it * RP * rowb);
    };
    load(A, t0);
    __builtin_amdgcn_sched_barrier(0);

    // ---- RoPE of q (every split) and of the new k (owner) under the latency of the first tile ----
    if (tid < ATT_HD / 2) {
        const int c = tid;
        float cs, sn;
        rope_cos_sin(a.rope_tab, pos, c, ATT_HD / 2, a.inv_base, cs, sn);
        half_t rq0, rq1;
        rope_rotate(q0, q1, cs, sn, rq0, rq1);
        qh[c] = rq0;
        qh[c + ATT_HD / 2] = rq1;
        if (owner) {
            half_t nk0, nk1;
            rope_rotate(k0, k1, cs, sn, nk0, nk1);
            knew[c] = nk0;
            knew[c + ATT_HD / 2] = nk1;
            vnew[c] = nv0;
            vnew[c + ATT_HD / 2] = nv1;
        }
    }
    __syncthreads();
    // this lane's group of the rotated query as 16 fp16 pairs, and the group's sum (once per row)
    half2_t qp[16];
    float qsum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const half8_t v = *(const half8_t *)(qh + g * 32 + j * 8);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            qp[4 * j + i] = half2_t{v[2 * i], v[2 * i + 1]};
            qsum += (float)v[2 * i] + (float)v[2 * i + 1];
        }
    }
    // the new token's row in the cache format: this lane's group of k and of v (owner only; the fp16 rows are in LDS)
    u32x4 kn = u32x4{0u, 0u, 0u, 0u}, vn = u32x4{0u, 0u, 0u, 0u};
    uint32_t mkn = 0u, mvn = 0u;
    if (owner) {
        half8_t r[4];
#pragma unroll
        for (int j = 0; j < 4; j++) r[j] = *(const half8_t *)(knew + g * 32 + j * 8);
        kn = kv4_quant_group(r, mkn);
#pragma unroll
        for (int j = 0; j < 4; j++) r[j] = *(const half8_t *)(vnew + g * 32 + j * 8);
        vn = kv4_quant_group(r, mvn);
    }

    // ---- the wave's running state: M (log2 domain), l, acc[32 dims of this lane] and the minimum term sm, relative to M ----
    const Kv4Consts uc = kv4_consts();
    float M = ATT_M_FLOOR, l = 0.f, sm = 0.f, av[32];
#pragma unroll
    for (int j = 0; j < 32; j++) av[j] = 0.f;
    auto score = [&](const u32x4 k, uint32_t meta) {     // scale2 (q . k^): the same value in the 4 lanes of the timestep
        float dot = 0.f;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            dot = __builtin_amdgcn_fdot2(qp[4 * w], kv4_pair<0>(k[w], uc), dot, false);
            dot = __builtin_amdgcn_fdot2(qp[4 * w + 1], kv4_pair<1>(k[w], uc), dot, false);
            dot = __builtin_amdgcn_fdot2(qp[4 * w + 2], kv4_pair<2>(k[w], uc), dot, false);
            dot = __builtin_amdgcn_fdot2(qp[4 * w + 3], kv4_pair<3>(k[w], uc), dot, false);
        }
        float d, mo;
        kv4_meta(meta, d, mo);
        float v = __builtin_fmaf(d, dot, mo * qsum);
        v += dpp_row_f32<0xB1>(v);           // the four groups of the head row: xor 1, 2
        v += dpp_row_f32<0x4E>(v);
        return v * a.scale2;
    };
    auto wave_max = [&](float v) {           // the wave's 16 timesteps: the other three of this 16-lane row (row_ror 8, 4), then the four rows
        v = fmaxf(v, dpp_row_f32<0x128>(v));
        v = fmaxf(v, dpp_row_f32<0x124>(v));
        return rows_max(v);
    };
    auto accumulate = [&](const u32x4 v, float p, uint32_t meta) {
        float d, mo;
        kv4_meta(meta, d, mo);
        const float pd = p * d;
        sm = __builtin_fmaf(p, mo, sm);
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const half2_t c0 = kv4_pair<0>(v[w], uc), c1 = kv4_pair<1>(v[w], uc), c2 = kv4_pair<2>(v[w], uc), c3 = kv4_pair<3>(v[w], uc);
            float *o = av + 8 * w;
            o[0] = __builtin_fmaf(pd, (float)c0[0], o[0]);
            o[1] = __builtin_fmaf(pd, (float)c0[1], o[1]);
            o[2] = __builtin_fmaf(pd, (float)c1[0], o[2]);
            o[3] = __builtin_fmaf(pd, (float)c1[1], o[3]);
            o[4] = __builtin_fmaf(pd, (float)c2[0], o[4]);
            o[5] = __builtin_fmaf(pd, (float)c2[1], o[5]);
            o[6] = __builtin_fmaf(pd, (float)c3[0], o[6]);
            o[7] = __builtin_fmaf(pd, (float)c3[1], o[7]);
        }
    };
    // a tile.  FULL: all of its rows are cache rows of this split.  Otherwise a pass that lies wholly past t_end is skipped (a branch the whole
    // workgroup takes together: a first token costs one pass, not eight), rows past t_end are masked, and the lanes that hold position `pos`
    // take that row from the registers above (the new token is not in the cache yet).
    auto tile_any = [&](const Tile &T, int tb, auto full) {
        constexpr bool FULL = decltype(full)::value;
        float sc[NP];
        float mt = -INFINITY;
#pragma unroll
        for (int it = 0; it < NP; it++) {
            sc[it] = -INFINITY;
            if (!FULL && tb + it * RP >= t_end) continue;
            const int t = tb + it * RP + tsub;
            const bool isnew = !FULL && owner && t == pos;
            const float v = score(isnew ? kn : T.K[it], isnew ? mkn : T.MK[it]);
            sc[it] = (FULL || t < t_end) ? v : -INFINITY;
            mt = fmaxf(mt, sc[it]);
        }
        mt = wave_max(mt);
        const float Mn = fmaxf(M, mt), alpha = __builtin_amdgcn_exp2f(M - Mn);
        l *= alpha;
        sm *= alpha;
#pragma unroll
        for (int j = 0; j < 32; j++) av[j] *= alpha;
#pragma unroll
        for (int it = 0; it < NP; it++) {
            if (!FULL && tb + it * RP >= t_end) continue;
            const bool isnew = !FULL && owner && tb + it * RP + tsub == pos;
            const float p = __builtin_amdgcn_exp2f(sc[it] - Mn);     // masked slots hold -inf: 0
            l += p;
            accumulate(isnew ? vn : T.V[it], p, isnew ? mvn : T.MV[it]);
        }
        M = Mn;
    };
    auto tile = [&](const Tile &T, int tb) {
        if (tb + TILE <= n_old) tile_any(T, tb, std::true_type());
        else tile_any(T, tb, std::false_type());
    };
    if (ntiles == 1) {       // every context up to a tile: one register set, no loop
        tile(A, t0);
    } else {
        for (int i = 0; i < ntiles; i += 2) {
            load(B, t0 + (i + 1) * TILE);                            // (past the split's rows: zeros, no traffic)
            __builtin_amdgcn_sched_barrier(0);
            tile(A, t0 + i * TILE);
            __builtin_amdgcn_sched_barrier(0);
            load(A, t0 + (i + 2) * TILE);
            __builtin_amdgcn_sched_barrier(0);
            if (i + 1 < ntiles) tile(B, t0 + (i + 1) * TILE);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (owner && tid < 4) {    // append the new token's row (nothing in this launch reads it back), after the last cache load has been consumed
        *(u32x4 *)(a.k4 + slice + (size_t)pos * rowb + tid * KV4_GB) = kn;
        *(u32x4 *)(a.v4 + slice + (size_t)pos * rowb + tid * KV4_GB) = vn;
        a.kmeta[mslice + (size_t)pos * a.heads * 4 + tid] = mkn;
        a.vmeta[mslice + (size_t)pos * a.heads * 4 + tid] = mvn;
    }

    // ---- the minimum term joins its group's dims; the wave's 16 timesteps -> one, the NW waves -> one (LDS): {Mx, den, num[tid]} of the split ----
    auto wave_sum = [&](float v) {           // over the lanes of this group: row_ror 8, 4 inside the 16-lane row, then the four rows
        v += dpp_row_f32<0x128>(v);
        v += dpp_row_f32<0x124>(v);
        return rows_sum(v);
    };
#pragma unroll
    for (int j = 0; j < 32; j++) av[j] = wave_sum(av[j] + sm);
    l = wave_sum(l);
    if (lane < 4) {
#pragma unroll
        for (int j = 0; j < 32; j += 4) *(float4_t *)(&accs[wave][lane * 32 + j]) = float4_t{av[j], av[j + 1], av[j + 2], av[j + 3]};
    }
    if (lane == 0) {
        mw[wave] = M;
        lw[wave] = l;
    }
    __syncthreads();
    float Mx = mw[0];
#pragma unroll
    for (int w = 1; w < NW; w++) Mx = fmaxf(Mx, mw[w]);
    float num = 0.f, den = 0.f;
    if (tid < ATT_HD) {
#pragma unroll
        for (int w = 0; w < NW; w++) {
            const float e = __builtin_amdgcn_exp2f(mw[w] - Mx);
            num = __builtin_fmaf(e, accs[w][tid], num);
            den = __builtin_fmaf(e, lw[w], den);
        }
    }
    const half_t o = attn_round_f16(num * __builtin_amdgcn_rcpf(den));   // the split's normalised output (one split: the row itself)
    if (sp.nsp == 1) {       // this workgroup is the whole head
        if (tid < ATT_HD) a.out[(size_t)b * a.ldo + ocol] = o;
        return;
    }
    // ---- several splits: system-scope records, arrival ticket, the last split merges ----
    half_t *ro = a.o16 + ((size_t)b * S) * hd + h * ATT_HD;
    float *rmd = a.md + (((size_t)b * S) * a.heads + h) * 2;
    if (tid < ATT_HD) __hip_atomic_store((uint16_t *)(ro + (size_t)s * hd + tid), __builtin_bit_cast(uint16_t, o), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (tid == 0) {
        __hip_atomic_store(rmd + (size_t)s * a.heads * 2, Mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(rmd + (size_t)s * a.heads * 2 + 1, den, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (!attn_ticket_last(a.tickets + (size_t)b * a.heads + h, sp.nsp, &last_flag)) return;
    if (tid < ATT_HD) {
        half_t res[1];
        attn_merge_records(rmd, (size_t)a.heads * 2, (const uint16_t *)ro + tid, hd, sp.nsp, res);
        a.out[(size_t)b * a.ldo + ocol] = res[0];
    }
}

int decode_attn_kv4_launch(const half_t *qkv, const int64_t *pos, uint8_t *k4, uint8_t *v4, half_t *kmeta, half_t *vmeta, half_t *out, float *ws,
                           int heads, int t_max, float base, float scale, const float *rope_table, hipStream_t s, int batch, int64_t ldq,
                           int64_t ldo, const int32_t *out_perm, int tps) {
    const DecodeAttnWs w = decode_attn_ws(batch, heads, t_max);
    AttnKv4Args a{};
    a.qkv = qkv; a.pos = pos; a.k4 = k4; a.v4 = v4; a.kmeta = (uint32_t *)kmeta; a.vmeta = (uint32_t *)vmeta; a.out = out;
    a.o16 = (half_t *)((char *)ws + w.o16);
    a.md = (float *)((char *)ws + w.md);
    a.tickets = (unsigned *)((char *)ws + w.tickets);
    a.rope_tab = (const float2 *)rope_table;
    a.out_perm = out_perm;
    a.heads = heads; a.t_max = t_max; a.ldq = (int)ldq; a.ldo = (int)ldo;
    a.tps = tps > 0 ? tps : decode_attn_tps(false);
    a.inv_base = rope_inv_base(base, ATT_HD);
    a.scale2 = scale * 1.44269504088896340736f;
    hipLaunchKernelGGL(attn_stream_kv4_kernel, dim3(heads, batch, w.S), dim3(KV4_NW * 64), 0, s, a);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// fp16 cache rows -> int4 cache rows at the same coordinates, for a table of segments (the prompt paths: prompt attention runs on an fp16
// staging cache, this converts what it appended).  grid = (groups of the longest segment / 256, segments, 2: K / V), 256 threads: a thread
// owns one group -- four 16-byte loads, the quantiser above, one 16-byte store and one 4-byte store.
// ---------------------------------------------------------------------------------------
struct Kv4StoreArgs {
    gptq_prompt_seg_t seg[GPTQ_PROMPT_ATTN_MAX_SEQS];
    const half_t *src[2];
    uint8_t *dst[2];
    uint32_t *meta[2];
    int64_t slot_stride;
    int heads, t_max;
};

__global__ void __launch_bounds__(256) kv4_store_kernel(const Kv4StoreArgs a) {
    const gptq_prompt_seg_t sg = a.seg[blockIdx.y];
    const int kv = blockIdx.z;
    const int64_t unit = (int64_t)blockIdx.x * 256 + threadIdx.x;           // group of the segment: (row, head, group)
    if (unit >= (int64_t)sg.rows * a.heads * 4) return;
    const int64_t r = unit / (a.heads * 4), hg = unit - r * (a.heads * 4);  // hg = head * 4 + group: 32 values each
    const int64_t t = (int64_t)sg.start + r;
    const half_t *src = a.src[kv] + sg.slot * a.slot_stride + (t * a.heads * 4 + hg) * 32;
    half8_t v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = *(const half8_t *)(src + 8 * j);
    uint32_t meta;
    const u32x4 q = kv4_quant_group(v, meta);
    const int64_t grp = ((int64_t)sg.slot * a.t_max + t) * a.heads * 4 + hg;
    *(u32x4 *)(a.dst[kv] + grp * KV4_GB) = q;
    a.meta[kv][grp] = meta;
}

int kv4_store_launch(const half_t *k16, const half_t *v16, int64_t slot_stride, const gptq_prompt_seg_t *segs, int nseq, uint8_t *k4, uint8_t *v4,
                     half_t *kmeta, half_t *vmeta, int heads, int t_max, hipStream_t s) {
    Kv4StoreArgs a{};
    int most = 0;
    for (int i = 0; i < nseq; i++) {
        a.seg[i] = segs[i];
        most = std::max(most, segs[i].rows);
    }
    a.src[0] = k16; a.src[1] = v16;
    a.dst[0] = k4; a.dst[1] = v4;
    a.meta[0] = (uint32_t *)kmeta; a.meta[1] = (uint32_t *)vmeta;
    a.slot_stride = slot_stride;
    a.heads = heads; a.t_max = t_max;
    const unsigned blocks = (unsigned)(((int64_t)most * heads * 4 + 255) / 256);
    hipLaunchKernelGGL(kv4_store_kernel, dim3(blocks, nseq, 2), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace gptq
