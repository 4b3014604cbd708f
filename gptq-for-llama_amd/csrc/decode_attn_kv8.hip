// decode_attn_kv8.hip -- the decode attention of decode_attn.hip (attn_stream_kernel: RoPE + KV append + single-query attention in one launch,
// run-time splits, per-wave online softmax, one LDS meeting, ticket merge) over an FP8 K/V cache, and the kernel that converts rows of an fp16
// cache into that format (the prompt paths).  The format (include/gptq_mi355x.h "fp8 KV cache"):
//   k8 / v8     uint8 [slot][t_max][heads * 128]   OCP e4m3fn bytes
//   kexp / vexp int8  [slot][t_max][heads]         one exponent e per (token, head): the stored head row means q_i * 2^e
// A head row r[0..128) of fp16 values is quantised by kv8_quant_row below: e is the smallest integer with max|r| * 2^-e <= 448 (0 for a row of
// zeros), q_i = RNE_e4m3(r_i * 2^-e).  The power of two folds into the per-key scalars of the attention: the score is multiplied by 2^ek, the
// probability by 2^ev (v_ldexp_f32 each), so the inner loops see plain e4m3 -> fp32 conversions (v_cvt_pk_f32_fp8: two elements per instruction).
//
// A 16-byte load is 16 elements here: 8 lanes hold a 128-byte head row, a wave instruction covers 8 timesteps, a pass of the four waves 32, and
// a tile of 8 passes 256 timesteps -- per lane the same 8 + 8 loads of 16 bytes per tile, two tiles in flight, as the fp16 kernel.
// The exponents of a tile are ONE byte load per lane and array (lane j of a row's 8 lanes asks for pass j) handed round by ds_bpermute.
#include <algorithm>
#include <type_traits>

#include "attn_device.h"
#include "gptq_internal.h"

namespace gptq {

// ---- the quantiser, written once for the attention's owner split and for the store kernel -------------------------------------------------
GPTQ_DEV float row_sum8(float v) {    // every lane of an aligned group of 8 ends with the group's sum (xor 1, 2, then the mirror of the half row)
    v += dpp_row_f32<0xB1>(v);
    v += dpp_row_f32<0x4E>(v);
    v += dpp_row_f32<0x141>(v);
    return v;
}
GPTQ_DEV float row_max8(float v) {
    v = fmaxf(v, dpp_row_f32<0xB1>(v));
    v = fmaxf(v, dpp_row_f32<0x4E>(v));
    v = fmaxf(v, dpp_row_f32<0x141>(v));
    return v;
}
// the exponent of a head row with amax = max|r_i| (a finite fp16 magnitude as fp32): amax = m 2^x, m in [0.5, 1) -> x - 9 when m <= 0.875, else
// x - 8; from the bits, so that no libm call and no rounding is involved.  [-32, 8] for every finite fp16 amax.
GPTQ_DEV int kv8_exponent(float amax) {
    const uint32_t u = __builtin_bit_cast(uint32_t, amax);
    const int e = (int)(u >> 23) - 126 - 9 + ((u & 0x7fffffu) > 0x600000u);
    return amax == 0.f ? 0 : e;
}
// 16 consecutive fp16 values of a head row (two 16-byte words) -> 16 e4m3 bytes under the row's exponent.  The scaling by 2^-e is exact
// (v_ldexp_f32 on values of magnitude <= 448), v_cvt_pk_fp8_f32 rounds to nearest even.
GPTQ_DEV u32x4 kv8_quant16(const half8_t lo, const half8_t hi, int e) {
    u32x4 q;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const half8_t &src = w < 2 ? lo : hi;
        const int j = (w & 1) * 4;
        int word = 0;
        word = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_ldexpf((float)src[j], -e), __builtin_ldexpf((float)src[j + 1], -e), word, false);
        word = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_ldexpf((float)src[j + 2], -e), __builtin_ldexpf((float)src[j + 3], -e), word, true);
        q[w] = (uint32_t)word;
    }
    return q;
}
GPTQ_DEV float kv8_amax16(const half8_t lo, const half8_t hi) {
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++) m = fmaxf(m, fmaxf(__builtin_fabsf((float)lo[j]), __builtin_fabsf((float)hi[j])));
    return m;
}
// a head row held by an aligned group of 8 lanes, 16 values each: exponent (the same in all 8 lanes) and this lane's 16 bytes
GPTQ_DEV u32x4 kv8_quant_row(const half8_t lo, const half8_t hi, int &e) {
    e = kv8_exponent(row_max8(kv8_amax16(lo, hi)));
    return kv8_quant16(lo, hi, e);
}
// 16 e4m3 bytes -> fp32 (exact)
GPTQ_DEV void kv8_dequant16(const u32x4 q, float (&f)[16]) {
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const float2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)q[w], false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)q[w], true);
        f[4 * w] = a[0];
        f[4 * w + 1] = a[1];
        f[4 * w + 2] = b[0];
        f[4 * w + 3] = b[1];
    }
}

// ---------------------------------------------------------------------------------------
// The streaming decode attention over the fp8 cache.  grid = (heads, rows of the decode batch, S splits), 256 threads; everything that is not
// about the cache format is attn_stream_kernel<4, false> of decode_attn.hip: the split rule and the workspace of attn_split.h, an idle row
// (pos < 0 or >= t_max) reads and writes nothing, K / V rows by buffer loads whose descriptor ends at the split's last old row (lanes past it
// read zeros without a memory request), the next tile requested before the current one is used, scores in the log2 domain, one split stores
// the row itself, several go through the system-scope records and the arrival ticket of attn_device.h.
// The split that owns position `pos` rotates the new k, quantises k and v from LDS (every group of 8 lanes for itself: no second barrier),
// attends to the QUANTISED row -- a step is a function of the cache alone -- and appends bytes and exponents at the end.
// ---------------------------------------------------------------------------------------
struct AttnKv8Args {
    const half_t *qkv;
    const int64_t *pos;
    uint8_t *k8, *v8;
    int8_t *kexp, *vexp;
    half_t *out;
    half_t *o16;                 // records: [batch][S][heads * 128] fp16 partial outputs
    float *md;                   //          [batch][S][heads] {M, den}
    unsigned *tickets;
    const float2 *rope_tab;
    const int32_t *out_perm;
    int heads, t_max, ldq, ldo, tps;
    float inv_base, scale2;      // scale2 = softmax scale x log2(e)
};

GPTQ_DEV u32x4 kv8_load16(__amdgpu_buffer_rsrc_t r, int voff) {
    return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0));
}
GPTQ_DEV int kv8_load_exp(__amdgpu_buffer_rsrc_t r, int voff) { return (int)(int8_t)__builtin_amdgcn_raw_buffer_load_b8(r, voff, 0, 0); }

constexpr int KV8_NW = 4;                    // waves of a split
constexpr int KV8_RP = KV8_NW * 8;           // timesteps per pass of the workgroup (8 lanes per timestep)
constexpr int KV8_NP = 8;                    // passes per tile = 16-byte K (and V) loads per lane and tile
constexpr int KV8_TILE = KV8_RP * KV8_NP;    // 256 timesteps: a multiple of ATT_TILE, the unit of a split's range

__global__ void __launch_bounds__(KV8_NW * 64) attn_stream_kv8_kernel(const AttnKv8Args a) {
    constexpr int NW = KV8_NW, RP = KV8_RP, NP = KV8_NP, TILE = KV8_TILE;
    __shared__ float qs[ATT_HD];
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
    const int d8 = tid & 7, tsub = tid >> 3;     // this lane: dims [16 d8, 16 d8 + 16) of timestep tsub of a pass

    // descriptors over rows [0, n_old) of this (row, head), bytes and exponents: anything past the split's last cache row reads as zero
    const size_t slice = ((size_t)b * a.t_max) * hd + (size_t)h * ATT_HD;
    const size_t eslice = ((size_t)b * a.t_max) * a.heads + h;
    const int nrec = n_old > 0 ? (n_old - 1) * hd + ATT_HD : 0;
    const int nrec_e = n_old > 0 ? (n_old - 1) * a.heads + 1 : 0;
    const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void *)(a.k8 + slice), 0, nrec, 0x00020000);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void *)(a.v8 + slice), 0, nrec, 0x00020000);
    const __amdgpu_buffer_rsrc_t rke = __builtin_amdgcn_make_buffer_rsrc((void *)(a.kexp + eslice), 0, nrec_e, 0x00020000);
    const __amdgpu_buffer_rsrc_t rve = __builtin_amdgcn_make_buffer_rsrc((void *)(a.vexp + eslice), 0, nrec_e, 0x00020000);
    u32x4 KA[NP], VA[NP], KB[NP], VB[NP];
    int EKA, EVA, EKB, EVB;      // lane d8 of a timestep's 8 lanes: the exponents of pass d8
    auto load_exp = [&](int &EK, int &EV, int tb) {
        const int eo = (tb + d8 * RP + tsub) * a.heads;
        EK = kv8_load_exp(rke, eo);
        EV = kv8_load_exp(rve, eo);
    };
    auto load = [&](u32x4 (&K)[NP], u32x4 (&V)[NP], int &EK, int &EV, int tb) {
        const int vo = (tb + tsub) * hd + d8 * 16;
        load_exp(EK, EV, tb);
#pragma unroll
        for (int it = 0; it < NP; it++) K[it] = kv8_load16(rk, vo + it * RP * hd);
#pragma unroll
        for (int it = 0; it < NP; it++) V[it] = kv8_load16(rv, vo + it * RP * hd);
    };
    // a context of up to two passes (64 timesteps: the first tokens of a sequence) requests and computes two passes, not eight
    const bool tiny = t_end - t0 <= 2 * RP;
    if (tiny) {
        const int vo = (t0 + tsub) * hd + d8 * 16;
        load_exp(EKA, EVA, t0);
        KA[0] = kv8_load16(rk, vo);
        KA[1] = kv8_load16(rk, vo + RP * hd);
        VA[0] = kv8_load16(rv, vo);
        VA[1] = kv8_load16(rv, vo + RP * hd);
    } else {
        load(KA, VA, EKA, EVA, t0);
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- RoPE of q (every split) and of the new k (owner) under the latency of the first tile ----
    if (tid < ATT_HD / 2) {
        const int c = tid;
        float cs, sn;
        rope_cos_sin(a.rope_tab, pos, c, ATT_HD / 2, a.inv_base, cs, sn);
        half_t rq0, rq1;
        rope_rotate(q0, q1, cs, sn, rq0, rq1);
        qs[c] = (float)rq0;
        qs[c + ATT_HD / 2] = (float)rq1;
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
    float qf[16];
#pragma unroll
    for (int j = 0; j < 16; j++) qf[j] = qs[d8 * 16 + j];
    // the new token's row in the cache format: bytes of this lane's 16 dims, the row's exponents (owner only; the fp16 rows are in LDS)
    u32x4 kn = u32x4{0u, 0u, 0u, 0u}, vn = u32x4{0u, 0u, 0u, 0u};
    int ekn = 0, evn = 0;
    if (owner) {
        kn = kv8_quant_row(*(const half8_t *)(knew + d8 * 16), *(const half8_t *)(knew + d8 * 16 + 8), ekn);
        vn = kv8_quant_row(*(const half8_t *)(vnew + d8 * 16), *(const half8_t *)(vnew + d8 * 16 + 8), evn);
    }

    // ---- the wave's running state: M (log2 domain), l and acc[16 dims of this lane] relative to M ----
    float M = ATT_M_FLOOR, l = 0.f, av[16];
#pragma unroll
    for (int j = 0; j < 16; j++) av[j] = 0.f;
    const int grp = (lane & ~7) << 2;            // ds_bpermute address of lane 0 of this lane's group
    auto pass_exp = [&](int E, int it) { return __builtin_amdgcn_ds_bpermute(grp + 4 * it, E); };
    auto score16 = [&](const u32x4 k, int ek) {  // scale2 (q . k 2^ek): the same value in the 8 lanes of the timestep
        float kf[16];
        kv8_dequant16(k, kf);
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < 16; j++) dot = __builtin_fmaf(qf[j], kf[j], dot);
        return __builtin_ldexpf(row_sum8(dot) * a.scale2, ek);
    };
    auto wave_max = [&](float v) { return rows_max(fmaxf(v, dpp_row_f32<0x140>(v))); };   // the wave's eight timesteps (row_mirror: the other half row)
    auto accumulate = [&](const u32x4 v, float p, int ev) {
        float vf[16];
        kv8_dequant16(v, vf);
        const float pe = __builtin_ldexpf(p, ev);
#pragma unroll
        for (int j = 0; j < 16; j++) av[j] = __builtin_fmaf(pe, vf[j], av[j]);
    };
    // a tile (PASSES = NP), or a tiny context (PASSES = 2).  FULL: all of its rows are cache rows of this split; otherwise rows past t_end are
    // masked, and the lanes that hold position `pos` take that row from the registers above (the new token is not in the cache yet).
    // Straight-line code: masks and selects, no branches.
    auto tile_any = [&](const u32x4 (&K)[NP], const u32x4 (&V)[NP], int EK, int EV, int tb, auto passes, auto full) {
        constexpr int PASSES = decltype(passes)::value;
        constexpr bool FULL = decltype(full)::value;
        float sc[PASSES];
        float mt = -INFINITY;
#pragma unroll
        for (int it = 0; it < PASSES; it++) {
            const int t = tb + it * RP + tsub;
            const bool isnew = !FULL && owner && t == pos;
            const int ek = pass_exp(EK, it);
            const float v = score16(isnew ? kn : K[it], isnew ? ekn : ek);
            sc[it] = (FULL || t < t_end) ? v : -INFINITY;
            mt = fmaxf(mt, sc[it]);
        }
        mt = wave_max(mt);
        const float Mn = fmaxf(M, mt), alpha = __builtin_amdgcn_exp2f(M - Mn);
        float p[PASSES], ps = 0.f;
#pragma unroll
        for (int it = 0; it < PASSES; it++) {
            p[it] = __builtin_amdgcn_exp2f(sc[it] - Mn);         // masked slots hold -inf: 0
            ps += p[it];
        }
        l = __builtin_fmaf(l, alpha, ps);
#pragma unroll
        for (int j = 0; j < 16; j++) av[j] *= alpha;
#pragma unroll
        for (int it = 0; it < PASSES; it++) {
            const bool isnew = !FULL && owner && tb + it * RP + tsub == pos;
            const int ev = pass_exp(EV, it);
            accumulate(isnew ? vn : V[it], p[it], isnew ? evn : ev);
        }
        M = Mn;
    };
    auto tile = [&](const u32x4 (&K)[NP], const u32x4 (&V)[NP], int EK, int EV, int tb) {
        if (tb + TILE <= n_old) tile_any(K, V, EK, EV, tb, std::integral_constant<int, NP>(), std::true_type());
        else tile_any(K, V, EK, EV, tb, std::integral_constant<int, NP>(), std::false_type());
    };
    if (tiny) {
        tile_any(KA, VA, EKA, EVA, t0, std::integral_constant<int, 2>(), std::false_type());
    } else if (ntiles == 1) {    // every context up to a tile: one register set, no loop
        tile(KA, VA, EKA, EVA, t0);
    } else {
        for (int i = 0; i < ntiles; i += 2) {
            load(KB, VB, EKB, EVB, t0 + (i + 1) * TILE);             // (past the split's rows: zeros, no traffic)
            __builtin_amdgcn_sched_barrier(0);
            tile(KA, VA, EKA, EVA, t0 + i * TILE);
            __builtin_amdgcn_sched_barrier(0);
            load(KA, VA, EKA, EVA, t0 + (i + 2) * TILE);
            __builtin_amdgcn_sched_barrier(0);
            if (i + 1 < ntiles) tile(KB, VB, EKB, EVB, t0 + (i + 1) * TILE);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (owner && tid < 8) {    // append the new token's row (nothing in this launch reads it back), after the last cache load has been consumed
        *(u32x4 *)(a.k8 + slice + (size_t)pos * hd + tid * 16) = kn;
        *(u32x4 *)(a.v8 + slice + (size_t)pos * hd + tid * 16) = vn;
        if (tid == 0) {
            a.kexp[eslice + (size_t)pos * a.heads] = (int8_t)ekn;
            a.vexp[eslice + (size_t)pos * a.heads] = (int8_t)evn;
        }
    }

    // ---- the wave's eight timesteps -> one, the NW waves -> one (LDS): {Mx, den, num[tid]} of the split ----
#pragma unroll
    for (int j = 0; j < 16; j++) av[j] = rows_sum(av[j] + dpp_row_f32<0x128>(av[j]));     // row_ror 8: the other half row, same dims
    l = rows_sum(l + dpp_row_f32<0x128>(l));
    if (lane < 8) {
#pragma unroll
        for (int j = 0; j < 16; j += 4) *(float4_t *)(&accs[wave][lane * 16 + j]) = float4_t{av[j], av[j + 1], av[j + 2], av[j + 3]};
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

int decode_attn_kv8_launch(const half_t *qkv, const int64_t *pos, uint8_t *k8, uint8_t *v8, int8_t *kexp, int8_t *vexp, half_t *out, float *ws,
                           int heads, int t_max, float base, float scale, const float *rope_table, hipStream_t s, int batch, int64_t ldq,
                           int64_t ldo, const int32_t *out_perm, int tps) {
    const DecodeAttnWs w = decode_attn_ws(batch, heads, t_max);
    AttnKv8Args a{};
    a.qkv = qkv; a.pos = pos; a.k8 = k8; a.v8 = v8; a.kexp = kexp; a.vexp = vexp; a.out = out;
    a.o16 = (half_t *)((char *)ws + w.o16);
    a.md = (float *)((char *)ws + w.md);
    a.tickets = (unsigned *)((char *)ws + w.tickets);
    a.rope_tab = (const float2 *)rope_table;
    a.out_perm = out_perm;
    a.heads = heads; a.t_max = t_max; a.ldq = (int)ldq; a.ldo = (int)ldo;
    a.tps = tps > 0 ? tps : decode_attn_tps(false);
    a.inv_base = rope_inv_base(base, ATT_HD);
    a.scale2 = scale * 1.44269504088896340736f;
    hipLaunchKernelGGL(attn_stream_kv8_kernel, dim3(heads, batch, w.S), dim3(KV8_NW * 64), 0, s, a);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// fp16 cache rows -> fp8 cache rows at the same coordinates, for a table of segments (the prompt paths: prompt attention runs on an fp16
// staging cache, this converts what it appended).  grid = (head rows of the longest segment / 32, segments, 2: K / V), 256 threads: a group
// of 8 lanes owns one head row -- two 16-byte loads, the quantiser above, one 16-byte store per lane and one exponent byte per group.
// ---------------------------------------------------------------------------------------
struct Kv8StoreArgs {
    gptq_prompt_seg_t seg[GPTQ_PROMPT_ATTN_MAX_SEQS];
    const half_t *src[2];
    uint8_t *dst[2];
    int8_t *exp[2];
    int64_t slot_stride;
    int heads, t_max;
};

__global__ void __launch_bounds__(256) kv8_store_kernel(const Kv8StoreArgs a) {
    const gptq_prompt_seg_t sg = a.seg[blockIdx.y];
    const int kv = blockIdx.z;
    const int d8 = threadIdx.x & 7;
    const int64_t unit = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);      // head row of the segment: (row, head)
    if (unit >= (int64_t)sg.rows * a.heads) return;                          // (the 8 lanes of a group leave together)
    const int r = (int)(unit / a.heads), h = (int)(unit - (int64_t)r * a.heads);
    const int64_t t = (int64_t)sg.start + r, hd = (int64_t)a.heads * ATT_HD;
    const half_t *src = a.src[kv] + sg.slot * a.slot_stride + t * hd + h * ATT_HD + d8 * 16;
    const half8_t lo = *(const half8_t *)src, hi = *(const half8_t *)(src + 8);
    int e;
    const u32x4 q = kv8_quant_row(lo, hi, e);
    const int64_t row = (int64_t)sg.slot * a.t_max + t;
    *(u32x4 *)(a.dst[kv] + row * hd + h * ATT_HD + d8 * 16) = q;
    if (d8 == 0) a.exp[kv][row * a.heads + h] = (int8_t)e;
}

int kv8_store_launch(const half_t *k16, const half_t *v16, int64_t slot_stride, const gptq_prompt_seg_t *segs, int nseq, uint8_t *k8, uint8_t *v8,
                     int8_t *kexp, int8_t *vexp, int heads, int t_max, hipStream_t s) {
    Kv8StoreArgs a{};
    int most = 0;
    for (int i = 0; i < nseq; i++) {
        a.seg[i] = segs[i];
        most = std::max(most, segs[i].rows);
    }
    a.src[0] = k16; a.src[1] = v16;
    a.dst[0] = k8; a.dst[1] = v8;
    a.exp[0] = kexp; a.exp[1] = vexp;
    a.slot_stride = slot_stride;
    a.heads = heads; a.t_max = t_max;
    const unsigned blocks = (unsigned)(((int64_t)most * heads + 31) / 32);
    hipLaunchKernelGGL(kv8_store_kernel, dim3(blocks, nseq, 2), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace gptq
