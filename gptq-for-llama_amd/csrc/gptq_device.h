// gptq_device.h -- shared device helpers for the gfx950 kernels (wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef _Float16 half_t;
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef float float4_t __attribute__((ext_vector_type(4)));
typedef float float2_t __attribute__((ext_vector_type(2)));
typedef float float16_t __attribute__((ext_vector_type(16)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define GPTQ_DEV static __device__ __forceinline__

GPTQ_DEV half2_t as_half2(uint32_t u) { return __builtin_bit_cast(half2_t, u); }
GPTQ_DEV uint32_t as_u32(half2_t h) { return __builtin_bit_cast(uint32_t, h); }

// Number of XCDs on MI355X; block b is observed to run on XCD b % 8 (speed only, never
// correctness).  Bijective remap that hands every XCD a contiguous range of logical ids so
// neighbouring tiles (which share 128-B lines / x) hit the same L2.
GPTQ_DEV int xcd_remap(int bid, int nwg) {
    constexpr int NXCD = 8;
    if (nwg < 2 * NXCD) return bid;
    int xcd = bid % NXCD, idx = bid / NXCD;
    int q = nwg / NXCD, r = nwg % NXCD;
    int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

// ---------------------------------------------------------------------------------------
// Field extraction.  A packed word holds KPW = 32/BITS consecutive k of ONE column.
// Unpack<BITS>::pairs() turns a word into NP = KPW/2 half2 values t[p] = {OFF + q_p,
// OFF + q_{p+NP}} using the fp16 "magic exponent" trick: OR-ing the field into the mantissa
// of a constant whose ulp equals the field's bit weight, so no int->float convert is needed.
// The constant offset OFF is removed exactly (fp16 subtract) or folded into the zero point.
// ---------------------------------------------------------------------------------------
template <int BITS>
struct Unpack;

template <>
struct Unpack<4> {
    static constexpr int KPW = 8, NP = 4;
    static constexpr float OFF = 64.0f;  // 0x5400 = 64.0, ulp 1/16: field at bits [7:4] -> +q
    GPTQ_DEV void pairs(uint32_t w, half2_t (&t)[NP]) {
        constexpr uint32_t MSK = 0x00F000F0u, MAG = 0x54005400u;
        t[0] = as_half2(((w << 4) & MSK) | MAG);  // fields 0,4
        t[1] = as_half2((w & MSK) | MAG);          // fields 1,5
        t[2] = as_half2(((w >> 4) & MSK) | MAG);  // fields 2,6
        t[3] = as_half2(((w >> 8) & MSK) | MAG);  // fields 3,7
    }
    // same with the mask in an SGPR and the magic in a VGPR: 3 shifts + 4 v_and_or_b32
    static constexpr uint32_t MSK_C = 0x00F000F0u, MAG_C = 0x54005400u;
    GPTQ_DEV void pairs_rc(uint32_t w, half2_t (&t)[NP], uint32_t msk, uint32_t mag) {
        t[0] = as_half2(((w << 4) & msk) | mag);
        t[1] = as_half2((w & msk) | mag);
        t[2] = as_half2(((w >> 4) & msk) | mag);
        t[3] = as_half2(((w >> 8) & msk) | mag);
    }
};

template <>
struct Unpack<2> {
    static constexpr int KPW = 16, NP = 8;
    static constexpr float OFF = 64.0f;  // field at bits [5:4] of 0x5400 -> +q
    GPTQ_DEV void pairs(uint32_t w, half2_t (&t)[NP]) {
        constexpr uint32_t MSK = 0x00300030u, MAG = 0x54005400u;
        t[0] = as_half2(((w << 4) & MSK) | MAG);   // fields 0,8
        t[1] = as_half2(((w << 2) & MSK) | MAG);   // 1,9
        t[2] = as_half2((w & MSK) | MAG);           // 2,10
        t[3] = as_half2(((w >> 2) & MSK) | MAG);   // 3,11
        t[4] = as_half2(((w >> 4) & MSK) | MAG);   // 4,12
        t[5] = as_half2(((w >> 6) & MSK) | MAG);   // 5,13
        t[6] = as_half2(((w >> 8) & MSK) | MAG);   // 6,14
        t[7] = as_half2(((w >> 10) & MSK) | MAG);  // 7,15
    }
    static constexpr uint32_t MSK_C = 0x00300030u, MAG_C = 0x54005400u;
    GPTQ_DEV void pairs_rc(uint32_t w, half2_t (&t)[NP], uint32_t msk, uint32_t mag) {
        t[0] = as_half2(((w << 4) & msk) | mag);
        t[1] = as_half2(((w << 2) & msk) | mag);
        t[2] = as_half2((w & msk) | mag);
        t[3] = as_half2(((w >> 2) & msk) | mag);
        t[4] = as_half2(((w >> 4) & msk) | mag);
        t[5] = as_half2(((w >> 6) & msk) | mag);
        t[6] = as_half2(((w >> 8) & msk) | mag);
        t[7] = as_half2(((w >> 10) & msk) | mag);
    }
};

template <>
struct Unpack<8> {
    static constexpr int KPW = 4, NP = 2;
    static constexpr float OFF = 256.0f;  // 0x5C00 = 256.0, ulp 1/4: byte at bits [9:2] -> +q
    GPTQ_DEV void pairs(uint32_t w, half2_t (&t)[NP]) {
        constexpr uint32_t MSK = 0x03FC03FCu, MAG = 0x5C005C00u;
        t[0] = as_half2(((w << 2) & MSK) | MAG);  // bytes 0,2
        t[1] = as_half2(((w >> 6) & MSK) | MAG);  // bytes 1,3
    }
    static constexpr uint32_t MSK_C = 0x03FC03FCu, MAG_C = 0x5C005C00u;
    GPTQ_DEV void pairs_rc(uint32_t w, half2_t (&t)[NP], uint32_t msk, uint32_t mag) {
        t[0] = as_half2(((w << 2) & msk) | mag);
        t[1] = as_half2(((w >> 6) & msk) | mag);
    }
};

// Staged-x order for one word-row of KPW values: position 2p <- field p, 2p+1 <- field p+NP.
template <int BITS>
GPTQ_DEV int staged_pos(int field) {
    constexpr int NP = Unpack<BITS>::NP;
    return (field < NP) ? 2 * field : 2 * (field - NP) + 1;
}

// Generic integer field j (0..31) of a 32-k block for one column; rows w[0..CH) are the
// BITS consecutive qweight rows of that block.  Used by the fallback kernels and by 3-bit.
template <int BITS>
GPTQ_DEV int field_of_block(const uint32_t *w, int j) {
    if constexpr (BITS == 3) {
        int bit = 3 * j, wi = bit >> 5, o = bit & 31;
        uint64_t lo = w[wi];
        uint64_t hi = (wi < 2) ? w[wi + 1] : 0;
        return (int)(((lo | (hi << 32)) >> o) & 7u);
    } else {
        constexpr int KPW = 32 / BITS;
        return (int)((w[j / KPW] >> (BITS * (j % KPW))) & ((1u << BITS) - 1u));
    }
}

// zero point (stored + 1, not re-masked) of column n from a qzeros row pointer.
template <int BITS>
GPTQ_DEV int zero_of(const int32_t *zrow, int n) {
    if constexpr (BITS == 3) {
        const uint32_t *p = (const uint32_t *)zrow + 3 * (n >> 5);
        int bit = 3 * (n & 31), wi = bit >> 5, o = bit & 31;
        uint64_t lo = p[wi];
        uint64_t hi = (wi < 2) ? p[wi + 1] : 0;
        return (int)(((lo | (hi << 32)) >> o) & 7u) + 1;
    } else {
        constexpr int KPW = 32 / BITS;
        uint32_t w = (uint32_t)zrow[n / KPW];
        return (int)((w >> (BITS * (n % KPW))) & ((1u << BITS) - 1u)) + 1;
    }
}

// Cross-lane reductions on the VALU.  __shfl_xor lowers to ds_bpermute_b32 (an LDS round trip, ~120 cycles per dependent step: the
// per-wave stamps of tools/timeline_attn.py showed 3500 cycles in the 32 dependent shuffles of the decode attention's score loop, 6500 of
// the launch's 10 000); the xor offsets inside a 16-lane row run as DPP row operations and 16 / 32 as gfx950 permlane swaps instead -- the
// SAME operand pairs in the same order as the xor butterfly, so the results are bit-identical to it.  Do not reorder the steps.
template <int CTRL>
GPTQ_DEV float dpp_row_f32(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
GPTQ_DEV float row_sum16(float v) {   // every lane of a 16-lane row ends with the row's sum (xor 1, 2, 4, 8)
    v += dpp_row_f32<0xB1>(v);    // quad_perm [1,0,3,2]
    v += dpp_row_f32<0x4E>(v);    // quad_perm [2,3,0,1]
    v += dpp_row_f32<0x141>(v);   // row_half_mirror
    v += dpp_row_f32<0x140>(v);   // row_mirror
    return v;
}
GPTQ_DEV float row_max16(float v) {
    v = fmaxf(v, dpp_row_f32<0xB1>(v));
    v = fmaxf(v, dpp_row_f32<0x4E>(v));
    v = fmaxf(v, dpp_row_f32<0x141>(v));
    v = fmaxf(v, dpp_row_f32<0x140>(v));
    return v;
}
GPTQ_DEV float halves_sum(float v) {   // over the wave's two 32-lane halves (xor 32)
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    auto a = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __builtin_bit_cast(float, (uint32_t)a[0]) + __builtin_bit_cast(float, (uint32_t)a[1]);
}
GPTQ_DEV float halves_max(float v) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    auto a = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return fmaxf(__builtin_bit_cast(float, (uint32_t)a[0]), __builtin_bit_cast(float, (uint32_t)a[1]));
}
GPTQ_DEV float rows_sum(float v) {   // over the wave's four 16-lane rows (xor 16, then 32): every lane ends with the total of its lane position
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    return halves_sum(__builtin_bit_cast(float, (uint32_t)a[0]) + __builtin_bit_cast(float, (uint32_t)a[1]));
}
GPTQ_DEV float rows_max(float v) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    return halves_max(fmaxf(__builtin_bit_cast(float, (uint32_t)a[0]), __builtin_bit_cast(float, (uint32_t)a[1])));
}
// sum over the xor butterfly offsets from, 2 from, ... 32.  (from = 2, 4, 8 keep the shuffle for the in-row steps: the mirror patterns
// only equal the xor pairs when the finer steps ran first.)
GPTQ_DEV float wave_sum_xor(float v, int from) {
    if (from == 1) {
        v = row_sum16(v);
    } else {
#pragma unroll
        for (int off = from; off < 16; off <<= 1) v += __shfl_xor(v, off, 64);
    }
    if (from <= 16) return rows_sum(v);
    return from <= 32 ? halves_sum(v) : v;
}

typedef unsigned long long u64_t;
constexpr int SPLITK_MAX_SINGLE = 64;
constexpr int SPLITK_MAX_PAIR = 64;

// Opaque register-resident constants: (a & mask) | magic is ONE v_and_or_b32 only when the mask
// sits in an SGPR and the magic in a VGPR (VOP3 on gfx9 takes no literals); with literal operands
// hipcc emits v_and_b32 + v_or_b32.
GPTQ_DEV uint32_t vreg_const(uint32_t c) {
    uint32_t v;
    asm("v_mov_b32 %0, %1" : "=v"(v) : "s"(c));
    return v;
}
GPTQ_DEV uint32_t sreg_const(uint32_t c) {
    uint32_t v;
    asm("s_mov_b32 %0, %1" : "=s"(v) : "i"(c));
    return v;
}

// 16-byte system-scope (sc0 sc1: write-through / cache-bypassing) accesses for hand-offs between
// workgroups (MI355X_MICROARCH.md "Valid forms").  The loads are issued without a wait; call
// wait_sys_loads() on the whole batch before using any of them.
// The s_nop is REQUIRED: a global store of more than 8 bytes reads its data VGPRs one wait state after
// issue ("12-dword store" hazard).  The compiler's hazard recogniser does not look inside inline asm, so
// without it the next VALU write to v's first register was stored instead of v (found by the fused-MLP
// fuzz test: zeros at every 4th column of the partial tiles).
GPTQ_DEV void store_sys16(float *p, float4_t v) {
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
// Eight independent 16-byte system-scope loads and their wait as ONE asm statement: the compiler
// cannot see that the destination registers are not valid until the s_waitcnt, so issue and wait
// must not be separable (a register move scheduled in between would copy stale data).  Early-clobber outputs: the data
// lands asynchronously, so no destination may share registers with any of the address operands.
GPTQ_DEV void load_sys16_x8(float4_t (&v)[8], const float *const (&p)[8]) {
    asm volatile(
        "global_load_dwordx4 %0, %8, off sc0 sc1\n\t"
        "global_load_dwordx4 %1, %9, off sc0 sc1\n\t"
        "global_load_dwordx4 %2, %10, off sc0 sc1\n\t"
        "global_load_dwordx4 %3, %11, off sc0 sc1\n\t"
        "global_load_dwordx4 %4, %12, off sc0 sc1\n\t"
        "global_load_dwordx4 %5, %13, off sc0 sc1\n\t"
        "global_load_dwordx4 %6, %14, off sc0 sc1\n\t"
        "global_load_dwordx4 %7, %15, off sc0 sc1\n\t"
        "s_waitcnt vmcnt(0)"
        : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7])
        : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]), "v"(p[5]), "v"(p[6]), "v"(p[7])
        : "memory");
}

// Development-only s_memtime / s_memrealtime checkpoints (tools/timeline.py).
GPTQ_DEV u64_t stamp_cycles(uint32_t dep) {
    u64_t t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : "v"(dep) : "memory");
    return t;
}
GPTQ_DEV u64_t stamp_realtime() {
    u64_t t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
    return t;
}
