// stripe_unpack.inc -- constants and the word -> half2 unpack of the stripe16 layout for ONE bit width (STRIPE_BITS); shared by the
// decode kernel (stripe_kernel.inc) and the small-batch MFMA kernel (stripe_mm.inc).  Included inside namespace gptq { namespace {.
constexpr int SB = STRIPE_BITS;
// 2 / 4 / 8 bits: a lane's row-block share is a dwordx4 = four packed rows of KPW = 32 / bits k.  3 bits: 32 k = 96 bits = a dwordx3
// (no whole number of fields per word: ten fields per word + the two spare bits 15 / 31, which carry the bits of k 30 and k 31).
constexpr int WPL = SB == 3 ? 3 : 4;                 // words per lane and row block
constexpr int KPW = SB == 3 ? 10 : 32 / SB;          // k per packed word: 16 / 10 (+ spare bits) / 8 / 4
constexpr int NPAIR = KPW / 2;                       // half2 pairs per word
constexpr int LK = SB == 3 ? 32 : 4 * KPW;           // k per lane and row block: 64 / 32 / 32 / 16
constexpr int BK = 4 * LK;                           // k per row block (one wave load): 256 / 128 / 128 / 64
constexpr int PPB = LK / 8;                          // 16-byte pieces of x per lane block: 8 / 4 / 4 / 2
constexpr int NPB = LK / 2;                          // half2 pairs per lane block

template <int CTRL>
GPTQ_DEV float dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// sum over the four 16-lane rows of a wave (every lane ends with the total of its lane position): gfx950 permlane swaps
GPTQ_DEV float fold_rows(float v) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    const float s16 = __builtin_bit_cast(float, (uint32_t)a[0]) + __builtin_bit_cast(float, (uint32_t)a[1]);
    const uint32_t u2 = __builtin_bit_cast(uint32_t, s16);
    auto b = __builtin_amdgcn_permlane32_swap(u2, u2, false, false);
    return __builtin_bit_cast(float, (uint32_t)b[0]) + __builtin_bit_cast(float, (uint32_t)b[1]);
}
// sum over the PPB adjacent lanes that hold the pieces of one lane block (2, 4 or 8 lanes)
GPTQ_DEV float block_sum(float v) {
    v += dpp_f<0xB1>(v);                               // quad_perm [1,0,3,2]
    if constexpr (PPB >= 4) v += dpp_f<0x4E>(v);       // quad_perm [2,3,0,1]
    if constexpr (PPB >= 8) v += dpp_f<0x141>(v);      // row_half_mirror: the other quad of the 8
    return v;
}
GPTQ_DEV float wave_sum_all(float v) {
    v += dpp_f<0xB1>(v);
    v += dpp_f<0x4E>(v);
    v += dpp_f<0x141>(v);
    v += dpp_f<0x140>(v);  // row_mirror: the other half of the 16
    return fold_rows(v);
}

// The fp16 magic offsets of a lane block.  pair_off_block(p) is the offset the magic of pair p (natural k order, NPB pairs) carries -- the field
// value is OFF + q; the decode kernels' x staging calls it with a run-time pair.  The MFMA kernels (dequant_block, stripe_mm.inc) need the same
// fact as CLASSES: NOFFC distinct offsets, off_class(p) the class of pair p, class_off(c) its offset -- and class c IS the magic g[c] of
// unpack_consts() (MAGIC<c>).  The static_assert below ties the three together: every pair's offset is its class's, every magic decodes to its
// class's offset.
// Selects, NOT constant tables: indexed with a run-time pair number a table becomes a global load from .rodata, and its s_waitcnt vmcnt(0)
// -- in the staging phase, or (act-order) in every K-loop iteration -- also waits for every weight load in flight (found in round 4.  3-bit
// 4096 x 4096 at M = 1: 4.27 -> 3.86 us, 11008 x 4096: 6.76 -> 5.90 us; with act-order 10.0 -> 6.9 us)
__host__ __device__ constexpr float pair_off(int i) {   // ... of pair i of a packed WORD
    if (SB == 8) return 1024.f;
    if (SB == 4) return (i & 1) ? 64.f : 1024.f;
    if (SB == 3) {   // 1024 128 16 1024 128
        const int r = i % 5, c = r >= 3 ? r - 3 : r;
        return c == 0 ? 1024.f : (c == 1 ? 128.f : 16.f);
    }
    const int r = i & 7;   // 1024 256 64 16 4 64 16 4
    if (r < 2) return r == 0 ? 1024.f : 256.f;
    const int c = r >= 5 ? r - 5 : r - 2;
    return c == 0 ? 64.f : (c == 1 ? 16.f : 4.f);
}
__host__ __device__ constexpr float pair_off_block(int p) {
    if (SB == 3) return p == 15 ? 1024.f : pair_off(p % 5);   // (pair 15: k 30 / k 31 from the spare bits)
    return pair_off(p % NPAIR);
}
constexpr int NOFFC = SB == 8 ? 1 : (SB == 4 ? 2 : (SB == 3 ? 3 : 5));   // distinct offsets of a width
__host__ __device__ constexpr int off_class(int p) {
    if (SB == 8) return 0;
    if (SB == 4) return p & 1;
    if (SB == 3) return p == 15 ? 0 : (p % 5) % 3;    // offsets 1024, 128, 16, 1024, 128 per word; the spare-bit pair 1024
    const int r = p & 7;                               // 1024, 256, 64, 16, 4, 64, 16, 4 per word
    return r < 5 ? r : r - 3;
}
__host__ __device__ constexpr float class_off(int c) {
    if (SB == 8) return 1024.f;
    if (SB == 4) return c ? 64.f : 1024.f;
    if (SB == 3) return c == 0 ? 1024.f : (c == 1 ? 128.f : 16.f);
    return c == 0 ? 1024.f : (c == 1 ? 256.f : (c == 2 ? 64.f : (c == 3 ? 16.f : 4.f)));
}
// the magic of an offset: fp16 OFF (a power of two 2^e, 0 <= e <= 15: bits (e + 15) << 10, zero mantissa) in both halves; OR-ing a field into
// its mantissa gives OFF + q.  Anything that is no such power of two gives 0, which the static_assert below refuses.
__host__ __device__ constexpr uint32_t off_magic(float off) {
    for (int e = 0; e <= 15; e++)
        if ((float)(1 << e) == off) return (uint32_t)((e + 15) << 10) * 0x10001u;
    return 0u;
}
// ... and back: the fp16 value both halves of a magic carry (0 if they differ or the mantissa is not empty)
__host__ __device__ constexpr float magic_off(uint32_t m) {
    const uint32_t h = m & 0xFFFFu, e = h >> 10;
    return ((m >> 16) != h || (h & 0x3FFu) || e < 15 || e > 30) ? 0.f : (float)(1 << (e - 15));
}
constexpr bool magics_match() {      // every class's magic decodes back to the class's offset, and every pair's offset is its class's
    for (int c = 0; c < NOFFC; c++)
        if (magic_off(off_magic(class_off(c))) != class_off(c)) return false;
    for (int p = 0; p < NPB; p++)
        if (off_class(p) < 0 || off_class(p) >= NOFFC || class_off(off_class(p)) != pair_off_block(p)) return false;
    return true;
}
static_assert(magics_match(), "pair_off_block() <-> offset classes <-> magics of unpack_consts()");
template <int C> constexpr uint32_t MAGIC = off_magic(class_off(C < NOFFC ? C : 0));   // of class C.  1024: 0x6400, 256: 0x5C00, 128: 0x5800, 64: 0x5400, 16: 0x4C00, 4: 0x4400

struct UnpackConsts {
    uint32_t m[5], g[5];   // masks in SGPRs, magics in VGPRs: (w & m) | g is ONE v_and_or_b32; g[c] = MAGIC<c>, the magic of offset class c
};
GPTQ_DEV UnpackConsts unpack_consts() {
    UnpackConsts c{};
    if constexpr (SB == 8) {
        c.m[0] = sreg_const(0x00FF00FFu); c.g[0] = vreg_const(MAGIC<0>);
    } else if constexpr (SB == 4) {
        c.m[0] = sreg_const(0x000F000Fu); c.g[0] = vreg_const(MAGIC<0>);   // bits [3:0]  -> 1024 + q
        c.m[1] = sreg_const(0x00F000F0u); c.g[1] = vreg_const(MAGIC<1>);   // bits [7:4]  ->   64 + q
    } else if constexpr (SB == 3) {
        c.m[0] = sreg_const(0x00070007u); c.g[0] = vreg_const(MAGIC<0>);   // bits [2:0]  -> 1024 + q
        c.m[1] = sreg_const(0x00380038u); c.g[1] = vreg_const(MAGIC<1>);   // bits [5:3]  ->  128 + q
        c.m[2] = sreg_const(0x01C001C0u); c.g[2] = vreg_const(MAGIC<2>);   // bits [8:6]  ->   16 + q
        c.m[3] = sreg_const(0x00010001u);                                     // the spare bits, shifted down to [0], [1], [2]
        c.m[4] = sreg_const(0x00020002u);
        c.g[4] = sreg_const(0x00040004u);                                     // (third spare mask parked in g[4]: an SGPR like the others)
    } else {
        c.m[0] = sreg_const(0x00030003u); c.g[0] = vreg_const(MAGIC<0>);   // [1:0] -> 1024 + q
        c.m[1] = sreg_const(0x000C000Cu); c.g[1] = vreg_const(MAGIC<1>);   // [3:2] ->  256 + q
        c.m[2] = sreg_const(0x00300030u); c.g[2] = vreg_const(MAGIC<2>);   // [5:4] ->   64 + q
        c.m[3] = sreg_const(0x00C000C0u); c.g[3] = vreg_const(MAGIC<3>);   // [7:6] ->   16 + q
        c.m[4] = sreg_const(0x03000300u); c.g[4] = vreg_const(MAGIC<4>);   // [9:8] ->    4 + q
    }
    return c;
}
// word -> NPAIR half2 {OFF + q_2i, OFF + q_2i+1} in natural k order
GPTQ_DEV void unpack_word(uint32_t w, const UnpackConsts &c, uint32_t (&t)[NPAIR]) {
    if constexpr (SB == 3) {
        const uint32_t hi = w >> 9;   // fields 3, 4 (bits [14:9]) land on [5:0]
        t[0] = (w & c.m[0]) | c.g[0]; t[1] = (w & c.m[1]) | c.g[1]; t[2] = (w & c.m[2]) | c.g[2];
        t[3] = (hi & c.m[0]) | c.g[0]; t[4] = (hi & c.m[1]) | c.g[1];
    } else if constexpr (SB == 8) {
        t[0] = (w & c.m[0]) | c.g[0];
        t[1] = ((w >> 8) & c.m[0]) | c.g[0];
    } else if constexpr (SB == 4) {
        const uint32_t hi = w >> 8;
        t[0] = (w & c.m[0]) | c.g[0]; t[1] = (w & c.m[1]) | c.g[1];
        t[2] = (hi & c.m[0]) | c.g[0]; t[3] = (hi & c.m[1]) | c.g[1];
    } else {
        const uint32_t hi = w >> 6;   // fields 5..7 (bits [15:10]) land on [9:4]
#pragma unroll
        for (int i = 0; i < 5; i++) t[i] = (w & c.m[i]) | c.g[i];
#pragma unroll
        for (int i = 0; i < 3; i++) t[5 + i] = (hi & c.m[2 + i]) | c.g[2 + i];
    }
}

// a lane's row-block share (WPL words) -> NPB half2 pairs in natural k order
template <typename WV>
GPTQ_DEV void unpack_block(const WV &w, const UnpackConsts &c, uint32_t (&t)[NPB]) {
#pragma unroll
    for (int j = 0; j < WPL; j++) {
        uint32_t tw[NPAIR];
        unpack_word(w[j], c, tw);
#pragma unroll
        for (int q = 0; q < NPAIR; q++) t[j * NPAIR + q] = tw[q];
    }
    if constexpr (SB == 3)   // k 30 / k 31: bit j of each from the spare bits 15 / 31 of word j
        t[15] = ((w[0] >> 15) & c.m[3]) | (((w[1] >> 14) & c.m[4]) | (((w[2] >> 13) & c.g[4]) | c.g[0]));
}
