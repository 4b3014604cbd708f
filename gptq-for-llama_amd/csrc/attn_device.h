// attn_device.h -- the device-side pieces the attention entries share (decode_attn.hip, chunk_attn.hip, prompt_attn.hip; the RoPE also
// elementwise.hip), each written ONCE: the engine promises that a K/V cache row has the same bits whichever entry appended it, and that
// promise rests on every entry running the same instructions -- so they come from one place.
//   1. RoPE: rope_inv_base / rope_cos_sin / rope_rotate / rope_kv_row.  The accurate libm exp / cos / sin and two roundings per product: a
//      translation unit that includes this header for the RoPE is built with CXXFLAGS_STRICT (see the Makefile).
//   2. the LDS image of a K or V tile: 256-byte rows with a chunk swizzle, row reads and transposed reads.
//   3. the hand-off between the splits of one (row, head): arrival ticket + the last arriver's merge of the records.
// The wave reductions (row_sum16, rows_sum, halves_sum, ...) live in gptq_device.h; the split rule, the merge arithmetic and the
// workspace layouts in attn_split.h.
#pragma once
#include <math.h>

#include "attn_split.h"
#include "gptq_device.h"

namespace gptq {

// ---------------------------------------------------------------------------------------
// RoPE (rotate-half, fp32 trig like the reference's libdevice calls, quant/fused_attn.py:43-57)
// ---------------------------------------------------------------------------------------
// the exponent's factor: base^(-2c / head_dim) = exp(c * inv_base) (reference fused_attn.py:91)
inline float rope_inv_base(float base, int head_dim) { return -2.0f * logf(base) / (float)head_dim; }

// cs, sn = {cos, sin} of pos * base^(-2c / head_dim), c < half: from the table rope_table_kernel filled with the instructions below, or computed
// here.  (Reference outputs, not a returned pair: a returned struct changed the schedule of the unrolled trig in rope_kernel.)
template <typename P>
GPTQ_DEV void rope_cos_sin(const float2 *tab, P pos, int c, int half, float inv_base, float &cs, float &sn) {
    if (tab) {
        const float2 e = tab[(size_t)pos * half + c];
        cs = e.x;
        sn = e.y;
    } else {
        const float freq = expf((float)c * inv_base) * (float)pos;
        cs = cosf(freq);
        sn = sinf(freq);
    }
}

// (x, y) = columns c and c + half of a head -> (x cos - y sin, x sin + y cos), each rounded to fp16 once like the in-place reference RoPE
GPTQ_DEV void rope_rotate(half_t x, half_t y, float cs, float sn, half_t &ox, half_t &oy) {
    const float xf = (float)x, yf = (float)y;
    ox = (half_t)(xf * cs - yf * sn);
    oy = (half_t)(xf * sn + yf * cs);
}
GPTQ_DEV void rope_rotate(const half_t *src, half_t *dst, int half, float cs, float sn) {   // src == dst: in place
    half_t ox, oy;
    rope_rotate(src[0], src[half], cs, sn, ox, oy);
    dst[0] = ox;
    dst[half] = oy;
}

// one thread's share of a token's head: q rotated into qdst, k rotated into the cache row, v copied.  All pointers at column c of the head.
GPTQ_DEV void rope_kv_row(const half_t *q, const half_t *k, const half_t *v, half_t *qdst, half_t *kdst, half_t *vdst, int half, float cs, float sn) {
    rope_rotate(q, qdst, half, cs, sn);
    rope_rotate(k, kdst, half, cs, sn);
    vdst[0] = v[0];
    vdst[half] = v[half];
}

// ---------------------------------------------------------------------------------------
// LDS image of a tile: [rows][128 fp16], 16 chunks of 16 bytes per row, chunk ch of row `row` at ch ^ (((row & 3) << 2) | ((row >> 2) & 3)):
// conflict-free for the ds_read_b128 row reads of K and for the ds_read_b64_tr_b16 transposed reads of V
// ---------------------------------------------------------------------------------------
#define ATTN_LDS __attribute__((address_space(3)))
typedef short attn_short4 __attribute__((__vector_size__(4 * sizeof(short))));

GPTQ_DEV int attn_lds_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }   // byte offset

GPTQ_DEV half8_t attn_row_read(const half_t *img, int off) { return *(const ATTN_LDS half8_t *)((const ATTN_LDS char *)img + off); }
// ds_read_b64_tr_b16: per 16-lane group a block of 4 rows x 16 columns, lane i receives column i (row q in element q).  Every lane supplies an
// address (EXEC must be full: only ever called under wave-uniform control flow).
GPTQ_DEV half4_t attn_tr_read(const half_t *img, int off) {
    return __builtin_bit_cast(half4_t, __builtin_amdgcn_ds_read_tr16_b64_v4i16((ATTN_LDS attn_short4 *)((ATTN_LDS char *)img + off)));
}

// ---------------------------------------------------------------------------------------
// The hand-off between the nsp active splits of one (row, head) when no later launch merges their records.  Every split publishes its record
// -- {M, den} and o = num / den in fp16 -- with SYSTEM-scope stores, then calls attn_ticket_last; the one workgroup it returns true to calls
// attn_merge_records.  The ticket decides who merges, never what is computed: same records, same bits.
// ---------------------------------------------------------------------------------------
// Called by every thread of the workgroup, behind its record stores: waits for them, takes an arrival ticket (agent scope; the last arriver
// leaves it at 0 for the next launch) and tells every thread whether this workgroup arrived last.  last_flag: an int in LDS.
GPTQ_DEV bool attn_ticket_last(unsigned *ticket, int nsp, int *last_flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = (t == (unsigned)(nsp - 1));
        if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *last_flag = last;
    }
    __syncthreads();
    return *last_flag != 0;
}

// The last arriver's merge of W adjacent fp16 outputs per thread into res (W = 1: the decode attention, 8: the chunk attention).  rmd: {M, den} of split 0, mstride floats between splits; ro: this thread's outputs in the record of split 0 as words of type T
// (uint16_t: one fp16, uint32_t: a pair), ostride words between splits.  The records of all ATT_MAX_SPLITS slots are requested together (one
// memory latency; slots past nsp re-read the last live record and get coefficient 0) and merged in split order.
template <int W, typename T>
GPTQ_DEV void attn_merge_records(const float *rmd, size_t mstride, const T *ro, size_t ostride, int nsp, half_t (&res)[W]) {
    constexpr int NT = W * sizeof(half_t) / sizeof(T);
    typedef T words_t __attribute__((ext_vector_type(NT)));
    typedef half_t halves_t __attribute__((ext_vector_type(W)));
    float mi[ATT_MAX_SPLITS], di[ATT_MAX_SPLITS];
    words_t oi[ATT_MAX_SPLITS];
#pragma unroll
    for (int i = 0; i < ATT_MAX_SPLITS; i++) {
        const int ii = min(i, nsp - 1);
        mi[i] = __hip_atomic_load(rmd + (size_t)ii * mstride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        di[i] = __hip_atomic_load(rmd + (size_t)ii * mstride + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#pragma unroll
        for (int j = 0; j < NT; j++) oi[i][j] = __hip_atomic_load(ro + (size_t)ii * ostride + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    float c[ATT_MAX_SPLITS];
    attn_merge_coeffs(mi, di, nsp, c);
#pragma unroll
    for (int j = 0; j < W; j++) {
        half_t oj[ATT_MAX_SPLITS];
#pragma unroll
        for (int i = 0; i < ATT_MAX_SPLITS; i++) oj[i] = __builtin_bit_cast(halves_t, oi[i])[j];
        res[j] = attn_round_f16(attn_merge_value(oj, c));
    }
}

}  // namespace gptq
