// constrain.hip -- gptq_constrain_rows_f16: constrained decoding for regular languages.  A deterministic automaton over TOKENS lives in device memory
// as next[state][class] (int16, -1: not allowed) with one class per token (cls[v], int16: tokens whose columns agree in every state share a class);
// each sequence's state is one device word.  ONE launch per step, grid (B), one workgroup per sequence b: it advances state[b] by the token the step
// consumed and sets the logits of every token the NEW state does not allow to fp16 -inf, in place, ahead of the draw (include/gptq_mi355x.h
// "constrained decoding" states the semantics; tests/constrain_ref.py restates them in numpy).
//
// One workgroup per sequence, on purpose: that workgroup reads AND writes state[b].  A second workgroup on the same row would have to read the
// word its sibling stores in the same launch.  Inside the workgroup every wave reads state[b] for itself -- the advance is a handful of
// wave-uniform loads -- and thread 0 stores the new state behind a barrier, when no wave can still be about to read the old one.
//
// The kernel is bound by LATENCY, not by bytes: one row is 64 KB of logits and 64 KB of classes, and inside a decode step both come from HBM
// (3.4 GB of weights have gone through the caches since the last step).  So the dependent loads are few and everything else is in flight at
// once: level 1 -- len, state, map_of, last, all independent; level 2 -- the consumed token's class, and, without waiting for it, 16-byte
// loads of the row's classes and logits into registers, 8 tokens per load, CS_U loads of each per lane: 1024 lanes hold 32 768 tokens, a
// Llama vocabulary in one round; level 3 -- the transition; level 4 -- the new state's row next[s'][0 .. C) into LDS (2 C bytes, at most
// 32 KiB).  Then the registers are masked by LDS gathers and a group of 8 is stored back only where one of its logits changed: each element
// has one writer, and an allowed element keeps its bits whatever they are (NaN, +-inf, -0.0).  A vocabulary above 32 768 takes further
// rounds of loads behind the staged row.  1024 lanes instead of the siblings' 256 on a measurement: profiles/constrain/README.md.
// Rows whose base is not 16-byte aligned take a scalar head up to the first aligned element; where the class map's row is not aligned alike,
// the whole row goes scalar.  No arithmetic, no atomics, no workspace: the result depends on the inputs only (the fast-math flags of the
// default rule change nothing here).
#include "../../include/gptq_mi355x.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gptq_internal.h"

namespace {

using gptq::aligned;

constexpr int CS_NT = 1024;
constexpr int CS_U = 4;                     // 16-byte groups of classes and of logits a lane holds in flight
constexpr uint32_t CS_NEG_INF = 0xFC00u;

__device__ inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// the entry of the staged row for class c, or "banned" for a class outside the table
__device__ inline bool banned(const uint16_t *row, uint32_t c, int n_states, int n_classes) {
    if ((int)c >= n_classes) return true;                   // (a negative int16 is >= 32768 as uint16: out of range as well)
    return (int)row[c] >= n_states;                         // ... and so is a negative entry
}

// 8 logits under their 8 classes; true when a logit changed
__device__ inline bool mask8(const uint16_t *row, const uint4 &cw, uint4 &lw, int n_states, int n_classes) {
    const uint32_t cv[4] = {cw.x, cw.y, cw.z, cw.w};
    uint32_t lv[4] = {lw.x, lw.y, lw.z, lw.w};
    bool any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (banned(row, cv[j] & 0xFFFFu, n_states, n_classes) && (lv[j] & 0xFFFFu) != CS_NEG_INF) {
            lv[j] = (lv[j] & 0xFFFF0000u) | CS_NEG_INF;
            any = true;
        }
        if (banned(row, cv[j] >> 16, n_states, n_classes) && (lv[j] >> 16) != CS_NEG_INF) {
            lv[j] = (lv[j] & 0x0000FFFFu) | (CS_NEG_INF << 16);
            any = true;
        }
    }
    lw = make_uint4(lv[0], lv[1], lv[2], lv[3]);
    return any;
}

__global__ __launch_bounds__(CS_NT) void constrain_rows_kernel(uint16_t *logits, int64_t ld, int vocab, const int16_t *next, int64_t ld_next,
                                                               int n_states, int n_classes, const int16_t *cls, int64_t ld_cls, int n_maps,
                                                               const int32_t *map_of, int32_t *state, const int64_t *last, const int64_t *len,
                                                               int64_t len_add, int64_t t_limit) {
    extern __shared__ __attribute__((aligned(16))) uint16_t row[];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;

    // ---- level 1: four independent, wave-uniform loads (all in bounds for every row of the launch) ----
    const int64_t nb = len[b] + len_add;
    const int32_t s = state[b];
    const int32_t m = map_of[b];
    const int64_t t = last ? last[b] : 0;
    if (nb < 0 || nb > t_limit) return;                     // 1 idle (the whole workgroup: nothing is written, no logit is read)
    if (s < 0) return;                                      // 2 switched off (-1), left (-2): the row's bits are untouched
    const bool in_tables = s < n_states && m >= 0 && m < n_maps;

    // ---- level 2: the row's classes and logits on their way into registers ----
    uint16_t *l = logits + (int64_t)b * ld;
    const uint16_t *c = (const uint16_t *)cls + (int64_t)(in_tables ? m : 0) * ld_cls;
    int head = (int)(((16 - ((uintptr_t)l & 15)) & 15) >> 1);            // elements up to the first 16-byte aligned logit
    if (head > vocab || !aligned16(c + head)) head = vocab;              // no aligned body: the whole row by the scalar loop
    const int n8 = in_tables ? (vocab - head) >> 3 : 0;
    const uint4 *c4 = (const uint4 *)(c + head);
    uint4 *l4 = (uint4 *)(l + head);
    uint4 cw[CS_U], lw[CS_U];
#pragma unroll
    for (int u = 0; u < CS_U; ++u) {
        const int i = tid + u * CS_NT;
        if (i < n8) {
            cw[u] = c4[i];
            lw[u] = l4[i];
        }
    }

    // ---- levels 2, 3: the advance (3, 4 of the header), by every wave for itself ----
    int32_t s2 = s;
    if (!in_tables) {
        s2 = -2;                                            // a state or a map that is not in the tables: the row has left its automaton
    } else if (last) {
        s2 = -2;
        if (t >= 0 && t < vocab) {
            const int k = cls[(int64_t)m * ld_cls + t];
            if (k >= 0 && k < n_classes) {
                const int e = next[(int64_t)s * ld_next + k];
                if (e >= 0 && e < n_states) s2 = e;
            }
        }
    }
    __syncthreads();                                        // every wave has read state[b]
    if (tid == 0 && (last || s2 != s)) state[b] = s2;       // 5, 6
    if (s2 < 0) return;

    // ---- level 4: the new state's row into LDS ----
    const int16_t *src = next + (int64_t)s2 * ld_next;
    const int c8 = aligned16(src) ? n_classes >> 3 : 0;
    for (int i = tid; i < c8; i += CS_NT) ((uint4 *)row)[i] = ((const uint4 *)src)[i];
    for (int i = (c8 << 3) + tid; i < n_classes; i += CS_NT) row[i] = (uint16_t)src[i];
    __syncthreads();

    // ---- 7: the mask -- the round in registers, further rounds of a larger vocabulary, the scalar head and tail ----
#pragma unroll
    for (int u = 0; u < CS_U; ++u) {
        const int i = tid + u * CS_NT;
        if (i < n8 && mask8(row, cw[u], lw[u], n_states, n_classes)) l4[i] = lw[u];
    }
    for (int i = tid + CS_U * CS_NT; i < n8; i += CS_NT) {
        const uint4 cv = c4[i];
        uint4 lv = l4[i];
        if (mask8(row, cv, lv, n_states, n_classes)) l4[i] = lv;
    }
    for (int64_t v = tid; v < head; v += CS_NT)
        if (banned(row, c[v], n_states, n_classes)) l[v] = (uint16_t)CS_NEG_INF;
    for (int64_t v = (int64_t)head + ((int64_t)n8 << 3) + tid; v < vocab; v += CS_NT)
        if (banned(row, c[v], n_states, n_classes)) l[v] = (uint16_t)CS_NEG_INF;
}

}  // namespace

extern "C" int gptq_constrain_rows_f16(void *logits, int64_t ld, int seqs, int vocab, const int16_t *next, int64_t ld_next, int n_states,
                                       int n_classes, const int16_t *cls, int64_t ld_cls, int n_maps, const int32_t *map_of, int32_t *state,
                                       const int64_t *last, const int64_t *len, int64_t len_add, int64_t t_limit, gptq_stream_t stream) {
    if (!logits || !next || !cls || !map_of || !state || !len) return GPTQ_E_NULL;
    if (seqs < 1 || seqs > GPTQ_CONSTRAIN_MAX_SEQS || vocab < 1 || ld < vocab || n_states < 1 || n_states > GPTQ_CONSTRAIN_MAX_STATES ||
        n_classes < 1 || n_classes > GPTQ_CONSTRAIN_MAX_CLASSES || ld_next < n_classes || ld_cls < vocab || n_maps < 1)
        return GPTQ_E_SHAPE;
    if (!aligned(logits, 2) || !aligned(next, 2) || !aligned(cls, 2) || !aligned(map_of, 4) || !aligned(state, 4) || !aligned(last, 8) ||
        !aligned(len, 8))
        return GPTQ_E_ALIGN;
    const size_t lds = 2 * (size_t)n_classes;
    hipLaunchKernelGGL(constrain_rows_kernel, dim3(seqs), dim3(CS_NT), lds, (hipStream_t)stream, (uint16_t *)logits, ld, vocab, next, ld_next,
                       n_states, n_classes, cls, ld_cls, n_maps, map_of, state, last, len, len_add, t_limit);
    return (int)hipGetLastError();
}
