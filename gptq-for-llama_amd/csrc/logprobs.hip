// logprobs.hip -- token log-probabilities on the device (include/gptq_mi355x.h "token log-probabilities" states the rule; tests/logprobs_ref.py
// restates it in float64):
//   gptq_logprobs_rows_f16   for each of 1 .. 128 rows of fp16 logits: the log-probability of one chosen token, its rank, and the row's first
//                            `top` tokens with their log-probabilities, ONE launch, no workspace, no global atomics.
//
// One workgroup per row.  Pass 1 (sample_common.h's row_top, shared with sampling and beam.hip) finds the row's largest key and its first
// NaN / +inf (what a bad row means is this file's); passes 2 .. 4 are row_select.h's row_select, shared with beam.hip: the fp32 sum of exp(l - max) through a fixed tree -- the same bits on every call -- and the
// row's first n = max(top, 1) tokens in (key descending, id ascending) order.  The chosen token's key is known from the start (one load), so its
// rank -- the tokens with a larger key, plus the ones with its key and a lower id -- is one more count in row_select's pass 3, per thread in a
// register, summed over the wave by shuffles and over the 16 waves by thread 0: integers, no atomics.  Pass 5: log p of a token is a function of
// its key and the row's two numbers only, so the chosen token's value has the bits of its entry in the top list.
// The slot of the [steps][rows] outputs comes from device memory: one captured launch serves every step of a generation.
// Built with the strict flags: accurate expf / logf.
#include "../../include/gptq_mi355x.h"
#include "gptq_internal.h"
#include "row_select.h"

namespace {

using gptq::aligned;

constexpr int LP_MAX_TOP = GPTQ_LOGPROBS_MAX_TOP, LP_MAX_ROWS = 128;
static_assert(LP_MAX_TOP <= RS_MAX_N, "row_select's list holds a row's top entries");

__global__ __launch_bounds__(SM_NT) void logprobs_rows_kernel(const uint16_t *logits, int64_t ld, int vocab, const int64_t *ids, int top,
                                                              const int64_t *step, int64_t steps, float *chosen, int32_t *rank, int32_t *top_ids,
                                                              float *top_logprobs) {
    __shared__ RowSelectLds L;
    __shared__ u64 red64[SM_NW];
    __shared__ int red32[SM_NW];

    const int64_t slot = step ? step[0] : 0;
    if (slot < 0 || slot >= steps) return;                     // (the whole launch: nothing is written)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint16_t *row = logits + (int64_t)blockIdx.x * ld;
    const int64_t o = slot * (int64_t)gridDim.x + blockIdx.x;  // this row's record
    int32_t *oid = top_ids + o * top;                          // (never dereferenced with top == 0)
    float *olp = top_logprobs + o * top;
    const float nan = __builtin_nanf("");

    const int64_t cid64 = ids[blockIdx.x];
    const bool known = cid64 >= 0 && cid64 < (int64_t)vocab;
    const int cid = known ? (int)cid64 : 0;
    const uint32_t cbits = (uint32_t)row[cid];

    // ---- 1: the largest key, the first NaN / +inf (sample_common.h's row_top; its barrier stands behind the clear) ----
    row_select_clear(L, tid);
    const RowTop t1 = row_top<false>(row, vocab, tid, red64, red32);
    const uint32_t maxkey = t1.maxkey;
    if (t1.bad != SM_NONE || maxkey == key_of(0xFC00u)) {         // a NaN or +inf, or -inf only: no distribution
        if (tid == 0) {
            chosen[o] = nan;
            rank[o] = -1;
        }
        if (tid < top) {
            oid[tid] = tid;
            olp[tid] = nan;
        }
        return;
    }
    const float lmax = logit_of_key(maxkey);
    const uint32_t ckey = key_of(cbits);                       // (the row holds no NaN here)

    // ---- 2 .. 4: the sum, the first n tokens, and the chosen token's rank as one more count of pass 3 ----
    const int n = max(top, 1);
    int ahead = 0;
    const float total = row_select(row, vocab, tid, lmax, n, L, [&](int i, uint32_t key) { ahead += (key > ckey || (key == ckey && i < cid)) ? 1 : 0; });
    for (int d = 32; d > 0; d >>= 1) ahead += __shfl_xor(ahead, d, 64);
    if (lane == 0) red32[wave] = ahead;                        // (pass 1's values were read before row_select's first barrier)
    __syncthreads();

    // ---- 5: log p = (l - max) - log sum, from the key: equal keys give equal bits ----
    const float lse = logf(total);
    if (tid == 0) {
        int r = 0;
#pragma unroll
        for (int w = 0; w < SM_NW; w++) r += red32[w];
        chosen[o] = known ? (logit_of_key(ckey) - lmax) - lse : nan;
        rank[o] = known ? r : -1;
    }
    if (tid < top) {
        const u64 mine = L.list[tid];
        int p = 0;
        for (int q = 0; q < top; q++) p += L.list[q] > mine ? 1 : 0;
        oid[p] = (int32_t)~(uint32_t)mine;
        olp[p] = (logit_of_key((uint32_t)(mine >> 32)) - lmax) - lse;
    }
}

}  // namespace

extern "C" int gptq_logprobs_rows_f16(const void *logits, int64_t ld, int rows, int vocab, const int64_t *ids, int top, const int64_t *step,
                                      int64_t steps, float *chosen, int32_t *rank, int32_t *top_ids, float *top_logprobs, gptq_stream_t stream) {
    if (!logits || !ids || !chosen || !rank || (top > 0 && (!top_ids || !top_logprobs))) return GPTQ_E_NULL;
    if (rows < 1 || rows > LP_MAX_ROWS || top < 0 || top > LP_MAX_TOP || vocab < 1 || vocab < top || ld < vocab || steps < 1) return GPTQ_E_SHAPE;
    if (!aligned(logits, 2) || !aligned(ids, 8) || !aligned(step, 8) || !aligned(chosen, 4) || !aligned(rank, 4) ||
        (top > 0 && (!aligned(top_ids, 4) || !aligned(top_logprobs, 4))))
        return GPTQ_E_ALIGN;
    hipLaunchKernelGGL(logprobs_rows_kernel, dim3(rows), dim3(SM_NT), 0, (hipStream_t)stream, (const uint16_t *)logits, ld, vocab, ids, top, step,
                       steps, chosen, rank, top_ids, top_logprobs);
    return (int)hipGetLastError();
}
