// logits_process.hip -- gptq_logits_process_f16: repetition / presence penalty, logit bias and the min-new-tokens EOS mask applied IN PLACE to rows of
// fp16 logits, ONE launch, grid (R, B): workgroup (i, b) edits row b R + i under sequence b's settings and token history, all of them in device
// memory (include/gptq_mi355x.h "logit processors" states the semantics; tests/logits_process_ref.py restates them in numpy).
//
// The history of a row is a list of up to t_hist token ids with any number of duplicates; what the penalties need is the SET of ids in it (S) and
// the set of those at generated positions (G).  Both are bitmaps of ceil(vocab / 32) words in dynamic LDS: the threads stride over the history and
// set bits with LDS atomicOr -- a duplicate sets a set bit --, then every thread sweeps its share of the words and edits a logit only where a bit
// is set, so each touched token has exactly ONE writer and is rounded once.  The bias list (distinct ids: thread j owns entry j) and the EOS list
// follow behind one workgroup barrier each; the three steps may hit the same token and must see each other's stores, which the barrier gives for
// the threads of one workgroup (one CU, one L1).  Nothing but LDS atomics: no global atomics, no workspace -- the bits of the result depend on the
// inputs only.
//
// With `last` (the tokens this step consumed) workgroup (i, b) appends hist[b, n_b + i] = last[b R + i] itself.  Its siblings take those tokens
// from `last`, never from hist, so no workgroup reads a hist word that another one writes in the same launch.
// Built with the strict flags: the penalty is an IEEE division and l * rp - presence must stay two roundings (no contraction).
#include "../../include/gptq_mi355x.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gptq_internal.h"

namespace {

using gptq::aligned;

constexpr int LP_NT = 256;            // thread j owns bias entry j and EOS entry j
constexpr int LP_MAX_ROWS = GPTQ_LOGITS_PROCESS_MAX_ROWS;
constexpr int LP_MAX_EOS = GPTQ_LOGITS_PROCESS_MAX_EOS;
constexpr int LP_MAX_BIAS = GPTQ_LOGITS_PROCESS_MAX_BIAS;
constexpr int LP_MAX_VOCAB = GPTQ_LOGITS_PROCESS_MAX_VOCAB;  // two bitmaps of vocab / 8 bytes: 32 KiB of LDS
static_assert(LP_MAX_BIAS <= LP_NT && LP_MAX_EOS <= LP_NT && LP_MAX_ROWS <= LP_NT, "one thread per list entry");

__device__ inline float h2f(uint16_t b) {
    _Float16 h;
    __builtin_memcpy(&h, &b, 2);
    return (float)h;
}

__device__ inline uint16_t f2h(float x) {     // round to nearest even
    const _Float16 h = (_Float16)x;
    uint16_t b;
    __builtin_memcpy(&b, &h, 2);
    return b;
}

__global__ __launch_bounds__(LP_NT) void logits_process_kernel(uint16_t *logits, int64_t ld, int rows, int vocab, int32_t *hist, int64_t ld_hist,
                                                               int64_t t_hist, const int64_t *last, const int64_t *len, int64_t len_add,
                                                               const int64_t *gen_start, const float *rep_penalty, const float *presence_penalty,
                                                               const int32_t *min_new_tokens, const int32_t *eos_ids, int n_eos,
                                                               const int32_t *bias_ids, const float *bias_vals, int n_bias) {
    extern __shared__ uint32_t bitmap[];
    const int tid = threadIdx.x;
    const int i = blockIdx.x, b = blockIdx.y;
    const int nwords = (vocab + 31) >> 5;
    uint32_t *S = bitmap, *G = bitmap + nwords;

    // ---- the row's history: hist[b, 0 : nh] and then last[b R + 0 .. i] -- or idle ----
    const int64_t nb = len[b] + len_add;
    const int64_t n = nb + i + (last ? 1 : 0);            // the history's length
    if (nb < 0 || nb > t_hist || n > t_hist) return;      // (the whole workgroup: nothing is read or written)
    const int64_t nh = last ? nb : nb + i;
    const int64_t gs = gen_start[b];
    int32_t *h = hist + (int64_t)b * ld_hist;
    uint16_t *row = logits + ((int64_t)b * rows + i) * ld;

    for (int w = tid; w < 2 * nwords; w += LP_NT) bitmap[w] = 0;
    __syncthreads();
    for (int64_t p = tid; p < nh; p += LP_NT) {
        const int32_t t = h[p];
        if (t >= 0 && t < vocab) {
            atomicOr(&S[t >> 5], 1u << (t & 31));
            if (p >= gs) atomicOr(&G[t >> 5], 1u << (t & 31));
        }
    }
    if (last && tid <= i) {
        const int64_t t = last[(int64_t)b * rows + tid];
        if (t >= 0 && t < vocab) {
            atomicOr(&S[t >> 5], 1u << ((int)t & 31));
            if (nb + tid >= gs) atomicOr(&G[t >> 5], 1u << ((int)t & 31));
        }
        if (tid == i) h[nb + i] = (int32_t)t;             // the append: position nb + i < t_hist (n <= t_hist)
    }
    __syncthreads();

    // ---- 1: the penalties on every token of S, one writer per token, one rounding ----
    float rp = rep_penalty[b];
    if (!(rp > 0.f) || isinf(rp)) rp = 1.f;
    float pres = presence_penalty[b];
    if (isnan(pres)) pres = 0.f;
    for (int w = tid; w < nwords; w += LP_NT) {
        uint32_t s = S[w];
        const uint32_t g = G[w];
        while (s) {
            const int bit = __builtin_ctz(s);
            s &= s - 1;
            const int v = (w << 5) + bit;
            const float l = h2f(row[v]);
            float x = l < 0.f ? l * rp : l / rp;
            if ((g >> bit) & 1u) x -= pres;
            row[v] = f2h(x);
        }
    }
    __syncthreads();

    // ---- 2: the bias list (distinct ids), on what step 1 stored ----
    if (tid < n_bias) {
        const int32_t v = bias_ids[tid];
        if (v >= 0 && v < vocab) row[v] = f2h(h2f(row[v]) + bias_vals[tid]);
    }
    __syncthreads();

    // ---- 3: no EOS before min_new_tokens generated ones ----
    const int32_t m = min_new_tokens[b];
    if (m > 0 && n - gs < (int64_t)m && tid < n_eos) {
        const int32_t v = eos_ids[tid];
        if (v >= 0 && v < vocab) row[v] = 0xFC00u;
    }
}

}  // namespace

extern "C" int gptq_logits_process_f16(void *logits, int64_t ld, int seqs, int rows, int vocab, int32_t *hist, int64_t ld_hist, int64_t t_hist,
                                       const int64_t *last, const int64_t *len, int64_t len_add, const int64_t *gen_start,
                                       const float *repetition_penalty, const float *presence_penalty, const int32_t *min_new_tokens,
                                       const int32_t *eos_ids, int n_eos, const int32_t *bias_ids, const float *bias_vals, int n_bias,
                                       gptq_stream_t stream) {
    if (!logits || !hist || !len || !gen_start || !repetition_penalty || !presence_penalty || !min_new_tokens || (n_eos > 0 && !eos_ids) ||
        (n_bias > 0 && (!bias_ids || !bias_vals)))
        return GPTQ_E_NULL;
    if (seqs < 1 || seqs > 65535 || rows < 1 || rows > LP_MAX_ROWS || vocab < 1 || vocab > LP_MAX_VOCAB || ld < vocab || t_hist < 1 ||
        ld_hist < t_hist || n_eos < 0 || n_eos > LP_MAX_EOS || n_bias < 0 || n_bias > LP_MAX_BIAS)
        return GPTQ_E_SHAPE;
    if (!aligned(logits, 2) || !aligned(hist, 4) || !aligned(last, 8) || !aligned(len, 8) || !aligned(gen_start, 8) ||
        !aligned(repetition_penalty, 4) || !aligned(presence_penalty, 4) || !aligned(min_new_tokens, 4) || (n_eos > 0 && !aligned(eos_ids, 4)) ||
        (n_bias > 0 && (!aligned(bias_ids, 4) || !aligned(bias_vals, 4))))
        return GPTQ_E_ALIGN;
    const size_t lds = 2 * (size_t)((vocab + 31) / 32) * sizeof(uint32_t);
    hipLaunchKernelGGL(logits_process_kernel, dim3(rows, seqs), dim3(LP_NT), lds, (hipStream_t)stream, (uint16_t *)logits, ld, rows, vocab, hist,
                       ld_hist, t_hist, last, len, len_add, gen_start, repetition_penalty, presence_penalty, min_new_tokens, eos_ids, n_eos,
                       bias_ids, bias_vals, n_bias);
    return (int)hipGetLastError();
}
