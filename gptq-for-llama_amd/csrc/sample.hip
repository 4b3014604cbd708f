// sample.hip -- gptq_sample_rows_f16: temperature / top-k / top-p sampling of one token per row of fp16 logits, ONE launch, one workgroup per row,
// every parameter per row and in device memory (include/gptq_mi355x.h "sampling" states the semantics; tests/sample_ref.py restates them in float64).
//
// Two tokens are tied iff their fp16 logits compare equal, so a row has at most 65 536 classes and an order-preserving 16-bit key exists.  The
// thresholds of top-k and top-p are keys, found by a two-level 256-bin radix select: level 1 histograms the key's high byte over the whole row
// (count and mass per bin), level 2 the low byte inside the one bin a threshold falls into.  A token's weight exp((l - l_max) / T) is computed in
// fp32 by the accurate expf and accumulated as an INTEGER multiple of 2^-40 (2^-(62 - ceil(log2 vocab)) for vocabularies above 2^22, so that no sum
// can overflow 64 bits): integer sums do not depend on the order the LDS atomics arrive in, so every mass -- and with it every decision and the id
// drawn -- is the same bits on every call, and the same token gets the same weight in every pass.  The rounding of a weight is at most 2^-41 of
// the top class's weight, vocab 2^-41 (1.5e-8 at 32 000) of the row's mass in total.
//
// Passes over the row (64 KB at vocab 32 000: L2 hits after the first): A max / first argmax / first non-finite, B level-1 histogram,
// C level-2 histogram of top-k's bin (top-k on), D level-2 histogram of top-p's bin (top-p on and another bin than C's), E the draw: a block-wide
// running sum of the kept weights in ascending token id that stops in the round where it passes u W.
// Rows need 2-byte alignment only: up to 7 leading and 7 trailing elements are read one by one, everything between as 16-byte vectors.
// The passes live in sample_common.h, each once: A .. D are select_row, E is draw_row.  spec_sample.hip calls the same two functions, so the bonus
// row of a verify step is this kernel's draw to the bit.
#include "../../include/gptq_mi355x.h"
#include "gptq_internal.h"
#include "sample_common.h"

namespace {

using gptq::aligned;

__global__ __launch_bounds__(SM_NT) void sample_rows_kernel(const uint16_t *logits, int64_t ld, int vocab, const float *u, const float *temperature,
                                                            const int32_t *top_k, const float *top_p, int64_t *ids_out) {
    __shared__ SelectLds L;
    __shared__ u64 wsum[2][SM_NW];

    const int tid = threadIdx.x;
    const int r = blockIdx.x;
    const uint16_t *row = logits + (int64_t)r * ld;

    const RowDist D = select_row(row, vocab, tid, temperature[r], top_k[r], top_p[r], L);
    if (tid == 0) ids_out[r] = D.bad != SM_NONE ? D.bad : D.argmax;      // (a row of -inf only has no mass to draw from: its first element)
    if (D.bad != SM_NONE || D.point) return;
    const float uu = clamp_u(u[r]);
    __syncthreads();               // (the argmax above is the fallback of the draw: W is the integer sum of exactly the masses it adds, target < W)
    draw_row(row, vocab, tid, D.W, uu, [&](int, uint32_t b) { return D.mass(key_of(b)); }, wsum, ids_out + r);
}

}  // namespace

extern "C" int gptq_sample_rows_f16(const void *logits, int64_t ld, int rows, int vocab, const float *u, const float *temperature, const int32_t *top_k,
                                    const float *top_p, int64_t *ids_out, gptq_stream_t stream) {
    if (!logits || !u || !temperature || !top_k || !top_p || !ids_out) return GPTQ_E_NULL;
    if (rows < 1 || vocab < 1 || ld < vocab) return GPTQ_E_SHAPE;
    if (!aligned(logits, 2) || !aligned(u, 4) || !aligned(temperature, 4) || !aligned(top_k, 4) || !aligned(top_p, 4) || !aligned(ids_out, 8))
        return GPTQ_E_ALIGN;
    hipLaunchKernelGGL(sample_rows_kernel, dim3(rows), dim3(SM_NT), 0, (hipStream_t)stream, (const uint16_t *)logits, ld, vocab, u, temperature, top_k,
                       top_p, ids_out);
    return (int)hipGetLastError();
}
