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
// The key, the row scan, the weigher and the wave's select live in sample_common.h, shared with spec_sample.hip.  That header also holds a COPY of
// the passes A .. E below as functions (select_row, draw_row): an edit to either must be mirrored in the other.
#include "../../include/gptq_mi355x.h"
#include "sample_common.h"

namespace {

__global__ __launch_bounds__(SM_NT) void sample_rows_kernel(const uint16_t *logits, int64_t ld, int vocab, const float *u, const float *temperature,
                                                            const int32_t *top_k, const float *top_p, int64_t *ids_out) {
    __shared__ uint32_t h1c[256], h2c[256];
    __shared__ u64 h1m[256], h2m[256];
    __shared__ u64 red64[SM_NW];
    __shared__ int red32[SM_NW];
    __shared__ u64 wsum[2][SM_NW];
    __shared__ Select sel;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x;
    const uint16_t *row = logits + (int64_t)r * ld;

    // ---- A: the largest key with its first index, and the first NaN / +inf ----
    u64 best = 0;                  // key << 32 | ~index: the maximum is the largest key at its lowest index
    int bad = 0x7FFFFFFF;
    scan_row(row, vocab, tid, [&](int i, uint32_t b) {
        if (not_finite_above(b)) bad = min(bad, i);
        const u64 cand = ((u64)key_of(b) << 32) | (uint32_t)~(uint32_t)i;
        best = cand > best ? cand : best;
    });
    for (int d = 32; d > 0; d >>= 1) {
        const u64 o = __shfl_xor(best, d, 64);
        best = o > best ? o : best;
        bad = min(bad, __shfl_xor(bad, d, 64));
    }
    if (lane == 0) {
        red64[wave] = best;
        red32[wave] = bad;
    }
    if (tid < 256) {
        h1c[tid] = 0;
        h1m[tid] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < SM_NW; w++) {
        best = red64[w] > best ? red64[w] : best;
        bad = min(bad, red32[w]);
    }
    const int argmax = (int)~(uint32_t)best;
    const uint32_t maxkey = (uint32_t)(best >> 32);
    const float T = temperature[r];
    const bool greedy = !(T > 0.f) || isinf(T);
    if (bad != 0x7FFFFFFF || greedy || maxkey == key_of(0xFC00u)) {      // (a row of -inf only has no mass to draw from: its first element)
        if (tid == 0) ids_out[r] = bad != 0x7FFFFFFF ? bad : argmax;
        return;
    }

    // ---- the row's parameters, sanitised ----
    const int kraw = top_k[r];
    const uint32_t k = (kraw > 0 && kraw < vocab) ? (uint32_t)kraw : 0u;          // 0: top-k off
    const float praw = top_p[r];
    const bool pon = !(isnan(praw) || praw >= 1.f);
    const double pd = praw > 0.f ? (double)praw : 1e-300;                           // p <= 0: only the top class survives
    float uu = u[r];
    uu = isnan(uu) || uu < 0.f ? 0.f : (uu >= 1.f ? 0x1.fffffep-1f : uu);
    const int bits_v = 32 - __builtin_clz((uint32_t)max(vocab - 1, 1));
    Weigher wq;
    wq.lmax = logit_of_key(maxkey);
    wq.T = T;
    wq.scale = ldexp(1.0, min(40, 62 - bits_v));

    // ---- B: level-1 histogram ----
    scan_row(row, vocab, tid, [&](int, uint32_t b) {
        const uint32_t key = key_of(b);
        atomicAdd(&h1c[key >> 8], 1u);
        atomicAdd(&h1m[key >> 8], wq(key));
    });
    __syncthreads();
    if (tid < 64) wave_select(h1c, h1m, 0u, 0, k, 0, &sel, lane);
    if (tid < 256) {
        h2c[tid] = 0;
        h2m[tid] = 0;
    }
    __syncthreads();

    // ---- C: top-k's threshold key and the mass Z of what it keeps ----
    uint32_t fkey = 0;             // the final kept set: key >= fkey, of mass W
    u64 W = sel.total;
    int kbin = -1;
    uint32_t kcnt = 0;
    u64 kabove = 0;
    if (k) {
        kbin = sel.kbin;
        kcnt = sel.kcnt;
        kabove = sel.kabove;
        scan_row(row, vocab, tid, [&](int, uint32_t b) {
            const uint32_t key = key_of(b);
            if ((int)(key >> 8) == kbin) {
                atomicAdd(&h2c[key & 255u], 1u);
                atomicAdd(&h2m[key & 255u], wq(key));
            }
        });
        __syncthreads();
        if (tid < 64) wave_select(h2c, h2m, kcnt, kabove, k, 0, &sel, lane);
        __syncthreads();
        fkey = ((uint32_t)kbin << 8) | (uint32_t)sel.kbin;
        W = sel.kge;
    }

    // ---- D: top-p on what top-k kept: a class stays iff the mass of the larger kept logits is < p Z ----
    if (pon) {
        const double x = ceil(pd * (double)W);
        const u64 thr = x < 1.0 ? 1 : (u64)x;           // integer masses: S < p Z  <=>  S < ceil(p Z)
        __syncthreads();                                 // (everybody has read sel)
        if (tid < 64) wave_select(h1c, h1m, 0u, 0, 0u, thr, &sel, lane);
        __syncthreads();
        const int pbin = sel.pbin;
        const u64 pabove = sel.pabove;
        if (pbin > kbin) {
            __syncthreads();
            if (tid < 256) {
                h2c[tid] = 0;
                h2m[tid] = 0;
            }
            __syncthreads();
            scan_row(row, vocab, tid, [&](int, uint32_t b) {
                const uint32_t key = key_of(b);
                if ((int)(key >> 8) == pbin) atomicAdd(&h2m[key & 255u], wq(key));
            });
            __syncthreads();
            if (tid < 64) wave_select(h2c, h2m, 0u, pabove, 0u, thr, &sel, lane);
            __syncthreads();
            fkey = ((uint32_t)pbin << 8) | (uint32_t)sel.pbin;
            W = sel.pge;
        } else if (pbin == kbin) {                       // the same bin as top-k's: its level-2 histogram is still there
            __syncthreads();
            if (tid < 64) wave_select(h2c, h2m, kcnt, kabove, 0u, thr, &sel, lane);
            __syncthreads();
            const uint32_t pkey = ((uint32_t)pbin << 8) | (uint32_t)sel.pbin;
            if (pkey > fkey) {
                fkey = pkey;
                W = sel.pge;
            }
        }
    }

    // ---- E: the first kept id whose running mass c_j (ascending id) exceeds u W; integer c_j: c_j > u W  <=>  c_j > floor(u W) ----
    const u64 target = (u64)((double)uu * (double)W);
    u64 running = 0;
    int parity = 0;
    // one round: m[j] = the mass of token base + j of this thread (0: not kept / none); rounds cover ascending, thread-contiguous id ranges
    auto round = [&](const u64(&m)[8], int base) -> bool {
        const u64 s = m[0] + m[1] + m[2] + m[3] + m[4] + m[5] + m[6] + m[7];
        u64 incl = s;
        for (int d = 1; d < 64; d <<= 1) {
            const u64 o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wsum[parity][wave] = incl;
        __syncthreads();
        u64 tot = 0, below = 0;
#pragma unroll
        for (int w = 0; w < SM_NW; w++) {
            const u64 t = wsum[parity][w];
            below += w < wave ? t : 0;
            tot += t;
        }
        parity ^= 1;
        if (running + tot > target) {
            u64 c = running + below + incl - s;          // the mass in front of this thread's tokens
            if (c <= target && target < c + s) {
                int pick = 0;
                bool found = false;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    c += m[j];
                    if (!found && c > target) {
                        pick = j;
                        found = true;
                    }
                }
                ids_out[r] = base + pick;
            }
            return true;
        }
        running += tot;
        return false;
    };
    const int head = min(vocab, (int)(((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) >> 1));
    const int nvec = (vocab - head) >> 3;
    {
        u64 m[8] = {};
        if (tid < head) {
            const uint32_t key = key_of(row[tid]);
            m[0] = key >= fkey ? wq(key) : 0;
        }
        if (head > 0 && round(m, tid)) return;
    }
    const u32x4 *v = (const u32x4 *)(row + head);
    for (int i0 = 0; i0 < nvec; i0 += SM_NT) {
        const int i = i0 + tid;
        u64 m[8] = {};
        if (i < nvec) {
            const u32x4 q = v[i];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t ka = key_of(q[j] & 0xFFFFu), kb = key_of(q[j] >> 16);
                m[2 * j] = ka >= fkey ? wq(ka) : 0;
                m[2 * j + 1] = kb >= fkey ? wq(kb) : 0;
            }
        }
        if (round(m, head + i * 8)) return;
    }
    {
        const int t = head + nvec * 8 + tid;
        u64 m[8] = {};
        if (t < vocab) {
            const uint32_t key = key_of(row[t]);
            m[0] = key >= fkey ? wq(key) : 0;
        }
        if (round(m, t)) return;
    }
    // not reached: W is the integer sum of exactly the masses added above and target < W.  Kept in range whatever happens.
    if (tid == 0) ids_out[r] = argmax;
}

inline bool aligned(const void *p, size_t a) { return ((uintptr_t)p % a) == 0; }

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
