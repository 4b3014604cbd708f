// sample_common.h -- the row passes of the token-choice kernels, each written once: one workgroup of SM_NT threads walks one row of fp16 logits.
// The order-preserving 16-bit key of an fp16 logit, the row walk that needs 2-byte alignment only (scan_row), pass 1 -- the largest key, its
// first index, the first NaN / +inf (row_top) --, a token's integer mass, the 256-bin radix select of one wave, the block-wide running prefix
// (block_prefix), and the passes of sample.hip as functions: A .. D as select_row, E as draw_row for any mass.  sample.hip states the method and
// calls the two once per row; spec_sample.hip calls them for up to two rows and a residual mass.  row_select.h (beam.hip, logprobs.hip) takes
// the key, the walk, pass 1, the prefix and the count-only select from here.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "gptq_device.h"

namespace {

typedef unsigned long long u64;
constexpr int SM_NT = 1024, SM_NW = SM_NT / 64;
constexpr int SM_NONE = 0x7FFFFFFF;

// -0 == +0; then negative values in reversed order below the positive ones: a larger logit has a larger key (NaN rows never get this far)
GPTQ_DEV uint32_t key_of(uint32_t b) {
    b = (b == 0x8000u) ? 0u : b;
    return (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
}
GPTQ_DEV float logit_of_key(uint32_t key) {
    const uint16_t b = (uint16_t)((key & 0x8000u) ? (key & 0x7FFFu) : (~key & 0xFFFFu));
    return (float)__builtin_bit_cast(half_t, b);
}
GPTQ_DEV bool not_finite_above(uint32_t b) { return (b & 0x7FFFu) > 0x7C00u || b == 0x7C00u; }   // NaN or +inf

// f(token id, fp16 bits, slot) for every element of the row, thread `tid` of SM_NT; a thread sees its ids in ascending order.  Up to 7 leading and
// 7 trailing elements are read one by one, everything between as 16-byte vectors.  slot: element j of a vector has slot j, a leading element
// slot 0, a trailing one slot 1 -- a constant at every call once the loop is unrolled, so f may index registers with it.
template <class F>
GPTQ_DEV void scan_row_slots(const uint16_t *row, int vocab, int tid, F f) {
    const int head = min(vocab, (int)(((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) >> 1));
    if (tid < head) f(tid, (uint32_t)row[tid], 0);
    const int nvec = (vocab - head) >> 3;
    const u32x4 *v = (const u32x4 *)(row + head);
    for (int i = tid; i < nvec; i += SM_NT) {
        const u32x4 q = v[i];
        const int base = head + i * 8;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            f(base + 2 * j, q[j] & 0xFFFFu, 2 * j);
            f(base + 2 * j + 1, q[j] >> 16, 2 * j + 1);
        }
    }
    const int t = head + nvec * 8 + tid;
    if (t < vocab) f(t, (uint32_t)row[t], 1);
}
template <class F>
GPTQ_DEV void scan_row(const uint16_t *row, int vocab, int tid, F f) {
    scan_row_slots(row, vocab, tid, [&](int i, uint32_t b, int) { f(i, b); });
}

// pass 1: the row's largest key, with INDEX its first index (key << 32 | ~index: the maximum is the largest key at its lowest index), and the first
// NaN / +inf (SM_NONE without one); the same values in every thread.  A shuffle tree per wave, the SM_NW wave results in red64 / red32, ONE
// __syncthreads(): what the caller clears in LDS before the call is clear behind it.  What a bad row means stays with the caller.
struct RowTop {
    uint32_t maxkey;
    int argmax, bad;
};
template <bool INDEX>
GPTQ_DEV RowTop row_top(const uint16_t *row, int vocab, int tid, u64 *red64, int *red32) {
    typedef typename std::conditional<INDEX, u64, uint32_t>::type best_t;
    const int lane = tid & 63, wave = tid >> 6;
    best_t best = 0;
    int bad = SM_NONE;
    scan_row(row, vocab, tid, [&](int i, uint32_t b) {
        if (not_finite_above(b)) bad = min(bad, i);
        best_t cand = key_of(b);
        if constexpr (INDEX) cand = (cand << 32) | (uint32_t)~(uint32_t)i;
        best = cand > best ? cand : best;
    });
    for (int d = 32; d > 0; d >>= 1) {
        const best_t o = __shfl_xor(best, d, 64);
        best = o > best ? o : best;
        bad = min(bad, __shfl_xor(bad, d, 64));
    }
    if (lane == 0) {
        red64[wave] = best;
        red32[wave] = bad;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < SM_NW; w++) {
        const best_t o = (best_t)red64[w];
        best = o > best ? o : best;
        bad = min(bad, red32[w]);
    }
    RowTop t;
    t.bad = bad;
    if constexpr (INDEX) {
        t.maxkey = (uint32_t)(best >> 32);
        t.argmax = (int)~(uint32_t)best;
    } else {
        t.maxkey = best;
        t.argmax = 0;
    }
    return t;
}

// the block-wide running prefix of one value per thread: returns the sum over the threads in front of this one and sets tot to the sum over all
// -- an inclusive shuffle scan per wave, the wave totals in wsum[parity] (the parity flips per call, so ONE __syncthreads() per call is enough).
// Every thread of the workgroup must call it.
template <class T>
GPTQ_DEV T block_prefix(T s, int tid, T (*wsum)[SM_NW], int &parity, T &tot) {
    const int lane = tid & 63, wave = tid >> 6;
    T incl = s;
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[parity][wave] = incl;
    __syncthreads();
    T below = 0;
    tot = 0;
#pragma unroll
    for (int w = 0; w < SM_NW; w++) {
        const T t = wsum[parity][w];
        below += w < wave ? t : 0;
        tot += t;
    }
    parity ^= 1;
    return below + incl - s;
}

struct Weigher {
    float lmax, T;
    double scale;
    // the token's mass as an integer multiple of 1 / scale; -inf gives exp(-inf) = 0
    __device__ __forceinline__ u64 operator()(uint32_t key) const {
        const float w = expf((logit_of_key(key) - lmax) / T);
        return (u64)((double)w * scale + 0.5);
    }
};

// what wave 0 reads off a 256-bin histogram {count, mass}; bins above a bin = the larger keys
struct Select {
    int kbin;          // top-k: the bin that holds the k-th largest element
    uint32_t kcnt;     //   elements above that bin (base included)
    u64 kabove, kge;   //   mass above that bin / of that bin and above (base included)
    int pbin;          // top-p: the lowest bin whose top has less than thr above it
    u64 pabove, pge;
    u64 total;
};

// wave 0 only (lane = tid < 64, four bins per lane).  k > 0: the bin with baseC + count above < k <= baseC + count above + own count.
// thr > 0: the bin with baseM + mass above < thr that is bin 0 or whose own mass brings it to thr.
GPTQ_DEV void wave_select(const uint32_t *hc, const u64 *hm, uint32_t baseC, u64 baseM, uint32_t k, u64 thr, Select *out, int lane) {
    uint32_t c[4], ca[4];
    u64 m[4], ma[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        c[j] = hc[4 * lane + j];
        m[j] = hm[4 * lane + j];
    }
    const uint32_t cs = c[0] + c[1] + c[2] + c[3];
    const u64 ms = m[0] + m[1] + m[2] + m[3];
    uint32_t ci = cs;
    u64 mi = ms;
    for (int d = 1; d < 64; d <<= 1) {           // inclusive suffix sums over the lanes
        const uint32_t cn = __shfl_down(ci, d, 64);
        const u64 mn = __shfl_down(mi, d, 64);
        if (lane + d < 64) {
            ci += cn;
            mi += mn;
        }
    }
    uint32_t cr = baseC + ci - cs;
    u64 mr = baseM + mi - ms;
#pragma unroll
    for (int j = 3; j >= 0; j--) {
        ca[j] = cr;
        ma[j] = mr;
        cr += c[j];
        mr += m[j];
    }
    if (lane == 0) out->total = mr;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int b = 4 * lane + j;
        if (k > 0 && ca[j] < k && ca[j] + c[j] >= k) {
            out->kbin = b;
            out->kcnt = ca[j];
            out->kabove = ma[j];
            out->kge = ma[j] + m[j];
        }
        if (thr > 0 && ma[j] < thr && (b == 0 || ma[j] + m[j] >= thr)) {
            out->pbin = b;
            out->pabove = ma[j];
            out->pge = ma[j] + m[j];
        }
    }
}

// the same for counts alone (beam.hip: no masses): sets out->kbin and out->kcnt for k > 0
GPTQ_DEV void wave_select(const uint32_t *hc, uint32_t baseC, uint32_t k, Select *out, int lane) {
    uint32_t c[4];
#pragma unroll
    for (int j = 0; j < 4; j++) c[j] = hc[4 * lane + j];
    const uint32_t cs = c[0] + c[1] + c[2] + c[3];
    uint32_t ci = cs;
    for (int d = 1; d < 64; d <<= 1) {           // inclusive suffix sums over the lanes
        const uint32_t cn = __shfl_down(ci, d, 64);
        if (lane + d < 64) ci += cn;
    }
    uint32_t cr = baseC + ci - cs;               // elements above this lane's bins
#pragma unroll
    for (int j = 3; j >= 0; j--) {
        if (cr < k && cr + c[j] >= k) {
            out->kbin = 4 * lane + j;
            out->kcnt = cr;
        }
        cr += c[j];
    }
}

// the exponent of the mass unit: masses are integer multiples of 2^-40, of 2^-(62 - ceil(log2 vocab)) above 2^22 tokens (no sum overflows 64 bits)
GPTQ_DEV int mass_exponent(int vocab) { return min(40, 62 - (32 - __builtin_clz((uint32_t)max(vocab - 1, 1)))); }

// the uniform of a draw, into [0, 1): NaN and negatives draw the first kept token, 1 and above the last
GPTQ_DEV float clamp_u(float u) { return isnan(u) || u < 0.f ? 0.f : (u >= 1.f ? 0x1.fffffep-1f : u); }

// ---- the passes as functions -------------------------------------------------------------------------------------------------------------
struct SelectLds {
    uint32_t h1c[256], h2c[256];
    u64 h1m[256], h2m[256];
    u64 red64[SM_NW];
    int red32[SM_NW];
    Select sel;
};

// one row under one setting, the same values in every thread of the workgroup
struct RowDist {
    int bad;           // the first NaN / +inf, SM_NONE without one: nothing below is set then
    int argmax;        // the first maximal logit
    bool point;        // a greedy setting, or a row of -inf only: the row's whole mass sits on argmax, nothing below is set
    uint32_t fkey;     // the kept set: key >= fkey ...
    u64 W;             // ... of mass W
    Weigher wq;
    __device__ __forceinline__ u64 mass(uint32_t key) const { return key >= fkey ? wq(key) : 0; }
};

// passes A .. D of sample.hip
GPTQ_DEV RowDist select_row(const uint16_t *row, int vocab, int tid, float T, int kraw, float praw, SelectLds &L) {
    const int lane = tid & 63;
    RowDist D;
    __syncthreads();               // (L may still be read by the previous call's last pass)
    if (tid < 256) {
        L.h1c[tid] = 0;
        L.h1m[tid] = 0;
    }
    const RowTop top = row_top<true>(row, vocab, tid, L.red64, L.red32);
    const int bad = top.bad;
    D.bad = bad;
    D.argmax = top.argmax;
    const uint32_t maxkey = top.maxkey;
    const bool greedy = !(T > 0.f) || isinf(T);
    D.point = greedy || maxkey == key_of(0xFC00u);
    D.fkey = 0;
    D.W = 0;
    D.wq.lmax = 0.f;
    D.wq.T = 1.f;
    D.wq.scale = 0.0;
    if (bad != SM_NONE || D.point) return D;

    const uint32_t k = (kraw > 0 && kraw < vocab) ? (uint32_t)kraw : 0u;          // 0: top-k off
    const bool pon = !(isnan(praw) || praw >= 1.f);
    const double pd = praw > 0.f ? (double)praw : 1e-300;                           // p <= 0: only the top class survives
    Weigher wq;
    wq.lmax = logit_of_key(maxkey);
    wq.T = T;
    wq.scale = ldexp(1.0, mass_exponent(vocab));

    scan_row(row, vocab, tid, [&](int, uint32_t b) {
        const uint32_t key = key_of(b);
        atomicAdd(&L.h1c[key >> 8], 1u);
        atomicAdd(&L.h1m[key >> 8], wq(key));
    });
    __syncthreads();
    if (tid < 64) wave_select(L.h1c, L.h1m, 0u, 0, k, 0, &L.sel, lane);
    if (tid < 256) {
        L.h2c[tid] = 0;
        L.h2m[tid] = 0;
    }
    __syncthreads();

    uint32_t fkey = 0;
    u64 W = L.sel.total;
    int kbin = -1;
    uint32_t kcnt = 0;
    u64 kabove = 0;
    if (k) {
        kbin = L.sel.kbin;
        kcnt = L.sel.kcnt;
        kabove = L.sel.kabove;
        scan_row(row, vocab, tid, [&](int, uint32_t b) {
            const uint32_t key = key_of(b);
            if ((int)(key >> 8) == kbin) {
                atomicAdd(&L.h2c[key & 255u], 1u);
                atomicAdd(&L.h2m[key & 255u], wq(key));
            }
        });
        __syncthreads();
        if (tid < 64) wave_select(L.h2c, L.h2m, kcnt, kabove, k, 0, &L.sel, lane);
        __syncthreads();
        fkey = ((uint32_t)kbin << 8) | (uint32_t)L.sel.kbin;
        W = L.sel.kge;
    }
    if (pon) {
        const double x = ceil(pd * (double)W);
        const u64 thr = x < 1.0 ? 1 : (u64)x;           // integer masses: S < p Z  <=>  S < ceil(p Z)
        __syncthreads();                                 // (everybody has read sel)
        if (tid < 64) wave_select(L.h1c, L.h1m, 0u, 0, 0u, thr, &L.sel, lane);
        __syncthreads();
        const int pbin = L.sel.pbin;
        const u64 pabove = L.sel.pabove;
        if (pbin > kbin) {
            __syncthreads();
            if (tid < 256) {
                L.h2c[tid] = 0;
                L.h2m[tid] = 0;
            }
            __syncthreads();
            scan_row(row, vocab, tid, [&](int, uint32_t b) {
                const uint32_t key = key_of(b);
                if ((int)(key >> 8) == pbin) atomicAdd(&L.h2m[key & 255u], wq(key));
            });
            __syncthreads();
            if (tid < 64) wave_select(L.h2c, L.h2m, 0u, pabove, 0u, thr, &L.sel, lane);
            __syncthreads();
            fkey = ((uint32_t)pbin << 8) | (uint32_t)L.sel.pbin;
            W = L.sel.pge;
        } else if (pbin == kbin) {                       // the same bin as top-k's: its level-2 histogram is still there
            __syncthreads();
            if (tid < 64) wave_select(L.h2c, L.h2m, kcnt, kabove, 0u, thr, &L.sel, lane);
            __syncthreads();
            const uint32_t pkey = ((uint32_t)pbin << 8) | (uint32_t)L.sel.pbin;
            if (pkey > fkey) {
                fkey = pkey;
                W = L.sel.pge;
            }
        }
    }
    D.fkey = fkey;
    D.W = W;
    D.wq = wq;
    return D;
}

// pass E of sample.hip for any integer mass(token id, fp16 bits of row[id]) of sum `total` > 0: the first id, ascending, whose running mass exceeds
// floor(uu total), written to *tok (an int in LDS, an int64_t of the result) by the thread that holds it.  *tok must hold the fallback (an id in
// range) before the call; the caller puts a __syncthreads() between this call and its read of *tok.  The id found does not depend on how the
// row is split over threads and rounds.  The walk is scan_row's, kept as rounds: every thread reaches every barrier, all leave in the same round.
template <class M, class O>
GPTQ_DEV void draw_row(const uint16_t *row, int vocab, int tid, u64 total, float uu, M mass, u64 (*wsum)[SM_NW], O *tok) {
    const u64 target = (u64)((double)uu * (double)total);
    u64 running = 0;
    int parity = 0;
    // one round: m[j] = the mass of token base + j of this thread (0: none); rounds cover ascending, thread-contiguous id ranges
    auto round = [&](const u64(&m)[8], int base) -> bool {
        const u64 s = m[0] + m[1] + m[2] + m[3] + m[4] + m[5] + m[6] + m[7];
        u64 tot;
        const u64 before = block_prefix(s, tid, wsum, parity, tot);
        if (running + tot > target) {
            u64 c = running + before;                    // the mass in front of this thread's tokens
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
                *tok = base + pick;
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
        if (tid < head) m[0] = mass(tid, (uint32_t)row[tid]);
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
                m[2 * j] = mass(head + i * 8 + 2 * j, q[j] & 0xFFFFu);
                m[2 * j + 1] = mass(head + i * 8 + 2 * j + 1, q[j] >> 16);
            }
        }
        if (round(m, head + i * 8)) return;
    }
    {
        const int t = head + nvec * 8 + tid;
        u64 m[8] = {};
        if (t < vocab) m[0] = mass(t, (uint32_t)row[t]);
        round(m, t);
    }
}

}  // namespace
