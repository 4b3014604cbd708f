// row_select.h -- the device code gptq_beam_select_f16 (beam.hip, launch A) and gptq_logprobs_rows_f16 (logprobs.hip) share: for ONE row of fp16
// logits and one workgroup of SM_NT threads, the fp32 sum of exp(l - max) through a fixed tree and the first n tokens of the row in (key
// descending, id ascending) order -- sample_common.h's 16-bit order-preserving key, so -0 == +0 and -inf sorts below everything finite.
//
// What a bad row means (a NaN, +inf, -inf only) and what is written where stay with the caller: it finds the row's largest key first (pass 1,
// sample_common.h's row_top), and it gets the n entries back unsorted, in LDS.  Pass 2 sums exp(l - max) in fp32 -- eight accumulators per thread,
// one per slot of the row walk (scan_row_slots), added pairwise, a shuffle tree per wave, the 16 wave sums in a fixed tree: the same bits on every
// call -- and counts the high byte of the key into 256 bins; the wave's radix select finds the bin of the n-th largest element, pass 3 counts the
// low byte inside that bin, the select gives the threshold key; pass 4 collects every element above the threshold and, of the elements AT it, the
// ones with the lowest ids (all of them where they just fill the n places -- the usual case; otherwise a block-wide running count in ascending id,
// sample_common.h's block_prefix, hands out the places).  Only integer counts go through LDS atomics, so nothing depends on the order they arrive in.
#pragma once
#include "sample_common.h"

namespace {

constexpr int RS_MAX_N = 32;       // places of the list: 2 x GPTQ_BEAM_MAX_BEAMS, GPTQ_LOGPROBS_MAX_TOP

struct RowSelectLds {
    uint32_t h1c[256], h2c[256];
    float redf[SM_NW];
    int wcnt[2][SM_NW];
    Select sel;
    u64 list[RS_MAX_N];            // key << 32 | ~id: descending = (key descending, id ascending); the entries are distinct
    uint32_t filled;
};

// before row_select, with a __syncthreads() between the two (row_top, the caller's pass 1, has one)
GPTQ_DEV void row_select_clear(RowSelectLds &L, int tid) {
    if (tid < 256) {
        L.h1c[tid] = 0;
        L.h2c[tid] = 0;
    }
    if (tid == 0) L.filled = 0;
}

// passes 2 .. 4 for a row without NaN / +inf whose largest element is lmax (finite), 1 <= n <= min(RS_MAX_N, vocab).  Returns the sum of
// exp(l - lmax) (the same value in every thread); L.list[0 .. n) holds the first n tokens of the order, in no particular order, behind the
// function's last __syncthreads().  each(token id, key) is called once per element of the row, in pass 3 -- a count of the caller's rides there.
template <class F>
GPTQ_DEV float row_select(const uint16_t *row, int vocab, int tid, float lmax, int n, RowSelectLds &L, F each) {
    const int lane = tid & 63, wave = tid >> 6;

    // ---- 2: sum exp(l - max) through a fixed tree, and the level-1 histogram ----
    float a[8] = {};                                           // eight accumulators, one per slot of the walk
    scan_row_slots(row, vocab, tid, [&](int, uint32_t b, int slot) {
        const uint32_t key = key_of(b);
        atomicAdd(&L.h1c[key >> 8], 1u);
        a[slot] += expf(logit_of_key(key) - lmax);             // -inf gives 0
    });
    float sum = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0) L.redf[wave] = sum;
    __syncthreads();
    static_assert(SM_NW == 16, "the tree over the wave sums");
    const float *redf = L.redf;
    const float total = (((redf[0] + redf[1]) + (redf[2] + redf[3])) + ((redf[4] + redf[5]) + (redf[6] + redf[7]))) +
                        (((redf[8] + redf[9]) + (redf[10] + redf[11])) + ((redf[12] + redf[13]) + (redf[14] + redf[15])));

    // ---- 3: the key of the n-th largest element (vocab >= n: there is one) ----
    if (tid < 64) wave_select(L.h1c, 0u, (uint32_t)n, &L.sel, lane);
    __syncthreads();
    const int kbin = L.sel.kbin;
    const uint32_t kcnt = L.sel.kcnt;
    scan_row(row, vocab, tid, [&](int i, uint32_t b) {
        const uint32_t key = key_of(b);
        if ((int)(key >> 8) == kbin) atomicAdd(&L.h2c[key & 255u], 1u);
        each(i, key);
    });
    __syncthreads();
    if (tid < 64) wave_select(L.h2c, kcnt, (uint32_t)n, &L.sel, lane);
    __syncthreads();
    const uint32_t fkey = ((uint32_t)kbin << 8) | (uint32_t)L.sel.kbin;
    const int above = (int)L.sel.kcnt;                         // elements with a key above fkey: at most n - 1
    const int need = n - above;                                // places for the elements AT fkey: 1 .. ties
    const int ties = (int)L.h2c[L.sel.kbin];

    // ---- 4: collect ----
    const bool all_ties = ties == need;
    scan_row(row, vocab, tid, [&](int i, uint32_t b) {
        const uint32_t key = key_of(b);
        if (key > fkey || (all_ties && key == fkey)) {
            const uint32_t slot = atomicAdd(&L.filled, 1u);    // exactly n (or `above`) elements qualify
            if (slot < RS_MAX_N) L.list[slot] = ((u64)key << 32) | (uint32_t)~(uint32_t)i;
        }
    });
    if (!all_ties) {                                           // the `need` lowest ids at fkey: a running count in ascending id
        int running = 0, parity = 0;
        for (int base = 0; base < vocab && running < need; base += SM_NT * 8) {
            const int i0 = base + tid * 8;
            uint32_t mask = 0;
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (i0 + j < vocab && key_of((uint32_t)row[i0 + j]) == fkey) mask |= 1u << j;
            const int c = __builtin_popcount(mask);
            int tot;
            int rank = running + block_prefix(c, tid, L.wcnt, parity, tot);
#pragma unroll
            for (int j = 0; j < 8; j++)
                if ((mask >> j) & 1u) {
                    if (rank < need) L.list[above + rank] = ((u64)fkey << 32) | (uint32_t)~(uint32_t)(i0 + j);
                    rank++;
                }
            running += tot;
        }
    }
    __syncthreads();
    return total;
}

}  // namespace
