// beam.hip -- beam search on the device (include/gptq_mi355x.h "beam search" states the rule and the layout of the state block; tests/beam_ref.py
// restates the rule in float64):
//   gptq_beam_select_f16   one beam step on N = 2 .. 16 rows of fp16 logits, TWO launches whose only hand-off is the kernel boundary -- no tickets,
//                          no flags, no global atomics;
//   gptq_kv_reorder_f16    cache row b of every layer continues row parent[b], in place, ONE launch.
//
// Launch A, one workgroup per row (passes 2 .. 4 are row_select.h's row_select, shared with logprobs.hip; what a bad row means and what is written
// stay here): pass 1 (sample_common.h's row_top, shared with sampling) finds the row's largest key and its first NaN / +inf; pass 2 sums
// exp(l - max) in fp32 -- eight accumulators per thread added pairwise, a shuffle tree per wave, the 16 wave sums in a fixed tree: the same bits on every call -- and counts the
// high byte of the 16-bit order-preserving key (sample_common.h) into 256 bins; the wave's radix select finds the bin of the 2N-th largest element,
// pass 3 counts the low byte inside that bin, the select gives the threshold key; pass 4 collects every element above the threshold and, of the
// elements AT it, the ones with the lowest ids (all of them where they just fill the 2N places -- the usual case; otherwise a block-wide running
// count in ascending id hands out the places).  The counts are integers, so nothing depends on the order the LDS atomics arrive in.  Wave 0 puts
// the 2N entries into (logit descending, id ascending) order and writes the row's record {max, log sum, bad, 2N x (id, fp16 bits)}.  The global
// top 2N of the N x vocab candidates is a subset of the union of the rows' top 2N: adding the beam's score is monotone in the logit.
//
// Launch B, one wave: scores the N x 2N candidates -- log p is a function of the logit's bits and the row's two numbers only, so equal logits of
// a row give bit-equal scores --, takes the best 2N by (score descending, beam ascending, id ascending) in 2N rounds of a wave-wide maximum, and
// applies the rule's steps 3 .. 6 to the state block.
//
// The reorder: one thread owns a 16-byte column (layer, k or v, t, chunk) across ALL rows.  It loads the source rows it needs into registers and
// then stores only the rows with parent[b] != b: swaps and cycles are right without any order between threads or workgroups, and an identity step
// writes nothing.  A fixed grid walks the columns below len[0] (read from device memory: one captured launch serves every step).
// Built with the strict flags: accurate expf / logf / powf and IEEE division.
#include "../../include/gptq_mi355x.h"
#include "gptq_internal.h"
#include "row_select.h"

namespace {

using gptq::aligned;

constexpr int BM_MAX = GPTQ_BEAM_MAX_BEAMS;          // beams, and the slots every per-beam array of the state block has
constexpr float BM_DEAD = -1e9f;
// the state block in 4-byte words (the header documents it)
constexpr int ST_EOS = 0, ST_MAX_NEW = 1, ST_LP = 2, ST_ES = 3, ST_T_CAP = 4, ST_BEAMS = 5, ST_T = 6, ST_OPEN = 7, ST_DONE = 8, ST_STATUS = 9;
constexpr int ST_SCORE = 16, ST_PARENT = 32, ST_TOKEN = 48, ST_POOL = 80, ST_CAND = 160, ST_REC = 288, ST_TABLES = 1376;
constexpr int POOL_WORDS = 5, CAND_WORDS = 4, REC_WORDS = 4 + 4 * BM_MAX;
static_assert(ST_TOKEN + 2 * BM_MAX == ST_POOL && ST_POOL + POOL_WORDS * BM_MAX == ST_CAND && ST_CAND + CAND_WORDS * 2 * BM_MAX == ST_REC &&
                  ST_REC + REC_WORDS * BM_MAX == ST_TABLES && ST_TOKEN % 2 == 0,
              "the layout of the state block");
static_assert(2 * BM_MAX <= RS_MAX_N, "row_select's list holds a row's 2N entries");

GPTQ_DEV uint32_t bits_of_key(uint32_t key) { return (key & 0x8000u) ? (key & 0x7FFFu) : (~key & 0xFFFFu); }

// ---- launch A ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SM_NT) void beam_row_kernel(const uint16_t *logits, int64_t ld, int vocab, int n2, uint32_t *state) {
    __shared__ RowSelectLds L;
    __shared__ u64 red64[SM_NW];
    __shared__ int red32[SM_NW];

    const int tid = threadIdx.x;
    const uint16_t *row = logits + (int64_t)blockIdx.x * ld;
    uint32_t *rec = state + ST_REC + blockIdx.x * REC_WORDS;

    // ---- 1: the largest key, the first NaN / +inf (sample_common.h's row_top; its barrier stands behind the clear) ----
    row_select_clear(L, tid);
    const RowTop t1 = row_top<false>(row, vocab, tid, red64, red32);
    const uint32_t maxkey = t1.maxkey;
    if (t1.bad != SM_NONE || maxkey == key_of(0xFC00u)) {         // a NaN or +inf, or -inf only: ids in range, the update scores them DEAD
        if (tid == 0) {
            rec[0] = 0;
            rec[1] = 0;
            rec[2] = 1;
            rec[3] = 0;
        }
        if (tid < n2) {
            rec[4 + 2 * tid] = (uint32_t)tid;
            rec[5 + 2 * tid] = 0;
        }
        return;
    }
    const float lmax = logit_of_key(maxkey);

    // ---- 2 .. 4: the sum of exp(l - max) and the row's first 2N tokens (row_select.h) ----
    const float total = row_select(row, vocab, tid, lmax, n2, L, [](int, uint32_t) {});
    const u64 *list = L.list;

    // ---- 5: (logit descending, id ascending) = the composite descending; the entries are distinct ----
    if (tid == 0) {
        rec[0] = __builtin_bit_cast(uint32_t, lmax);
        rec[1] = __builtin_bit_cast(uint32_t, logf(total));
        rec[2] = 0;
        rec[3] = 0;
    }
    if (tid < n2) {
        const u64 mine = list[tid];
        int rank = 0;
        for (int q = 0; q < n2; q++) rank += list[q] > mine ? 1 : 0;
        rec[4 + 2 * rank] = ~(uint32_t)mine;
        rec[5 + 2 * rank] = bits_of_key((uint32_t)(mine >> 32));
    }
}

// ---- launch B ------------------------------------------------------------------------------------------------------------------------------
GPTQ_DEV uint32_t score_key(float x) {                       // a larger score has a larger key; no NaN gets here
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(64) void beam_update_kernel(uint32_t *st, int N) {
    __shared__ uint32_t sk[2 * BM_MAX * BM_MAX];
    __shared__ u64 so[2 * BM_MAX * BM_MAX];
    __shared__ float sc[2 * BM_MAX * BM_MAX];
    __shared__ float cs[2 * BM_MAX], ps[BM_MAX];
    __shared__ int cb[2 * BM_MAX], cv[2 * BM_MAX], pf[BM_MAX];

    const int lane = threadIdx.x;
    int *sti = (int *)st;
    float *stf = (float *)st;
    if (sti[ST_DONE]) return;
    const int t = sti[ST_T], t_cap = sti[ST_T_CAP];
    if (sti[ST_BEAMS] != N || t_cap < 1 || t < 0 || t >= t_cap) {     // a block that was not set up for this call: nothing is touched but the flags
        if (lane == 0) {
            sti[ST_STATUS] |= 2;
            sti[ST_DONE] = 1;
        }
        return;
    }
    const int n2 = 2 * N, total = N * n2;
    const int eos = sti[ST_EOS], max_new = min(sti[ST_MAX_NEW], t_cap), es = sti[ST_ES];
    const float lp = stf[ST_LP];
    const int open = sti[ST_OPEN];

    // ---- 1: the N x 2N scores ----
    bool anybad = false;
    for (int c = lane; c < total; c += 64) {
        const int b = c / n2, j = c - b * n2;
        const uint32_t *rec = st + ST_REC + b * REC_WORDS;
        const bool bad = rec[2] != 0;
        anybad |= bad;
        const float l = (float)__builtin_bit_cast(half_t, (uint16_t)rec[5 + 2 * j]);
        const float logp = (l - __builtin_bit_cast(float, rec[0])) - __builtin_bit_cast(float, rec[1]);
        float s = bad ? BM_DEAD : stf[ST_SCORE + b] + logp;
        s = s == 0.f ? 0.f : s;
        sc[c] = s;
        sk[c] = score_key(s);
        so[c] = ((u64)(uint32_t)(255 - b) << 32) | (uint32_t)~rec[4 + 2 * j];
    }
    if (__ballot(anybad) != 0 && lane == 0) sti[ST_STATUS] |= 1;
    __syncthreads();

    // ---- 2: the best 2N by (score descending, beam ascending, id ascending): one wave-wide maximum per rank ----
    for (int r = 0; r < n2; r++) {
        uint32_t bk = 0;
        u64 bo = 0;
        int bc = 0;
        for (int c = lane; c < total; c += 64) {
            const uint32_t k = sk[c];
            const u64 o = so[c];
            if (k > bk || (k == bk && o > bo)) {
                bk = k;
                bo = o;
                bc = c;
            }
        }
        for (int d = 32; d > 0; d >>= 1) {
            const uint32_t k = (uint32_t)__shfl_xor((int)bk, d, 64);
            const u64 o = __shfl_xor(bo, d, 64);
            const int c = __shfl_xor(bc, d, 64);
            if (k > bk || (k == bk && o > bo)) {
                bk = k;
                bo = o;
                bc = c;
            }
        }
        if (lane == 0) {
            cs[r] = sc[bc];
            cb[r] = bc / n2;
            cv[r] = (int)~(uint32_t)bo;
            sk[bc] = 0;                                        // taken (below every real key)
            so[bc] = 0;
        }
        __syncthreads();
    }

    // ---- 3: the next running beams: the first N by (score with the hits at DEAD) descending, rank ascending ----
    const bool live = lane < n2;
    const float c = live ? cs[lane] : 0.f;
    const int b = live ? cb[lane] : 0, v = live ? cv[lane] : 0;
    const bool hit = live && (v == eos || t + 1 >= max_new);
    const float m = hit ? BM_DEAD : c;
    int p = 0;
    for (int q = 0; q < n2; q++) {
        const float mq = __shfl(m, q, 64);
        p += (mq > m || (mq == m && q < lane)) ? 1 : 0;
    }
    // the pool before this step, one entry and one offer per lane < N (every word is read before any is written)
    const bool isold = lane < N;
    float osc = BM_DEAD;
    int ofin = 0, ostep = 0, opar = 0, otok = 0;
    if (isold) {
        const uint32_t *e = st + ST_POOL + lane * POOL_WORDS;
        osc = __builtin_bit_cast(float, e[0]);
        ofin = (int)e[1];
        ostep = (int)e[2];
        opar = (int)e[3];
        otok = (int)e[4];
    }
    const bool full = __popcll(__ballot(isold && ofin != 0)) == N;
    __syncthreads();
    if (live && p < N) {
        stf[ST_SCORE + p] = m;
        sti[ST_PARENT + p] = b;
        ((int64_t *)(st + ST_TOKEN))[p] = (int64_t)v;
        sti[ST_TABLES + t * N + p] = b;
        sti[ST_TABLES + (t_cap + t) * N + p] = v;
    }
    const u64 first = __ballot(live && p == 0);
    const float s0 = __shfl(m, __builtin_ctzll(first), 64);
    if (live) {
        uint32_t *e = st + ST_CAND + lane * CAND_WORDS;
        e[0] = __builtin_bit_cast(uint32_t, c);
        e[1] = (uint32_t)b;
        e[2] = (uint32_t)v;
        e[3] = hit ? 1u : 0u;
    }

    // ---- 4: the pool: its old entries and the offers, by score descending; an old entry wins a tie, offers keep their rank order ----
    const bool offer = hit && lane < N && open != 0 && !(full && es == 1);
    const float fsc = c / powf((float)(t + 1), lp);
    int pold = 0, poff = 0;
    for (int q = 0; q < N; q++) {
        const float qs = __shfl(osc, q, 64), qf = __shfl(fsc, q, 64);
        const bool qo = __shfl((int)offer, q, 64) != 0;
        pold += (qs > osc || (qs == osc && q < lane)) ? 1 : 0;
        pold += (qo && qf > osc) ? 1 : 0;
        poff += (qs >= fsc) ? 1 : 0;
        poff += (qo && (qf > fsc || (qf == fsc && q < lane))) ? 1 : 0;
    }
    if (isold && pold < N) {
        uint32_t *e = st + ST_POOL + pold * POOL_WORDS;
        e[0] = __builtin_bit_cast(uint32_t, osc);
        e[1] = (uint32_t)ofin;
        e[2] = (uint32_t)ostep;
        e[3] = (uint32_t)opar;
        e[4] = (uint32_t)otok;
        ps[pold] = osc;
        pf[pold] = ofin;
    }
    if (offer && poff < N) {
        uint32_t *e = st + ST_POOL + poff * POOL_WORDS;
        e[0] = __builtin_bit_cast(uint32_t, fsc);
        e[1] = 1u;
        e[2] = (uint32_t)t;
        e[3] = (uint32_t)b;
        e[4] = (uint32_t)v;
        ps[poff] = fsc;
        pf[poff] = 1;
    }
    const bool allhit = __popcll(__ballot(hit)) == n2;
    __syncthreads();

    // ---- 5, 6: can the best running beam still enter the pool; does the search go on ----
    if (lane == 0) {
        const int t1 = t + 1;
        const int L = (es == 2 && lp > 0.f) ? sti[ST_MAX_NEW] : t1;
        const float best = s0 / powf((float)L, lp);
        float worst = ps[0];
        bool fullnow = true;
        for (int i = 0; i < N; i++) {
            worst = fminf(worst, ps[i]);
            fullnow = fullnow && pf[i] != 0;
        }
        bool any = false;
        for (int i = 0; i < N; i++) any = any || best > (pf[i] != 0 ? worst : BM_DEAD);
        const bool opennow = open != 0 && any;
        sti[ST_T] = t1;
        sti[ST_OPEN] = opennow ? 1 : 0;
        sti[ST_DONE] = (opennow && !(fullnow && es == 1) && !allhit) ? 0 : 1;
    }
}

// ---- the reorder ---------------------------------------------------------------------------------------------------------------------------
constexpr int RO_NT = 256, RO_BLOCKS = 2048;

__global__ __launch_bounds__(RO_NT) void kv_reorder_kernel(uint16_t *k_cache, uint16_t *v_cache, int layers, int rows, int t_max, int row_elems,
                                                           int64_t layer_stride, const int32_t *parent, const int64_t *len) {
    const int64_t n = min(max(len[0], (int64_t)0), (int64_t)t_max);
    int par[BM_MAX];
    bool anymove = false;
#pragma unroll
    for (int b = 0; b < BM_MAX; b++) {
        int p = b < rows ? parent[b] : b;
        if (p < 0 || p >= rows) p = b;                         // (never from gptq_beam_select_f16; no row outside the cache is ever read)
        par[b] = p;
        anymove |= p != b;
    }
    if (!anymove) return;
    const int chunks = row_elems >> 3;
    const int64_t per = n * chunks;                            // columns of one (layer, k or v)
    const int64_t columns = per * 2 * layers;
    const int64_t row_stride = (int64_t)t_max * row_elems;
    for (int64_t i = (int64_t)blockIdx.x * RO_NT + threadIdx.x; i < columns; i += (int64_t)RO_BLOCKS * RO_NT) {
        const int64_t lk = i / per, within = i - lk * per;     // within = t chunks + chunk: a wave reads consecutive 16-byte chunks of a row
        uint16_t *base = ((lk & 1) ? v_cache : k_cache) + (lk >> 1) * layer_stride + within * 8;
        u32x4 reg[BM_MAX];
#pragma unroll
        for (int b = 0; b < BM_MAX; b++)
            if (par[b] != b) reg[b] = *(const u32x4 *)(base + par[b] * row_stride);
#pragma unroll
        for (int b = 0; b < BM_MAX; b++)
            if (par[b] != b) *(u32x4 *)(base + b * row_stride) = reg[b];
    }
}

}  // namespace

extern "C" size_t gptq_beam_state_bytes(int beams, int t_max) {
    if (beams < 2 || beams > BM_MAX || t_max < 1) return 0;
    return ((size_t)ST_TABLES + 2 * (size_t)t_max * (size_t)beams) * sizeof(uint32_t);
}

extern "C" int gptq_beam_select_f16(const void *logits, int64_t ld, int beams, int vocab, void *state, gptq_stream_t stream) {
    if (!logits || !state) return GPTQ_E_NULL;
    if (beams < 2 || beams > BM_MAX || vocab < 2 * beams || ld < vocab) return GPTQ_E_SHAPE;
    if (!aligned(logits, 2) || !aligned(state, 16)) return GPTQ_E_ALIGN;
    hipLaunchKernelGGL(beam_row_kernel, dim3(beams), dim3(SM_NT), 0, (hipStream_t)stream, (const uint16_t *)logits, ld, vocab, 2 * beams,
                       (uint32_t *)state);
    hipLaunchKernelGGL(beam_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (uint32_t *)state, beams);
    return (int)hipGetLastError();
}

extern "C" int gptq_kv_reorder_f16(void *k_cache, void *v_cache, int layers, int rows, int t_max, int row_elems, int64_t layer_stride,
                                   const int32_t *parent, const int64_t *len, gptq_stream_t stream) {
    if (!k_cache || !v_cache || !parent || !len) return GPTQ_E_NULL;
    if (layers < 1 || rows < 1 || rows > BM_MAX || t_max < 1 || row_elems < 8 || row_elems % 8 != 0 ||
        layer_stride < (int64_t)rows * t_max * row_elems || layer_stride % 8 != 0)
        return GPTQ_E_SHAPE;
    if (!aligned(k_cache, 16) || !aligned(v_cache, 16) || !aligned(parent, 4) || !aligned(len, 8)) return GPTQ_E_ALIGN;
    hipLaunchKernelGGL(kv_reorder_kernel, dim3(RO_BLOCKS), dim3(RO_NT), 0, (hipStream_t)stream, (uint16_t *)k_cache, (uint16_t *)v_cache, layers,
                       rows, t_max, row_elems, layer_stride, parent, len);
    return (int)hipGetLastError();
}
