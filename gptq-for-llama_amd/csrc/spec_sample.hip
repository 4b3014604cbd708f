// spec_sample.hip -- gptq_spec_sample_rows_f16 / gptq_spec_sample_batch_f16: the accept / resample rule of speculative sampling for one verify step
// of R rows of each of B sequences, ONE launch, grid (R, B), one workgroup per row (include/gptq_mi355x.h "speculative sampling" states the
// semantics; tests/spec_sample_ref.py restates them in float64).  ONE kernel, two entries: the rows entry is the B = 1 launch without the idle rule.
// What follows describes one sequence; sequence b reads rows b R .. b R + R - 1 of the packed per-row arrays, rows b (R - 1) .. of the draft
// logits, ids + b R, pos[b], and owns out + b (R + 1) and workspace words b (R + 1) .. : its own ticket and records.
//
// Row i of the target logits is the distribution p after ids[0 .. i]; ids[i + 1] = d is the token drafted for that place, from q: row i of the draft
// logits under the row's own setting, or a point mass at d without draft logits.  p and q are the kept sets and integer masses of sample.hip
// (sample_common.h: select_row and draw_row, the functions that kernel calls, so the last row's plain draw is its draw to the bit).  The two rows have different totals; a token's mass
// goes onto a common scale by one double multiplication with the row's factor c_p = 2^S / W_p (ONE IEEE division per row; S = the exponent of the
// mass unit): P(x) = floor(m_p(x) c_p + 1/2), Q(x) likewise, which are integers again (a division per token made the reject path slower):
//   accept    u_accept Q(d) < P(d)                     (doubles of integers below 2^41: one rounding, in the product)
//   reject    the first id whose running sum of r(x) = max(P(x) - Q(x), 0) exceeds floor(u_draw sum r)        (draw_row, as every draw)
// Every sum is an integer sum: no result depends on the order anything arrives in.
//
// The rows meet through the workspace: a workgroup stores its record {accepted, token} with a system-scope store, drains it and takes a ticket;
// the last to arrive reads all records with system-scope loads, finds the first rejecting row a, writes out = [a, d_0 .. d_{a-1}, t_a, t_a ..] and
// pos += a + 1, and puts the ticket word back to 0 for the next launch or replay.  Who arrives last decides nothing but who writes.
//
// Idle sequences (t_max > 0, the batch entry): sequence b is active iff 0 <= pos[b] < t_max, the rule of chunk_attn.hip.  The workgroups of an idle
// sequence return at once: no logits read, no ticket, nothing written.
#include "../../include/gptq_mi355x.h"
#include "gptq_internal.h"
#include "sample_common.h"

namespace {

using gptq::aligned;

// the row's factor onto the common scale 2^sh, and a mass on that scale, rounded to an integer; m <= W
GPTQ_DEV double scale_of(u64 W, int sh) { return ldexp(1.0, sh) / (double)W; }
GPTQ_DEV u64 scaled(u64 m, double c) { return (u64)((double)m * c + 0.5); }

__global__ __launch_bounds__(SM_NT) void spec_sample_rows_kernel(const uint16_t *logits, int64_t ld, const uint16_t *qlogits, int64_t ldq, int rows,
                                                                 int vocab, const int64_t *ids, const float *temperature, const int32_t *top_k,
                                                                 const float *top_p, const float *u_accept, const float *u_draw, int64_t *pos,
                                                                 int64_t t_max, int64_t *out, u64 *ws) {
    __shared__ SelectLds L;
    __shared__ u64 wsum[2][SM_NW];
    __shared__ int s_tok, s_last, s_first;
    __shared__ uint32_t s_dbits[2];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ri = blockIdx.x, sq = blockIdx.y;                     // row ri of sequence sq
    const bool bonus = ri == rows - 1;
    pos += sq;
    if (t_max > 0) {
        // The sequence's verdict, read ONCE, before this workgroup's ticket.  The only writer of pos[sq] in this launch is the sequence's last
        // arriver, and it writes behind the last ticket -- which every workgroup of an active sequence takes after this read -- so all R
        // workgroups see the launch's initial value and reach the same verdict.  A second read further down could see the advanced position.
        const int64_t p0 = __hip_atomic_load(pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p0 < 0 || p0 >= t_max) return;                          // (uniform over the workgroup: nobody waits at a barrier below)
    }
    const int r = sq * rows + ri;                                     // the row of the packed [B, R] arrays
    ids += (int64_t)sq * rows;
    out += (int64_t)sq * (rows + 1);
    ws += (int64_t)sq * (rows + 1);
    const uint16_t *row = logits + (int64_t)r * ld;
    const uint16_t *qrow = (qlogits && !bonus) ? qlogits + ((int64_t)sq * (rows - 1) + ri) * ldq : nullptr;
    const float T = temperature[r];
    const int kraw = top_k[r];
    const float praw = top_p[r];
    const float ud = clamp_u(u_draw[r]);
    const int64_t d64 = bonus ? -1 : ids[ri + 1];
    const int d = (d64 >= 0 && d64 < vocab) ? (int)d64 : -1;        // a draft outside the vocabulary is a draft nobody keeps
    const int sh = mass_exponent(vocab);

    const RowDist P = select_row(row, vocab, tid, T, kraw, praw, L);
    int acc = 0;
    if (tid == 0) s_tok = P.bad != SM_NONE ? P.bad : P.argmax;       // what the row emits unless a draw below says otherwise
    if (P.bad == SM_NONE) {
        RowDist Q;
        Q.bad = SM_NONE;
        Q.point = false;
        if (qrow) Q = select_row(qrow, vocab, tid, T, kraw, praw, L);
        const bool qdead = qrow && (Q.bad != SM_NONE || (Q.point && !P.point));      // a draft row with a NaN / +inf, or with no mass at all
        auto pmass = [&](int, uint32_t b) { return P.mass(key_of(b)); };
        if (P.point) {
            acc = !bonus && !qdead && d == P.argmax;
        } else if (bonus || d < 0 || qdead) {
            draw_row(row, vocab, tid, P.W, ud, pmass, wsum, &s_tok);                 // the plain draw of gptq_sample_rows_f16
        } else {
            const u64 one = (u64)1 << sh;
            const double cp = scale_of(P.W, sh), cq = qrow ? scale_of(Q.W, sh) : 0.0;
            if (tid == 0) {                                                          // one lane fetches the drafted token's logits for all
                s_dbits[0] = row[d];
                s_dbits[1] = qrow ? qrow[d] : 0u;
            }
            __syncthreads();
            const u64 Pd = scaled(P.mass(key_of(s_dbits[0])), cp);
            const u64 Qd = qrow ? scaled(Q.mass(key_of(s_dbits[1])), cq) : one;
            acc = (double)clamp_u(u_accept[r]) * (double)Qd < (double)Pd;
            if (!acc) {
                auto resid = [&](int i, uint32_t b) -> u64 {
                    const u64 p = scaled(P.mass(key_of(b)), cp);
                    const u64 q = qrow ? scaled(Q.mass(key_of(qrow[i])), cq) : (i == d ? one : 0);
                    return p > q ? p - q : 0;
                };
                u64 sum = 0;
                scan_row(row, vocab, tid, [&](int i, uint32_t b) { sum += resid(i, b); });
                for (int s = 32; s > 0; s >>= 1) sum += __shfl_xor(sum, s, 64);
                __syncthreads();                                                     // (red64 of the last select_row has been read)
                if (lane == 0) L.red64[wave] = sum;
                __syncthreads();
                sum = 0;
#pragma unroll
                for (int w = 0; w < SM_NW; w++) sum += L.red64[w];
                if (sum > 0) draw_row(row, vocab, tid, sum, ud, resid, wsum, &s_tok);   // sum == 0 (not in exact arithmetic): the argmax stays
            } else if (tid == 0) {
                s_tok = d;
            }
        }
    }
    __syncthreads();

    // ---- the record, the ticket, and the last arriver's prefix ----
    if (tid == 0) {
        __hip_atomic_store(ws + 1 + ri, ((u64)acc << 32) | (uint32_t)s_tok, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned *ticket = (unsigned *)ws;
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = (t == (unsigned)(rows - 1));
        if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = last;
        s_first = rows - 1;
    }
    __syncthreads();
    if (!s_last) return;
    int first = rows - 1;
    for (int i = tid; i < rows - 1; i += SM_NT) {
        const u64 rec = __hip_atomic_load(ws + 1 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (!(rec >> 32)) first = min(first, i);
    }
    if (first < rows - 1) atomicMin(&s_first, first);
    __syncthreads();
    const int a = s_first;
    const int64_t ta = (int64_t)(uint32_t)__hip_atomic_load(ws + 1 + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    for (int j = tid; j <= rows; j += SM_NT) out[j] = j == 0 ? (int64_t)a : (j <= a ? ids[j] : ta);
    if (tid == 0) *pos += a + 1;
}

}  // namespace

// the ONE validation and launch behind both entries; idle_rule false (the rows entry): t_max is not looked at and the kernel gets 0, any pos runs
static int launch(const void *logits, int64_t ld, const void *draft_logits, int64_t ld_draft, int seqs, int rows, int vocab, const int64_t *ids,
                  const float *temperature, const int32_t *top_k, const float *top_p, const float *u_accept, const float *u_draw, int64_t *pos,
                  bool idle_rule, int64_t t_max, int64_t *out, void *workspace, size_t workspace_bytes, gptq_stream_t stream) {
    if (!logits || !ids || !temperature || !top_k || !top_p || !u_accept || !u_draw || !pos || !out || !workspace) return GPTQ_E_NULL;
    if (seqs < 1 || seqs > 65535 || rows < 2 || vocab < 1 || ld < vocab || (draft_logits && ld_draft < vocab) ||
        (idle_rule && t_max < 1))
        return GPTQ_E_SHAPE;
    if (workspace_bytes < gptq_spec_sample_batch_workspace_bytes(seqs, rows)) return GPTQ_E_WORKSPACE;
    if (!aligned(logits, 2) || !aligned(draft_logits, 2) || !aligned(ids, 8) || !aligned(temperature, 4) || !aligned(top_k, 4) ||
        !aligned(top_p, 4) || !aligned(u_accept, 4) || !aligned(u_draw, 4) || !aligned(pos, 8) || !aligned(out, 8) || !aligned(workspace, 8))
        return GPTQ_E_ALIGN;
    hipLaunchKernelGGL(spec_sample_rows_kernel, dim3(rows, seqs), dim3(SM_NT), 0, (hipStream_t)stream, (const uint16_t *)logits, ld,
                       (const uint16_t *)draft_logits, ld_draft, rows, vocab, ids, temperature, top_k, top_p, u_accept, u_draw, pos,
                       idle_rule ? t_max : (int64_t)0, out, (u64 *)workspace);
    return (int)hipGetLastError();
}

extern "C" size_t gptq_spec_sample_workspace_bytes(int rows) { return rows < 2 ? 0 : ((size_t)rows + 1) * sizeof(u64); }

extern "C" size_t gptq_spec_sample_batch_workspace_bytes(int seqs, int rows) {
    return seqs < 1 ? 0 : (size_t)seqs * gptq_spec_sample_workspace_bytes(rows);
}

extern "C" int gptq_spec_sample_rows_f16(const void *logits, int64_t ld, const void *draft_logits, int64_t ld_draft, int rows, int vocab,
                                         const int64_t *ids, const float *temperature, const int32_t *top_k, const float *top_p,
                                         const float *u_accept, const float *u_draw, int64_t *pos, int64_t *out, void *workspace,
                                         size_t workspace_bytes, gptq_stream_t stream) {
    return launch(logits, ld, draft_logits, ld_draft, 1, rows, vocab, ids, temperature, top_k, top_p, u_accept, u_draw, pos, false, 0, out,
                  workspace, workspace_bytes, stream);
}

extern "C" int gptq_spec_sample_batch_f16(const void *logits, int64_t ld, const void *draft_logits, int64_t ld_draft, int seqs, int rows, int vocab,
                                          const int64_t *ids, const float *temperature, const int32_t *top_k, const float *top_p,
                                          const float *u_accept, const float *u_draw, int64_t *pos, int64_t t_max, int64_t *out, void *workspace,
                                          size_t workspace_bytes, gptq_stream_t stream) {
    return launch(logits, ld, draft_logits, ld_draft, seqs, rows, vocab, ids, temperature, top_k, top_p, u_accept, u_draw, pos, true, t_max, out,
                  workspace, workspace_bytes, stream);
}
