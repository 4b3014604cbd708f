"""numpy restatement of gptq_logits_process_f16 (include/gptq_mi355x.h "logit processors") in exactly the stated arithmetic: the penalties are
np.float32 operations followed by ONE .astype(np.float16), the bias starts from the stored fp16 value and rounds a second time, the EOS mask
writes fp16 -inf.  Shared by tests/test_host_logits_process.py (pinned there to transformers' own processors) and the GPU tests."""
import numpy as np

MAX_ROWS, MAX_EOS, MAX_BIAS, MAX_VOCAB = 16, 8, 256, 131072


def sanitise(repetition_penalty, presence_penalty, min_new_tokens):
    rp = np.float32(repetition_penalty)
    if not np.isfinite(rp) or rp <= 0:
        rp = np.float32(1)
    pres = np.float32(presence_penalty)
    if np.isnan(pres):
        pres = np.float32(0)
    return rp, pres, max(int(min_new_tokens), 0)


def process_row(row, history, gen_start, repetition_penalty=1.0, presence_penalty=0.0, min_new_tokens=0, eos_ids=(), bias=()):
    """one row: `row` fp16 [vocab] (a new array is returned), `history` the ids of positions 0 .. n - 1, bias a sequence of (id, value) with
    distinct ids"""
    row = np.array(row, dtype=np.float16, copy=True)
    vocab = row.shape[0]
    history = np.asarray(history, dtype=np.int64).reshape(-1)
    n = history.shape[0]
    rp, pres, m = sanitise(repetition_penalty, presence_penalty, min_new_tokens)
    ok = (history >= 0) & (history < vocab)
    S = np.unique(history[ok])
    G = np.unique(history[ok & (np.arange(n) >= gen_start)])
    if S.size:
        with np.errstate(all='ignore'):
            l = row[S].astype(np.float32)
            x = np.where(l < 0, l * rp, l / rp).astype(np.float32)
            x = np.where(np.isin(S, G), x - pres, x).astype(np.float32)
            row[S] = x.astype(np.float16)
    for v, val in bias:
        if 0 <= int(v) < vocab:
            with np.errstate(all='ignore'):
                row[int(v)] = (row[int(v)].astype(np.float32) + np.float32(val)).astype(np.float16)
    if m > 0 and n - int(gen_start) < m:                    # (m <= 0 is OFF, also where gen_start lies above n)
        for v in eos_ids:
            if 0 <= int(v) < vocab:
                row[int(v)] = np.float16(-np.inf)
    return row


def process(logits, hist, t_hist, last, lens, len_add, gen_start, repetition_penalty, presence_penalty, min_new_tokens, eos_ids=(), bias=()):
    """the whole launch: logits fp16 [B, R, vocab], hist int32 [B, ld_hist], last int64 [B, R] or None, the per-sequence arrays of length B.
    Returns (new logits, new hist); idle rows come back as they went in."""
    logits = np.array(logits, dtype=np.float16, copy=True)
    hist = np.array(hist, dtype=np.int32, copy=True)
    hist_in = hist.copy()                       # every row reads the history as it was BEFORE the launch (siblings' tokens come from `last`)
    B, R, _ = logits.shape
    for b in range(B):
        nb = int(lens[b]) + int(len_add)
        for i in range(R):
            n = nb + i + (1 if last is not None else 0)
            if nb < 0 or n > t_hist:
                continue
            if last is not None:
                history = np.concatenate([hist_in[b, :nb].astype(np.int64), np.asarray(last[b, :i + 1], dtype=np.int64)])
                hist[b, nb + i] = np.int64(last[b, i]).astype(np.int32)
            else:
                history = hist_in[b, :nb + i].astype(np.int64)
            logits[b, i] = process_row(logits[b, i], history, int(gen_start[b]), repetition_penalty[b], presence_penalty[b], min_new_tokens[b],
                                       eos_ids, bias)
    return logits, hist


def realistic_logits(rng, shape, sigma=3.0, n_neg_inf=3):
    """fp16 logits at the scale an LM head produces (sigma ~ 3), with a few -inf and one -0 planted in every row"""
    x = (sigma * rng.standard_normal(shape)).astype(np.float16)
    flat = x.reshape(-1, shape[-1])
    for r in flat:
        at = rng.choice(shape[-1], size=min(n_neg_inf + 1, shape[-1]), replace=False)
        r[at[:-1]] = np.float16(-np.inf)
        r[at[-1]] = np.float16(-0.0)
    return x
