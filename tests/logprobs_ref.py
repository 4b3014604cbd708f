"""The rule of gptq_logprobs_rows_f16 (include/gptq_mi355x.h "token log-probabilities") restated in float64 on numpy fp16 bits, for
tests/test_host_logprobs.py and tests/test_gpu_logprobs.py.

Order: the 16-bit order-preserving key of the fp16 bits (csrc/sample_common.h key_of) descending, then the id ascending.  The key maps -0 onto
+0 -- the two are one value and the id decides between them --, every negative value below every positive one, and -inf below everything finite.
lp(v) = (l_v - max) - log(sum exp(l - max)).  A row with a NaN or +inf, or of -inf only, has no distribution."""
import numpy as np

MAX_TOP, MAX_ROWS = 32, 128
NEG = float('-inf')


def keys(bits):
    """the order-preserving key of fp16 bit patterns (uint16 array) as uint32: a larger logit has a larger key"""
    b = np.asarray(bits).astype(np.uint32)
    b = np.where(b == 0x8000, 0, b)
    return np.where(b & 0x8000, ~b & 0xFFFF, b | 0x8000).astype(np.uint32)


def order(row):
    """the ids of an fp16 row in (key descending, id ascending) order"""
    k = keys(np.asarray(row, dtype=np.float16).view(np.uint16)).astype(np.int64)
    return np.lexsort((np.arange(k.size), -k))


def no_distribution(row):
    b = np.asarray(row, dtype=np.float16).view(np.uint16)
    return bool(((b & 0x7FFF) > 0x7C00).any() or (b == 0x7C00).any() or (b == 0xFC00).all())


def log_softmax(row):
    """float64 lp of every token of an fp16 row that has a distribution (-inf stays -inf)"""
    x = np.asarray(row, dtype=np.float16).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        d = x - x.max()
        return d - np.log(np.exp(d).sum())


def record(row, token, top):
    """(chosen, rank, top_ids [top], top_logprobs [top]) of one fp16 row and its chosen token id, in float64 / int64"""
    row = np.asarray(row, dtype=np.float16)
    vocab = row.size
    assert 0 <= top <= MAX_TOP and vocab >= max(top, 1)
    if no_distribution(row):
        return float('nan'), -1, np.arange(top, dtype=np.int64), np.full(top, np.nan)
    o, lp = order(row), log_softmax(row)
    first = o[:top]
    if not 0 <= token < vocab:
        return float('nan'), -1, first, lp[first]
    return float(lp[token]), int(np.nonzero(o == token)[0][0]), first, lp[first]


def bar(ref):
    """the error bar of a log-probability with float64 value ref: 1e-5 up to |ref| = 32, 2^-21 |ref| beyond.  The sum has about 17 additions
    in depth plus a 2-ulp expf: <= 1.2e-6 relative, hence <= 1.2e-6 in the logarithm; logf is one ulp of at most 10.4, about 1e-6; the final
    subtraction is half an ulp of 32, about 1e-6: together about 3.2e-6, and the bar is three times that (2^-21 |ref| is the same at 21)."""
    ref = np.abs(np.asarray(ref, dtype=np.float64))
    return np.where(ref <= 32, 1e-5, ref * 2.0 ** -21)


def close(got, ref):
    """None when every float32 `got` is within bar(ref) of float64 `ref` (NaN where ref is NaN, -inf where it is -inf), else a message"""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    if got.shape != ref.shape:
        return 'shapes %r and %r' % (got.shape, ref.shape)
    fin = np.isfinite(ref)
    if not np.array_equal(np.isnan(got), np.isnan(ref)) or not np.array_equal(got == NEG, ref == NEG) or not np.isfinite(got[fin]).all():
        return 'NaN / -inf pattern differs: %r against %r' % (got, ref)
    err = np.abs(got[fin] - ref[fin])
    over = err > bar(ref[fin])
    if over.any():
        i = int(np.argmax(err / bar(ref[fin])))
        return 'entry %d: %.9g against %.12g, error %.3g > bar %.3g' % (i, got[fin][i], ref[fin][i], err[i], bar(ref[fin])[i])
    return None


def random_rows(rows, vocab, seed):
    """N(0, 4^2) rounded to fp16 (many natural ties at 32 000); with three rows or more, row 1 is shifted by +30 and row 2 scaled by 2^-6"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, vocab)) * 4.0
    if rows >= 3:
        x[1] += 30.0
        x[2] *= 2.0 ** -6
    return x.astype(np.float16)


def pick_ids(logits, top, seed, orders=None):
    """one chosen id per row, by turns: the argmax (rank 0), a random id, a member of the tie class at the `top` boundary (the LAST id of the
    class of the token in place max(top, 1) - 1: beyond the boundary where the class straddles it), the last token of the order.
    orders: order(row) of every row, where the caller has them"""
    rng = np.random.default_rng(seed)
    ids = []
    for r, row in enumerate(logits):
        o = order(row) if orders is None else orders[r]
        k = keys(row.view(np.uint16))
        kind = (r + seed) % 4                              # (a one-row launch gets every kind over the seeds)
        if kind == 0:
            ids.append(int(o[0]))
        elif kind == 1:
            ids.append(int(rng.integers(row.size)))
        elif kind == 2:
            edge = o[max(top, 1) - 1]
            ids.append(int(np.nonzero(k == k[edge])[0][-1]))
        else:
            ids.append(int(o[-1]))
    return np.array(ids, dtype=np.int64)
