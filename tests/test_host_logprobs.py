"""CPU-side tests of the token log-probabilities (include/gptq_mi355x.h "token log-probabilities"): the symbol is exported and bound, every NULL /
shape / alignment rule of gptq_logprobs_rows_f16 returns its code on fake pointers (nothing is launched), the float64 restatement of the rule
(tests/logprobs_ref.py) gives the hand-worked answers and agrees with torch.log_softmax / torch.topk in float64 on tie-free rows."""
import math

import numpy as np
import torch

import logprobs_ref as R
from quant import _native

E_SHAPE, E_ALIGN, E_NULL = -2, -3, -4
NEG = float('-inf')


# ---- 1. the symbol ----
def test_symbols_are_exported_and_bound():
    lib = _native.lib()
    name = 'gptq_logprobs_rows_f16'
    assert hasattr(lib, name) and name in _native.EXPORTS
    assert len(getattr(lib, name).argtypes) == 13


# ---- 2. validation on fake pointers ----
def _call(lib, logits=4096, ld=1000, rows=4, vocab=1000, ids=8192, top=5, step=16384, steps=4, chosen=1 << 16, rank=1 << 17, top_ids=1 << 18,
          top_logprobs=1 << 19):
    return lib.gptq_logprobs_rows_f16(logits, ld, rows, vocab, ids, top, step, steps, chosen, rank, top_ids, top_logprobs, None)


def test_validation():
    lib = _native.lib()
    for name in ('logits', 'ids', 'chosen', 'rank', 'top_ids', 'top_logprobs'):
        assert _call(lib, **{name: None}) == E_NULL, name
    assert _call(lib, logits=None, rows=0) == E_NULL                           # NULL before shape
    assert _call(lib, ids=None, logits=4097) == E_NULL                         # ... and before alignment
    for kw in (dict(rows=0), dict(rows=129), dict(rows=-1), dict(top=-1), dict(top=33), dict(vocab=0, ld=0, top=0), dict(vocab=4, ld=4),
               dict(ld=999), dict(steps=0), dict(steps=-3), dict(vocab=0, ld=5, top=0, top_ids=None, top_logprobs=None)):
        assert _call(lib, **kw) == E_SHAPE, kw
    assert _call(lib, rows=129, ids=8192 + 4) == E_SHAPE                       # shape before alignment
    assert _call(lib, logits=4097) == E_ALIGN                                  # fp16 rows: 2 bytes, nothing more
    assert _call(lib, ids=8192 + 4) == E_ALIGN and _call(lib, step=16384 + 4) == E_ALIGN
    for name, at in (('chosen', 1 << 16), ('rank', 1 << 17), ('top_ids', 1 << 18), ('top_logprobs', 1 << 19)):
        assert _call(lib, **{name: at + 2}) == E_ALIGN, name


# ---- 3. hand-worked rows ----
def test_forty_equal_maxima_and_the_sixth_lowest_id():
    vocab = 100
    tied = np.sort(np.random.default_rng(0).permutation(vocab)[:40])
    row = np.full(vocab, -13.0, dtype=np.float16)
    row[tied] = 3.0
    lp_max = -math.log(40 + 60 * math.exp(-16.0))
    chosen, rank, ids, lps = R.record(row, int(tied[5]), 5)
    assert rank == 5 and abs(chosen - lp_max) < 1e-12
    assert ids.tolist() == tied[:5].tolist() and np.abs(lps - lp_max).max() < 1e-12
    for place in (0, 4, 39):
        assert R.record(row, int(tied[place]), 5)[1] == place
    low = np.setdiff1d(np.arange(vocab), tied)
    chosen, rank, _, _ = R.record(row, int(low[-1]), 0)
    assert rank == vocab - 1 and abs(chosen - (lp_max - 16.0)) < 1e-12


def test_minus_infinity_entries_and_fewer_finite_entries_than_top():
    row = np.array([NEG, 2.0, NEG, 1.0, 1.0], dtype=np.float16)
    lse = math.log(1 + 2 * math.exp(-1.0))
    chosen, rank, ids, lps = R.record(row, 2, 5)
    assert chosen == NEG and rank == 4                                         # -inf sorts last, in id order among themselves
    assert ids.tolist() == [1, 3, 4, 0, 2]
    assert np.abs(lps[:3] - np.array([-lse, -1 - lse, -1 - lse])).max() < 1e-12 and lps[3:].tolist() == [NEG, NEG]
    chosen, rank, _, _ = R.record(row, 4, 1)
    assert rank == 2 and abs(chosen - (-1 - lse)) < 1e-12


def test_a_vocabulary_of_one():
    for v in (0.0, -7.5, 60000.0):
        chosen, rank, ids, lps = R.record(np.array([v], dtype=np.float16), 0, 1)
        assert chosen == 0.0 and rank == 0 and ids.tolist() == [0] and lps.tolist() == [0.0]
    chosen, rank, ids, lps = R.record(np.array([NEG], dtype=np.float16), 0, 1)   # -inf only: no distribution
    assert math.isnan(chosen) and rank == -1 and ids.tolist() == [0] and np.isnan(lps).all()


def test_signed_zeros_are_one_value():
    z = np.full(40, -3.0, dtype=np.float16)
    z[[30, 4, 9, 20]] = 0.0, -0.0, 0.0, -0.0
    _, rank, ids, lps = R.record(z, 30, 4)
    assert ids.tolist() == [4, 9, 20, 30] and rank == 3 and len(set(lps.tolist())) == 1
    k = R.keys(np.array([-1.0, -0.0, 0.0, 6e-8, -6e-8, NEG, 65504.0], dtype=np.float16).view(np.uint16)).tolist()
    assert k[1] == k[2] and k[5] < k[0] < k[4] < k[1] < k[3] < k[6]


def test_rows_without_a_distribution_and_ids_out_of_range():
    good = np.array([0.5, -1.0, 2.0, 0.0], dtype=np.float16)
    for poison in (np.nan, np.inf):
        row = good.copy()
        row[1] = poison
        chosen, rank, ids, lps = R.record(row, 2, 3)
        assert math.isnan(chosen) and rank == -1 and ids.tolist() == [0, 1, 2] and np.isnan(lps).all()
    for token in (-1, 4, 2 ** 40):
        chosen, rank, ids, lps = R.record(good, token, 2)
        assert math.isnan(chosen) and rank == -1 and ids.tolist() == [2, 0] and np.isfinite(lps).all()


# ---- 4. the restatement against torch on tie-free rows ----
def test_restatement_is_log_softmax_and_topk_on_tie_free_rows():
    rng = np.random.default_rng(3)
    for vocab, scale in ((1000, 4.0), (257, 0.05), (33, 30.0)):
        values = np.unique((rng.standard_normal(8 * vocab) * scale).astype(np.float16))     # (-0 == +0 for unique: one of them survives)
        row = rng.permutation(values)[:vocab]
        assert row.size == vocab and np.unique(row).size == vocab
        x = torch.from_numpy(row.astype(np.float64))
        want = torch.log_softmax(x, dim=0)
        top = min(32, vocab)
        for token in (int(x.argmax()), int(x.argmin()), int(rng.integers(vocab))):
            chosen, rank, ids, lps = R.record(row, token, top)
            assert abs(chosen - float(want[token])) < 1e-12 and rank == int((x > x[token]).sum())
            assert ids.tolist() == torch.topk(x, top).indices.tolist()
            assert np.abs(lps - want[ids].numpy()).max() < 1e-12
