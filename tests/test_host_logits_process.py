"""CPU-side tests of the logit processors (include/gptq_mi355x.h "logit processors"): the numpy restatement of the semantics
(tests/logits_process_ref.py) is pinned to transformers' own RepetitionPenaltyLogitsProcessor / MinNewTokensLengthLogitsProcessor on fp32 logits
-- equal after rounding both to fp16 --, its own edge rules give the hand-worked answers, and every rule of gptq_logits_process_f16's host
validation returns its code on fake aligned pointers: nothing is launched, no device is needed."""
import numpy as np
import torch

import logits_process_ref as R
from quant import _native

E_SHAPE, E_ALIGN, E_NULL = -2, -3, -4
INF = float('inf')
F16 = np.float16


def _bits(a):
    return np.asarray(a, dtype=np.float16).view(np.uint16)


# ---- 1. the restatement against transformers ----
def _hf_inputs(vocab=32000, n_ids=300, seed=0):
    rng = np.random.default_rng(seed)
    logits = R.realistic_logits(rng, (vocab,))
    ids = rng.integers(0, vocab, size=n_ids)
    ids[n_ids // 2:] = ids[:n_ids - n_ids // 2]             # every id at least twice
    ids[:4] = np.flatnonzero(np.isinf(logits.astype(np.float32)))[0], np.flatnonzero(_bits(logits) == 0x8000)[0], 7, 7
    return logits, ids


def test_repetition_penalty_is_hfs_arithmetic():
    from transformers import RepetitionPenaltyLogitsProcessor
    logits, ids = _hf_inputs()
    for penalty in (0.9, 1.18, 1.3):
        hf = RepetitionPenaltyLogitsProcessor(penalty)(torch.from_numpy(ids)[None], torch.from_numpy(logits.astype(np.float32))[None].clone())
        ours = R.process_row(logits, ids, gen_start=len(ids), repetition_penalty=penalty)
        assert np.array_equal(_bits(hf[0].numpy().astype(F16)), _bits(ours)), penalty
        changed = _bits(ours) != _bits(logits)
        assert 100 < changed.sum() <= len(np.unique(ids)) and not changed[np.setdiff1d(np.arange(len(logits)), ids)].any()


def test_min_new_tokens_is_hfs_rule_on_both_sides_of_the_boundary():
    from transformers import MinNewTokensLengthLogitsProcessor
    logits, ids = _hf_inputs(vocab=1000, n_ids=40)
    prompt, m, eos = 30, 10, [5, 999]
    for n in (prompt, prompt + m - 1, prompt + m, prompt + m + 1):
        hf = MinNewTokensLengthLogitsProcessor(prompt, m, eos)(torch.from_numpy(ids[:n])[None], torch.from_numpy(logits.astype(np.float32))[None].clone())
        ours = R.process_row(logits, ids[:n], gen_start=prompt, min_new_tokens=m, eos_ids=eos)
        assert np.array_equal(_bits(hf[0].numpy().astype(F16)), _bits(ours)), n
        masked = n - prompt < m
        assert (ours[eos] == -INF).all() == masked and (_bits(ours) != _bits(logits)).sum() == (2 if masked else 0)


# ---- 2. the restatement's own edge rules ----
def _row(values):
    return np.array(values, dtype=np.float16)


def test_ids_outside_the_vocabulary_are_ignored():
    l = _row([2, -2, 4, -4])
    out = R.process_row(l, [-1, 4, 2 ** 31, -2 ** 40, 1], 0, repetition_penalty=2.0, presence_penalty=1.0, min_new_tokens=9, eos_ids=[-1, 4, 9],
                        bias=[(-1, 5.0), (4, 5.0)])
    assert out.tolist() == [2, -5, 4, -4]                    # only token 1: -2 * 2 - 1


def test_minus_zero_is_not_negative_and_minus_infinity_stays():
    l = _row([-0.0, -INF, INF, 0.0])
    out = R.process_row(l, [0, 1, 2, 3], 4, repetition_penalty=1.5)
    assert _bits(out).tolist() == [0x8000, 0xFC00, 0x7C00, 0x0000]          # -0 / 1.5 = -0 (the division branch), -inf * 1.5, inf / 1.5
    out = R.process_row(l, [0, 1, 2, 3], 0, repetition_penalty=1.5, presence_penalty=0.5)
    assert _bits(out).tolist() == [0xB800, 0xFC00, 0x7C00, 0xB800]          # -0.5, -inf, inf, -0.5
    assert np.isnan(R.process_row(_row([np.nan, 1]), [0], 0, repetition_penalty=1.2)[0])


def test_bias_follows_the_penalty_with_a_second_rounding():
    l = _row([1.0, 3.0, -1.0])
    out = R.process_row(l, [1, 1], 0, repetition_penalty=1.3, presence_penalty=0.5, bias=[(1, 100.0), (2, -INF), (0, 0.25)])
    stored = F16(np.float32(3.0) / np.float32(1.3) - np.float32(0.5))
    assert out[1] == F16(np.float32(stored) + np.float32(100.0)) and out[2] == -INF and out[0] == 1.25
    # the EOS mask wins over a bias on the same token
    assert R.process_row(l, [], 0, min_new_tokens=1, eos_ids=[0], bias=[(0, 50.0)])[0] == -INF


def test_presence_counts_generated_positions_only_and_sanitising():
    l = _row([4.0, 4.0, 4.0, 4.0])
    out = R.process_row(l, [0, 1, 1, 2], 2, repetition_penalty=2.0, presence_penalty=1.0)
    assert out.tolist() == [2, 1, 1, 4]                      # 0: prompt only; 1: prompt and generated; 2: generated; 3: not in the history
    for rp in (0.0, -1.0, INF, float('nan')):
        assert R.process_row(l, [0, 1], 2, repetition_penalty=rp).tolist() == [4, 4, 4, 4], rp
    assert R.process_row(l, [0, 1], 0, presence_penalty=float('nan')).tolist() == [4, 4, 4, 4]
    assert R.process_row(l, [0], 5, min_new_tokens=-3, eos_ids=[1]).tolist() == [4, 4, 4, 4]
    assert R.process_row(l, [0], 5, min_new_tokens=1, eos_ids=[1])[1] == -INF          # gen_start above n: n - gen_start < m


def test_launch_restatement_rows_append_and_idle_rule():
    rng = np.random.default_rng(1)
    B, Rr, V, T = 4, 3, 40, 8
    logits = R.realistic_logits(rng, (B, Rr, V))
    hist = rng.integers(0, V, size=(B, T)).astype(np.int32)
    last = rng.integers(0, V, size=(B, Rr))
    lens = [3, 0, 7, 6]                                      # len_add = -1: n_b = 2, -1 (idle), 6 (rows 0, 1 fit: n = 7, 8; row 2 idle), 5
    args = ([0, 0, 0, 0], [1.3] * B, [0.5] * B, [0] * B)
    out, h2 = R.process(logits, hist, T, last, lens, -1, *args)
    assert np.array_equal(_bits(out[1]), _bits(logits[1])) and np.array_equal(h2[1], hist[1])
    assert np.array_equal(_bits(out[2, 2]), _bits(logits[2, 2])) and h2[2, 6] == last[2, 0] and h2[2, 7] == last[2, 1]
    assert h2[0, 2:5].tolist() == last[0].tolist() and np.array_equal(h2[0, :2], hist[0, :2]) and np.array_equal(h2[0, 5:], hist[0, 5:])
    for i in range(Rr):                                      # row i sees hist[:n_b] and last[0 .. i], never what a sibling appended
        want = R.process_row(logits[0, i], list(hist[0, :2]) + list(last[0, :i + 1]), 0, 1.3, 0.5)
        assert np.array_equal(_bits(out[0, i]), _bits(want))
    out, h2 = R.process(logits, hist, T, None, lens, 0, *args)               # without `last`: hist[b, 0 : n_b + i], nothing appended
    assert np.array_equal(h2, hist)
    assert np.array_equal(_bits(out[2, 1]), _bits(R.process_row(logits[2, 1], hist[2, :8], 0, 1.3, 0.5)))
    assert np.array_equal(_bits(out[2, 2]), _bits(logits[2, 2]))                     # n = 9 > t_hist


# ---- 3. the C entry's validation, on fake pointers ----
B_, R_, V_ = 2, 4, 1000
_PTRS = dict(logits=4096, hist=8192, last=12288, len=16384, gen_start=20480, rp=24576, pp=28672, min_new=32768, eos_ids=36864, bias_ids=40960,
             bias_vals=45056)


def _call(lib, ld=V_, seqs=B_, rows=R_, vocab=V_, ld_hist=64, t_hist=64, len_add=-1, n_eos=2, n_bias=3, **ptrs):
    p = dict(_PTRS, **ptrs)
    return lib.gptq_logits_process_f16(p['logits'], ld, seqs, rows, vocab, p['hist'], ld_hist, t_hist, p['last'], p['len'], len_add, p['gen_start'],
                                       p['rp'], p['pp'], p['min_new'], p['eos_ids'], n_eos, p['bias_ids'], p['bias_vals'], n_bias, None)


def test_symbol_is_exported_and_bound():
    lib = _native.lib()
    assert hasattr(lib, 'gptq_logits_process_f16') and 'gptq_logits_process_f16' in _native.EXPORTS
    assert len(lib.gptq_logits_process_f16.argtypes) == 21


def test_null_rules():
    lib = _native.lib()
    for name in ('logits', 'hist', 'len', 'gen_start', 'rp', 'pp', 'min_new', 'eos_ids', 'bias_ids', 'bias_vals'):
        assert _call(lib, **{name: None}) == E_NULL, name
    assert _call(lib, hist=None, vocab=0) == E_NULL                            # NULL is reported before any shape rule
    assert _call(lib, len=None, gen_start=20480 + 4) == E_NULL                 # ... and before any alignment rule
    # `last` may be NULL, and so may the lists whose count is 0: these reach the shape rules
    assert _call(lib, last=None, rows=0) == E_SHAPE
    assert _call(lib, eos_ids=None, n_eos=0, rows=0) == E_SHAPE
    assert _call(lib, bias_ids=None, bias_vals=None, n_bias=0, rows=0) == E_SHAPE


def test_shape_rules():
    lib = _native.lib()
    for kw in (dict(seqs=0), dict(seqs=65536), dict(rows=0), dict(rows=17), dict(vocab=0, ld=0), dict(vocab=131073, ld=131073), dict(ld=V_ - 1),
               dict(t_hist=0), dict(ld_hist=63), dict(n_eos=-1), dict(n_eos=9), dict(n_bias=-1), dict(n_bias=257)):
        assert _call(lib, **kw) == E_SHAPE, kw
    assert _call(lib, rows=17, hist=8192 + 2) == E_SHAPE                       # shape before alignment


def test_alignment_rules():
    lib = _native.lib()
    assert _call(lib, logits=4096 + 1) == E_ALIGN                              # fp16 rows: 2 bytes, nothing more
    for name in ('hist', 'rp', 'pp', 'min_new', 'eos_ids', 'bias_ids', 'bias_vals'):
        assert _call(lib, **{name: _PTRS[name] + 2}) == E_ALIGN, name          # int32 / float arrays: 4 bytes
    for name in ('last', 'len', 'gen_start'):
        assert _call(lib, **{name: _PTRS[name] + 4}) == E_ALIGN, name          # int64 arrays: 8 bytes
