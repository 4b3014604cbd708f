"""CPU-side tests of gptq_sample_rows_f16 (include/gptq_mi355x.h "sampling"): the symbol is exported and bound, every rule of the host validation
returns its code on fake aligned pointers -- nothing is launched, no device is needed --, the float64 oracle of the semantics (tests/sample_ref.py)
gives the hand-worked answers, and every input of the GPU tests keeps its top-p decision MARGIN (1e-4 of Z, ten times the kernel's bar) away from
the nearest class edge."""
import numpy as np
import pytest
import torch

import sample_ref as R
from quant import _native

E_SHAPE, E_ALIGN, E_NULL = -2, -3, -4
ROWS, VOCAB = 3, 1000
INF = float('inf')


def _call(lib, logits=4096, ld=VOCAB, rows=ROWS, vocab=VOCAB, u=8192, temperature=12288, top_k=16384, top_p=20480, ids_out=24576):
    """fake, aligned, non-NULL "device pointers": every failing case below is refused before anything is launched"""
    return lib.gptq_sample_rows_f16(logits, ld, rows, vocab, u, temperature, top_k, top_p, ids_out, None)


def _row(values):
    return torch.tensor(values, dtype=torch.float32).half()


def test_sample_symbol_is_exported_and_bound():
    lib = _native.lib()
    assert hasattr(lib, 'gptq_sample_rows_f16') and 'gptq_sample_rows_f16' in _native.EXPORTS
    assert len(lib.gptq_sample_rows_f16.argtypes) == 10


def test_sample_null_rules():
    lib = _native.lib()
    for name in ('logits', 'u', 'temperature', 'top_k', 'top_p', 'ids_out'):
        assert _call(lib, **{name: None}) == E_NULL, name
    assert _call(lib, u=None, vocab=0) == E_NULL                               # NULL is reported before any shape rule
    assert _call(lib, ids_out=None, u=8192 + 2) == E_NULL                      # ... and before any alignment rule


def test_sample_shape_rules():
    lib = _native.lib()
    assert _call(lib, ld=VOCAB - 1) == E_SHAPE
    assert _call(lib, vocab=0, ld=0) == E_SHAPE
    assert _call(lib, vocab=-3) == E_SHAPE
    assert _call(lib, rows=0) == E_SHAPE
    assert _call(lib, rows=-1) == E_SHAPE
    assert _call(lib, rows=0, u=8192 + 2) == E_SHAPE                           # shape before alignment


def test_sample_alignment_rules():
    lib = _native.lib()
    assert _call(lib, logits=4096 + 1) == E_ALIGN                              # fp16 rows: 2 bytes, nothing more
    assert _call(lib, u=8192 + 2) == E_ALIGN                                   # float / int32 arrays: 4 bytes
    assert _call(lib, temperature=12288 + 2) == E_ALIGN
    assert _call(lib, top_k=16384 + 1) == E_ALIGN
    assert _call(lib, top_p=20480 + 2) == E_ALIGN
    assert _call(lib, ids_out=24576 + 4) == E_ALIGN                            # int64 ids: 8 bytes


def test_oracle_top_k_keeps_every_tie_at_the_kth_place():
    l = _row([1, 2, 1, 0])
    assert R.kept_set(l, 1.0, 2, 1.0).tolist() == [True, True, True, False]     # the 2nd largest is 1: both 1s stay, three tokens survive k = 2
    assert R.kept_set(l, 1.0, 1, 1.0).tolist() == [False, True, False, False]
    assert R.kept_set(l, 1.0, 3, 1.0).tolist() == [True, True, True, False]
    assert R.kept_set(l, 1.0, 4, 1.0).all() and R.kept_set(l, 1.0, 0, 1.0).all() and R.kept_set(l, 1.0, -3, 1.0).all()      # k >= vocab, k <= 0: off
    # c = 1/e, 1 + 1/e, 1 + 2/e of W = 1 + 2/e = 1.7358: u W = 0.3 -> 0, 0.8679 -> 1, 1.5 -> 2
    assert [R.sample(l, 1.0, 2, 1.0, u) for u in (0.0, 0.3 / 1.7358, 0.5, 1.5 / 1.7358)] == [0, 0, 1, 2]


def test_oracle_top_p_keeps_the_whole_boundary_class():
    l = _row([2, 1, 1, 0])
    # w = 1, 1/e, 1/e, 1/e^2; Z = 1.8711; p Z = 1.1227: the class of the 1s has S_gt = 1 < p Z and stays WHOLE (a stable sort would keep one of the
    # two: 1 + 1/e = 1.3679 already passes p Z); the 0 has S_gt = 1.7358 and goes
    assert R.kept_set(l, 1.0, 0, 0.6).tolist() == [True, True, True, False]
    assert R.kept_set(l, 1.0, 0, 0.5).tolist() == [True, False, False, False]   # p Z = 0.9355 < 1 = S_gt of the 1s
    assert R.kept_set(l, 1.0, 0, 0.93).tolist() == [True, True, True, True]     # p Z = 1.7401 > 1.7358
    assert R.kept_set(l, 1.0, 0, 0.92).tolist() == [True, True, True, False]    # p Z = 1.7214
    # top-p works on what top-k kept: k = 1 leaves Z = 1
    assert R.kept_set(l, 1.0, 1, 0.99).tolist() == [True, False, False, False]
    # temperature: T = 0.5 squares the weights: w = 1, e^-2, e^-2, e^-4; Z = 1.2890; p = 0.8: p Z = 1.0312 > 1
    assert R.kept_set(l, 0.5, 0, 0.8).tolist() == [True, True, True, False]
    assert np.allclose(R.probabilities(l, 0.5, 0, 0.8), np.array([1, np.exp(-2), np.exp(-2), 0]) / (1 + 2 * np.exp(-2)), rtol=1e-12)


def test_oracle_minus_infinity_is_never_drawn():
    l = _row([-INF, 0, -INF, 0])
    assert R.first_non_finite(l) is None
    assert R.weights(l, 1.0).tolist() == [0, 1, 0, 1]
    assert [R.sample(l, 1.0, 0, 1.0, u) for u in (0.0, 0.49, 0.5, 0.99, 1.0)] == [1, 1, 3, 3, 3]
    assert R.probabilities(l, 1.0, 0, 1.0).tolist() == [0, 0.5, 0, 0.5]


def test_oracle_p_to_zero_and_the_ends_of_u():
    l = _row([0, 3, 3, 1])
    for p in (0.0, -1.0, 1e-30, 1e-6):
        assert R.kept_set(l, 1.0, 0, p).tolist() == [False, True, True, False], p      # only the top class -- all of it
    assert [R.sample(l, 1.0, 0, 0.0, u) for u in (0.0, 0.49, 0.5, 1.0)] == [1, 1, 2, 2]
    flat = _row([0, 0, 0, 0])
    below_one = float(np.nextafter(np.float32(1), np.float32(0)))
    assert [R.sample(flat, 1.0, 0, 1.0, u) for u in (0.0, 0.25, 0.5, below_one, 1.0, 7.0, -1.0, float('nan'))] == [0, 1, 2, 3, 3, 3, 0, 0]
    assert R.admissible(1, flat, 1.0, 0, 1.0, 0.25) and R.admissible(0, flat, 1.0, 0, 1.0, 0.25)     # on the edge: either side
    assert not R.admissible(2, flat, 1.0, 0, 1.0, 0.25) and not R.admissible(4, flat, 1.0, 0, 1.0, 0.25)


def test_oracle_greedy_and_non_finite_rows():
    l = _row([1, 5, 5, -0.0])
    for T in (0.0, -1.0, INF, float('nan')):
        assert R.sample(l, T, 1, 0.5, 0.9) == 1                                 # the FIRST maximal logit
        assert R.admissible(1, l, T, 0, 1.0, 0.9) and not R.admissible(2, l, T, 0, 1.0, 0.9)
    assert R.sample(_row([0, float('nan'), INF, 1]), 1.0, 0, 1.0, 0.5) == 1
    assert R.sample(_row([0, 7, INF, float('nan')]), 0.0, 0, 1.0, 0.5) == 2
    assert R.kept_set(_row([0.0, -0.0, -1]), 1.0, 1, 1.0).tolist() == [True, True, False]        # -0 == +0: one class


@pytest.mark.parametrize('name', [c[0] for c in R.CASES])
def test_gpu_inputs_keep_their_top_p_decision_inside_a_class(name):
    logits, T, k, p = R.case(name)
    margin = R.top_p_margin(logits, T, k, p)
    kept = R.kept_set(logits, T, k, p)
    print('%s: V %d, T %g, k %d, p %.9g: %d kept, margin %.3e of Z' % (name, logits.numel(), T, k, p, int(kept.sum()), margin))
    assert margin >= R.MARGIN, (name, margin)
    assert p == float(np.float32(p))                                            # what the kernel reads is what the oracle read
    assert 1 <= kept.sum() < logits.numel()


def test_gpu_inputs_are_the_ones_the_bars_were_worked_out_for():
    kept = {name: int(R.kept_set(*R.case(name)).sum()) for name in ('v1000', 'ties', 'ties-k40', 'plateau', 'plateau-k2000')}
    assert kept == {'v1000': 34, 'ties': 25, 'ties-k40': 41, 'plateau': 1142, 'plateau-k2000': 1485}
    logits, T, k, p = R.case('ties')
    assert len(np.unique(logits.numpy())) == 70 and len(np.unique(logits.numpy()[R.kept_set(logits, T, k, p)])) == 11
