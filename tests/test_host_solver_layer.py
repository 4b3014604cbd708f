"""gptq_solver_layer_f32 without a GPU: the symbol, its binding, and the validation that returns before any launch (the pointers of the bad
calls are never dereferenced)."""
import os
import re

import pytest

from quant import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'gptq_solver_layer_f32'
P = 0x10000                                   # a 16-byte aligned address nobody reads
GOOD = dict(W=P, ldw=256, Hinv=P, ldh=256, rows=8, cols=256, groupsize=128, maxq=15, sym=0, fit=1, scale=P, zero=P, ldg=2, Q=P, ldq=256,
            loss_rows=P, stream=None)


def test_symbol_is_exported_bound_and_declared():
    hdr = open(os.path.join(ROOT, 'include', 'gptq_mi355x.h')).read()
    decl = re.search(r'int %s\(([^;]*)\);' % NAME, hdr)
    assert decl and NAME in _native.EXPORTS and hasattr(_native.lib(), NAME)
    assert len(decl.group(1).split(',')) == len(_native.lib().gptq_solver_layer_f32.argtypes) == len(GOOD) == 17


@pytest.mark.parametrize('bad,code', [(dict(W=None), -4), (dict(cols=200), -2), (dict(cols=64), -2), (dict(groupsize=0), -2), (dict(maxq=0), -2),
                                      (dict(ldw=252), -2), (dict(ldg=1), -2), (dict(W=P + 4), -3), (dict(ldq=258), -3)])
def test_bad_calls_are_refused_before_the_launch(bad, code):
    assert _native.lib().gptq_solver_layer_f32(*{**GOOD, **bad}.values()) == code
