"""CPU-side tests of batched speculative sampling: gptq_spec_sample_batch_f16 (csrc/spec_sample.hip) is exported, bound, declared and validates its
arguments on the host before anything is launched, and the inputs tests/test_gpu_spec_sample_batch.py feeds it -- windows of the 16-row case of
spec_sample_ref.gpu_case (tests/spec_sample_batch_cases.py) -- keep the margins that make the oracle's accept flags binding."""
import functools
import os
import re

import numpy as np
import pytest

import sample_ref as S
import spec_sample_batch_cases as C
import spec_sample_ref as X
from quant import _native

E_SHAPE, E_ALIGN, E_NULL, E_WORKSPACE = -2, -3, -4, -5       # include/gptq_mi355x.h
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'gptq_mi355x.h')


def test_both_symbols_are_exported_bound_and_declared():
    lib = _native.lib()
    text = open(HEADER).read()
    for name, nargs in (('gptq_spec_sample_batch_f16', 19), ('gptq_spec_sample_batch_workspace_bytes', 2)):
        assert hasattr(lib, name) and name in _native.EXPORTS
        assert len(getattr(lib, name).argtypes) == nargs
        decl = re.search(r'^(?:int|size_t) %s\(([^;]*)\);' % name, text, re.M)
        assert decl is not None and decl.group(1).count(',') == nargs - 1, name
    import ctypes
    assert lib.gptq_spec_sample_batch_workspace_bytes.restype is ctypes.c_size_t


def test_workspace_formula():
    lib = _native.lib()
    ws, single = lib.gptq_spec_sample_batch_workspace_bytes, lib.gptq_spec_sample_workspace_bytes
    for B in (1, 2, 3, 16, 65535):
        for R in (2, 5, 8, 16):
            assert ws(B, R) == B * single(R) == B * (R + 1) * 8
    assert ws(0, 5) == 0 and ws(-1, 5) == 0 and ws(4, 1) == 0


def test_every_validation_rule_on_the_host():
    lib = _native.lib()
    B, R, V = 4, 5, 50
    need = lib.gptq_spec_sample_batch_workspace_bytes(B, R)
    P = 4096                                                   # any aligned non-NULL address: nothing is launched
    ok = dict(logits=P, ld=V, q=P, ldq=V, seqs=B, rows=R, vocab=V, ids=P, T=P, k=P, p=P, ua=P, ud=P, pos=P, tm=128, out=P, ws=P, wb=need)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gptq_spec_sample_batch_f16(a['logits'], a['ld'], a['q'], a['ldq'], a['seqs'], a['rows'], a['vocab'], a['ids'], a['T'], a['k'],
                                              a['p'], a['ua'], a['ud'], a['pos'], a['tm'], a['out'], a['ws'], a['wb'], None)
    pointers = ('logits', 'ids', 'T', 'k', 'p', 'ua', 'ud', 'pos', 'out', 'ws')
    for name in pointers:
        assert call(**{name: None}) == E_NULL, name
        assert call(**{name: None, 'seqs': 0, 'wb': 0, 'q': P + 1}) == E_NULL, name          # reported first
    for kw in (dict(seqs=0), dict(seqs=-3), dict(seqs=65536), dict(rows=1), dict(rows=0), dict(rows=-1), dict(vocab=0), dict(ld=V - 1),
               dict(ldq=V - 1), dict(tm=0), dict(tm=-7)):
        assert call(**dict(kw, wb=1 << 40)) == E_SHAPE, kw
    assert call(seqs=0, wb=0) == E_SHAPE and call(tm=0, wb=0) == E_SHAPE                   # ... before the workspace
    for kw in (dict(wb=need - 1), dict(wb=0), dict(seqs=B + 1), dict(rows=R + 1), dict(seqs=65535)):
        assert call(**kw) == E_WORKSPACE, kw
    assert call(wb=need - 1, logits=P + 1) == E_WORKSPACE                                  # ... before the alignment
    for kw in (dict(logits=P + 1), dict(q=P + 1), dict(T=P + 2), dict(k=P + 2), dict(p=P + 2), dict(ua=P + 2), dict(ud=P + 2), dict(ids=P + 4),
               dict(pos=P + 4), dict(out=P + 4), dict(ws=P + 4)):
        assert call(**kw) == E_ALIGN, kw
    # the old entry validates as it did: no t_max, the single-sequence workspace
    old = lib.gptq_spec_sample_rows_f16
    assert old(None, V, P, V, R, V, P, P, P, P, P, P, P, P, P, 48, None) == E_NULL
    assert old(P, V, P, V, 1, V, P, P, P, P, P, P, P, P, P, 48, None) == E_SHAPE
    assert old(P, V, P, V, R, V, P, P, P, P, P, P, P, P, P, 47, None) == E_WORKSPACE
    assert old(P, V, P, V, R, V, P, P, P, P, P, P, P + 4, P, P, 48, None) == E_ALIGN


@functools.lru_cache(maxsize=None)
def _margins(V, with_q):
    """per row of the 16-row case: (top-p margin of the target row, of the draft row, accept margin); inf where the row has no such threshold"""
    c = X.gpu_case(V, C.FULL, with_q)
    pds, qds = X._dists(c['P'], c['ids'], c['Q'], c['T'], c['k'], c['p'])
    out = []
    for i in range(C.FULL):
        mp = S.top_p_margin(c['P'][i], c['T'][i], c['k'][i], c['p'][i]) if pds[i][0] == 'prob' else np.inf
        mq = ma = np.inf
        if i < C.FULL - 1:
            if qds[i] is not None and qds[i][0] == 'prob':
                mq = S.top_p_margin(c['Q'][i], c['T'][i], c['k'][i], c['p'][i])
            ma = X.accept_margin(pds[i], qds[i], c['ids'][i + 1], V, c['ua'][i])
        out.append((mp, mq, ma))
    return out


@pytest.mark.parametrize('with_q', [False, True], ids=['point', 'draft'])
@pytest.mark.parametrize('R', C.ROWS)
@pytest.mark.parametrize('V', C.VOCABS + (1000,))
def test_the_windows_keep_their_margins(V, R, with_q):
    m = _margins(V, with_q)
    for o in range(C.FULL - R + 1):                              # every window there is: the GPU test uses a subset
        for i in range(R):
            mp, mq, ma = m[o + i]
            assert mp >= S.MARGIN, (o, i)
            if i < R - 1:                                       # the window's last row is a bonus row: its draft row and u_accept are not used
                assert mq >= S.MARGIN and ma >= S.MARGIN, (o, i)
        w = C.window(V, R, with_q, o)
        a, emitted, flags, tokens = C.oracle(w)
        assert C.admissible(w, flags, tokens).all()
        assert len(emitted) == a + 1 and not flags[R - 1] and a == next((i for i in range(R - 1) if not flags[i]), R - 1)


def test_the_windows_cover_every_accepted_count():
    """R = 5: the twelve windows, with and without draft logits, give accepted counts 0 .. 4; offset 11 with draft logits is a full accept; greedy
    and non-finite rows are among the windows' rows"""
    R = 5
    counts = set()
    for V in (50, 1000, 32001):
        mine = {C.oracle(C.window(V, R, with_q, o))[0] for with_q in (False, True) for o in range(C.FULL - R + 1)}
        print('V %d: accepted counts %s' % (V, sorted(mine)))
        assert {0, 1, 2, R - 1} <= mine, (V, mine)
        assert C.oracle(C.window(V, R, True, 11))[0] == R - 1
        counts |= mine
    assert counts == {0, 1, 2, 3, 4}, counts
    for V in C.VOCABS:
        kinds = set()
        for w in C.batch(V, R, True, 3):
            pds, _ = X._dists(w['P'], w['ids'], w['Q'], w['T'], w['k'], w['p'])
            kinds |= {d[0] for d in pds}
        assert kinds == {'prob', 'point', 'bad'}, (V, kinds)


def test_the_batches_are_distinct_windows():
    for R in C.ROWS:
        o = C.offsets(R, 3)
        assert len(set(o)) == 3 and max(o) == C.FULL - R
    assert sorted(set(C.offsets(8, 16))) == list(range(9)) and 16 * 8 == 128
