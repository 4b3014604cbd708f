"""CPU tests of the speculative-sampling oracle (tests/spec_sample_ref.py) and of the inputs tests/test_gpu_spec_sample.py feeds the kernel: the
accept / resample rule emits exactly the target distribution, and every decision of the GPU cases keeps its margin from an edge."""
import numpy as np
import pytest
import torch

import sample_ref as S
import spec_sample_ref as X


def _perturbed(logits, seed, step=None):
    noise = torch.randn(logits.numel(), generator=torch.Generator().manual_seed(seed)) * 0.7
    if step is not None:
        noise = torch.round(noise / step) * step
    return (logits.float() + noise).half()


def _mixture(p, q):
    """sum_d q(d) [acc(d) delta_{x,d} + (1 - acc(d)) r(x) / sum r]: r does not depend on d for a draft distribution q"""
    out = np.zeros_like(p)
    rejected = 0.0
    for d in np.nonzero(q > 0)[0]:
        acc = X.accept_probability(p, q, int(d))
        out[d] += q[d] * acc
        rejected += q[d] * (1 - acc)
    r = X.residual(p, q)
    return out + (rejected * r / r.sum() if r.sum() > 0 else 0.0)


@pytest.mark.parametrize('name', [c[0] for c in S.CASES])
def test_the_rule_emits_the_target_distribution(name):
    logits, T, k, p = S.case(name)
    V = logits.numel()
    pv = S.probabilities(logits, T, k, p)
    qv = S.probabilities(_perturbed(logits, 77, 0.25 if 'ties' in name else None), T, k, p)
    assert np.abs(pv - qv).max() > 1e-3 or (pv > 0).sum() == 1     # (a draft that differs, unless one token is all top-p keeps)
    assert np.abs(_mixture(pv, qv) - pv).max() <= 1e-12
    kept = np.nonzero(pv > 0)[0]
    if V <= 1000:                                              # the same through emitted_distribution, one draft at a time
        mix = sum(qv[d] * X.emitted_distribution(pv, qv, int(d)) for d in np.nonzero(qv > 0)[0])
        assert np.abs(mix - pv).max() <= 1e-12
    # a point-mass draft emits p whatever the draft is: inside the kept set, outside it, the likeliest token
    for d in (int(kept[0]), int(kept[-1]), int(np.argmax(pv)), int(np.argmin(pv))):
        onehot = np.bincount([d], minlength=V).astype(np.float64)
        assert np.abs(X.emitted_distribution(pv, onehot, d) - pv).max() <= 1e-12, d
    # q = p: every draft from the kept set is accepted, and the mixture is p
    assert all(X.accept_probability(pv, pv, int(d)) == 1.0 for d in kept[:50])
    assert np.abs(_mixture(pv, pv) - pv).max() <= 1e-12


def test_row_decisions_follow_the_uniforms():
    logits, T, k, p = S.case('v1000-k40')
    pd = X.dist(logits, T, k, p)
    qd = X.dist(_perturbed(logits, 3), T, k, p)
    pv, qv, V = pd[1], qd[1], logits.numel()
    d = int(np.argmax(qv))
    acc = X.accept_probability(pv, qv, d)
    assert 0 < acc < 1
    assert X.row_decision(pd, qd, d, V, acc - 1e-3, 0.5) == (True, d)
    flag, tok = X.row_decision(pd, qd, d, V, acc + 1e-3, 0.5)
    assert not flag and X.residual(pv, qv)[tok] > 0
    out = int(np.argmin(pv))                                    # outside the target's kept set: never survives
    assert pv[out] == 0 and not X.row_decision(pd, qd, out, V, 0.0, 0.5)[0] and not X.row_decision(pd, None, out, V, 0.0, 0.5)[0]
    top = int(np.argmax(pv))
    assert X.row_decision(pd, None, top, V, pv[top] - 1e-3, 0.5)[0] and not X.row_decision(pd, None, top, V, pv[top] + 1e-3, 0.5)[0]
    g = X.dist(logits, 0.0, k, p)                               # greedy: accepts iff the draft is the first maximum
    assert g == ('point', int(torch.argmax(logits))) and X.row_decision(g, None, g[1], V, 0.99, 0.5) == (True, g[1])
    assert X.row_decision(g, None, (g[1] + 1) % V, V, 0.0, 0.5) == (False, g[1])
    bad = logits.clone(); bad[5] = float('nan')
    assert X.row_decision(X.dist(bad, T, k, p), None, d, V, 0.0, 0.5) == (False, 5)
    flag, tok = X.row_decision(pd, X.dist(bad, T, k, p), d, V, 0.0, 0.37)      # a NaN in the draft row: the target's plain draw
    assert not flag and tok == S.sample(logits, T, k, p, 0.37)


@pytest.mark.parametrize('with_q', [False, True], ids=['point', 'draft'])
@pytest.mark.parametrize('R', X.ROWS)
@pytest.mark.parametrize('V', X.VOCABS)
def test_gpu_cases_keep_their_margins(V, R, with_q):
    c = X.gpu_case(V, R, with_q)
    pds, qds = X._dists(c['P'], c['ids'], c['Q'], c['T'], c['k'], c['p'])
    for i in range(R):
        if pds[i][0] == 'prob':
            assert S.top_p_margin(c['P'][i], c['T'][i], c['k'][i], c['p'][i]) >= S.MARGIN, i
        if i < R - 1 and qds[i] is not None and qds[i][0] == 'prob':
            assert S.top_p_margin(c['Q'][i], c['T'][i], c['k'][i], c['p'][i]) >= S.MARGIN, i
        if i < R - 1:
            assert X.accept_margin(pds[i], qds[i], c['ids'][i + 1], V, c['ua'][i]) >= S.MARGIN, i
    kinds = [d[0] for d in pds]
    assert 'prob' in kinds and (R < 5 or ('bad' in kinds and 'point' in kinds))     # greedy and non-finite rows among the sampled ones
    a, emitted, flags, tokens = X.verify(c['P'], c['ids'], c['Q'], c['T'], c['k'], c['p'], c['ua'], c['ud'])
    assert X.admissible(flags, tokens, c['P'], c['ids'], c['Q'], c['T'], c['k'], c['p'], c['ua'], c['ud']).all()
    assert len(emitted) == a + 1 and not flags[R - 1]


@pytest.mark.parametrize('with_q', [False, True], ids=['point', 'draft'])
@pytest.mark.parametrize('name', ['v1000-k40', 'ties', 'v257-k7', 'v50'])
def test_grid_cases_keep_their_top_p_margin(name, with_q):
    logits, T, k, p = S.case(name)
    V = logits.numel()
    g = torch.Generator().manual_seed(5)
    ql = (logits.float() + torch.round(torch.randn(V, generator=g) * 0.7 / 0.25) * 0.25).half() if with_q else None
    p = X.snap_top_p_both(logits, ql, T, k, p)
    assert S.top_p_margin(logits, T, k, p) >= S.MARGIN and (ql is None or S.top_p_margin(ql, T, k, p) >= S.MARGIN)
