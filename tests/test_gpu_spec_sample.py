"""GPU tests of gptq_spec_sample_rows_f16 (csrc/spec_sample.hip) through the C ABI.  The oracle is the float64 restatement of the semantics in
tests/spec_sample_ref.py; its `admissible` lets an accept decision or a draw within 1e-5 of the row's mass of its edge go either way, and
tests/test_host_spec_sample.py asserts on the CPU that every top-p decision and every accept threshold of the inputs used here (spec_sample_ref.gpu_case)
sits at least ten times that far from an edge -- so the accept flags, and with them the prefix, must be the oracle's exactly."""
import numpy as np
import pytest
import torch

import sample_ref as S
import spec_sample_ref as X
from quant import _native

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(values, dtype):
    return torch.tensor(values, dtype=dtype).to(DEV)


def _odd(t):
    """the rows of t in a buffer whose rows are 2-byte aligned only (an odd leading dimension, an odd offset)"""
    R, V = t.shape
    ld = V + 1 if V % 2 == 0 else V + 2
    buf = torch.full((R * ld + 1,), float('nan'), dtype=torch.float16, device=DEV)      # a NaN the kernel read would decide the row
    view = buf[1:].view(R, ld)[:, :V]
    view.copy_(t.to(DEV))
    assert view.data_ptr() % 4 == 2 and (view.stride(0) * 2) % 4 == 2
    return view


def _op(P, Q, ids, T, k, p, ua, ud, pos=100, calls=1, rc_only=False, override=None):
    """gptq_spec_sample_rows_f16 on device views P [R, V], Q [R - 1, V] or None; returns (out [R + 1], pos, flags [R], tokens [R]) as numpy"""
    lib = _native.lib()
    R, V = P.shape
    a = dict(ids=_dev(list(ids), torch.int64), T=_dev(list(T), torch.float32), k=_dev(list(k), torch.int32), p=_dev(list(p), torch.float32),
             ua=ua if torch.is_tensor(ua) else _dev(list(ua), torch.float32), ud=ud if torch.is_tensor(ud) else _dev(list(ud), torch.float32),
             pos=_dev([pos], torch.int64), out=torch.full((R + 1,), -1, dtype=torch.int64, device=DEV),
             ws=torch.zeros(lib.gptq_spec_sample_workspace_bytes(R) // 8, dtype=torch.int64, device=DEV))
    ptr = {n: t.data_ptr() for n, t in a.items()}
    ptr.update(P=P.data_ptr(), Q=Q.data_ptr() if Q is not None else None, ld=P.stride(0), ldq=Q.stride(0) if Q is not None else 0, rows=R, vocab=V,
               ws_bytes=a['ws'].numel() * 8)
    ptr.update(override or {})
    seen = []
    for _ in range(calls):
        rc = lib.gptq_spec_sample_rows_f16(ptr['P'], ptr['ld'], ptr['Q'], ptr['ldq'], ptr['rows'], ptr['vocab'], ptr['ids'], ptr['T'], ptr['k'],
                                           ptr['p'], ptr['ua'], ptr['ud'], ptr['pos'], ptr['out'], ptr['ws'], ptr['ws_bytes'],
                                           _native.stream_ptr(torch.device(DEV)))
        if rc_only:
            return rc
        assert rc == 0, rc
        seen.append(torch.cat([a['out'], a['pos'], a['ws']]).clone())
    first = seen[0].cpu().numpy()
    for s in seen[1:]:                                         # the ticket word is back at 0 and the same inputs give the same bits
        s = s.cpu().numpy()
        assert np.array_equal(s[:R + 1], first[:R + 1]) and np.array_equal(s[R + 2:], first[R + 2:])
    assert first[R + 2] == 0
    rec = first[R + 3:]
    last = seen[-1].cpu().numpy()
    return first[:R + 1], int(last[R + 1]), (rec >> 32).astype(bool), (rec & 0xFFFFFFFF).astype(np.int64)


def _sample_op(row, T, k, p, u):
    out = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    u, T, k, p = _dev([u], torch.float32), _dev([T], torch.float32), _dev([k], torch.int32), _dev([p], torch.float32)
    rc = _native.lib().gptq_sample_rows_f16(row.data_ptr(), row.shape[0], 1, row.shape[0], u.data_ptr(), T.data_ptr(), k.data_ptr(), p.data_ptr(),
                                            out.data_ptr(), _native.stream_ptr(torch.device(DEV)))
    assert rc == 0, rc
    return int(out[0])


@pytest.mark.parametrize('with_q', [False, True], ids=['point', 'draft'])
@pytest.mark.parametrize('R', X.ROWS)
@pytest.mark.parametrize('V', X.VOCABS)
def test_rows_against_the_oracle(V, R, with_q):
    c = X.gpu_case(V, R, with_q)
    P, Q = _odd(c['P']), _odd(c['Q']) if with_q else None
    CALLS = 50
    out, pos, flags, tokens = _op(P, Q, c['ids'], c['T'], c['k'], c['p'], c['ua'], c['ud'], pos=100, calls=CALLS)
    a, emitted, want_flags, want_tokens = X.verify(c['P'], c['ids'], c['Q'], c['T'], c['k'], c['p'], c['ua'], c['ud'])
    ok = X.admissible(flags, tokens, c['P'], c['ids'], c['Q'], c['T'], c['k'], c['p'], c['ua'], c['ud'])
    print('V %d R %d: flags %s (oracle %s), tokens %s (oracle %s), out %s' % (V, R, flags.astype(int).tolist(), [int(f) for f in want_flags],
                                                                            tokens.tolist(), want_tokens, out.tolist()))
    assert ok.all(), (np.nonzero(~ok)[0], flags, tokens, want_flags, want_tokens)
    assert flags.tolist() == want_flags                       # (every threshold has its margin)
    assert ((tokens >= 0) & (tokens < V)).all() and ((out[1:] >= 0) & (out[1:] < V)).all()
    # the prefix: out = [a, d_0 .. d_{a-1}, t_a, ...], pos advanced by a + 1 per call
    assert int(out[0]) == a and out[1:a + 1].tolist() == c['ids'][1:a + 1] and int(out[a + 1]) == int(tokens[a])
    assert pos == 100 + CALLS * (a + 1)
    if tokens.tolist() == want_tokens:
        assert out[1:a + 2].tolist() == emitted
    # the bonus row is gptq_sample_rows_f16's draw, to the bit
    row = P[R - 1].contiguous()
    assert int(tokens[R - 1]) == _sample_op(row, c['T'][R - 1], c['k'][R - 1], c['p'][R - 1], c['ud'][R - 1])
    assert not flags[R - 1]


@pytest.mark.parametrize('with_q', [False, True], ids=['point', 'draft'])
@pytest.mark.parametrize('name', ['v1000-k40', 'ties', 'v257-k7', 'v50'])
def test_grid_of_uniforms_reproduces_the_distribution(name, with_q):
    """64 x 64 (u_accept, u_draw) as 4096 rows of ONE input (+ the bonus row).  A point-mass draft d emits p whatever d is; with draft logits the rows
    emit spec_sample_ref.emitted_distribution(p, q, d), whose q-mixture tests/test_host_spec_sample.py shows to be p."""
    logits, T, k, p = S.case(name)
    V, G = logits.numel(), 64
    N = G * G
    g = torch.Generator().manual_seed(5)
    ql = (logits.float() + torch.round(torch.randn(V, generator=g) * 0.7 / 0.25) * 0.25).half() if with_q else None
    p = X.snap_top_p_both(logits, ql, T, k, p)
    pv = S.probabilities(logits, T, k, p)
    qv = S.probabilities(ql, T, k, p) if with_q else None
    order = np.argsort(-(qv if with_q else pv), kind='stable')
    d = int(order[1])                                          # the second likeliest draft: p(d) / q(d) off 0 and 1 in most cases
    if not with_q:
        qv = np.bincount([d], minlength=V).astype(np.float64)
    strat = (torch.arange(G, dtype=torch.float64) + 0.5).div(G).float()
    ua = torch.cat([strat.repeat_interleave(G), torch.zeros(1)]).to(DEV)
    ud = torch.cat([strat.repeat(G), torch.full((1,), 0.5)]).to(DEV)
    P = logits.to(DEV)[None].expand(N + 1, V).contiguous()
    Q = ql.to(DEV)[None].expand(N, V).contiguous() if with_q else None
    out, pos, flags, tokens = _op(P, Q, [0] + [d] * N, [T] * (N + 1), [k] * (N + 1), [p] * (N + 1), ua, ud, pos=7)
    pd, qd = ('prob', pv), (('prob', qv) if with_q else None)
    ok = X.admissible_draws(flags[:N], tokens[:N], pd, qd, d, V, ua[:N].cpu().numpy(), ud[:N].cpu().numpy())
    assert ok.all(), (name, int((~ok).sum()), np.nonzero(~ok)[0][:8])
    assert (tokens[:N][flags[:N]] == d).all()
    want = X.emitted_distribution(pv, qv, d)
    if not with_q:
        assert np.abs(want - pv).max() < 1e-12                 # a point-mass draft emits p itself
    count = np.bincount(tokens[:N], minlength=V)
    # the grid's resolution, per token.  A of the G u_accept strata accept, |A - G acc| <= 1 + da; each accepting stratum gives d its G rows.  In
    # each rejecting stratum token t is drawn n_t times, |n_t - G r_t / sum(r)| <= 1 + dr.  EPS moves an edge by at most EPS / q(d), EPS / sum(r)
    # of the unit interval.  So |count_t - N e_t| <= G (1 + dr) + (1 + da) G r_t / sum(r) for t != d, and G (1 + da) more for d.
    acc, r = X.accept_probability(pv, qv, d), X.residual(pv, qv)
    rs = r.sum()
    da, dr = G * X.EPS / max(qv[d], 1e-3), 2 * G * X.EPS / max(rs, 1e-3)
    bar = G * (1 + dr) + (1 + da) * G * (r / rs if rs > 0 else (np.arange(V) == int(np.argmax(pv))))
    bar[d] += G * (1 + da)
    excess = np.abs(count - N * want) - bar
    print('%s: acc %.4f, sum r %.4f, accepted %d of %d, worst |count - N e_t| - bar_t = %.1f (bar %.1f .. %.1f)' % (
        name, acc, rs, int(flags[:N].sum()), N, excess.max(), bar.min(), bar.max()))
    assert (excess <= 0).all()
    assert (count[(pv == 0)] == 0).all()
    a = int(np.argmin(flags[:N])) if not flags[:N].all() else N
    assert int(out[0]) == a and pos == 7 + a + 1 and int(out[a + 1]) == int(tokens[a])


def test_error_codes():
    c = X.gpu_case(50, 5, True)
    P, Q = c['P'].to(DEV), c['Q'].to(DEV)
    args = (P, Q, c['ids'], c['T'], c['k'], c['p'], c['ua'], c['ud'])
    assert _op(*args, rc_only=True) == 0
    for name in ('P', 'ids', 'T', 'k', 'p', 'ua', 'ud', 'pos', 'out', 'ws'):
        assert _op(*args, rc_only=True, override={name: None}) == -4, name                      # GPTQ_E_NULL
    assert _op(*args, rc_only=True, override=dict(Q=None)) == 0                                          # (no draft logits is a mode, not an error)
    for bad in (dict(rows=1), dict(rows=0), dict(vocab=0), dict(ld=49), dict(ldq=49)):
        assert _op(*args, rc_only=True, override=bad) == -2, bad                                 # GPTQ_E_SHAPE
    assert _op(*args, rc_only=True, override=dict(ws_bytes=5 * 8)) == -5                                 # GPTQ_E_WORKSPACE
    for name, base in (('P', P), ('Q', Q)):
        assert _op(*args, rc_only=True, override={name: base.data_ptr() + 1}) == -3, name      # GPTQ_E_ALIGN
    t = torch.zeros(8, dtype=torch.int64, device=DEV)
    for name, off in (('T', 2), ('k', 2), ('p', 2), ('ua', 2), ('ud', 2), ('ids', 4), ('pos', 4), ('out', 4), ('ws', 4)):
        assert _op(*args, rc_only=True, override={name: t.data_ptr() + off}) == -3, name
    assert _native.lib().gptq_spec_sample_workspace_bytes(5) == 48
