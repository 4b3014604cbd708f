"""The float64 oracle of gptq_spec_sample_rows_f16 (include/gptq_mi355x.h "speculative sampling"), built on sample_ref.

One verify step has R rows.  Row i of the target logits P gives p, the probabilities sample_ref.probabilities defines under the row's (T, k, p)
setting; d = ids[i + 1] is the token drafted for that place; q is the same of row i of the draft logits Q under the SAME setting, or one-hot at d
when Q is None.
  accept      row i < R - 1 accepts iff u_accept[i] q(d) < p(d); its token is d
  reject      the first id, ascending, whose running sum of r = max(p - q, 0) exceeds u_draw[i] sum(r); sum(r) = 0: the first maximal target logit
  bonus       row R - 1 never accepts and draws from p with u_draw[R - 1] (sample_ref.sample)
  greedy      p is one-hot at the first maximal logit: accepts iff d is that id, and that id is the row's token
  non-finite  a target or draft row with a NaN / +inf, or a draft row of -inf only, rejects; the token is sample_ref.sample of the target row
  prefix      a = the number of leading accepting rows among 0 .. R - 2; the step emits d_0 .. d_{a-1}, t_a
An accept decision or a draw within EPS (of the row's mass, as in sample_ref) of its edge may go either way: `admissible`.
Everything here is numpy float64 on the CPU; nothing imports the product."""
import numpy as np

import sample_ref as S

EPS = S.EPS


def _row(x):
    return x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x)


def dist(logits, T, k, p):
    """one row under one setting: ('bad', index) for a row with a NaN / +inf, ('point', index) for a greedy setting or a row of -inf only,
    else ('prob', float64 [V])"""
    logits = _row(logits)
    bad = S.first_non_finite(logits)
    if bad is not None:
        return 'bad', bad
    l = logits.astype(np.float64)
    if S.sanitise(T, k, p, 0.0, l.size)[0] or l.max() == -np.inf:
        return 'point', int(np.argmax(l))
    return 'prob', S.probabilities(logits, T, k, p)


def _case(pd, qd, d, V):
    """what rule a row falls under: ('fixed', accept, token), ('plain', p) -- reject and draw from p -- or ('ratio', p, q)"""
    d = int(d)
    inside = 0 <= d < V
    qdead = qd is not None and (qd[0] == 'bad' or (qd[0] == 'point' and pd[0] == 'prob'))
    if pd[0] == 'bad':
        return 'fixed', False, pd[1]
    if pd[0] == 'point':
        return 'fixed', bool(inside and not qdead and d == pd[1]), pd[1]
    if not inside or qdead:
        return 'plain', pd[1]
    q = qd[1] if qd is not None else np.bincount([d], minlength=V).astype(np.float64)
    return 'ratio', pd[1], q


def residual(p, q):
    return np.maximum(p - q, 0.0)


def accept_probability(p, q, d):
    """P(u q(d) < p(d)) for u uniform in [0, 1)"""
    return 1.0 if q[d] <= p[d] and p[d] > 0 else (0.0 if p[d] <= 0 else p[d] / q[d])


def emitted_distribution(p, q, d):
    """float64 [V]: the distribution of the row's token given the draft d, over uniform (u_accept, u_draw)"""
    acc = accept_probability(p, q, d)
    r = residual(p, q)
    out = np.zeros_like(p)
    out[d] = acc
    if acc < 1:
        if r.sum() > 0:
            out += (1 - acc) * r / r.sum()
        else:
            out[int(np.argmax(p))] += 1 - acc
    return out


def _draw(mass, u, fallback):
    c = np.cumsum(mass)
    if not c[-1] > 0:
        return fallback
    hit = (mass > 0) & (c > u * c[-1])
    return int(np.argmax(hit)) if hit.any() else int(np.nonzero(mass > 0)[0][-1])


def row_decision(pd, qd, d, V, ua, ud):
    """(accept, token) of one row, exactly as the semantics say; pd / qd from dist(), qd None for a point-mass draft"""
    ua, ud = S.sanitise(1.0, 0, 1.0, ua, V)[3], S.sanitise(1.0, 0, 1.0, ud, V)[3]
    c = _case(pd, qd, d, V)
    if c[0] == 'fixed':
        return c[1], c[2]
    if c[0] == 'plain':
        return False, _draw(c[1], ud, int(np.argmax(c[1])))
    p, q = c[1], c[2]
    if ua * q[d] < p[d]:
        return True, int(d)
    return False, _draw(residual(p, q), ud, int(np.argmax(p)))


def _per_row(v, R):
    return list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * R


def _dists(P, ids, Q, T, k, p):
    R = len(ids)
    T, k, p = _per_row(T, R), _per_row(k, R), _per_row(p, R)
    pds = [dist(P[i], T[i], k[i], p[i]) for i in range(R)]
    qds = [None if Q is None or i == R - 1 else dist(Q[i], T[i], k[i], p[i]) for i in range(R)]
    return pds, qds


def verify(P, ids, Q, T, k, p, ua, ud):
    """P [R, V] fp16 target logits, ids [R], Q [R - 1, V] fp16 draft logits or None, T / k / p a scalar or one per row, ua / ud [R].
    Returns (a, emitted tokens [a + 1], flags [R], tokens [R])."""
    ids = [int(x) for x in _row(ids)]
    R, V = len(ids), _row(P[0]).size
    pds, qds = _dists(P, ids, Q, T, k, p)
    flags, tokens = [], []
    for i in range(R):
        if i == R - 1:
            acc, tok = False, S.sample(P[i], _per_row(T, R)[i], _per_row(k, R)[i], _per_row(p, R)[i], ud[i])
        else:
            acc, tok = row_decision(pds[i], qds[i], ids[i + 1], V, ua[i], ud[i])
        flags.append(bool(acc))
        tokens.append(int(tok))
    a = next((i for i in range(R - 1) if not flags[i]), R - 1)
    return a, ids[1:a + 1] + [tokens[a]], flags, tokens


def admissible_draws(flags, tokens, pd, qd, d, V, uas, uds, bonus=False, eps=EPS):
    """bool [n]: may (flags[j], tokens[j]) be the record of a row (pd, qd, d) under (uas[j], uds[j])?  The sums are computed once for n draws of
    ONE row.  bonus: the last row of a step -- never accepts, draws from p."""
    flags, tokens = np.asarray(flags).astype(bool).reshape(-1), np.asarray(tokens, dtype=np.int64).reshape(-1)
    ua = np.array([S.sanitise(1.0, 0, 1.0, x, V)[3] for x in np.asarray(uas, dtype=np.float32).reshape(-1)])
    ud = np.array([S.sanitise(1.0, 0, 1.0, x, V)[3] for x in np.asarray(uds, dtype=np.float32).reshape(-1)])
    inside = (tokens >= 0) & (tokens < V)
    t = np.where(inside, tokens, 0)
    c = ('fixed', False, pd[1]) if pd[0] == 'bad' else (('fixed', False, pd[1]) if bonus and pd[0] == 'point' else
                                                       (('plain', pd[1]) if bonus else _case(pd, qd, d, V)))
    if c[0] == 'fixed':
        return inside & (flags == c[1]) & (t == c[2])

    def draw_ok(mass, support):
        cs = np.cumsum(mass)
        W = cs[-1]
        if not W > 0:
            return t == int(np.argmax(support))
        lo = np.where(t > 0, cs[t - 1], 0.0)
        return (support[t] > 0) & (lo - eps <= ud * W) & (ud * W <= cs[t] + eps)
    if c[0] == 'plain':
        return inside & ~flags & draw_ok(c[1], c[1])
    p, q = c[1], c[2]
    d = int(d)
    edge = ua * q[d] - p[d]                                # < 0: accept
    ok_acc = flags & (edge < eps) & (t == d) & (p[d] > 0)
    ok_rej = ~flags & (edge >= -eps) & draw_ok(residual(p, q), p)
    return inside & (ok_acc | ok_rej)


def admissible(flags, tokens, P, ids, Q, T, k, p, ua, ud, eps=EPS):
    """bool [R]: row i's record (flags[i], tokens[i]) is one the semantics allow within eps"""
    ids = [int(x) for x in _row(ids)]
    R, V = len(ids), _row(P[0]).size
    pds, qds = _dists(P, ids, Q, T, k, p)
    return np.array([bool(admissible_draws([flags[i]], [tokens[i]], pds[i], qds[i], ids[i + 1] if i < R - 1 else -1, V, [ua[i]], [ud[i]],
                                           bonus=i == R - 1, eps=eps)[0]) for i in range(R)])


def accept_margin(pd, qd, d, V, ua):
    """the distance of u_accept q(d) from p(d) (inf where the row does not use the ratio test)"""
    c = _case(pd, qd, d, V)
    if c[0] != 'ratio' or c[1][int(d)] == 0:                # (p(d) = 0 never survives, whatever u: no threshold)
        return np.inf
    return float(abs(S.sanitise(1.0, 0, 1.0, ua, V)[3] * c[2][int(d)] - c[1][int(d)]))


# ---- the inputs tests/test_gpu_spec_sample.py runs and tests/test_host_spec_sample.py checks the margins of ---------------------------------------
import functools

import torch

VOCABS, ROWS = (50, 257, 1000, 32001), (2, 5, 16)
NAN, INF = float('nan'), float('inf')
# (T, k, p) by vocabulary; p is snapped for the target AND the draft row before use.  32001: natural rows keep the margin only under a small top-k
# (sample_ref.CASES), the wide setting goes to plateau rows.
SETTINGS = {50: ((0.8, 0, 0.95), (1.0, 0, 0.5), (0.0, 0, 1.0), (1.3, 7, 0.8), (1.0, 0, 1.0)),
            257: ((0.8, 0, 0.95), (1.3, 7, 0.8), (0.0, 5, 0.5), (1.0, 40, 0.9), (1.0, 0, 1.0)),
            1000: ((0.8, 0, 0.95), (1.0, 40, 0.9), (0.0, 0, 1.0), (0.8, 40, 1.0), (1.0, 0, 1.0)),
            32001: ((1.0, 50, 0.9), (1.0, 2000, 0.8), (0.0, 0, 1.0), (0.7, 50, 1.0), (1.0, 50, 0.9))}


def snap_top_p_both(pl, ql, T, k, p):
    """float32 top-p inside the target row's class interval around p that also sits MARGIN inside a class of the draft row (ql None: the target's
    snap_top_p); p >= 1 (off) and greedy settings are returned as they are"""
    if p >= 1 or S.sanitise(T, k, p, 0.0, pl.numel())[0]:
        return float(p)
    if ql is None:
        return float(S.snap_top_p(pl, T, k, p))
    _, gt, ge = S.class_edges(pl, T, k)
    c = min(int(np.searchsorted(ge, p, side='right')), len(ge) - 1)
    for f in (0.5, 0.4, 0.6, 0.3, 0.7, 0.2, 0.8, 0.45, 0.55, 0.35, 0.65, 0.25, 0.75):
        x = np.float32(gt[c] + f * (ge[c] - gt[c]))
        if S.top_p_margin(pl, T, k, x) >= S.MARGIN and S.top_p_margin(ql, T, k, x) >= S.MARGIN:
            return float(x)
    raise AssertionError('no top-p with the margin in both rows')


@functools.lru_cache(maxsize=None)
def gpu_case(V, R, with_q):
    """dict(P [R, V] fp16, Q [R - 1, V] fp16 or None, ids [R], T, k, p, ua, ud: lists of R) -- ties (step 0.25) and plateaus among the rows, greedy
    among sampled settings, a NaN and a +inf row from R = 5 on, and drafts inside / outside the target's kept set, outside q's, and q = p"""
    g = torch.Generator().manual_seed(1000 * R + V + (7 if with_q else 0))
    sets = SETTINGS[V]
    P, Q, ids, T, k, p, ua, ud = [], [], [int(torch.randint(0, V, (1,), generator=g))], [], [], [], [], []
    for i in range(R):
        Ti, ki, pi = sets[i % len(sets)]
        plateau = V >= 1000 and ki == 2000 or (V == 1000 and i % 5 == 4)
        if plateau:
            pl = S.plateau(V, max(V // 10, 8), 50 + i)
        else:
            pl = S.make_logits(V, 2.5 if V > 1000 else 3.0, 100 * R + i, step=0.25 if i % 3 == 1 else None)
        kind = (0, 3, 0, 2, 1, 0, 3, 1)[i % 8]                                        # 0 inside p's kept set, 1 outside it, 2 outside q's kept set, 3 q = p
        ql = None
        if with_q and i < R - 1:
            if kind == 3:
                ql = pl.clone()
            else:
                noise = torch.randn(V, generator=g) * (0.3 if plateau else 0.7)
                ql = (pl.float() + (torch.round(noise / 0.25) * 0.25 if i % 3 == 1 else noise)).half()
        pi = snap_top_p_both(pl, ql, Ti, ki, pi)
        if i < R - 1:
            greedy = S.sanitise(Ti, ki, pi, 0.0, V)[0]
            keep_p = np.ones(V, bool) if greedy else S.kept_set(pl, Ti, ki, pi)
            keep_q = keep_p if ql is None or greedy else S.kept_set(ql, Ti, ki, pi)
            order = torch.argsort((ql if ql is not None else pl).float(), descending=True, stable=True).numpy()
            if kind == 1 and not keep_p.all():
                d = int(np.nonzero(~keep_p)[0][len(np.nonzero(~keep_p)[0]) // 2])
            elif kind == 2 and (keep_p & ~keep_q).any():
                cand = np.nonzero(keep_p & ~keep_q)[0]
                d = int(cand[np.argmax(pl.float().numpy()[cand])])          # the likeliest under p of those q dropped
            else:
                d = int(order[i % 3]) if keep_p[order[i % 3]] and not greedy else int(order[0])
            ids.append(d)
        P.append(pl); T.append(Ti); k.append(ki); p.append(pi)
        if i < R - 1:
            Q.append(ql)
        ua.append((0.05, 0.35, 0.62, 0.93)[i % 4] if i % 7 != 6 else 0.0)
        ud.append((0.11 + 0.17 * i) % 1.0)
    if R >= 5:                                                  # non-finite rows: a NaN in a target row, a +inf in another, a NaN in a draft row
        if R > 5:
            P[3] = P[3].clone(); P[3][V // 3] = NAN
            P[7] = P[7].clone(); P[7][V - 1] = INF
            if with_q:
                Q[9] = Q[9].clone(); Q[9][1] = NAN
        else:                                                   # (row 2 is the greedy one)
            P[1] = P[1].clone(); P[1][V // 3] = NAN
            P[3] = P[3].clone(); P[3][0] = INF
    Pt = torch.stack(P)
    Qt = torch.stack(Q) if with_q else None
    pds, qds = _dists(Pt, ids, Qt, T, k, p)
    for i in range(R - 1):                                      # u_accept off the thresholds
        for _ in range(100):
            if accept_margin(pds[i], qds[i], ids[i + 1], V, ua[i]) >= S.MARGIN:
                break
            ua[i] = (ua[i] + 0.013) % 1.0
    return dict(P=Pt, Q=Qt, ids=ids, T=T, k=k, p=p, ua=ua, ud=ud)
