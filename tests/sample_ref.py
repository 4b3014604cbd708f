"""The float64 oracle of gptq_sample_rows_f16 (include/gptq_mi355x.h "sampling") and the inputs its tests share.

Per row, with l_i the fp16 logits and T, k, p, u the row's (float32 / int32) parameters:
  sanitising  T not finite or <= 0: greedy (the first maximal logit).  k <= 0 or k >= vocab: top-k off.  p NaN or >= 1: top-p off; p <= 0 is the
              smallest positive float.  u is clamped into [0, 1), NaN becomes 0.
  classes     tokens are tied iff their logits compare equal (-0 == +0); a class is kept or dropped whole
  weights     w_i = exp((l_i - l_max) / T); -inf weighs 0
  top-k       keeps every logit >= the k-th largest (all ties)
  top-p       on what top-k kept (mass Z): token i stays iff the kept mass with a strictly larger logit is < p Z
  draw        W = mass of the kept set, c_j its running sum in ascending id: the first kept id with c_j > u W, else the last kept id
  non-finite  a row with a NaN or +inf: the index of the first such element
Everything here is numpy float64 on the CPU; nothing imports the product."""
import numpy as np
import torch

EPS = 1e-5          # the kernel's bar: every mass within EPS of the row's mass of the float64 value


def make_logits(V, sigma, seed, step=None):
    """[V] fp16 (torch, CPU): randn * sigma, optionally rounded to multiples of `step` (ties)"""
    x = torch.randn(V, generator=torch.Generator().manual_seed(seed)) * sigma
    if step is not None:
        x = torch.round(x / step) * step
    return x.half()


def plateau(V, n, seed):
    """[V] fp16: -20 everywhere except n random positions that hold randn * 0.3 -- thousands of tokens of comparable mass"""
    g = torch.Generator().manual_seed(seed)
    x = torch.full((V,), -20.0)
    idx = torch.randperm(V, generator=g)[:n]
    x[idx] = torch.randn(n, generator=g) * 0.3
    return x.half()


def _f64(logits):
    if torch.is_tensor(logits):
        logits = logits.detach().cpu().numpy()
    assert logits.dtype == np.float16 and logits.ndim == 1
    return logits.astype(np.float64)


def sanitise(T, k, p, u, V):
    """(greedy, k or 0, p or None, u) as the kernel reads the row's raw parameters"""
    T, p, u = np.float32(T), np.float32(p), np.float32(u)
    greedy = not (np.isfinite(T) and T > 0)
    k = int(k)
    k = k if 0 < k < V else 0
    if np.isnan(p) or p >= 1:
        p = None
    else:
        p = np.float64(p) if p > 0 else np.float64(np.finfo(np.float32).smallest_subnormal)
    if np.isnan(u) or u < 0:
        u = np.float32(0)
    elif u >= 1:
        u = np.nextafter(np.float32(1), np.float32(0))
    return greedy, k, p, np.float64(u)


def first_non_finite(logits):
    l = _f64(logits)
    bad = np.isnan(l) | (l == np.inf)
    return int(np.argmax(bad)) if bad.any() else None


def weights(logits, T):
    l = _f64(logits)
    with np.errstate(over='ignore', invalid='ignore'):
        return np.exp((l - l.max()) / np.float64(np.float32(T)))


def class_edges(logits, T, k):
    """the classes top-k keeps, by descending logit: (values, S_gt / Z, S_ge / Z) -- class c stays under top-p iff S_gt[c] / Z < p"""
    l, w = _f64(logits), weights(logits, T)
    _, k, _, _ = sanitise(T, k, 1.0, 0.0, l.size)
    keep = l >= np.sort(l)[::-1][k - 1] if k else np.ones(l.size, bool)
    vals, inv = np.unique(l[keep], return_inverse=True)
    vals, mass = vals[::-1], np.bincount(inv.reshape(-1), weights=w[keep], minlength=vals.size)[::-1]
    Z = mass.sum()
    ge = np.cumsum(mass)
    return vals, (ge - mass) / Z, ge / Z


def kept_set(logits, T, k, p):
    """bool [V]: the tokens that survive top-k and top-p (finite-or--inf rows, T > 0)"""
    l = _f64(logits)
    _, _, p, _ = sanitise(T, k, p, 0.0, l.size)
    vals, gt, _ = class_edges(logits, T, k)
    stay = vals if p is None else vals[gt < p]
    return np.isin(l, stay)


def sample(logits, T, k, p, u):
    """the id the semantics draw"""
    bad = first_non_finite(logits)
    if bad is not None:
        return bad
    l = _f64(logits)
    greedy, _, _, u = sanitise(T, k, p, u, l.size)
    if greedy:
        return int(np.argmax(l))
    keep = kept_set(logits, T, k, p)
    c = np.cumsum(np.where(keep, weights(logits, T), 0.0))
    hit = keep & (c > u * c[-1])
    return int(np.argmax(hit)) if hit.any() else int(np.nonzero(keep)[0][-1])


def probabilities(logits, T, k, p):
    """float64 [V]: the probability of every token under the semantics (0 outside the kept set)"""
    w = np.where(kept_set(logits, T, k, p), weights(logits, T), 0.0)
    return w / w.sum()


def snap_top_p(logits, T, k, p):
    """float32: the midpoint of the class interval [S_gt / Z, S_ge / Z) that contains p, so that the top-p decision sits in the middle of a class and not
    on an edge; p >= 1 (off) is returned as it is"""
    if p >= 1:
        return np.float32(p)
    _, gt, ge = class_edges(logits, T, k)
    c = int(np.searchsorted(ge, p, side='right'))           # the first class with S_ge / Z > p
    c = min(c, len(ge) - 1)
    return np.float32((gt[c] + ge[c]) / 2)


def top_p_margin(logits, T, k, p):
    """distance of p Z to the nearest class edge, as a fraction of Z (inf with top-p off)"""
    _, _, p64, _ = sanitise(T, k, p, 0.0, _f64(logits).size)
    if p64 is None:
        return np.inf
    _, gt, ge = class_edges(logits, T, k)
    return float(np.abs(np.concatenate([gt, ge]) - p64).min())


def admissible_rows(tokens, logits, T, k, p, us, eps=EPS):
    """bool [n]: admissible(tokens[j], logits, T, k, p, us[j]) for n draws from ONE row under ONE (sampling) setting, the sums computed once"""
    tokens, l = np.asarray(tokens, dtype=np.int64), _f64(logits)
    inside = (tokens >= 0) & (tokens < l.size)
    t = np.where(inside, tokens, 0)
    bad = first_non_finite(logits)
    if bad is not None:
        return inside & (t == bad)
    if sanitise(T, k, p, 0.0, l.size)[0]:
        return inside & (t == int(np.argmax(l)))
    u = np.array([sanitise(T, k, p, x, l.size)[3] for x in np.asarray(us, dtype=np.float32).reshape(-1)])
    keep = kept_set(logits, T, k, p)
    c = np.cumsum(np.where(keep, weights(logits, T), 0.0))
    W = c[-1]
    lo = np.where(t > 0, c[t - 1], 0.0)
    return inside & keep[t] & (lo - eps * W <= u * W) & (u * W <= c[t] + eps * W)


def admissible(token, logits, T, k, p, u, eps=EPS):
    """True iff `token` is a draw the semantics allow within eps: the documented index for a non-finite or greedy row; otherwise a member of the
    float64 kept set whose interval [c_{t-1}, c_t] of the running kept mass, widened by eps W on both sides, holds u W.  A draw within eps of an edge
    may go either way."""
    return bool(admissible_rows([token], logits, T, k, p, [u], eps)[0])


# every (input, T, k, p) of tests/test_gpu_sample.py's whole-CDF test; p is snapped (snap_top_p) before use and tests/test_host_sample.py asserts the
# margins on the CPU.  The wide cases are plateaus: a natural wide distribution has boundary classes of mass ~2e-5 and cannot keep the margin.
CASES = (
    ('v1000', lambda: make_logits(1000, 3.0, 1), 0.8, 0, 0.95),
    ('v1000-k40', lambda: make_logits(1000, 3.0, 1), 1.0, 40, 0.9),
    ('v32001-k50', lambda: make_logits(32001, 2.5, 2), 1.0, 50, 0.9),
    ('v32000', lambda: make_logits(32000, 4.0, 3), 0.7, 0, 0.9),
    ('ties', lambda: make_logits(1000, 3.0, 4, step=0.25), 0.8, 0, 0.9),
    ('ties-k40', lambda: make_logits(1000, 3.0, 4, step=0.25), 0.8, 40, 1.0),
    ('plateau', lambda: plateau(32001, 3000, 7), 1.0, 0, 0.5),
    ('plateau-k2000', lambda: plateau(32001, 3000, 7), 1.0, 2000, 0.8),
    ('v257-k7', lambda: make_logits(257, 3.0, 6), 1.3, 7, 0.8),
    ('v50', lambda: make_logits(50, 3.0, 5), 1.0, 0, 0.5),
)
MARGIN = 1e-4       # of Z: ten times the kernel's bar


def case(name):
    """(logits fp16 [V], T, k, snapped p) of the named case"""
    for n, build, T, k, p in CASES:
        if n == name:
            logits = build()
            return logits, T, k, float(snap_top_p(logits, T, k, p))
    raise KeyError(name)
