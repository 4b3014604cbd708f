"""Shared helpers for the parity tests (test infrastructure; may use the oracle)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name)))


def golden_names(prefix):
    return sorted(f for f in os.listdir(GOLDEN) if f.startswith(prefix) and f.endswith('.npz'))


def act_order_g_idx(K, gs, rng):
    perm = rng.permutation(K)
    return (np.arange(K) // gs)[np.argsort(perm)].astype(np.int32)


def make_random_layer(bits, groupsize, K, N, act_order=False, seed=0):
    """SURVEY 8(d) synthetic distribution: uniform int32 bit patterns (every field uniform, sign
    bit exercised), scales ~ U(0.001, 0.011) fp16, trivial or act-order g_idx."""
    rng = np.random.default_rng(seed)
    gs = K if groupsize == -1 else groupsize
    G = -(-K // gs)
    qweight = rng.integers(-2**31, 2**31, size=(K // 32 * bits, N), dtype=np.int64).astype(np.int32)
    qzeros = rng.integers(-2**31, 2**31, size=(G, N // 32 * bits), dtype=np.int64).astype(np.int32)
    scales = rng.uniform(0.001, 0.011, size=(G, N)).astype(np.float16)
    g_idx = act_order_g_idx(K, gs, rng) if act_order else (np.arange(K) // gs).astype(np.int32)
    return dict(qweight=qweight, qzeros=qzeros, scales=scales, g_idx=g_idx, bits=bits, groupsize=gs)


def rel_err(a, b):
    """max|a-b| / max|b| -- the tolerance definition of SURVEY 0.6 (bar: < 1e-3)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


TOL = 1e-3


def within(name, err, tol):
    """assert err < tol; with GPTQ_TEST_ERRLOG=<file> the observed error is logged (used to set the model-level tolerances)."""
    path = os.environ.get('GPTQ_TEST_ERRLOG')
    if path:
        with open(path, 'a') as f:
            f.write('%s %.3e %.1e\n' % (name, float(err), tol))
    assert err < tol, (name, float(err), tol)


def fp16_ulp(v):
    """spacing of fp16 at |v| (elementwise; subnormal spacing 2^-24 below 2^-14)"""
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 10)


def assert_not_worse_than_reference(hip, faithful, exact, extra_ulp=1.0, name=''):
    """'more exact than the reference' as a TESTED claim: per element, the HIP result may be further from the
    float64 result than the reference-faithful oracle only by ``extra_ulp`` fp16 spacings of the value (one rounding flip), and its
    max-normalised error against the float64 result stays below the op-level bar."""
    hip, faithful, exact = (np.asarray(t, dtype=np.float64) for t in (hip, faithful, exact))
    # elements more than 2^10 times smaller than the largest output sit on cancelled sums: BOTH results carry the same fp32
    # accumulation-order noise there (~1e-6 of the partial sums), which exceeds the fp16 spacing of such a tiny value -- the slack never
    # drops below the spacing at max|exact| / 1024 (observed on the MI355X: excess of 1e-7 .. 1.4e-5 on outputs of magnitude <= 1e-3)
    # plus the accumulation-order noise itself: both kernels sum K ~ 10^3 products in fp32 (eps32 sqrt(K) ~ 2e-6 of the largest partial sums)
    # in different orders, which is an ABSOLUTE error and can exceed even a subnormal fp16 spacing on an output near zero
    mx = np.abs(exact).max()
    floor = mx * 2.0 ** -10
    slack = extra_ulp * fp16_ulp(np.maximum(np.abs(exact), floor)) + mx * 2.0 ** -16 + 1e-30   # (silu(g) * u: the noise of BOTH sums, times the other factor)
    worse = np.abs(hip - exact) - np.abs(faithful - exact) - slack
    assert worse.max() <= 0, (name, 'element further from the exact result than the reference by more than %.1f ulp' % extra_ulp, float(worse.max()))
    assert rel_err(hip, exact) < TOL, (name, rel_err(hip, exact))


# ---------------------------------------------------------------------------------------
# Off unit-scale data: realistic GPTQ layers and activations, per-row error bars, power-of-two scaling
# ---------------------------------------------------------------------------------------

FP16_MIN_NORMAL = 2.0 ** -14
FP16_MAX = 65504.0


def realistic_layer(bits, groupsize, K, N, act_order=False, sym=False, seed=0, dead_cols=4):
    """A layer quantised the way a GPTQ checkpoint is: a heavy-tailed float weight (Student-t, nu = 4) with a per-column std spread
    log-uniformly over 1e-3 .. 5e-2 and ``dead_cols`` all-zero columns, quantised per group by the project's Quantizer (min/max grid,
    perchannel) and packed field by field.  So the zero points sit near mid-range, q - z is centred, and the fp16 scales span about
    two decades within the layer.  Returns make_random_layer's dict plus the float weight ``w`` [K, N] (float32)."""
    import torch
    from quant.quantizer import Quantizer
    from oracle import oracle
    rng = np.random.default_rng(seed)
    gs = K if groupsize == -1 else groupsize
    G = -(-K // gs)
    std = np.exp(rng.uniform(np.log(1e-3), np.log(5e-2), size=N)).astype(np.float32)
    w = (rng.standard_t(4, size=(K, N)).astype(np.float32) / np.float32(np.sqrt(2.0))) * std[None, :]
    w[:, rng.choice(N, size=min(dead_cols, N), replace=False)] = 0.0
    g_idx = act_order_g_idx(K, gs, rng) if act_order else (np.arange(K) // gs).astype(np.int32)
    maxq = 2 ** bits - 1
    q = np.empty((K, N), dtype=np.int64)
    z = np.empty((G, N), dtype=np.int64)
    s = np.empty((G, N), dtype=np.float16)
    quantizer = Quantizer()
    quantizer.configure(bits, perchannel=True, sym=sym)
    for g in range(G):
        rows = np.nonzero(g_idx == g)[0]
        quantizer.find_params(torch.from_numpy(np.ascontiguousarray(w[rows].T)), weight=True)
        sg = quantizer.scale.reshape(-1).numpy().astype(np.float16)        # the checkpoint stores fp16 scales
        zg = quantizer.zero.reshape(-1).numpy().astype(np.int64)
        zg = np.clip(zg, 1, maxq)                                           # z = 0 would hit the reference's (z - 1) packing quirk
        q[rows] = np.clip(np.round(w[rows] / sg.astype(np.float32)[None, :]) + zg[None, :], 0, maxq).astype(np.int64)
        s[g], z[g] = sg, zg
    qweight = oracle.np_pack_fields_rows(q, bits)
    qzeros = oracle.np_pack_fields_cols(z - 1, bits)      # stored as z - 1 (the kernels add 1 back)
    return dict(qweight=qweight, qzeros=qzeros, scales=s, g_idx=g_idx, bits=bits, groupsize=gs, w=w)


ACTIVATION_KINDS = ('outliers', 'massive_row', 'positive', 'tiny')


def activations(kind, M, K, seed):
    """fp16 activations [M, K] shaped like a real LLaMA layer's inputs:
    'outliers'    N(0, 1) with 0.3 % fixed channels at 20 .. 100 x (the same channels in every row);
    'massive_row' ordinary rows, and row M // 2 carries one channel near 1000;
    'positive'    silu(g) * u with g ~ N(0.5, 1.5), u log-normal: the down_proj input -- mean > 0, heavy right tail;
    'tiny'        the whole tensor is about 1e-3."""
    rng = np.random.default_rng(seed)
    if kind == 'outliers':
        x = rng.standard_normal((M, K))
        ch = rng.choice(K, size=max(1, int(round(0.003 * K))), replace=False)
        x[:, ch] *= rng.uniform(20, 100, size=ch.size) * rng.choice([-1.0, 1.0], size=ch.size)
    elif kind == 'massive_row':
        x = rng.standard_normal((M, K))
        x[M // 2, rng.integers(K)] = rng.choice([-1.0, 1.0]) * rng.uniform(900, 1100)
    elif kind == 'positive':
        g = 0.5 + 1.5 * rng.standard_normal((M, K))
        u = np.exp(0.5 * rng.standard_normal((M, K)))
        x = g / (1.0 + np.exp(-g)) * u
    elif kind == 'tiny':
        x = 1e-3 * rng.standard_normal((M, K))
    else:
        raise ValueError(kind)
    return x.astype(np.float16)


def rowwise_rel_err(y, exact):
    """per row: max|y - exact| / max|exact| of that row (a row of zeros divides by 1e-30) -> float64 array [M]"""
    y = np.asarray(y, dtype=np.float64).reshape(-1, np.shape(y)[-1])
    e = np.asarray(exact, dtype=np.float64).reshape(y.shape)
    return np.abs(y - e).max(1) / np.maximum(np.abs(e).max(1), 1e-30)


def assert_rows_not_worse_than_reference(hip, faithful, exact, extra_ulp=1.0, name=''):
    """assert_not_worse_than_reference applied to every row on its own: each row is held to the op bar against ITS maximum, and
    its slack (fp16 spacing, accumulation-order noise) is that of its own largest value, not the whole array's."""
    hip, faithful, exact = (np.asarray(t, dtype=np.float64).reshape(-1, np.shape(t)[-1]) for t in (hip, faithful, exact))
    for m in range(hip.shape[0]):
        assert_not_worse_than_reference(hip[m], faithful[m], exact[m], extra_ulp=extra_ulp, name='%s row %d' % (name, m))


def pow2_scaled(L, j):
    """the layer with every scale multiplied by 2^j (exact while the scales stay fp16 normals)"""
    s = (L['scales'].astype(np.float64) * 2.0 ** j)
    assert np.all((s == 0) | ((np.abs(s) >= FP16_MIN_NORMAL) & (np.abs(s) <= FP16_MAX))), 'pow2_scaled: a scale leaves the fp16 normal range'
    out = dict(L)
    out['scales'] = s.astype(np.float16)
    return out


def fp16_normal_or_zero(v):
    """elementwise: v == 0 or 2^-14 <= |v| <= 65504 (where scaling by a power of two commutes with fp16 rounding)"""
    a = np.abs(np.asarray(v, dtype=np.float64))
    return (a == 0) | ((a >= FP16_MIN_NORMAL) & (a <= FP16_MAX))


def exact_scaling_domain(y, j, x=None, jx=0, w=None, jw=0):
    """The elements of y [M, N] where scaling by a power of two must be bit-exact: y and y * 2^j are fp16 normals ABOVE the smallest one
    (a zero output may be a flushed tiny sum, and an output of exactly 2^-14 may be a value just below it rounded up on the subnormal
    grid, which lands elsewhere on the finer grid after scaling up: neither is admitted), and every input of its row (x [M, K], before and after x * 2^jx) and every dequantised weight of its
    column (w [K, N], before and after w * 2^jw) is zero or an fp16 normal.  Inside it both fp16 roundings of the output (and every fp16
    rounding of an input or weight) commute with the scaling, and an fp32 accumulation of exact power-of-two multiples yields the exact
    multiple of the unscaled sum."""
    y = np.asarray(y, dtype=np.float64)
    a = np.abs(y)
    ok = (a > FP16_MIN_NORMAL) & (a <= FP16_MAX) & (a * 2.0 ** j > FP16_MIN_NORMAL) & (a * 2.0 ** j <= FP16_MAX)
    if x is not None:
        x = np.asarray(x, dtype=np.float64)
        ok &= (fp16_normal_or_zero(x) & fp16_normal_or_zero(x * 2.0 ** jx)).all(1)[:, None]
    if w is not None:
        w = np.asarray(w, dtype=np.float64)
        ok &= (fp16_normal_or_zero(w) & fp16_normal_or_zero(w * 2.0 ** jw)).all(0)[None, :]
    return ok


def in_domain_normal(rng, shape, lo=2.0 ** -9):
    """fp16 N(0, 1) draws with every magnitude raised to at least ``lo``: inputs that stay fp16 normals after x * 2^-5"""
    x = rng.standard_normal(shape)
    x = np.where(np.abs(x) < lo, np.copysign(lo, x), x)
    return x.astype(np.float16)


def pow2_layer(bits, groupsize, K, N, act_order=False, seed=0):
    """make_random_layer with scales ~ U(2^-9, 0.011): every dequantised weight (|q - z| >= 1 or 0) stays an fp16 normal from
    2^-5 to 2^+4 times its value"""
    L = make_random_layer(bits, groupsize, K, N, act_order=act_order, seed=seed)
    rng = np.random.default_rng(seed + 1)
    L['scales'] = rng.uniform(2.0 ** -9, 0.011, size=L['scales'].shape).astype(np.float16)
    return L


def exact_domain_case(bits, groupsize, K, N, M, nsets=1, act_order=False, seed=0, x_max=4, scale_exps=(-7, -6, -5)):
    """Data on which a quantised matmul has ONE right answer whatever the order of its fp32 sums: make_random_layer with every scale a power
    of two drawn per (group, column) from 2^scale_exps, and x integer-valued in [-x_max, x_max] as fp16.  Every product x (q - z) s -- and
    x q s, x z s, which the decode kernels sum separately -- is a multiple of the granule 2^min(scale_exps) (the bound below allows 2^-3 of
    it, the grid of a bias of eighths), so every partial sum in any order is exact in fp32 while it stays below 2^24 granules.  That is
    asserted here in float64, with the largest output below the fp16 maximum: a cap on the data, not a tolerance.
    Returns (list of nsets layers, x [M, K] fp16)."""
    from oracle import oracle
    rng = np.random.default_rng(seed + 7919)
    x = rng.integers(-x_max, x_max + 1, size=(M, K)).astype(np.float16)
    granule = 2.0 ** min(scale_exps) * 2.0 ** -3
    Ls = []
    for i in range(nsets):
        L = make_random_layer(bits, groupsize, K, N, act_order=act_order, seed=seed + i)
        L['scales'] = (2.0 ** rng.choice(np.asarray(scale_exps, dtype=np.float64), size=L['scales'].shape)).astype(np.float16)
        w = oracle.dequant(L['qweight'], L['qzeros'], L['scales'], L['g_idx'], bits, faithful=False).astype(np.float64)              # (q - z) s, exact
        zs = -oracle.dequant(np.zeros_like(L['qweight']), L['qzeros'], L['scales'], L['g_idx'], bits, faithful=False).astype(np.float64)   # z s
        assert np.all(w == np.round(w / granule) * granule)
        bound = (np.abs(x.astype(np.float64)) @ (np.abs(w + zs) + zs)).max()         # sum |x| (q + z) s >= sum |x| |q - z| s
        assert bound / granule < 2.0 ** 24, ('exact_domain_case: a partial sum may leave the exact range of fp32', bits, K, N, M, bound / granule)
        assert np.abs(x.astype(np.float64) @ w).max() < FP16_MAX
        Ls.append(L)
    return Ls, x


def rows_excess_over_reference(hip, faithful, exact, extra_ulp=1.0):
    """how far the worst row of ``hip`` is further from ``exact`` than ``faithful`` beyond assert_not_worse_than_reference's per-row
    slack, relative to that row's max|exact| (0 where every row passes that check)"""
    hip, faithful, exact = (np.asarray(t, dtype=np.float64).reshape(-1, np.shape(t)[-1]) for t in (hip, faithful, exact))
    out = 0.0
    for h, f, e in zip(hip, faithful, exact):
        mx = np.abs(e).max()
        slack = extra_ulp * fp16_ulp(np.maximum(np.abs(e), mx * 2.0 ** -10)) + mx * 2.0 ** -16 + 1e-30
        worse = (np.abs(h - e) - np.abs(f - e) - slack).max()
        out = max(out, float(worse) / max(mx, 1e-30))
    return out
