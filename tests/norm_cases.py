"""RMSNorm cases shared by the host and GPU norm tests (plain numpy, no GPU): rows whose rstd differs by decades, a norm weight that is
not ~1, and the float64 formula.  On N(0, 1) rows with a weight of ~1 a wrong eps, another weight vector or a neighbouring row's rstd
moves the result by less than the op-level bar; on these rows each of them moves it by far more (tests/test_host_norm.py measures it)."""
import numpy as np

ROW_KINDS = ('unit', 'tiny', 'embed', 'massive', 'large', 'zero', 'sub')
EPS_VALUES = (1e-6, 1e-5)


def row_kinds(K, rng):
    """fp16 rows [7, K], one per ROW_KINDS entry, in that order:
    unit     N(0, 1)
    tiny     1e-3 N(0, 1): var ~ 1e-6, the size of eps
    embed    0.02 N(0, 1): a LLaMA embedding row, the first norm's input
    massive  N(0, 1) with one channel at +1000 and another at -700 (the "massive activations" of the later layers)
    large    200 N(0, 1)
    zero     all zeros (a padded row)
    sub      2e-5 N(0, 1): fp16 subnormals"""
    x = rng.standard_normal((len(ROW_KINDS), K))
    x[1] *= 1e-3
    x[2] *= 0.02
    ch = rng.choice(K, size=min(2, K), replace=False)
    x[3, ch[0]] = 1000.0
    x[3, ch[-1]] = -700.0 if K > 1 else 1000.0
    x[4] *= 200.0
    x[5] = 0.0
    x[6] *= 2e-5
    return x.astype(np.float16)


def batch_rows(M, K, rng):
    """M rows cycling through ROW_KINDS (a fresh draw per cycle): neighbouring rows have rstd 10^2 .. 10^5 apart"""
    reps = -(-M // len(ROW_KINDS))
    return np.concatenate([row_kinds(K, rng) for _ in range(reps)])[:M]


def kind_of_row(m):
    return ROW_KINDS[m % len(ROW_KINDS)]


def norm_weight(K, rng):
    """fp16 [K]: magnitude log-uniform over 0.02 .. 4, 5 % of the entries negative, 1 % exactly 0"""
    w = np.exp(rng.uniform(np.log(0.02), np.log(4.0), size=K))
    u = rng.random(K)
    w = np.where(u < 0.05, -w, w)
    w = np.where(u >= 0.99, 0.0, w)
    return w.astype(np.float16)


def exact_rmsnorm(x, w, eps):
    """x w / sqrt(mean(x^2) + float32(eps)) in float64 (eps is the float32 the kernels receive)"""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    var = (x * x).mean(-1, keepdims=True)
    return x * w / np.sqrt(var + np.float64(np.float32(eps)))


# the formulas a kernel could compute instead without any unit-scale test noticing (float64, same signature)
def rmsnorm_eps_dropped(x, w, eps):
    x = np.asarray(x, dtype=np.float64)
    var = (x * x).mean(-1, keepdims=True)
    return x * np.asarray(w, dtype=np.float64) / np.sqrt(np.maximum(var, 1e-300))


def rmsnorm_eps_outside_sqrt(x, w, eps):
    x = np.asarray(x, dtype=np.float64)
    var = (x * x).mean(-1, keepdims=True)
    return x * np.asarray(w, dtype=np.float64) / (np.sqrt(var) + np.float64(np.float32(eps)))


def rmsnorm_eps_over_n(x, w, eps):
    x = np.asarray(x, dtype=np.float64)
    var = (x * x).mean(-1, keepdims=True)
    return x * np.asarray(w, dtype=np.float64) / np.sqrt(var + np.float64(np.float32(eps)) / x.shape[-1])


WRONG_FORMULAS = (rmsnorm_eps_dropped, rmsnorm_eps_outside_sqrt, rmsnorm_eps_over_n)


def exact_linear(xn64, L):
    """float64 product of normalised rows [M, K] (float64, unrounded) with the layer's dequantised weight (never rounded to fp16)"""
    from oracle import oracle
    W = np.asarray(oracle.np_dequant(L['qweight'], L['qzeros'], L['scales'], L['g_idx'], L['bits'], faithful=False), dtype=np.float64)
    return np.asarray(xn64, dtype=np.float64) @ W


def exact_silu_pair(xn64, A, B):
    g, u = exact_linear(xn64, A), exact_linear(xn64, B)
    return g / (1.0 + np.exp(-g)) * u


def layer_sets(L):
    return (L['qweight'], L['scales'], L['qzeros'], L['g_idx'])


def faithful_forward(x, Ls, nw, eps, residual=None):
    """the oracle composition: fp16(rmsnorm) -> matmul248 or the SiLU pair -> fp16(+ residual): the module chain's roundings"""
    from oracle import oracle
    xn = oracle.rmsnorm(x, nw, eps)
    bits = Ls[0]['bits']
    y = oracle.matmul248(xn, *layer_sets(Ls[0]), bits) if len(Ls) == 1 else oracle.fused_mlp(xn, layer_sets(Ls[0]), layer_sets(Ls[1]), bits)
    if residual is not None:
        y = (y.astype(np.float32) + residual.astype(np.float32)).astype(np.float16)
    return y


def exact_forward(x, Ls, nw, eps):
    xn = exact_rmsnorm(x, nw, eps)
    return exact_linear(xn, Ls[0]) if len(Ls) == 1 else exact_silu_pair(xn, Ls[0], Ls[1])


SILU_ROW_FLOOR = 2.0 ** -10


def silu_rows_kept(exact):
    """rows of a SiLU-pair result that carry a per-row bar: float64 maximum >= 2^-10.  silu(g) u is quadratic in the row's scale: below
    that maximum most of the row sits on the fp16 subnormal grid (spacing 2^-24, absolute), which no longer shrinks with the row."""
    return np.abs(np.asarray(exact, dtype=np.float64)).max(-1) >= SILU_ROW_FLOOR
