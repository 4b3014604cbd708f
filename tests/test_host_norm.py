"""The RMSNorm cases of tests/norm_cases.py, checked on the references alone (CPU): the fp32 oracle against the float64 formula, how
far the plausible WRONG formulas sit from the right one on these rows (the reason the rows exist), and the composed reference of the
fused-norm tests against the float64 product."""
import numpy as np
import pytest

from oracle import oracle
from util import TOL, fp16_ulp, make_random_layer, rowwise_rel_err
import norm_cases as NC


@pytest.mark.parametrize('eps', NC.EPS_VALUES)
@pytest.mark.parametrize('K', [256, 4096, 11008])
def test_oracle_rmsnorm_is_the_float64_formula_rounded_once(K, eps):
    """fp32 arithmetic + one fp16 rounding: every element within 0.55 fp16 ulp of the float64 result (observed maximum 0.505)"""
    rng = np.random.default_rng(K)
    x, w = NC.row_kinds(K, rng), NC.norm_weight(K, rng)
    assert (w == 0).any() and (w < 0).any() and np.abs(w).max() > 2 and np.abs(w[w != 0]).min() < 0.05
    got = oracle.rmsnorm(x, w, eps).astype(np.float64)
    exact = NC.exact_rmsnorm(x, w, eps)
    ulps = np.abs(got - exact) / fp16_ulp(exact)
    print('K=%d eps=%g max ulp %.3f' % (K, eps, ulps.max()))
    assert ulps.max() <= 0.55, (ulps.max(), np.unravel_index(ulps.argmax(), ulps.shape))
    assert not got[NC.ROW_KINDS.index('zero')].any()


@pytest.mark.parametrize('K', [256, 4096, 11008])
def test_wrong_formulas_are_far_from_the_right_one(K):
    """eps dropped, eps outside the square root, eps / N: each more than 10 x the op bar from the right result on the `tiny` rows (both
    eps) and on the `embed` row at eps = 1e-5 -- and invisible on the `unit` row, which is why unit-scale tests cannot see eps"""
    rng = np.random.default_rng(K)
    x, w = NC.row_kinds(K, rng), NC.norm_weight(K, rng)
    tiny, embed, unit = (NC.ROW_KINDS.index(k) for k in ('tiny', 'embed', 'unit'))
    for eps in NC.EPS_VALUES:
        right = NC.exact_rmsnorm(x, w, eps)
        for f in NC.WRONG_FORMULAS:
            d = rowwise_rel_err(f(x, w, eps), right)
            print('K=%d eps=%g %s: tiny %.3g embed %.3g unit %.3g' % (K, eps, f.__name__, d[tiny], d[embed], d[unit]))
            assert d[tiny] > 10 * TOL, (f.__name__, eps, d[tiny])
            if eps == 1e-5:
                assert d[embed] > 10 * TOL, (f.__name__, d[embed])
            assert d[unit] < TOL / 10


def test_rows_of_a_batch_are_decades_apart():
    x = NC.batch_rows(17, 256, np.random.default_rng(0)).astype(np.float64)
    assert x.shape == (17, 256)
    rms = np.sqrt((x * x).mean(1))
    assert [NC.kind_of_row(m) for m in (0, 6, 7, 16)] == ['unit', 'sub', 'unit', 'embed']
    rstd = 1.0 / np.sqrt(rms ** 2 + 1e-6)
    ratios = [max(a, b) / min(a, b) for a, b in zip(rstd[:-1], rstd[1:])]
    # unit | tiny | embed | massive | large | zero | sub: rstd 1, 700, 50, 0.013, 0.005, 1000, 1000 -- a neighbour's rstd is wrong by
    # x 2.6 at the least (massive -> large), by x 14 .. 10^5 elsewhere; zero -> sub share theirs (eps alone sets it)
    assert rstd.max() / rstd.min() > 1e5 and sum(r > 10 for r in ratios) >= 9 and sum(r < 2 for r in ratios) == 2, ratios


COMPOSED = [(256, 256, 128), (1056, 288, 32)]


@pytest.mark.parametrize('eps', NC.EPS_VALUES)
@pytest.mark.parametrize('bits', [2, 3, 4, 8])
@pytest.mark.parametrize('K,N,gs', COMPOSED)
def test_composed_reference_against_float64(K, N, gs, bits, eps):
    """oracle.matmul248(oracle.rmsnorm(x)) and oracle.fused_mlp(oracle.rmsnorm(x)) -- the faithful reference of the fused-norm GPU tests
    -- against the float64 product of the UNROUNDED float64 norm, per row.  The reference rounds the normalised x, the dequantised weight
    and the output to fp16 (2^-11 each): on the `massive` row ONE product dominates every output, so the three do not average out and
    the row may sit up to 3 x 2^-11 = 1.46e-3 from float64 (observed 1.04e-3 there, <= 6.6e-4 on every other row).  The SiLU pair does
    that for g and for u (d silu(g) g / silu(g) <= 1.1 .. 2 for g >= 0) and rounds the product: 2 x 3 x 2^-11 x 1.5 + 2^-11 = 4.9e-3
    bounds it; observed <= 1.9e-3."""
    rng = np.random.default_rng(K + bits)
    x, w = NC.row_kinds(K, rng), NC.norm_weight(K, rng)
    A, B = make_random_layer(bits, gs, K, N, seed=bits), make_random_layer(bits, gs, K, N, seed=bits + 10)
    zero = NC.ROW_KINDS.index('zero')
    single = rowwise_rel_err(NC.faithful_forward(x, [A], w, eps), NC.exact_forward(x, [A], w, eps))
    print('single', single)
    assert single[zero] == 0 and single.max() < 3 * 2.0 ** -11, single
    exact = NC.exact_forward(x, [A, B], w, eps)
    keep = NC.silu_rows_kept(exact)
    dropped = {NC.ROW_KINDS[m] for m in np.nonzero(~keep)[0]} - {'zero'}    # (the zero row is held to exact zeros instead)
    assert dropped <= {'sub'}, dropped                                       # the filter may drop the subnormal row and nothing else
    pair_y = NC.faithful_forward(x, [A, B], w, eps)
    pair = rowwise_rel_err(pair_y[keep], exact[keep])
    print('pair', pair, sorted(dropped))
    assert pair.max() < 10 * 2.0 ** -11, pair
    assert not pair_y[zero].any()
