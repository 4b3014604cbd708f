"""RMSNorm on rows that can see eps, the norm weight and the row's own rstd (tests/norm_cases.py): the stand-alone kernels of
csrc/elementwise.hip -- every vector instance on both sides of its boundary, the scalar kernel, strided and misaligned layouts --
against the float64 formula, and every entry that fuses the norm into a matvec against the oracle composition, per row.
Observed per-row maxima on the MI355X (bars 1e-3 single, 1.5e-3 with a residual, 2e-3 layer_decode pair): row-wave 8.8e-4, act-order row-wave
6.5e-4 / pair 6.0e-4, stripe matvec 8.6e-4, layer_decode 9.0e-4 / residual 1.3e-3 / pair 1.6e-3, dense head 4.5e-4.  With `+ eps` taken out
of every norm in csrc/ each test below fails."""
import functools

import numpy as np
import pytest
import torch

import quant
from quant import quant_linear as QL
from quant import _native
from quant.layer import prepared
from oracle import oracle
from util import TOL, make_random_layer, rowwise_rel_err, assert_rows_not_worse_than_reference
import norm_cases as NC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ZERO = NC.ROW_KINDS.index('zero')
E_VARIANT = -6


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    return _native.stream_ptr(torch.device(DEV))


@functools.lru_cache(maxsize=None)
def norm_case(N, seed=0):
    """(x fp16 [7, N], one row per kind; w fp16 [N]) -- drawn once per width, shared and never modified"""
    rng = np.random.default_rng(1000 + N + seed)
    x, w = NC.row_kinds(N, rng), NC.norm_weight(N, rng)
    x.setflags(write=False)
    w.setflags(write=False)
    return x, w


def check_norm(y, x, w, eps, name):
    y = np.asarray(y)
    assert np.isfinite(y.astype(np.float32)).all(), name
    assert_rows_not_worse_than_reference(y, oracle.rmsnorm(x, w, eps), NC.exact_rmsnorm(x, w, eps), extra_ulp=1, name=name)
    assert not (y[ZERO] != 0).any(), name                      # numerically zero (-0 allowed)


# ---------------------------------------------------------------------------------------
# the stand-alone norm
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('eps', NC.EPS_VALUES)
@pytest.mark.parametrize('N', [8, 264, 2048, 2056, 4096, 4104, 8192, 8200, 16384, 16392, 32768])
def test_rmsnorm_vector_kernel_every_instance(N, eps):
    """rmsnorm_kernel<1 | 2 | 4 | 8 | 16>: N / 8 <= 256, 512, 1024, 2048, 4096 -- the last width of an instance and the first of the next"""
    x, w = norm_case(N)
    y = quant.triton_norm.rms_norm(dev(x), dev(w), eps)
    torch.cuda.synchronize()
    check_norm(y.cpu().numpy(), x, w, eps, 'vector N=%d eps=%g' % (N, eps))


@pytest.mark.parametrize('eps', NC.EPS_VALUES)
@pytest.mark.parametrize('N', [1, 7, 100, 4100, 32767])
def test_rmsnorm_scalar_kernel_odd_widths(N, eps):
    """rmsnorm_scalar_kernel: N % 8 != 0"""
    x, w = norm_case(N)
    y = quant.triton_norm.rms_norm(dev(x), dev(w), eps)
    torch.cuda.synchronize()
    check_norm(y.cpu().numpy(), x, w, eps, 'scalar N=%d eps=%g' % (N, eps))


@pytest.mark.parametrize('eps', NC.EPS_VALUES)
@pytest.mark.parametrize('layout', ['x_stride', 'y_stride', 'x_misaligned', 'w_misaligned'])
def test_rmsnorm_scalar_kernel_layouts(layout, eps):
    """the layouts that send an N % 8 == 0 row to the scalar kernel, each on its own, through the C ABI: a row stride of N + 4 on x or on
    y, x or the weight one element off 16-byte alignment.  y lives inside a NaN-filled allocation -- a guard row before and after, the
    padding columns of a strided y -- of which nothing may be written."""
    N, M = 4096, len(NC.ROW_KINDS)
    x, w = norm_case(N)
    ldx = N + 4 if layout == 'x_stride' else N
    ldy = N + 4 if layout == 'y_stride' else N
    xoff = 1 if layout == 'x_misaligned' else 0
    woff = 1 if layout == 'w_misaligned' else 0
    xbuf = torch.zeros(M * ldx + 8, dtype=torch.float16, device=DEV)
    xd = xbuf[xoff:xoff + M * ldx].view(M, ldx)
    xd[:, :N] = dev(x)
    wbuf = torch.zeros(N + 8, dtype=torch.float16, device=DEV)
    wd = wbuf[woff:woff + N]
    wd.copy_(dev(w))
    ybuf = torch.full((M + 2, ldy), float('nan'), dtype=torch.float16, device=DEV)
    yd = ybuf[1:M + 1]
    assert xbuf.data_ptr() % 16 == 0 and wbuf.data_ptr() % 16 == 0 and ybuf.data_ptr() % 16 == 0
    assert (xd.data_ptr() % 16 != 0) == bool(xoff) and (wd.data_ptr() % 16 != 0) == bool(woff)
    rc = _native.lib().gptq_rmsnorm_f16(xd.data_ptr(), ldx, wd.data_ptr(), yd.data_ptr(), ldy, M, N, eps, stream())
    _native.check(rc, 'gptq_rmsnorm_f16')
    torch.cuda.synchronize()
    got = ybuf.cpu().numpy()
    assert np.isnan(got[0].astype(np.float32)).all() and np.isnan(got[M + 1].astype(np.float32)).all(), 'a guard row was written'
    assert np.isnan(got[1:M + 1, N:].astype(np.float32)).all(), 'a padding column was written'
    check_norm(got[1:M + 1, :N], x, w, eps, '%s eps=%g' % (layout, eps))


# ---------------------------------------------------------------------------------------
# every fused norm: same rows, same weight
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layers(bits, gs, K, N, nsets, act=False):
    Ls = [make_random_layer(bits, gs, K, N, act_order=act, seed=3000 + 10 * bits + i) for i in range(nsets)]
    for L in Ls[1:]:
        L['g_idx'] = Ls[0]['g_idx']
    return tuple(Ls)


def dsets(Ls):
    return tuple(tuple(dev(L[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx')) for L in Ls)


def check_rows(got, x, Ls, nw, eps, bar, residual=None, name=''):
    """per row against the oracle composition; the zero row exactly the residual (or zero); a SiLU pair keeps a row only if its float64
    maximum is >= 2^-10 (tests/test_host_norm.py: that drops the subnormal row and nothing else)"""
    got = np.asarray(got)
    assert np.isfinite(got.astype(np.float32)).all(), name
    ref = NC.faithful_forward(x, Ls, nw, eps, residual)
    err = rowwise_rel_err(got, ref)
    keep = np.ones(len(x), dtype=bool)
    if len(Ls) == 2:
        keep = NC.silu_rows_kept(NC.exact_forward(x, Ls, nw, eps))
    iszero = ~np.asarray(x).any(axis=1)
    for m in np.nonzero(iszero)[0]:
        want = residual[m] if residual is not None else np.zeros_like(got[m])
        assert np.array_equal(got[m].astype(np.float32), want.astype(np.float32)), (name, 'zero row', int(m))
    print('%s: per-row err [%s] (bar %.1e)%s' % (name, ' '.join('%.2e' % e for e in err), bar, '' if keep.all() else ' kept %s' % keep.astype(int)))
    sel = keep & ~iszero
    assert (err[sel] < bar).all(), (name, err, bar)


@pytest.mark.parametrize('eps', NC.EPS_VALUES)
@pytest.mark.parametrize('bits', [2, 3, 4, 8])
@pytest.mark.parametrize('K,N,gs', [(256, 256, 128), (1056, 288, 32)])
@pytest.mark.parametrize('pair', [False, True])
def test_rowwave_fused_norm(pair, K, N, gs, bits, eps):
    """gptq_rmsnorm_matmul248_f16 / gptq_rmsnorm_fused_mlp_f16 (csrc/gemv.hip, NORM), one launch per row kind.  Where the entry declines
    (GPTQ_E_VARIANT: bits != 4, groups that are no multiple of 64) the caller's two launches are held to the same bar."""
    lib = _native.lib()
    Ls = layers(bits, gs, K, N, 2 if pair else 1)
    x, nw = norm_case(K, seed=1)
    d = dsets(Ls)
    nwd = dev(nw)
    ws = _native.workspace(torch.device(DEV))
    got = np.empty((len(x), N), dtype=np.float16)
    for m in range(len(x)):
        xd = dev(x[m:m + 1])
        y = torch.full((1, N), float('nan'), dtype=torch.float16, device=DEV)
        if pair:
            rc = lib.gptq_rmsnorm_fused_mlp_f16(xd.data_ptr(), nwd.data_ptr(), eps, d[0][0].data_ptr(), d[0][1].data_ptr(), d[0][2].data_ptr(), None,
                                                d[1][0].data_ptr(), d[1][1].data_ptr(), d[1][2].data_ptr(), None, y.data_ptr(), K, N, bits, gs,
                                                ws.data_ptr(), ws.numel(), stream())
        else:
            rc = lib.gptq_rmsnorm_matmul248_f16(xd.data_ptr(), nwd.data_ptr(), eps, d[0][0].data_ptr(), d[0][1].data_ptr(), d[0][2].data_ptr(), None, None,
                                                y.data_ptr(), K, N, bits, gs, ws.data_ptr(), ws.numel(), stream())
        if rc == E_VARIANT:
            # the documented decline (include/gptq_mi355x.h): the fused launch is the 4-bit row-wave kernel on groups of a multiple of 64;
            # every other layer takes gptq_rmsnorm_f16 + the plain entry -- two launches, the same values, the same bar
            assert bits != 4 or gs % 64 != 0, 'the fused launch declined a shape it documents to serve'
            h = torch.full((1, K), float('nan'), dtype=torch.float16, device=DEV)
            _native.check(lib.gptq_rmsnorm_f16(xd.data_ptr(), K, nwd.data_ptr(), h.data_ptr(), K, 1, K, eps, stream()), 'gptq_rmsnorm_f16')
            if pair:
                rc = lib.gptq_fused_mlp_f16(h.data_ptr(), K, d[0][0].data_ptr(), d[0][1].data_ptr(), d[0][2].data_ptr(), None, d[1][0].data_ptr(),
                                            d[1][1].data_ptr(), d[1][2].data_ptr(), None, y.data_ptr(), N, 1, K, N, bits, gs, ws.data_ptr(), ws.numel(), stream())
            else:
                rc = lib.gptq_matmul248_f16(h.data_ptr(), K, d[0][0].data_ptr(), d[0][1].data_ptr(), d[0][2].data_ptr(), None, None, y.data_ptr(), N, 1,
                                            K, N, bits, gs, ws.data_ptr(), ws.numel(), stream())
            _native.check(rc, 'two launches')
        else:
            _native.check(rc, 'gptq_rmsnorm_%s_f16' % ('fused_mlp' if pair else 'matmul248'))
            assert bits == 4 and gs % 64 == 0
        torch.cuda.synchronize()
        got[m] = y.cpu().numpy()[0]
    check_rows(got, x, Ls, nw, eps, TOL, name='rowwave pair=%d %dx%d w%d eps=%g' % (pair, K, N, bits, eps))


@pytest.mark.parametrize('eps', NC.EPS_VALUES)
@pytest.mark.parametrize('pair', [False, True])
def test_rowwave_fused_norm_act_order(pair, eps):
    """gptq_rmsnorm_sorted_f16: x AND the norm weight gathered through the act-order permutation (a weight taken in checkpoint order
    would pair every x with another channel's weight: invisible while the weight is ~1)"""
    lib = _native.lib()
    K, N, gs, bits = 1024, 288, 128, 4
    Ls = layers(bits, gs, K, N, 2 if pair else 1, act=True)
    x, nw = norm_case(K, seed=2)
    d = dsets(Ls)
    srt = [QL.act_order_sorted(s[0], s[3], K, gs, bits) for s in d]
    assert all(s is not None for s in srt)
    perm = srt[0][1]
    assert not torch.equal(perm, torch.arange(K, dtype=torch.int32, device=DEV))
    nwd = dev(nw)
    ws = _native.workspace(torch.device(DEV))
    got = np.empty((len(x), N), dtype=np.float16)
    for m in range(len(x)):
        xd = dev(x[m:m + 1])
        y = torch.full((1, N), float('nan'), dtype=torch.float16, device=DEV)
        up = (srt[1][0].data_ptr(), d[1][1].data_ptr(), d[1][2].data_ptr()) if pair else (None, None, None)
        rc = lib.gptq_rmsnorm_sorted_f16(xd.data_ptr(), nwd.data_ptr(), eps, perm.data_ptr(), srt[0][0].data_ptr(), d[0][1].data_ptr(), d[0][2].data_ptr(),
                                         up[0], up[1], up[2], None, y.data_ptr(), K, N, bits, gs, ws.data_ptr(), ws.numel(), stream())
        _native.check(rc, 'gptq_rmsnorm_sorted_f16')
        torch.cuda.synchronize()
        got[m] = y.cpu().numpy()[0]
    check_rows(got, x, Ls, nw, eps, TOL, name='sorted pair=%d eps=%g' % (pair, eps))


@pytest.mark.parametrize('eps', NC.EPS_VALUES)
@pytest.mark.parametrize('bits', [4, 3])
@pytest.mark.parametrize('act', [False, True])
@pytest.mark.parametrize('nsets', [1, 2])
@pytest.mark.parametrize('K,N', [(256, 768), (1024, 288)])
def test_stripe_matvec_fused_norm(K, N, nsets, act, bits, eps):
    """QL.stripe_matvec(norm_weight=...) (csrc/stripe_kernel.inc, one row): single set and gate | up pair, with and without the act-order
    permutation of x and of the norm weight, one launch per row kind"""
    gs = 128
    Ls = layers(bits, gs, K, N, nsets, act=act)
    x, nw = norm_case(K, seed=3)
    keep = dsets(Ls)
    pl = prepared(keep, None, bits, gs, K, N)
    assert pl.stripe is not None and (pl.perm16 is not None) == act
    nwd = dev(nw)
    got = np.empty((len(x), N), dtype=np.float16)
    for m in range(len(x)):
        out = torch.full((1, N), float('nan'), dtype=torch.float16, device=DEV)
        QL.stripe_matvec(dev(x[m:m + 1]), pl.stripe, out, K, N, bits, gs, nsets=nsets, norm_weight=nwd, eps=eps, perm=pl.perm16)
        torch.cuda.synchronize()
        got[m] = out.cpu().numpy()[0]
    check_rows(got, x, Ls, nw, eps, TOL, name='stripe %dx%d ns=%d act=%d w%d eps=%g' % (K, N, nsets, act, bits, eps))


def layer_decode(pl, x, N, nw, eps, residual):
    lib = _native.lib()
    M = x.shape[0]
    s = stream()
    ws = _native.layer_workspace(torch.device(DEV), s)
    need = lib.gptq_layer_decode_scratch_bytes(pl.handle, M)
    scratch = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
    y = torch.full((M, N), float('nan'), dtype=torch.float16, device=DEV)
    rc = lib.gptq_layer_decode_f16(pl.handle, x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), M, nw.data_ptr(), eps, _native.ptr(residual),
                                   0 if residual is None else residual.stride(0), ws.data_ptr(), ws.numel(), scratch.data_ptr(), scratch.numel(), s)
    _native.check(rc, 'gptq_layer_decode_f16')
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize('M', [1, 2, 4, 5, 8, 9, 16, 17])
@pytest.mark.parametrize('K,N,nsets', [(256, 768, 1), (256, 512, 2), (4096, 4096, 1)])
def test_layer_decode_norm_rows_of_different_scale(K, N, nsets, M):
    """gptq_layer_decode_f16 with a norm on a batch whose rows cycle through the kinds: the norm inside the decode launch (one rstd per
    row: MR > 1), and the norm as its own launch in front of the 16-row tiles; with and without a residual; both eps"""
    bits, gs = 4, 128
    Ls = layers(bits, gs, K, N, nsets)
    keep = dsets(Ls)
    pl = prepared(keep, None, bits, gs, K, N)
    rng = np.random.default_rng(K + N + M)
    x, nw = NC.batch_rows(M, K, rng), NC.norm_weight(K, rng)
    res = rng.standard_normal((M, N)).astype(np.float16)
    xd, nwd, resd = dev(x), dev(nw), dev(res)
    for eps in NC.EPS_VALUES:
        for use_res in ((False,) if nsets == 2 else (False, True)):
            y = layer_decode(pl, xd, N, nwd, eps, resd if use_res else None)
            bar = 2 * TOL if nsets == 2 else 1.5 * TOL if use_res else TOL
            check_rows(y, x, Ls, nw, eps, bar, residual=res if use_res else None,
                       name='layer_decode %dx%d ns=%d M=%d eps=%g res=%d' % (K, N, nsets, M, eps, use_res))


@functools.lru_cache(maxsize=None)
def dense_head(N, K):
    rng = np.random.default_rng(N + K)
    W = (rng.standard_normal((N, K)) * 0.02).astype(np.float16)
    W.setflags(write=False)
    return W


@pytest.mark.parametrize('eps', NC.EPS_VALUES)
@pytest.mark.parametrize('M', [1, 2, 7, 16])
@pytest.mark.parametrize('N,K', [(50, 256), (1000, 4096)])
def test_dense_head_fused_final_norm(N, K, M, eps):
    """gptq_dense_matmat_f16 (and, at one row, gptq_dense_matvec_f16 per row kind) with the final norm fused (csrc/dense_gemv.hip): against
    the float64 product of oracle.rmsnorm's fp16 output, per row"""
    lib = _native.lib()
    W = dense_head(N, K)
    rng = np.random.default_rng(N + K + M)
    x, nw = NC.batch_rows(M if M > 1 else len(NC.ROW_KINDS), K, rng), NC.norm_weight(K, rng)
    bias = rng.standard_normal(N).astype(np.float16) if N == 50 else None
    Wd, xd, nwd = dev(W), dev(x), dev(nw)
    bd = None if bias is None else dev(bias)
    exact = oracle.rmsnorm(x, nw, eps).astype(np.float64) @ W.astype(np.float64).T
    if bias is not None:
        exact = exact.astype(np.float16).astype(np.float64) + bias.astype(np.float64)
    y = torch.full((len(x), N), float('nan'), dtype=torch.float16, device=DEV)
    if M == 1:
        for m in range(len(x)):
            ym = torch.full((1, N), float('nan'), dtype=torch.float16, device=DEV)
            rc = lib.gptq_dense_matvec_f16(xd[m].data_ptr(), Wd.data_ptr(), K, _native.ptr(bd), ym.data_ptr(), N, K, nwd.data_ptr(), eps, stream())
            _native.check(rc, 'gptq_dense_matvec_f16')
            y[m] = ym[0]
        y1 = torch.full((1, N), float('nan'), dtype=torch.float16, device=DEV)
        rc = lib.gptq_dense_matmat_f16(xd[1].data_ptr(), K, Wd.data_ptr(), K, _native.ptr(bd), y1.data_ptr(), N, 1, N, K, nwd.data_ptr(), eps, stream())
        _native.check(rc, 'gptq_dense_matmat_f16')
        torch.cuda.synchronize()
        assert rowwise_rel_err(y1.cpu().numpy(), exact[1:2])[0] < TOL             # matmat at one row, on the `tiny` row
    else:
        rc = lib.gptq_dense_matmat_f16(xd.data_ptr(), K, Wd.data_ptr(), K, _native.ptr(bd), y.data_ptr(), N, M, N, K, nwd.data_ptr(), eps, stream())
        _native.check(rc, 'gptq_dense_matmat_f16')
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert np.isfinite(got.astype(np.float32)).all()
    err = rowwise_rel_err(got, exact)
    print('dense %dx%d M=%d eps=%g: per-row err [%s]' % (N, K, M, eps, ' '.join('%.2e' % e for e in err)))
    for m in np.nonzero(~x.any(axis=1))[0]:
        want = bias if bias is not None else np.zeros(N, dtype=np.float16)
        assert np.array_equal(got[m].astype(np.float32), want.astype(np.float32)), ('zero row', int(m))
    assert (err < TOL).all(), err
