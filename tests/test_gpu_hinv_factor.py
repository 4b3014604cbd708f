"""GPU tests of gptq_hinv_factor_f32 (csrc/hinv_factor.hip): U upper triangular with U^T U = A^-1 from the reversed blocked Cholesky sweep, against
float64.  The block edge is 128: n = 128 is the diagonal kernel alone, 256 the first panel, row and trailing tile, 384 a row tile whose sum spans
two blocks and an off-diagonal trailing tile, 640 five blocks.  The bar is today's three-call torch route on the same matrix: the sweep may be at
most 4 x as far from float64 (both are backward stable; the two algorithms differ by 0.67 .. 2.31 in LAPACK, and a max-norm over 1e4 .. 1e5
elements moves that much with summation order alone; a mis-indexed tile is wrong by O(1))."""
import functools

import pytest
import torch

from quant import _native

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
A_PAD, U_PAD = 777.0, 1234.5
CASES = [(n, kind, 0, 0) for n in (128, 256, 384, 640) for kind in ('mixed', 'rank', 'scaled')] + [(256, 'mixed', 4, 8)]


@functools.lru_cache(maxsize=None)
def problem(n, kind):
    """(A fp32 damped, U64, error of the three-call torch route on the GPU): A = 2/T X^T X in float64 from fp16 rows, rounded, damped with 1 %"""
    gen = torch.Generator().manual_seed(n + len(kind))
    T = n // 2 if kind == 'rank' else 2 * n                       # 'rank': deficient, only the damping makes it definite
    x = torch.randn((T, n), generator=gen) + 0.5 * torch.randn((T, 1), generator=gen)   # mixed columns: a shared component
    if kind == 'scaled':
        x = x * torch.exp2(torch.rand((1, n), generator=gen) * 12 - 6)
    x = x.half().double()
    a = (2.0 / T * (x.t() @ x)).float()
    a.diagonal().add_(0.01 * a.diagonal().mean())
    u64 = torch.linalg.cholesky(torch.linalg.inv(a.double())).t().contiguous()
    ad = a.to(DEV)
    old = torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(ad)), upper=True).cpu()
    return a, u64, float((old.double() - u64).abs().max() / u64.abs().max())


def factor(a, apad=0, upad=0):
    """run the entry on a fresh padded copy of a (CPU fp32): (rc, info, A after, U after)"""
    n = a.shape[0]
    A = torch.full((n, n + apad), A_PAD)
    A[:, :n] = a
    A, U, info = A.to(DEV), torch.full((n, n + upad), U_PAD, device=DEV), torch.full((1,), -7, dtype=torch.int32, device=DEV)
    rc = _native.lib().gptq_hinv_factor_f32(A.data_ptr(), n + apad, n, U.data_ptr(), n + upad, info.data_ptr(), _native.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, int(info.item()), A.cpu(), U.cpu()


@pytest.mark.parametrize('n,kind,apad,upad', CASES)
def test_against_float64(n, kind, apad, upad):
    a, u64, err_torch = problem(n, kind)
    rc, info, A, U = factor(a, apad, upad)
    assert rc == 0 and info == 0
    got = U[:, :n]
    err = float((got.double() - u64).abs().max() / u64.abs().max())
    print('n %d %s: max|U - U64| / max|U64| %.3g, three torch calls %.3g, ratio %.2f' % (n, kind, err, err_torch, err / err_torch))
    assert err <= 4 * err_torch
    assert torch.equal(torch.tril(got, -1), torch.zeros(n, n)) and not torch.signbit(torch.tril(got, -1)).any(), 'exact +0 below the diagonal'
    assert bool((got.diagonal() > 0).all())
    assert torch.equal(A[:, n:], torch.full((n, apad), A_PAD)) and torch.equal(U[:, n:], torch.full((n, upad), U_PAD)), 'padding of the rows'
    assert torch.equal(factor(a, apad, upad)[3], U), 'same input, same bits'


def test_exact_on_a_diagonal():
    """A = diag(4^k), k cycling through -3 .. 3: every operation is exact, U = diag(2^-k) and nothing else"""
    k = torch.arange(384) % 7 - 3
    rc, info, _, U = factor(torch.diag(torch.exp2(2.0 * k)))
    assert rc == 0 and info == 0
    assert torch.equal(U, torch.diag(torch.exp2(-1.0 * k)))


def test_not_positive_definite_is_reported_not_fatal():
    """a negative diagonal element in block 1 of 3: the columns behind it do not depend on it, so it is the first bad pivot the sweep meets"""
    a, u64, err_torch = problem(384, 'mixed')
    broken = a.clone()
    broken[200, 200] = -1.0
    rc, info, _, _ = factor(broken)
    assert rc == 0 and info == 201
    rc, info, _, U = factor(a)
    assert rc == 0 and info == 0
    assert float((U.double() - u64).abs().max() / u64.abs().max()) <= 4 * err_torch


@pytest.mark.parametrize('bad,code', [(dict(n=200), -2), (dict(lda=252), -2), (dict(offset=4), -3), (dict(info=False), -4)])
def test_validation_leaves_u_alone(bad, code):
    A = torch.eye(260, device=DEV)[:256].contiguous()
    U, info = torch.full((256, 256), U_PAD, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    v = {**dict(n=256, lda=260, offset=0, info=True), **bad}
    rc = _native.lib().gptq_hinv_factor_f32(A.data_ptr() + v['offset'], v['lda'], v['n'], U.data_ptr(), 256, info.data_ptr() if v['info'] else None,
                                            _native.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == code and bool((U == U_PAD).all())
