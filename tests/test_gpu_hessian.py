"""GPU tests of gptq_hessian_update_f16 (csrc/hessian.hip): H <- decay H + weight X^T X in place on fp16 rows, against float64.  The tile edge is
128 columns and the staged chunk 64 tokens (the kernel does not split the tokens over workgroups): k = 8 is one partial tile, 136 / 264 / 520
are 8 past one, two and four tile edges; the token counts straddle the MFMA's 16-token step and the chunk."""
import itertools

import pytest
import torch

from quant import _native

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
X_PAD, H_PAD = 777.0, 1234.5                 # sentinels in the padding of rows (ldx > k, ldh > k)
# (k, tokens, ldx - k, ldh - k)
CASES = [(k, t, 0, 0) for k, t in itertools.product((8, 136, 264, 520), (1, 15, 17, 63, 65, 130))] + [(8, 17, 8, 4), (136, 65, 8, 4), (264, 130, 24, 12)]


def update(x, k, H, decay, weight):
    """x [tokens, ldx] fp16, H [k, ldh] fp32, both on the device; in place"""
    rc = _native.lib().gptq_hessian_update_f16(x.data_ptr(), x.shape[1], x.shape[0], k, H.data_ptr(), H.shape[1], decay, weight,
                                               _native.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc


def padded(m, pad, fill):
    out = torch.full((m.shape[0], m.shape[1] + pad), fill, dtype=m.dtype)
    out[:, :m.shape[1]] = m
    return out.to(DEV)


def symmetric(k, gen, integer):
    a = torch.randint(-50, 51, (k, k), generator=gen).double() if integer else torch.randn((k, k), generator=gen, dtype=torch.float64)
    return torch.triu(a) + torch.triu(a, 1).t()


@pytest.mark.parametrize('k,tokens,xpad,hpad', CASES)
def test_exact_on_integers(k, tokens, xpad, hpad):
    """integer x in [-3, 3] and an integer H: every sum stays below 2^24, so the result IS the float64 one -- indexing, edge masking, the
    diagonal-tile path and the mirror"""
    gen = torch.Generator().manual_seed(1000 * k + tokens)
    x = torch.randint(-3, 4, (tokens, k), generator=gen).double()
    h0 = symmetric(k, gen, True)
    xd, H = padded(x.half(), xpad, X_PAD), padded(h0.float(), hpad, H_PAD)
    assert update(xd, k, H, 1.0, 1.0) == 0
    want = padded((h0 + x.t() @ x).float(), hpad, H_PAD)
    assert torch.equal(H, want), 'H + X^T X, or the padding of its rows'
    assert torch.equal(xd, padded(x.half(), xpad, X_PAD))


@pytest.mark.parametrize('n', [0, 5])
@pytest.mark.parametrize('k,tokens,xpad,hpad', CASES)
def test_off_unit_scale(k, tokens, xpad, hpad, n):
    """rows N(0, 1) x 2^U(-6, 6), a random symmetric H, the running mean's scalars: within 1e-5 of max|H| of float64 (summation order only),
    bit-symmetric, and the same bits on a second call"""
    gen = torch.Generator().manual_seed(7000 * k + 10 * tokens + n)
    x = (torch.randn((tokens, k), generator=gen) * torch.exp2(torch.rand((tokens, 1), generator=gen) * 12 - 6)).half()
    h0 = symmetric(k, gen, False).float()
    decay, weight = n / (n + 1), 2 / (n + 1)
    want = decay * h0.double() + weight * (x.double().t() @ x.double())
    xd, H = padded(x, xpad, X_PAD), padded(h0, hpad, H_PAD)
    again = H.clone()
    assert update(xd, k, H, decay, weight) == 0 and update(xd, k, again, decay, weight) == 0
    got = H[:, :k].cpu()
    x32 = (weight ** 0.5 * x.float().to(DEV)).t()
    torch_route = (h0.to(DEV) * decay).addmm_(x32, x32.t()).cpu()
    err, err_torch = ((m.double() - want).abs().max() / want.abs().max() for m in (got, torch_route))
    print('k %d tokens %d n %d: max err / max|H| %.3g (torch fp32 route %.3g)' % (k, tokens, n, err, err_torch))
    assert err < 1e-5
    assert torch.equal(got, got.t()), 'H[j][i] must have the bits of H[i][j]'
    assert torch.equal(H, again), 'same inputs, same bits'
    assert torch.equal(H[:, k:].cpu(), torch.full((k, hpad), H_PAD))


@pytest.mark.parametrize('bad,code', [(dict(k=12), -2), (dict(ldx=8), -2), (dict(tokens=0), -2), (dict(offset=2), -3)])
def test_validation_leaves_h_alone(bad, code):
    x = torch.ones((16, 24), dtype=torch.float16, device=DEV)
    H = torch.full((16, 16), H_PAD, device=DEV)
    a = {**dict(k=16, ldx=24, tokens=16, offset=0), **bad}
    rc = _native.lib().gptq_hessian_update_f16(x.data_ptr() + a['offset'], a['ldx'], a['tokens'], a['k'], H.data_ptr(), 16, 1.0, 1.0,
                                               _native.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == code and bool((H == H_PAD).all())
