"""GPU tests of the inverse-factor dispatch of GPTQ.fasterquant (gptq-for-llama_amd/gptq.py): a width that is a multiple of 128 takes
gptq_hinv_factor_f32 and no library factorisation, every other width keeps the three torch calls bit for bit."""
import pytest
import torch
import torch.nn as nn

import gptq
from quant import _native

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def run(cols, actorder=False, observe=False, hess=None):
    """quantise a 64 x cols layer to 4-bit g128 on a fixed Hessian: (Q, scale, zero, loss, the GPTQ object)"""
    gen = torch.Generator().manual_seed(cols)
    layer = nn.Linear(cols, 64, bias=False)
    layer.weight.data = torch.randn((64, cols), generator=gen) * 0.05
    x = torch.randn((2 * cols, cols), generator=gen) * torch.exp2(torch.rand((1, cols), generator=gen) * 2 - 1)
    g = gptq.GPTQ(layer.to(DEV), observe=observe)
    g.quantizer.configure(4, perchannel=True, sym=False, mse=False)
    g.H, g.nsamples = (x.t() @ x / cols).to(DEV) if hess is None else hess.to(DEV), 1
    scale, zero, _, loss = g.fasterquant(blocksize=128, percdamp=0.01, groupsize=128, actorder=actorder, name='t')
    return layer.weight.data.float().cpu(), scale.cpu(), zero.cpu(), loss, g


def raising(*args, **kwargs):
    raise AssertionError('a library factorisation was called')


def direct(hess, percdamp):
    """the C entry itself, as the dispatch must call it"""
    hess.diagonal().add_(percdamp * hess.diagonal().mean())
    n, work = hess.shape[0], hess.clone()
    U, info = torch.zeros_like(work), torch.zeros(1, dtype=torch.int32, device=hess.device)
    assert _native.lib().gptq_hinv_factor_f32(work.data_ptr(), n, n, U.data_ptr(), n, info.data_ptr(), _native.stream_ptr(hess.device)) == 0
    assert int(info.item()) == 0
    return U


def three_calls(hess, percdamp):
    hess.diagonal().add_(percdamp * hess.diagonal().mean())
    return torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(hess)), upper=True).contiguous()


@pytest.mark.parametrize('actorder', [False, True])
def test_multiple_of_128_takes_the_hip_sweep(monkeypatch, actorder):
    want = run(384, actorder)                                      # before the patches: the dispatch as shipped
    with monkeypatch.context() as m:
        m.setattr(torch.linalg, 'cholesky', raising)
        m.setattr(torch, 'cholesky_inverse', raising)
        got = run(384, actorder)
    monkeypatch.setattr(gptq, '_inverse_factor', direct)
    ref = run(384, actorder)
    for a, b, c in zip(got[:3], ref[:3], want[:3]):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert got[3] == ref[3] == want[3]


def test_other_widths_keep_the_torch_route(monkeypatch):
    got = run(200)
    monkeypatch.setattr(gptq, '_inverse_factor', three_calls)
    ref = run(200)
    assert torch.equal(got[0], ref[0]) and got[3] == ref[3]


def test_indefinite_hessian_raises_linalg_error():
    with pytest.raises(torch.linalg.LinAlgError):
        run(384, hess=-torch.eye(384))


def test_observe_keeps_the_damped_hessian():
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((768, 384), generator=gen)
    want = x.t() @ x / 384
    g = run(384, observe=True, hess=want)[4]
    want = want.to(DEV)
    want.diagonal().add_(0.01 * want.diagonal().mean())
    assert torch.equal(g.H, want), 'GPTQ.H is the damped Hessian, not the storage of R'
