"""GPU test of GPTQ.add_batch (gptq-for-llama_amd/gptq.py): fp16 activations of an nn.Linear take gptq_hessian_update_f16, everything else keeps
the reference's torch expression bit for bit."""
import math

import pytest
import torch
import torch.nn as nn

import gptq

pytestmark = pytest.mark.gpu
DEV, K = 'cuda:0', 264


def test_add_batch_fp16_native_and_fp32_unchanged():
    layer = nn.Linear(K, 128, bias=False).half().to(DEV)
    gen = torch.Generator().manual_seed(11)
    xs = [(torch.randn(s, generator=gen) * torch.exp2(torch.rand(s[:-1] + (1,), generator=gen) * 12 - 6)).half().to(DEV)
          for s in [(1, 33, K), (2, 17, K), (40, K)]]
    g, g32 = gptq.GPTQ(layer), gptq.GPTQ(layer)
    # the arithmetic of oracle/gptq_solver.hessian_add_batch (reference gptq.py:71-96) in float64, and the parent's fp32 expression inline
    want, ref, n = torch.zeros((K, K), dtype=torch.float64), torch.zeros((K, K), device=DEV), 0
    for x in xs:
        g.add_batch(x, None)
        g32.add_batch(x.float(), None)
        b = 1 if x.dim() == 2 else x.shape[0]
        want *= n / (n + b)
        ref *= n / (n + b)
        n += b
        xt = math.sqrt(2 / n) * x.reshape(-1, K).double().cpu().t()
        want += xt @ xt.t()
        xt = math.sqrt(2 / n) * x.float().reshape(-1, K).t().float()
        ref.addmm_(xt, xt.t())
    H = g.H.cpu()
    assert g.nsamples == g32.nsamples == n == 4
    assert float((H.double() - want).abs().max() / want.abs().max()) < 1e-5
    assert torch.equal(H, H.t()), 'the native route leaves H bit-symmetric'
    assert torch.equal(g32.H, ref), 'fp32 activations keep the torch route'
