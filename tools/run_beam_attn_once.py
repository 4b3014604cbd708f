#!/usr/bin/env python
"""a few calls of gptq_decode_attn_beam_f16 and of gptq_decode_attn_batch_f16 on the same N rows at ONE (N, position, tail) -- for rocprofv3
--kernel-trace / --pmc runs (profiles/beam_indirect/).    python tools/run_beam_attn_once.py [N] [position] [tail] [calls]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'gptq-for-llama_amd')]
import torch
from quant import _native

N, p, tail, calls = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 4), (2, 512), (3, 4), (4, 50)))
T_MAX, H, heads = 2048, 4096, 32
lib, dev = _native.lib(), torch.device('cuda:0')
s = _native.stream_ptr(dev)
g = torch.Generator(device=dev).manual_seed(N)
qkv = torch.randn((N, 3 * H), device=dev, generator=g).half()
k = (torch.randn((N, T_MAX, H), device=dev, generator=g) * 0.5).half()
v = torch.randn((N, T_MAX, H), device=dev, generator=g).half()
out = torch.zeros((N, H), dtype=torch.float16, device=dev)
ws_b = torch.zeros(lib.gptq_decode_attn_beam_ws_bytes(N, heads, T_MAX), dtype=torch.uint8, device=dev)
ws_r = torch.zeros(lib.gptq_decode_attn_batch_workspace_bytes(N, heads, 128, T_MAX), dtype=torch.uint8, device=dev)
pos = torch.full((N,), p, dtype=torch.int64, device=dev)
common = max(p - tail + 1, 0)
src = (torch.arange(T_MAX, device=dev) % N).to(torch.uint8).repeat(N, 1)
src[:, common:] = torch.arange(N, device=dev, dtype=torch.uint8)[:, None]
cm = torch.tensor([common], dtype=torch.int32, device=dev)
for _ in range(calls):
    rc = lib.gptq_decode_attn_beam_f16(qkv.data_ptr(), 3 * H, N, pos.data_ptr(), k.data_ptr(), v.data_ptr(), T_MAX * H, src.data_ptr(), cm.data_ptr(),
                                       out.data_ptr(), H, None, ws_b.data_ptr(), ws_b.numel(), heads, 128, T_MAX, 10000.0, 0.0884, None, s)
    assert rc == 0, rc
    rc = lib.gptq_decode_attn_batch_f16(qkv.data_ptr(), 3 * H, pos.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), H, ws_r.data_ptr(),
                                        ws_r.numel(), N, heads, 128, T_MAX, 10000.0, 0.0884, None, None, s)
    assert rc == 0, rc
torch.cuda.synchronize()
print('done', N, p, tail, calls)
