"""CPU-side tests of the int4 KV cache (include/gptq_mi355x.h "int4 KV cache"): the properties of the quantisation rule as tests/kv4_ref.py
restates it, and the host validation of gptq_decode_attn_batch_kv4_f16 and gptq_kv4_store_f16 on fake aligned pointers -- nothing is launched,
no device is needed."""
import os

import pytest
import torch

import kv4_ref as R
from kv8_ref import random_rows
from quant import _native

HEADS, HD, T_MAX, B = 4, 128, 384, 3
H = HEADS * HD
E_SHAPE, E_ALIGN, E_NULL, E_WORKSPACE = -2, -3, -4, -5


def test_rule_codes_constant_groups_and_round_trip():
    x = random_rows(torch.Generator().manual_seed(11), (4096,), 1)
    x[:3, :32] = torch.tensor([[65504.0], [-3.25], [2.0 ** -24]], dtype=torch.float16)      # constant groups at the ends of the range
    x[3, :32] = torch.linspace(-65504.0, 65504.0, 32).half()                                  # the widest group
    x[4, :32] = torch.arange(32).half() % 16                                                  # d = 1, m = 0: the codes are the values
    codes, meta = R.quantise(x)
    assert codes.shape == (x.shape[0], 64) and meta.shape == (x.shape[0], 1, 4, 2)
    back = R.dequantise(codes, meta).reshape(-1, 4, 32)
    g, d = x.double().reshape(-1, 4, 32), meta[:, 0, :, 0:1].double()
    const = (g.amax(-1) == g.amin(-1))
    assert int(const.sum()) > 3 and bool((d[const] == 0).all()) and bool((back[const] == g[const]).all())
    assert bool((meta[:, 0, :, 1].double() == g.amin(-1)).all())                              # m is the minimum, exactly
    assert codes[4, :4].tolist() == [0x20, 0x64, 0x31, 0x75] and meta[4, 0, 0].tolist() == [1.0, 0.0]      # the header's nibble order
    ulp = torch.ldexp(torch.ones(1, dtype=torch.float64), (torch.frexp(d * 15)[1] - 11).clamp_min(-24))      # one fp16 ulp of d * 15
    err = (back - g).abs()
    assert bool((err <= d / 2 + ulp).all())
    assert float((err / (d / 2 + ulp).clamp_min(1e-300)).max()) > 0.8                         # ... and the bound is the format's, not a loose one


def _attn(lib, qkv=4096, ldq=3 * H, pos=4096, k4=4096, v4=4096, kmeta=4096, vmeta=4096, out=4096, ldo=H, ws=4096, ws_bytes=1 << 30, batch=B,
          heads=HEADS, hd=HD, t_max=T_MAX, table=None, perm=None, tps=0):
    return lib.gptq_decode_attn_batch_kv4_f16(qkv, ldq, pos, k4, v4, kmeta, vmeta, out, ldo, ws, ws_bytes, batch, heads, hd, t_max, 10000.0, 0.088,
                                              table, perm, tps, None)


GOOD = [(0, 8, 0, 0), (0, 5, 10, 2), (0, 1, 383, 1)]       # (row0: ignored, rows, start, slot)


def _store(lib, segs=GOOD, nseq=None, k16=4096, v16=4096, stride=T_MAX * H, k4=4096, v4=4096, kmeta=4096, vmeta=4096, heads=HEADS, hd=HD, t_max=T_MAX):
    tab = None if segs is None else (_native.PromptSeg * max(1, len(segs)))(*[_native.PromptSeg(*s) for s in segs])
    n = (0 if segs is None else len(segs)) if nseq is None else nseq
    return lib.gptq_kv4_store_f16(k16, v16, stride, tab, n, k4, v4, kmeta, vmeta, heads, hd, t_max, None)


def test_symbols_are_exported_bound_and_declared():
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'gptq_mi355x.h')).read()
    for name, nargs in (('gptq_decode_attn_batch_kv4_f16', 21), ('gptq_kv4_store_f16', 13)):
        assert name in _native.EXPORTS and len(getattr(_native.lib(), name).argtypes) == nargs and ('int %s(' % name) in header


NEED = 'need'       # stands for gptq_decode_attn_batch_workspace_bytes(B, HEADS, HD, T_MAX) - 1
CASES = [(_attn, {n: None}, E_NULL) for n in ('qkv', 'pos', 'k4', 'v4', 'kmeta', 'vmeta', 'out', 'ws')] + [
    (_attn, dict(qkv=None, hd=64), E_NULL),                        # NULL is reported first
] + [(_attn, kw, E_SHAPE) for kw in (dict(batch=0), dict(batch=65536), dict(heads=0), dict(hd=64), dict(hd=256), dict(t_max=0), dict(ldq=3 * H - 8),
                                     dict(ldo=H - 8), dict(t_max=1 << 22, heads=32), dict(hd=64, qkv=4096 + 2))] + [
    (_attn, kw, E_ALIGN) for kw in (dict(qkv=4096 + 8), dict(k4=4096 + 8), dict(v4=4096 + 4), dict(kmeta=4096 + 2), dict(vmeta=4096 + 1),
                                    dict(ws=4096 + 8), dict(table=4096 + 4), dict(ldq=3 * H + 4), dict(ldo=H + 4), dict(out=4096 + 1),
                                    dict(perm=4096 + 2))] + [
    (_attn, dict(ws_bytes=0), E_WORKSPACE), (_attn, dict(ws_bytes=NEED), E_WORKSPACE),
] + [(_store, {n: None}, E_NULL) for n in ('k16', 'v16', 'k4', 'v4', 'kmeta', 'vmeta')] + [
    (_store, dict(segs=None, nseq=2), E_NULL),
] + [(_store, kw, E_SHAPE) for kw in (dict(segs=[], nseq=0), dict(segs=[(0, 1, 0, i) for i in range(17)]), dict(heads=0), dict(hd=64), dict(t_max=0),
                                      dict(stride=T_MAX * H - 8), dict(segs=[(0, 0, 0, 0)]), dict(segs=[(0, 4, -1, 0)]),
                                      dict(segs=[(0, 8, T_MAX - 7, 0)]), dict(segs=[(0, 8, 0, -1)]), dict(hd=64, k16=4096 + 2))] + [
    (_store, kw, E_ALIGN) for kw in (dict(k16=4096 + 8), dict(v16=4096 + 2), dict(k4=4096 + 8), dict(v4=4096 + 4), dict(kmeta=4096 + 2),
                                     dict(vmeta=4096 + 3), dict(stride=T_MAX * H + 4))]


@pytest.mark.parametrize('fn,kw,code', CASES, ids=['%s-%s-%d' % (f.__name__, '+'.join(k), c) for f, k, c in CASES])
def test_validation_codes(fn, kw, code):
    lib = _native.lib()
    if kw.get('ws_bytes') == NEED:
        kw = dict(kw, ws_bytes=lib.gptq_decode_attn_batch_workspace_bytes(B, HEADS, HD, T_MAX) - 1)
    assert fn(lib, **kw) == code
