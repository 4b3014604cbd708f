"""CPU-side tests of the fp8 KV cache (include/gptq_mi355x.h "fp8 KV cache"): the properties of the quantisation rule as tests/kv8_ref.py restates
it, and the host validation of gptq_decode_attn_batch_kv8_f16 and gptq_kv8_store_f16 on fake aligned pointers -- nothing is launched, no device
is needed."""
import torch

import kv8_ref as R
from quant import _native

HEADS, HD, T_MAX, B = 4, 128, 384, 3
H = HEADS * HD
E_SHAPE, E_ALIGN, E_NULL, E_WORKSPACE = -2, -3, -4, -5


def _rows():
    gen = torch.Generator().manual_seed(11)
    x = R.random_rows(gen, (4096,), 1)
    # the ends of the fp16 range, exact powers of two around the two cases of the rule, a lone subnormal
    edge = torch.zeros((8, HD), dtype=torch.float16)
    edge[0, 0] = 65504.0
    edge[1, 5] = 2.0 ** -24
    edge[2, :2] = torch.tensor([448.0, 0.3])
    edge[3, :2] = torch.tensor([449.0, 0.3])            # m = 0.877: the other case
    edge[4, :3] = torch.tensor([-224.0, 1.0, 2.0 ** -10])
    edge[5, :2] = torch.tensor([0.875, -0.874])
    edge[6, :2] = torch.tensor([1.0, 2.0 ** -24])
    return torch.cat([x, edge])


def test_rule_exponent_range_and_scaled_amax():
    x = _rows()
    q, e = R.quantise(x)
    e = e.to(torch.int32).reshape(-1)
    amax = x.float().abs().amax(dim=-1)
    assert int(e.min()) >= -32 and int(e.max()) <= 8
    assert int(e[-8]) == 8 and int(e[-7]) == -32       # 65504 and 2^-24: both ends are reached
    zero = amax == 0
    assert int(zero.sum()) > 0 and bool((e[zero] == 0).all()) and bool((q[zero] == 0).all())
    scaled = torch.ldexp(amax, -e)[~zero]
    assert bool((scaled > 224).all()) and bool((scaled <= 448).all())
    assert float(torch.ldexp(amax, -e)[-6]) == 448.0 and float(torch.ldexp(amax, -e)[-5]) == 224.5      # 448 stays, 449 takes the next exponent
    # the smallest such exponent: one less would overflow
    assert bool((torch.ldexp(amax, -(e - 1))[~zero] > 448).all())
    assert not bool(((q & 0x7f) == 0x7f).any())        # never NaN


def test_rule_round_trip_error():
    x = _rows()
    q, e = R.quantise(x)
    back = R.dequantise(q, e)
    err = (back - x.double()).abs()
    step = torch.ldexp(torch.ones(1, dtype=torch.float64), e.to(torch.int32)).reshape(-1, 1)      # 2^e
    bound = torch.maximum(x.double().abs() * 2.0 ** -4, step * 2.0 ** -10)     # half an ulp of 3 mantissa bits, or half the subnormal spacing 2^-9
    assert bool((err <= bound).all())
    assert float((err / bound.clamp_min(1e-300)).max()) > 0.9                  # ... and the bound is reached: it is the format's, not a loose one


def test_rule_ties_and_subnormals():
    """what the restatement was checked for: ties go to even, 2^-10 -> 0, and no NaN below 464"""
    f8 = torch.float8_e4m3fn
    t = torch.tensor([17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10, 463.9, 448.0]).to(f8).float()     # 17 = 16 + 1: between 16 and 18
    assert t.tolist() == [16.0, 20.0, 0.0, 2.0 ** -8, 448.0, 448.0]


def _attn(lib, qkv=4096, ldq=3 * H, pos=4096, k8=4096, v8=4096, kexp=4096, vexp=4096, out=4096, ldo=H, ws=4096, ws_bytes=1 << 30, batch=B,
          heads=HEADS, hd=HD, t_max=T_MAX, table=None, perm=None, tps=0):
    return lib.gptq_decode_attn_batch_kv8_f16(qkv, ldq, pos, k8, v8, kexp, vexp, out, ldo, ws, ws_bytes, batch, heads, hd, t_max, 10000.0, 0.088,
                                              table, perm, tps, None)


def test_decode_attn_kv8_validation():
    lib = _native.lib()
    assert hasattr(lib, 'gptq_decode_attn_batch_kv8_f16') and 'gptq_decode_attn_batch_kv8_f16' in _native.EXPORTS
    assert len(lib.gptq_decode_attn_batch_kv8_f16.argtypes) == 21
    for name in ('qkv', 'pos', 'k8', 'v8', 'kexp', 'vexp', 'out', 'ws'):
        assert _attn(lib, **{name: None}) == E_NULL, name
    assert _attn(lib, qkv=None, hd=64) == E_NULL                   # NULL is reported first
    for kw in (dict(batch=0), dict(batch=65536), dict(heads=0), dict(hd=64), dict(hd=256), dict(t_max=0), dict(ldq=3 * H - 8), dict(ldo=H - 8),
               dict(t_max=1 << 22, heads=32)):                     # byte offsets of a slice beyond 32 bits
        assert _attn(lib, **kw) == E_SHAPE, kw
    assert _attn(lib, hd=64, qkv=4096 + 2) == E_SHAPE              # SHAPE before ALIGN
    for kw in (dict(qkv=4096 + 8), dict(k8=4096 + 8), dict(v8=4096 + 4), dict(ws=4096 + 8), dict(table=4096 + 4), dict(ldq=3 * H + 4),
               dict(ldo=H + 4), dict(out=4096 + 1), dict(perm=4096 + 2)):
        assert _attn(lib, **kw) == E_ALIGN, kw
    assert _attn(lib, kexp=4096 + 1, vexp=4096 + 3, ws_bytes=0) == E_WORKSPACE      # exponents are bytes: any address
    need = lib.gptq_decode_attn_batch_workspace_bytes(B, HEADS, HD, T_MAX)
    assert need > 0 and _attn(lib, ws_bytes=need - 1) == E_WORKSPACE


GOOD = [(0, 8, 0, 0), (0, 5, 10, 2), (0, 1, 383, 1)]       # (row0: ignored, rows, start, slot)


def _store(lib, segs=GOOD, nseq=None, k16=4096, v16=4096, stride=T_MAX * H, k8=4096, v8=4096, kexp=4096, vexp=4096, heads=HEADS, hd=HD, t_max=T_MAX):
    tab = None if segs is None else (_native.PromptSeg * max(1, len(segs)))(*[_native.PromptSeg(*s) for s in segs])
    n = (0 if segs is None else len(segs)) if nseq is None else nseq
    return lib.gptq_kv8_store_f16(k16, v16, stride, tab, n, k8, v8, kexp, vexp, heads, hd, t_max, None)


def test_kv8_store_validation():
    lib = _native.lib()
    assert hasattr(lib, 'gptq_kv8_store_f16') and 'gptq_kv8_store_f16' in _native.EXPORTS
    assert len(lib.gptq_kv8_store_f16.argtypes) == 13
    for name in ('k16', 'v16', 'k8', 'v8', 'kexp', 'vexp'):
        assert _store(lib, **{name: None}) == E_NULL, name
    assert _store(lib, segs=None, nseq=2) == E_NULL
    assert _store(lib, segs=[], nseq=0) == E_SHAPE
    assert _store(lib, segs=[(0, 1, 0, i) for i in range(17)]) == E_SHAPE
    for kw in (dict(heads=0), dict(hd=64), dict(t_max=0), dict(stride=T_MAX * H - 8), dict(segs=[(0, 0, 0, 0)]), dict(segs=[(0, 4, -1, 0)]),
               dict(segs=[(0, 8, T_MAX - 7, 0)]), dict(segs=[(0, 8, 0, -1)])):
        assert _store(lib, **kw) == E_SHAPE, kw
    assert _store(lib, hd=64, k16=4096 + 2) == E_SHAPE             # SHAPE before ALIGN
    for kw in (dict(k16=4096 + 8), dict(v16=4096 + 2), dict(k8=4096 + 8), dict(v8=4096 + 4), dict(stride=T_MAX * H + 4)):
        assert _store(lib, **kw) == E_ALIGN, kw
