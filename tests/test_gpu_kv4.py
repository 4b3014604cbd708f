"""The int4 KV cache kernels through the C entries, against tests/kv4_ref.py and a float64 attention over the dequantised cache.  Lengths ride in
the batch: two launches of 16 rows cover a first token, the ends of a wave instruction (16), of a pass (64), of a split's unit (128), of a tile
(512) and of the cache (640), idle rows included; with the default split rule (one split) and with 32 tokens per split (the ticket merge)."""
import functools

import pytest
import torch

import kv4_ref as R
from kv8_ref import random_rows
from quant import _native

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HD, T_MAX, BASE = 128, 640, 10000.0
SCALE = 1.0 / HD ** 0.5
SENT_Q, SENT_M, SENT_OUT = 0xC3, 77.0, 7.0
POS_A = (0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 300, -1)
POS_B = (510, 511, 512, 513, 575, 576, 600, 638, 639, -1, 640, 383, 384, 385, 1, 0)
CASES = {'A16': (POS_A, 2), 'B16': (POS_B, 2), 'B1': ((200,), 2), 'B3': ((5, 300, 639), 2), 'H32': ((70, 300, 639), 32)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """computed once: qkv; the cache before the call (quantised test rows below pos, sentinels above); the cache after it, restated from the rows
    gptq_decode_attn_batch_f16 appends for the same qkv; q rotated by the library's own RoPE"""
    positions, heads = CASES[name]
    lib, B, H = _native.lib(), len(positions), heads * HD
    gen = torch.Generator().manual_seed(len(name) * 100 + B + heads)
    k4, kmeta = R.quantise(random_rows(gen, (B, T_MAX), heads))
    v4, vmeta = R.quantise(random_rows(gen, (B, T_MAX), heads))
    new, q = random_rows(gen, (B, 2), heads), torch.randn((B, H), generator=gen)      # the new token's k and v; q scaled to scores of std 2.5
    s0 = torch.cat([(R.dequantise(k4[b, :max(p, 1)], kmeta[b, :max(p, 1)]).reshape(-1, heads, HD) * q[b].double().reshape(heads, HD)).sum(-1).reshape(-1)
                    for b, p in enumerate(positions)])
    q = (q * (2.5 / (float(s0.std()) * SCALE))).half()
    qkv = torch.cat([q, new[:, 0], new[:, 1]], dim=1).to(DEV)
    for b, p in enumerate(positions):
        lo = max(0, min(p, T_MAX))
        k4[b, lo:], v4[b, lo:], kmeta[b, lo:], vmeta[b, lo:] = SENT_Q, SENT_Q, SENT_M, SENT_M
    pos = torch.tensor(positions, dtype=torch.int64, device=DEV)
    kc, vc = torch.zeros((B, T_MAX, H), dtype=torch.float16, device=DEV), torch.zeros((B, T_MAX, H), dtype=torch.float16, device=DEV)
    ws = torch.zeros(lib.gptq_decode_attn_batch_workspace_bytes(B, heads, HD, T_MAX), dtype=torch.uint8, device=DEV)
    o16 = torch.zeros((B, H), dtype=torch.float16, device=DEV)
    rc = lib.gptq_decode_attn_batch_f16(qkv.data_ptr(), 3 * H, pos.data_ptr(), kc.data_ptr(), vc.data_ptr(), o16.data_ptr(), H, ws.data_ptr(), ws.numel(),
                                        B, heads, HD, T_MAX, BASE, SCALE, None, None, None)
    assert rc == 0
    qrot = torch.zeros((B, H), dtype=torch.float16)
    want = [t.clone() for t in (k4, v4, kmeta, vmeta)]
    for b, p in enumerate(positions):
        if not 0 <= p < T_MAX:
            continue
        want[0][b, p], want[2][b, p] = R.quantise(kc[b, p])
        want[1][b, p], want[3][b, p] = R.quantise(vc[b, p])
        one, scratch = qkv[b].clone(), torch.zeros((2, T_MAX, H), dtype=torch.float16, device=DEV)
        assert lib.gptq_decode_rope_kv_f16(one.data_ptr(), pos[b:b + 1].data_ptr(), scratch[0].data_ptr(), scratch[1].data_ptr(), heads, HD, T_MAX, BASE,
                                           None) == 0
        qrot[b] = one[:H].cpu()
    torch.cuda.synchronize()
    return dict(qkv=qkv, pos=pos, before=(k4, v4, kmeta, vmeta), want=want, qrot=qrot, heads=heads, positions=positions)


def _run(c, tps, perm=None):
    lib, B, heads = _native.lib(), len(c['positions']), c['heads']
    H = heads * HD
    k4, v4, kmeta, vmeta = (t.to(DEV) for t in c['before'])
    out = torch.full((B, H), SENT_OUT, dtype=torch.float16, device=DEV)
    ws = torch.zeros(lib.gptq_decode_attn_batch_workspace_bytes(B, heads, HD, T_MAX), dtype=torch.uint8, device=DEV)
    outs = []
    for _ in range(2):
        rc = lib.gptq_decode_attn_batch_kv4_f16(c['qkv'].data_ptr(), 3 * H, c['pos'].data_ptr(), k4.data_ptr(), v4.data_ptr(), kmeta.data_ptr(),
                                                vmeta.data_ptr(), out.data_ptr(), H, ws.data_ptr(), ws.numel(), B, heads, HD, T_MAX, BASE, SCALE, None,
                                                None if perm is None else perm.data_ptr(), tps, None)
        assert rc == 0
        torch.cuda.synchronize()
        outs.append(out.cpu())
    return outs, [t.cpu() for t in (k4, v4, kmeta, vmeta)]


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.float16 else t


@pytest.mark.parametrize('tps', [0, 32])
@pytest.mark.parametrize('name', list(CASES))
def test_decode_attn_kv4(name, tps):
    c = _case(name)
    (out, again), cache = _run(c, tps)
    assert torch.equal(_bits(out), _bits(again))                                      # two calls, the same bits
    for got, want, what in zip(cache, c['want'], ('k4', 'v4', 'kmeta', 'vmeta')):     # the appended row byte-exact, every other byte unchanged
        assert torch.equal(_bits(got), _bits(want)), what
    for b, p in enumerate(c['positions']):
        if not 0 <= p < T_MAX:                                                        # an idle row: out untouched (the cache was compared above)
            assert bool((out[b] == SENT_OUT).all())
            continue
        ref = R.attention(c['qrot'][b], cache[0][b], cache[2][b], cache[1][b], cache[3][b], p + 1, SCALE)
        err = float((out[b].double() - ref).abs().max() / ref.abs().max())
        assert err < 1e-3, 'row %d (pos %d): %.3g' % (b, p, err)


@pytest.mark.parametrize('tps', [0, 32])
def test_decode_attn_kv4_out_perm(tps):
    c = _case('B3')
    H = c['heads'] * HD
    perm = torch.randperm(H, generator=torch.Generator().manual_seed(5)).to(dtype=torch.int32, device=DEV)
    (plain, _), _ = _run(c, tps)
    (moved, _), _ = _run(c, tps, perm)
    want = torch.empty_like(plain)
    want[:, perm.cpu().long()] = plain
    assert torch.equal(_bits(moved), _bits(want))


def test_kv4_store_segments():
    lib, heads, slots = _native.lib(), 2, 4
    H = heads * HD
    gen = torch.Generator().manual_seed(9)
    pad = 8                                                          # slots of the source further apart than t_max rows
    src = [random_rows(gen, (slots, T_MAX + pad), heads) for _ in range(2)]
    k16, v16 = (t.to(DEV) for t in src)
    segs = [(0, 37, 0, 2), (5, 1, T_MAX - 1, 0), (0, 200, 100, 3), (0, 3, 62, 1)]       # (row0: ignored, rows, start, slot)
    table = (_native.PromptSeg * len(segs))(*[_native.PromptSeg(*s) for s in segs])
    k4, v4 = (torch.full((slots, T_MAX, H // 2), SENT_Q, dtype=torch.uint8, device=DEV) for _ in range(2))
    kmeta, vmeta = (torch.full((slots, T_MAX, heads, 4, 2), SENT_M, dtype=torch.float16, device=DEV) for _ in range(2))
    rc = lib.gptq_kv4_store_f16(k16.data_ptr(), v16.data_ptr(), (T_MAX + pad) * H, table, len(segs), k4.data_ptr(), v4.data_ptr(), kmeta.data_ptr(),
                                vmeta.data_ptr(), heads, HD, T_MAX, None)
    assert rc == 0
    torch.cuda.synchronize()
    for got_q, got_m, s16 in ((k4.cpu(), kmeta.cpu(), src[0]), (v4.cpu(), vmeta.cpu(), src[1])):
        want_q, want_m = torch.full_like(got_q, SENT_Q), torch.full_like(got_m, SENT_M)
        for _, rows, start, slot in segs:
            want_q[slot, start:start + rows], want_m[slot, start:start + rows] = R.quantise(s16[slot, start:start + rows])
        assert torch.equal(got_q, want_q) and torch.equal(_bits(got_m), _bits(want_m))
