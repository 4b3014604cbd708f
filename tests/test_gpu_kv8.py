"""GPU tests of the fp8 KV cache kernels through the C entries (csrc/decode_attn_kv8.hip): gptq_decode_attn_batch_kv8_f16 against the format's
restatement (tests/kv8_ref.py) and a float64 attention over the dequantised cache, gptq_kv8_store_f16 byte for byte.  Lengths ride in the
batch: two launches of 16 rows cover a first token, the ends of a pass (32), of the tiny path (64), of a tile (256), of a split's unit (128)
and of the cache (t_max = 640), idle rows included; each runs with the default split rule (one split) and with 32 tokens per split (several
splits and the ticket merge at these sizes)."""
import functools

import pytest
import torch

import kv8_ref as R
from quant import _native

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HD, T_MAX, BASE = 128, 640, 10000.0
SCALE = 1.0 / HD ** 0.5
SENT_Q, SENT_E, SENT_OUT = 0xC3, 77, 7.0
POS_A = (0, 1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 127, 128, 129, 255, -1)
POS_B = (256, 257, 300, 511, 512, 513, 600, 638, 639, -1, 640, 383, 384, 385, 1, 0)
CASES = {'A16': (POS_A, 2), 'B16': (POS_B, 2), 'B1': ((200,), 2), 'B3': ((5, 300, 639), 2), 'H32': ((70, 300, 639), 32)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs of a launch, its fp16 reference rows and the rotated query, computed once: qkv [B, 3 H]; the fp8 cache before the call (rows below
    pos: quantised test rows, the rest a sentinel pattern); the rows gptq_decode_attn_batch_f16 appends to an fp16 cache from the same qkv,
    restated; q rotated by the library's own RoPE"""
    positions, heads = CASES[name]
    lib, B, H = _native.lib(), len(positions), heads * HD
    gen = torch.Generator().manual_seed(len(name) * 100 + B + heads)
    hist = R.random_rows(gen, (B, T_MAX), heads)
    k8, kexp = R.quantise(hist)
    v8, vexp = R.quantise(R.random_rows(gen, (B, T_MAX), heads))
    new = R.random_rows(gen, (B, 2), heads)                       # the new token's k and v
    q = torch.randn((B, H), generator=gen)
    # scores scale q (k / 2^ek) 2^ek: choose |q| so that their standard deviation over the launch is 2.5
    s0 = torch.cat([(R.dequantise(k8[b, :max(p, 1)], kexp[b, :max(p, 1)]).reshape(-1, heads, HD) * q[b].double().reshape(heads, HD)).sum(-1).reshape(-1)
                    for b, p in enumerate(positions)])
    q = (q * (2.5 / (float(s0.std()) * SCALE))).half()
    qkv = torch.cat([q, new[:, 0], new[:, 1]], dim=1).to(DEV)
    for b, p in enumerate(positions):
        lo = max(0, min(p, T_MAX))
        k8[b, lo:], v8[b, lo:], kexp[b, lo:], vexp[b, lo:] = SENT_Q, SENT_Q, SENT_E, SENT_E
    pos = torch.tensor(positions, dtype=torch.int64, device=DEV)
    # the fp16 entry on the same qkv: the rows it appends are what the fp8 entry must quantise
    kc, vc = torch.zeros((B, T_MAX, H), dtype=torch.float16, device=DEV), torch.zeros((B, T_MAX, H), dtype=torch.float16, device=DEV)
    ws = torch.zeros(lib.gptq_decode_attn_batch_workspace_bytes(B, heads, HD, T_MAX), dtype=torch.uint8, device=DEV)
    o16 = torch.zeros((B, H), dtype=torch.float16, device=DEV)
    rc = lib.gptq_decode_attn_batch_f16(qkv.data_ptr(), 3 * H, pos.data_ptr(), kc.data_ptr(), vc.data_ptr(), o16.data_ptr(), H, ws.data_ptr(), ws.numel(),
                                        B, heads, HD, T_MAX, BASE, SCALE, None, None, None)
    assert rc == 0
    qrot = torch.zeros((B, H), dtype=torch.float16)
    want = [t.clone() for t in (k8, v8, kexp, vexp)]
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
    return dict(qkv=qkv, pos=pos, before=(k8, v8, kexp, vexp), want=want, qrot=qrot, heads=heads, positions=positions)


def _run(c, tps, perm=None):
    lib, B, heads = _native.lib(), len(c['positions']), c['heads']
    H = heads * HD
    k8, v8, kexp, vexp = (t.to(DEV) for t in c['before'])
    out = torch.full((B, H), SENT_OUT, dtype=torch.float16, device=DEV)
    ws = torch.zeros(lib.gptq_decode_attn_batch_workspace_bytes(B, heads, HD, T_MAX), dtype=torch.uint8, device=DEV)
    outs = []
    for _ in range(2):
        rc = lib.gptq_decode_attn_batch_kv8_f16(c['qkv'].data_ptr(), 3 * H, c['pos'].data_ptr(), k8.data_ptr(), v8.data_ptr(), kexp.data_ptr(),
                                                vexp.data_ptr(), out.data_ptr(), H, ws.data_ptr(), ws.numel(), B, heads, HD, T_MAX, BASE, SCALE, None,
                                                None if perm is None else perm.data_ptr(), tps, None)
        assert rc == 0
        torch.cuda.synchronize()
        outs.append(out.cpu())
    return outs, [t.cpu() for t in (k8, v8, kexp, vexp)]


@pytest.mark.parametrize('tps', [0, 32])
@pytest.mark.parametrize('name', list(CASES))
def test_decode_attn_kv8(name, tps):
    c = _case(name)
    (out, again), cache = _run(c, tps)
    assert torch.equal(out.view(torch.int16), again.view(torch.int16))                # two calls, the same bits
    for got, want, what in zip(cache, c['want'], ('k8', 'v8', 'kexp', 'vexp')):       # the appended row byte-exact, every other byte unchanged
        bad = (got != want).nonzero()
        assert bad.numel() == 0, '%s differs at %s: %s, expected %s' % (what, bad[0].tolist(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item())
    worst = 0.0
    for b, p in enumerate(c['positions']):
        if not 0 <= p < T_MAX:                                                        # an idle row: out untouched (the cache was compared above)
            assert bool((out[b] == SENT_OUT).all())
            continue
        ref = R.attention(c['qrot'][b], cache[0][b], cache[2][b], cache[1][b], cache[3][b], p + 1, SCALE)
        err = float((out[b].double() - ref).abs().max() / ref.abs().max())
        worst = max(worst, err)
        assert err < 1e-3, 'row %d (pos %d): %.3g' % (b, p, err)
    print('%s tps=%d: worst max|y - y_ref| / max|y_ref| = %.3g' % (name, tps, worst))


def test_decode_attn_kv8_scores_are_realistic():
    c = _case('B16')
    after = c['want']
    s = torch.cat([(R.dequantise(after[0][b, :p + 1], after[2][b, :p + 1]).reshape(p + 1, 2, HD) * c['qrot'][b].double().reshape(2, HD)).sum(-1).reshape(-1)
                   for b, p in enumerate(c['positions']) if 0 <= p < T_MAX]) * SCALE
    assert 2.0 <= float(s.std()) <= 3.0


@pytest.mark.parametrize('tps', [0, 32])
def test_decode_attn_kv8_out_perm(tps):
    c = _case('B3')
    H = c['heads'] * HD
    perm = torch.randperm(H, generator=torch.Generator().manual_seed(5)).to(dtype=torch.int32, device=DEV)
    (plain, _), _ = _run(c, tps)
    (moved, _), _ = _run(c, tps, perm)
    want = torch.empty_like(plain)
    want[:, perm.cpu().long()] = plain
    assert torch.equal(moved.view(torch.int16), want.view(torch.int16))


def test_kv8_store_segments():
    lib, heads, slots = _native.lib(), 2, 4
    H = heads * HD
    gen = torch.Generator().manual_seed(9)
    pad = 8                                                          # slots of the source further apart than t_max rows
    src = [R.random_rows(gen, (slots, T_MAX + pad), heads) for _ in range(2)]
    k16, v16 = (t.to(DEV) for t in src)
    segs = [(0, 37, 0, 2), (5, 1, T_MAX - 1, 0), (0, 200, 100, 3), (0, 3, 62, 1)]       # (row0: ignored, rows, start, slot)
    table = (_native.PromptSeg * len(segs))(*[_native.PromptSeg(*s) for s in segs])
    k8, v8 = (torch.full((slots, T_MAX, H), SENT_Q, dtype=torch.uint8, device=DEV) for _ in range(2))
    kexp, vexp = (torch.full((slots, T_MAX, heads), SENT_E, dtype=torch.int8, device=DEV) for _ in range(2))
    rc = lib.gptq_kv8_store_f16(k16.data_ptr(), v16.data_ptr(), (T_MAX + pad) * H, table, len(segs), k8.data_ptr(), v8.data_ptr(), kexp.data_ptr(),
                                vexp.data_ptr(), heads, HD, T_MAX, None)
    assert rc == 0
    torch.cuda.synchronize()
    for got_q, got_e, s16 in ((k8.cpu(), kexp.cpu(), src[0]), (v8.cpu(), vexp.cpu(), src[1])):
        want_q, want_e = torch.full_like(got_q, SENT_Q), torch.full_like(got_e, SENT_E)
        for _, rows, start, slot in segs:
            want_q[slot, start:start + rows], want_e[slot, start:start + rows] = R.quantise(s16[slot, start:start + rows])
        assert torch.equal(got_q, want_q) and torch.equal(got_e, want_e)
