"""GPU tests of gptq_decode_attn_beam_f16 (csrc/beam_attn.hip) through the C ABI, with the constants and helpers of tests/test_gpu_attn_chunk.py:
float64 on the fp16 values with the explicit gather K[src[b, t], t] as the reference, the op-level bar TOL, guards around cache, output and table,
NaN in every cache row the table does not reference and in every row at or past p -- a wrong slot or an over-read poisons the output."""
import functools

import numpy as np
import pytest
import torch

import attn_cases as AC
import test_gpu_attn_chunk as C
from quant import _native
from test_gpu_attn_chunk import BASE, DEV, GUARD, GUARD_BITS, H, HD, HEADS, NAN_BITS, SCALE, T_MAX
from util import rel_err, TOL

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _split_cases():
    """(common, p) per active split count 1 .. 8, the common prefix ending half way into the LAST active split"""
    lib, found = _native.lib(), {}
    for p in range(3, T_MAX, 61):
        found.setdefault(lib.gptq_decode_attn_beam_splits(HEADS, HD, T_MAX, p + 1), p)
    assert sorted(found) == list(range(1, 9)) and lib.gptq_decode_attn_beam_splits(HEADS, HD, T_MAX, T_MAX) == 8, found
    chunk = lambda p: AC.attn_split(p + 1, AC.grid_splits(HEADS, T_MAX), 256)
    return [(((n - 1) * chunk(p)[1] + p) // 2, p) for n, p in sorted(found.items())]


@functools.lru_cache(maxsize=None)
def _table(n, p, common):
    """src [n, T_MAX] of a genuine ancestry of p steps whose rows share exactly the first `common` columns: below `common` every step continues
    ONE random beam (the trunk's slot varies along t), from there on random parents with beams 0 and 1 kept apart; 0xEE at and past p"""
    rng = np.random.default_rng(97 * p + 7 * common + n)
    src = np.full((n, T_MAX), 0xEE, dtype=np.uint8)
    for t in range(p):
        src[:, t] = np.arange(n)
        par = np.full(n, rng.integers(n)) if t < common else np.concatenate([[0, 1], rng.integers(n, size=n - 2)])
        src[:, :t + 1] = src[par, :t + 1]
    assert p == 0 or common == p or ((src[:, :common] == src[0, :common]).all() and src[0, common] != src[1, common])
    return src


@functools.lru_cache(maxsize=None)
def _pool(n, sharp):
    """K / V [n, T_MAX, heads, HD] and the rotated queries [n, heads, HD].  sharp: the planted logits of attn_cases.py -- queries u + 0.3 noise,
    background keys 0.2 N(0,1), every 37th key row an amp-8 needle with a 4 x value"""
    rng = np.random.default_rng(5 + n)
    q, k, v = rng.standard_normal((n, HEADS, HD)), 0.5 * rng.standard_normal((n, T_MAX, HEADS, HD)), rng.standard_normal((n, T_MAX, HEADS, HD))
    if sharp:
        u = rng.standard_normal((HEADS, HD))
        q, k = u[None] + 0.3 * q, 0.4 * k
        k[:, 3::37] += AC.AMP / SCALE * u / (u * u).sum(-1, keepdims=True)
        v[:, 3::37] *= 4.0
    return q, k.astype(np.float16), v.astype(np.float16)


@functools.lru_cache(maxsize=2)
def _case(n, p, common, sharp=False, kq=0):
    """(qkv [n, 3 H], caches [n T_MAX, H], table): q un-rotated so that the kernel's RoPE gives the pool's queries; k x 2^kq, q x 2^-kq, v x 4^-kq"""
    src, (qt, k, v) = _table(n, p, common), _pool(n, sharp)
    new = np.random.default_rng(1000 * p + n).standard_normal((2, n, HEADS, HD))
    qkv = np.stack([AC._unrotate(qt, [p] * n) * 2.0 ** -kq, 0.5 * new[0] * 2.0 ** kq, new[1] * 4.0 ** -kq], axis=1).reshape(n, 3 * H).astype(np.float16)
    live = np.zeros((n, T_MAX), dtype=bool)
    live[src[:, :p], np.arange(p)[None, :]] = True
    nan = np.uint16(NAN_BITS).view(np.float16)
    kc = np.where(live[..., None, None], k * np.float16(2.0 ** kq), nan).reshape(n * T_MAX, H)
    vc = np.where(live[..., None, None], v * np.float16(4.0 ** -kq), nan).reshape(n * T_MAX, H)
    return qkv, kc, vc, src


def _framed(a, bits=GUARD_BITS):
    """the host image of an array between its guard rows (C._guarded) or guard bytes"""
    g = np.full((GUARD,) + a.shape[1:], bits, dtype=a.dtype)
    return np.concatenate([g, a, g])


def _run(n, p, case, common, perm=None, ws=None):
    """one call on guarded allocations; returns the raw allocations on the host"""
    lib = _native.lib()
    qkv, kc, vc, src = case
    qd, kd, vd = C._dev(qkv), C._guarded(kc), C._guarded(vc)
    od = C._guarded(np.full((n, H), NAN_BITS, dtype=np.uint16).view(np.float16))
    sd = C._dev(_framed(src.reshape(-1), 0x5A))
    pos, cm = torch.tensor([p], dtype=torch.int64, device=DEV), torch.tensor([common], dtype=torch.int32, device=DEV)
    pd = None if perm is None else C._dev(perm.astype(np.int32))
    if ws is None:
        ws = torch.empty(lib.gptq_decode_attn_beam_ws_bytes(n, HEADS, T_MAX), dtype=torch.uint8, device=DEV).fill_(0xA5)
    rc = lib.gptq_decode_attn_beam_f16(qd.data_ptr(), 3 * H, n, pos.data_ptr(), kd[GUARD:].data_ptr(), vd[GUARD:].data_ptr(), T_MAX * H,
                                       sd[GUARD:].data_ptr(), cm.data_ptr(), od[GUARD:].data_ptr(), H, _native.ptr(pd), ws.data_ptr(), ws.numel(),
                                       HEADS, HD, T_MAX, BASE, SCALE, None, torch.cuda.current_stream().cuda_stream)
    _native.check(rc, 'gptq_decode_attn_beam_f16')
    torch.cuda.synchronize()
    assert np.array_equal(C._bits(qd), qkv.view(np.uint16)), 'qkv was modified'
    return dict(kc=C._bits(kd), vc=C._bits(vd), out=C._bits(od), src=sd.cpu().numpy())


def _check(n, p, case, res):
    """appended rows bit for bit against gptq_decode_rope_kv_f16, src[b, p] = b, every other byte of cache, table and guards as before, the
    output against float64 with the explicit gather; returns the float64 result"""
    qkv, kc, vc, src = case
    want = {'kc': _framed(kc.view(np.uint16)), 'vc': _framed(vc.view(np.uint16)), 'src': _framed(src.reshape(-1), 0x5A)}
    q_rot = np.zeros((n, H), dtype=np.float16)
    for b in range(n):                                       # beam b's token appended to a one-slot cache by the token-by-token entry
        qr, k1, v1 = C._row_by_row(qkv[b:b + 1], kc[b * T_MAX:(b + 1) * T_MAX], vc[b * T_MAX:(b + 1) * T_MAX], p)
        q_rot[b] = qr[0]
        want['kc'][GUARD + b * T_MAX + p], want['vc'][GUARD + b * T_MAX + p] = k1[p].view(np.uint16), v1[p].view(np.uint16)
        want['src'][GUARD + b * T_MAX + p] = b
    for name in ('kc', 'vc', 'src'):
        assert np.array_equal(res[name], want[name]), name + ': more or other bytes than the appended rows changed'
    o = res['out']
    assert (o[:GUARD] == GUARD_BITS).all() and (o[GUARD + n:] == GUARD_BITS).all(), 'out guard rows written'
    tab = want['src'][GUARD:GUARD + n * T_MAX].reshape(n, T_MAX)[:, :p + 1].astype(np.int64)
    rows = tab * T_MAX + np.arange(p + 1)[None, :]           # [n, p + 1] cache rows of the explicit gather
    K, V = (want[c][GUARD:GUARD + n * T_MAX].view(np.float16)[rows].reshape(n, p + 1, HEADS, HD).astype(np.float64) for c in ('kc', 'vc'))
    s = np.einsum('bhd,bthd->bht', q_rot.reshape(n, HEADS, HD).astype(np.float64), K) * SCALE
    e = np.exp(s - s.max(-1, keepdims=True))
    exact = np.einsum('bht,bthd->bhd', e / e.sum(-1, keepdims=True), V).reshape(n, H)
    got = o[GUARD:GUARD + n].view(np.float16)
    assert np.isfinite(got.astype(np.float32)).all(), 'a NaN row was read'
    err = rel_err(got, exact)
    print('N %d p %d: rel err %.3e' % (n, p, err))
    assert err < TOL, err
    return exact


PAIRS = [(0, 0), (40, 40), (0, 70), (45, 83), (1000, T_MAX - 1)]


@pytest.mark.parametrize('n', [2, 5, 16])
@pytest.mark.parametrize('pair', list(range(len(PAIRS))) + ['split%d' % i for i in range(1, 9)])
def test_beam_attention(n, pair):
    common, p = _split_cases()[int(pair[5:]) - 1] if isinstance(pair, str) else PAIRS[pair]
    case = _case(n, p, common)
    ws = torch.empty(_native.lib().gptq_decode_attn_beam_ws_bytes(n, HEADS, T_MAX), dtype=torch.uint8, device=DEV).fill_(0xA5)
    first, second = _run(n, p, case, common, ws=ws), _run(n, p, case, common, ws=ws)
    _check(n, p, case, first)
    for name in first:
        assert np.array_equal(first[name], second[name]), 'a second call on the same workspace differs in ' + name


@pytest.mark.parametrize('kq', [0, 3, -3])
def test_sharp_logits_and_power_of_two_scales(kq):
    """planted amp-8 keys in trunk and tail; k x 2^kq, q x 2^-kq (the same logits), v x 4^-kq"""
    for common, p in ((45, 83), _split_cases()[-1]):
        case = _case(5, p, common, True, kq)
        exact = _check(5, p, case, _run(5, p, case, common))
        assert np.abs(exact).max() * 4.0 ** kq > 1.0          # a needle holds the weight: the output is a 4 x value row


@pytest.mark.parametrize('n', [5, 16])
def test_smaller_common_out_perm_and_idle_positions(n):
    common, p = _split_cases()[2]                            # three splits, the true prefix ends in the last
    case = _case(n, p, common)
    for given in (0, common // 2):                           # keys move from the shared path to the gathered one
        _check(n, p, case, _run(n, p, case, given))
    base, perm = _run(n, p, case, common), np.random.default_rng(3).permutation(H)
    res = _run(n, p, case, common, perm=perm)
    assert np.array_equal(res['out'][GUARD:GUARD + n][:, perm], base['out'][GUARD:GUARD + n])
    assert np.array_equal(res['kc'], base['kc']) and np.array_equal(res['src'], base['src'])
    for idle in (-1, T_MAX, 2 ** 40):                        # nothing is read or written
        res = _run(n, idle, case, common)
        assert np.array_equal(res['out'], _framed(np.full((n, H), NAN_BITS, dtype=np.uint16)))
        assert all(np.array_equal(res[c], _framed(a.view(np.uint16))) for c, a in (('kc', case[1]), ('vc', case[2])))
        assert np.array_equal(res['src'][GUARD:-GUARD], case[3].reshape(-1))
