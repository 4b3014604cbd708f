"""gptq_decode_attn_batch_gqa_f16 (csrc/decode_attn_gqa.hip) through the C entry, on inputs made as tests/attn_cases.py makes them: per K/V head a
direction u, a planted key whose logit lies 8 natural-log units above a 0.2-sigma background, and per query head of the group the raw query
R(p)^-1 (u + noise).  The reference is float64: RoPE (the device's rotated q and appended k are held to the RoPE bar), then softmax attention
over the appended cache per query head h with K/V head h // G, judged elementwise by the bar attn_cases applies to gptq_decode_attn_batch_f16
(kind 'stream').  The appended cache row must carry the bits gptq_decode_attn_batch_f16 appends."""
import numpy as np
import pytest
import torch

import attn_cases as AC
import rope_cases as RC
from quant import _native

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HD, BASE, SCALE = AC.HD, AC.BASE, AC.SCALE
GUARD, GUARD_BITS, NAN_BITS = 8, 0x5A5A, AC.NAN_BITS
GQA_TPS = 128                # tokens a split owns at least (GA_TPS of the kernel)
SHAPES = [(4, 2), (6, 2), (7, 1), (8, 1), (16, 1)]       # G = 2, 3, 7, 8 and a full 16-column tile
T_MAX = 64


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).to(DEV)


def _guarded(a):
    """a [n][c] uint16 inside an allocation with GUARD rows of GUARD_BITS before and behind"""
    full = np.full((a.shape[0] + 2 * GUARD, a.shape[1]), GUARD_BITS, dtype=np.uint16)
    full[GUARD:-GUARD] = a
    return _dev(full).view(torch.float16)


def _inner(t):
    a = t.cpu().numpy().view(np.uint16)
    assert (a[:GUARD] == GUARD_BITS).all() and (a[-GUARD:] == GUARD_BITS).all(), 'guard rows written'
    return a[GUARD:-GUARD]


def make_row(heads, kv, pos, t_max, key=None):
    """(qkv row [(heads + 2 kv) HD] fp16, the attn_cases case of the kv heads, needle on cache row `key`; None: pos // 2, at pos 0 the token's own
    key): the group's queries are the case's query plus noise of their own"""
    needle = ('history', pos // 2 if key is None else key) if pos > 0 else ('self', 0)
    c = AC.build_case(pos, 1, t_max, kv, needle=needle)
    q_kv = c.qkv[0, :kv * HD].reshape(kv, HD).astype(np.float64)
    noise = AC._unrotate(0.3 * np.random.default_rng(1000 * heads + pos).standard_normal((1, heads, HD)), [pos])[0]
    q = (np.repeat(q_kv, heads // kv, axis=0) + noise).astype(np.float16)
    return np.concatenate([q.reshape(-1), c.qkv[0, kv * HD:]]), c


def ungrouped(q_raw, c, kv, t_max):
    """what the library's ungrouped entries make of the same token: the rotated queries (gptq_decode_rope_kv_f16 on a scratch row [q | q | q]) and
    cache row c.start of K and V as gptq_decode_attn_batch_f16 appends it for the same k / v heads"""
    lib, s = _native.lib(), torch.cuda.current_stream().cuda_stream
    heads, H = q_raw.shape[0], kv * HD
    p = torch.tensor([c.start], dtype=torch.int64, device=DEV)
    row = _dev(np.tile(q_raw.reshape(-1), 3))
    kd, vd = (torch.zeros((t_max, heads * HD), dtype=torch.float16, device=DEV) for _ in range(2))
    _native.check(lib.gptq_decode_rope_kv_f16(row.data_ptr(), p.data_ptr(), kd.data_ptr(), vd.data_ptr(), heads, HD, t_max, BASE, s), 'rope_kv')
    qd, kd, vd, od = _dev(c.qkv), _dev(c.kc), _dev(c.vc), torch.zeros((1, H), dtype=torch.float16, device=DEV)
    nb = lib.gptq_decode_attn_batch_workspace_bytes(1, kv, HD, t_max)
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    _native.check(lib.gptq_decode_attn_batch_f16(qd.data_ptr(), 3 * H, p.data_ptr(), kd.data_ptr(), vd.data_ptr(), od.data_ptr(), H, ws.data_ptr(), nb, 1, kv,
                                                 HD, t_max, BASE, c.scale, None, None, s), 'gptq_decode_attn_batch_f16')
    return row.cpu().numpy()[:heads * HD].reshape(1, heads, HD), kd[c.start].cpu().numpy().view(np.uint16), vd[c.start].cpu().numpy().view(np.uint16)


def run_gqa(rows, caches, positions, heads, kv, t_max, perm=None, out_before=None):
    """one call on B rows: (out [B, heads HD], K, V [B t_max, kv HD]) as uint16, guards checked; the workspace is poisoned"""
    lib = _native.lib()
    B, H = len(rows), heads * HD
    qd = _dev(np.stack(rows).view(np.uint16)).view(torch.float16)
    kd, vd = (_guarded(np.concatenate([c[i] for c in caches]).view(np.uint16)) for i in (0, 1))
    od = _guarded(np.full((B, H), NAN_BITS, dtype=np.uint16) if out_before is None else out_before)
    p = torch.tensor(positions, dtype=torch.int64, device=DEV)
    nb = lib.gptq_decode_attn_batch_gqa_workspace_bytes(B, heads, kv, HD, t_max)
    assert nb > 0
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=DEV)
    pd = None if perm is None else _dev(perm.astype(np.int32))
    rc = lib.gptq_decode_attn_batch_gqa_f16(qd.data_ptr(), qd.stride(0), p.data_ptr(), kd[GUARD:].data_ptr(), vd[GUARD:].data_ptr(), od[GUARD:].data_ptr(), H,
                                            ws.data_ptr(), nb, B, heads, kv, HD, t_max, BASE, SCALE, None, None if pd is None else pd.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)
    _native.check(rc, 'gptq_decode_attn_batch_gqa_f16')
    torch.cuda.synchronize()
    assert np.array_equal(qd.cpu().numpy().view(np.uint16), np.stack(rows).view(np.uint16)), 'qkv was modified'
    return _inner(od), _inner(kd), _inner(vd)


def judge(out_row, K_after, V_after, row, c, heads, kv, t_max, ranges=None):
    """one row of a call against the float64 reference: the caches (only row pos changed, and to the bits of the ungrouped entry; k within the
    RoPE bar), then every output element within its bar"""
    pos, n, G = c.start, c.start + 1, heads // kv
    K, V = K_after.reshape(t_max, kv, HD), V_after.reshape(t_max, kv, HD)
    for after, before in ((K, c.kc), (V, c.vc)):
        before = before.view(np.uint16).reshape(t_max, kv, HD)
        assert np.array_equal(after[:pos], before[:pos]) and np.array_equal(after[n:], before[n:]), 'rows other than the appended one changed'
    q_raw = row[:heads * HD].reshape(heads, HD)
    q_rot, k_want, v_want = ungrouped(q_raw, c, kv, t_max)
    assert np.array_equal(K[pos].reshape(-1), k_want) and np.array_equal(V[pos].reshape(-1), v_want), 'appended row differs from the ungrouped entry'
    assert np.array_equal(v_want, row[(heads + kv) * HD:].view(np.uint16)), 'appended v'
    RC.assert_heads_close(q_rot, q_raw[None], np.array([pos]), HD, BASE, 'rotated q')
    RC.assert_heads_close(K[pos:n].view(np.float16), row[heads * HD:(heads + kv) * HD].reshape(1, kv, HD), np.array([pos]), HD, BASE, 'appended k')
    Kg, Vg = (np.repeat(a[:n].view(np.float16), G, axis=1) for a in (K, V))          # query head h attends over K/V head h // G
    st = AC.attention_stats(q_rot, Kg, Vg, pos, SCALE)
    nsp, span = AC.span_of(ranges) if ranges else (1, None)
    return AC.assert_attn_close(out_row.view(np.float16), st, 'stream', nsp, span, name='gqa %d/%d pos %d' % (heads, kv, pos))


@pytest.mark.parametrize('pos', [0, 1, 15, 16, 31, 32, 33, T_MAX - 1])
@pytest.mark.parametrize('heads,kv', SHAPES)
def test_one_row(heads, kv, pos):
    row, c = make_row(heads, kv, pos, T_MAX)
    out, K, V = run_gqa([row], [(c.kc, c.vc)], [pos], heads, kv, T_MAX)
    print('worst err/bar %.3f' % judge(out[0], K, V, row, c, heads, kv, T_MAX))
    again = run_gqa([row], [(c.kc, c.vc)], [pos], heads, kv, T_MAX)
    assert all(np.array_equal(a, b) for a, b in zip((out, K, V), again)), 'a second call on the same inputs gave other bits'


@pytest.mark.parametrize('heads,kv', SHAPES)
def test_three_rows_and_an_idle_one(heads, kv):
    positions = [33, -1, 0, T_MAX - 1]
    made = [make_row(heads, kv, max(p, 0), T_MAX) for p in positions]
    rows = [r for r, _ in made]
    rows[1] = np.full_like(rows[1], np.uint16(NAN_BITS).view(np.float16))          # the idle row: whatever it holds is never read
    out0 = np.full((4, heads * HD), NAN_BITS, dtype=np.uint16)
    out0[1] = 0x1234
    out, K, V = run_gqa(rows, [(c.kc, c.vc) for _, c in made], positions, heads, kv, T_MAX, out_before=out0)
    for b, (row, c) in enumerate(made):
        sl = slice(b * T_MAX, (b + 1) * T_MAX)
        if positions[b] < 0:
            assert (out[b] == 0x1234).all() and np.array_equal(K[sl], c.kc.view(np.uint16)) and np.array_equal(V[sl], c.vc.view(np.uint16)), 'idle row touched'
        else:
            judge(out[b], K[sl], V[sl], row, c, heads, kv, T_MAX)


# t_max 384.  (heads, kv, batch, pos, planted key): the batch is one live row and idle ones -- it shapes the grid: S = min(256 / (kv batch), 3).
#   6/2 and 7/1 alone: three splits of 128 keys, one tile per wave; the key is the last of one split or the first of the next
#   16/8 x 16: two splits of 256 keys, TWO tiles per wave (the rescale between tiles, both register sets, the LDS image reused); the key in
#              wave 0's first tile, in its second, and in the second split
#   32/16 x 16: one split of 384 (300) keys, THREE tiles per wave (the first register set requested again): the key in each of wave 0's tiles,
#              and in a wave's last, partly filled tile
LONG = [(6, 2, 1, 299, 127), (6, 2, 1, 299, 128), (7, 1, 1, 383, 255), (7, 1, 1, 383, 256),
        (16, 8, 16, 383, 5), (16, 8, 16, 383, 133), (16, 8, 16, 299, 260),
        (32, 16, 16, 383, 5), (32, 16, 16, 383, 133), (32, 16, 16, 383, 261), (32, 16, 16, 299, 290)]


@pytest.mark.parametrize('heads,kv,batch,pos,key', LONG)
def test_long_rows(heads, kv, batch, pos, key):
    t_max = 384
    ranges = AC.split_ranges(pos + 1, AC.grid_splits(kv, t_max, batch), GQA_TPS)
    assert len(ranges) == {1: 3, 16: 256 // (16 * kv)}[batch]
    row, c = make_row(heads, kv, pos, t_max, key)
    idle = (np.zeros_like(c.kc), np.zeros_like(c.vc))
    args = ([row] * batch, [(c.kc, c.vc)] + [idle] * (batch - 1), [pos] + [-1] * (batch - 1), heads, kv, t_max)
    out, K, V = run_gqa(*args)
    judge(out[0], K[:t_max], V[:t_max], row, c, heads, kv, t_max, ranges)
    assert (out[1:] == NAN_BITS).all() and not K[t_max:].any() and not V[t_max:].any(), 'idle rows touched'
    assert all(np.array_equal(a, b) for a, b in zip((out, K, V), run_gqa(*args))), 'a second call on the same inputs gave other bits'


def test_out_perm_stores_element_n_at_perm_n():
    heads, kv, pos = 6, 2, 33
    row, c = make_row(heads, kv, pos, T_MAX)
    plain = run_gqa([row], [(c.kc, c.vc)], [pos], heads, kv, T_MAX)[0]
    perm = np.random.default_rng(3).permutation(heads * HD)
    permuted = run_gqa([row], [(c.kc, c.vc)], [pos], heads, kv, T_MAX, perm=perm)[0]
    assert np.array_equal(permuted[0][perm], plain[0])
