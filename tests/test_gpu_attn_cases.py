"""GPU tests of every attention entry on the planted-key cases of tests/attn_cases.py: one key, one row, one split edge or the softmax scale
decides the result, and every output element is held to its own bar (attn_cases.attn_bound, derived from the kernels' rounding points) -- never
to a maximum over the output.  tests/test_host_attn.py shows on the CPU that fp32 models of the kernels sit inside that bar on these very
cases and that a dropped, doubled, stale or leaked key, a forgotten split maximum, a rescale that misses the accumulator and an ignored scale
argument are thrown out by ten times the bar or more.

The reference is float64 attention on the device's own values: q_rot from gptq_decode_rope_kv_f16 row by row, K and V read back from the caches
after the call (whose appended rows are checked on their own: v to the bit, k within the RoPE bar of tests/rope_cases.py).  Calling conventions,
guard rows and NaN tails are those of the existing attention tests (the small helpers are copies).  Entries: the prompt entry and its batch
entry (t_max 384), the chunk entry and its batch entry (t_max 1930), and the decode entries (t_max 2048): the partial + combine pair, the fused
launch with and without the table, the batch entry, the split records merged on the host, and the records merged by o_proj's decode kernel."""
import functools

import numpy as np
import pytest
import torch

import attn_cases as AC
import rope_cases as RC
from quant import _native
from util import TOL, make_random_layer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HD, BASE = AC.HD, AC.BASE
GUARD = 64                   # guard rows in front of and behind every cache / output allocation
GUARD_BITS = 0x5A5A          # their bit pattern (fp16 209.25)
NAN_BITS = AC.NAN_BITS       # fp16 NaN: cache rows behind the call's own, padding, the output before the call
WORST = {}                   # (kernel, family) -> worst err / bar seen in this run
_FRESH = set()               # ... the keys touched since the last report


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).to(DEV)      # (a copy: the shared inputs are read-only)


def _bits(t):
    return t.cpu().numpy().view(np.uint16)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(a, cols=None):
    """a [n][c] inside an allocation with GUARD rows of GUARD_BITS before and behind (and, with cols > c, NaN padding behind every row)"""
    n, c = a.shape
    cols = c if cols is None else cols
    full = np.full((n + 2 * GUARD, cols), GUARD_BITS, dtype=np.uint16)
    full[GUARD:GUARD + n] = NAN_BITS
    full[GUARD:GUARD + n, :c] = a.view(np.uint16)
    return _dev(full).view(torch.float16)


def _inner(t, n):
    """rows GUARD .. GUARD + n of a guarded allocation as an fp16 array, after checking the guard rows"""
    a = _bits(t)
    assert (a[:GUARD] == GUARD_BITS).all() and (a[GUARD + n:] == GUARD_BITS).all(), 'guard rows written'
    return a[GUARD:GUARD + n].view(np.float16)


@functools.lru_cache(maxsize=None)
def _rope_table(t_max):
    tab = torch.empty((t_max, HD // 2, 2), dtype=torch.float32, device=DEV)
    _native.check(_native.lib().gptq_rope_table_f32(tab.data_ptr(), t_max, HD, BASE, _stream()), 'rope_table')
    return tab


@functools.lru_cache(maxsize=None)
def _q_rot(start, rows, t_max, heads):
    """the rotated queries of a shape, from gptq_decode_rope_kv_f16 fed row by row (the queries of a shape are the same for every needle, amplitude
    and scale: _judge checks that): [rows, heads, HD] fp16 and the unrotated q part they belong to"""
    lib = _native.lib()
    case = AC.build_case(start, rows, t_max, heads)
    H = heads * HD
    qd = _dev(case.qkv)
    kd, vd = (torch.zeros((t_max, H), dtype=torch.float16, device=DEV) for _ in range(2))
    pos = torch.arange(start, start + rows, dtype=torch.int64, device=DEV)
    for r in range(rows):
        _native.check(lib.gptq_decode_rope_kv_f16(qd[r].data_ptr(), pos[r:].data_ptr(), kd.data_ptr(), vd.data_ptr(), heads, HD, t_max, BASE, _stream()), 'rope_kv')
    torch.cuda.synchronize()
    q = qd.cpu().numpy()[:, :H].reshape(rows, heads, HD)
    q.setflags(write=False)
    return q, case.qkv[:, :H]


def _judge(kernel, family, case, out, kc_after, vc_after, kind, ranges=None):
    """the caches after the call (history untouched, tail still NaN, v rows to the bit, k rows within the RoPE bar), then every output element
    against its bar of float64 attention on those caches; returns (worst err / bar, the reference)"""
    c = case
    H, n = c.heads * HD, c.start + c.rows
    ka, va = np.ascontiguousarray(kc_after).view(np.uint16), np.ascontiguousarray(vc_after).view(np.uint16)
    assert np.array_equal(ka[:c.start], c.kc.view(np.uint16)[:c.start]) and np.array_equal(va[:c.start], c.vc.view(np.uint16)[:c.start]), 'history changed'
    assert (ka[n:] == NAN_BITS).all() and (va[n:] == NAN_BITS).all(), 'rows behind the call written'
    x = c.qkv.reshape(c.rows, 3, c.heads, HD)
    assert np.array_equal(va[c.start:n], x[:, 2].reshape(c.rows, H).view(np.uint16)), 'appended v rows'
    K, V = kc_after[:n].reshape(n, c.heads, HD), vc_after[:n].reshape(n, c.heads, HD)
    RC.assert_heads_close(K[c.start:], x[:, 1], c.start + np.arange(c.rows), HD, BASE, 'appended k rows')
    q_rot, q_raw = _q_rot(c.start, c.rows, c.t_max, c.heads)
    assert np.array_equal(q_raw.view(np.uint16), c.qkv[:, :H].view(np.uint16))
    st = AC.attention_stats(q_rot, K, V, c.start, c.scale)
    if c.needle is not None:
        w = st.w[:, :, c.key]
        assert (w[:c.first_row] == 0.0).all() and (w[c.first_row:] >= 0.3).all(), (c.name, 'needle weight', float(w[c.first_row:].min()))
    nsp, span = AC.span_of(ranges) if ranges else (1, None)
    r = AC.assert_attn_close(out, st, kind, nsp, span, name='%s, %s' % (kernel, c.name))
    WORST[(kernel, family)] = max(WORST.get((kernel, family), 0.0), r)
    _FRESH.add((kernel, family))
    return r, st


def _report():
    """worst err / bar so far of every (kernel, family) the test touched"""
    for k, family in sorted(_FRESH):
        print('%-14s %-10s worst err/bar %.3f' % (k, family, WORST[(k, family)]))
    _FRESH.clear()


def test_the_split_rule_port_matches_the_library():
    lib = _native.lib()
    for batch in (1, 5):
        assert lib.gptq_decode_attn_splits(batch, AC.DECODE_HEADS, HD, AC.DECODE_T_MAX) == AC.grid_splits(AC.DECODE_HEADS, AC.DECODE_T_MAX, batch)
    for length in list(range(1, AC.CHUNK_T_MAX + 1, 37)) + [255, 256, 257, 300, 1792, 1793, AC.CHUNK_T_MAX]:
        assert lib.gptq_decode_attn_chunk_splits(AC.CHUNK_HEADS, HD, AC.CHUNK_T_MAX, length) == AC.attn_split(length, AC.chunk_cap(), AC.CHUNK_TPS)[0], length
    for rows in AC.CHUNK_ROWS:
        pos = AC.chunk_positions(rows)
        assert [AC.attn_split(pos[w] + rows, AC.chunk_cap(), AC.CHUNK_TPS)[0] for w in ('one', 'two', 'deep')] == [1, 2, AC.ATT_MAX_SPLITS]


# ---------------------------------------------------------------------------------------------------------------------------------
# the prompt entry and its batch entry
# ---------------------------------------------------------------------------------------------------------------------------------
def _prompt(case, table=False):
    """gptq_prompt_attn_f16 on guarded allocations: (out [rows, H], k cache, v cache [t_max, H]) fp16 on the host"""
    c = case
    lib = _native.lib()
    H = c.heads * HD
    qd = _dev(c.qkv)
    kd, vd = _guarded(c.kc), _guarded(c.vc)
    od = _guarded(np.full((c.rows, H), NAN_BITS, dtype=np.uint16).view(np.float16))
    ws = torch.empty(lib.gptq_prompt_attn_workspace_bytes(c.rows, c.heads, HD, c.t_max), dtype=torch.uint8, device=DEV)
    tab = _rope_table(c.t_max) if table else None
    rc = lib.gptq_prompt_attn_f16(qd.data_ptr(), 3 * H, c.rows, c.start, kd[GUARD:].data_ptr(), vd[GUARD:].data_ptr(), od[GUARD:].data_ptr(), H,
                                  ws.data_ptr(), ws.numel(), c.heads, HD, c.t_max, BASE, c.scale, _native.ptr(tab), _stream())
    _native.check(rc, 'gptq_prompt_attn_f16')
    torch.cuda.synchronize()
    assert np.array_equal(_bits(qd), c.qkv.view(np.uint16)), 'qkv was modified'
    return _inner(od, c.rows), _inner(kd, c.t_max), _inner(vd, c.t_max)


def _prompt_case(start, rows, **kw):
    return AC.build_case(start, rows, AC.PROMPT_T_MAX, AC.PROMPT_HEADS, **kw)


@pytest.mark.parametrize('start,rows', AC.PROMPT_SHAPES)
def test_prompt_needles(start, rows):
    """a needle on history rows 0, 63, 64, 127, 128, start - 1, on chunk rows 0, 31, 32, 63, 64, rows - 1 (the rows below stay inside THEIR bar: a
    leak would exceed it a thousandfold) and on the last row's own key"""
    for needle in AC.prompt_needles(start, rows):
        case = _prompt_case(start, rows, needle=needle)
        _judge('prompt', needle[0], case, *_prompt(case), 'prompt')
    _report()


@pytest.mark.parametrize('start,rows', AC.PROMPT_SINK_SHAPES)
def test_prompt_sink(start, rows):
    """key 0 at 12, 16 and 20 above the rest: every later p is an fp16 subnormal or zero relative to the one running maximum"""
    for amp in AC.SINK_AMPS:
        case = _prompt_case(start, rows, needle=AC.sink_needle(start), amp=amp)
        _judge('prompt', 'sink %g' % amp, case, *_prompt(case), 'prompt')
    _report()


@pytest.mark.parametrize('scale', AC.SCALES)
@pytest.mark.parametrize('start,rows', AC.PROMPT_SCALE_SHAPES)
def test_prompt_scale(start, rows, scale):
    for needle, amp in AC.scale_patterns(start, rows):
        case = _prompt_case(start, rows, scale=scale, needle=needle, amp=amp)
        res = _prompt(case)
        _judge('prompt', 'scale', case, *res, 'prompt')
        res_t = _prompt(case, table=True)
        assert all(np.array_equal(a.view(np.uint16), b.view(np.uint16)) for a, b in zip(res, res_t)), 'table variant differs'
    _report()


@pytest.mark.parametrize('scale', AC.SCALES)
def test_prompt_batch_segments(scale):
    """the five segments of tests/test_gpu_prompt_attn_batch.py in one call, a different pattern per segment, each held to the bar on its own"""
    lib = _native.lib()
    heads, t_max = AC.PROMPT_HEADS, AC.PROMPT_T_MAX
    H = heads * HD
    cases = [_prompt_case(start, rows, scale=scale, needle=needle, amp=amp) for start, rows, needle, amp in AC.prompt_segment_patterns()]
    assert tuple((c.start, c.rows) for c in cases) == AC.PROMPT_SEGS
    total = sum(c.rows for c in cases)
    qf = np.concatenate([c.qkv for c in cases])
    kf = np.full((2 * GUARD + len(cases) * t_max, H), GUARD_BITS, dtype=np.uint16)
    vf = kf.copy()
    layout, r0 = [], 0
    for i, c in enumerate(cases):
        kf[GUARD + i * t_max:GUARD + (i + 1) * t_max] = c.kc.view(np.uint16)
        vf[GUARD + i * t_max:GUARD + (i + 1) * t_max] = c.vc.view(np.uint16)
        layout.append((r0, c.rows, c.start, i))
        r0 += c.rows
    qd, kd, vd = _dev(qf), _dev(kf).view(torch.float16), _dev(vf).view(torch.float16)
    od = _guarded(np.full((total, H), NAN_BITS, dtype=np.uint16).view(np.float16))
    ws = torch.empty(lib.gptq_prompt_attn_workspace_bytes(total, heads, HD, t_max), dtype=torch.uint8, device=DEV)
    segs = (_native.PromptSeg * len(layout))(*[_native.PromptSeg(*e) for e in layout])
    rc = lib.gptq_prompt_attn_batch_f16(qd.data_ptr(), 3 * H, total, segs, len(layout), kd[GUARD:].data_ptr(), vd[GUARD:].data_ptr(), t_max * H,
                                        od[GUARD:].data_ptr(), H, ws.data_ptr(), ws.numel(), heads, HD, t_max, BASE, scale, None, _stream())
    _native.check(rc, 'gptq_prompt_attn_batch_f16')
    torch.cuda.synchronize()
    out = _inner(od, total)
    ka, va = _inner(kd, len(cases) * t_max), _inner(vd, len(cases) * t_max)
    for (r0, n, _, i), c in zip(layout, cases):
        _judge('prompt batch', 'segment', c, out[r0:r0 + n], ka[i * t_max:(i + 1) * t_max], va[i * t_max:(i + 1) * t_max], 'prompt')
    _report()


# ---------------------------------------------------------------------------------------------------------------------------------
# the chunk entry and its batch entry
# ---------------------------------------------------------------------------------------------------------------------------------
SLOT_GUARD = 48              # guard rows behind every slot of the batch entry: slot_stride = (T_MAX + SLOT_GUARD) * H


def _chunk_case(p, rows, **kw):
    return AC.build_case(p, rows, AC.CHUNK_T_MAX, AC.CHUNK_HEADS, **kw)


def _chunk_ranges(case):
    return AC.split_ranges(case.start + case.rows, AC.chunk_cap(), AC.CHUNK_TPS)


def _chunk(cases, table=False):
    """gptq_decode_attn_chunk_f16 (one case) or gptq_decode_attn_chunk_batch_f16 (several, the same row count and scale, guard rows between the
    slots): [(out [rows, H], k cache, v cache [T_MAX, H])] per case"""
    lib = _native.lib()
    B, rows, heads, t_max, scale = len(cases), cases[0].rows, cases[0].heads, cases[0].t_max, cases[0].scale
    assert all((c.rows, c.heads, c.t_max, c.scale) == (rows, heads, t_max, scale) for c in cases)
    H = heads * HD
    srows = t_max + SLOT_GUARD
    qd = _dev(np.concatenate([c.qkv for c in cases]))
    kf = np.full((2 * GUARD + B * srows, H), GUARD_BITS, dtype=np.uint16)
    vf = kf.copy()
    for b, c in enumerate(cases):
        kf[GUARD + b * srows:GUARD + b * srows + t_max] = c.kc.view(np.uint16)
        vf[GUARD + b * srows:GUARD + b * srows + t_max] = c.vc.view(np.uint16)
    kd, vd = _dev(kf).view(torch.float16), _dev(vf).view(torch.float16)
    od = _guarded(np.full((B * rows, H), NAN_BITS, dtype=np.uint16).view(np.float16))
    pos = torch.tensor([c.start for c in cases], dtype=torch.int64, device=DEV)
    tab = _native.ptr(_rope_table(t_max) if table else None)
    if B == 1:
        ws = torch.empty(lib.gptq_decode_attn_chunk_workspace_bytes(rows, heads, HD, t_max), dtype=torch.uint8, device=DEV).fill_(0xA5)
        rc = lib.gptq_decode_attn_chunk_f16(qd.data_ptr(), 3 * H, rows, pos.data_ptr(), kd[GUARD:].data_ptr(), vd[GUARD:].data_ptr(), od[GUARD:].data_ptr(),
                                            H, ws.data_ptr(), ws.numel(), heads, HD, t_max, BASE, scale, tab, _stream())
    else:
        ws = torch.empty(lib.gptq_decode_attn_chunk_batch_workspace_bytes(B, rows, heads, HD, t_max), dtype=torch.uint8, device=DEV).fill_(0xA5)
        rc = lib.gptq_decode_attn_chunk_batch_f16(qd.data_ptr(), 3 * H, B, rows, pos.data_ptr(), kd[GUARD:].data_ptr(), vd[GUARD:].data_ptr(), srows * H,
                                                  od[GUARD:].data_ptr(), H, ws.data_ptr(), ws.numel(), heads, HD, t_max, BASE, scale, tab, _stream())
    _native.check(rc, 'gptq_decode_attn_chunk%s_f16' % ('' if B == 1 else '_batch'))
    torch.cuda.synchronize()
    assert pos.tolist() == [c.start for c in cases]
    out = _inner(od, B * rows)
    ka, va = _bits(kd), _bits(vd)
    res = []
    for a in (ka, va):
        assert (a[:GUARD] == GUARD_BITS).all() and (a[GUARD + B * srows:] == GUARD_BITS).all(), 'guard rows written'
    for b in range(B):
        lo = GUARD + b * srows
        for a in (ka, va):
            assert (a[lo + t_max:lo + srows] == GUARD_BITS).all(), 'guard rows behind a slot written'
        res.append((out[b * rows:(b + 1) * rows], ka[lo:lo + t_max].view(np.float16), va[lo:lo + t_max].view(np.float16)))
    return res


@pytest.mark.parametrize('rows', AC.CHUNK_ROWS)
def test_chunk_needles(rows):
    """the maximum split count (and, with 5 rows, one and two splits): needles on keys 0, 31, 32, the first and last key of split 1 and of the
    last split, p - 1, chunk rows 0 and rows - 1, and the last row's own key"""
    pos = AC.chunk_positions(rows)
    for which in (('one', 'two', 'deep') if rows == 5 else ('deep',)):
        for needle in AC.chunk_needles(pos[which], rows):
            case = _chunk_case(pos[which], rows, needle=needle)
            _judge('chunk', needle[0], case, *_chunk([case])[0], 'chunk', _chunk_ranges(case))
    _report()


def test_chunk_sink():
    p = AC.chunk_positions(5)['deep']
    for amp in AC.SINK_AMPS:
        case = _chunk_case(p, 5, needle=('history', 0), amp=amp)
        _judge('chunk', 'sink %g' % amp, case, *_chunk([case])[0], 'chunk', _chunk_ranges(case))
    _report()


@pytest.mark.parametrize('scale', AC.SCALES)
@pytest.mark.parametrize('which', ['one', 'deep'])
def test_chunk_scale(which, scale):
    p = AC.chunk_positions(5)[which]
    for needle, amp in AC.scale_patterns(p, 5):
        case = _chunk_case(p, 5, scale=scale, needle=needle, amp=amp)
        res = _chunk([case])[0]
        _judge('chunk', 'scale', case, *res, 'chunk', _chunk_ranges(case))
        res_t = _chunk([case], table=True)[0]
        assert all(np.array_equal(a.view(np.uint16), b.view(np.uint16)) for a, b in zip(res, res_t)), 'table variant differs'
    _report()


@pytest.mark.parametrize('scale', AC.SCALES)
def test_chunk_batch(scale):
    """four sequences of five rows in one call: one, two and the maximum number of splits, a different pattern per sequence"""
    pos = AC.chunk_positions(5)
    sp1 = AC.split_ranges(pos['deep'] + 5, AC.chunk_cap(), AC.CHUNK_TPS)[1]
    cases = [_chunk_case(pos['one'], 5, scale=scale, needle=('self', 4)),
             _chunk_case(pos['two'], 5, scale=scale, needle=('history', 255)),
             _chunk_case(pos['deep'], 5, scale=scale, needle=('history', sp1[0])),
             _chunk_case(pos['deep'], 5, scale=scale, needle=('chunk', 0))]
    for case, res in zip(cases, _chunk(cases)):
        _judge('chunk batch', case.needle[0], case, *res, 'chunk', _chunk_ranges(case))
    _report()


# ---------------------------------------------------------------------------------------------------------------------------------
# the decode entries
# ---------------------------------------------------------------------------------------------------------------------------------
D_HEADS, D_T_MAX = AC.DECODE_HEADS, AC.DECODE_T_MAX
D_H = D_HEADS * HD


def _decode_case(pos, **kw):
    return AC.build_case(pos, 1, D_T_MAX, D_HEADS, **kw)


def _stream_ranges(pos, tps, batch=1):
    return AC.split_ranges(pos + 1, AC.grid_splits(D_HEADS, D_T_MAX, batch), tps)


def _decode_bufs(case):
    qd = _dev(case.qkv)
    kd, vd = _guarded(case.kc), _guarded(case.vc)
    od = _guarded(np.full((1, D_H), NAN_BITS, dtype=np.uint16).view(np.float16))
    p = torch.tensor([case.start], dtype=torch.int64, device=DEV)
    return qd, kd, vd, od, p


def _decode_done(case, qd, kd, vd, od, modified_q=False):
    torch.cuda.synchronize()
    if not modified_q:
        assert np.array_equal(_bits(qd), case.qkv.view(np.uint16)), 'qkv was modified'
    return (None if od is None else _inner(od, 1)), _inner(kd, D_T_MAX), _inner(vd, D_T_MAX)


def _pair(case):
    """gptq_decode_rope_kv_f16 + gptq_decode_attn_f16: the partial + combine pair (fp32 records of 128 timesteps)"""
    lib = _native.lib()
    qd, kd, vd, od, p = _decode_bufs(case)
    nb = lib.gptq_decode_attn_workspace_bytes(D_HEADS, HD, D_T_MAX)
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    _native.check(lib.gptq_decode_rope_kv_f16(qd.data_ptr(), p.data_ptr(), kd[GUARD:].data_ptr(), vd[GUARD:].data_ptr(), D_HEADS, HD, D_T_MAX, BASE, _stream()),
                  'rope_kv')
    _native.check(lib.gptq_decode_attn_f16(qd.data_ptr(), kd[GUARD:].data_ptr(), vd[GUARD:].data_ptr(), p.data_ptr(), od[GUARD:].data_ptr(), ws.data_ptr(), nb,
                                           D_HEADS, HD, D_T_MAX, case.scale, _stream()), 'gptq_decode_attn_f16')
    return _decode_done(case, qd, kd, vd, od, modified_q=True)


def _fused(case, table=False):
    lib = _native.lib()
    qd, kd, vd, od, p = _decode_bufs(case)
    nb = lib.gptq_decode_attn_workspace_bytes(D_HEADS, HD, D_T_MAX)
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    args = (qd.data_ptr(), p.data_ptr(), kd[GUARD:].data_ptr(), vd[GUARD:].data_ptr(), od[GUARD:].data_ptr(), ws.data_ptr(), nb, D_HEADS, HD, D_T_MAX, BASE,
            case.scale)
    if table:
        rc = lib.gptq_decode_attn_fused_table_f16(*args, _rope_table(D_T_MAX).data_ptr(), _stream())
    else:
        rc = lib.gptq_decode_attn_fused_f16(*args, _stream())
    _native.check(rc, 'gptq_decode_attn_fused_f16')
    return _decode_done(case, qd, kd, vd, od)


def _split(case, tps, layer=None):
    """gptq_decode_attn_split_f16: the records ({M, den} fp32, normalised partial rows fp16) merged in float64 on the host -- or, with a layer, by
    gptq_layer_decode_attn_f16 (y [N] fp16 with a zero residual)"""
    lib = _native.lib()
    qd, kd, vd, _, p = _decode_bufs(case)
    S = lib.gptq_decode_attn_splits(1, D_HEADS, HD, D_T_MAX)
    nb = lib.gptq_decode_attn_batch_workspace_bytes(1, D_HEADS, HD, D_T_MAX)
    ws = torch.full((nb // 4 * 4,), 0xFF, dtype=torch.uint8, device=DEV).view(torch.float32)   # poisoned: NaN as fp16 and as fp32
    rc = lib.gptq_decode_attn_split_f16(qd.data_ptr(), 3 * D_H, p.data_ptr(), kd[GUARD:].data_ptr(), vd[GUARD:].data_ptr(), ws.data_ptr(), nb, 1, D_HEADS, HD,
                                        D_T_MAX, BASE, case.scale, _rope_table(D_T_MAX).data_ptr(), tps, _stream())
    _native.check(rc, 'gptq_decode_attn_split_f16')
    y = None
    if layer is not None:
        N = D_H
        y = torch.full((1, N), float('nan'), dtype=torch.float16, device=DEV)
        res = torch.zeros((1, N), dtype=torch.float16, device=DEV)
        _native.check(lib.gptq_layer_decode_attn_f16(layer.handle, ws.data_ptr(), nb, p.data_ptr(), 1, D_HEADS, HD, D_T_MAX, tps, y.data_ptr(), N,
                                                     res.data_ptr(), N, _stream()), 'gptq_layer_decode_attn_f16')
    _, ka, va = _decode_done(case, qd, kd, vd, None)
    o16 = ws.view(torch.float16)[:S * D_H].view(S, D_H).double().cpu().numpy()
    md = ws[S * D_H // 2:S * D_H // 2 + S * D_HEADS * 2].view(S, D_HEADS, 2).double().cpu().numpy()
    nsp = len(_stream_ranges(case.start, tps if tps > 0 else 128))
    assert np.isfinite(md[:nsp]).all() and np.isfinite(o16[:nsp]).all() and np.isnan(md[nsp:]).all() and np.isnan(o16[nsp:]).all(), 'active splits'
    o16, md = o16[:nsp], md[:nsp]
    c = np.exp2(md[:, :, 0] - md[:, :, 0].max(0)[None]) * md[:, :, 1]
    c = c / c.sum(0)[None]
    merged = (c[:, :, None] * o16.reshape(nsp, D_HEADS, HD)).sum(0).reshape(1, D_H)
    return (merged if y is None else y.cpu().numpy()), ka, va


DECODE_ENTRIES = {   # name: (run, kind of the bar, split ranges of a position)
    'pair': (_pair, 'partial', lambda pos: None),
    'fused': (_fused, 'stream', lambda pos: _stream_ranges(pos, 768)),
    'fused table': (lambda case: _fused(case, table=True), 'stream', lambda pos: _stream_ranges(pos, 768)),
    'split 128': (lambda case: _split(case, 128), 'stream', lambda pos: _stream_ranges(pos, 128)),
    'split 768': (lambda case: _split(case, 768), 'stream', lambda pos: _stream_ranges(pos, 768)),
    'split 0': (lambda case: _split(case, 0), 'stream', lambda pos: _stream_ranges(pos, 128)),
}


def _needle_ranges(entry, pos):
    """the splits whose first and last keys carry a needle: the entry's own cut (the pair: its fixed 128-token splits)"""
    return AC.fixed_ranges(pos + 1) if entry == 'pair' else DECODE_ENTRIES[entry][2](pos)


@pytest.mark.parametrize('pos', AC.DECODE_POSITIONS)
@pytest.mark.parametrize('entry', list(DECODE_ENTRIES))
def test_decode_needles(entry, pos):
    """a needle on the first and last key of every split the entry cuts at this position, on pos - 1, on key 0, and on the new token's OWN key, which
    the streaming kernel takes from LDS and the pair from the row appended a launch earlier"""
    run, kind, ranges = DECODE_ENTRIES[entry]
    for needle in AC.decode_needles(pos, _needle_ranges(entry, pos)):
        case = _decode_case(pos, needle=needle)
        _judge(entry, needle[0], case, *run(case), kind, ranges(pos))
    _report()


@pytest.mark.parametrize('scale', AC.SCALES)
@pytest.mark.parametrize('entry', list(DECODE_ENTRIES))
def test_decode_scale(entry, scale):
    """the tiny-context path (pos 5), one split (129) and the deepest position, flat and with one amp-8 key"""
    run, kind, ranges = DECODE_ENTRIES[entry]
    for pos in AC.DECODE_SCALE_POSITIONS:
        for needle, amp in AC.scale_patterns(pos, 1):
            case = _decode_case(pos, scale=scale, needle=needle, amp=amp)
            _judge(entry, 'scale', case, *run(case), kind, ranges(pos))
    _report()


@pytest.mark.parametrize('scale', AC.SCALES)
def test_decode_batch(scale):
    """gptq_decode_attn_batch_f16: five rows at the five positions in one call, every row with its own needle (call i plants the i-th needle of
    each row's list, the lists wrapping round; at the other two scales the first two calls), then the scale patterns: all rows flat, all rows
    with a key in the middle"""
    lib = _native.lib()
    B = len(AC.DECODE_POSITIONS)
    lists = [AC.decode_needles(pos, _stream_ranges(pos, 768, B)) for pos in AC.DECODE_POSITIONS]
    calls = max(len(l) for l in lists) if scale == AC.SCALE else 2
    picks = [[l[i % len(l)] for l in lists] for i in range(calls)] + [[AC.scale_patterns(pos, 1)[j][0] for pos in AC.DECODE_POSITIONS] for j in (0, 1)]
    nb = lib.gptq_decode_attn_batch_workspace_bytes(B, D_HEADS, HD, D_T_MAX)
    for i, needles in enumerate(picks):
        cases = [_decode_case(pos, scale=scale, needle=needle) for pos, needle in zip(AC.DECODE_POSITIONS, needles)]
        qd = _dev(np.concatenate([c.qkv for c in cases]))
        kd, vd = (_guarded(np.concatenate([getattr(c, name) for c in cases])) for name in ('kc', 'vc'))
        od = _guarded(np.full((B, D_H), NAN_BITS, dtype=np.uint16).view(np.float16))
        p = torch.tensor(AC.DECODE_POSITIONS, dtype=torch.int64, device=DEV)
        ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
        rc = lib.gptq_decode_attn_batch_f16(qd.data_ptr(), 3 * D_H, p.data_ptr(), kd[GUARD:].data_ptr(), vd[GUARD:].data_ptr(), od[GUARD:].data_ptr(), D_H,
                                            ws.data_ptr(), nb, B, D_HEADS, HD, D_T_MAX, BASE, scale, _rope_table(D_T_MAX).data_ptr(), None, _stream())
        _native.check(rc, 'gptq_decode_attn_batch_f16')
        torch.cuda.synchronize()
        out, ka, va = _inner(od, B), _inner(kd, B * D_T_MAX), _inner(vd, B * D_T_MAX)
        for b, c in enumerate(cases):
            sl = slice(b * D_T_MAX, (b + 1) * D_T_MAX)
            _judge('batch', 'scale' if i >= calls else c.needle[0], c, out[b:b + 1], ka[sl], va[sl], 'stream', _stream_ranges(c.start, 768, B))
    _report()


@functools.lru_cache(maxsize=None)
def _o_proj():
    """a 4-bit o_proj of the decode shape: (prepared layer, |W| [K, N] float64, the layer)"""
    from oracle import oracle
    from quant.layer import prepared
    L = make_random_layer(4, 128, D_H, D_H, seed=5)
    pl = prepared(((_dev(L['qweight']), _dev(L['scales']), _dev(L['qzeros']), _dev(L['g_idx'])),), None, 4, 128, D_H, D_H)
    assert _native.lib().gptq_layer_decode_attn_supported(pl.handle, 1, D_HEADS, HD) == 1
    W = np.asarray(oracle.np_dequant(L['qweight'], L['qzeros'], L['scales'], L['g_idx'], 4, faithful=False), dtype=np.float64)
    return pl, W


@pytest.mark.parametrize('tps', [128, 768, 0])
def test_o_proj_record_merge(tps):
    """gptq_decode_attn_split_f16 + gptq_layer_decode_attn_f16: o_proj's decode kernel merges the records while it stages x.  y = x W is linear in
    the attention row, so the attention bar B passes through as B |W| per output; o_proj's own arithmetic and the store of y get the project's
    op-level bar TOL x max|y| on top (tests/util.py) -- against |dy| of order |W| sqrt(128) for a lost needle."""
    pl, W = _o_proj()
    t_eff = tps if tps > 0 else 128
    worst = 0.0
    for pos in AC.DECODE_POSITIONS:
        ranges = _stream_ranges(pos, t_eff)
        needles = AC.decode_needles(pos, ranges)
        picks = [(n, AC.AMP, AC.SCALE) for n in needles[::3] + needles[-1:]] + [(('history', pos // 2), AC.AMP, s) for s in (0.05, 0.2)]
        for needle, amp, scale in picks:
            case = _decode_case(pos, scale=scale, needle=needle, amp=amp)
            y, ka, va = _split(case, tps, layer=pl)
            merged, ka2, va2 = _split(case, tps)
            _, st = _judge('split %d' % tps, 'o_proj x', case, merged, ka2, va2, 'stream', ranges)
            assert np.array_equal(ka.view(np.uint16), ka2.view(np.uint16)) and np.array_equal(va.view(np.uint16), va2.view(np.uint16))
            nsp, span = AC.span_of(ranges)
            x, Bx = st.out.reshape(-1), AC.attn_bound(st, 'stream', nsp, span).reshape(-1)
            exact = x @ W
            bar = Bx @ np.abs(W) + TOL * np.abs(exact).max()
            assert np.isfinite(y.astype(np.float64)).all()
            r = float((np.abs(y.astype(np.float64).reshape(-1) - exact) / bar).max())
            assert r <= 1.0, (case.name, tps, r)
            worst = max(worst, r)
    print('o_proj merge tps %d: worst err/bar %.3f' % (tps, worst))
