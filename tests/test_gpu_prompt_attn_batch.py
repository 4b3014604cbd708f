"""GPU tests of gptq_prompt_attn_batch_f16 (csrc/prompt_attn.hip): up to 16 segments -- chunks of different sequences, lengths and start
positions -- of one packed qkv / out matrix and one cache allocation in two launches.  Per segment every bit must be that of
gptq_prompt_attn_f16 on the segment alone; the float64 bar is the project's op-level TOL.  Guard rows / NaN fill as in
tests/test_gpu_prompt_attn.py (the small helpers are copies: that file is not imported)."""
import functools

import numpy as np
import pytest
import torch

from quant import _native
from util import rel_err, TOL

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HEADS, HD = 4, 128
H = HEADS * HD
T_MAX = 384
BASE = 10000.0
SCALE = float(1.0 / np.sqrt(HD))
GUARD = 64                   # guard rows in front of and behind every cache / output allocation
GUARD_BITS = 0x5A5A          # their bit pattern (fp16 209.25); unused cache slots carry it too
NAN_BITS = 0x7E00            # fp16 NaN: cache rows at and beyond start + rows, rows between segments, padding of strided rows

# (start, rows): 266 packed rows; cross the 64-key and the 128-row tile edges; the tail of the last one sits in a key tile that t_max cuts
SEGS = [(0, 1), (5, 1), (0, 65), (130, 70), (255, 129)]


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).to(DEV)      # (a copy: the shared inputs are read-only)


def _bits(t):
    return t.cpu().numpy().view(np.uint16)


def _u16(a):
    return np.ascontiguousarray(a).view(np.uint16)


@functools.lru_cache(maxsize=None)
def _inputs(start, rows, seed=0):
    """N(0,1) qkv, 0.5 N(0,1) keys / N(0,1) values below start, NaN from start + rows on (the rows of the chunk itself hold values the
    call must overwrite).  Read-only: callers copy."""
    rng = np.random.default_rng(1000 * start + rows + 77777 * seed)
    qkv = rng.standard_normal((rows, 3 * H)).astype(np.float16)
    kc = (rng.standard_normal((T_MAX, H)) * 0.5).astype(np.float16)
    vc = rng.standard_normal((T_MAX, H)).astype(np.float16)
    kc[start + rows:] = np.uint16(NAN_BITS).view(np.float16)
    vc[start + rows:] = np.uint16(NAN_BITS).view(np.float16)
    for a in (qkv, kc, vc):
        a.setflags(write=False)
    return qkv, kc, vc


@functools.lru_cache(maxsize=None)
def _rope_table():
    tab = torch.empty((T_MAX, HD // 2, 2), dtype=torch.float32, device=DEV)
    _native.check(_native.lib().gptq_rope_table_f32(tab.data_ptr(), T_MAX, HD, BASE, torch.cuda.current_stream().cuda_stream), 'rope_table')
    return tab


def _single(start, rows, qkv, kc, vc, table=False):
    """gptq_prompt_attn_f16 on one segment alone: (out [rows][H], k cache, v cache [T_MAX][H]) as uint16"""
    lib = _native.lib()
    qd, kd, vd = _dev(qkv), _dev(kc), _dev(vc)
    od = torch.zeros((rows, H), dtype=torch.float16, device=DEV)
    ws = torch.empty(lib.gptq_prompt_attn_workspace_bytes(rows, HEADS, HD, T_MAX), dtype=torch.uint8, device=DEV)
    tab = _rope_table() if table else None
    rc = lib.gptq_prompt_attn_f16(qd.data_ptr(), 3 * H, rows, start, kd.data_ptr(), vd.data_ptr(), od.data_ptr(), H, ws.data_ptr(), ws.numel(),
                                  HEADS, HD, T_MAX, BASE, SCALE, _native.ptr(tab), torch.cuda.current_stream().cuda_stream)
    _native.check(rc, 'gptq_prompt_attn_f16')
    torch.cuda.synchronize()
    return _bits(od), _bits(kd), _bits(vd)


@functools.lru_cache(maxsize=None)
def _single_ref(start, rows, table=False):
    """the single-sequence entry on the shared inputs of a segment: computed once, never modified"""
    res = _single(start, rows, *_inputs(start, rows), table=table)
    for a in res:
        a.setflags(write=False)
    return res


def _run(layout, data, nslot, total=None, table=False, ldq=3 * H, ldo=H):
    """ONE batch call.  layout: [(row0, rows, start, slot)] in table order; data[i] = (qkv, kc, vc) of entry i (kc / vc: the slot's content
    before the call).  Guarded allocations: the cache is [GUARD | nslot slices of T_MAX rows | GUARD], slots no segment names hold GUARD_BITS;
    packed rows no segment covers and the padding of strided rows hold NaN.  Returns the raw allocations as uint16 arrays."""
    lib = _native.lib()
    total = max(r0 + n for r0, n, _, _ in layout) if total is None else total
    qf = np.full((total, ldq), NAN_BITS, dtype=np.uint16)
    kf = np.full((2 * GUARD + nslot * T_MAX, H), GUARD_BITS, dtype=np.uint16)
    vf = kf.copy()
    for (r0, n, _, slot), (qkv, kc, vc) in zip(layout, data):
        qf[r0:r0 + n, :3 * H] = _u16(qkv)
        kf[GUARD + slot * T_MAX:GUARD + (slot + 1) * T_MAX] = _u16(kc)
        vf[GUARD + slot * T_MAX:GUARD + (slot + 1) * T_MAX] = _u16(vc)
    of = np.full((2 * GUARD + total, ldo), GUARD_BITS, dtype=np.uint16)
    of[GUARD:GUARD + total] = NAN_BITS
    qd, kd, vd, od = (_dev(a).view(torch.float16) for a in (qf, kf, vf, of))
    ws = torch.empty(lib.gptq_prompt_attn_workspace_bytes(total, HEADS, HD, T_MAX), dtype=torch.uint8, device=DEV)
    tab = _rope_table() if table else None
    segs = (_native.PromptSeg * len(layout))(*[_native.PromptSeg(*e) for e in layout])
    rc = lib.gptq_prompt_attn_batch_f16(qd.data_ptr(), ldq, total, segs, len(layout), kd[GUARD:].data_ptr(), vd[GUARD:].data_ptr(), T_MAX * H,
                                        od[GUARD:].data_ptr(), ldo, ws.data_ptr(), ws.numel(), HEADS, HD, T_MAX, BASE, SCALE, _native.ptr(tab),
                                        torch.cuda.current_stream().cuda_stream)
    for i in range(len(layout)):
        segs[i].rows = -1                       # the table was taken by value: the caller may reuse the array at once
    _native.check(rc, 'gptq_prompt_attn_batch_f16')
    torch.cuda.synchronize()
    return dict(qkv=_bits(qd), qkv_in=qf, kc=_bits(kd), vc=_bits(vd), kc_in=kf, vc_in=vf, out=_bits(od), total=total, nslot=nslot)


def _slot(res, name, slot):
    return res[name][GUARD + slot * T_MAX:GUARD + (slot + 1) * T_MAX]


def _seg_out(res, r0, n):
    return res['out'][GUARD + r0:GUARD + r0 + n, :H]


def _check_untouched(res, layout):
    """guard rows, rows between the segments, row padding, slots no segment names, and qkv itself: bit-unchanged"""
    total, nslot = res['total'], res['nslot']
    for name in ('kc', 'vc'):
        a = res[name]
        assert (a[:GUARD] == GUARD_BITS).all() and (a[GUARD + nslot * T_MAX:] == GUARD_BITS).all(), name + ' guard rows written'
        for slot in set(range(nslot)) - set(e[3] for e in layout):
            assert (_slot(res, name, slot) == GUARD_BITS).all(), '%s slot %d written' % (name, slot)
    o = res['out']
    assert (o[:GUARD] == GUARD_BITS).all() and (o[GUARD + total:] == GUARD_BITS).all(), 'out guard rows written'
    assert (o[GUARD:GUARD + total, H:] == NAN_BITS).all(), 'padding of the output rows written'
    covered = np.zeros(total, dtype=bool)
    for r0, n, _, _ in layout:
        covered[r0:r0 + n] = True
    assert (o[GUARD:GUARD + total][~covered] == NAN_BITS).all(), 'an output row between the segments was written'
    assert np.array_equal(res['qkv'], res['qkv_in']), 'qkv was modified'


def _packed(segs=SEGS, slots=None):
    """rows back to back in the order given, slot i (or slots[i]) for entry i"""
    layout, r0 = [], 0
    for i, (start, rows) in enumerate(segs):
        layout.append((r0, rows, start, i if slots is None else slots[i]))
        r0 += rows
    return layout


def _assert_segments_equal_single(res, layout, table=False):
    for r0, n, start, slot in layout:
        out, kc, vc = _single_ref(start, n, table)
        assert np.array_equal(_seg_out(res, r0, n), out), ('output rows differ from the single-sequence entry', start, n)
        assert np.array_equal(_slot(res, 'kc', slot), kc), ('k cache differs', start, n)
        assert np.array_equal(_slot(res, 'vc', slot), vc), ('v cache differs', start, n)


@functools.lru_cache(maxsize=None)
def _base():
    layout = _packed()
    res = _run(layout, [_inputs(s, n) for s, n in SEGS], nslot=len(SEGS))
    for a in res.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return layout, res


@pytest.mark.parametrize('table', [False, True])
def test_batch_is_bit_identical_to_the_single_sequence_entry(table):
    layout = _packed()
    assert sum(n for _, n in SEGS) == 266
    res = _base()[1] if not table else _run(layout, [_inputs(s, n) for s, n in SEGS], nslot=len(SEGS), table=True)
    _check_untouched(res, layout)
    _assert_segments_equal_single(res, layout, table)
    again = _run(layout, [_inputs(s, n) for s, n in SEGS], nslot=len(SEGS), table=table)
    for name in ('out', 'kc', 'vc'):
        assert np.array_equal(again[name], res[name]), 'not deterministic: ' + name
        assert np.array_equal(res[name], _base()[1][name]), 'table variant differs in ' + name


def _rotated_q(qkv, start):
    """the rotated q rows by the existing gptq_decode_rope_kv_f16, one row at a time at its position (on throw-away caches)"""
    lib = _native.lib()
    s = torch.cuda.current_stream().cuda_stream
    qd = _dev(qkv)
    kd = torch.zeros((T_MAX, H), dtype=torch.float16, device=DEV)
    vd = torch.zeros_like(kd)
    pos = torch.arange(start, start + qkv.shape[0], dtype=torch.int64, device=DEV)
    for r in range(qkv.shape[0]):
        _native.check(lib.gptq_decode_rope_kv_f16(qd[r].data_ptr(), pos[r:].data_ptr(), kd.data_ptr(), vd.data_ptr(), HEADS, HD, T_MAX, BASE, s), 'rope_kv')
    torch.cuda.synchronize()
    return qd.cpu().numpy()[:, :H]


def _exact(q_rot, kc, vc, start, rows):
    """float64 causal softmax attention on the fp16 values: q_rot [rows][H] rotated, kc / vc the caches AFTER the append"""
    out = np.zeros((rows, H))
    n = start + rows
    for h in range(HEADS):
        q = q_rot[:, h * HD:(h + 1) * HD].astype(np.float64)
        k = kc[:n, h * HD:(h + 1) * HD].astype(np.float64)
        v = vc[:n, h * HD:(h + 1) * HD].astype(np.float64)
        s = (q @ k.T) * SCALE
        s[np.arange(n)[None, :] > (start + np.arange(rows))[:, None]] = -np.inf
        s -= s.max(axis=1, keepdims=True)
        p = np.exp(s)
        out[:, h * HD:(h + 1) * HD] = (p / p.sum(axis=1, keepdims=True)) @ v
    return out


def test_batch_against_float64():
    layout, res = _base()
    for r0, n, start, slot in layout:
        qkv = _inputs(start, n)[0]
        kc, vc = _slot(res, 'kc', slot).view(np.float16), _slot(res, 'vc', slot).view(np.float16)
        assert (_u16(kc[start + n:]) == NAN_BITS).all() and (_u16(vc[start + n:]) == NAN_BITS).all()
        assert np.array_equal(_u16(vc[start:start + n]), _u16(qkv[:, 2 * H:]))                  # v rows are appended as they are
        exact = _exact(_rotated_q(qkv, start), kc, vc, start, n)
        out = _seg_out(res, r0, n).view(np.float16)
        assert np.isfinite(out.astype(np.float32)).all(), (start, n)
        err = rel_err(out, exact)
        print('prompt_attn_batch segment (%d, %d): rel err %.3e' % (start, n, err))
        assert err < TOL, (start, n, err)


def test_batch_segments_do_not_leak_into_each_other():
    layout, base = _base()
    data = [_inputs(s, n) for s, n in SEGS]
    loud, dead = 2, 3                                   # segment (0, 65): k and v x 64; segment (130, 70): k and v NaN
    q = data[loud][0].copy()
    q[:, H:] = (q[:, H:].astype(np.float32) * 64).astype(np.float16)
    data[loud] = (q, data[loud][1], data[loud][2])
    q = data[dead][0].copy()
    q[:, H:] = np.uint16(NAN_BITS).view(np.float16)
    data[dead] = (q, data[dead][1], data[dead][2])
    res = _run(layout, data, nslot=len(SEGS))
    assert not np.array_equal(_seg_out(res, *layout[loud][:2]), _seg_out(base, *layout[loud][:2]))
    assert np.isnan(_seg_out(res, *layout[dead][:2]).view(np.float16).astype(np.float32)).all()
    for i, (r0, n, start, slot) in enumerate(layout):
        if i in (loud, dead):
            continue
        assert np.array_equal(_seg_out(res, r0, n), _seg_out(base, r0, n)), ('another segment reached the output of', start, n)
        assert np.array_equal(_slot(res, 'kc', slot), _slot(base, 'kc', slot)) and np.array_equal(_slot(res, 'vc', slot), _slot(base, 'vc', slot))


@pytest.mark.parametrize('order', [(4, 3, 2, 1, 0), (1, 4, 0, 3, 2)])
def test_batch_table_order_does_not_matter(order):
    layout, base = _base()
    data = [_inputs(s, n) for s, n in SEGS]
    res = _run([layout[i] for i in order], [data[i] for i in order], nslot=len(SEGS))
    for name in ('out', 'kc', 'vc', 'qkv'):
        assert np.array_equal(res[name], base[name]), name + ' depends on the order of the table'


def test_batch_layout_gaps_slots_and_strides():
    """gaps between the row ranges, slots out of order (4 and 6 unused), row strides above the row widths"""
    slots, r0s = (3, 0, 2, 5, 1), (7, 1, 150, 20, 230)                 # rows 7 | 1 | 150..214 | 20..89 | 230..358; gaps everywhere
    layout = [(r0, n, start, slot) for (start, n), slot, r0 in zip(SEGS, slots, r0s)]
    data = [_inputs(s, n) for s, n in SEGS]
    res = _run(layout, data, nslot=7, total=366, ldq=3 * H + 64, ldo=H + 32)
    _check_untouched(res, layout)
    _assert_segments_equal_single(res, layout)


def test_batch_continuation():
    """a second batch call continues two of the sequences at start + rows on the caches the first left: the single-sequence entry fed the same
    two chunks agrees in every bit"""
    first = [(0, 65), (130, 70), (5, 1)]
    layout1 = _packed(first)
    res1 = _run(layout1, [_inputs(s, n) for s, n in first], nslot=3)
    second = [(200, 30), (65, 100)]                                    # sequence 1 (slot 1), then sequence 0 (slot 0)
    slots2 = (1, 0)
    chunks = [_inputs(s, n, seed=1)[0] for s, n in second]
    data2 = [(chunks[i], _slot(res1, 'kc', slots2[i]).view(np.float16), _slot(res1, 'vc', slots2[i]).view(np.float16)) for i in range(2)]
    layout2 = _packed(second, slots2)
    res2 = _run(layout2, data2, nslot=2)
    _check_untouched(res2, layout2)
    for i, (start, n) in enumerate(second):
        prev_start, prev_n = first[slots2[i]]
        assert prev_start + prev_n == start
        _, kc1, vc1 = _single_ref(prev_start, prev_n)
        assert np.array_equal(kc1, _slot(res1, 'kc', slots2[i]))
        out, kc, vc = _single(start, n, chunks[i], kc1.view(np.float16), vc1.view(np.float16))
        assert np.array_equal(_seg_out(res2, layout2[i][0], n), out), ('continued output differs', start, n)
        assert np.array_equal(_slot(res2, 'kc', slots2[i]), kc) and np.array_equal(_slot(res2, 'vc', slots2[i]), vc)
        assert (kc[start + n:] == NAN_BITS).all() and not (kc[:start + n] == NAN_BITS).any()
