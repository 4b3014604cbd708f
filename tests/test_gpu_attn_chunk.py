"""GPU tests of gptq_decode_attn_chunk_f16 (csrc/chunk_attn.hip) through the C ABI: RoPE + cache append + causal attention of 1 .. 16 consecutive
tokens of one sequence at a position read from DEVICE memory -- the verify step of speculative decoding.  Method of tests/test_gpu_prompt_attn.py:
float64 on the fp16 values as the reference, the project's op-level bar TOL through rel_err, every buffer inside an allocation with sentinel guard
rows (and NaN padding columns), so that a stray write shows in a guard."""
import functools

import numpy as np
import pytest
import torch

from quant import _native
from util import rel_err, TOL

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HEADS, HD = 3, 128
H = HEADS * HD
BASE = 10000.0
SCALE = float(1.0 / np.sqrt(HD))
T_MAX = 1930                 # not a multiple of 128 (nor of the kernel's 32-key tile); long enough for the maximum number of splits
GUARD = 64                   # guard rows in front of and behind every cache / output allocation
GUARD_BITS = 0x5A5A          # their bit pattern (fp16 209.25)
NAN_BITS = 0x7E00            # fp16 NaN: cache rows at and beyond p + rows, padding of strided rows, the output before the call


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).to(DEV)      # (a copy: the shared inputs are read-only)


def _bits(t):
    return t.cpu().numpy().view(np.uint16)


@functools.lru_cache(maxsize=None)
def _split_positions(rows):
    """{number of active splits: a position p that gives it for `rows` rows}, from the library's own split rule (attn_split with the entry's
    parameters): every count the rule can choose at T_MAX, 1 and the maximum included"""
    lib = _native.lib()
    found = {}
    for p in range(3, T_MAX - rows, 61):
        n = lib.gptq_decode_attn_chunk_splits(HEADS, HD, T_MAX, p + rows)
        assert n >= 1
        found.setdefault(n, p)
    top = lib.gptq_decode_attn_chunk_splits(HEADS, HD, T_MAX, T_MAX)
    assert sorted(found) == list(range(1, top + 1)) and top >= 3, (found, top)
    return found


def _resolve(p, rows):
    if p == 'end':
        return T_MAX - rows
    if isinstance(p, str):
        n = int(p[5:])
        sp = _split_positions(rows)
        return sp[max(sp) if n == 0 else n]
    return p


@functools.lru_cache(maxsize=None)
def _inputs(p, rows, qk_scale=1.0):
    """N(0,1) qkv, 0.5 N(0,1) keys / N(0,1) values below p, NaN from p + rows on (the rows of the chunk itself hold values the call must
    overwrite).  Read-only: callers copy."""
    rng = np.random.default_rng(1000 * p + rows)
    qkv = rng.standard_normal((rows, 3 * H)).astype(np.float32)
    qkv[:, :2 * H] *= qk_scale
    kc = (rng.standard_normal((T_MAX, H)) * 0.5 * qk_scale).astype(np.float16)
    vc = rng.standard_normal((T_MAX, H)).astype(np.float16)
    kc[p + rows:] = np.uint16(NAN_BITS).view(np.float16)
    vc[p + rows:] = np.uint16(NAN_BITS).view(np.float16)
    qkv = qkv.astype(np.float16)
    for a in (qkv, kc, vc):
        a.setflags(write=False)
    return qkv, kc, vc


def _exact(q_rot, kc, vc, p, rows):
    """float64 causal softmax attention on the fp16 values: q_rot [rows][H] rotated, kc / vc the caches AFTER the append"""
    out = np.zeros((rows, H))
    n = p + rows
    for h in range(HEADS):
        q = q_rot[:, h * HD:(h + 1) * HD].astype(np.float64)
        k = kc[:n, h * HD:(h + 1) * HD].astype(np.float64)
        v = vc[:n, h * HD:(h + 1) * HD].astype(np.float64)
        s = (q @ k.T) * SCALE
        s[np.arange(n)[None, :] > (p + np.arange(rows))[:, None]] = -np.inf
        s -= s.max(axis=1, keepdims=True)
        e = np.exp(s)
        out[:, h * HD:(h + 1) * HD] = (e / e.sum(axis=1, keepdims=True)) @ v
    return out


def _row_by_row(qkv, kc, vc, p):
    """gptq_decode_rope_kv_f16 fed row by row at its position: rotated q rows and the caches a token-by-token feed leaves"""
    lib = _native.lib()
    s = torch.cuda.current_stream().cuda_stream
    qd, kd, vd = _dev(qkv), _dev(kc), _dev(vc)
    pos = torch.arange(p, p + qkv.shape[0], dtype=torch.int64, device=DEV)
    for r in range(qkv.shape[0]):
        _native.check(lib.gptq_decode_rope_kv_f16(qd[r].data_ptr(), pos[r:].data_ptr(), kd.data_ptr(), vd.data_ptr(), HEADS, HD, T_MAX, BASE, s), 'rope_kv')
    torch.cuda.synchronize()
    return qd.cpu().numpy()[:, :H], kd.cpu().numpy(), vd.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(p, rows, qk_scale=1.0):
    """(row-by-row caches, float64 result) of a case: computed once, shared, never modified"""
    qkv, kc, vc = _inputs(p, rows, qk_scale)
    q_rot, kc_ref, vc_ref = _row_by_row(qkv, kc, vc, p)
    exact = _exact(q_rot, kc_ref, vc_ref, p, rows)
    for a in (kc_ref, vc_ref, exact):
        a.setflags(write=False)
    return kc_ref, vc_ref, exact


@functools.lru_cache(maxsize=None)
def _rope_table():
    tab = torch.empty((T_MAX, HD // 2, 2), dtype=torch.float32, device=DEV)
    _native.check(_native.lib().gptq_rope_table_f32(tab.data_ptr(), T_MAX, HD, BASE, torch.cuda.current_stream().cuda_stream), 'rope_table')
    return tab


def _guarded(a, cols=None):
    """a [n][c] inside an allocation with GUARD rows of GUARD_BITS before and behind (and, with cols > c, NaN padding behind every row)"""
    n, c = a.shape
    cols = c if cols is None else cols
    full = np.full((n + 2 * GUARD, cols), GUARD_BITS, dtype=np.uint16)
    full[GUARD:GUARD + n] = NAN_BITS
    full[GUARD:GUARD + n, :c] = a.view(np.uint16)
    return _dev(full).view(torch.float16)


def _workspace(rows):
    n = _native.lib().gptq_decode_attn_chunk_workspace_bytes(rows, HEADS, HD, T_MAX)
    assert n > 0
    return torch.empty(n, dtype=torch.uint8, device=DEV).fill_(0xA5)       # pure scratch: no initialisation asked


def _call(lib, qd, ldq, rows, pos, kd, vd, od, ldo, ws, tab, s):
    return lib.gptq_decode_attn_chunk_f16(qd.data_ptr(), ldq, rows, pos.data_ptr(), kd[GUARD:].data_ptr(), vd[GUARD:].data_ptr(), od[GUARD:].data_ptr(),
                                          ldo, ws.data_ptr(), ws.numel(), HEADS, HD, T_MAX, BASE, SCALE, _native.ptr(tab), s)


def _run(p, rows, qkv, kc, vc, table=False, ldq=3 * H, ldo=H):
    """one call on guarded allocations with *position = p; returns the raw allocations (as uint16 arrays on the host)"""
    lib = _native.lib()
    s = torch.cuda.current_stream().cuda_stream
    qf = np.full((rows, ldq), NAN_BITS, dtype=np.uint16)
    qf[:, :3 * H] = qkv.view(np.uint16)
    qd = _dev(qf).view(torch.float16)
    kd, vd = _guarded(kc), _guarded(vc)
    od = _guarded(np.full((rows, H), NAN_BITS, dtype=np.uint16).view(np.float16), cols=ldo)
    pos = torch.tensor([p], dtype=torch.int64, device=DEV)
    rc = _call(lib, qd, ldq, rows, pos, kd, vd, od, ldo, _workspace(rows), _rope_table() if table else None, s)
    _native.check(rc, 'gptq_decode_attn_chunk_f16')
    torch.cuda.synchronize()
    assert int(pos[0]) == p
    return dict(qkv=_bits(qd), qkv_in=qf, kc=_bits(kd), vc=_bits(vd), out=_bits(od))


def _out(res, rows):
    return res['out'][GUARD:GUARD + rows, :H].view(np.float16)


def _check_guards(res, rows):
    for name in ('kc', 'vc'):
        a = res[name]
        assert (a[:GUARD] == GUARD_BITS).all() and (a[GUARD + T_MAX:] == GUARD_BITS).all(), name + ' guard rows written'
    o = res['out']
    assert (o[:GUARD] == GUARD_BITS).all() and (o[GUARD + rows:] == GUARD_BITS).all(), 'out guard rows written'
    assert (o[GUARD:GUARD + rows, H:] == NAN_BITS).all(), 'padding of the output rows written'
    assert np.array_equal(res['qkv'], res['qkv_in']), 'qkv was modified'


# every p with 5 rows; the other row counts at the tile / split edges
CASES = [(p, 5) for p in (0, 1, 127, 128, 129, 'split1', 'split2', 'split3', 'split4', 'split5', 'split6', 'split7', 'split0', 'end')]
CASES += [(p, rows) for rows in (1, 2, 8, 16) for p in (0, 1, 127, 128, 129, 'split2', 'split0', 'end')]


@pytest.mark.parametrize('p,rows', CASES)
def test_chunk_attn_against_float64(p, rows):
    """'splitN': a position at which the library cuts the range into N splits (0: the most it can choose at T_MAX); 'end': p = T_MAX - rows"""
    if isinstance(p, str) and p.startswith('split') and int(p[5:]) > max(_split_positions(rows)):
        p = 'split0'                                  # (the rule's maximum at T_MAX is below this count: that maximum again)
    p = _resolve(p, rows)
    qkv, kc, vc = _inputs(p, rows)
    kc_ref, vc_ref, exact = _reference(p, rows)
    res = _run(p, rows, qkv, kc, vc)
    _check_guards(res, rows)
    # the cache: rows of the chunk bit-identical to the token-by-token feed, every other row untouched (the reference holds both)
    assert np.array_equal(res['kc'][GUARD:GUARD + T_MAX], kc_ref.view(np.uint16))
    assert np.array_equal(res['vc'][GUARD:GUARD + T_MAX], vc_ref.view(np.uint16))
    for ref, inp in ((kc_ref, kc), (vc_ref, vc)):
        assert np.array_equal(ref.view(np.uint16)[:p], inp.view(np.uint16)[:p]) and (ref.view(np.uint16)[p + rows:] == NAN_BITS).all()
    out = _out(res, rows)
    finite = bool(np.isfinite(out.astype(np.float32)).all())
    err = rel_err(out, exact) if finite else float('inf')
    nsp = _native.lib().gptq_decode_attn_chunk_splits(HEADS, HD, T_MAX, p + rows)
    print('chunk_attn (p %d, rows %d, %d splits): rel err %.3e' % (p, rows, nsp, err))
    assert finite
    assert err < TOL, err
    if rows == 1 and p == 0:         # one key: softmax = 1, the output is v exactly
        assert np.array_equal(out.view(np.uint16), qkv[:, 2 * H:].view(np.uint16))
    # the table variant and a second call on identical inputs: bit-identical
    res_t = _run(p, rows, qkv, kc, vc, table=True)
    for name in ('out', 'kc', 'vc'):
        assert np.array_equal(res_t[name], res[name]), 'table variant differs in ' + name
    res_2 = _run(p, rows, qkv, kc, vc)
    assert np.array_equal(res_2['out'], res['out']), 'not deterministic'


def test_split_counts_cover_one_two_and_the_maximum():
    sp = _split_positions(5)
    lib = _native.lib()
    assert min(sp) == 1 and 2 in sp and max(sp) == lib.gptq_decode_attn_chunk_splits(HEADS, HD, T_MAX, T_MAX)
    # 2 047 tokens at 32 heads: at least one workgroup per CU (256)
    assert 32 * lib.gptq_decode_attn_chunk_splits(32, HD, 2048, 2047) >= 256


def test_chunk_attn_large_scores():
    """q and k scaled by 8: score standard deviation ~ 60, maxima beyond 89 -- exp overflows without the running maximum, and a rescale applied
    to only one of l and the accumulator (or a merge that forgets a split's maximum) shows at once"""
    rows = 5
    p = _resolve('split3', rows)
    qkv, kc, vc = _inputs(p, rows, 8.0)
    _, _, exact = _reference(p, rows, 8.0)
    out = _out(_run(p, rows, qkv, kc, vc), rows)
    assert np.isfinite(out.astype(np.float32)).all()
    err = rel_err(out, exact)
    print('chunk_attn large scores: rel err %.3e' % err)
    assert err < TOL, err


@pytest.mark.parametrize('p,rows', [(129, 5), ('split2', 16), ('split0', 8)])
def test_chunk_attn_agrees_with_the_prompt_entry(p, rows):
    """the same inputs through gptq_prompt_attn_f16 (start a host value): caches bitwise equal, both outputs within the bar of float64"""
    p = _resolve(p, rows)
    lib = _native.lib()
    s = torch.cuda.current_stream().cuda_stream
    qkv, kc, vc = _inputs(p, rows)
    _, _, exact = _reference(p, rows)
    res = _run(p, rows, qkv, kc, vc)
    qd, kd, vd = _dev(qkv), _dev(kc), _dev(vc)
    od = torch.zeros((rows, H), dtype=torch.float16, device=DEV)
    ws = torch.empty(lib.gptq_prompt_attn_workspace_bytes(rows, HEADS, HD, T_MAX), dtype=torch.uint8, device=DEV)
    rc = lib.gptq_prompt_attn_f16(qd.data_ptr(), 3 * H, rows, p, kd.data_ptr(), vd.data_ptr(), od.data_ptr(), H, ws.data_ptr(), ws.numel(), HEADS, HD,
                                  T_MAX, BASE, SCALE, None, s)
    _native.check(rc, 'gptq_prompt_attn_f16')
    torch.cuda.synchronize()
    assert np.array_equal(res['kc'][GUARD:GUARD + T_MAX], _bits(kd))
    assert np.array_equal(res['vc'][GUARD:GUARD + T_MAX], _bits(vd))
    e_chunk, e_prompt = rel_err(_out(res, rows), exact), rel_err(od.cpu().numpy(), exact)
    print('chunk %.3e, prompt %.3e against float64' % (e_chunk, e_prompt))
    assert e_chunk < TOL and e_prompt < TOL, (e_chunk, e_prompt)


@pytest.mark.parametrize('p', [3, 'split2'])
def test_chunk_attn_causality_within_the_chunk(p):
    rows, j = 8, 5
    p = _resolve(p, rows)
    qkv, kc, vc = _inputs(p, rows)
    base = _out(_run(p, rows, qkv, kc, vc), rows)
    qkv2 = qkv.copy()
    qkv2[j] = np.random.default_rng(5).standard_normal(3 * H).astype(np.float16)
    got = _out(_run(p, rows, qkv2, kc, vc), rows)
    assert np.array_equal(got[:j].view(np.uint16), base[:j].view(np.uint16)), 'a later row reached an earlier output'
    assert not np.array_equal(got[j].view(np.uint16), base[j].view(np.uint16))
    assert all(not np.array_equal(got[r].view(np.uint16), base[r].view(np.uint16)) for r in range(j + 1, rows))


@pytest.mark.parametrize('p,rows', [(40, 5), ('split2', 5), ('split0', 16)])
def test_chunk_attn_stale_tail(p, rows):
    """what rejected drafts leave: NaN in every cache row behind the chunk (the inputs' default) AND in the chunk's own rows before the call"""
    p = _resolve(p, rows)
    qkv, kc, vc = _inputs(p, rows)
    clean = _run(p, rows, qkv, kc, vc)
    kc2, vc2 = kc.copy(), vc.copy()
    kc2[p:] = np.uint16(NAN_BITS).view(np.float16)
    vc2[p:] = np.uint16(NAN_BITS).view(np.float16)
    got = _run(p, rows, qkv, kc2, vc2)
    assert np.isfinite(_out(got, rows).astype(np.float32)).all()
    for name in ('out', 'kc', 'vc'):
        assert np.array_equal(got[name], clean[name]), name
    # and the history counts: cache row p - 1 reaches every row
    kc3, vc3 = kc.copy(), vc.copy()
    rng = np.random.default_rng(6)
    kc3[p - 1] = (rng.standard_normal(H) * 4).astype(np.float16)
    vc3[p - 1] = (rng.standard_normal(H) * 4).astype(np.float16)
    seen = _out(_run(p, rows, qkv, kc3, vc3), rows)
    assert all(not np.array_equal(seen[r].view(np.uint16), _out(clean, rows)[r].view(np.uint16)) for r in range(rows))


def test_chunk_attn_idle_position():
    rows = 5
    qkv, kc, vc = _inputs(200, rows)
    res = _run(-1, rows, qkv, kc, vc)
    _check_guards(res, rows)
    assert np.array_equal(res['kc'][GUARD:GUARD + T_MAX], kc.view(np.uint16)) and np.array_equal(res['vc'][GUARD:GUARD + T_MAX], vc.view(np.uint16))
    assert (res['out'][GUARD:GUARD + rows] == NAN_BITS).all()


@pytest.mark.parametrize('p', [T_MAX, T_MAX + 7, 2 ** 31 + 5, 2 ** 40])
def test_chunk_attn_position_beyond_the_slot(p):
    rows = 5
    qkv, kc, vc = _inputs(200, rows)
    res = _run(p, rows, qkv, kc, vc)
    _check_guards(res, rows)
    assert np.array_equal(res['kc'][GUARD:GUARD + T_MAX], kc.view(np.uint16)) and np.array_equal(res['vc'][GUARD:GUARD + T_MAX], vc.view(np.uint16))
    assert (res['out'][GUARD:GUARD + rows] == NAN_BITS).all()


def test_chunk_attn_rows_that_do_not_fit():
    """p = t_max - 2 with 4 rows: rows 0 and 1 are served, rows 2 and 3 skipped"""
    rows, fit = 4, 2
    p = T_MAX - fit
    qkv, kc, vc = _inputs(p, fit)                      # (the reference of the two rows that fit)
    kc_ref, vc_ref, exact = _reference(p, fit)
    qkv4 = np.concatenate([qkv, np.random.default_rng(8).standard_normal((rows - fit, 3 * H)).astype(np.float16)])
    res = _run(p, rows, qkv4, kc, vc)
    _check_guards(res, rows)
    assert np.array_equal(res['kc'][GUARD:GUARD + T_MAX], kc_ref.view(np.uint16)) and np.array_equal(res['vc'][GUARD:GUARD + T_MAX], vc_ref.view(np.uint16))
    out = _out(res, rows)
    assert (out[fit:].view(np.uint16) == NAN_BITS).all(), 'a skipped row was written'
    err = rel_err(out[:fit], exact)
    print('chunk_attn rows that fit: rel err %.3e' % err)
    assert err < TOL, err
    assert np.array_equal(out[:fit].view(np.uint16), _out(_run(p, fit, qkv, kc, vc), fit).view(np.uint16))


def test_chunk_attn_strides():
    rows = 5
    p = _resolve('split2', rows)
    qkv, kc, vc = _inputs(p, rows)
    base = _run(p, rows, qkv, kc, vc)
    res = _run(p, rows, qkv, kc, vc, ldq=3 * H + 64, ldo=H + 32)
    _check_guards(res, rows)                           # (the NaN padding of qkv and out rows included)
    assert np.array_equal(_out(res, rows).view(np.uint16), _out(base, rows).view(np.uint16))
    assert np.array_equal(res['kc'], base['kc']) and np.array_equal(res['vc'], base['vc'])


def test_chunk_attn_position_is_read_on_the_device():
    """one capture, replays at three positions of different split counts: each bitwise equal to an eager call at that position"""
    rows = 5
    lib = _native.lib()
    sp = _split_positions(rows)
    positions = [sp[1], sp[2], sp[max(sp)]]
    qkv, kc, vc = _inputs(positions[-1], rows)         # history everywhere below the deepest position
    qd = _dev(qkv)
    kd, vd = _guarded(kc), _guarded(vc)
    od = _guarded(np.zeros((rows, H), dtype=np.float16))
    k0, v0, o0 = kd.clone(), vd.clone(), od.clone()
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    ws = _workspace(rows)
    tab = _rope_table()

    def reset(p):
        kd.copy_(k0); vd.copy_(v0); od.copy_(o0)
        pos.fill_(p)

    def eager(p):
        reset(p)
        _native.check(_call(lib, qd, 3 * H, rows, pos, kd, vd, od, H, ws, tab, torch.cuda.current_stream().cuda_stream), 'chunk')
        torch.cuda.synchronize()
        return _bits(od), _bits(kd), _bits(vd)
    expect = [eager(p) for p in positions]
    again = eager(positions[1])
    assert all(np.array_equal(a, b) for a, b in zip(again, expect[1])), 'two eager calls differ'
    reset(positions[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _native.check(_call(lib, qd, 3 * H, rows, pos, kd, vd, od, H, ws, tab, torch.cuda.current_stream().cuda_stream), 'chunk')
    for p, exp in zip(positions, expect):
        reset(p)
        g.replay()
        torch.cuda.synchronize()
        got = (_bits(od), _bits(kd), _bits(vd))
        assert (got[0][GUARD:GUARD + rows] != 0).any()
        for name, a, b in zip(('out', 'kc', 'vc'), got, exp):
            assert np.array_equal(a, b), 'replay at %d differs from the eager call in %s' % (p, name)


def test_chunk_attn_argument_errors():
    """validated on the host: the documented codes, and nothing is launched (every buffer keeps its bits)"""
    lib = _native.lib()
    rows, t_max = 4, 64
    qd = torch.zeros((rows, 3 * H + 8), dtype=torch.float16, device=DEV)
    kd = torch.full((t_max, H), 3.0, dtype=torch.float16, device=DEV)
    vd = torch.full((t_max, H), 5.0, dtype=torch.float16, device=DEV)
    od = torch.full((rows, H + 8), 7.0, dtype=torch.float16, device=DEV)
    pos = torch.zeros(2, dtype=torch.int64, device=DEV)
    need = lib.gptq_decode_attn_chunk_workspace_bytes(rows, HEADS, HD, t_max)
    ws = torch.zeros(need + 64, dtype=torch.uint8, device=DEV)
    E_SHAPE, E_ALIGN, E_NULL = -2, -3, -4              # GPTQ_E_SHAPE, GPTQ_E_ALIGN, GPTQ_E_NULL (include/gptq_mi355x.h)

    def call(qkv=None, ldq=3 * H, rows_=rows, position=None, k=None, v=None, out=None, ldo=H, w=None, wb=need, heads=HEADS, hd=HD, tm=t_max, tab=None):
        pick = lambda x, d: d if x is None else (x or None)       # 0 stands for a NULL pointer
        return lib.gptq_decode_attn_chunk_f16(pick(qkv, qd.data_ptr()), ldq, rows_, pick(position, pos.data_ptr()), pick(k, kd.data_ptr()),
                                              pick(v, vd.data_ptr()), pick(out, od.data_ptr()), ldo, pick(w, ws.data_ptr()), wb, heads, hd, tm, BASE, SCALE,
                                              tab, torch.cuda.current_stream().cuda_stream)
    for name in ('qkv', 'position', 'k', 'v', 'out', 'w'):
        assert call(**{name: 0}) == E_NULL, name
    assert call(rows_=0) == E_SHAPE and call(rows_=17) == E_SHAPE and call(rows_=-1) == E_SHAPE
    assert call(hd=64) == E_SHAPE and call(hd=256) == E_SHAPE
    assert call(ldq=3 * H - 8) == E_SHAPE and call(ldo=H - 8) == E_SHAPE
    assert call(wb=need - 1) == E_SHAPE and call(wb=0) == E_SHAPE
    assert call(heads=0) == E_SHAPE and call(tm=0) == E_SHAPE
    assert call(qkv=qd.data_ptr() + 2) == E_ALIGN and call(k=kd.data_ptr() + 8) == E_ALIGN and call(v=vd.data_ptr() + 8) == E_ALIGN
    assert call(out=od.data_ptr() + 2) == E_ALIGN and call(w=ws.data_ptr() + 4) == E_ALIGN and call(position=pos.data_ptr() + 4) == E_ALIGN
    assert call(ldq=3 * H + 4) == E_ALIGN and call(ldo=H + 4) == E_ALIGN
    assert call(tab=_rope_table().data_ptr() + 4) == E_ALIGN
    assert lib.gptq_decode_attn_chunk_workspace_bytes(0, HEADS, HD, t_max) == 0 and lib.gptq_decode_attn_chunk_workspace_bytes(17, HEADS, HD, t_max) == 0
    assert lib.gptq_decode_attn_chunk_workspace_bytes(4, HEADS, 64, t_max) == 0
    torch.cuda.synchronize()
    assert bool((kd == 3.0).all()) and bool((vd == 5.0).all()) and bool((od == 7.0).all()) and not bool(ws.any()), 'a refused call launched something'
    assert call(ldq=3 * H + 8, ldo=H + 8) == 0         # and the valid call goes through: rows 0 .. 3 of the cache, nothing else
    torch.cuda.synchronize()
    assert bool((kd[rows:] == 3.0).all()) and bool((vd[rows:] == 5.0).all()) and bool((vd[:rows] == 0.0).all()) and bool((od[:, H:] == 7.0).all())
