"""GPU tests of the prompt path of the decode engine: gptq_prompt_attn_f16 (csrc/prompt_attn.hip: RoPE + cache append + causal flash-style
attention of a chunk of tokens over the engine's cache layout) against float64, against the token-by-token decode entries, and
DecodeEngine.prefill / engine_generate(prefill='engine') against the eager module chain."""
import functools

import numpy as np
import pytest
import torch

from quant import _native
from quant import decode as D
from util import rel_err, TOL

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HEADS, HD = 4, 128
H = HEADS * HD
BASE = 10000.0
SCALE = float(1.0 / np.sqrt(HD))
GUARD = 64                   # guard rows in front of and behind every cache / output allocation
GUARD_BITS = 0x5A5A          # their bit pattern (fp16 209.25)
NAN_BITS = 0x7E00            # fp16 NaN: cache rows at and beyond start + rows, padding of strided rows
HOOK_TOL = 2e-2      # generate() / model(...) through the engine hook vs the eager chain, up to 48 tokens deep (fp16 KV cache on both sides)
KV_ATOL = 4e-3       # rotated cache rows against the HF cache (the bar of the decode RoPE test: one fp16 rounding of values up to ~4)

CASES = [(0, 1, 384), (5, 1, 384), (0, 17, 384), (0, 64, 384), (0, 65, 384), (0, 130, 384), (130, 70, 384), (255, 129, 384), (150, 50, 200)]


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).to(DEV)      # (a copy: the shared inputs are read-only)


def _bits(t):
    return t.cpu().numpy().view(np.uint16)


@functools.lru_cache(maxsize=None)
def _inputs(start, rows, t_max, qk_scale=1.0):
    """N(0,1) qkv, 0.5 N(0,1) keys / N(0,1) values below start, NaN from start + rows on (the rows of the chunk itself hold values the
    call must overwrite).  Read-only: callers copy."""
    rng = np.random.default_rng(1000 * start + rows)
    qkv = rng.standard_normal((rows, 3 * H)).astype(np.float32)
    qkv[:, :2 * H] *= qk_scale
    kc = (rng.standard_normal((t_max, H)) * 0.5 * qk_scale).astype(np.float16)
    vc = rng.standard_normal((t_max, H)).astype(np.float16)
    kc[start + rows:] = np.uint16(NAN_BITS).view(np.float16)
    vc[start + rows:] = np.uint16(NAN_BITS).view(np.float16)
    for a in (qkv, kc, vc):
        a.setflags(write=False)
    return qkv.astype(np.float16), kc, vc


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


def _row_by_row(qkv, kc, vc, start, t_max):
    """the existing gptq_decode_rope_kv_f16, one row at a time at its position: rotated q rows and the caches a token-by-token feed leaves"""
    lib = _native.lib()
    s = torch.cuda.current_stream().cuda_stream
    qd, kd, vd = _dev(qkv), _dev(kc), _dev(vc)
    pos = torch.arange(start, start + qkv.shape[0], dtype=torch.int64, device=DEV)
    for r in range(qkv.shape[0]):
        _native.check(lib.gptq_decode_rope_kv_f16(qd[r].data_ptr(), pos[r:].data_ptr(), kd.data_ptr(), vd.data_ptr(), HEADS, HD, t_max, BASE, s), 'rope_kv')
    torch.cuda.synchronize()
    return qd.cpu().numpy()[:, :H], kd.cpu().numpy(), vd.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(start, rows, t_max, qk_scale=1.0):
    """(row-by-row caches, float64 result) of a case: computed once, shared, never modified"""
    qkv, kc, vc = _inputs(start, rows, t_max, qk_scale)
    q_rot, kc_ref, vc_ref = _row_by_row(qkv, kc, vc, start, t_max)
    exact = _exact(q_rot, kc_ref, vc_ref, start, rows)
    for a in (kc_ref, vc_ref, exact):
        a.setflags(write=False)
    return kc_ref, vc_ref, exact


@functools.lru_cache(maxsize=None)
def _rope_table(t_max):
    tab = torch.empty((t_max, HD // 2, 2), dtype=torch.float32, device=DEV)
    _native.check(_native.lib().gptq_rope_table_f32(tab.data_ptr(), t_max, HD, BASE, torch.cuda.current_stream().cuda_stream), 'rope_table')
    return tab


def _guarded(a, cols=None):
    """a [n][c] inside an allocation with GUARD rows of GUARD_BITS before and behind (and, with cols > c, NaN padding behind every row)"""
    n, c = a.shape
    cols = c if cols is None else cols
    full = np.full((n + 2 * GUARD, cols), GUARD_BITS, dtype=np.uint16)
    full[GUARD:GUARD + n] = NAN_BITS
    full[GUARD:GUARD + n, :c] = a.view(np.uint16)
    return _dev(full).view(torch.float16)


def _run(start, rows, t_max, qkv, kc, vc, table=False, ldq=3 * H, ldo=H):
    """one call on guarded allocations; returns the raw allocations (fp16 tensors on the host side as uint16 arrays)"""
    lib = _native.lib()
    s = torch.cuda.current_stream().cuda_stream
    qf = np.full((rows, ldq), NAN_BITS, dtype=np.uint16)
    qf[:, :3 * H] = qkv.view(np.uint16)
    qd = _dev(qf).view(torch.float16)
    kd, vd = _guarded(kc), _guarded(vc)
    od = _guarded(np.full((rows, H), NAN_BITS, dtype=np.uint16).view(np.float16), cols=ldo)
    ws = torch.empty(lib.gptq_prompt_attn_workspace_bytes(rows, HEADS, HD, t_max), dtype=torch.uint8, device=DEV)
    tab = _rope_table(t_max) if table else None
    rc = lib.gptq_prompt_attn_f16(qd.data_ptr(), ldq, rows, start, kd[GUARD:].data_ptr(), vd[GUARD:].data_ptr(), od[GUARD:].data_ptr(), ldo,
                                  ws.data_ptr(), ws.numel(), HEADS, HD, t_max, BASE, SCALE, _native.ptr(tab), s)
    _native.check(rc, 'gptq_prompt_attn_f16')
    torch.cuda.synchronize()
    return dict(qkv=_bits(qd), qkv_in=qf, kc=_bits(kd), vc=_bits(vd), out=_bits(od))


def _out(res, rows):
    return res['out'][GUARD:GUARD + rows, :H].view(np.float16)


def _check_guards(res, rows, t_max, ldo=H):
    for name in ('kc', 'vc'):
        a = res[name]
        assert (a[:GUARD] == GUARD_BITS).all() and (a[GUARD + t_max:] == GUARD_BITS).all(), name + ' guard rows written'
    o = res['out']
    assert (o[:GUARD] == GUARD_BITS).all() and (o[GUARD + rows:] == GUARD_BITS).all(), 'out guard rows written'
    assert (o[GUARD:GUARD + rows, H:] == NAN_BITS).all(), 'padding of the output rows written'
    assert np.array_equal(res['qkv'], res['qkv_in']), 'qkv was modified'


@pytest.mark.parametrize('start,rows,t_max', CASES)
def test_prompt_attn_against_float64(start, rows, t_max):
    qkv, kc, vc = _inputs(start, rows, t_max)
    kc_ref, vc_ref, exact = _reference(start, rows, t_max)
    res = _run(start, rows, t_max, qkv, kc, vc)
    _check_guards(res, rows, t_max)
    # the cache: rows of the chunk bit-identical to the token-by-token feed, every other row untouched (the reference holds both)
    assert np.array_equal(res['kc'][GUARD:GUARD + t_max], kc_ref.view(np.uint16))
    assert np.array_equal(res['vc'][GUARD:GUARD + t_max], vc_ref.view(np.uint16))
    for ref, inp in ((kc_ref, kc), (vc_ref, vc)):
        assert np.array_equal(ref.view(np.uint16)[:start], inp.view(np.uint16)[:start]) and (ref.view(np.uint16)[start + rows:] == NAN_BITS).all()
    out = _out(res, rows)
    err = rel_err(out, exact) if np.isfinite(out.astype(np.float32)).all() else float('inf')
    print('prompt_attn (%d, %d, %d): rel err %.3e' % (start, rows, t_max, err))
    assert np.isfinite(out.astype(np.float32)).all()
    assert err < TOL, err
    if rows == 1 and start == 0:     # one key: softmax = 1, the output is v exactly
        assert np.array_equal(out.view(np.uint16), qkv[:, 2 * H:].view(np.uint16))
    # the table variant and a second run: bit-identical
    res_t = _run(start, rows, t_max, qkv, kc, vc, table=True)
    for name in ('out', 'kc', 'vc'):
        assert np.array_equal(res_t[name], res[name]), 'table variant differs in ' + name
    res_2 = _run(start, rows, t_max, qkv, kc, vc)
    assert np.array_equal(res_2['out'], res['out']), 'not deterministic'


def test_prompt_attn_large_scores():
    """q and k scaled by 8: score standard deviation ~ 60, maxima beyond 89 -- exp overflows without the running maximum, and a rescale applied
    to only one of l and the accumulator shows at once"""
    start, rows, t_max = 0, 130, 384
    qkv, kc, vc = _inputs(start, rows, t_max, 8.0)
    _, _, exact = _reference(start, rows, t_max, 8.0)
    out = _out(_run(start, rows, t_max, qkv, kc, vc), rows)
    assert np.isfinite(out.astype(np.float32)).all()
    err = rel_err(out, exact)
    print('prompt_attn large scores: rel err %.3e' % err)
    assert err < TOL, err


def test_prompt_attn_causality_within_the_chunk():
    start, rows, t_max, j = 0, 130, 384, 77
    qkv, kc, vc = _inputs(start, rows, t_max)
    base = _out(_run(start, rows, t_max, qkv, kc, vc), rows)
    qkv2 = qkv.copy()
    qkv2[j, H:] = np.random.default_rng(5).standard_normal(2 * H).astype(np.float16)     # the k and v parts of row j
    got = _out(_run(start, rows, t_max, qkv2, kc, vc), rows)
    assert np.array_equal(got[:j].view(np.uint16), base[:j].view(np.uint16)), 'a later row reached an earlier output'
    assert not np.array_equal(got[j].view(np.uint16), base[j].view(np.uint16))
    assert any(not np.array_equal(got[r].view(np.uint16), base[r].view(np.uint16)) for r in range(j + 1, rows))


def test_prompt_attn_reads_the_history_and_nothing_beyond():
    start, rows, t_max = 130, 70, 384
    qkv, kc, vc = _inputs(start, rows, t_max)
    base = _out(_run(start, rows, t_max, qkv, kc, vc), rows)
    rng = np.random.default_rng(6)
    kc2, vc2 = kc.copy(), vc.copy()
    kc2[start - 1] = (rng.standard_normal(H) * 4).astype(np.float16)
    vc2[start - 1] = (rng.standard_normal(H) * 4).astype(np.float16)
    got = _out(_run(start, rows, t_max, qkv, kc2, vc2), rows)
    assert all(not np.array_equal(got[r].view(np.uint16), base[r].view(np.uint16)) for r in range(rows)), 'a row did not see cache row start - 1'
    kc3, vc3 = kc.copy(), vc.copy()
    kc3[start + rows] = (rng.standard_normal(H) * 4).astype(np.float16)
    vc3[start + rows] = (rng.standard_normal(H) * 4).astype(np.float16)
    got = _out(_run(start, rows, t_max, qkv, kc3, vc3), rows)
    assert np.array_equal(got.view(np.uint16), base.view(np.uint16)), 'cache row start + rows reached the result'


def test_prompt_attn_agrees_with_the_decode_path():
    """the same 70 rows one at a time through gptq_decode_attn_batch_f16 (batch 1): identical caches, both outputs within the bar of float64"""
    start, rows, t_max = 130, 70, 384
    lib = _native.lib()
    s = torch.cuda.current_stream().cuda_stream
    qkv, kc, vc = _inputs(start, rows, t_max)
    _, _, exact = _reference(start, rows, t_max)
    res = _run(start, rows, t_max, qkv, kc, vc)
    qd, kd, vd = _dev(qkv), _dev(kc), _dev(vc)
    od = torch.zeros((rows, H), dtype=torch.float16, device=DEV)
    ws = torch.zeros(lib.gptq_decode_attn_batch_workspace_bytes(1, HEADS, HD, t_max), dtype=torch.uint8, device=DEV)
    pos = torch.arange(start, start + rows, dtype=torch.int64, device=DEV)
    for r in range(rows):
        rc = lib.gptq_decode_attn_batch_f16(qd[r].data_ptr(), 3 * H, pos[r:].data_ptr(), kd.data_ptr(), vd.data_ptr(), od[r].data_ptr(), H, ws.data_ptr(),
                                            ws.numel(), 1, HEADS, HD, t_max, BASE, SCALE, None, None, s)
        _native.check(rc, 'gptq_decode_attn_batch_f16')
    torch.cuda.synchronize()
    assert np.array_equal(res['kc'][GUARD:GUARD + t_max], _bits(kd))
    assert np.array_equal(res['vc'][GUARD:GUARD + t_max], _bits(vd))
    e_prompt, e_decode = rel_err(_out(res, rows), exact), rel_err(od.cpu().numpy(), exact)
    print('prompt %.3e, decode %.3e against float64' % (e_prompt, e_decode))
    assert e_prompt < TOL and e_decode < TOL, (e_prompt, e_decode)


def test_prompt_attn_strides():
    start, rows, t_max = 130, 70, 384
    qkv, kc, vc = _inputs(start, rows, t_max)
    base = _run(start, rows, t_max, qkv, kc, vc)
    res = _run(start, rows, t_max, qkv, kc, vc, ldq=3 * H + 64, ldo=H + 32)
    _check_guards(res, rows, t_max, ldo=H + 32)          # (the NaN padding of qkv and out rows included)
    assert np.array_equal(_out(res, rows).view(np.uint16), _out(base, rows).view(np.uint16))
    assert np.array_equal(res['kc'], base['kc']) and np.array_equal(res['vc'], base['vc'])


# ---- the engine ---------------------------------------------------------------------------------------------------------------
HD128 = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
             vocab_size=512, max_position_embeddings=512)
ENGINE_T_MAX = 160            # not a multiple of the kernel's key tile


@functools.lru_cache(maxsize=None)
def _model():
    return D.build_random_llama(DEV, seed=3, **HD128)


def _ids(n, seed):
    return torch.randint(0, HD128['vocab_size'], (1, n), device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _chain(model, ids, prefill):
    """the eager module chain, engine hook disabled, DynamicCache: logits after the prompt and after every further token, and the cache"""
    from transformers.cache_utils import DynamicCache
    cache = DynamicCache(config=model.config)
    outs = []
    model._gptq_engine_disabled = True
    try:
        with torch.no_grad():
            out = model(ids[:, :prefill], past_key_values=cache, use_cache=True)
            outs.append(out.logits[0, -1].float().cpu().numpy())
            kv = []
            for li in range(model.config.num_hidden_layers):
                k, v = D._cache_layer_kv(cache, li)
                kv.append((k[0].transpose(0, 1).reshape(prefill, -1).float().cpu().numpy(), v[0].transpose(0, 1).reshape(prefill, -1).float().cpu().numpy()))
            for i in range(prefill, ids.shape[1]):
                out = model(ids[:, i:i + 1], past_key_values=cache, use_cache=True)
                outs.append(out.logits[0, -1].float().cpu().numpy())
    finally:
        model._gptq_engine_disabled = False
    return np.stack(outs), kv


@functools.lru_cache(maxsize=None)
def _engine(batch=1):
    return D.DecodeEngine(_model(), t_max=ENGINE_T_MAX, batch=batch)


@pytest.mark.parametrize('T', [1, 9, 70, 127])
def test_engine_prefill_matches_the_module_chain(T):
    model, eng = _model(), _engine()
    ids = _ids(T + 8, 100 + T)
    expect, kv = _chain(model, ids, T)
    got = [eng.prefill(ids[0, :T], start=0).float().cpu().numpy()]
    assert int(eng.pos[0]) == T
    for li, (k, v) in enumerate(kv):
        assert np.abs(eng.kc[li, :T].float().cpu().numpy() - k).max() < KV_ATOL
        assert np.abs(eng.vc[li, :T].float().cpu().numpy() - v).max() < KV_ATOL
    for i in range(T, T + 8):                      # teacher-forced decode steps on the prefilled cache
        got.append(eng.decode(ids[0, i]).float().cpu().numpy()[0])
    for i, (g, e) in enumerate(zip(got, expect)):
        err = rel_err(g, e)
        print('prefill T=%d step %d: %.3e' % (T, i, err))
        assert err < HOOK_TOL, (T, i, err)


def test_engine_prefill_in_chunks():
    eng = _engine()
    ids = _ids(74, 7)
    one = [eng.prefill(ids[0, :70], start=0).float().cpu().numpy()]
    one += [eng.decode(ids[0, i]).float().cpu().numpy()[0] for i in range(70, 74)]
    eng.prefill(ids[0, :40], start=0)
    assert int(eng.pos[0]) == 40
    two = [eng.prefill(ids[:, 40:70]).float().cpu().numpy()]             # [1, T] ids, start=None: continue at pos
    assert int(eng.pos[0]) == 70
    two += [eng.decode(ids[0, i]).float().cpu().numpy()[0] for i in range(70, 74)]
    for i, (g, e) in enumerate(zip(two, one)):
        assert rel_err(g, e) < HOOK_TOL, (i, rel_err(g, e))


def test_engine_prefill_rows_of_a_batch_engine():
    model, eng = _model(), _engine(4)
    lens = [3, 20, 64, 65]
    prompts = [_ids(n + 1, 40 + n) for n in lens]
    for r in (0, 1, 3):
        eng.prefill(prompts[r][0, :lens[r]], row=r, start=0)
    snap = (eng.kcb.clone(), eng.vcb.clone(), eng.pos.clone())
    eng.prefill(prompts[2][0, :lens[2]], row=2, start=0)
    for r in (0, 1, 3):                                                 # the other rows: bit-unchanged
        assert torch.equal(eng.kcb[:, r].view(torch.int16), snap[0][:, r].view(torch.int16))
        assert torch.equal(eng.vcb[:, r].view(torch.int16), snap[1][:, r].view(torch.int16))
        assert int(eng.pos[r]) == int(snap[2][r]) == lens[r]
    assert int(eng.pos[2]) == lens[2]
    got = eng.decode(torch.stack([prompts[r][0, lens[r]] for r in range(4)])).float().cpu().numpy()
    for r in range(4):
        expect, _ = _chain(model, prompts[r], lens[r])
        err = rel_err(got[r], expect[1])
        print('batch row %d (prompt %d): %.3e' % (r, lens[r], err))
        assert err < HOOK_TOL, (r, err)


def test_engine_generate_with_the_engine_prefill():
    model = _model()
    prompt = _ids(23, 77)
    eng = D.DecodeEngine(model, t_max=64).capture()
    n_new = 24
    plain = D.engine_generate(model, prompt, max_new_tokens=n_new, engine=eng)
    hf = D.engine_generate(model, prompt, max_new_tokens=n_new, engine=eng, prefill='hf')
    assert torch.equal(plain, hf)                                        # 'hf' IS the route without the keyword
    got = D.engine_generate(model, prompt, max_new_tokens=n_new, engine=eng, prefill='engine')
    assert got.shape == hf.shape and torch.equal(got[:, :23], prompt)
    diff = (got[0] != hf[0]).nonzero()
    if diff.numel():
        # the sequences agree up to the first differing step; there the 'hf' run must have had a near tie (the only legitimate reason for a
        # flip) -- and what follows a flip is another sequence: one excused step, nothing to compare behind it.  The 'hf' run's own logits
        # of that step: the prompt's (module chain) for the first token, else what the engine holds after generating up to that token.
        p = int(diff[0])
        if p == 23:
            logits = _chain(model, prompt, 23)[0][0]
        else:
            again = D.engine_generate(model, prompt, max_new_tokens=p - 23 + 1, engine=eng, prefill='hf')
            assert torch.equal(again[0], hf[0, :p + 1])
            logits = eng.logits[0].float().cpu().numpy()
        top2 = np.sort(logits)[-2:]
        print('engine prefill: token %d differs, margin %.3e of max %.3e' % (p, top2[1] - top2[0], np.abs(logits).max()))
        assert top2[1] - top2[0] < HOOK_TOL * np.abs(logits).max(), ('engine prefill changed a token with a clear winner', p)


def test_engine_prefill_errors():
    model, eng = _model(), _engine()
    eng.prefill(_ids(5, 1)[0], start=0)
    with pytest.raises(ValueError):
        eng.prefill(_ids(11, 2)[0], start=ENGINE_T_MAX - 10)
    with pytest.raises(ValueError):
        eng.prefill(_ids(ENGINE_T_MAX, 3)[0])                            # start=None: 5 + t_max
    assert int(eng.pos[0]) == 5
    with pytest.raises(ValueError):
        D.engine_generate(model, _ids(4, 4), max_new_tokens=2, engine=eng, prefill='x')
