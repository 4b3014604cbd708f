"""GPU tests of DecodeEngine.prefill_batch / engine_generate_batch (quant/decode.py): several prompts of different lengths enter the engine
in one packed pass (gptq_prompt_attn_batch_f16), checked against the eager module chain per prompt (engine hook disabled, DynamicCache --
the reference of tests/test_gpu_prompt_attn.py, whose bars HOOK_TOL and KV_ATOL these are) and against the single-row routes."""
import functools

import numpy as np
import pytest
import torch

from quant import decode as D
from util import rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HOOK_TOL = 2e-2      # logits through the engine vs the eager chain (fp16 KV cache on both sides)
KV_ATOL = 4e-3       # rotated cache rows against the HF cache (one fp16 rounding of values up to ~4)
HD128 = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
             vocab_size=512, max_position_embeddings=512)
ENGINE_T_MAX = 160            # not a multiple of the kernel's key tile
LENS = [3, 20, 64, 65]
STEPS = 4


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
def _engine(batch=4):
    return D.DecodeEngine(_model(), t_max=ENGINE_T_MAX, batch=batch)


@functools.lru_cache(maxsize=None)
def _prompts():
    """ids of LENS[r] + STEPS tokens per row: the prompt and the teacher-forced continuation"""
    return tuple(_ids(n + STEPS, 40 + n) for n in LENS)


def _one_pass(eng, **kw):
    """prefill_batch of the four prompts + STEPS teacher-forced batched decode steps: logits [1 + STEPS][4][vocab], positions after the prefill"""
    ids = _prompts()
    got = [eng.prefill_batch([ids[r][0, :LENS[r]] for r in range(4)], **kw).float().cpu().numpy()]
    pos = eng.pos.tolist()
    for i in range(STEPS):
        got.append(eng.decode(torch.stack([ids[r][0, LENS[r] + i] for r in range(4)])).float().cpu().numpy())
    return np.stack(got), pos


def test_prefill_batch_matches_the_module_chain():
    model, eng = _model(), _engine()
    got, pos = _one_pass(eng)
    assert pos == LENS
    eng.prefill_batch([_prompts()[r][0, :LENS[r]] for r in range(4)])          # the caches right after the prompts
    for r in range(4):
        expect, kv = _chain(model, _prompts()[r], LENS[r])
        for li, (k, v) in enumerate(kv):
            assert np.abs(eng.kcb[li, r, :LENS[r]].float().cpu().numpy() - k).max() < KV_ATOL
            assert np.abs(eng.vcb[li, r, :LENS[r]].float().cpu().numpy() - v).max() < KV_ATOL
        for i in range(1 + STEPS):
            err = rel_err(got[i, r], expect[i])
            print('prefill_batch row %d (T = %d) step %d: %.3e' % (r, LENS[r], i, err))
            assert err < HOOK_TOL, (r, i, err)


def test_prefill_batch_in_passes():
    """max_rows = 48 of 152 packed rows: four passes, the 64- and the 65-token prompt each straddle a boundary"""
    eng = _engine()
    one, pos_one = _one_pass(eng)
    rows_before = eng._prefill_bufs['x'].shape[0]
    passes, pos_passes = _one_pass(eng, max_rows=48)
    assert pos_passes == pos_one == LENS
    assert eng._prefill_bufs['x'].shape[0] == rows_before                      # the buffers are kept (and never grow beyond what a call needs)
    for i in range(1 + STEPS):
        for r in range(4):
            err = rel_err(passes[i, r], one[i, r])
            print('passes row %d step %d: %.3e' % (r, i, err))
            assert err < HOOK_TOL, (r, i, err)
    fresh = D.DecodeEngine(_model(), t_max=ENGINE_T_MAX, batch=4)
    fresh.prefill_batch([_prompts()[r][0, :LENS[r]] for r in range(4)], max_rows=48)
    assert fresh._prefill_bufs['x'].shape[0] == 48                             # min(sum T, max_rows) rows


def test_prefill_batch_subset_of_rows():
    eng = _engine()
    ids = _prompts()
    eng.prefill(ids[1][0, :LENS[1]], row=1, start=0)
    eng.prefill(ids[3][0, :LENS[3]], row=3, start=0)
    single = {r: eng.prefill(ids[r][0, :LENS[r]], row=r, start=0).float().cpu().numpy() for r in (2, 0)}
    eng.pos[0] = 7                                                              # must be overwritten: starts default to 0
    snap = (eng.kcb.clone(), eng.vcb.clone(), eng.pos.clone())
    got = eng.prefill_batch([ids[2][0, :LENS[2]], ids[0][0, :LENS[0]]], rows=[2, 0]).float().cpu().numpy()
    for r in (1, 3):                                                            # the rows not named: bit-unchanged
        assert torch.equal(eng.kcb[:, r].view(torch.int16), snap[0][:, r].view(torch.int16))
        assert torch.equal(eng.vcb[:, r].view(torch.int16), snap[1][:, r].view(torch.int16))
        assert int(eng.pos[r]) == int(snap[2][r]) == LENS[r]
    assert int(eng.pos[2]) == LENS[2] and int(eng.pos[0]) == LENS[0]
    assert torch.equal(eng.logits[[2, 0]].float().cpu(), torch.from_numpy(got))
    for i, r in enumerate((2, 0)):
        err = rel_err(got[i], single[r])
        print('subset row %d: %.3e against prefill' % (r, err))
        assert err < HOOK_TOL, (r, err)
    # starts: a None entry continues at pos[row] -- the second half of a prompt lands behind the first
    eng.prefill_batch([ids[2][0, :30]], rows=[2])
    assert int(eng.pos[2]) == 30
    cont = eng.prefill_batch([ids[2][0, 30:LENS[2]], ids[0][0, :LENS[0]]], rows=[2, 0], starts=[None, 0]).float().cpu().numpy()
    assert int(eng.pos[2]) == LENS[2]
    assert rel_err(cont[0], single[2]) < HOOK_TOL and rel_err(cont[1], single[0]) < HOOK_TOL


def test_prefill_batch_errors():
    eng = _engine()
    eng.prefill_batch([_ids(5, 1)[0], _ids(6, 2)[0]])
    pos = eng.pos.tolist()
    a, b = _ids(4, 3)[0], _ids(9, 4)[0]
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    bad = [dict(prompts=[a, empty]),                                            # an empty prompt
           dict(prompts=[]),
           dict(prompts=[a] * 5),                                               # more prompts than rows
           dict(prompts=[a, b], rows=[1, 1]),                                   # duplicate rows
           dict(prompts=[a, b], rows=[0, 4]),                                   # a row outside the batch
           dict(prompts=[a, b], rows=[0, -1]),
           dict(prompts=[a, b], rows=[0]),
           dict(prompts=[a, b], starts=[0, ENGINE_T_MAX - 8]),                  # positions .. t_max: one too many
           dict(prompts=[a, b], starts=[-1, 0]),
           dict(prompts=[a, _ids(ENGINE_T_MAX - 5, 5)[0]], starts=[0, None]),   # continues at pos[1] = 6
           dict(prompts=[a, b], starts=[0]),
           dict(prompts=[a, b], max_rows=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.prefill_batch(**kw)
        assert eng.pos.tolist() == pos, kw
    eng.prefill_batch([a, b], starts=[0, ENGINE_T_MAX - 9])                     # the last position that fits
    assert eng.pos.tolist()[:2] == [4, ENGINE_T_MAX]
    eng.reset()                                                                 # (a shared engine: leave no row at the end of its cache)


def test_engine_generate_batch():
    model = _model()
    lens, n_new = [5, 23, 40], 12
    prompts = [_ids(n, 300 + n)[0] for n in lens]
    one = D.DecodeEngine(model, t_max=64).capture()
    free = D.engine_generate(model, prompts[1].unsqueeze(0), max_new_tokens=n_new, engine=one, prefill='engine')[0]
    eos = int(free[lens[1] + 5])                                                # occurs in row 1: that row is cut, at the latest there
    eng = D.DecodeEngine(model, t_max=64, batch=3)
    got = D.engine_generate_batch(model, prompts, max_new_tokens=n_new, eos_token_id=eos, engine=eng)
    assert len(got) == 3
    refs = [D.engine_generate(model, p.unsqueeze(0), max_new_tokens=n_new, eos_token_id=eos, engine=one, prefill='engine')[0] for p in prompts]
    assert refs[1].numel() <= lens[1] + 6 < lens[1] + n_new and int(refs[1][-1]) == eos
    for r, (g, ref) in enumerate(zip(got, refs)):
        T = lens[r]
        assert g.dim() == 1 and g.dtype == prompts[r].dtype and torch.equal(g[:T], prompts[r])
        assert T < g.numel() <= T + n_new
        assert (g[T:-1] != eos).all()                                           # cut after the FIRST eos
        assert g.numel() == T + n_new or int(g[-1]) == eos
        m = min(g.numel(), ref.numel())
        diff = (g[:m] != ref[:m]).nonzero()
        if not diff.numel():
            assert g.numel() == ref.numel(), (r, g.numel(), ref.numel())
            continue
        # the sequences agree up to the first differing step; there the single-prompt run must have had a near tie (the only legitimate reason
        # for a flip) -- and what follows a flip is another sequence: one excused step, nothing to compare behind it.  The reference run's own
        # logits of that step: what its engine holds after the prompt, or after generating up to that token.
        p = int(diff[0])
        if p == T:
            logits = one.prefill(prompts[r], start=0).float().cpu().numpy()
        else:
            again = D.engine_generate(model, prompts[r].unsqueeze(0), max_new_tokens=p - T + 1, engine=one, prefill='engine')[0]
            assert torch.equal(again, ref[:p + 1])
            logits = one.logits[0].float().cpu().numpy()
        top2 = np.sort(logits)[-2:]
        print('generate_batch row %d: token %d differs, margin %.3e of max %.3e' % (r, p, top2[1] - top2[0], np.abs(logits).max()))
        assert top2[1] - top2[0] < HOOK_TOL * np.abs(logits).max(), ('the batch route changed a token with a clear winner', r, p)
    with pytest.raises(ValueError):
        D.engine_generate_batch(model, prompts[:2], max_new_tokens=4, engine=eng)           # engine.batch != len(prompts)
    with pytest.raises(ValueError):
        D.engine_generate_batch(model, prompts, max_new_tokens=25, engine=eng)              # 40 + 25 > t_max
