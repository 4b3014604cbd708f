"""A grouped-query model (4 query heads on 2 K/V heads) through the fused module, the DecodeEngine and the engine hook: the fused chain against
the unfused HF chain, the engine against the module chain, the captured step against the eager one, model.generate through the hook against the
same call without it, and every path that has no grouped kernel yet refusing with 'not built yet' before it changes anything."""
import numpy as np
import pytest
import torch

from quant import decode as D
from quant.fused_attn import QuantLlamaAttention

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TWIN_TOL, HOOK_TOL = 1.2e-2, 2e-2        # the bars of tests/test_gpu_model.py (fused vs unfused chain; engine vs module chain), restated
CFG = dict(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=512,
           max_position_embeddings=128)
T_MAX = 64


@pytest.fixture(scope='module')
def model():
    return D.build_random_llama(DEV, bits=4, groupsize=128, seed=21, fused=True, **CFG)


def _ids(n, rows=1, seed=5):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    return torch.randint(1, CFG['vocab_size'], (rows, n), device=DEV, generator=gen)


def run_steps(m, ids, prefill):
    """the module chain, launch by launch, with the engine hook switched off: logits [steps, rows, vocab]"""
    from transformers.cache_utils import DynamicCache
    cache, outs = DynamicCache(config=m.config), []
    m._gptq_engine_disabled = True
    try:
        with torch.no_grad():
            outs.append(m(ids[:, :prefill], past_key_values=cache, use_cache=True).logits[:, -1].float().cpu().numpy())
            for i in range(prefill, ids.shape[1]):
                outs.append(m(ids[:, i:i + 1], past_key_values=cache, use_cache=True).logits[:, -1].float().cpu().numpy())
    finally:
        m._gptq_engine_disabled = False
    return np.stack(outs)


@pytest.mark.parametrize('heads,kv', [(4, 2), (8, 1)])        # 8 + 1: an odd number of heads to rotate
def test_fused_chain_matches_the_unfused_one_and_the_engine_the_fused(heads, kv):
    cfg = dict(CFG, hidden_size=heads * 128, num_attention_heads=heads, num_key_value_heads=kv)
    fused, plain = (D.build_random_llama(DEV, bits=4, groupsize=128, seed=21, fused=f, **cfg) for f in (True, False))
    attns = [l.self_attn for l in fused.model.layers]
    assert all(type(a) is QuantLlamaAttention and a.num_kv_heads == kv and a.num_heads == heads for a in attns)
    assert attns[0].qkv_proj.outfeatures == (heads + 2 * kv) * 128
    ids = _ids(12)
    a, b = run_steps(fused, ids, 5), run_steps(plain, ids, 5)
    assert np.isfinite(a).all() and np.abs(a - b).max() / np.abs(b).max() < TWIN_TOL
    eng = D.DecodeEngine(fused, t_max=T_MAX)                 # an HF prefill, then the engine's own steps
    assert eng.grouped and eng.kcb.shape == (2, 1, T_MAX, kv * 128) and eng.qkvb.shape == (1, (heads + 2 * kv) * 128)
    with torch.no_grad():
        got = [D._prompt_into_engine(fused, ids[:, :5], eng, 'hf').float().cpu().numpy()]
        for i in range(5, ids.shape[1]):
            got.append(eng.decode(ids[0, i]).float().cpu().numpy()[0])
    assert int(eng.pos[0]) == ids.shape[1]
    for g, r in zip(got, a[:, 0]):
        assert np.abs(g - r).max() / max(1.0, np.abs(r).max()) < HOOK_TOL


@pytest.mark.parametrize('batch', [1, 3])
def test_captured_step_matches_the_eager_step_to_the_bit(model, batch):
    eng = D.DecodeEngine(model, t_max=T_MAX, batch=batch)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(batch)
    k0 = (0.2 * torch.randn(eng.kcb.shape, device=DEV, generator=gen)).half()
    v0 = torch.randn(eng.vcb.shape, device=DEV, generator=gen).half()
    pos0 = torch.tensor([33, 0, T_MAX - 1][:batch], device=DEV)
    ids = _ids(1, rows=batch)[:, 0]

    def step(run):
        eng.kcb.copy_(k0), eng.vcb.copy_(v0), eng.pos.copy_(pos0), eng.ids.copy_(ids)
        with torch.no_grad():
            run()
        torch.cuda.synchronize()
        assert torch.equal(eng.pos, pos0 + 1)
        return eng.logits.clone(), eng.kcb.clone(), eng.vcb.clone()
    eager = step(eng._step)
    assert torch.isfinite(eager[0]).all() and not torch.equal(eager[1], k0)
    eng.capture()
    for _ in range(3):
        assert all(torch.equal(a, b) for a, b in zip(step(eng.graph.replay), eager))


def test_generate_through_the_hook_returns_the_eager_tokens(model):
    from quant.engine_hook import engine_steps
    one = _ids(6)
    three = _ids(7, rows=3, seed=9)
    mask = torch.ones_like(three)
    mask[1, :2] = 0
    mask[2, :4] = 0
    three = three * mask
    for ids, kw in ((one, dict(attention_mask=torch.ones_like(one))), (three, dict(attention_mask=mask))):
        kw.update(do_sample=False, max_new_tokens=12, min_new_tokens=12, pad_token_id=0)
        before = engine_steps(model)
        got = model.generate(ids, **kw)
        assert engine_steps(model) > before, 'the hook did not take the call'
        model._gptq_engine_disabled = True
        try:
            want = model.generate(ids, **kw)
        finally:
            model._gptq_engine_disabled = False
        assert torch.equal(got, want)
        if ids is one:
            assert torch.equal(D.engine_generate(model, one, 12, t_max=T_MAX), want)


REFUSED_BUILDS = [dict(chunk=4), dict(batch=2, batch_chunk=3), dict(chunk=4, tree=True), dict(batch=2, beam_search=True), dict(kv_cache='fp8'), dict(fuse_attn=False)]


def test_what_has_no_grouped_kernel_is_refused_before_anything_changes(model):
    for kw in REFUSED_BUILDS:
        with pytest.raises(ValueError, match='not built yet'):
            D.DecodeEngine(model, t_max=T_MAX, **kw)
    eng = D.DecodeEngine(model, t_max=T_MAX, batch=2)
    eng.pos.copy_(torch.tensor([3, 5], device=DEV))
    eng.kcb.fill_(0.25), eng.vcb.fill_(-0.5)
    state = [t.clone() for t in (eng.pos, eng.kcb, eng.vcb)]
    ids = _ids(6)
    calls = [lambda: eng.prefill(ids), lambda: eng.prefill_batch([ids[0], ids[0]]), lambda: eng.score(ids), lambda: eng.score_batch([ids[0]]),
             lambda: D.engine_generate(model, ids, 4, engine=eng, prefill='engine'), lambda: D.engine_generate(model, ids, 4, prefill='engine'),
             lambda: D.engine_generate_batch(model, [ids[0], ids[0]], 4, engine=eng), lambda: D.engine_generate_batch(model, [ids[0]], 4),
             lambda: D.engine_generate(model, ids, 4, kv_cache='fp8'), lambda: D.engine_generate_beam(model, ids, 4, num_beams=2)]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError, match='not built yet'):
            call()
        assert all(torch.equal(a, b) for a, b in zip((eng.pos, eng.kcb, eng.vcb), state)), i


def test_tensor_parallel_engine_refuses_a_grouped_model(model, monkeypatch):
    import torch.distributed as dist
    from quant.tp_decode import TPDecodeEngine
    monkeypatch.setattr(dist, 'get_rank', lambda group=None: 0)
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 1)
    with pytest.raises(ValueError, match='not built yet'):
        TPDecodeEngine(model, t_max=T_MAX)


def test_an_ungrouped_engine_keeps_its_shapes():
    cfg = dict(CFG, num_key_value_heads=4)
    plain = D.build_random_llama(DEV, bits=4, groupsize=128, seed=22, fused=True, **cfg)
    eng = D.DecodeEngine(plain, t_max=T_MAX, batch=2)
    assert not eng.grouped and eng.kcb.shape == eng.vcb.shape == (2, 2, T_MAX, 512) and eng.qkvb.shape == (2, 3 * 512)
    assert eng.attn_ws.numel() == eng.lib.gptq_decode_attn_batch_workspace_bytes(2, 4, 128, T_MAX)
