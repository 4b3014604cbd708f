"""GPU tests of DecodeEngine(kv_cache='int4') on the tiny model of test_gpu_kv8_engine.py (hidden 256, 2 heads of 128, vocab 512, t_max 64, 2
layers) at batch 1 and 3 with prompts of different lengths: the prompt rows of its cache are the restatement (tests/kv4_ref.py) of the rows an
fp16 engine holds, graph and eager steps and driver and host loop agree to the bit, and what is not built is refused before anything changes."""
import pytest
import torch

import kv4_ref as R
from quant import decode as D
from test_gpu_kv4 import _bits
from test_gpu_kv8_engine import DEV, SHAPE, STEPS, T_MAX, _feed, _forced, _model, _tokens

pytestmark = pytest.mark.gpu
ARRAYS = ('k4b', 'v4b', 'kmetab', 'vmetab')


@pytest.mark.parametrize('B,route', [(1, 'engine'), (1, 'hf'), (3, 'engine')])
def test_prompt_rows_are_the_restatement_of_the_fp16_cache(B, route):
    """every layer's prompt rows (the prompt attends to unquantised rows) and all of layer 0's (they depend on the tokens only); logits printed"""
    model = _model(2)
    prompts, forced = _tokens(B)
    e16, e4 = D.DecodeEngine(model, t_max=T_MAX, batch=B), D.DecodeEngine(model, t_max=T_MAX, batch=B, kv_cache='int4')
    l16, l4 = _forced(e16, model, prompts, forced, route), _forced(e4, model, prompts, forced, route)
    assert e4.pos.tolist() == e16.pos.tolist() == [int(p.numel()) + STEPS for p in prompts]
    for b, p in enumerate(prompts):
        T = int(p.numel())
        for li, n in ((0, T + STEPS), (1, T)):
            for c16, q4, m4, what in ((e16.kcb, e4.k4b, e4.kmetab, 'k'), (e16.vcb, e4.v4b, e4.vmetab, 'v')):
                wq, wm = R.quantise(c16[li, b, :n])
                assert torch.equal(q4[li, b, :n].cpu(), wq), '%s codes of layer %d, row %d' % (what, li, b)
                assert torch.equal(_bits(m4[li, b, :n].cpu()), _bits(wm)), '%s metadata of layer %d, row %d' % (what, li, b)
    print('B %d, %s: max|logit4 - logit16| / max|logit16| over %d forced steps = %.3g, argmax agreement %.3f' % (
        B, route, STEPS, float((l4 - l16).abs().max() / l16.abs().max()), float((l4.argmax(-1) == l16.argmax(-1)).float().mean())))


@pytest.mark.parametrize('B', [1, 3])
def test_graph_and_eager_steps_give_the_same_logits(B):
    model = _model(2)
    prompts, _ = _tokens(B)
    eng = D.DecodeEngine(model, t_max=T_MAX, batch=B, kv_cache='int4')
    graph = eng.graph_for('greedy_rows')                              # before the prompts enter: the warm-up step writes cache row 0
    runs = []
    for replay in (True, False):
        first = _feed(eng, model, prompts, 'engine').argmax(dim=-1)
        eng.ids.copy_(first)
        eng.stepc.zero_()
        logits = []
        with torch.no_grad():
            for _ in range(4):
                graph.replay() if replay else eng._greedy_rows_step()
                logits.append(eng.logits.clone())
        runs.append((torch.stack(logits), eng.stream_rows[:4].clone()))
    assert torch.equal(runs[0][0].view(torch.int16), runs[1][0].view(torch.int16))
    assert torch.equal(runs[0][1], runs[1][1])


def test_drivers_equal_a_host_loop_of_decode_and_argmax():
    model, new, (prompts, _) = _model(2), 10, _tokens(3)
    got = D.engine_generate(model, prompts[0].unsqueeze(0), new, prefill='engine', kv_cache='int4')
    hf = D.engine_generate(model, prompts[0].unsqueeze(0), new, prefill='hf', kv_cache='int4')
    assert got.shape == hf.shape == (1, prompts[0].numel() + new)

    def loop(eng, ps):
        tok = _feed(eng, model, ps, 'engine').argmax(dim=-1)
        out = [tok.clone()]
        for _ in range(new - 1):
            tok = eng.decode(tok).argmax(dim=-1)
            out.append(tok.clone())
        return torch.stack(out, dim=1)
    want = loop(D.DecodeEngine(model, t_max=T_MAX, kv_cache='int4'), prompts[:1])
    assert torch.equal(got[0, prompts[0].numel():], want[0])
    rows = D.engine_generate_batch(model, list(prompts), new, t_max=T_MAX, kv_cache='int4')      # engine=None builds an int4 engine
    want = loop(D.DecodeEngine(model, t_max=T_MAX, batch=3, kv_cache='int4'), prompts)
    for b, p in enumerate(prompts):
        assert torch.equal(rows[b][p.numel():], want[b])


def test_what_is_not_built_is_refused_and_changes_nothing():
    model = _model(1)
    prompts, _ = _tokens(3)
    for kw in (dict(chunk=4), dict(batch=2, batch_chunk=2), dict(batch=2, beam_search=True), dict(fuse_attn=False)):
        with pytest.raises(ValueError, match='not built yet'):
            D.DecodeEngine(model, t_max=T_MAX, kv_cache='int4', **kw)
    grouped = D.build_random_llama(DEV, seed=3, num_hidden_layers=1, **dict(SHAPE, num_key_value_heads=1))
    with pytest.raises(ValueError, match='not built yet'):
        D.DecodeEngine(grouped, t_max=T_MAX, kv_cache='int4')
    eng = D.DecodeEngine(model, t_max=T_MAX, batch=3, kv_cache='int4')
    assert not hasattr(eng, 'kcb') and eng.k4b.shape == (1, 3, T_MAX, 128) and eng.kmetab.shape == (1, 3, T_MAX, 2, 4, 2)
    _feed(eng, model, prompts, 'engine')
    state = [getattr(eng, n).clone() for n in ('pos',) + ARRAYS]
    calls = [lambda: eng.prefill(prompts[0], row=1, start=3), lambda: eng.prefill(prompts[0], row=1),          # start=None: pos[1] = 10
             lambda: eng.prefill_batch(list(prompts), starts=[0, 2, 0]),
             lambda: eng.prefill_batch(list(prompts), max_rows=16),                                               # 30 packed rows: two passes
             lambda: eng.score(prompts[0]), lambda: eng.score_batch(list(prompts)),
             lambda: D.engine_generate(model, prompts[0].unsqueeze(0), 4, speculate=dict(k=2), kv_cache='int4')]
    for call in calls:
        with pytest.raises(ValueError, match='not built yet'):
            call()
    with pytest.raises(ValueError, match='kv_cache'):
        D.engine_generate_batch(model, list(prompts), 4, engine=eng, kv_cache='fp8')
    for n, t0 in zip(('pos',) + ARRAYS, state):
        assert torch.equal(_bits(getattr(eng, n)), _bits(t0)), n
