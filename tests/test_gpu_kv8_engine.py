"""GPU tests of DecodeEngine(kv_cache='fp8') on the tiny model of test_gpu_generate_constrain.py (hidden 256, 2 heads of 128, vocab 512, t_max 64)
with 1 and 2 layers, at batch 1 and 3 with prompts of different lengths: the cache an fp8 engine builds is the restatement (tests/kv8_ref.py) of
the cache an fp16 engine builds, the attention it computes is the float64 attention over its own dequantised cache, graph and eager steps and
driver and host loop agree to the bit, and what is not built is refused before anything changes."""
import functools

import pytest
import torch

import kv8_ref as R
from quant import decode as D

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPE = dict(hidden_size=256, intermediate_size=512, num_attention_heads=2, num_key_value_heads=2, vocab_size=512, max_position_embeddings=512)
V, T_MAX, STEPS, HEADS, HD = SHAPE['vocab_size'], 64, 12, 2, 128


@functools.lru_cache(maxsize=None)
def _model(layers):
    """scales x 0.05 keep the logits finite"""
    fill = D.fill_random_quant_

    def small(layer, gen):
        fill(layer, gen)
        layer.scales.mul_(0.05)
    D.fill_random_quant_ = small
    try:
        return D.build_random_llama(DEV, seed=3, num_hidden_layers=layers, **SHAPE)
    finally:
        D.fill_random_quant_ = fill


@functools.lru_cache(maxsize=None)
def _tokens(n):
    """n prompts of different lengths and STEPS teacher-forced tokens per row"""
    gen = torch.Generator(device=DEV).manual_seed(70 + n)
    prompts = tuple(torch.randint(3, V, (6 + 4 * i,), device=DEV, generator=gen) for i in range(n))
    return prompts, torch.randint(3, V, (STEPS, n), device=DEV, generator=gen)


def _feed(eng, model, prompts, route):
    """the prompts into the engine by `route`: 'engine' (prefill / prefill_batch) or 'hf' (one prompt through the module chain)"""
    with torch.no_grad():
        if route == 'hf':
            return D._prompt_into_engine(model, prompts[0].unsqueeze(0), eng, 'hf').reshape(1, -1)
        if len(prompts) == 1:
            return eng.prefill(prompts[0], start=0).reshape(1, -1).clone()
        return eng.prefill_batch(list(prompts), starts=[0] * len(prompts)).clone()


def _forced(eng, model, prompts, forced, route):
    _feed(eng, model, prompts, route)
    out = []
    for t in forced:
        out.append(eng.decode(t).float().cpu())
    torch.cuda.synchronize()
    return torch.stack(out)


@pytest.mark.parametrize('layers,B,route', [(1, 1, 'engine'), (1, 1, 'hf'), (1, 3, 'engine'), (2, 1, 'engine'), (2, 1, 'hf'), (2, 3, 'engine')])
def test_layer0_cache_is_the_restatement_of_the_fp16_cache(layers, B, route):
    """layer 0's K / V rows depend on the tokens only: after the prompts and 12 teacher-forced steps, bytes and exponents of the fp8 engine equal
    the quantised rows of the fp16 engine, byte for byte -- rows the store kernel wrote (prompt) and rows the attention appended (steps).  (The
    module-chain prompt route takes one prompt.)"""
    model = _model(layers)
    prompts, forced = _tokens(B)
    e16, e8 = D.DecodeEngine(model, t_max=T_MAX, batch=B), D.DecodeEngine(model, t_max=T_MAX, batch=B, kv_cache='fp8')
    l16, l8 = _forced(e16, model, prompts, forced, route), _forced(e8, model, prompts, forced, route)
    assert e8.pos.tolist() == e16.pos.tolist() == [int(p.numel()) + STEPS for p in prompts]
    for b, p in enumerate(prompts):
        n = int(p.numel()) + STEPS
        for c16, q8, x8, what in ((e16.kcb, e8.k8b, e8.kexpb, 'k'), (e16.vcb, e8.v8b, e8.vexpb, 'v')):
            wq, we = R.quantise(c16[0, b, :n])
            assert torch.equal(q8[0, b, :n].cpu(), wq), '%s bytes of row %d' % (what, b)
            assert torch.equal(x8[0, b, :n].cpu(), we), '%s exponents of row %d' % (what, b)
            assert not bool(q8[:, b, n:].any()) and not bool(x8[:, b, n:].any())       # nothing beyond the sequence was written
    print('layers %d, B %d, %s: max|logit8 - logit16| / max|logit16| over %d forced steps = %.3g, argmax agreement %.3f' % (
        layers, B, route, STEPS, float((l8 - l16).abs().max() / l16.abs().max()), float((l8.argmax(-1) == l16.argmax(-1)).float().mean())))


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('layers', [1, 2])
def test_last_layer_attention_matches_the_oracle_on_its_own_cache(layers, B):
    model = _model(layers)
    prompts, forced = _tokens(B)
    eng = D.DecodeEngine(model, t_max=T_MAX, batch=B, kv_cache='fp8')
    _forced(eng, model, prompts, forced[:3], 'engine')
    H, li, lib = HEADS * HD, layers - 1, eng.lib
    for b in range(B):
        p = int(eng.pos[b]) - 1                                       # the position the last step consumed
        one, scratch = eng.qkvb[b].clone(), torch.zeros((2, T_MAX, H), dtype=torch.float16, device=DEV)
        at = torch.tensor([p], dtype=torch.int64, device=DEV)
        assert lib.gptq_decode_rope_kv_f16(one.data_ptr(), at.data_ptr(), scratch[0].data_ptr(), scratch[1].data_ptr(), HEADS, HD, T_MAX,
                                           eng.layers[li]['theta'], None) == 0
        torch.cuda.synchronize()
        # the row the step appended is the quantised (rotated k, v) of qkvb
        wq, we = R.quantise(scratch[0, p])
        assert torch.equal(eng.k8b[li, b, p].cpu(), wq) and torch.equal(eng.kexpb[li, b, p].cpu(), we)
        ref = R.attention(one[:H], eng.k8b[li, b], eng.kexpb[li, b], eng.v8b[li, b], eng.vexpb[li, b], p + 1, eng.scale)
        err = float((eng.ab[b].double().cpu() - ref).abs().max() / ref.abs().max())
        assert err < 1e-3, 'row %d: %.3g' % (b, err)


@pytest.mark.parametrize('B', [1, 3])
def test_graph_and_eager_steps_give_the_same_logits(B):
    model = _model(2)
    prompts, _ = _tokens(B)
    eng = D.DecodeEngine(model, t_max=T_MAX, batch=B, kv_cache='fp8')
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
    model = _model(2)
    new = 10
    prompts, _ = _tokens(3)
    got = D.engine_generate(model, prompts[0].unsqueeze(0), new, prefill='engine', kv_cache='fp8')
    hf = D.engine_generate(model, prompts[0].unsqueeze(0), new, prefill='hf', kv_cache='fp8')
    assert got.shape == hf.shape == (1, prompts[0].numel() + new)

    def loop(eng, ps):
        tok = _feed(eng, model, ps, 'engine').argmax(dim=-1)
        out = [tok.clone()]
        for _ in range(new - 1):
            tok = eng.decode(tok).argmax(dim=-1)
            out.append(tok.clone())
        return torch.stack(out, dim=1)
    want = loop(D.DecodeEngine(model, t_max=T_MAX, kv_cache='fp8'), prompts[:1])
    assert torch.equal(got[0, prompts[0].numel():], want[0])
    eng = D.DecodeEngine(model, t_max=T_MAX, batch=3, kv_cache='fp8')
    rows = D.engine_generate_batch(model, list(prompts), new, engine=eng, kv_cache='fp8')
    want = loop(D.DecodeEngine(model, t_max=T_MAX, batch=3, kv_cache='fp8'), prompts)
    for b, p in enumerate(prompts):
        assert torch.equal(rows[b][p.numel():], want[b])
    built = D.engine_generate_batch(model, list(prompts), new, t_max=T_MAX, kv_cache='fp8')     # engine=None builds an fp8 engine
    assert all(torch.equal(x, y) for x, y in zip(built, rows))


def test_what_is_not_built_is_refused_and_changes_nothing():
    model = _model(1)
    prompts, _ = _tokens(3)
    for kw in (dict(chunk=4), dict(batch=2, batch_chunk=2), dict(batch=2, beam_search=True), dict(fuse_attn=False)):
        with pytest.raises(ValueError, match='not built yet'):
            D.DecodeEngine(model, t_max=T_MAX, kv_cache='fp8', **kw)
    with pytest.raises(ValueError, match='kv_cache'):
        D.DecodeEngine(model, t_max=T_MAX, kv_cache='bf16')
    eng = D.DecodeEngine(model, t_max=T_MAX, batch=3, kv_cache='fp8')
    _feed(eng, model, prompts, 'engine')
    state = [t.clone() for t in (eng.pos, eng.k8b, eng.v8b, eng.kexpb, eng.vexpb)]
    calls = [lambda: eng.prefill(prompts[0], row=1, start=3), lambda: eng.prefill(prompts[0], row=1),          # start=None: pos[1] = 10
             lambda: eng.prefill_batch(list(prompts), starts=[0, 2, 0]), lambda: eng.prefill_batch(list(prompts), starts=[0, None, 0]),
             lambda: eng.prefill_batch(list(prompts), max_rows=16),                                               # 30 packed rows: two passes
             lambda: eng.score(prompts[0]), lambda: eng.score_batch(list(prompts))]
    for call in calls:
        with pytest.raises(ValueError, match='not built yet'):
            call()
    for t, t0 in zip((eng.pos, eng.k8b, eng.v8b, eng.kexpb, eng.vexpb), state):
        assert torch.equal(t, t0)
    e16 = D.DecodeEngine(model, t_max=T_MAX, batch=3)
    with pytest.raises(ValueError, match='kv_cache'):
        D.engine_generate_batch(model, list(prompts), 4, engine=e16, kv_cache='fp8')
    with pytest.raises(ValueError, match='kv_cache'):
        D.engine_generate_batch(model, list(prompts), 4, engine=eng)
    with pytest.raises(ValueError, match='not built yet'):
        D.engine_generate(model, prompts[0].unsqueeze(0), 4, speculate=dict(k=2), kv_cache='fp8')
    for t, t0 in zip((eng.pos, eng.k8b), state):
        assert torch.equal(t, t0)


def test_flag_off_is_the_fp16_engine_and_flag_on_has_the_fp8_buffers():
    model = _model(2)
    B, H = 3, HEADS * HD
    e16, e8 = D.DecodeEngine(model, t_max=T_MAX, batch=B), D.DecodeEngine(model, t_max=T_MAX, batch=B, kv_cache='fp8')
    assert e16.kv_cache == 'fp16' and e16.kcb.shape == e16.vcb.shape == (2, B, T_MAX, H) and e16.kcb.dtype == torch.float16
    assert not any(hasattr(e16, n) for n in ('k8b', 'v8b', 'kexpb', 'vexpb', 'kst', 'vst'))
    assert e8.kv_cache == 'fp8' and not any(hasattr(e8, n) for n in ('kcb', 'vcb', 'kc', 'vc'))
    assert e8.k8b.shape == e8.v8b.shape == (2, B, T_MAX, H) and e8.k8b.dtype == e8.v8b.dtype == torch.uint8
    assert e8.kexpb.shape == e8.vexpb.shape == (2, B, T_MAX, HEADS) and e8.kexpb.dtype == e8.vexpb.dtype == torch.int8
    assert e8.kst.shape == e8.vst.shape == (B, T_MAX, H) and e8.kst.dtype == torch.float16
    assert not e8.attn_records and not D.DecodeEngine(model, t_max=T_MAX, kv_cache='fp8').attn_records
