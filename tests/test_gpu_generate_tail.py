"""GPU tests of the ONE tail loop of the generation drivers (quant/decode.py _self_feeding_tail behind engine_generate and
engine_generate_batch) at its edges: lengths around the 16-token burst and an eos at the first token and around the end of the first burst.
The oracle is a HOST loop on an engine of the same kind -- prefill, argmax, decode(token) -- run once without an eos for the longest length:
greedy decoding is deterministic, so the host loop of a shorter length or with an eos is that stream cut at the length and behind the first
eos.  The same stream gives the number of replays the burst rule allows, which the engine's positions must show afterwards.  A tiny random
head_dim-128 model, t_max 64."""
import functools

import pytest
import torch

from quant import decode as D

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HD128 = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
             vocab_size=512, max_position_embeddings=512)
V = HD128['vocab_size']
T_MAX = 64
LENGTHS = (1, 2, 16, 17, 18, 33)
LONGEST = max(LENGTHS)


@functools.lru_cache(maxsize=None)
def _model():
    """the tiny model of the sampling tests: scales x 0.05 keep the logits finite"""
    fill = D.fill_random_quant_

    def small(layer, gen):
        fill(layer, gen)
        layer.scales.mul_(0.05)
    D.fill_random_quant_ = small
    try:
        return D.build_random_llama(DEV, seed=3, **HD128)
    finally:
        D.fill_random_quant_ = fill


@functools.lru_cache(maxsize=None)
def _prompts():
    """three prompts of 6, 10 and 14 tokens.  Greedy streams of this tiny model often fall into a short cycle within a dozen tokens; under
    this seed no row repeats a token in its first 20.  The last prompt is the ONE prompt, and the row the eos tokens of the batch come from"""
    gen = torch.Generator(device=DEV).manual_seed(561)
    return tuple(torch.randint(1, V, (6 + 4 * i,), device=DEV, generator=gen) for i in range(3))


@functools.lru_cache(maxsize=None)
def _engine(batch):
    eng = D.DecodeEngine(_model(), t_max=T_MAX, batch=batch)
    return eng.capture() if batch == 1 else eng


@functools.lru_cache(maxsize=None)
def _host_streams(batch):
    """the eos-free greedy tokens of the host loop, LONGEST per row: one prompt on the batch-1 engine, the three on the batch-3 engine"""
    eng = _engine(batch)
    with torch.no_grad():
        if batch == 1:
            logits = D._prompt_into_engine(_model(), _prompts()[2][None], eng, 'engine').reshape(1, -1)
        else:
            logits = eng.prefill_batch(list(_prompts()), starts=[0] * batch)
        outs = [[] for _ in range(batch)]
        for step in range(LONGEST):
            toks = logits.argmax(dim=-1)
            for b, t in enumerate(toks.tolist()):
                outs[b].append(t)
            if step + 1 < LONGEST:
                logits = eng.decode(toks)
    return tuple(tuple(o) for o in outs)


def _eos_choices(stream):
    """None, the first generated token, and for i in (15, 16, 17) the token at the first index >= i that repeats no earlier token of the
    eos-free stream: its first occurrence lies at the end of the first burst, at the start of the second, and one further"""
    out = [None, stream[0]]
    for i in (15, 16, 17):
        fresh = [j for j in range(i, len(stream)) if stream[j] not in stream[:j]]
        assert fresh, 'the stream repeats itself from index %d on: %r' % (i, stream)
        out.append(stream[fresh[0]])
    return out


def _cut(tokens, n, eos):
    tokens = list(tokens[:n])
    return tokens[:tokens.index(eos) + 1] if eos in tokens else tokens


def _replays(streams, n, eos):
    """the burst rule on the host streams: bursts of min(16, what remains) until n tokens per row exist or every row has shown the eos"""
    done = 1
    while done < n and not (eos is not None and all(eos in s[:done] for s in streams)):
        done += min(16, n - done)
    return done - 1


@pytest.mark.parametrize('n', LENGTHS)
def test_one_prompt_equals_the_host_loop_and_replays_what_the_burst_rule_says(n):
    model, eng, prompt = _model(), _engine(1), _prompts()[2]
    stream, T = _host_streams(1)[0], prompt.numel()
    for eos in _eos_choices(stream):
        out = D.engine_generate(model, prompt[None], n, eos_token_id=eos, engine=eng, prefill='engine')
        got, want, replays = out[0, T:].tolist(), _cut(stream, n, eos), _replays([stream], n, eos)
        print('n', n, 'eos', eos, 'tokens', len(got), 'replays', replays)
        assert torch.equal(out[0, :T], prompt) and got == want, (n, eos)
        assert int(eng.pos[0]) == T + replays, (n, eos)


@pytest.mark.parametrize('n', LENGTHS)
def test_three_prompts_equal_the_host_loop_and_replay_what_the_burst_rule_says(n):
    model, eng, prompts = _model(), _engine(3), list(_prompts())
    streams = _host_streams(3)
    for eos in _eos_choices(streams[2]):
        out = D.engine_generate_batch(model, prompts, n, eos_token_id=eos, engine=eng)
        replays = _replays(streams, n, eos)
        print('n', n, 'eos', eos, 'tokens', [o.numel() - p.numel() for o, p in zip(out, prompts)], 'replays', replays)
        for b, p in enumerate(prompts):
            assert torch.equal(out[b][:p.numel()], p) and out[b][p.numel():].tolist() == _cut(streams[b], n, eos), (n, eos, b)
        assert eng.pos.tolist() == [p.numel() + replays for p in prompts], (n, eos)


def test_temperature_zero_takes_the_same_tail():
    model, prompts = _model(), list(_prompts())
    for n in LENGTHS:
        out = D.engine_generate(model, prompts[2][None], n, engine=_engine(1), prefill='engine', sample=dict(temperature=0))
        assert out[0, prompts[2].numel():].tolist() == list(_host_streams(1)[0][:n]), n
        assert int(_engine(1).pos[0]) == prompts[2].numel() + n - 1
        outs = D.engine_generate_batch(model, prompts, n, engine=_engine(3), sample=dict(temperature=0))
        assert [o[p.numel():].tolist() for o, p in zip(outs, prompts)] == [list(s[:n]) for s in _host_streams(3)], n
        assert _engine(3).pos.tolist() == [p.numel() + n - 1 for p in prompts]
