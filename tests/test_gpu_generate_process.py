"""GPU tests of the logit processors in the engine (DecodeEngine(logits_process=True), set_logits_process / set_history / process_logits, the
process launch inside the capture_sample_native graph, engine_generate / engine_generate_batch with repetition_penalty, presence_penalty,
min_new_tokens and logit_bias).  The oracle is a HOST loop on an engine WITHOUT the flag: its raw logits, step by step, through the numpy
restatement of the kernel (tests/logits_process_ref.py) and the first argmax -- so both sides see the same logits bits and no near-tie can part
them.  A tiny random head_dim-128 model, t_max 64."""
import functools

import numpy as np
import pytest
import torch

import logits_process_ref as R
from quant import decode as D

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INF = float('inf')
HD128 = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
             vocab_size=512, max_position_embeddings=512)
V = HD128['vocab_size']
T_MAX = 64
NEW = 24


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
def _prompts(n):
    gen = torch.Generator(device=DEV).manual_seed(70 + n)
    return tuple(torch.randint(1, V, (6 + 4 * i,), device=DEV, generator=gen) for i in range(n))


@functools.lru_cache(maxsize=None)
def _plain():
    return D.DecodeEngine(_model(), t_max=T_MAX).capture()


@functools.lru_cache(maxsize=None)
def _proc():
    return D.DecodeEngine(_model(), t_max=T_MAX, logits_process=True).capture()


@functools.lru_cache(maxsize=None)
def _plain3():
    return D.DecodeEngine(_model(), t_max=T_MAX, batch=3)


@functools.lru_cache(maxsize=None)
def _proc3():
    return D.DecodeEngine(_model(), t_max=T_MAX, batch=3, logits_process=True)


def _np16(t):
    return t.detach().to(torch.float16).cpu().numpy().reshape(-1)


def _cut(tokens, eos):
    return tokens[:tokens.index(eos) + 1] if eos in tokens else tokens


@functools.lru_cache(maxsize=None)
def _eos_and_ban(prefill):
    """E = the token unpenalised greedy emits first (so the min_new_tokens mask really acts), and the next different one to ban"""
    ids = _prompts(1)[0][None]
    greedy = D.engine_generate(_model(), ids, 12, engine=_plain(), prefill=prefill)[0, ids.shape[1]:].tolist()
    E = greedy[0]
    return E, next((t for t in greedy[1:] if t != E), (E + 1) % V)


def _host_loop(prompt, prefill, new, rp, pp, m, eos, bias):
    """greedy under the processors on the flag-off engine's raw logits: restatement, first argmax, decode(token)"""
    eng, model = _plain(), _model()
    with torch.no_grad():
        logits = D._prompt_into_engine(model, prompt[None], eng, prefill)
        hist, out = prompt.tolist(), []
        T = len(hist)
        for step in range(new):
            row = R.process_row(_np16(logits), hist, T, rp, pp, m, [] if eos is None else [eos], bias)
            assert not np.isnan(row.astype(np.float32)).any()
            out.append(int(np.argmax(row)))
            if out[-1] == eos or step + 1 == new:
                break
            hist.append(out[-1])
            logits = eng.decode(out[-1])[0]
    return out


@pytest.mark.parametrize('prefill', ['hf', 'engine'])
def test_graph_equals_the_host_loop(prefill):
    model, eng, prompt = _model(), _proc(), _prompts(1)[0]
    E, ban = _eos_and_ban(prefill)
    T = prompt.numel()
    sample = dict(temperature=0, repetition_penalty=1.3, presence_penalty=0.5, min_new_tokens=5, logit_bias={ban: -INF})
    out = D.engine_generate(model, prompt[None], NEW, eos_token_id=E, engine=eng, prefill=prefill, sample=sample)
    got = out[0, T:].tolist()
    want = _host_loop(prompt, prefill, NEW, 1.3, 0.5, 5, E, [(ban, -INF)])
    print(prefill, 'E', E, 'ban', ban, got)
    assert torch.equal(out[0, :T], prompt) and got == want
    assert E not in got[:5] and ban not in got and len(got) >= 6
    raw = D.engine_generate(model, prompt[None], NEW, eos_token_id=None, engine=_plain(), prefill=prefill)[0, T:].tolist()
    assert raw[0] == E and got != _cut(raw, E)                # the processors changed the tokens
    # the history invariant: hist[0, :pos] = prompt + consumed tokens (the run above may have stepped past its eos: compare what it consumed)
    full = D.engine_generate(model, prompt[None], NEW, engine=eng, prefill=prefill, sample=sample)[0]
    pos = int(eng.pos[0])
    assert pos == T + NEW - 1 and int(eng.gen_start[0]) == T
    assert torch.equal(eng.hist[0, :pos].to(torch.int64), full[:pos])


def test_batch_equals_the_host_loop_and_a_finished_row_disturbs_nobody():
    model, eng, plain = _model(), _proc3(), _plain3()
    prompts = list(_prompts(3))
    rp, pp, mn = [1.3, 1.0, 1.18], [0.5, 0.25, 0.0], [5, 0, 3]
    ban = (int(prompts[0][0]) + 1) % V
    bias = [(ban, -INF), (7 if ban != 7 else 8, 1.5)]

    def host(eos):
        with torch.no_grad():
            logits = plain.prefill_batch(prompts, starts=[0, 0, 0]).clone()
            hists = [p.tolist() for p in prompts]
            outs = [[], [], []]
            for step in range(NEW):
                toks = []
                for b in range(3):
                    row = R.process_row(_np16(logits[b]), hists[b], prompts[b].numel(), rp[b], pp[b], mn[b], [] if eos is None else [eos], bias)
                    toks.append(int(np.argmax(row)))
                    outs[b].append(toks[-1])
                    hists[b].append(toks[-1])
                if step + 1 < NEW:
                    logits = plain.decode(torch.tensor(toks, device=DEV))
        return outs
    E = host(None)[1][0]                                     # row 1 has no min_new_tokens: it emits its eos at once and is finished
    want = [_cut(o, E) for o in host(E)]
    out = D.engine_generate_batch(model, prompts, NEW, eos_token_id=E, engine=eng,
                                  sample=dict(temperature=0, repetition_penalty=rp, presence_penalty=pp, min_new_tokens=mn, logit_bias=dict(bias)))
    got = [o[p.numel():].tolist() for o, p in zip(out, prompts)]
    print('E', E, [len(g) for g in got])
    assert got == want and got[1] == [E]
    assert E not in got[0][:5] and E not in got[2][:3] and all(ban not in g for g in got) and len(got[0]) > 5
    pos = eng.pos.tolist()                                   # every row kept stepping: its history is prompt + what it consumed
    for b, p in enumerate(prompts):
        assert int(eng.gen_start[b]) == p.numel() and torch.equal(eng.hist[b, :p.numel()].to(torch.int64), p)
        assert pos[b] > p.numel() and eng.hist[b, p.numel():p.numel() + len(got[b]) - 1].tolist() == got[b][:-1]


def test_neutral_keys_take_todays_route(monkeypatch):
    model, prompt = _model(), _prompts(1)[0]
    built = []

    class Recording(D.DecodeEngine):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            built.append(self)
    monkeypatch.setattr(D, 'DecodeEngine', Recording)

    def run(sample):
        torch.manual_seed(11)
        return D.engine_generate(model, prompt[None], 16, t_max=T_MAX, prefill='engine', sample=sample)
    a = run(dict(temperature=0.8))
    b = run(dict(temperature=0.8, repetition_penalty=1.0, presence_penalty=0.0, min_new_tokens=0, logit_bias=None))
    c = run(dict(temperature=0.8, repetition_penalty=1.5))
    assert torch.equal(a, b) and c.shape == a.shape
    assert [e.logits_process for e in built] == [False, False, True] and not hasattr(built[1], 'hist')


def test_sampling_never_draws_a_banned_token_or_an_early_eos():
    model, eng, prompt = _model(), _proc(), _prompts(1)[0]
    E, ban = _eos_and_ban('engine')
    T = prompt.numel()
    for seed in range(4):
        torch.manual_seed(seed)
        out = D.engine_generate(model, prompt[None], NEW, eos_token_id=E, engine=eng, prefill='engine',
                                sample=dict(temperature=0.8, min_new_tokens=6, logit_bias={ban: -INF, E: 8.0}))
        gen = out[0, T:].tolist()
        assert ban not in gen and E not in gen[:6] and len(gen) >= 7, (seed, gen)
        assert gen[-1] == E or len(gen) == NEW                # (with + 8 on its logit the eos comes soon after the mask lifts)


def test_set_logits_process_between_replays_needs_no_recapture():
    model, eng, prompt = _model(), _proc(), _prompts(1)[0]
    D.engine_generate(model, prompt[None], 8, eos_token_id=3, engine=eng, prefill='engine', sample=dict(temperature=0, logit_bias={5: -INF}))
    g = eng.sample_native_graph
    assert g is not None
    pos, ids = eng.pos.clone(), eng.ids.clone()

    def step():
        eng.pos.copy_(pos)
        eng.ids.copy_(ids)
        eng.stepc.zero_()
        eng.sample_native_graph.replay()
        return int(eng.stream_rows[0, 0])
    a = step()
    assert step() == a
    eng.set_logits_process(eos_token_id=3, logit_bias={a: -INF})           # one eos id, one bias entry: the counts of the captured step
    assert eng.sample_native_graph is g
    b = step()
    assert b != a
    eng.set_logits_process(eos_token_id=b, min_new_tokens=T_MAX, logit_bias={a: -INF})
    assert eng.sample_native_graph is g and step() not in (a, b)
    eng.set_logits_process(eos_token_id=3, logit_bias={a: -INF, b: -INF})  # two entries: the launch argument changes, the graph goes
    assert eng.sample_native_graph is None


def test_set_history_and_process_logits():
    eng = _proc()
    eng.set_logits_process(repetition_penalty=2.0, presence_penalty=1.0)
    ids = torch.tensor([4, 9, 9, 300], device=DEV)
    eng.set_history(0, ids, gen_start=2)
    eng.pos.fill_(4)
    logits = torch.full((V,), 4.0, dtype=torch.float16, device=DEV)
    assert eng.process_logits(logits) is logits
    want = R.process_row(np.full(V, 4.0, np.float16), [4, 9, 9, 300], 2, 2.0, 1.0)
    assert np.array_equal(logits.cpu().numpy(), want) and want[4] == 2 and want[9] == 1 and want[300] == 1 and want[5] == 4
    assert eng.hist[0, :4].tolist() == [4, 9, 9, 300] and int(eng.gen_start[0]) == 2
    eng.set_history(0, ids)
    assert int(eng.gen_start[0]) == 4
    logits.fill_(4.0)
    eng.process_logits(logits, last=torch.tensor([17], device=DEV))          # consumed at position pos, not in hist yet: counted and appended
    assert float(logits[17]) == 1.0 and float(logits[9]) == 2.0 and int(eng.hist[0, 4]) == 17


def test_decode_returns_processed_logits_and_appends_its_tokens():
    eng, plain, prompt = _proc(), _plain(), _prompts(1)[0]
    eng.set_logits_process(repetition_penalty=1.3, presence_penalty=0.5, min_new_tokens=3, eos_token_id=[9, 11], logit_bias={4: -INF})
    T = prompt.numel()
    with torch.no_grad():
        eng.prefill(prompt, start=0)
        plain.prefill(prompt, start=0)
        hist = prompt.tolist()
        for step, tok in enumerate((17, int(prompt[0]), 17)):
            got, raw = _np16(eng.decode(tok)[0]), _np16(plain.decode(tok)[0])
            hist.append(tok)
            want = R.process_row(raw, hist, T, 1.3, 0.5, 3, [9, 11], [(4, -INF)])
            assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), step
            assert (got[9] == -INF) == (step < 2) and got[4] == -INF and not np.array_equal(got, raw)
    assert eng.hist[0, :len(hist)].tolist() == hist and int(eng.pos[0]) == len(hist) and int(eng.gen_start[0]) == T


def test_value_errors():
    model, prompt = _model(), _prompts(1)[0]
    for kw in (dict(chunk=4), dict(batch=2, batch_chunk=3)):
        with pytest.raises(ValueError, match='logits_process'):
            D.DecodeEngine(model, t_max=T_MAX, logits_process=True, **kw)
    with pytest.raises(ValueError, match='speculat'):
        D.engine_generate(model, prompt[None], 4, t_max=T_MAX, speculate=dict(k=2, sample=dict(temperature=0.8, repetition_penalty=1.2)))
    with pytest.raises(ValueError, match='speculat'):
        D.engine_generate_batch(model, list(_prompts(3)), 4, t_max=T_MAX, speculate=dict(k=2, sample=dict(temperature=0.8, min_new_tokens=2)))
    with pytest.raises(ValueError, match='logits_process=True'):
        D.engine_generate(model, prompt[None], 4, engine=_plain(), sample=dict(temperature=0, repetition_penalty=1.2))
    with pytest.raises(ValueError, match='logits_process=True'):
        D.engine_generate_batch(model, list(_prompts(3)), 4, engine=_plain3(), sample=dict(temperature=0, logit_bias={3: -1.0}))
    with pytest.raises(ValueError, match='logits_process=True'):
        _plain().set_logits_process(repetition_penalty=1.2)
    eng = _proc()
    for bad in (dict(eos_token_id=list(range(9))), dict(logit_bias=[(3, 1.0), (3, 2.0)]), dict(logit_bias={V: 1.0}), dict(logit_bias={-1: 1.0}),
                dict(logit_bias={i: 0.5 for i in range(257)}), dict(logit_bias={3: INF}), dict(logit_bias={3: float('nan')}),
                dict(repetition_penalty=0.0), dict(repetition_penalty=[1.0, 1.2]), dict(presence_penalty=INF), dict(min_new_tokens=-1),
                dict(min_new_tokens=1.5), dict(eos_token_id=2.0)):
        with pytest.raises(ValueError):
            eng.set_logits_process(**bad)
