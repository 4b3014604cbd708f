"""GPU tests of constrained decoding in the engine (DecodeEngine(constrain=...), set_constraint / reset_constraint / constrain_logits, the
constraint launch inside the captured self-feeding steps, engine_generate / engine_generate_batch with constrain=).  The oracle is a HOST loop
on an engine WITHOUT the flag: its raw logits, step by step, through the numpy restatement of the kernel (tests/constrain_ref.py), the first
argmax, decode(token) -- so both sides see the same logits bits and no near-tie can part them.  A tiny random head_dim-128 model, t_max 64; a
synthetic 512-token vocabulary of byte strings stands in for a tokenizer."""
import functools
import re

import numpy as np
import pytest
import torch

import constrain_ref as R
import logits_process_ref as PR
import logprobs_ref as LP
from quant import decode as D
from quant.constrain import TokenDFA

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INF = float('inf')
HD128 = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
             vocab_size=512, max_position_embeddings=512)
V = HD128['vocab_size']
T_MAX = 64
NEW = 24
EOS = 2
NUMBER, LETTERS = r'-?\d{1,3}(\.\d\d)?', r'[a-c]{2,5}'          # bounded: FINAL is reached before NEW tokens


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
    return tuple(torch.randint(3, V, (6 + 4 * i,), device=DEV, generator=gen) for i in range(n))


@functools.lru_cache(maxsize=None)
def _vocab():
    """ids 0 .. 2 are specials (2 is eos), then every single byte of the alphabet, then strings of 2 .. 3 bytes, a few of them empty"""
    rng = np.random.default_rng(4)
    alphabet = b'0123456789-.abc'
    texts = [None, None, None] + [bytes([b]) for b in alphabet]
    while len(texts) < V:
        texts.append(bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=rng.integers(2, 4)).tolist()))
    for i in rng.integers(20, V, size=6):
        texts[i] = b''
    return texts


@functools.lru_cache(maxsize=None)
def _engine(batch=1, constrain=None, logprobs=None, logits_process=False):
    return D.DecodeEngine(_model(), t_max=T_MAX, batch=batch, constrain=constrain, logprobs=logprobs, logits_process=logits_process)


@functools.lru_cache(maxsize=None)
def _plain():
    return D.DecodeEngine(_model(), t_max=T_MAX).capture()


def _np16(t):
    return t.detach().to(torch.float16).cpu().numpy().reshape(-1)


def _cut(tokens, eos=EOS):
    return tokens[:tokens.index(eos) + 1] if eos in tokens else tokens


def _text(tokens):
    return b''.join(_vocab()[t] for t in tokens if t != EOS)


@functools.lru_cache(maxsize=None)
def _raw_greedy(prefill='engine'):
    ids = _prompts(1)[0][None]
    return D.engine_generate(_model(), ids, NEW, engine=_plain(), prefill=prefill)[0, ids.shape[1]:].tolist()


@functools.lru_cache(maxsize=None)
def _dfa(kind):
    """automata whose start state BANS the token unconstrained greedy emits first, so that the mask demonstrably acts"""
    g0 = _raw_greedy()[0]
    if kind == 'sequences':
        a, b, c, d = [(g0 + k) % (V - 3) + 3 for k in (7, 19, 101, 202)]          # four tokens that are neither g0 nor a special
        dfa = TokenDFA.from_sequences([[a, b, c], [a, d], [a, b, c, d, d], [c]], V, EOS)
    else:
        dfa = TokenDFA.from_regex(NUMBER, _vocab(), EOS)
        if dfa.allowed(0)[g0]:                                   # (a token cannot open both languages)
            dfa = TokenDFA.from_regex(LETTERS, _vocab(), EOS)
    assert not dfa.allowed(0)[g0]
    return dfa


def _pattern(dfa):
    """the regex a from_regex automaton of this file was built from"""
    digit = _vocab().index(b'7')
    return NUMBER if dfa.allowed(0)[digit] else LETTERS


def _other_regex():
    """the regex automaton _dfa('regex') is NOT"""
    return TokenDFA.from_regex(LETTERS if _pattern(_dfa('regex')) == NUMBER else NUMBER, _vocab(), EOS)


def _host_loop(prompt, prefill, new, dfa, pre=None, rows=None):
    """greedy under the automaton on the flag-off engine's raw logits: (processors first: pre(row, history),) restatement, first argmax,
    decode(token).  rows: a list that receives the masked fp16 row of every step"""
    eng, model = _plain(), _model()
    with torch.no_grad():
        logits = D._prompt_into_engine(model, prompt[None], eng, prefill)
        hist, out, state = prompt.tolist(), [], [0]
        for step in range(new):
            row = _np16(logits)
            if pre is not None:
                row = pre(row, hist)
            row, state = R.constrain_dfa(row[None], dfa, state, last=out[-1:] or None)
            assert state[0] >= 0 and not np.isnan(row.astype(np.float32)).any()
            if rows is not None:
                rows.append(row[0])
            out.append(int(np.argmax(row[0])))
            if out[-1] == EOS or step + 1 == new:
                break
            hist.append(out[-1])
            logits = eng.decode(out[-1])[0]
    return out


# ---- greedy, one prompt ----
@pytest.mark.parametrize('prefill', ['hf', 'engine'])
@pytest.mark.parametrize('kind', ['sequences', 'regex'])
def test_greedy_equals_the_host_loop(kind, prefill):
    model, eng, prompt, dfa = _model(), _engine(constrain=True), _prompts(1)[0], _dfa(kind)
    T = prompt.numel()
    out = D.engine_generate(model, prompt[None], NEW, eos_token_id=EOS, engine=eng, prefill=prefill, constrain=dfa)
    got = out[0, T:].tolist()
    want = _host_loop(prompt, prefill, NEW, dfa)
    print(kind, prefill, got, _text(got))
    assert torch.equal(out[0, :T], prompt) and got == want
    assert got[0] != _raw_greedy(prefill)[0] and got[-1] == EOS and len(got) < NEW       # FINAL was reached: eos, and the cut
    assert dfa.walk(got) >= 0
    if kind == 'regex':
        assert re.fullmatch(_pattern(dfa).encode(), _text(got)) is not None and len(got) >= 2
    # without eos_token_id nothing is cut: the row stays in FINAL and keeps emitting eos
    full = D.engine_generate(model, prompt[None], NEW, engine=eng, prefill=prefill, constrain=dfa)[0, T:].tolist()
    assert len(full) == NEW and full[:len(got)] == got and set(full[len(got):]) == {EOS}
    assert int(eng.c_state[0]) == dfa.walk(full[:-1])        # the state lags the stream by the one token not consumed yet


# ---- sampling ----
def test_sampled_tokens_stay_in_the_language():
    model, eng, prompt, dfa = _model(), _engine(constrain=True), _prompts(1)[0], _dfa('regex')
    T = prompt.numel()
    rx = re.compile(_pattern(dfa).encode())
    sample = dict(temperature=1.5)
    seen = set()
    for seed in range(6):
        torch.manual_seed(seed)
        free = D.engine_generate(model, prompt[None], 8, engine=_plain(), prefill='engine', sample=sample)[0, T:].tolist()
        assert dfa.walk(free) == -1                              # unconstrained draws leave the language within a few steps
        torch.manual_seed(seed)
        got = D.engine_generate(model, prompt[None], NEW, eos_token_id=EOS, engine=eng, prefill='engine', sample=sample, constrain=dfa)[0, T:].tolist()
        state = 0
        for t in got:                                            # every emitted token is allowed in its state
            assert dfa.allowed(state)[t], (seed, got, t)
            state = dfa.step(state, t)
        assert got[-1] == EOS and rx.fullmatch(_text(got)) is not None, (seed, got, _text(got))
        seen.add(tuple(got))
    print(sorted(_text(list(g)) for g in seen))
    assert len(seen) > 1                                         # it does sample


# ---- a batch of 3: automaton A, none, automaton B ----
def test_batch_rows_run_under_their_own_automata():
    model, prompts = _model(), list(_prompts(3))
    A, B = _dfa('sequences'), _dfa('regex')
    dfas = [A, None, B]
    eng = _engine(batch=3, constrain=True)
    outs = D.engine_generate_batch(model, prompts, NEW, eos_token_id=EOS, engine=eng, constrain=dfas)
    got = [o[p.numel():].tolist() for o, p in zip(outs, prompts)]
    plain = _engine(batch=3)
    with torch.no_grad():                                        # the host loop on the flag-off batch engine
        logits = plain.prefill_batch(prompts, starts=[0, 0, 0])
        state, want, last = [0, -1, 0], [[], [], []], None
        for step in range(NEW):
            rows = logits.to(torch.float16).cpu().numpy()
            for b, d in enumerate(dfas):
                if d is not None:
                    r, s = R.constrain_dfa(rows[b][None], d, [state[b]], last=None if last is None else [last[b]])
                    rows[b], state[b] = r[0], int(s[0])
            last = [int(np.argmax(r)) for r in rows]
            for b in range(3):
                want[b].append(last[b])
            logits = plain.decode(torch.tensor(last, device=DEV))
    print(got)
    for b in range(3):
        assert got[b] == _cut(want[b]), b
    assert got[0][-1] == EOS and got[2][-1] == EOS and A.walk(got[0]) >= 0 and B.walk(got[2]) >= 0
    assert re.fullmatch(_pattern(B).encode(), _text(got[2])) is not None
    free = D.engine_generate_batch(model, prompts, NEW, eos_token_id=EOS, engine=plain)
    assert got[1] == free[1][prompts[1].numel():].tolist()       # the unconstrained row is the flag-off engine's
    assert eng.c_state.tolist()[1] == -1
    # rows that pass the same object share its states and its class map
    eng.set_constraint([B, B, None])
    assert eng.c_map.tolist()[:2] == [0, 0] and eng.c_state.tolist() == [0, 0, -1]
    eng.set_constraint([A, B, A])
    assert eng.c_map.tolist() == [0, 1, 0] and eng.c_state.tolist() == [0, A.n_states, 0]
    eng.c_state.fill_(-2)
    eng.reset_constraint(rows=[1])
    assert eng.c_state.tolist() == [-2, A.n_states, -2]
    assert eng.reset_constraint().c_state.tolist() == [0, A.n_states, 0]


# ---- one capture serves every automaton ----
def test_one_captured_graph_serves_every_automaton():
    model, prompt = _model(), _prompts(1)[0]
    eng = D.DecodeEngine(model, t_max=T_MAX, constrain=True)
    T = prompt.numel()
    A, B = _dfa('regex'), _other_regex()
    a = D.engine_generate(model, prompt[None], NEW, eos_token_id=EOS, engine=eng, prefill='engine', constrain=A)[0, T:].tolist()
    graph = eng.greedy_graph
    assert graph is not None and a == _host_loop(prompt, 'engine', NEW, A)
    eng.set_constraint(B)
    assert eng.greedy_graph is graph                             # set_constraint never drops a graph
    b = D.engine_generate(model, prompt[None], NEW, eos_token_id=EOS, engine=eng, prefill='engine', constrain=B)[0, T:].tolist()
    assert eng.greedy_graph is graph and b == _host_loop(prompt, 'engine', NEW, B) and a != b
    assert re.fullmatch(_pattern(B).encode(), _text(b)) is not None
    # constrain=None on the same engine: the rows are unconstrained again, still the same graph
    free = D.engine_generate(model, prompt[None], NEW, engine=eng, prefill='engine')[0, T:].tolist()
    assert eng.greedy_graph is graph and free == _raw_greedy() and eng.c_state.tolist() == [-1]


def test_a_capture_leaves_the_states_where_they_were():
    model, dfa = _model(), _dfa('sequences')
    eng = D.DecodeEngine(model, t_max=T_MAX, constrain=dict(states=64, classes=16))
    eng.set_constraint(dfa)
    first = int(np.flatnonzero(dfa.allowed(0))[0])
    logits = torch.zeros((1, V), dtype=torch.float16, device=DEV)
    eng.constrain_logits(logits, last=torch.tensor([first], device=DEV))
    before = eng.c_state.tolist()
    assert before == [dfa.step(0, first)] and before != [0]
    nxt = int(np.flatnonzero(dfa.allowed(before[0]))[0])
    for capture in (eng.capture_sample_native, eng.capture_greedy_rows, eng.capture_greedy):
        eng.pos.zero_()
        eng.ids.fill_(nxt)                                       # a step from here WOULD move the state: the capture runs two
        capture()
        assert eng.c_state.tolist() == before, capture.__name__
    eng.greedy_graph.replay()                                    # ... and a replay does
    assert eng.c_state.tolist() == [dfa.step(before[0], nxt)]


# ---- with logprobs: the records are those of the constrained distribution ----
def test_logprobs_are_those_of_the_masked_logits():
    model, prompt, dfa = _model(), _prompts(1)[0], _dfa('regex')
    eng = _engine(constrain=True, logprobs=5)
    T = prompt.numel()
    seq, info = D.engine_generate(model, prompt[None], NEW, eos_token_id=EOS, engine=eng, prefill='engine', constrain=dfa, logprobs=5)
    got = seq[0, T:].tolist()
    rows = []
    assert got == _host_loop(prompt, 'engine', NEW, dfa, rows=rows) and len(rows) == len(got)
    state = 0
    for n, tok in enumerate(got):
        ok = dfa.allowed(state)
        top_ids, top_lp = info['top_ids'][n].cpu().numpy(), info['top_logprobs'][n].cpu().numpy()
        finite = np.isfinite(top_lp)
        assert finite.any() and ok[top_ids[finite]].all(), (n, top_ids, top_lp)
        assert finite.sum() == min(5, ok.sum())                  # banned tokens have -inf and sort last
        c, k, ti, tl = LP.record(rows[n], tok, 5)
        assert k == int(info['ranks'][n]) == 0 and ti.tolist() == top_ids.tolist(), n
        msg = LP.close(info['token_logprobs'][n:n + 1].cpu().numpy(), [c]) or LP.close(top_lp, tl)
        assert msg is None, (n, msg)
        state = dfa.step(state, tok)


# ---- with a processor: processors first, then the mask ----
def test_processors_act_before_the_mask():
    model, prompt, dfa = _model(), _prompts(1)[0], _dfa('regex')
    eng = _engine(constrain=True, logits_process=True)
    T = prompt.numel()
    sample = dict(temperature=0, repetition_penalty=1.3)
    out = D.engine_generate(model, prompt[None], NEW, eos_token_id=EOS, engine=eng, prefill='engine', sample=sample, constrain=dfa)
    got = out[0, T:].tolist()
    pre = lambda row, hist: PR.process_row(row, hist, T, 1.3, 0.0, 0, [EOS], [])
    assert got == _host_loop(prompt, 'engine', NEW, dfa, pre=pre)
    assert got[-1] == EOS and re.fullmatch(_pattern(dfa).encode(), _text(got)) is not None


# ---- eager, and the row that leaves its automaton ----
def test_a_banned_token_puts_the_row_at_minus_two_and_the_driver_raises():
    """The RuntimeError is provoked end to end: logit_bias = -inf on the only token the start state allows empties the first row of logits, the
    sampler's rule for a row of -inf only is its first element (token 0, a special that no state allows), and the first replay consumes it.
    That is deterministic on any model."""
    model, prompt = _model(), _prompts(1)[0]
    only = _vocab().index(b'a')
    dfa = TokenDFA.from_sequences([[only, only]], V, EOS)
    eng = _engine(constrain=True, logits_process=True)
    eng.set_constraint(dfa)
    x = torch.randn((1, V), device=DEV).to(torch.float16)
    y = eng.constrain_logits(x.clone(), last=torch.tensor([only], device=DEV))
    assert eng.c_state.tolist() == [1] and torch.isinf(y[0]).sum() == V - 1 and y[0, only] == x[0, only]
    z = eng.constrain_logits(x.clone(), last=torch.tensor([EOS], device=DEV))              # eos is banned there
    assert eng.c_state.tolist() == [-2] and torch.equal(z, x)
    assert torch.equal(eng.constrain_logits(x.clone()), x) and eng.c_state.tolist() == [-2]  # ... and the row stays out
    assert eng.reset_constraint().c_state.tolist() == [0]
    y1 = eng.constrain_logits(x[0].clone())                                                 # a 1-D row, no token consumed
    assert eng.c_state.tolist() == [0] and torch.isinf(y1).sum() == V - 1 and y1[only] == x[0, only]
    with pytest.raises(RuntimeError, match='row 0 left its automaton'):
        D.engine_generate(model, prompt[None], 6, eos_token_id=EOS, engine=eng, prefill='engine', constrain=dfa,
                          sample=dict(temperature=0, logit_bias={only: -INF}))
    ok = D.engine_generate(model, prompt[None], 6, eos_token_id=EOS, engine=eng, prefill='engine', constrain=dfa, sample=dict(temperature=0))
    assert ok[0, prompt.numel():].tolist() == [only, only, EOS]
    for bad in (x.float(), x[:, :V - 1], torch.zeros((2, V), dtype=torch.float16, device=DEV), x.cpu()):
        with pytest.raises(ValueError, match='logits must be fp16'):
            eng.constrain_logits(bad)
    with pytest.raises(ValueError, match='last must be'):
        eng.constrain_logits(x, last=torch.tensor([only], device=DEV, dtype=torch.int32))


# ---- flag off, and what is not built yet ----
def test_flag_off_and_unbuilt_combinations_raise():
    model, prompt, dfa = _model(), _prompts(1)[0], _dfa('sequences')
    plain = _plain()
    assert plain.constrain is None and not hasattr(plain, 'c_state')
    for call in (lambda: plain.set_constraint(dfa), lambda: plain.reset_constraint(),
                 lambda: plain.constrain_logits(torch.zeros((1, V), dtype=torch.float16, device=DEV)),
                 lambda: D.engine_generate(model, prompt[None], 4, engine=plain, constrain=dfa),
                 lambda: D.engine_generate_batch(model, list(_prompts(3)), 4, engine=_engine(batch=3), constrain=dfa)):
        with pytest.raises(ValueError, match='constrain'):
            call()
    for kw in (dict(chunk=4), dict(batch=2, batch_chunk=4), dict(batch=2, beam_search=True)):
        with pytest.raises(ValueError, match='not built yet'):
            D.DecodeEngine(model, t_max=T_MAX, constrain=True, **kw)
    for bad in (dict(states=0), dict(classes=16385), dict(states=32768), dict(rows=3), 5, 'yes'):
        with pytest.raises(ValueError, match='constrain'):
            D.DecodeEngine(model, t_max=T_MAX, constrain=bad)
    with pytest.raises(ValueError, match='not built yet'):
        D.engine_generate(model, prompt[None], 4, t_max=T_MAX, constrain=dfa, speculate=dict(k=3))
    with pytest.raises(ValueError, match='not built yet'):
        D.engine_generate_batch(model, list(_prompts(3)), 4, t_max=T_MAX, constrain=dfa, speculate=dict(k=3))
    with pytest.raises(ValueError, match='not built yet'):
        D.engine_generate_beam(model, prompt[None], 4, num_beams=2, t_max=T_MAX, constrain=dfa)
    for bad in ([dfa, dfa], 'a+', [None, 3, None]):
        with pytest.raises(ValueError, match='constrain must be'):
            D.engine_generate_batch(model, list(_prompts(3)), 4, t_max=T_MAX, constrain=bad)
    # constrain=None is the call as it always was
    a = D.engine_generate(model, prompt[None], 8, engine=plain, prefill='engine', constrain=None)
    assert torch.equal(a, D.engine_generate(model, prompt[None], 8, engine=plain, prefill='engine'))


def test_automata_beyond_the_capacities_raise_before_anything_changes():
    model, prompt = _model(), _prompts(1)[0]
    A, B = _dfa('sequences'), _dfa('regex')
    eng = D.DecodeEngine(model, t_max=T_MAX, batch=2, constrain=dict(states=A.n_states + 1, classes=max(A.n_classes, B.n_classes)))
    eng.set_constraint([A, None])
    before = [t.clone() for t in (eng.c_next, eng.c_cls, eng.c_map, eng.c_state)]
    other = TokenDFA.from_sequences([[5]], V - 1, EOS)
    for bad in ([A, B], [other, None], [A], A.next, [A, 'x']):
        with pytest.raises(ValueError, match='set_constraint'):
            eng.set_constraint(bad)
        assert all(torch.equal(t, t0) for t, t0 in zip((eng.c_next, eng.c_cls, eng.c_map, eng.c_state), before))
    small = D.DecodeEngine(model, t_max=T_MAX, constrain=dict(states=A.n_states, classes=1))
    with pytest.raises(ValueError, match='classes'):
        small.set_constraint(A)
    with pytest.raises(ValueError, match='set_constraint'):
        D.engine_generate(model, prompt[None], 4, engine=small, constrain=A)
    # engine=None: the driver takes the capacities from the automata
    out = D.engine_generate(model, prompt[None], NEW, eos_token_id=EOS, t_max=T_MAX, prefill='engine', constrain=A)
    assert out[0, prompt.numel():].tolist() == _host_loop(prompt, 'engine', NEW, A)
