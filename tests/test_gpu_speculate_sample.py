"""GPU tests of the engine's speculative-sampling step: DecodeEngine(chunk=R).verify_sample / capture_verify_sample on the tiny head_dim-128 model
of the other engine tests (quant/decode.py; the kernel itself: tests/test_gpu_spec_sample.py)."""
import functools

import numpy as np
import pytest
import torch

import spec_sample_ref as X
from quant import decode as D

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HD128 = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
             vocab_size=512, max_position_embeddings=512)
VOCAB, T_MAX, R, PROMPT = HD128['vocab_size'], 160, 5, 23


@functools.lru_cache(maxsize=None)
def _model():
    """finite logits: the initialisation of the sampling tests (scales x 0.05)"""
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
def _engine():
    return D.DecodeEngine(_model(), t_max=T_MAX, chunk=R)


def _prompt(seed=77):
    return torch.randint(1, VOCAB, (PROMPT,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _start(eng):
    """the prompt in the cache, pos = PROMPT; returns the greedy first token"""
    return int(eng.prefill(_prompt(), start=0).argmax())


def _u(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(R, generator=g).to(DEV), torch.rand(R, generator=g).to(DEV)


def test_verify_sample_follows_the_oracle_on_the_steps_own_logits():
    eng = _engine()
    first = _start(eng)
    eng.set_sampling(temperature=1.3, top_k=0, top_p=1.0)
    tokens = [first] + torch.topk(eng.logits[0].float(), R - 1).indices.tolist()
    for seed, dl in ((1, None), (2, None), (3, torch.randn(R - 1, VOCAB, generator=torch.Generator().manual_seed(9)).half().to(DEV))):
        eng.pos.fill_(PROMPT)
        ua, ud = _u(seed)
        a, out = eng.verify_sample(tokens, draft_logits=dl, u_accept=ua, u_draw=ud)
        assert int(eng.pos[0]) == PROMPT + a + 1 and len(out) == a + 1 and out[:a] == tokens[1:a + 1]
        rec = eng.spec_ws[1:].cpu().numpy()
        flags, toks = (rec >> 32).astype(bool), (rec & 0xFFFFFFFF).astype(np.int64)
        P = eng.chunk_logits.cpu()
        assert torch.isfinite(P.float()).all()
        ok = X.admissible(flags, toks, P, tokens, None if dl is None else dl.cpu(), 1.3, 0, 1.0, ua.cpu().numpy(), ud.cpu().numpy())
        assert ok.all(), (seed, flags, toks)
        assert a == (int(np.argmin(flags[:R - 1])) if not flags[:R - 1].all() else R - 1) and out[a] == int(toks[a])


def test_eager_and_graph_agree_for_equal_uniforms():
    eng = _engine()
    first = _start(eng)
    eng.set_sampling(temperature=1.5, top_k=50, top_p=0.95)
    tokens = torch.tensor([first] + torch.topk(eng.logits[0].float(), R - 1).indices.tolist(), device=DEV)
    for with_q in (False, True):
        dl = torch.randn(R - 1, VOCAB, generator=torch.Generator().manual_seed(4)).half().to(DEV) if with_q else None
        eng.pos.fill_(PROMPT)
        torch.manual_seed(21)
        a, out = eng.verify_sample(tokens, draft_logits=dl)
        eng.pos.fill_(PROMPT)
        torch.manual_seed(21)
        before = torch.cuda.get_rng_state(DEV)
        g = eng.capture_verify_sample(draft_logits=with_q)
        assert torch.equal(torch.cuda.get_rng_state(DEV), before) and int(eng.pos[0]) == PROMPT
        assert eng.verify_sample_graphs[with_q] is g
        eng.chunk_ids.copy_(tokens)
        if with_q:
            eng.chunk_draft_logits.copy_(dl)
        g.replay()
        res = eng.verify_out.tolist()
        assert (res[0], res[1:res[0] + 2]) == (a, out) and int(eng.pos[0]) == PROMPT + a + 1


def test_temperature_zero_is_the_verify_greedy_step():
    eng = _engine()
    first = _start(eng)
    am = torch.topk(eng.logits[0].float(), 2).indices.tolist()
    eng.set_sampling(temperature=0)
    plain = D.engine_generate(_model(), _prompt()[None], R + 3, engine=D.DecodeEngine(_model(), t_max=T_MAX).capture(), prefill='engine')[0, PROMPT:]
    for drafts in (plain[1:R].tolist(), [plain[1].item(), plain[2].item()] + am + [0], [am[1]] * (R - 1)):
        tokens = torch.tensor([first] + drafts[:R - 1], device=DEV)
        _start(eng)
        eng.chunk_ids.copy_(tokens)
        with torch.no_grad():
            eng._verify_greedy_step()
        want = eng.verify_out.tolist()
        _start(eng)
        a, out = eng.verify_sample(tokens)
        assert (a, out) == (want[0], want[1:want[0] + 2]) and int(eng.pos[0]) == PROMPT + a + 1, (drafts, a, out, want)


def test_short_steps_are_padded_and_bad_arguments_refused():
    eng = _engine()
    first = _start(eng)
    eng.set_sampling(temperature=1.0)
    ua, ud = torch.zeros(R, device=DEV), torch.full((R,), 0.5, device=DEV)
    top = int(torch.topk(eng.logits[0].float(), 1).indices[0])
    a, out = eng.verify_sample([first, top], u_accept=ua, u_draw=ud)             # u_accept = 0 accepts every draft the target keeps
    assert a == 1 and len(out) == 2 and out[0] == top and int(eng.pos[0]) == PROMPT + 2
    eng.pos.fill_(PROMPT)
    for bad in (dict(tokens=[first]), dict(tokens=[first] * (R + 1)), dict(tokens=[first, top], u_accept=ua[:2]),
                dict(tokens=[first, top], draft_logits=torch.zeros(2, VOCAB, dtype=torch.float16, device=DEV))):
        with pytest.raises(ValueError):
            eng.verify_sample(**bad)
        assert int(eng.pos[0]) == PROMPT
    eng.pos.fill_(T_MAX - R + 1)
    with pytest.raises(ValueError):
        eng.verify_sample([first, top])
    with pytest.raises(ValueError):
        eng.capture_verify_sample()
    with pytest.raises(ValueError):
        D.DecodeEngine(_model(), t_max=T_MAX).verify_sample([first, top])
    eng.pos.fill_(PROMPT)


# ---- engine_generate(speculate=dict(sample=..., draft_model=...)) ---------------------------------------------------------------------------------
K, NEW, T_END = R - 1, 24, 132
SETTING = dict(temperature=0.8, top_p=0.95)                      # the reference script's default call


@functools.lru_cache(maxsize=None)
def _draft_model(seed):
    """a random tiny model of the same vocabulary with ONE layer, finite logits as _model()"""
    fill = D.fill_random_quant_

    def small(layer, gen):
        fill(layer, gen)
        layer.scales.mul_(0.05)
    D.fill_random_quant_ = small
    try:
        return D.build_random_llama(DEV, seed=seed, **dict(HD128, num_hidden_layers=1))
    finally:
        D.fill_random_quant_ = fill


def _gen(prompt, new=NEW, eos=None, **speculate):
    out = D.engine_generate(_model(), prompt[None], new, eos_token_id=eos, engine=_engine(), prefill='engine', speculate=dict(k=K, **speculate))
    assert torch.equal(out[0, :prompt.numel()], prompt)
    g = out[0, prompt.numel():]
    assert int(g.min()) >= 0 and int(g.max()) < VOCAB
    return g.tolist()


def _oracle(prompt, known):
    full = prompt.tolist() + known
    return lambda toks, k: (full[len(toks):len(toks) + k] + [0] * k)[:k]


def test_top_k_one_gives_the_greedy_speculative_tokens():
    prompt = _prompt()
    greedy = _gen(prompt)
    stats = _engine().spec_stats
    assert _gen(prompt, sample=dict(top_k=1)) == greedy and len(greedy) == NEW
    assert _engine().spec_stats == stats
    assert _gen(prompt, sample=dict(temperature=0)) == greedy


def test_seeded_runs_agree_and_an_oracle_draft_is_accepted_whole():
    prompt = _prompt()
    torch.manual_seed(3)
    a = _gen(prompt, sample=dict(temperature=1.5))
    torch.manual_seed(3)
    b = _gen(prompt, sample=dict(temperature=1.5))
    torch.manual_seed(4)
    c = _gen(prompt, sample=dict(temperature=1.5))
    assert a == b and a != c and len(a) == NEW
    st = _engine().spec_stats
    assert st['steps'] == len(st['accepted']) > 0 and all(0 <= x <= K for x in st['accepted']) and st['steps'] <= st['emitted'] <= NEW - 1
    # a draft that knows the (deterministic: top_k = 1) continuation: every step accepts every token the draft knew
    known = _gen(prompt, sample=dict(top_k=1))
    assert _gen(prompt, sample=dict(top_k=1), draft=_oracle(prompt, known)) == known
    st = _engine().spec_stats
    # (the last step's draft holds only the (NEW - 1) % R tokens the oracle still knows, then padding)
    assert st['accepted'] == [K] * ((NEW - 1) // R) + [(NEW - 1) % R] and st['emitted'] == NEW - 1, st
    assert int(_engine().pos[0]) == PROMPT + NEW - 1


def test_draft_model():
    prompt = _prompt()
    eng = _engine()
    for seed in (3, 11):                                         # the target's own seed, and another one
        torch.manual_seed(5)
        a = _gen(prompt, sample=SETTING, draft_model=_draft_model(seed))
        st = dict(eng.spec_stats)
        print('draft model, seed %d: %r' % (seed, st))
        assert len(a) == NEW and st['steps'] > 0 and all(0 <= x <= K for x in st['accepted'])
        if seed == 3:
            assert sum(st['accepted']) > 0
        torch.manual_seed(5)
        assert _gen(prompt, sample=SETTING, draft_model=_draft_model(seed)) == a
        assert eng._draft_engine[0] is _draft_model(seed)
    # without `sample` the draft model drafts greedily and the greedy graph verifies: the greedy speculative tokens
    assert _gen(prompt, draft_model=_draft_model(3)) == _gen(prompt)


def test_eos_inside_an_accepted_run_and_a_run_to_the_end_of_the_cache():
    prompt = _prompt()
    known = _gen(prompt, sample=dict(top_k=1))
    fn = _oracle(prompt, known)
    cut = next(j for j in range(2, NEW - 1) if j % R != 0 and known.index(known[j]) == j)       # first occurs inside an accepted run
    got = _gen(prompt, eos=known[cut], sample=dict(top_k=1), draft=fn)
    assert got == known[:cut + 1] and _engine().spec_stats['emitted'] == cut and int(_engine().pos[0]) == PROMPT + cut
    assert _gen(prompt, eos=known[0], sample=dict(top_k=1), draft=fn) == known[:1] and _engine().spec_stats['steps'] == 0
    # prompt + new tokens = t_max exactly: the last tokens come from the single-step sampling graph
    long = torch.randint(1, VOCAB, (T_END,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(78))
    new = T_MAX - T_END
    torch.manual_seed(8)
    got = _gen(long, new=new, sample=SETTING)
    st = _engine().spec_stats
    assert len(got) == new and 1 + st['emitted'] < new and T_END + st['emitted'] + R > T_MAX and int(_engine().pos[0]) == T_MAX - 1
    torch.manual_seed(8)
    assert _gen(long, new=new, sample=SETTING) == got
    assert _gen(long, new=new, sample=dict(top_k=1)) == _gen(long, new=new)


def test_speculate_value_errors():
    prompt = _prompt()
    other = D.build_random_llama(DEV, seed=1, **dict(HD128, num_hidden_layers=1, vocab_size=256))
    for bad in (dict(sample=dict(foo=1)), dict(sample=dict(temperature=-1)), dict(sample=3), dict(samples=dict(top_k=1)),
                dict(draft=lambda t, k: [0] * k, draft_model=_draft_model(3)), dict(draft_model=other), dict(draft_model=object())):
        with pytest.raises(ValueError):
            _gen(prompt, **bad)
    with pytest.raises(ValueError):                              # the existing rule stays
        D.engine_generate(_model(), prompt[None], 4, engine=_engine(), prefill='engine', sample=dict(top_k=1), speculate=dict(k=K))
