"""GPU tests of BATCHED speculative sampling in the engine (quant/decode.py): DecodeEngine(batch=B, batch_chunk=R, spec_sample=True)
.verify_sample_batch / capture_verify_sample_batch and engine_generate_batch(speculate=dict(sample=..., draft_model=...)), on the tiny
head_dim-128 model and the draft twin of tests/test_gpu_speculate_sample.py (the kernel itself: tests/test_gpu_spec_sample_batch.py).
B = 3 sequences of R = 5 rows, prompts of 23 / 7 / 64 tokens, t_max 160."""
import functools

import numpy as np
import pytest
import torch

import spec_sample_ref as X
import test_gpu_speculate_sample as SS
from quant import decode as D
from test_gpu_speculate_sample import DEV, T_MAX, VOCAB

pytestmark = pytest.mark.gpu
B, R = 3, 5
K = R - 1
LENS = (23, 7, 64)
SEEDS = (77, 1077, 2077)
END_LENS, END_SEEDS = (132, 100, 7), (78, 1078, 2078)
NEW = 24
SETTING = dict(temperature=0.8, top_p=0.95)                      # the reference script's default call
TEMPS = [1.3, 0.9, 1.6]


@functools.lru_cache(maxsize=None)
def _engine():
    return D.DecodeEngine(SS._model(), t_max=T_MAX, batch=B, batch_chunk=R, spec_sample=True)


@functools.lru_cache(maxsize=None)
def _greedy_only_engine():
    return D.DecodeEngine(SS._model(), t_max=T_MAX, batch=B, batch_chunk=R)


def _prompts(lens=LENS, seeds=SEEDS):
    return [torch.randint(1, VOCAB, (T,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(s)) for T, s in zip(lens, seeds)]


def _start(eng, prompts=None):
    """the prompts in the cache, pos = LENS; returns per sequence [the greedy first token, the R - 1 likeliest tokens behind the prompt]"""
    logits = eng.prefill_batch(_prompts() if prompts is None else prompts, starts=[0] * B)
    return [[int(l.argmax())] + torch.topk(l.float(), R - 1).indices.tolist() for l in logits]


def _u(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, R, generator=g).to(DEV), torch.rand(B, R, generator=g).to(DEV)


def _records(eng):
    rec = eng.spec_ws.view(B, R + 1).cpu().numpy()
    assert (rec[:, 0] == 0).all()                               # every ticket is back at 0
    return (rec[:, 1:] >> 32).astype(bool), (rec[:, 1:] & 0xFFFFFFFF).astype(np.int64)


def test_verify_sample_batch_follows_the_oracle_on_the_steps_own_logits():
    eng = _engine()
    eng.set_sampling(temperature=TEMPS, top_k=0, top_p=1.0)
    assert eng.chunk_temperature.view(B, R).tolist() == [[pytest.approx(t)] * R for t in TEMPS]
    g = torch.Generator().manual_seed(9)
    for seed, dls in ((1, None), (2, None), (3, [torch.randn(R - 1, VOCAB, generator=g).half().to(DEV) for _ in range(B)])):
        tokens = _start(eng)
        ua, ud = _u(seed)
        res = eng.verify_sample_batch(tokens, draft_logits=dls, u_accept=ua, u_draw=ud)
        flags, toks = _records(eng)
        P = eng.chunk_logits.view(B, R, VOCAB).cpu()
        assert torch.isfinite(P.float()).all()
        for b in range(B):
            a, out = res[b]
            assert int(eng.pos[b]) == LENS[b] + a + 1 and len(out) == a + 1 and out[:a] == tokens[b][1:a + 1]
            ok = X.admissible(flags[b], toks[b], P[b], tokens[b], None if dls is None else dls[b].cpu(), TEMPS[b], 0, 1.0, ua[b].cpu().numpy(),
                              ud[b].cpu().numpy())
            assert ok.all(), (seed, b, flags[b], toks[b])
            assert a == (int(np.argmin(flags[b, :R - 1])) if not flags[b, :R - 1].all() else R - 1) and out[a] == int(toks[b, a])
        print('seed %d: accepted %s' % (seed, [r[0] for r in res]))


def test_eager_and_graph_agree_for_equal_uniforms():
    eng = _engine()
    eng.set_sampling(temperature=[1.5, 0.8, 1.0], top_k=50, top_p=0.95)
    for with_q in (False, True):
        dls = [torch.randn(R - 1, VOCAB, generator=torch.Generator().manual_seed(4 + b)).half().to(DEV) for b in range(B)] if with_q else None
        tokens = _start(eng)
        torch.manual_seed(21)
        res = eng.verify_sample_batch(tokens, draft_logits=dls)
        _start(eng)
        torch.manual_seed(21)
        before = torch.cuda.get_rng_state(DEV)
        g = eng.capture_verify_sample_batch(draft_logits=with_q)
        assert torch.equal(torch.cuda.get_rng_state(DEV), before) and eng.pos.tolist() == list(LENS)
        assert eng.verify_sample_graphs[with_q] is g
        eng.chunk_ids.copy_(torch.tensor(tokens, device=DEV))
        if with_q:
            eng.chunk_draft_logits.copy_(torch.cat(dls))
        g.replay()
        out = eng.verify_out.tolist()
        assert [(r[0], r[1:r[0] + 2]) for r in out] == res and eng.pos.tolist() == [T + a + 1 for T, (a, _) in zip(LENS, res)]


def test_an_idle_entry_leaves_its_slot_its_position_and_its_row_alone():
    eng = _engine()
    eng.set_sampling(temperature=1.2)
    ua, ud = _u(5)
    tokens = _start(eng)
    everyone = eng.verify_sample_batch(tokens, u_accept=ua, u_draw=ud)
    _start(eng)
    nan = torch.tensor(float('nan'), dtype=torch.float16, device=DEV)
    eng.kcb[:, 1, LENS[1]:] = nan                               # rows behind the prompt of the idle sequence: a stray write would show
    eng.vcb[:, 1, LENS[1]:] = nan
    k0, v0 = eng.kcb[:, 1].clone(), eng.vcb[:, 1].clone()
    eng.verify_out[1].fill_(-7)
    eng.spec_ws.view(B, R + 1)[1, 1:].fill_(-9)
    res = eng.verify_sample_batch([tokens[0], None, tokens[2]], u_accept=ua, u_draw=ud)
    assert res[1] is None and res[0] == everyone[0] and res[2] == everyone[2]        # (a sequence does not depend on its neighbours)
    assert eng.pos.tolist() == [LENS[0] + res[0][0] + 1, LENS[1], LENS[2] + res[2][0] + 1]
    assert eng.verify_out[1].tolist() == [-7] * (R + 1) and eng.spec_ws.view(B, R + 1)[1].tolist() == [0] + [-9] * R
    assert torch.equal(eng.kcb[:, 1].view(torch.int16), k0.view(torch.int16)) and torch.equal(eng.vcb[:, 1].view(torch.int16), v0.view(torch.int16))
    eng.kcb[:, 1, LENS[1]:] = 0
    eng.vcb[:, 1, LENS[1]:] = 0


def test_short_entries_are_padded_and_bad_arguments_refused():
    eng = _engine()
    eng.set_sampling(temperature=1.0)
    tokens = _start(eng)
    ua, ud = torch.zeros(B, R, device=DEV), torch.full((B, R), 0.5, device=DEV)       # u_accept = 0 accepts every draft the target keeps
    n = (2, R, 3)
    short = [t[:m] for t, m in zip(tokens, n)]
    for dls in (None, [torch.randn(m - 1, VOCAB, generator=torch.Generator().manual_seed(b)).half().to(DEV) for b, m in enumerate(n)]):
        _start(eng)
        res = eng.verify_sample_batch(short, draft_logits=dls, u_accept=ua, u_draw=ud)
        assert [r[0] for r in res] == [m - 1 for m in n] and eng.pos.tolist() == [T + m for T, m in zip(LENS, n)]
        assert all(r[1][:m - 1] == t[1:m] and len(r[1]) == m for r, t, m in zip(res, tokens, n))
        assert eng.chunk_ids[0].tolist() == tokens[0][:2] + [tokens[0][1]] * (R - 2)
        if dls is not None:                                      # the padding rows' drafts are point masses at the padding token
            pad = eng.chunk_draft_logits.view(B, R - 1, VOCAB)[2, 2:].float()
            assert (pad[:, tokens[2][2]] == 0).all() and int(torch.isinf(pad).sum()) == 2 * (VOCAB - 1)
    _start(eng)
    dl = lambda m: torch.zeros(m, VOCAB, dtype=torch.float16, device=DEV)
    for bad in (dict(tokens=tokens[:2]), dict(tokens=[tokens[0], tokens[1][:1], tokens[2]]), dict(tokens=[tokens[0], tokens[1] + [3], None]),
                dict(tokens=torch.zeros(B, dtype=torch.int64)), dict(tokens=tokens, u_accept=ua[0]), dict(tokens=tokens, u_draw=ud.double()),
                dict(tokens=tokens, draft_logits=[dl(R - 1), dl(R - 2), dl(R - 1)]), dict(tokens=tokens, draft_logits=[dl(R - 1)] * 2),
                dict(tokens=tokens, draft_logits=[dl(R - 1).float()] * B), dict(tokens=tokens, draft_logits=dl(R - 1))):
        with pytest.raises(ValueError):
            eng.verify_sample_batch(**bad)
        assert eng.pos.tolist() == list(LENS)
    assert eng.verify_sample_batch([None, short[1], None], draft_logits=[None, dl(R - 1), 5])[1][0] >= 0      # idle entries' draft logits are ignored
    _start(eng)
    eng.pos[1:2].fill_(T_MAX - R + 1)                           # the chunk of sequence 1 no longer fits
    for call in (lambda: eng.verify_sample_batch(tokens), eng.capture_verify_sample_batch):
        with pytest.raises(ValueError):
            call()
    assert eng.pos.tolist() == [LENS[0], T_MAX - R + 1, LENS[2]]
    assert eng.verify_sample_batch([tokens[0], None, tokens[2]], u_accept=ua, u_draw=ud)[1] is None            # ... unless it idles
    # an engine built without spec_sample allocates nothing of this and refuses; so do the engines of the other kinds
    plain = _greedy_only_engine()
    assert not plain.spec_sample and not hasattr(plain, 'spec_ws') and not hasattr(plain, 'chunk_u_accept')
    plain.prefill_batch(_prompts(), starts=[0] * B)
    for call in (lambda: plain.verify_sample_batch(tokens), plain.capture_verify_sample_batch, lambda: SS._engine().verify_sample_batch([tokens[0]]),
                 lambda: eng.verify_sample(tokens[0]), lambda: D.DecodeEngine(SS._model(), t_max=32, batch=B, spec_sample=True),
                 lambda: D.DecodeEngine(SS._model(), t_max=32, spec_sample=True)):
        with pytest.raises(ValueError):
            call()
    assert plain.pos.tolist() == list(LENS)


# ---- engine_generate_batch(speculate=dict(sample=..., draft_model=...)) ----------------------------------------------------------------------
def _gen(prompts=None, new=NEW, eos=None, **speculate):
    prompts = _prompts() if prompts is None else prompts
    out = D.engine_generate_batch(SS._model(), prompts, max_new_tokens=new, eos_token_id=eos, engine=_engine(), speculate=dict(k=K, **speculate))
    assert len(out) == len(prompts)
    gens = []
    for o, p in zip(out, prompts):
        assert o.dtype == p.dtype and torch.equal(o[:p.numel()], p)
        g = o[p.numel():]
        assert int(g.min()) >= 0 and int(g.max()) < VOCAB
        gens.append(g.tolist())
    return gens


def _oracle(prompts, known):
    full = [p.tolist() + g for p, g in zip(prompts, known)]

    def draft(toks, k):
        f = next(f for f, p in zip(full, prompts) if toks[:p.numel()] == f[:p.numel()])
        return (f[len(toks):len(toks) + k] + [0] * k)[:k]
    return draft


def test_temperature_zero_and_top_k_one_give_the_greedy_speculative_tokens():
    greedy = _gen()
    stats = _engine().spec_stats
    assert all(len(g) == NEW for g in greedy) and len(stats['accepted']) == B and len(stats['emitted']) == B
    assert _gen(sample=dict(top_k=1)) == greedy and _engine().spec_stats == stats
    assert _gen(sample=dict(temperature=0)) == greedy and _engine().spec_stats == stats
    assert _engine().pos.tolist() == [T + NEW - 1 for T in LENS]


def test_seeded_runs_agree_and_an_oracle_draft_is_accepted_whole():
    torch.manual_seed(3)
    a = _gen(sample=dict(temperature=1.5))
    torch.manual_seed(3)
    b = _gen(sample=dict(temperature=1.5))
    torch.manual_seed(4)
    c = _gen(sample=dict(temperature=1.5))
    assert a == b and a != c and all(len(g) == NEW for g in a)
    st = _engine().spec_stats
    assert st['steps'] > 0 and all(0 < len(acc) <= st['steps'] and all(0 <= x <= K for x in acc) for acc in st['accepted'])
    assert all(len(acc) <= e <= NEW - 1 for acc, e in zip(st['accepted'], st['emitted']))
    # a draft that knows the (deterministic: top_k = 1) continuation: every step accepts every token the draft knew
    prompts = _prompts()
    known = _gen(sample=dict(top_k=1))
    assert _gen(sample=dict(top_k=1), draft=_oracle(prompts, known)) == known
    st = _engine().spec_stats
    # (the last step's draft holds only the (NEW - 1) % R tokens the oracle still knows, then padding)
    assert st['accepted'] == [[K] * ((NEW - 1) // R) + [(NEW - 1) % R]] * B and st['emitted'] == [NEW - 1] * B, st
    assert _engine().pos.tolist() == [T + NEW - 1 for T in LENS]


def test_settings_per_prompt_keep_the_greedy_sequence_greedy():
    """temperatures [0, 0.8, 1.5]: sequence 0 runs beside two sampled ones and emits its greedy tokens -- exactly: the same kernels at the same
    row counts see the same rows, whatever the neighbours do"""
    greedy = _gen()
    torch.manual_seed(12)
    mixed = _gen(sample=dict(temperature=[0, 0.8, 1.5], top_p=[1.0, 0.95, 1.0]))
    assert mixed[0] == greedy[0]
    assert mixed[1] != greedy[1] or mixed[2] != greedy[2]
    assert _engine().temperature.tolist() == [0, pytest.approx(0.8), 1.5]          # the settings stay


def test_eos_inside_an_accepted_run_with_sequences_finishing_at_different_steps():
    prompts = _prompts()
    known = _gen(sample=dict(top_k=1))
    fn = _oracle(prompts, known)
    cut_at = lambda g, eos: g[:g.index(eos) + 1] if eos in g else g
    steps_of = lambda g: -(-(len(g) - 1) // R)                  # every verify step of an oracle draft emits R tokens until the sequence ends
    # a token of some sequence s that first occurs INSIDE an accepted run (verify step n emits tokens R n - K .. R n: not the run's last one),
    # early enough that s stops at least a step before a sequence that does not meet it (or meets it later)
    s, cut = next((b, j) for j in range(2, NEW - 6) for b in range(B) if j % R != 0 and known[b].index(known[b][j]) == j and
                  max(steps_of(cut_at(g, known[b][j])) for g in known) > steps_of(known[b][:j + 1]))
    eos = known[s][cut]
    want = [cut_at(g, eos) for g in known]
    got = _gen(eos=eos, sample=dict(top_k=1), draft=fn)
    assert got == want and got[s] == known[s][:cut + 1]
    st = _engine().spec_stats
    print('eos %d of sequence %d at %d: %r' % (eos, s, cut, st))
    assert st['emitted'] == [len(g) - 1 for g in want] and [len(acc) for acc in st['accepted']] == [steps_of(g) for g in want]
    assert len(set(len(acc) for acc in st['accepted'])) > 1     # the sequences finished at different steps
    assert _engine().pos.tolist() == [T + len(g) - 1 for T, g in zip(LENS, want)]
    # eos as the very first token of one sequence: it never verifies
    got = _gen(eos=known[1][0], sample=dict(top_k=1), draft=fn)
    assert got == [cut_at(g, known[1][0]) for g in known] and got[1] == known[1][:1] and _engine().spec_stats['accepted'][1] == []


def test_a_run_to_the_end_of_the_cache_finishes_on_the_sampling_graph():
    """max(T) + max_new_tokens = t_max exactly: the verify steps stop where the longest sequence's chunk no longer fits, the
    capture_sample_native graph finishes all sequences"""
    prompts = _prompts(END_LENS, END_SEEDS)
    new = T_MAX - max(END_LENS)
    torch.manual_seed(8)
    got = _gen(prompts, new=new, sample=SETTING)
    st = _engine().spec_stats
    print('to the end of the cache: %r' % (st,))
    assert all(len(g) == new for g in got)
    assert 1 + st['emitted'][0] < new and END_LENS[0] + st['emitted'][0] + R > T_MAX
    assert _engine().pos.tolist() == [T + new - 1 for T in END_LENS]
    torch.manual_seed(8)
    assert _gen(prompts, new=new, sample=SETTING) == got
    assert _gen(prompts, new=new, sample=dict(top_k=1)) == _gen(prompts, new=new)


def test_draft_model():
    eng = _engine()
    for seed in (3, 11):                                         # the target's own seed, and another one
        torch.manual_seed(5)
        a = _gen(sample=SETTING, draft_model=SS._draft_model(seed))
        st = dict(eng.spec_stats)
        print('draft model, seed %d: %r' % (seed, st))
        assert all(len(g) == NEW for g in a) and st['steps'] > 0 and all(0 <= x <= K for acc in st['accepted'] for x in acc)
        if seed == 3:
            assert sum(sum(acc) for acc in st['accepted']) > 0
        torch.manual_seed(5)
        assert _gen(sample=SETTING, draft_model=SS._draft_model(seed)) == a
        assert eng._draft_engine[0] is SS._draft_model(seed) and eng._draft_engine[1].batch == B
    # without `sample` the draft model drafts greedily and the greedy graph verifies: the greedy batched tokens
    assert _gen(draft_model=SS._draft_model(3)) == _gen()
    # an eos: the finished sequence idles in the draft engine as well
    torch.manual_seed(5)
    full = _gen(sample=SETTING, draft_model=SS._draft_model(3))
    eos = full[1][5]
    torch.manual_seed(5)
    got = _gen(eos=eos, sample=SETTING, draft_model=SS._draft_model(3))
    assert got[1] == full[1][:full[1].index(eos) + 1] and all(len(g) <= NEW for g in got)


def test_value_errors_leave_the_positions_alone():
    model, eng, plain = SS._model(), _engine(), _greedy_only_engine()
    prompts = _prompts()
    eng.prefill_batch(prompts, starts=[0] * B)
    plain.prefill_batch(prompts, starts=[0] * B)
    other = D.build_random_llama(DEV, seed=1, **dict(SS.HD128, num_hidden_layers=1, vocab_size=256))
    gen = lambda engine=eng, **kw: D.engine_generate_batch(model, prompts, max_new_tokens=4, engine=engine, **kw)
    for kw in (dict(engine=plain, speculate=dict(k=K, sample=dict(top_k=1))), dict(engine=plain, speculate=dict(k=K, draft_model=SS._draft_model(3))),
               dict(speculate=dict(k=K, draft=lambda t, k: [0] * k, draft_model=SS._draft_model(3))), dict(speculate=dict(k=K, draft_model=other)),
               dict(speculate=dict(k=K, draft_model=object())), dict(speculate=dict(k=K, sample=dict(foo=1))), dict(speculate=dict(k=K, sample=3)),
               dict(speculate=dict(k=K, samples=dict(top_k=1))), dict(speculate=dict(k=K, sample=dict(temperature=-1))),
               dict(speculate=dict(k=K, sample=dict(temperature=[1.0, 1.0]))), dict(speculate=dict(k=3, sample=dict(top_k=1))),
               dict(speculate=dict(k=K, sample=dict(top_k=1)), sample=dict(top_k=1))):
        with pytest.raises(ValueError):
            gen(**kw)
        assert eng.pos.tolist() == list(LENS) and plain.pos.tolist() == list(LENS), kw
