"""GPU tests of BATCHED speculative decoding in the engine (quant/decode.py): DecodeEngine(batch=B, batch_chunk=R).verify_batch / accept_batch /
capture_verify_greedy_batch and engine_generate_batch(speculate=...), on the model, the bars (HOOK_TOL / KV_ATOL) and the references of
tests/test_gpu_speculate.py, whose helpers are imported: the eager module chain (engine hook disabled, DynamicCache, teacher-forced) per sequence
for the logits and the cache, and -- for generated sequences -- the plain batch engine teacher-forced over the very sequences under test.
B = 3 sequences of R = 5 rows (M = 15), prompts of 23 / 7 / 64 tokens."""
import functools
import math

import numpy as np
import pytest
import torch

import test_gpu_speculate as S
from quant import decode as D
from test_gpu_speculate import DEV, HOOK_TOL, KV_ATOL, T_MAX, VOCAB
from util import rel_err

pytestmark = pytest.mark.gpu
B, R = 3, 5
K = R - 1
LENS = (23, 7, 64)
NEW = 24
KV_SEEDS = (500, 501, 522)     # token seeds of test_accept_different_counts_then_continue, see there
SEEDS = (77, 1077, 2077)       # prompt seeds of the generate tests, see test_generate_batch_speculative
END_LENS = (132, 100, 7)       # the run that ends exactly at t_max: the longest sequence's chunk stops fitting while the others still verify
END_SEEDS = (78, 1078, 2078)


@functools.lru_cache(maxsize=None)
def _engine():
    return D.DecodeEngine(S._model(), t_max=T_MAX, batch=B, batch_chunk=R)


@functools.lru_cache(maxsize=None)
def _plain_engine():
    return D.DecodeEngine(S._model(), t_max=T_MAX, batch=B)


def _check_rows(what, got, expect):
    for i in range(got.shape[0]):
        err = rel_err(got[i], expect[i])
        print('%s, row %d: %.3e' % (what, i, err))
        assert err < HOOK_TOL, (what, i, err)


# ---- verify_batch / accept_batch -------------------------------------------------------------------------------------------------
def _verify_case(eng, lens, seed0):
    """prompts of `lens` tokens in the engine, R further tokens each: (ids per sequence, chain logits per sequence -- row 1 + i after ids[: T + i + 1])"""
    model = S._model()
    ids = [S._ids(T + R, seed0 + b) for b, T in enumerate(lens)]
    expect = [S._chain(model, x, T)[0] for x, T in zip(ids, lens)]
    eng.prefill_batch([x[0, :T] for x, T in zip(ids, lens)], starts=[0] * len(lens))
    return ids, expect


def test_verify_batch_matches_the_module_chain():
    eng = _engine()
    ids, expect = _verify_case(eng, LENS, 300)
    got = eng.verify_batch([x[0, T:T + R] for x, T in zip(ids, LENS)])
    assert got.shape == (B, R, VOCAB) and eng.pos.tolist() == list(LENS)
    got = got.float().cpu().numpy()
    for b in range(B):
        _check_rows('verify_batch sequence %d' % b, got[b], expect[b][1:])
    # entries shorter than R (lists as well as tensors): the leading rows, padded with the last id behind them
    n = (2, R, 1)
    short = eng.verify_batch([x[0, T:T + m].tolist() for x, T, m in zip(ids, LENS, n)]).float().cpu().numpy()
    assert eng.pos.tolist() == list(LENS) and eng.chunk_ids[0].tolist() == ids[0][0, LENS[0]:LENS[0] + 2].tolist() + [int(ids[0][0, LENS[0] + 1])] * 3
    for b in range(B):
        _check_rows('short entry of sequence %d' % b, short[b, :n[b]], expect[b][1:])


def test_an_idle_entry_leaves_its_slot_and_its_position_alone():
    eng = _engine()
    ids, expect = _verify_case(eng, LENS, 320)
    nan = torch.tensor(float('nan'), dtype=torch.float16, device=DEV)
    eng.kcb[:, 1, LENS[1]:] = nan                               # rows behind the prompt of the idle sequence: a stray write would show
    eng.vcb[:, 1, LENS[1]:] = nan
    k0, v0 = eng.kcb[:, 1].clone(), eng.vcb[:, 1].clone()
    got = eng.verify_batch([ids[0][0, LENS[0]:LENS[0] + R], None, ids[2][0, LENS[2]:LENS[2] + R]]).float().cpu().numpy()
    assert eng.pos.tolist() == list(LENS)
    assert torch.equal(eng.kcb[:, 1].view(torch.int16), k0.view(torch.int16)) and torch.equal(eng.vcb[:, 1].view(torch.int16), v0.view(torch.int16))
    for b in (0, 2):
        _check_rows('next to an idle sequence, sequence %d' % b, got[b], expect[b][1:])
    eng.accept_batch([R, 0, 3])
    assert eng.pos.tolist() == [LENS[0] + R, LENS[1], LENS[2] + 3]
    eng.kcb[:, 1, LENS[1]:] = 0
    eng.vcb[:, 1, LENS[1]:] = 0


def test_accept_different_counts_then_continue():
    """verify five tokens per sequence, accept 2 / 5 / 1 of them, verify again, accept all, decode one step: logits and the cache rows below pos
    are the chain's -- the rejected rows leave no trace.
    KV_ATOL is an absolute bar of one fp16 ulp of values in [4, 8) (0.0039), and this model's second-layer cache holds values up to 8.5: a
    row whose hidden state went through another row count's kernels than the chain's can miss it through rounding alone.  KV_SEEDS are
    therefore sequences on which the single-sequence engine (DecodeEngine(chunk=R), whose contract every sequence of the batch gets) meets the
    bar itself.  Observed on the MI355X, largest difference of the batched engine / of the single-sequence engine fed the same tokens:
    seeds (500, 501, 522): 0.0039 / 0.0039 for every sequence (the choice); seed 502 for the third sequence: 0.0044 / 0.0073; 521 for the
    second: 0.0020 / 0.0049; 540 for the first: 0.0039 / 0.0059; 562 for the third: 0.0098 / 0.0078 (one row of layer 1, in both engines)."""
    model, eng = S._model(), _engine()
    ns = (2, R, 1)
    kept = [S._ids(T + n + R + 1, s) for s, T, n in zip(KV_SEEDS, LENS, ns)]              # prompt, accepted, five for a verify, one for a decode
    rejected = [S._ids(R - n, s + 10)[0] for s, n in zip(KV_SEEDS, ns)]
    every = [S._chain(model, x, T)[0] for x, T in zip(kept, LENS)]                        # every[b][i]: the logits after kept[b][: T + i]
    kv = [S._chain(model, x[:, :T + n + R], T + n + R)[1] for x, T, n in zip(kept, LENS, ns)]
    eng.prefill_batch([x[0, :T] for x, T in zip(kept, LENS)], starts=[0] * B)
    eng.verify_batch([torch.cat([x[0, T:T + n], r]) for x, T, n, r in zip(kept, LENS, ns, rejected)])
    eng.accept_batch(list(ns))
    assert eng.pos.tolist() == [T + n for T, n in zip(LENS, ns)]
    got = eng.verify_batch([x[0, T + n:T + n + R] for x, T, n in zip(kept, LENS, ns)]).float().cpu().numpy()
    for b in range(B):
        _check_rows('second verify of sequence %d' % b, got[b], every[b][ns[b] + 1:])
    eng.accept_batch([R] * B)
    end = [T + n + R for T, n in zip(LENS, ns)]
    assert eng.pos.tolist() == end
    for b in range(B):
        for li, (k, v) in enumerate(kv[b]):
            assert np.abs(eng.kcb[li, b, :end[b]].float().cpu().numpy() - k).max() < KV_ATOL
            assert np.abs(eng.vcb[li, b, :end[b]].float().cpu().numpy() - v).max() < KV_ATOL
    last = eng.decode(torch.stack([x[0, e] for x, e in zip(kept, end)])).float().cpu().numpy()
    for b in range(B):
        err = rel_err(last[b], every[b][ns[b] + R + 1])
        print('decode after the accepts, sequence %d: %.3e' % (b, err))
        assert err < HOOK_TOL, (b, err)
    assert eng.pos.tolist() == [e + 1 for e in end]


def test_verify_greedy_batch_graph_agrees_with_eager_verify_and_host_accept():
    """accepted counts 0 / 2 / K in ONE step; then the same step with sequence 1 idle: its position keeps the idle mark, its slot its bits"""
    eng = _engine()
    wants = (0, 2, K)
    prompts = [S._ids(T + 1, 900 + b)[0] for b, T in enumerate(LENS)]
    feed = lambda: eng.prefill_batch([p[:T] for p, T in zip(prompts, LENS)], starts=[0] * B)
    if eng.verify_batch_graph is None:
        eng.pos.zero_()
        eng.capture_verify_greedy_batch()
    feed()
    toks = [[int(p[T])] for p, T in zip(prompts, LENS)]
    for j in range(K):                                          # drafts that agree with the model for exactly wants[b] tokens
        am = eng.verify_batch(toks).argmax(dim=-1).tolist()
        for b in range(B):
            toks[b].append(am[b][j] if j < wants[b] else (am[b][j] + 1) % VOCAB if j == wants[b] else 7)
    am = eng.verify_batch(toks).argmax(dim=-1).tolist()
    acc = []
    for b in range(B):
        a = 0
        while a < K and am[b][a] == toks[b][a + 1]:
            a += 1
        acc.append(a)
    assert tuple(acc) == wants and eng.pos.tolist() == list(LENS)
    eng.accept_batch([a + 1 for a in acc])
    pos_eager = eng.pos.tolist()
    feed()                                                      # the same state again
    eng.chunk_ids.copy_(torch.tensor(toks, device=DEV))
    eng.verify_batch_graph.replay()
    res = eng.verify_out.tolist()
    assert [r[0] for r in res] == acc and [r[1:] for r in res] == am, (res, acc, am)
    assert eng.pos.tolist() == pos_eager == [T + a + 1 for T, a in zip(LENS, acc)]
    feed()
    eng.pos[1:2].fill_(-1)
    k0, v0 = eng.kcb[:, 1].clone(), eng.vcb[:, 1].clone()
    eng.chunk_ids.copy_(torch.tensor(toks, device=DEV))
    eng.verify_batch_graph.replay()
    res = eng.verify_out.tolist()
    assert eng.pos.tolist() == [pos_eager[0], -1, pos_eager[2]]
    assert [res[b][0] for b in (0, 2)] == [acc[0], acc[2]] and [res[b][1:] for b in (0, 2)] == [am[0], am[2]]
    assert torch.equal(eng.kcb[:, 1].view(torch.int16), k0.view(torch.int16)) and torch.equal(eng.vcb[:, 1].view(torch.int16), v0.view(torch.int16))
    eng.pos[1:2].fill_(LENS[1])


# ---- engine_generate_batch(speculate=...) -----------------------------------------------------------------------------------------
def _prompts(lens, seeds):
    return [S._ids(T, s)[0] for T, s in zip(lens, seeds)]


def _plain(prompts, new):
    return D.engine_generate_batch(S._model(), prompts, max_new_tokens=new, engine=_plain_engine())


def _teacher_forced(seqs, lens):
    """reference logits of plain code for the sequences themselves (all of one generated length): prefill_batch of the prompts + batch decode
    teacher-forced over the generated tokens; [b][i] is the distribution token lens[b] + i of sequence b was chosen from"""
    eng = _plain_engine()
    rows = [eng.prefill_batch([s[:T] for s, T in zip(seqs, lens)], starts=[0] * len(seqs)).float().cpu().numpy()]
    new = seqs[0].numel() - lens[0]
    for i in range(new - 1):
        rows.append(eng.decode(torch.stack([s[T + i] for s, T in zip(seqs, lens)])).float().cpu().numpy())
    return np.stack(rows, axis=1)


def _check_sequences(what, seqs, lens):
    """the rule of test_gpu_speculate._check_sequence for every sequence: every emitted token within the HOOK_TOL margin of the reference maximum,
    and at most one position off the exact reference argmax"""
    ref = _teacher_forced(seqs, lens)
    offs = []
    for b, (s, T) in enumerate(zip(seqs, lens)):
        gen = s[T:].tolist()
        assert len(gen) == ref.shape[1]
        off = 0
        for i, tok in enumerate(gen):
            r = ref[b, i]
            assert r[tok] >= r.max() - HOOK_TOL * np.abs(r).max(), (what, b, i, tok, float(r[tok]), float(r.max()))
            off += int(tok != int(r.argmax()))
        print('%s, sequence %d: %d of %d positions differ from the reference argmax' % (what, b, off, len(gen)))
        assert off <= 1, (what, b, off)
        offs.append(off)
    return offs


def _known(plain, prompts):
    """the plain run's sequence that starts with the prompt `toks` starts with (the drafts are called per sequence, without its index)"""
    full = [p.tolist() for p in plain]

    def find(toks):
        return next(f for f, p in zip(full, prompts) if toks[:p.numel()] == f[:p.numel()])
    return find


def _oracle_draft(plain, prompts):
    find = _known(plain, prompts)
    return lambda toks, k: (find(toks)[len(toks):len(toks) + k] + [0] * k)[:k]


def _adversarial_draft(plain, prompts):
    find = _known(plain, prompts)

    def draft(toks, k):
        known = find(toks)
        return [((known[len(toks) + j] if len(toks) + j < len(known) else 0) + 1) % VOCAB for j in range(k)]
    return draft


def test_plain_generate_batch_meets_the_cap_against_the_module_chain():
    """the observation SEEDS / END_SEEDS were picked on: plain engine_generate_batch differs from the eager chain's argmax (teacher-forced over
    its own output, per sequence) at no more than one position of any sequence (measured: none, for both triples)"""
    model = S._model()
    for lens, seeds, new in ((LENS, SEEDS, NEW), (END_LENS, END_SEEDS, T_MAX - max(END_LENS))):
        plain = _plain(_prompts(lens, seeds), new)
        for b, (p, T) in enumerate(zip(plain, lens)):
            chain, _ = S._chain(model, p[None, :-1], T)
            gen = p[T:].tolist()
            off = sum(int(tok != int(chain[i].argmax())) for i, tok in enumerate(gen))
            print('plain generate_batch, seed %d: %d of %d positions differ from the chain argmax' % (seeds[b], off, len(gen)))
            assert off <= 1


@pytest.mark.parametrize('draft', ['oracle', 'adversarial', 'lookup'])
def test_generate_batch_speculative(draft):
    """SEEDS = (77, 1077, 2077): with these prompts plain engine_generate_batch agrees with the module chain's argmax at all 24 positions of
    every sequence (so the cap of one differing position is met by the plain path,
    test_plain_generate_batch_meets_the_cap_against_the_module_chain), and the three speculative runs were observed to differ from their
    teacher-forced reference argmax at 0 positions of every sequence and to emit the plain run's tokens.  Observed accepted counts: oracle
    4, 4, 4, 4, 3 for every sequence (the fifth step has three tokens left to emit: the oracle's fourth draft is padding); adversarial 22 steps
    of 0; prompt lookup 18 steps.  Of six seed triples tried, (81, 1081, 2081) put one near tie into the first sequence."""
    model, eng = S._model(), _engine()
    prompts = _prompts(LENS, SEEDS)
    plain = _plain(prompts, NEW)
    fn = dict(oracle=_oracle_draft(plain, prompts), adversarial=_adversarial_draft(plain, prompts), lookup=None)[draft]
    got = D.engine_generate_batch(model, prompts, max_new_tokens=NEW, engine=eng, speculate=dict(k=K, draft=fn))
    assert len(got) == B
    for g, p in zip(got, prompts):
        assert g.shape == (p.numel() + NEW,) and g.dtype == p.dtype and torch.equal(g[:p.numel()], p)
    st = eng.spec_stats
    print('%s draft: %r' % (draft, st))
    _check_sequences(draft, got, LENS)
    assert len(st['accepted']) == B and all(len(acc) <= st['steps'] and all(0 <= a <= K for a in acc) for acc in st['accepted'])
    if draft == 'oracle':
        assert st['steps'] <= math.ceil(NEW / R) + 1
        for acc in st['accepted']:
            assert sum(1 for a in acc if a != K) <= 1, st                       # every step accepted 4, but for one near tie at most
    if draft == 'adversarial':
        assert all(a == 0 for acc in st['accepted'] for a in acc), st
        assert st['steps'] == NEW - 2 and st['emitted'] == [NEW - 2] * B       # the last token comes from the single-step graph
    assert eng.pos.tolist() == [T + NEW - 1 for T in LENS]


def test_generate_batch_speculative_eos_inside_an_accepted_run():
    """one sequence meets its eos inside an accepted run and idles; the others go on to their length and are what they were without an eos"""
    model, eng = S._model(), _engine()
    prompts = _prompts(LENS, SEEDS)
    fn = _oracle_draft(_plain(prompts, NEW), prompts)
    full = D.engine_generate_batch(model, prompts, max_new_tokens=NEW, engine=eng, speculate=dict(k=K, draft=fn))
    gens = [f[T:].tolist() for f, T in zip(full, LENS)]
    # a token of sequence 1 that first occurs INSIDE an accepted run (verify step n emits tokens 5 n - 4 .. 5 n: not the run's last one) and that
    # the other sequences never emit
    cut = next(j for j in range(2, NEW - 6) if j % R != 0 and gens[1].index(gens[1][j]) == j and gens[1][j] not in gens[0] + gens[2])
    eos = gens[1][cut]
    got = D.engine_generate_batch(model, prompts, max_new_tokens=NEW, eos_token_id=eos, engine=eng, speculate=dict(k=K, draft=fn))
    assert torch.equal(got[1], full[1][:LENS[1] + cut + 1])
    assert torch.equal(got[0], full[0]) and torch.equal(got[2], full[2])
    st = eng.spec_stats
    assert st['emitted'][1] == cut and len(st['accepted'][1]) < len(st['accepted'][0])
    assert eng.pos.tolist() == [LENS[0] + NEW - 1, LENS[1] + cut, LENS[2] + NEW - 1]
    # eos as the very first token of one sequence: it never verifies
    got = D.engine_generate_batch(model, prompts, max_new_tokens=NEW, eos_token_id=gens[1][0], engine=eng, speculate=dict(k=K, draft=fn))
    if gens[1][0] not in gens[0] + gens[2]:
        assert torch.equal(got[0], full[0]) and torch.equal(got[2], full[2])
    assert torch.equal(got[1], full[1][:LENS[1] + 1]) and eng.spec_stats['accepted'][1] == []


def test_generate_batch_speculative_up_to_the_end_of_the_cache():
    """max(T) + max_new_tokens = t_max exactly: the verify steps stop where the longest sequence's chunk no longer fits, the single-step graph
    finishes all sequences.  Observed with END_SEEDS = (78, 1078, 2078): five verify steps, every sequence accepts 4 in each (25 of its 28
    tokens), two single steps; 0 positions off the reference argmax."""
    model, eng = S._model(), _engine()
    new = T_MAX - max(END_LENS)
    prompts = _prompts(END_LENS, END_SEEDS)
    fn = _oracle_draft(_plain(prompts, new), prompts)
    got = D.engine_generate_batch(model, prompts, max_new_tokens=new, engine=eng, speculate=dict(k=K, draft=fn))
    assert [g.numel() for g in got] == [T + new for T in END_LENS] and got[0].numel() == T_MAX
    st = eng.spec_stats
    print('to the end of the cache: %r' % (st,))
    assert 1 + st['emitted'][0] < new                           # the verify steps stopped early ...
    assert END_LENS[0] + st['emitted'][0] + R > T_MAX           # ... exactly where the longest sequence's chunk stops fitting
    _check_sequences('end of cache', got, END_LENS)
    assert eng.pos.tolist() == [T + new - 1 for T in END_LENS]


def test_errors_leave_the_positions_alone():
    model, eng, plain = S._model(), _engine(), _plain_engine()
    prompts = _prompts(LENS, SEEDS)
    eng.prefill_batch(prompts, starts=[0] * B)
    plain.prefill_batch(prompts, starts=[0] * B)
    gen = lambda p=prompts, **kw: D.engine_generate_batch(model, p, max_new_tokens=4, **kw)
    for kw in (dict(engine=eng, speculate=dict(k=K), sample=dict(temperature=0.8)), dict(engine=eng, speculate=dict(k=K, sample=dict(temperature=0.8))),
               dict(engine=eng, speculate=dict(k=K, draft_model=model)),
               dict(engine=eng, speculate=dict(k=0)), dict(engine=eng, speculate=dict(k=16)), dict(engine=eng, speculate=dict(k=3)),
               dict(engine=eng, speculate=dict(k=K, tokens=3)), dict(engine=eng, speculate=4), dict(engine=eng, speculate=dict(k=K, max_ngram=0)),
               dict(engine=eng, speculate=dict(k=K, draft=5)), dict(engine=plain, speculate=dict(k=K)),
               dict(p=prompts[:2], engine=eng, speculate=dict(k=K)), dict(p=prompts[:1], speculate=dict(k=K))):
        with pytest.raises(ValueError):
            gen(**kw)
    single = S._engine()                                        # batch 1 with chunk = R: not a batch_chunk engine
    with pytest.raises(ValueError):
        D.engine_generate_batch(model, prompts[:1], max_new_tokens=4, engine=single, speculate=dict(k=K))
    for kw in (dict(batch=3, batch_chunk=1), dict(batch=3, batch_chunk=17), dict(batch=3, batch_chunk=-2), dict(batch=1, batch_chunk=R),
               dict(batch_chunk=R), dict(batch=16, batch_chunk=9), dict(batch=9, batch_chunk=15), dict(batch=3, chunk=R)):
        with pytest.raises(ValueError):
            D.DecodeEngine(model, t_max=32, **kw)
    with pytest.raises(ValueError):
        eng.verify_batch([[1], [2]])                            # two entries for three sequences
    with pytest.raises(ValueError):
        eng.verify_batch([[1], [], [3]])
    with pytest.raises(ValueError):
        eng.verify_batch([[1], [2] * (R + 1), None])
    with pytest.raises(ValueError):
        eng.verify_batch(torch.zeros(3, dtype=torch.int64))
    for ns in ([1, 1], [1, R + 1, 1], [1, -1, 1], 3):
        with pytest.raises(ValueError):
            eng.accept_batch(ns)
    for call in (lambda: plain.verify_batch([[1], [2], [3]]), lambda: plain.accept_batch([1, 1, 1]), plain.capture_verify_greedy_batch,
                 lambda: single.verify_batch([[1]]), lambda: eng.verify([1, 2]), lambda: eng.accept(1)):
        with pytest.raises(ValueError):
            call()
    assert eng.pos.tolist() == list(LENS) and plain.pos.tolist() == list(LENS)
    eng.pos[1:2].fill_(T_MAX - R + 1)                           # the chunk of sequence 1 no longer fits
    with pytest.raises(ValueError):
        eng.verify_batch([[1, 2], [3], [4]])
    with pytest.raises(ValueError):
        eng.accept_batch([1, R, 1])
    with pytest.raises(ValueError):
        eng.capture_verify_greedy_batch()                       # its warm-up step would not fit either
    assert eng.pos.tolist() == [LENS[0], T_MAX - R + 1, LENS[2]]
    assert eng.verify_batch([[1, 2], None, [4]]).shape == (B, R, VOCAB)        # ... but idle it may stay where it is
    eng.pos[1:2].fill_(T_MAX - R)
    assert eng.verify_batch([[1, 2], [3], [4]]).shape == (B, R, VOCAB)
    assert eng.pos.tolist() == [LENS[0], T_MAX - R, LENS[2]]


# ---- more than 16 rows: the LM head of lm_head_logits' library route, the 16-row tiles of the layers ------------------------------------------
def test_verify_batch_of_twenty_rows():
    """B = 4, R = 5: M = 20.  The 256-wide model of this file is the smallest shape in use here and every layer of it reports a route for 20 rows
    (gptq_layer_route_for: the 16-row tiles on the image for qkv, o_proj, the gate / up pair and down_proj) -- the constructor checks exactly
    that and raises NotImplementedError otherwise."""
    model = S._model()
    lens = (9, 40, 3, 64)
    eng = D.DecodeEngine(model, t_max=T_MAX, batch=4, batch_chunk=R)
    for L in eng.layers:
        for w in (L['qkv'], L['o'], L['gate'], L['down']):
            assert eng.lib.gptq_layer_route_for(w['_keep'].handle, 4 * R) in (1, 2)
    ids, expect = _verify_case(eng, lens, 700)
    got = eng.verify_batch([x[0, T:T + R] for x, T in zip(ids, lens)])
    assert got.shape == (4, R, VOCAB) and eng.pos.tolist() == list(lens)
    got = got.float().cpu().numpy()
    for b in range(4):
        _check_rows('20 rows, sequence %d' % b, got[b], expect[b][1:])
