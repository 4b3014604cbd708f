"""GPU tests of beam search in the engine (DecodeEngine(batch=N, beam_search=True), engine_generate_beam) on the tiny head_dim-128 model of
tests/test_gpu_generate_process.py (vocab 512, t_max 64), N in {2, 4}, 20 new tokens:
(a) eager steps one at a time -- the oracle's single step (tests/beam_ref.py) on exactly the logits and the state the kernel saw, the cache
    against index_select by the engine's own parents, bit for bit;
(b) the captured graph against that eager run, bit for bit, and a second run on the same engine;
(c) the driver: both prefill routes, the scores against a plain batch-1 engine fed the hypotheses token by token, an EOS that finishes
    hypotheses early, early_stopping=True, the ValueErrors."""
import functools

import numpy as np
import pytest
import torch

import beam_ref as R
import test_gpu_generate_process as P
from quant import decode as D

pytestmark = pytest.mark.gpu
DEV = P.DEV
T_MAX, V = P.T_MAX, P.V
NEW = 20
ENGINE_TOL = 2.7e-3        # as tests/test_gpu_model.py: DecodeEngine's logits against the module chain


@functools.lru_cache(maxsize=None)
def _engine(n):
    eng = D.DecodeEngine(P._model(), t_max=T_MAX, batch=n, beam_search=True)
    eng.graph_for('beam')                      # before any prompt: the capture warms up with a real step
    return eng


def _prompt():
    return P._prompts(1)[0]


def _words(eng):
    torch.cuda.synchronize()
    return eng.beam_state.cpu().numpy().copy()


def _begin(eng, prefill, **settings):
    eng.set_beam_search(NEW, **settings)
    with torch.no_grad():
        eng.kcb.zero_()                        # (every run from the same cache: the runs are compared bit for bit, past their last position too)
        eng.vcb.zero_()
        first = D._prompt_into_engine(P._model(), _prompt()[None], eng, prefill).clone()
    return first


@functools.lru_cache(maxsize=None)
def _eager_run(n, eos, lp):
    """(a): the search step by step, every step checked; returns (final words, k cache, v cache, steps, skipped)"""
    eng = _engine(n)
    first = _begin(eng, 'engine', eos_token_id=eos, length_penalty=lp)
    T = _prompt().numel()
    steps = skipped = 0
    with torch.no_grad():
        while True:
            before = _words(eng)
            if steps == 0:
                logits = first.reshape(1, -1).expand(n, -1).contiguous()
                k0, v0 = eng.kcb.clone(), eng.vcb.clone()
                eng.beam_begin(first)
            else:
                eng._step()
                logits = eng.logits.clone()
                k0, v0 = eng.kcb.clone(), eng.vcb.clone()
                eng._beam_advance(eng.logits)
            after = _words(eng)
            got, st = R.unpack(after), R.from_words(before)
            pos = T + steps
            assert int(eng.pos[0]) == pos and eng.pos.tolist() == [pos] * n and got['status'] == 0
            assert eng.ids.tolist() == got['token'].tolist()
            # the cache: row b continues row parent[b] below pos, nothing at or past pos moved
            par = torch.from_numpy(got['parent']).to(DEV)
            for now, was in ((eng.kcb, k0), (eng.vcb, v0)):
                assert torch.equal(now[:, :, :pos], was.index_select(1, par)[:, :, :pos]), steps
                assert torch.equal(now[:, :, pos:], was[:, :, pos:]), steps
            l64 = logits.cpu().numpy().astype(np.float64)
            c, order = R.candidates(l64, st.score)
            bar = R.ABS_BAR + R.REL_BAR * float(np.abs(c[order[:2 * n + 1]]).max())
            if R.min_gap(l64, st.score, n) >= 10 * bar:
                want = R.step(st, l64)
                msg = R.same_step(got, want)
                assert msg is None, (steps, msg)
                assert np.array_equal(got['parent_at'][:got['t']], want.parent_at[:want.t])
                assert np.array_equal(got['token_at'][:got['t']], want.token_at[:want.t])
            else:
                skipped += 1
            steps += 1
            if got['done']:
                break
    print('eager run: N', n, 'eos', eos, 'length_penalty', lp, 'steps', steps, 'skipped for a near tie', skipped)
    assert skipped * 10 <= steps
    return after, eng.kcb.clone(), eng.vcb.clone(), steps, skipped


def _graph_run(eng, prefill, **settings):
    first = _begin(eng, prefill, **settings)
    with torch.no_grad():
        eng.beam_begin(first)
        replays = 0
        while not int(eng.beam_state[D.BEAM_W_DONE]):
            eng.beam_graph.replay()
            replays += 1
    return _words(eng), replays


@functools.lru_cache(maxsize=None)
def _early_eos(n):
    """an EOS that finishes hypotheses early: a token from the middle of the best hypothesis of the search without one.  The tests use it with
    length_penalty 0, under which a short hypothesis keeps its place in the pool (on this random model the length-normalised scores of the
    hypotheses that run to the limit pass it)"""
    words, _, _, _, _ = _eager_run(n, None, 1.0)
    st = R.from_words(words)
    return R.result(st)[0][0][NEW // 2]


@pytest.mark.parametrize('n', [2, 4])
def test_eager_steps_follow_the_oracle_and_the_graph_follows_them(n):
    eng = _engine(n)
    for eos, lp in ((None, 1.0), (_early_eos(n), 0.0)):
        words, k, v, steps, _ = _eager_run(n, eos, lp)
        pool = R.unpack(words)['pool']
        assert all(e['finished'] for e in pool)
        assert [e['score'] for e in pool] == sorted((e['score'] for e in pool), reverse=True)
        if eos is None:
            assert steps == NEW
        else:
            assert any(e['step'] + 1 < NEW and e['token'] == eos for e in pool)
        for again in range(2):                 # (b): bit-identical, and nothing stale survives a run
            got, replays = _graph_run(eng, 'engine', eos_token_id=eos, length_penalty=lp)
            assert replays == steps - 1
            assert np.array_equal(got, words), again
            assert torch.equal(eng.kcb, k) and torch.equal(eng.vcb, v), again


def _reference_score(tokens, length_penalty):
    """the length-normalised sum of the log-softmaxes a plain batch-1 engine gives along the hypothesis"""
    plain, prompt = P._plain(), _prompt()
    with torch.no_grad():
        logits = plain.prefill(prompt, start=0)
        total = 0.0
        for i, tok in enumerate(tokens):
            total += float(torch.log_softmax(logits.double().reshape(-1), dim=-1)[tok])
            if i + 1 < len(tokens):
                logits = plain.decode(tok)[0]
    return total / len(tokens) ** length_penalty


@pytest.mark.parametrize('prefill', ['engine', 'hf'])
@pytest.mark.parametrize('n', [2, 4])
def test_driver_returns_the_pool(n, prefill):
    eng, model, prompt = _engine(n), P._model(), _prompt()
    T = prompt.numel()
    for kw in (dict(), dict(length_penalty=0.5), dict(eos_token_id=_early_eos(n), length_penalty=0.0),
               dict(eos_token_id=_early_eos(n), length_penalty=0.0, early_stopping=True)):
        words, _ = _graph_run(eng, prefill, **kw)
        want = R.result(R.from_words(words))
        seqs, scores = D.engine_generate_beam(model, prompt[None], NEW, num_beams=n, num_return_sequences=n, engine=eng, prefill=prefill, **kw)
        assert len(seqs) == n and scores.dtype == torch.float32 and scores.shape == (n,)
        assert scores.tolist() == sorted(scores.tolist(), reverse=True)
        lp = kw.get('length_penalty', 1.0)
        early = 0
        for seq, score, (toks, wscore) in zip(seqs, scores.tolist(), want):
            assert seq[:T].tolist() == prompt.tolist() and seq[T:].tolist() == toks and score == np.float32(wscore)
            ref = _reference_score(toks, lp)
            print(prefill, n, kw, 'len', len(toks), 'score %.5f reference %.5f' % (score, ref))
            assert abs(score - ref) <= ENGINE_TOL * len(toks)
            early += len(toks) < NEW
            assert len(toks) == NEW or toks[-1] == kw['eos_token_id']
        if 'eos_token_id' in kw:
            assert early >= 1
    one, s1 = D.engine_generate_beam(model, prompt[None], NEW, num_beams=n, engine=eng, prefill=prefill)
    assert len(one) == 1 and s1.shape == (1,)


def test_flag_and_argument_errors():
    model, prompt = P._model(), _prompt()
    plain3 = P._plain3()
    for call in (lambda: plain3.set_beam_search(5), lambda: plain3.beam_select(plain3.logits), lambda: plain3.beam_begin(plain3.logits[0]),
                 lambda: plain3.capture_beam_step(), lambda: plain3.beam_result()):
        with pytest.raises(ValueError):
            call()
    assert not hasattr(plain3, 'beam_state')
    for kw in (dict(logits_process=True), dict(batch_chunk=2), dict(batch=1), dict(batch=1, chunk=2)):
        with pytest.raises(ValueError):
            D.DecodeEngine(model, t_max=T_MAX, **dict(dict(batch=2, beam_search=True), **kw))
    eng = _engine(2)
    gen = functools.partial(D.engine_generate_beam, model)
    for call in (lambda: gen(prompt, 5, num_beams=2, engine=eng),                                   # not [1, T]
                 lambda: gen(torch.stack([prompt, prompt]), 5, num_beams=2, engine=eng),
                 lambda: gen(prompt[None], 5, num_beams=1), lambda: gen(prompt[None], 5, num_beams=17),
                 lambda: gen(prompt[None], 5, num_beams=4, engine=eng),                             # an engine of another batch
                 lambda: gen(prompt[None], 5, num_beams=3, engine=plain3),                          # ... without the flag
                 lambda: gen(prompt[None], 5, num_beams=2, num_return_sequences=3, engine=eng),
                 lambda: gen(prompt[None], 5, num_beams=2, eos_token_id=[1, 2], engine=eng),
                 lambda: gen(prompt[None], T_MAX, num_beams=2, engine=eng),                         # beyond the cache
                 lambda: gen(prompt[None], 5, num_beams=2, engine=eng, early_stopping='sometimes'),
                 lambda: gen(prompt[None], 5, num_beams=2, engine=eng, prefill='other')):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        eng.beam_select(eng.logits[:1])
    with pytest.raises(ValueError):
        eng.beam_result(3)


def test_driver_refuses_a_vocabulary_below_2n_and_a_row_that_is_not_finite(monkeypatch):
    import types
    model, prompt = P._model(), _prompt()
    # vocab < 2 num_beams: checked on the head's rows before any engine is built
    stub = types.SimpleNamespace(lm_head=types.SimpleNamespace(weight=torch.zeros((7, 4))))
    with pytest.raises(ValueError, match='vocabulary'):
        D.engine_generate_beam(stub, prompt[None], 5, num_beams=4)
    # ... and by the engine's constructor, on a model whose head has 6 rows
    tiny = D.build_random_llama(DEV, seed=3, **dict(P.HD128, vocab_size=6))
    with pytest.raises(ValueError, match='vocabulary'):
        D.DecodeEngine(tiny, t_max=T_MAX, batch=4, beam_search=True)
    # a NaN / +inf in the prompt's logits: the search runs to its end, then the status word raises
    eng = _engine(2)
    real = D._prompt_into_engine
    for poison in (float('nan'), float('inf')):
        def poisoned(*args, **kw):
            logits = real(*args, **kw).clone()
            logits.reshape(-1)[5] = poison
            return logits
        monkeypatch.setattr(D, '_prompt_into_engine', poisoned)
        with pytest.raises(ValueError, match='not finite'):
            D.engine_generate_beam(model, prompt[None], 5, num_beams=2, engine=eng)
        assert int(eng.beam_state[D.BEAM_W_STATUS]) & 1
    monkeypatch.setattr(D, '_prompt_into_engine', real)
    seqs, _ = D.engine_generate_beam(model, prompt[None], 5, num_beams=2, engine=eng)       # the next run is clean: nothing stale
    assert len(seqs) == 1 and int(eng.beam_state[D.BEAM_W_STATUS]) == 0
