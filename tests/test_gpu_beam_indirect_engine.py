"""GPU tests of the indirect beam cache in the engine (DecodeEngine(beam_search=True, beam_cache='indirect'), engine_generate_beam(beam_cache=
'indirect')) with the tiny model, seeds, settings and helpers of tests/test_gpu_beam_engine.py: eager steps against the oracle's single step with
the table and cache invariants, the captured graph against the eager run bit for bit, the driver against a plain batch-1 engine, the ValueErrors."""
import functools

import numpy as np
import pytest
import torch

import beam_ref as R
import test_gpu_beam_engine as E
import test_gpu_generate_process as P
from quant import decode as D

pytestmark = pytest.mark.gpu
NEW, T_MAX = E.NEW, E.T_MAX


@functools.lru_cache(maxsize=None)
def _engine(n):
    eng = D.DecodeEngine(P._model(), t_max=T_MAX, batch=n, beam_search=True, beam_cache='indirect')
    eng.graph_for('beam')
    return eng


@pytest.mark.parametrize('n', [2, 4])
def test_eager_steps_follow_the_oracle_and_the_graph_follows_them(n):
    eng = _engine(n)
    first = E._begin(eng, 'engine', eos_token_id=None, length_penalty=1.0)
    T, steps, skipped = E._prompt().numel(), 0, 0
    with torch.no_grad():
        while True:
            before, k0, v0, pos = E._words(eng), eng.kcb.clone(), eng.vcb.clone(), T + steps
            if steps == 0:
                logits, src0 = first.reshape(1, -1).expand(n, -1).contiguous(), np.zeros((n, T_MAX), dtype=np.uint8)
                eng.beam_begin(first)
            else:
                src0 = eng.beam_src.cpu().numpy()
                eng._step_batch(beam=True)
                logits = eng.logits.clone()
                src0[:, pos - 1] = np.arange(n)
                assert np.array_equal(eng.beam_src.cpu().numpy(), src0), 'the step wrote more than src[b, p] = b'
                eng._beam_advance(eng.logits)
            got, st, src = R.unpack(E._words(eng)), R.from_words(before), eng.beam_src.cpu().numpy()
            assert eng.pos.tolist() == [pos] * n and got['status'] == 0 and eng.ids.tolist() == got['token'].tolist()
            # the table is the numpy gather of the previous one by the engine's parents; common counts its leading uniform columns
            assert np.array_equal(src[:, :pos], src0[got['parent']][:, :pos]) and np.array_equal(src[:, pos:], src0[:, pos:]), steps
            same = (src[:, :pos] == src[0, :pos]).all(axis=0)
            assert int(eng.beam_common) == (pos if same.all() else int(np.argmin(same))) >= T
            for now, was in ((eng.kcb, k0), (eng.vcb, v0)):                  # rows never move: only the step's own column changed
                changed = (now != was).any(dim=-1).any(dim=0)                # [rows, t]
                assert not changed[:, :pos - 1].any() and not changed[:, pos:].any() and (steps == 0 or changed[:, pos - 1].all()), steps
            l64 = logits.cpu().numpy().astype(np.float64)
            c, order = R.candidates(l64, st.score)
            if R.min_gap(l64, st.score, n) >= 10 * (R.ABS_BAR + R.REL_BAR * float(np.abs(c[order[:2 * n + 1]]).max())):
                msg = R.same_step(got, R.step(st, l64))
                assert msg is None, (steps, msg)
            else:
                skipped += 1                                                 # a near tie: the existing skip rule
            steps += 1
            if got['done']:
                break
    print('eager run: N', n, 'steps', steps, 'skipped for a near tie', skipped)
    assert steps == NEW and skipped * 10 <= steps
    words, k, v = E._words(eng), eng.kcb.clone(), eng.vcb.clone()
    for again in range(2):                                                   # the graph: bit-identical, twice
        got, replays = E._graph_run(eng, 'engine', eos_token_id=None, length_penalty=1.0)
        assert replays == steps - 1 and np.array_equal(got, words), again
        assert torch.equal(eng.kcb, k) and torch.equal(eng.vcb, v) and np.array_equal(eng.beam_src.cpu().numpy(), src), again


@pytest.mark.parametrize('prefill', ['engine', 'hf'])
@pytest.mark.parametrize('n', [2, 4])
def test_driver(n, prefill):
    prompt = E._prompt()
    T = prompt.numel()
    gen = functools.partial(D.engine_generate_beam, P._model(), prompt[None], NEW, num_beams=n, num_return_sequences=n, engine=_engine(n),
                            prefill=prefill, beam_cache='indirect')
    eos = int(gen()[0][0][T + NEW // 2])                                     # a token from the middle of the best hypothesis: an early EOS
    for kw in (dict(), dict(eos_token_id=eos, length_penalty=0.0)):
        seqs, scores = gen(**kw)
        assert len(seqs) == n and scores.tolist() == sorted(scores.tolist(), reverse=True)
        for seq, score in zip(seqs, scores.tolist()):
            toks = seq[T:].tolist()
            assert seq[:T].tolist() == prompt.tolist() and (len(toks) == NEW or toks[-1] == eos)
            assert abs(score - E._reference_score(toks, kw.get('length_penalty', 1.0))) <= E.ENGINE_TOL * len(toks)
        assert not kw or any(len(s) - T < NEW for s in seqs)


def test_errors():
    model, prompt = P._model(), E._prompt()
    for kw in (dict(beam_cache='copy'), dict(beam_cache=None), dict(beam_search=False, beam_cache='indirect')):
        with pytest.raises(ValueError):
            D.DecodeEngine(model, t_max=T_MAX, **dict(dict(batch=2, beam_search=True), **kw))
    for kw in (dict(engine=_engine(2)), dict(engine=E._engine(2), beam_cache='indirect'), dict(beam_cache='copy')):
        with pytest.raises(ValueError):
            D.engine_generate_beam(model, prompt[None], 5, num_beams=2, **kw)
    assert not hasattr(E._engine(2), 'beam_src')
