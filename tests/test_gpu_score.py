"""GPU tests of DecodeEngine.score / score_batch and quant.decode.perplexity: the engine's prompt path followed by the LM head of every row with
the cross-entropy inside (gptq_lm_head_nll_f16), against the eager module chain (engine hook disabled): model(ids).logits in fp16 -> float64
cross-entropy.  Bar per token: |nll - chain| <= 2 HOOK_TOL max |logits of that row| -- HOOK_TOL is the project's accepted distance between engine
and chain logits (tests/test_gpu_prefill_batch.py), log-sum-exp is 1-Lipschitz in the max norm and the target logit adds the same error once more."""
import functools
import math

import pytest
import torch

from quant import decode as D

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HOOK_TOL = 2e-2      # logits through the engine vs the eager chain (the bar of tests/test_gpu_prefill_batch.py)
HD128 = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
             vocab_size=512, max_position_embeddings=512)
T_MAX = 128
T = 40


@functools.lru_cache(maxsize=None)
def _model():
    return D.build_random_llama(DEV, seed=3, **HD128)


@functools.lru_cache(maxsize=None)
def _engine(batch=1):
    return D.DecodeEngine(_model(), t_max=T_MAX, batch=batch)


@functools.lru_cache(maxsize=None)
def _ids(n=T, seed=71):
    return torch.randint(0, HD128['vocab_size'], (n,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


@functools.lru_cache(maxsize=None)
def _chain(n=T, seed=71):
    """(nll64 [n - 1], bar [n - 1]) of the eager module chain on _ids(n, seed): computed once, shared, never modified"""
    model, ids = _model(), _ids(n, seed)
    model._gptq_engine_disabled = True
    try:
        with torch.no_grad():
            logits = model(ids[None]).logits[0]
    finally:
        model._gptq_engine_disabled = False
    assert logits.dtype == torch.float16
    z = logits[:-1].double()
    nll = torch.logsumexp(z, dim=1) - z.gather(1, ids[1:, None])[:, 0]
    return nll, 2 * HOOK_TOL * z.abs().max(dim=1).values


def _within(got, want, bar, name):
    err = (got.double() - want.double()).abs()
    print('%s: worst %.3e of the bar (bar %.3e .. %.3e)' % (name, float((err / bar).max()), float(bar.min()), float(bar.max())))
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert bool((err <= bar).all()), name


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int64)


def test_score_matches_the_module_chain():
    want, bar = _chain()
    got = _engine().score(_ids())
    assert got.shape == (T - 1,) and got.device.type == 'cuda'
    _within(got, want, bar, 'score T = %d' % T)
    assert bool((got > 0).all())
    one = _engine().score(_ids()[:1])
    assert one.shape == (0,) and one.dtype == torch.float32                     # T == 1: nothing to score (the token still enters the cache)
    assert int(_engine().pos[0]) == 1


def test_score_leaves_the_state_of_prefill():
    ids = _ids()
    a, b = D.DecodeEngine(_model(), t_max=T_MAX), D.DecodeEngine(_model(), t_max=T_MAX)
    a.score(ids)
    kept = b.prefill(ids).clone()
    assert int(a.pos[0]) == int(b.pos[0]) == T
    assert torch.equal(_bits(a.kcb[:, 0, :T]), _bits(b.kcb[:, 0, :T])) and torch.equal(_bits(a.vcb[:, 0, :T]), _bits(b.vcb[:, 0, :T]))
    assert torch.equal(_bits(a.logits[0]), _bits(kept))
    nxt = int(torch.argmax(kept))
    assert torch.equal(_bits(a.decode(nxt)), _bits(b.decode(nxt)))               # score a prompt, go on generating
    assert int(a.pos[0]) == T + 1


def test_score_in_passes_and_continued():
    want, bar = _chain()
    eng, ids = _engine(), _ids()
    one = eng.score(ids).clone()
    passes = eng.score(ids, max_rows=16)                                        # 16 + 16 + 8 rows
    assert passes.shape == (T - 1,) and int(eng.pos[0]) == T
    _within(passes, one, bar, 'max_rows = 16 against one pass')
    seams = [15, 16, 31, 32]                                                    # last row of a pass: its target is the next pass's first token
    _within(passes[seams], want[seams], bar[seams], 'seams against the chain')
    head = eng.score(ids[:20])
    assert head.shape == (19,) and int(eng.pos[0]) == 20
    tail = eng.score(ids[20:], start=None)                                      # continues at pos[0] = 20
    assert tail.shape == (19,) and int(eng.pos[0]) == T
    _within(head, one[:19], bar[:19], 'first 20 tokens')
    _within(tail, one[20:], bar[20:], 'continued at position 20')


def test_score_batch():
    lens, rows = (1, 17, 40), (2, 0, 1)
    prompts = [_ids(n, 80 + n) for n in lens]
    eng = D.DecodeEngine(_model(), t_max=T_MAX, batch=3)
    got = eng.score_batch(prompts, rows=rows)
    assert len(got) == 3 and got[0].shape == (0,) and got[0].dtype == torch.float32
    assert eng.pos.tolist() == [17, 40, 1]
    single = _engine()
    for n, g in zip(lens[1:], got[1:]):
        assert g.shape == (n - 1,)
        _within(g, single.score(_ids(n, 80 + n)), _chain(n, 80 + n)[1], 'score_batch, prompt of %d' % n)
        _within(g, _chain(n, 80 + n)[0], _chain(n, 80 + n)[1], 'score_batch against the chain, prompt of %d' % n)
    passes = eng.score_batch(prompts, rows=rows, max_rows=16)                   # the 40-token prompt straddles two pass boundaries
    for n, g, p in zip(lens[1:], got[1:], passes[1:]):
        _within(p, g, _chain(n, 80 + n)[1], 'score_batch in passes, prompt of %d' % n)
    eng.score_batch(prompts, rows=rows)
    ref = D.DecodeEngine(_model(), t_max=T_MAX, batch=3)
    ref.prefill_batch(prompts, rows=list(rows))
    assert ref.pos.tolist() == eng.pos.tolist()
    for n, r in zip(lens, rows):
        assert torch.equal(_bits(eng.kcb[:, r, :n]), _bits(ref.kcb[:, r, :n])) and torch.equal(_bits(eng.vcb[:, r, :n]), _bits(ref.vcb[:, r, :n]))
    assert torch.equal(_bits(eng.logits), _bits(ref.logits))
    step = torch.tensor([5, 6, 7], device=DEV)
    assert torch.equal(_bits(eng.decode(step)), _bits(ref.decode(step)))


def test_perplexity():
    seqlen, ns = 32, 3
    ids = _ids(seqlen * ns + 5, 91)                                             # the 5 ids behind the last full segment are dropped
    eng = _engine(3)
    res = D.perplexity(_model(), ids, seqlen=seqlen, engine=eng, batch=1)
    per = [eng.score(ids[i * seqlen:(i + 1) * seqlen], start=0).double() for i in range(ns)]
    assert res['tokens'] == ns * (seqlen - 1)
    allv = torch.cat(per)
    assert math.isclose(res['nll_sum'], float(allv.sum()), rel_tol=1e-6)
    assert math.isclose(res['ppl'], math.exp(float(allv.mean())), rel_tol=1e-6)
    # the reference's formula (llama.py:254-258): the mean loss of a segment times seqlen, summed, over nsamples * seqlen
    nlls = torch.stack([v.mean().float() * seqlen for v in per])
    assert math.isclose(res['ppl_reference'], float(torch.exp(nlls.sum() / (ns * seqlen))), rel_tol=1e-6)
    assert math.isclose(res['ppl_reference'], res['ppl'], rel_tol=1e-5)         # equal segments: the two means coincide
    res3 = D.perplexity(_model(), ids, seqlen=seqlen, engine=eng, batch=3)
    bars = torch.cat([_chain_of(ids[i * seqlen:(i + 1) * seqlen])[1] for i in range(ns)])
    want = torch.cat([_chain_of(ids[i * seqlen:(i + 1) * seqlen])[0] for i in range(ns)])
    assert res3['tokens'] == res['tokens']
    print('perplexity: batch 1 %.6f, batch 3 %.6f, chain %.6f' % (res['ppl'], res3['ppl'], math.exp(float(want.mean()))))
    assert abs(res3['nll_sum'] - res['nll_sum']) / res['tokens'] <= float(bars.mean())
    assert abs(res['nll_sum'] / res['tokens'] - float(want.mean())) <= float(bars.mean())
    with pytest.raises(ValueError):
        D.perplexity(_model(), ids[:seqlen - 1], seqlen=seqlen, engine=eng)


def _chain_of(ids):
    model = _model()
    model._gptq_engine_disabled = True
    try:
        with torch.no_grad():
            z = model(ids[None]).logits[0, :-1].double()
    finally:
        model._gptq_engine_disabled = False
    return torch.logsumexp(z, dim=1) - z.gather(1, ids[1:, None])[:, 0], 2 * HOOK_TOL * z.abs().max(dim=1).values


def test_score_with_a_head_the_kernel_declines():
    """lm_head.weight as a non-contiguous view (column stride 2): the torch route, the same bar"""
    want, bar = _chain()
    eng = D.DecodeEngine(_model(), t_max=T_MAX)
    W = eng.lm_head
    wide = torch.zeros((W.shape[0], 2 * W.shape[1]), dtype=W.dtype, device=DEV)
    view = wide[:, ::2]
    view.copy_(W)
    assert view.stride(1) == 2 and torch.equal(view, W)
    eng.lm_head = view
    got = eng.score(_ids())
    _within(got, want, bar, 'torch route')
    _within(eng.score(_ids(), max_rows=16), want, bar, 'torch route in passes')
    assert int(eng.pos[0]) == T
    assert eng.__dict__.get('_nll_ws') is None                                  # the kernel's workspace was never needed


def test_score_errors_leave_the_engine_untouched():
    eng = D.DecodeEngine(_model(), t_max=T_MAX, batch=2)
    eng.score(_ids(9, 5), row=1)
    snap = (eng.kcb.clone(), eng.vcb.clone(), eng.pos.clone(), eng.logits.clone())
    vocab = HD128['vocab_size']
    over = _ids(9, 6).clone()
    over[4] = vocab
    under = _ids(9, 6).clone()
    under[0] = -1
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    bad = [lambda: eng.score(over),                                             # an id equal to the vocabulary size
           lambda: eng.score(under),
           lambda: eng.score(_ids(100, 7), start=60),                           # positions 60 .. 159 of a cache of 128
           lambda: eng.score(_ids(T_MAX, 7), row=1, start=None),                # continues at pos[1] = 9
           lambda: eng.score(_ids(5, 7), start=-1),
           lambda: eng.score(empty),
           lambda: eng.score(_ids(5, 7), row=2),
           lambda: eng.score(_ids(5, 7), max_rows=0),
           lambda: eng.score(_ids(6, 7).reshape(2, 3)),
           lambda: eng.score_batch([_ids(5, 7), over]),
           lambda: eng.score_batch([_ids(5, 7), empty]),
           lambda: eng.score_batch([_ids(5, 7)] * 3),
           lambda: eng.score_batch([_ids(5, 7), _ids(4, 8)], rows=[1, 1]),
           lambda: eng.score_batch([_ids(5, 7), _ids(T_MAX + 1, 8)])]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert torch.equal(eng.pos, snap[2]), i
    assert torch.equal(_bits(eng.kcb), _bits(snap[0])) and torch.equal(_bits(eng.vcb), _bits(snap[1])) and torch.equal(_bits(eng.logits), _bits(snap[3]))
    assert eng.score(_ids(T_MAX, 7), row=0).shape == (T_MAX - 1,)               # the longest sequence that fits
