"""GPU tests of speculative decoding in the engine (quant/decode.py): DecodeEngine(chunk=R).verify / accept / capture_verify_greedy and
engine_generate(speculate=...), on the model of tests/test_gpu_prefill_batch.py (HD128, 2 layers, vocab 512, t_max 160; bars HOOK_TOL / KV_ATOL),
R = 5.  References: the eager module chain (engine hook disabled, DynamicCache, teacher-forced) for the logits and the cache, and -- for generated
sequences -- the engine's own plain prefill + decode teacher-forced over the very sequence under test."""
import functools
import math

import numpy as np
import pytest
import torch

from quant import decode as D
from util import rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HOOK_TOL = 2e-2      # logits through the engine vs the eager chain (fp16 KV cache on both sides)
KV_ATOL = 4e-3       # rotated cache rows against the HF cache (one fp16 rounding of values up to ~4)
HD128 = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
             vocab_size=512, max_position_embeddings=512)
VOCAB = HD128['vocab_size']
T_MAX = 160          # not a multiple of the kernels' key tiles
R = 5
K = R - 1
NEW = 24
PROMPT_LEN = 23
SEED = 77            # prompt seed of the generate tests, see test_generate_speculative
SEED_END = 78        # ... of the run that ends exactly at t_max
END_LEN = 132        # its prompt: the chunk stops fitting (position 157) while two tokens are still to come


@functools.lru_cache(maxsize=None)
def _model():
    return D.build_random_llama(DEV, seed=3, **HD128)


def _ids(n, seed):
    return torch.randint(0, VOCAB, (1, n), device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _chain(model, ids, prefill):
    """the eager module chain, engine hook disabled, DynamicCache: logits after the prompt and after every further token, and the cache"""
    from transformers.cache_utils import DynamicCache
    cache = DynamicCache(config=model.config)
    outs = []
    model._gptq_engine_disabled = True
    try:
        with torch.no_grad():
            out = model(ids[:, :prefill], past_key_values=cache, use_cache=True)
            outs.append(out.logits[0, -1].float().cpu().numpy())
            kv = []
            for li in range(model.config.num_hidden_layers):
                k, v = D._cache_layer_kv(cache, li)
                kv.append((k[0].transpose(0, 1).reshape(prefill, -1).float().cpu().numpy(), v[0].transpose(0, 1).reshape(prefill, -1).float().cpu().numpy()))
            for i in range(prefill, ids.shape[1]):
                out = model(ids[:, i:i + 1], past_key_values=cache, use_cache=True)
                outs.append(out.logits[0, -1].float().cpu().numpy())
    finally:
        model._gptq_engine_disabled = False
    return np.stack(outs), kv


@functools.lru_cache(maxsize=None)
def _engine():
    return D.DecodeEngine(_model(), t_max=T_MAX, chunk=R)


@functools.lru_cache(maxsize=None)
def _plain_engine():
    return D.DecodeEngine(_model(), t_max=T_MAX).capture()


@pytest.mark.parametrize('T', [3, 64, 130])
def test_verify_matches_the_module_chain(T):
    model, eng = _model(), _engine()
    ids = _ids(T + R, 300 + T)
    expect, _ = _chain(model, ids, T)                       # expect[1 + i]: the logits after ids[: T + i + 1]
    eng.prefill(ids[0, :T], start=0)
    got = eng.verify(ids[0, T:T + R]).float().cpu().numpy()
    assert got.shape == (R, VOCAB) and int(eng.pos[0]) == T
    for i in range(R):
        err = rel_err(got[i], expect[1 + i])
        print('verify after %d tokens, row %d: %.3e' % (T, i, err))
        assert err < HOOK_TOL, (T, i, err)
    # fewer tokens than R: the leading rows only, the same values
    short = eng.verify(ids[0, T:T + 2].tolist()).float().cpu().numpy()
    assert short.shape == (2, VOCAB) and int(eng.pos[0]) == T
    assert np.array_equal(short, got[:2])


@pytest.mark.parametrize('T', [3, 64, 130])
def test_verify_has_the_bits_of_the_single_sequence_entry(T):
    """the engine's verify step (the batched chunk attention at one sequence) against the same step driven by hand through the single-sequence
    entry gptq_decode_attn_chunk_f16 on kc / vc with a workspace of its own: logits and the R new cache rows agree bit for bit"""
    eng = _engine()
    ids = _ids(T + R, 300 + T)
    bits = lambda t: t.clone().view(torch.int16)
    eng.prefill(ids[0, :T], start=0)
    eng.verify(ids[0, T:T + R])
    got = [bits(eng.chunk_logits), bits(eng.kc[:, T:T + R]), bits(eng.vc[:, T:T + R])]
    eng.prefill(ids[0, :T], start=0)
    heads, hd = eng.heads, eng.head_dim
    ws = torch.zeros(eng.lib.gptq_decode_attn_chunk_workspace_bytes(R, heads, hd, T_MAX), dtype=torch.uint8, device=DEV)

    def attn(li, L, qkvb, ab, tab, s):
        rc = eng.lib.gptq_decode_attn_chunk_f16(qkvb.data_ptr(), qkvb.stride(0), R, eng.pos.data_ptr(), eng.kc[li].data_ptr(), eng.vc[li].data_ptr(),
                                                ab.data_ptr(), ab.stride(0), ws.data_ptr(), ws.numel(), heads, hd, T_MAX, L['theta'], eng.scale,
                                                eng.native.ptr(tab), s)
        eng.native.check(rc, 'gptq_decode_attn_chunk_f16')
    with torch.no_grad(), torch.cuda.device(DEV):
        eng._step_rows(eng.chunk_bufs, ids[0, T:T + R].contiguous(), attn, eng.chunk_logits)
    torch.cuda.synchronize()
    assert int(eng.pos[0]) == T
    for new, old in zip(got, [bits(eng.chunk_logits), bits(eng.kc[:, T:T + R]), bits(eng.vc[:, T:T + R])]):
        assert torch.equal(new, old)


def test_accept_then_continue():
    """verify five tokens, accept two, go on: the three rejected rows leave no trace in the logits or in the cache rows below pos"""
    model, eng = _model(), _engine()
    T = 64
    kept = _ids(T + 2 + R + 1, 500)                         # the prompt, the two accepted tokens, five more for a verify, one for a decode
    rejected = _ids(3, 501)
    expect, kv = _chain(model, kept[:, :T + 2 + R + 1], T + 2 + R)      # cache of the first T + 7 tokens; expect[1] after the decode token
    every, _ = _chain(model, kept, T)                       # every[i]: the logits after kept[: T + i]
    eng.prefill(kept[0, :T], start=0)
    eng.verify(torch.cat([kept[0, T:T + 2], rejected[0]]))
    eng.accept(2)
    assert int(eng.pos[0]) == T + 2
    got = eng.verify(kept[0, T + 2:T + 2 + R]).float().cpu().numpy()
    for i in range(R):
        err = rel_err(got[i], every[3 + i])
        print('second verify row %d: %.3e' % (i, err))
        assert err < HOOK_TOL, (i, err)
    eng.accept(R)
    assert int(eng.pos[0]) == T + 2 + R
    for li, (k, v) in enumerate(kv):
        assert np.abs(eng.kc[li, :T + 2 + R].float().cpu().numpy() - k).max() < KV_ATOL
        assert np.abs(eng.vc[li, :T + 2 + R].float().cpu().numpy() - v).max() < KV_ATOL
    last = eng.decode(kept[0, T + 2 + R]).float().cpu().numpy()[0]
    err = rel_err(last, expect[1])
    print('decode after the accepts: %.3e' % err)
    assert err < HOOK_TOL, err
    assert int(eng.pos[0]) == T + 2 + R + 1


# ---- engine_generate(speculate=...) ------------------------------------------------------------------------------------------
def _plain(prompt, new):
    return D.engine_generate(_model(), prompt, max_new_tokens=new, engine=_plain_engine(), prefill='engine')


def _teacher_forced(seq, T):
    """reference logits of plain code for `seq` itself: prefill of the prompt + decode teacher-forced over the generated tokens; row i is the
    distribution token T + i was chosen from"""
    eng = _plain_engine()
    rows = [eng.prefill(seq[0, :T], start=0).float().cpu().numpy()]
    for i in range(T, seq.shape[1] - 1):
        rows.append(eng.decode(seq[0, i]).float().cpu().numpy()[0])
    return np.stack(rows)


def _check_sequence(what, seq, T):
    """every emitted token within the HOOK_TOL margin of the reference maximum (every position: there is no unexamined tail after a flip), and at
    most one position off the exact reference argmax"""
    ref = _teacher_forced(seq, T)
    gen = seq[0, T:].tolist()
    assert len(gen) == ref.shape[0]
    off = 0
    for i, tok in enumerate(gen):
        assert ref[i][tok] >= ref[i].max() - HOOK_TOL * np.abs(ref[i]).max(), (what, i, tok, float(ref[i][tok]), float(ref[i].max()))
        off += int(tok != int(ref[i].argmax()))
    print('%s: %d of %d positions differ from the reference argmax' % (what, off, len(gen)))
    assert off <= 1, (what, off)
    return off


def _oracle_draft(plain):
    known = plain[0].tolist()
    return lambda toks, k: (known[len(toks):len(toks) + k] + [0] * k)[:k]


def _adversarial_draft(plain):
    known = plain[0].tolist()
    return lambda toks, k: [((known[len(toks) + j] if len(toks) + j < len(known) else 0) + 1) % VOCAB for j in range(k)]


def test_plain_generate_meets_the_cap_against_the_module_chain():
    """the observation SEED was picked on: plain engine_generate differs from the eager chain's argmax (teacher-forced over its own output) at no
    more than one of the 24 positions (measured: none, see test_generate_speculative)"""
    model = _model()
    for seed, T, new in ((SEED, PROMPT_LEN, NEW), (SEED_END, END_LEN, T_MAX - END_LEN)):
        plain = _plain(_ids(T, seed), new)
        chain, _ = _chain(model, plain[:, :-1], T)
        gen = plain[0, T:].tolist()
        off = sum(int(tok != int(chain[i].argmax())) for i, tok in enumerate(gen))
        print('plain generate, seed %d: %d of %d positions differ from the chain argmax' % (seed, off, len(gen)))
        assert off <= 1


@pytest.mark.parametrize('draft', ['oracle', 'adversarial', 'lookup'])
def test_generate_speculative(draft):
    """SEED = 77: with this prompt plain engine_generate agrees with the module chain's argmax at all 24 positions (so the cap of one differing
    position is met by the plain path, test_plain_generate_meets_the_cap_against_the_module_chain), and the three speculative runs were observed
    to differ from their teacher-forced reference argmax at 0 positions each."""
    model, eng = _model(), _engine()
    prompt = _ids(PROMPT_LEN, SEED)
    plain = _plain(prompt, NEW)
    fn = dict(oracle=_oracle_draft(plain), adversarial=_adversarial_draft(plain), lookup=None)[draft]
    got = D.engine_generate(model, prompt, max_new_tokens=NEW, engine=eng, prefill='engine', speculate=dict(k=K, draft=fn))
    assert got.shape == (1, PROMPT_LEN + NEW) and got.dtype == prompt.dtype and torch.equal(got[:, :PROMPT_LEN], prompt)
    st = eng.spec_stats
    print('%s draft: %r' % (draft, st))
    _check_sequence(draft, got, PROMPT_LEN)
    assert st['steps'] == len(st['accepted']) and all(0 <= a <= K for a in st['accepted'])
    if draft == 'oracle':
        assert st['steps'] <= math.ceil(NEW / R) + 1
        assert sum(1 for a in st['accepted'] if a != K) <= 1, st            # every step accepted 4, but for one near tie at most
    if draft == 'adversarial':
        assert all(a == 0 for a in st['accepted']) and st['emitted'] == st['steps'], st
        assert st['steps'] == NEW - 2                                      # the last token comes from the single-step graph
    assert int(eng.pos[0]) == PROMPT_LEN + NEW - 1


def test_generate_speculative_eos_inside_an_accepted_run():
    model, eng = _model(), _engine()
    prompt = _ids(PROMPT_LEN, SEED)
    fn = _oracle_draft(_plain(prompt, NEW))
    full = D.engine_generate(model, prompt, max_new_tokens=NEW, engine=eng, prefill='engine', speculate=dict(k=K, draft=fn))
    gen = full[0, PROMPT_LEN:].tolist()
    # a token that first occurs INSIDE an accepted run (verify step n emits tokens 5 n - 4 .. 5 n: not the run's last one)
    cut = next(j for j in range(2, NEW - 1) if j % R != 0 and gen.index(gen[j]) == j)
    eos = gen[cut]
    got = D.engine_generate(model, prompt, max_new_tokens=NEW, eos_token_id=eos, engine=eng, prefill='engine', speculate=dict(k=K, draft=fn))
    assert torch.equal(got, full[:, :PROMPT_LEN + cut + 1])
    assert eng.spec_stats['emitted'] == cut and int(eng.pos[0]) == PROMPT_LEN + cut
    # eos as the very first token: nothing is verified
    got = D.engine_generate(model, prompt, max_new_tokens=NEW, eos_token_id=gen[0], engine=eng, prefill='engine', speculate=dict(k=K, draft=fn))
    assert torch.equal(got, full[:, :PROMPT_LEN + 1]) and eng.spec_stats['steps'] == 0


def test_generate_speculative_up_to_the_end_of_the_cache():
    """prompt + new tokens = t_max exactly: the last tokens come from the single-step greedy graph (the chunk no longer fits)"""
    model, eng = _model(), _engine()
    T, new = END_LEN, T_MAX - END_LEN
    prompt = _ids(T, SEED_END)
    fn = _oracle_draft(_plain(prompt, new))
    got = D.engine_generate(model, prompt, max_new_tokens=new, engine=eng, prefill='engine', speculate=dict(k=K, draft=fn))
    assert got.shape == (1, T_MAX)
    st = eng.spec_stats
    print('to the end of the cache: %r' % (st,))
    assert 1 + st['emitted'] < new                           # the verify steps stopped early ...
    assert T + st['emitted'] + R > T_MAX                     # ... exactly where the chunk stops fitting
    _check_sequence('end of cache', got, T)
    assert int(eng.pos[0]) == T_MAX - 1


def test_verify_greedy_graph_agrees_with_eager_verify_and_host_accept():
    eng = _engine()
    T = 64
    ids = _ids(T + 1, 900)
    if eng.verify_graph is None:
        eng.pos.zero_()
        eng.capture_verify_greedy()
    for want in (0, 2, K):
        # drafts that agree with the model for exactly `want` tokens
        eng.prefill(ids[0, :T], start=0)
        toks = [int(ids[0, T])]
        for j in range(want):
            am = eng.verify(toks).argmax(dim=-1).tolist()
            toks.append(am[j])
        if want < K:
            am = eng.verify(toks).argmax(dim=-1).tolist()
            toks.append((am[want] + 1) % VOCAB)
            toks += [7] * (R - len(toks))
        logits = eng.verify(toks)
        am = logits.argmax(dim=-1).tolist()
        a = 0
        while a < K and am[a] == toks[a + 1]:
            a += 1
        assert a == want and int(eng.pos[0]) == T
        eng.accept(a + 1)
        pos_eager = int(eng.pos[0])
        eng.prefill(ids[0, :T], start=0)                    # the same state again
        eng.chunk_ids.copy_(torch.tensor(toks, device=DEV))
        eng.verify_graph.replay()
        res = eng.verify_out.tolist()
        assert res[0] == a and res[1:] == am, (res, a, am)
        assert int(eng.pos[0]) == pos_eager == T + a + 1


def test_errors_leave_the_position_alone():
    model, eng, plain = _model(), _engine(), _plain_engine()
    prompt = _ids(PROMPT_LEN, SEED)
    eng.prefill(prompt[0], start=0)
    plain.prefill(prompt[0], start=0)
    gen = lambda **kw: D.engine_generate(model, prompt, max_new_tokens=4, prefill='engine', **kw)
    for kw in (dict(engine=eng, speculate=dict(k=K), sample=dict(temperature=0.8)),
               dict(engine=eng, speculate=dict(k=0)), dict(engine=eng, speculate=dict(k=16)), dict(engine=eng, speculate=dict(k=3)),
               dict(engine=eng, speculate=dict(k=K, tokens=3)), dict(engine=eng, speculate=4),
               dict(engine=plain, speculate=dict(k=K))):
        with pytest.raises(ValueError):
            gen(**kw)
    wide = D.DecodeEngine(model, t_max=32, batch=2)
    with pytest.raises(ValueError):
        D.engine_generate(model, prompt[:, :4], max_new_tokens=4, prefill='engine', engine=wide, speculate=dict(k=K))
    for kw in (dict(chunk=1), dict(chunk=17), dict(chunk=R, batch=2), dict(chunk=-3)):
        with pytest.raises(ValueError):
            D.DecodeEngine(model, t_max=32, **kw)
    for n in (0, R + 1, -1):
        with pytest.raises(ValueError):
            eng.accept(n)
    with pytest.raises(ValueError):
        eng.verify([])
    with pytest.raises(ValueError):
        eng.verify([1] * (R + 1))
    with pytest.raises(ValueError):
        plain.verify([1, 2])                                # an engine without chunk=R
    with pytest.raises(ValueError):
        plain.accept(1)
    with pytest.raises(ValueError):
        plain.capture_verify_greedy()
    assert int(eng.pos[0]) == PROMPT_LEN and int(plain.pos[0]) == PROMPT_LEN
    eng.pos.fill_(T_MAX - R + 1)                            # the chunk no longer fits
    with pytest.raises(ValueError):
        eng.verify([1, 2])
    with pytest.raises(ValueError):
        eng.capture_verify_greedy()                         # its warm-up step would not fit either
    assert int(eng.pos[0]) == T_MAX - R + 1
    eng.pos.fill_(T_MAX - R)
    assert eng.verify([1, 2]).shape == (2, VOCAB)
