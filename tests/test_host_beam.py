"""CPU-side tests of beam search (include/gptq_mi355x.h "beam search"): the three symbols are exported and bound, every NULL / shape / alignment
rule of gptq_beam_select_f16 and gptq_kv_reorder_f16 returns its code on fake pointers (nothing is launched), the float64 restatement of the rule
(tests/beam_ref.py) gives the hand-worked answers and agrees with the installed transformers' `generate(num_beams=N)` on a tiny fp32 CPU model,
and the inputs of the GPU select test keep their decisions far from the kernel's error bar."""
import functools

import numpy as np
import pytest
import torch

import beam_ref as R
from quant import _native

E_SHAPE, E_ALIGN, E_NULL = -2, -3, -4
NEG = float('-inf')


# ---- 1. the symbols ----
def test_symbols_are_exported_and_bound():
    lib = _native.lib()
    for name, nargs in (('gptq_beam_state_bytes', 2), ('gptq_beam_select_f16', 6), ('gptq_kv_reorder_f16', 10)):
        assert hasattr(lib, name) and name in _native.EXPORTS
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert lib.gptq_beam_state_bytes(4, 64) == 4 * R.state_words(4, 64)
    assert lib.gptq_beam_state_bytes(16, 2048) == 4 * R.state_words(16, 2048)
    for beams, t_max in ((1, 64), (17, 64), (4, 0)):
        assert lib.gptq_beam_state_bytes(beams, t_max) == 0


# ---- 2. validation on fake pointers ----
def _select(lib, logits=4096, ld=1000, beams=4, vocab=1000, state=8192):
    return lib.gptq_beam_select_f16(logits, ld, beams, vocab, state, None)


def test_select_validation():
    lib = _native.lib()
    assert _select(lib, logits=None) == E_NULL and _select(lib, state=None) == E_NULL
    assert _select(lib, logits=None, beams=1) == E_NULL                       # NULL before shape
    assert _select(lib, state=None, logits=4097) == E_NULL                    # ... and before alignment
    for kw in (dict(beams=1), dict(beams=17), dict(beams=0), dict(vocab=7, ld=7), dict(ld=999), dict(beams=16, vocab=31, ld=31)):
        assert _select(lib, **kw) == E_SHAPE, kw
    assert _select(lib, beams=17, state=8192 + 8) == E_SHAPE                  # shape before alignment
    assert _select(lib, logits=4097) == E_ALIGN                               # fp16 rows: 2 bytes, nothing more
    for off in (4, 8):
        assert _select(lib, state=8192 + off) == E_ALIGN


def _reorder(lib, k=4096, v=1 << 20, layers=2, rows=4, t_max=64, row_elems=256, layer_stride=4 * 64 * 256, parent=8192, len_=16384):
    return lib.gptq_kv_reorder_f16(k, v, layers, rows, t_max, row_elems, layer_stride, parent, len_, None)


def test_reorder_validation():
    lib = _native.lib()
    for name in ('k', 'v', 'parent', 'len_'):
        assert _reorder(lib, **{name: None}) == E_NULL, name
    assert _reorder(lib, k=None, rows=0) == E_NULL and _reorder(lib, parent=None, v=(1 << 20) + 2) == E_NULL
    for kw in (dict(rows=0), dict(rows=17), dict(row_elems=252), dict(row_elems=0), dict(row_elems=4), dict(layers=0), dict(t_max=0),
               dict(layer_stride=4 * 64 * 256 - 8), dict(layer_stride=4 * 64 * 256 + 4)):
        assert _reorder(lib, **kw) == E_SHAPE, kw
    assert _reorder(lib, rows=17, k=4096 + 8) == E_SHAPE
    assert _reorder(lib, k=4096 + 8) == E_ALIGN and _reorder(lib, v=(1 << 20) + 8) == E_ALIGN
    assert _reorder(lib, parent=8192 + 2) == E_ALIGN and _reorder(lib, len_=16384 + 4) == E_ALIGN


# ---- 3. hand-worked cases of the restatement ----
def _rows(*rows):
    """rows of PROBABILITIES (summing to one) as logits"""
    return np.log(np.array(rows, dtype=np.float64))


def test_first_step_takes_everything_from_beam_0():
    st = R.State(2, 5)
    R.step(st, _rows([0.1, 0.4, 0.2, 0.3], [0.7, 0.1, 0.1, 0.1]))
    assert [c[1:3] for c in st.cand] == [(0, 1), (0, 3), (0, 2), (0, 0)]
    assert st.parent.tolist() == [0, 0] and st.token.tolist() == [1, 3]
    assert np.allclose(st.score, np.log([0.4, 0.3]), atol=1e-7) and st.t == 1 and st.open and not st.done


def test_eos_below_n_is_pooled_and_above_n_is_dropped():
    # N = 2, eos = 3.  Second step: beam 0 (score log .5) and beam 1 (log .3)
    st = R.State(2, 5, eos=3)
    R.step(st, _rows([0.5, 0.3, 0.15, 0.05], [0.25] * 4))                      # beams (0, tok 0), (0, tok 1)
    assert st.token.tolist() == [0, 1] and not any(e['finished'] for e in st.pool)
    # candidates: b0: .5 x (.1, .1, .1, .7) -> eos .35 at rank 0; b1: .3 x (.6, .2, .1, .1) -> .18 rank 1, .06 rank 2, the others .05 | .03 eos
    R.step(st, _rows([0.1, 0.1, 0.1, 0.7], [0.6, 0.2, 0.1, 0.1]))
    assert [c[1:] for c in st.cand] == [(0, 3, True), (1, 0, False), (1, 1, False), (0, 0, False)]
    assert st.pool[0]['finished'] and (st.pool[0]['step'], st.pool[0]['parent'], st.pool[0]['token']) == (1, 0, 3)
    assert abs(st.pool[0]['score'] - np.log(0.35) / 2) < 1e-7 and not st.pool[1]['finished']
    assert st.parent.tolist() == [1, 1] and st.token.tolist() == [0, 1]         # the hit is no running beam
    assert R.result(st)[0][0] == [0, 3]
    # third step: the eos of beam 1 ranks 2 = N: neither pooled nor continued
    R.step(st, _rows([0.4, 0.3, 0.2, 0.1], [0.05, 0.05, 0.1, 0.8]))            # b0: .18 x .. = .072, .054, .036, .018; b1: .06 x .8 = .048 (eos)
    assert [c[1:] for c in st.cand] == [(0, 0, False), (0, 1, False), (1, 3, True), (0, 2, False)]
    assert sum(e['finished'] for e in st.pool) == 1
    assert st.parent.tolist() == [0, 0] and st.token.tolist() == [0, 1]


def test_last_step_pools_the_top_n():
    st = R.State(2, 2)
    R.step(st, _rows([0.5, 0.3, 0.15, 0.05], [0.25] * 4))
    R.step(st, _rows([0.4, 0.3, 0.2, 0.1], [0.7, 0.1, 0.1, 0.1]))             # .2, .15, .1, .05 | .21, .03 ..
    assert st.done and all(c[3] for c in st.cand)
    got = R.result(st)
    assert [g[0] for g in got] == [[1, 0], [0, 0]] and abs(got[0][1] - np.log(0.21) / 2) < 1e-7 and abs(got[1][1] - np.log(0.2) / 2) < 1e-7
    assert st.score.tolist() == [R.DEAD, R.DEAD]


def test_early_stopping_true_stops_at_a_full_pool():
    for es in (True, False):
        st = R.State(2, 9, eos=3, early_stopping=es, length_penalty=0.0)
        R.step(st, _rows([0.45, 0.05, 0.05, 0.45], [0.25] * 4))                # tok 0 and eos tie: eos at rank 1 < N is pooled
        assert sum(e['finished'] for e in st.pool) == 1 and not st.done
        R.step(st, _rows([0.1, 0.1, 0.1, 0.7], [0.25] * 4))
        assert sum(e['finished'] for e in st.pool) == 2
        # length_penalty 0: best = log .045 is below both pooled scores, so `open` closes either way; with True the full pool alone would do
        assert st.done
    st = R.State(2, 9, eos=3, early_stopping=True, length_penalty=5.0)          # a penalty under which the running beam could still win
    R.step(st, _rows([0.45, 0.05, 0.05, 0.45], [0.25] * 4))
    R.step(st, _rows([0.1, 0.1, 0.1, 0.7], [0.25] * 4))
    assert st.open and st.done and sum(e['finished'] for e in st.pool) == 2
    st = R.State(2, 9, eos=3, early_stopping=False, length_penalty=5.0)
    R.step(st, _rows([0.45, 0.05, 0.05, 0.45], [0.25] * 4))
    R.step(st, _rows([0.1, 0.1, 0.1, 0.7], [0.25] * 4))
    assert st.open and not st.done


def test_the_three_tie_levels():
    # score first; equal scores: the lower beam; equal beam: the lower token
    st = R.State(2, 5)
    st.score = np.array([-1.0, -1.0])
    st.t = 1
    l = np.log(np.array([0.125, 0.25, 0.25, 0.375]))
    R.step(st, np.stack([l, l]))
    assert [c[1:3] for c in st.cand] == [(0, 3), (1, 3), (0, 1), (0, 2)]
    assert st.parent.tolist() == [0, 1] and st.token.tolist() == [3, 3]


# ---- 4. the restatement against transformers ----
SETTINGS = ((2, 1.0, False, 5, 12), (4, 1.0, True, 7, 12), (3, 0.0, False, 11, 10), (4, 2.0, 'never', 3, 10), (4, 1.0, False, None, 6),
            (5, 0.5, False, 2, 14))


@functools.lru_cache(maxsize=None)
def _tiny(seed):
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(seed)
    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4, vocab_size=97,
                      max_position_embeddings=64, pad_token_id=0, bos_token_id=None, eos_token_id=None)
    model = LlamaForCausalLM(cfg).float().eval()
    with torch.no_grad():
        model.lm_head.weight.mul_(8)
    return model


def _hf_case(seed, n, lp, es, eos, max_new, early_eos):
    model = _tiny(seed)
    prompt = torch.randint(1, 97, (1, 5), generator=torch.Generator().manual_seed(100 + seed))

    def logits_fn(beams):
        ids = torch.tensor([prompt[0].tolist() + b for b in beams])
        with torch.no_grad():
            return model(ids).logits[:, -1].double().numpy()
    if early_eos and eos is not None:                   # a token from the middle of the best hypothesis without EOS: hypotheses finish early
        eos = R.result(R.search(logits_fn, n, max_new, None, lp, es))[0][0][max_new // 2]
    st = R.search(logits_fn, n, max_new, eos, lp, es)
    with torch.no_grad():
        out = model.generate(prompt, num_beams=n, num_return_sequences=n, do_sample=False, max_new_tokens=max_new, eos_token_id=eos,
                             length_penalty=lp, early_stopping=es, output_scores=True, return_dict_in_generate=True, pad_token_id=0)
    got = R.result(st)
    assert len(got) == n
    early = 0
    for i, (toks, score) in enumerate(got):
        hf = out.sequences[i, prompt.shape[1]:].tolist()
        assert hf[:len(toks)] == toks, (seed, i, hf, toks)
        assert len(set(hf[len(toks):])) <= 1                                  # HF's padding
        assert abs(float(out.sequences_scores[i]) - score) <= 1e-4 * abs(score), (seed, i)
        early += len(toks) < max_new
    return early


def test_restatement_is_transformers_beam_search():
    with_early = 0
    for n, lp, es, eos, max_new in SETTINGS:
        early = [_hf_case(seed, n, lp, es, eos, max_new, early_eos=seed == 1) for seed in range(2)]
        print('setting', (n, lp, es, eos, max_new), 'hypotheses finished before the limit, per seed:', early)
        with_early += sum(early) > 0
    assert with_early >= 2


# ---- 5. the GPU select test's inputs keep their decisions away from the kernel's error ----
@pytest.mark.parametrize('n,vocab', R.SELECT_SHAPES)
def test_select_inputs_have_margin(n, vocab):
    logits, score = R.select_inputs(n, vocab, 0)
    gap = R.min_gap(logits.astype(np.float64), score.astype(np.float64), n)
    c, order = R.candidates(logits.astype(np.float64), score.astype(np.float64))
    top = order[:2 * n]
    bar = R.ABS_BAR + R.REL_BAR * float(np.abs(c[top]).max())
    beams = len(set((top // vocab).tolist()))
    print(n, vocab, 'gap %.3g = %.0f x bar, candidates from %d beams' % (gap, gap / bar, beams))
    assert gap >= 100 * bar
    assert beams >= 2
