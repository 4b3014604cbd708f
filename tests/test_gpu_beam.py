"""GPU tests of the beam-search kernels (csrc/beam.hip) through the C entries: gptq_beam_select_f16 against the float64 restatement of the rule
(tests/beam_ref.py) -- exact parents, tokens, flags and pool entries, scores within the derived bar -- on random rows whose decision gaps
tests/test_host_beam.py holds far above that bar, and on constructed rows: ties at every level, -0, odd offsets, -inf, NaN, the first step, EOS
on both sides of rank N, the last step; gptq_kv_reorder_f16 against index_select, bit for bit, with everything at or past len untouched."""
import numpy as np
import pytest
import torch

import beam_ref as R
from quant import _native

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NEG = float('-inf')


def _select(logits, st):
    """one step of the kernel on `logits` (a torch fp16 [N, vocab] tensor, any row stride) from the oracle State `st`; returns (unpacked block,
    its words)"""
    lib = _native.lib()
    w = torch.from_numpy(R.pack(st)).to(DEV)
    rc = lib.gptq_beam_select_f16(logits.data_ptr(), logits.stride(0), st.n, logits.shape[1], w.data_ptr(), _native.stream_ptr(torch.device(DEV)))
    assert rc == 0, rc
    torch.cuda.synchronize()
    words = w.cpu().numpy()
    return R.unpack(words), words


def _mid(n, score, t=3, max_new=50, **kw):
    st = R.State(n, max_new, t_cap=64, **kw)
    st.t, st.score = t, np.asarray(score, dtype=np.float64)
    return st


def _check(logits_np, st, dev_logits=None):
    """the kernel's step against the oracle's on the same fp16 logits"""
    logits_np = np.asarray(logits_np, dtype=np.float16)
    dev = torch.from_numpy(logits_np).to(DEV) if dev_logits is None else dev_logits
    got, _ = _select(dev, st)
    want = R.step(st.copy(), logits_np.astype(np.float64))
    msg = R.same_step(got, want)
    assert msg is None, msg
    assert got['status'] == 0
    return got, want


@pytest.mark.parametrize('n,vocab', R.SELECT_SHAPES)
def test_select_against_the_oracle(n, vocab):
    logits, score = R.select_inputs(n, vocab, 0)
    got, want = _check(logits, _mid(n, score))
    print(n, vocab, 'parents', got['parent'].tolist(), 'max score error %.3g' % max(abs(a[0] - b[0]) for a, b in zip(got['cand'], want.cand)))
    assert len(set(c[1] for c in got['cand'])) >= 2


def test_equal_logits_straddle_the_last_place_of_a_row():
    # N = 2: a row's own top 4 = two distinct values and two of MANY equal ones: the lowest ids win, also far apart (several rounds of the count)
    vocab = 20011
    logits = np.full((2, vocab), -4.0, dtype=np.float16)
    logits[0, [17000, 3]] = 6.0, 5.0
    logits[0, [19999, 9000, 8192, 11]] = 3.0                                 # 11 and 8192: found in different rounds
    logits[1, [1, 20010]] = 6.5, 3.0
    logits[1, 5000:5003] = 2.0
    got, _ = _check(logits, _mid(2, [-0.5, -0.75]))
    assert all(c[2] in ((17000, 3, 11, 8192) if c[1] == 0 else (1, 20010, 5000, 5001)) for c in got['cand'])
    # ... and with every element of the row equal
    flat = np.zeros((2, 100), dtype=np.float16)
    got, _ = _check(flat, _mid(2, [-1.0, -2.0]))
    assert [c[1:3] for c in got['cand']] == [(0, 0), (0, 1), (0, 2), (0, 3)]


def test_identical_rows_with_identical_scores_and_signed_zero():
    rng = np.random.default_rng(5)
    row = (rng.standard_normal(300) * 3).astype(np.float16)
    got, _ = _check(np.stack([row, row, row]), _mid(3, [-1.0, -1.0, -1.0]))
    assert [c[1] for c in got['cand']] == [0, 1, 2, 0, 1, 2]                  # equal scores: the lower beam first
    z = np.full((2, 40), -3.0, dtype=np.float16)
    z[0, [30, 4, 9, 20]] = 0.0, -0.0, 0.0, -0.0                               # -0 == +0: the id decides
    z[1, :] = -9.0
    got, _ = _check(z, _mid(2, [-1.0, -1.0]))
    assert [c[1:3] for c in got['cand']] == [(0, 4), (0, 9), (0, 20), (0, 30)]


def test_rows_at_an_odd_element_offset():
    n, vocab = 4, 1000
    logits, score = R.select_inputs(n, vocab, 0)
    buf = torch.zeros(n * (vocab + 1) + 1, dtype=torch.float16, device=DEV)
    view = buf[1:].as_strided((n, vocab), (vocab + 1, 1))
    view.copy_(torch.from_numpy(logits))
    assert view.data_ptr() % 4 == 2
    _check(logits, _mid(n, score), dev_logits=view)


def test_minus_infinity_logits():
    logits = np.full((2, 50), NEG, dtype=np.float16)
    logits[0, [7, 40]] = 1.0, 2.0                                             # fewer finite logits than 2N: -inf candidates are ranked too
    logits[1, 3] = 0.5
    got, _ = _check(logits, _mid(2, [-0.25, -0.5]))
    assert [np.isfinite(c[0]) for c in got['cand']] == [True, True, True, False] and got['cand'][3] == (NEG, 0, 0, False)
    logits[1, [4, 5, 6, 8]] = 0.25, 0.0, -1.0, -2.0
    got, _ = _check(logits, _mid(2, [-0.25, -0.5]))
    assert all(np.isfinite(c[0]) for c in got['cand'])


def test_a_nan_row_sets_the_status_bit_and_keeps_every_id_in_range():
    n, vocab = 3, 200
    logits, score = R.select_inputs(n, vocab, 1)
    for poison in (np.nan, np.inf):
        bad = logits.copy()
        bad[1, 150] = poison
        got, _ = _select(torch.from_numpy(bad).to(DEV), _mid(n, score))
        assert got['status'] & 1
        assert all(0 <= p < n for p in got['parent']) and all(0 <= v < vocab for v in got['token'])
        assert all(0 <= c[1] < n and 0 <= c[2] < vocab for c in got['cand'])
        assert all(c[1] != 1 for c in got['cand'])                            # its candidates score DEAD: twelve live ones are ahead
    only = logits.copy()
    only[2, :] = NEG                                                          # a row of -inf only
    got, _ = _select(torch.from_numpy(only).to(DEV), _mid(n, score))
    assert got['status'] & 1 and all(0 <= v < vocab for v in got['token'])


def test_first_step_takes_all_candidates_from_row_0():
    rng = np.random.default_rng(11)
    logits = (rng.standard_normal((4, 333)) * 3).astype(np.float16)
    logits[1:] += np.float16(4.0)                                             # the dead beams' rows would win on logits alone
    got, _ = _check(logits, R.State(4, 20, t_cap=64))
    assert all(c[1] == 0 for c in got['cand']) and got['parent'].tolist() == [0] * 4 and got['t'] == 1


def _prob_rows(*rows):
    return np.log(np.array(rows, dtype=np.float64)).astype(np.float16)


def test_eos_below_and_above_rank_n():
    # the second and third step of tests/test_host_beam.py test_eos_below_n_is_pooled_and_above_n_is_dropped
    st = _mid(2, np.log([0.5, 0.3]), t=1, max_new=5, eos=3)
    got, want = _check(_prob_rows([0.1, 0.1, 0.1, 0.7], [0.6, 0.2, 0.1, 0.1]), st)
    assert got['cand'][0][1:] == (0, 3, True) and got['pool'][0]['finished'] and not got['pool'][1]['finished']
    assert got['parent'].tolist() == [1, 1] and got['token'].tolist() == [0, 1]
    got, _ = _check(_prob_rows([0.4, 0.3, 0.2, 0.1], [0.05, 0.05, 0.1, 0.8]), want)
    assert got['cand'][2][1:] == (1, 3, True) and sum(e['finished'] for e in got['pool']) == 1
    assert got['parent'].tolist() == [0, 0] and got['token'].tolist() == [0, 1]


@pytest.mark.parametrize('es', [False, True, 'never'])
def test_the_last_step_pools_the_top_n(es):
    n, vocab = 4, 1000
    logits, score = R.select_inputs(n, vocab, 0)
    got, _ = _check(logits, _mid(n, score, t=9, max_new=10, early_stopping=es, length_penalty=2.0))
    assert got['done'] and all(c[3] for c in got['cand']) and all(e['finished'] and e['step'] == 9 for e in got['pool'])
    # ... and a finished search is left alone
    st = _mid(n, score, t=9, max_new=10)
    st.done = True
    _, words = _select(torch.from_numpy(logits).to(DEV), st)
    assert np.array_equal(words[:R.W_REC], R.pack(st)[:R.W_REC]) and np.array_equal(words[R.W_TABLES:], R.pack(st)[R.W_TABLES:])


def test_two_calls_leave_bit_equal_state():
    n, vocab = 16, 32000
    logits, score = R.select_inputs(n, vocab, 0)
    dev = torch.from_numpy(logits).to(DEV)
    st = _mid(n, score, eos=int(np.argmax(logits[0].astype(np.float32))))
    _, a = _select(dev, st)
    _, b = _select(dev, st)
    assert np.array_equal(a, b)


# ---- the reorder ----
LAYERS, ROWS, T_MAX, H = 2, 4, 64, 256
PARENTS = ((0, 1, 2, 3), (1, 0, 2, 3), (0, 0, 0, 0), (1, 2, 3, 0), (2, 2, 0, 0))


def _pattern(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2 ** 15, 2 ** 15, (LAYERS, ROWS, T_MAX, H), generator=g, dtype=torch.int32).to(torch.int16).to(DEV)


@pytest.mark.parametrize('parent', PARENTS)
def test_reorder_is_index_select_below_len_and_touches_nothing_else(parent):
    lib = _native.lib()
    k0, v0 = _pattern(1), _pattern(2)
    par = torch.tensor(parent, dtype=torch.int32, device=DEV)
    for n in (0, 1, 37, 64):
        k, v = k0.clone(), v0.clone()
        ln = torch.tensor([n, 999], dtype=torch.int64, device=DEV)
        rc = lib.gptq_kv_reorder_f16(k.data_ptr(), v.data_ptr(), LAYERS, ROWS, T_MAX, H, k.stride(0), par.data_ptr(), ln.data_ptr(),
                                     _native.stream_ptr(torch.device(DEV)))
        assert rc == 0, rc
        torch.cuda.synchronize()
        for got, src in ((k, k0), (v, v0)):
            want = src.clone()
            want[:, :, :n] = src.index_select(1, par.long())[:, :, :n]
            assert torch.equal(got, want), (parent, n)


def test_reorder_walks_its_grid_more_than_once():
    """8 layers x 2 x 2047 positions x 32 chunks = 1 047 808 columns for the kernel's fixed grid of 2048 x 256 threads: the grid-stride step and the
    column split beyond the first pass; a cycle, so every row moves"""
    lib = _native.lib()
    layers, t_max, n = 8, 2048, 2047
    g = torch.Generator(device=DEV).manual_seed(3)
    k0 = torch.randint(-2 ** 15, 2 ** 15, (layers, ROWS, t_max, H), generator=g, dtype=torch.int32, device=DEV).to(torch.int16)
    v0 = torch.randint(-2 ** 15, 2 ** 15, (layers, ROWS, t_max, H), generator=g, dtype=torch.int32, device=DEV).to(torch.int16)
    assert layers * 2 * n * (H // 8) > 2048 * 256
    par = torch.tensor((1, 2, 3, 0), dtype=torch.int32, device=DEV)
    ln = torch.tensor([n], dtype=torch.int64, device=DEV)
    k, v = k0.clone(), v0.clone()
    rc = lib.gptq_kv_reorder_f16(k.data_ptr(), v.data_ptr(), layers, ROWS, t_max, H, k.stride(0), par.data_ptr(), ln.data_ptr(),
                                 _native.stream_ptr(torch.device(DEV)))
    assert rc == 0, rc
    torch.cuda.synchronize()
    for got, src in ((k, k0), (v, v0)):
        assert torch.equal(got[:, :, :n], src.index_select(1, par.long())[:, :, :n])
        assert torch.equal(got[:, :, n:], src[:, :, n:])
