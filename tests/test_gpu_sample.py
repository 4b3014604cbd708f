"""GPU tests of gptq_sample_rows_f16 (csrc/sample.hip) and of the engine's native sampling path (DecodeEngine.set_sampling / sample_logits /
capture_sample_native, engine_generate(..., sample=...)).  The oracle is the float64 restatement of the semantics in tests/sample_ref.py; its
`admissible` lets a draw within 1e-5 of the row's mass of a class edge go either way -- the bar the kernel's masses are held to -- and
tests/test_host_sample.py asserts on the CPU that every top-p decision used here sits at least ten times that far inside a class."""
import functools

import numpy as np
import pytest
import torch

import sample_ref as R
from quant import _native
from quant import decode as D

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN, INF = float('nan'), float('inf')
HD128 = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
             vocab_size=512, max_position_embeddings=512)
T_MAX = 128


def _dev(values, dtype):
    return torch.tensor(values, dtype=dtype).to(DEV)


def _per_row(v, rows):
    return list(v) if isinstance(v, (list, tuple)) else [v] * rows


def _op(logits, u, T, k, p, vocab=None):
    """gptq_sample_rows_f16 on a [rows, >= vocab] fp16 device tensor; u / T / k / p: a scalar or one value per row"""
    rows = logits.shape[0]
    vocab = logits.shape[1] if vocab is None else vocab
    u = u if torch.is_tensor(u) else _dev(_per_row(u, rows), torch.float32)
    T, k, p = _dev(_per_row(T, rows), torch.float32), _dev(_per_row(k, rows), torch.int32), _dev(_per_row(p, rows), torch.float32)
    out = torch.full((rows,), -1, dtype=torch.int64, device=DEV)
    rc = _native.lib().gptq_sample_rows_f16(logits.data_ptr(), logits.stride(0), rows, vocab, u.data_ptr(), T.data_ptr(), k.data_ptr(), p.data_ptr(),
                                            out.data_ptr(), _native.stream_ptr(torch.device(DEV)))
    assert rc == 0, rc
    return out.cpu().numpy()


def _stratified(n):
    return (torch.arange(n, dtype=torch.float64) + 0.5).div(n).float()


# ---- 1. the whole CDF of one row: N identical rows, u_j = (j + 0.5) / N ----
@pytest.mark.parametrize('name', [c[0] for c in R.CASES])
def test_whole_cdf(name):
    logits, T, k, p = R.case(name)
    V = logits.numel()
    N = 4096 if V <= 1000 else 512
    rows = logits.to(DEV)[None].expand(N, V).contiguous()
    u = _stratified(N)
    ids = _op(rows, u.to(DEV), T, k, p)
    ok = R.admissible_rows(ids, logits, T, k, p, u.numpy())
    print('%s: %d rows, %d distinct ids, %d not admissible' % (name, N, len(np.unique(ids)), int((~ok).sum())))
    assert ok.all(), (name, ids[~ok][:8], u.numpy()[~ok][:8])
    if V <= 1000:
        prob = R.probabilities(logits, T, k, p)
        count = np.bincount(ids, minlength=V)
        worst = np.abs(count - N * prob).max()
        print('%s: worst |count - N p_t| = %.3f (bar %.3f)' % (name, worst, 2 + 2 * N * R.EPS))
        assert worst <= 2 + 2 * N * R.EPS, name
        assert (count[prob == 0] == 0).all(), name
    assert np.array_equal(_op(rows, u.to(DEV), T, k, p), ids), name                 # the same inputs, the same ids


# ---- 2. every row its own parameters, one launch ----
def test_per_row_parameters_in_one_launch():
    logits = R.make_logits(1000, 3.0, 1)
    V = logits.numel()
    snapped = float(R.snap_top_p(logits, 0.8, 40, 0.9))
    #         T     k       p        u
    rows = [(0.0, 0, 1.0, 0.3),                 # greedy
            (1.0, 1, 1.0, 0.7),                 # k = 1: the top class only
            (1.0, 0, 1e-6, 0.9),                # p -> 0: the top class only
            (1.0, 0, 1.0, 0.41),                # everything off
            (-1.0, 0, 1.0, 0.5),                # T < 0, T NaN: greedy
            (NAN, 5, 0.5, 0.5),
            (1.0, -3, 1.0, 0.77),               # k <= 0, k >= vocab: off
            (1.0, V + 5, 1.0, 0.23),
            (1.0, 0, 2.0, 0.61),                # p >= 1: off
            (1.0, 0, 1.0, 1.0),                 # u = 1, u NaN: clamped
            (1.0, 0, 1.0, NAN),
            (0.8, 40, snapped, 0.05),
            (0.8, 40, snapped, 0.95),
            (INF, 0, 1.0, 0.5),                 # T not finite: greedy
            (1.0, 0, 0.0, 0.99),                # p <= 0: the top class only
            (1.0, 0, NAN, 0.66)]                # p NaN: off
    T, k, p, u = (list(c) for c in zip(*rows))
    ids = _op(logits.to(DEV)[None].expand(16, V).contiguous(), u, T, k, p)
    for r, (Tr, kr, pr, ur) in enumerate(rows):
        assert R.admissible(ids[r], logits, Tr, kr, pr, ur), (r, rows[r], int(ids[r]), R.sample(logits, Tr, kr, pr, ur))
    top = int(torch.argmax(logits.to(DEV)))
    assert [int(ids[r]) for r in (0, 4, 5, 13)] == [top] * 4 and [int(ids[r]) for r in (1, 2, 14)] == [top] * 3      # (one maximal logit in this row)


# ---- 3. edges ----
def test_vocab_of_one_and_a_single_row():
    assert _op(_dev([[0.3]] * 3, torch.float16), [0.0, 0.5, 0.999], [1.0, 0.0, 0.7], [0, 1, 5], [1.0, 0.5, 0.1]).tolist() == [0, 0, 0]
    logits = R.make_logits(1000, 3.0, 11)
    for u in (0.0, 0.37, 0.999):
        got = _op(logits.to(DEV)[None], u, 0.9, 0, 1.0)
        assert got.shape == (1,) and R.admissible(got[0], logits, 0.9, 0, 1.0, u), u


def test_padded_rows_are_not_read_past_the_vocabulary():
    N, V, LD = 256, 50, 64
    logits = R.make_logits(V, 3.0, 5)
    buf = torch.full((N, LD), NAN, dtype=torch.float16, device=DEV)              # a NaN the kernel read would decide the row
    buf[:, :V] = logits.to(DEV)
    u = _stratified(N)
    ids = _op(buf, u.to(DEV), 1.0, 0, 1.0, vocab=V)
    assert R.admissible_rows(ids, logits, 1.0, 0, 1.0, u.numpy()).all()
    assert len(np.unique(ids)) > 5


def test_misaligned_rows_of_a_contiguous_odd_vocabulary():
    V = 32001                                                                    # row r begins at byte 64002 r: every residue of 2 modulo 16
    rows = [R.make_logits(V, 2.5, 20 + r) for r in range(9)]
    p = [float(R.snap_top_p(l, 1.0, 50, 0.9)) for l in rows]
    u = [0.03 + 0.11 * r for r in range(9)]
    buf = torch.stack(rows).to(DEV)
    assert buf.is_contiguous() and buf.data_ptr() % 16 == 0
    ids = _op(buf, u, 1.0, 50, p)
    for r in range(9):
        assert R.top_p_margin(rows[r], 1.0, 50, p[r]) >= R.MARGIN
        assert R.admissible(ids[r], rows[r], 1.0, 50, p[r], u[r]), (r, int(ids[r]), R.sample(rows[r], 1.0, 50, p[r], u[r]))
    first = torch.argmax(buf, dim=-1).cpu().numpy()
    assert np.array_equal(_op(buf, u, 0.0, 50, p), first)                        # greedy on the same rows: torch.argmax


def test_minus_infinity_is_never_drawn():
    N = 4096
    logits = R.make_logits(1000, 3.0, 8)
    logits[::3] = -INF
    u = _stratified(N)
    ids = _op(logits.to(DEV)[None].expand(N, 1000).contiguous(), u.to(DEV), 1.0, 0, 1.0)
    assert (ids % 3 != 0).all()
    assert R.admissible_rows(ids, logits, 1.0, 0, 1.0, u.numpy()).all()
    # ... also where top-k's threshold is -inf itself: k = 900 reaches into the 334 tokens of -inf, which are kept and weigh nothing
    ids = _op(logits.to(DEV)[None].expand(N, 1000).contiguous(), u.to(DEV), 1.0, 900, 1.0)
    assert (ids % 3 != 0).all() and R.admissible_rows(ids, logits, 1.0, 900, 1.0, u.numpy()).all()


def test_non_finite_rows_give_the_documented_index():
    V = 1000
    rows = [R.make_logits(V, 3.0, 30 + r) for r in range(6)]
    rows[1][417] = NAN
    rows[2][5] = INF
    rows[3][998] = INF; rows[3][999] = NAN
    rows[4][:] = -INF                                                            # nothing to draw from: its first element
    rows[5][0] = -NAN
    T = [1.0, 1.0, 0.8, 0.0, 1.0, 1.0]
    ids = _op(torch.stack(rows).to(DEV), 0.5, T, 0, 1.0)
    assert ids.tolist()[1:4] == [417, 5, 998] and ids[5] == 0 and ids[4] == 0
    assert ((ids >= 0) & (ids < V)).all()
    for r in (0, 1, 2, 3, 5):                                                    # the finite row between them is sampled as ever
        assert R.admissible(ids[r], rows[r], T[r], 0, 1.0, 0.5)


# ---- 4. the engine ----
@functools.lru_cache(maxsize=None)
def _model():
    """the tiny head_dim-128 model of the other engine tests, with the finite-logits initialisation of the sampling bench leg (scales x 0.05)"""
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
    gen = torch.Generator(device=DEV).manual_seed(40 + n)
    return tuple(torch.randint(1, HD128['vocab_size'], (5 + 3 * i,), device=DEV, generator=gen) for i in range(n))


@functools.lru_cache(maxsize=None)
def _gen_engine():
    return D.DecodeEngine(_model(), t_max=T_MAX).capture()


@functools.lru_cache(maxsize=None)
def _gen_engine4():
    return D.DecodeEngine(_model(), t_max=T_MAX, batch=4)


@pytest.mark.parametrize('batch', [1, 4])
def test_capture_sample_native_replays_the_eager_step(batch):
    eng = D.DecodeEngine(_model(), t_max=T_MAX, batch=batch)
    assert torch.isfinite(eng.prefill_batch(list(_prompts(batch))).float()).all()
    eng.set_sampling(temperature=[0.9, 1.5, 0.7, 1.0][:batch], top_k=[0, 20, 0, 5][:batch], top_p=[0.95, 1.0, 0.8, 1.0][:batch])
    eng.ids.copy_(torch.argmax(eng.logits, dim=-1))
    pos0, ids0 = eng.pos.clone(), eng.ids.clone()
    torch.manual_seed(5)
    eager = []
    with torch.no_grad():
        for _ in range(24):
            eng._sample_native_step()
            eager.append(eng.ids.clone())
    eager = torch.stack(eager)
    assert torch.equal(eng.stream_rows[:24], eager) and int(eng.stepc) == 24
    eng.pos.copy_(pos0); eng.ids.copy_(ids0)
    torch.manual_seed(5)
    before = torch.cuda.get_rng_state(DEV)
    g = eng.capture_sample_native()
    assert torch.equal(torch.cuda.get_rng_state(DEV), before)                    # the capture leaves the generator where it found it
    assert torch.equal(eng.pos, pos0) and torch.equal(eng.ids, ids0) and int(eng.stepc) == 0
    for _ in range(24):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(eng.stream_rows[:24], eager), (eng.stream_rows[:24].t().tolist(), eager.t().tolist())
    assert len(torch.unique(eager)) > 4


def test_temperature_zero_is_the_greedy_generation():
    model, eng = _model(), _gen_engine()
    ids = _prompts(1)[0][None]
    greedy = D.engine_generate(model, ids, 24, engine=eng, prefill='engine')
    assert torch.equal(D.engine_generate(model, ids, 24, engine=eng, prefill='engine', sample=dict(temperature=0)), greedy)
    assert torch.equal(D.engine_generate(model, ids, 24, engine=eng, prefill='engine', sample=dict(temperature=0.0, top_k=7, top_p=0.5)), greedy)
    prompts, eng4 = list(_prompts(4)), _gen_engine4()
    want = D.engine_generate_batch(model, prompts, 20, engine=eng4)
    got = D.engine_generate_batch(model, prompts, 20, engine=eng4, sample=dict(temperature=[0, 0, 0, 0]))
    assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, want))


def test_sampled_generation_follows_the_seed():
    model, eng = _model(), _gen_engine()
    ids = _prompts(1)[0][None]

    def run(seed):
        torch.manual_seed(seed)
        out = D.engine_generate(model, ids, 32, engine=eng, prefill='engine', sample=dict(temperature=1.5))
        assert out.shape == (1, ids.shape[1] + 32) and torch.equal(out[:, :ids.shape[1]], ids)
        return out[0, ids.shape[1]:]
    a, b, c = run(3), run(3), run(4)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert int(a.min()) >= 0 and int(a.max()) < HD128['vocab_size']
    prompts, eng4 = list(_prompts(4)), _gen_engine4()
    torch.manual_seed(3)
    x = D.engine_generate_batch(model, prompts, 20, engine=eng4, sample=dict(temperature=[1.5, 0, 0.8, 1.0], top_k=[0, 0, 10, 0], top_p=0.95))
    torch.manual_seed(3)
    y = D.engine_generate_batch(model, prompts, 20, engine=eng4, sample=dict(temperature=[1.5, 0, 0.8, 1.0], top_k=[0, 0, 10, 0], top_p=0.95))
    greedy = D.engine_generate_batch(model, prompts, 20, engine=eng4)
    assert all(torch.equal(p, q) for p, q in zip(x, y))
    assert torch.equal(x[1], greedy[1]) and not torch.equal(x[0], greedy[0])    # the row with temperature 0 stays greedy among sampling neighbours


def test_sample_logits_against_the_oracle():
    eng = _gen_engine()
    eng.prefill(_prompts(1)[0], start=0)
    logits = eng.logits[:1].clone()
    row = logits[0].cpu()
    assert torch.isfinite(row.float()).all()
    eng.set_sampling(temperature=0.8, top_k=50, top_p=1.0)
    for u in (0.0, 0.21, 0.5, 0.87, 0.9999):
        got = eng.sample_logits(logits, u=_dev([u], torch.float32))
        assert got.dtype == torch.int64 and got.shape == (1,)
        assert R.admissible(int(got[0]), row, 0.8, 50, 1.0, u), (u, int(got[0]), R.sample(row, 0.8, 50, 1.0, u))
    p = float(R.snap_top_p(row, 1.0, 0, 0.9))
    eng.set_sampling(temperature=1.0, top_p=p)
    out = torch.empty(1, dtype=torch.int64, device=DEV)
    assert eng.sample_logits(logits[0], out=out, u=_dev([0.5], torch.float32)) is out
    assert R.top_p_margin(row, 1.0, 0, p) >= R.MARGIN and R.admissible(int(out[0]), row, 1.0, 0, p, 0.5)
    state = torch.cuda.get_rng_state(DEV)
    eng.sample_logits(logits, u=_dev([0.5], torch.float32))
    assert torch.equal(torch.cuda.get_rng_state(DEV), state)                     # with a given u nothing random happens
    torch.manual_seed(9)
    a = eng.sample_logits(logits)
    torch.manual_seed(9)
    assert torch.equal(eng.sample_logits(logits), a)                             # without: torch's CUDA generator


def test_set_sampling_changes_the_behaviour_without_a_new_capture():
    eng = D.DecodeEngine(_model(), t_max=T_MAX, batch=2)
    eng.prefill_batch(list(_prompts(2)))
    eng.ids.copy_(torch.argmax(eng.logits, dim=-1))
    eng.set_sampling(temperature=1.5)
    g = eng.capture_sample_native()
    torch.manual_seed(11)
    for _ in range(8):
        g.replay()
    eng.set_sampling(temperature=[0.0, 1.5])                                     # row 0 turns greedy, its neighbour keeps sampling
    assert eng.sample_native_graph is g
    pos0, ids0 = eng.pos.clone(), eng.ids.clone()
    eng.stepc.zero_()
    torch.manual_seed(12)
    for _ in range(16):
        g.replay()
    torch.cuda.synchronize()
    mixed = eng.stream_rows[:16].clone()
    assert eng.sample_native_graph is g
    eng.pos.copy_(pos0); eng.ids.copy_(ids0)
    eng.capture_greedy_rows()
    for _ in range(16):
        eng.greedy_rows_graph.replay()
    torch.cuda.synchronize()
    greedy = eng.stream_rows[:16].clone()
    assert torch.equal(mixed[:, 0], greedy[:, 0]), (mixed[:, 0].tolist(), greedy[:, 0].tolist())
    assert not torch.equal(mixed[:, 1], greedy[:, 1])
    eng.set_sampling(temperature=[0.0, 0.0])                                     # ... and now both: the greedy stream from the same state
    eng.pos.copy_(pos0); eng.ids.copy_(ids0); eng.stepc.zero_()
    for _ in range(16):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(eng.stream_rows[:16], greedy)


def test_bad_sampling_settings_are_refused():
    model, eng = _model(), _gen_engine()
    ids = _prompts(1)[0][None]
    for bad in (dict(foo=1), dict(temperature=-1), dict(top_p=0), dict(top_p=1.5), dict(top_k=-2), dict(temperature=INF), dict(temperature=NAN),
                dict(temperature=[1.0, 1.0])):
        with pytest.raises(ValueError):
            D.engine_generate(model, ids, 4, engine=eng, prefill='engine', sample=bad)
        with pytest.raises(ValueError):
            D.engine_generate_batch(model, list(_prompts(4)), 4, engine=_gen_engine4(), sample=bad)
    with pytest.raises(ValueError):
        eng.set_sampling(temperature=-0.5)
    with pytest.raises(ValueError):
        eng.sample_logits(eng.logits.float())
