"""GPU tests of the token log-probabilities: gptq_logprobs_rows_f16 (csrc/logprobs.hip) through the C entry against the float64 restatement of
the rule (tests/logprobs_ref.py) -- ranks and top ids exact, log-probabilities within the derived bar (logprobs_ref.bar) and no further from
float64 than fp32 torch.log_softmax is by more than that bar --, the structural, addressing and determinism cases, and the engine: the record
ring of the self-feeding steps (DecodeEngine(logprobs=K)), token_logprobs, engine_generate / engine_generate_batch(logprobs=K) on a tiny
random head_dim-128 model, t_max 64."""
import functools
import math

import numpy as np
import pytest
import torch

import logprobs_ref as R
from quant import _native
from quant import decode as D

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NEG = float('-inf')


# ---- the kernel through the C entry -------------------------------------------------------------------------------------------------------
def _view(logits_np, ld, offset=0):
    """the fp16 rows on the device at row stride ld, the first one `offset` elements behind a 256-byte boundary"""
    rows, vocab = logits_np.shape
    buf = torch.zeros(offset + rows * ld, dtype=torch.float16, device=DEV)
    view = buf[offset:].as_strided((rows, vocab), (ld, 1))
    view.copy_(torch.from_numpy(logits_np))
    return view


def _outputs(steps, rows, top, fill=None):
    out = [torch.empty((steps, rows), dtype=torch.float32, device=DEV), torch.empty((steps, rows), dtype=torch.int32, device=DEV),
           torch.empty((steps, rows, top), dtype=torch.int32, device=DEV), torch.empty((steps, rows, top), dtype=torch.float32, device=DEV)]
    if fill is not None:
        for t in out:
            t.view(torch.uint8).fill_(fill)
    return out


def _launch(view, ids, top, step=None, steps=1, out=None):
    """one launch; returns (chosen [steps, rows], rank, top_ids [steps, rows, top], top_logprobs) as numpy arrays"""
    lib = _native.lib()
    rows, vocab = view.shape
    ids_t = torch.as_tensor(np.asarray(ids, dtype=np.int64)).to(DEV)
    step_t = None if step is None else torch.tensor([step, 1], dtype=torch.int64, device=DEV)
    out = _outputs(steps, rows, top) if out is None else out
    rc = lib.gptq_logprobs_rows_f16(view.data_ptr(), view.stride(0), rows, vocab, ids_t.data_ptr(), top, _native.ptr(step_t), steps,
                                    out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr() if top else None, out[3].data_ptr() if top else None,
                                    _native.stream_ptr(torch.device(DEV)))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _check_rows(logits_np, ids, top, view):
    """slot 0 of one launch against the restatement, row by row"""
    chosen, rank, top_ids, top_lp = [a[0] for a in _launch(view, ids, top)]
    for r, row in enumerate(logits_np):
        c, k, ti, tl = R.record(row, int(ids[r]), top)
        assert int(rank[r]) == k, (r, int(rank[r]), k)
        assert top_ids[r].tolist() == ti.tolist(), r
        msg = R.close(chosen[r:r + 1], [c]) or R.close(top_lp[r], tl)
        assert msg is None, (r, msg)
    return chosen, rank, top_ids, top_lp


@pytest.mark.parametrize('vocab', [1, 7, 33, 1000, 8192 + 5, 32000, 32003])
def test_kernel_against_the_restatement(vocab):
    worst = 0.0
    for rows in (1, 3, 16):
        logits = R.random_rows(rows, vocab, 100 + rows)
        orders = [R.order(row) for row in logits]
        places = [np.argsort(o) for o in orders]                               # places[r][id] = the rank of id
        lp = [R.log_softmax(row) for row in logits]
        lp32 = torch.log_softmax(torch.from_numpy(logits).float(), dim=-1).numpy().astype(np.float64)
        for ld in (vocab + 1, (vocab + 7) // 8 * 8):                           # rows off / on 16-byte alignment
            view = _view(logits, ld)
            for seed, top in enumerate(t for t in (0, 1, 5, 32) if vocab >= t):
                ids = R.pick_ids(logits, top, seed + (ld & 1), orders)
                chosen, rank, top_ids, top_lp = [a[0] for a in _launch(view, ids, top)]
                for r in range(rows):
                    assert int(rank[r]) == int(places[r][ids[r]]), (rows, ld, top, r)
                    assert top_ids[r].tolist() == orders[r][:top].tolist(), (rows, ld, top, r)
                    got = np.concatenate([chosen[r:r + 1], top_lp[r]]).astype(np.float64)
                    at = np.concatenate([ids[r:r + 1], orders[r][:top]])
                    ref = lp[r][at]
                    msg = R.close(got, ref)
                    assert msg is None, (rows, ld, top, r, msg)
                    err = np.abs(got - ref)
                    assert (err <= np.abs(lp32[r][at] - ref) + R.bar(ref)).all(), (rows, ld, top, r)       # no worse than fp32 log_softmax
                    worst = max(worst, float((err / R.bar(ref)).max()))
                    if int(rank[r]) < top:
                        assert top_ids[r][rank[r]] == ids[r] and _bits(top_lp[r])[rank[r]] == _bits(chosen)[r]
    print('vocab', vocab, 'largest error / bar %.3f' % worst)


def test_forty_equal_maxima_straddle_the_top_boundary():
    vocab = 100
    tied = np.sort(np.random.default_rng(0).permutation(vocab)[:40])
    row = np.full((1, vocab), -13.0, dtype=np.float16)
    row[0, tied] = 3.0
    view = _view(row, vocab + 1, offset=1)
    for place in (0, 4, 5, 39):
        chosen, rank, top_ids, top_lp = _check_rows(row, [int(tied[place])], 5, view)
        assert int(rank[0]) == place and top_ids[0].tolist() == tied[:5].tolist()
        assert len(set(_bits(top_lp[0]).tolist() + _bits(chosen).tolist())) == 1  # equal logits: equal bits
    # the same class spread over several rounds of the running count, and -0 == +0
    far = np.full((2, 20011), -4.0, dtype=np.float16)
    far[0, [19999, 9000, 8192, 11]] = 3.0
    far[1, [17000, 3, 12000, 4]] = 0.0, -0.0, 0.0, -0.0
    _, rank, top_ids, _ = _check_rows(far, [19999, 17000], 2, _view(far, 20011 + 1))
    assert top_ids.tolist() == [[11, 8192], [3, 4]] and rank.tolist() == [3, 3]


def test_minus_infinity_entries():
    row = np.array([[NEG, 2.0, NEG, 1.0, 1.0]], dtype=np.float16)
    view = _view(row, 8)
    chosen, rank, top_ids, top_lp = _check_rows(row, [2], 5, view)
    assert chosen[0] == NEG and int(rank[0]) == 4 and top_ids[0].tolist() == [1, 3, 4, 0, 2] and top_lp[0, 3:].tolist() == [NEG, NEG]
    _check_rows(row, [4], 1, view)
    one = np.array([[-7.5]], dtype=np.float16)                                 # a vocabulary of one: lp = 0
    chosen, rank, top_ids, top_lp = _check_rows(one, [0], 1, _view(one, 1))
    assert chosen[0] == 0.0 and int(rank[0]) == 0 and top_lp[0, 0] == 0.0
    wide = np.full((1, 9000), NEG, dtype=np.float16)                           # fewer finite entries than top, far apart
    wide[0, [8500, 3, 700]] = 1.0, 0.5, 1.0
    _, _, top_ids, _ = _check_rows(wide, [8999], 32, _view(wide, 9001))
    assert top_ids[0, :5].tolist() == [700, 8500, 3, 0, 1]


def test_rows_without_a_distribution_leave_the_others_alone():
    rows, vocab, top = 6, 1000, 5
    logits = R.random_rows(rows, vocab, 7)
    logits[1, 150] = np.nan
    logits[3, 999] = np.inf
    logits[4, :] = NEG
    view = _view(logits, vocab + 1)
    ids = R.pick_ids(np.where(np.isfinite(logits), logits, np.float16(0)), top, 0)
    chosen, rank, top_ids, top_lp = _check_rows(logits, ids, top, view)
    for r in (1, 3, 4):
        assert math.isnan(chosen[r]) and int(rank[r]) == -1 and top_ids[r].tolist() == list(range(top)) and np.isnan(top_lp[r]).all()
    for r in (0, 2, 5):                                                        # bit-equal to the row's own launch
        alone = _launch(view[r:r + 1], ids[r:r + 1], top)
        assert _same_bits([chosen[r:r + 1], rank[r:r + 1], top_ids[r], top_lp[r]], [alone[0][0], alone[1][0], alone[2][0, 0], alone[3][0, 0]]), r


def test_an_id_outside_the_vocabulary():
    rows, vocab, top = 4, 333, 3
    logits = R.random_rows(rows, vocab, 9)
    ids = np.array([vocab, -1, 5, 2 ** 40], dtype=np.int64)
    chosen, rank, top_ids, top_lp = _check_rows(logits, ids, top, _view(logits, vocab + 1))
    assert np.isnan(chosen[[0, 1, 3]]).all() and rank.tolist()[:2] == [-1, -1] and int(rank[3]) == -1 and np.isfinite(chosen[2])
    assert np.isfinite(top_lp).all()


def test_the_slot_comes_from_device_memory():
    rows, vocab, top, steps = 3, 257, 4, 4
    logits = R.random_rows(rows, vocab, 11)
    view = _view(logits, vocab + 1)
    ids = R.pick_ids(logits, top, 1)
    want = _launch(view, ids, top)
    blank = [t.cpu().numpy() for t in _outputs(steps, rows, top, fill=0xA5)]
    got = _launch(view, ids, top, step=2, steps=steps, out=_outputs(steps, rows, top, fill=0xA5))
    for g, w, b in zip(got, want, blank):
        assert np.array_equal(_bits(g[2]), _bits(w[0]))
        for s in (0, 1, 3):
            assert np.array_equal(_bits(g[s]), _bits(b[s])), s
    for step in (4, -1, 2 ** 33):
        got = _launch(view, ids, top, step=step, steps=steps, out=_outputs(steps, rows, top, fill=0xA5))
        assert _same_bits(got, blank), step
    got = _launch(view, ids, top, step=None, steps=steps, out=_outputs(steps, rows, top, fill=0xA5))       # NULL: slot 0
    assert all(np.array_equal(_bits(g[0]), _bits(w[0])) and np.array_equal(_bits(g[1:]), _bits(b[1:])) for g, w, b in zip(got, want, blank))


def test_the_same_bits_on_every_call_and_for_a_row_on_its_own():
    rows, vocab, top = 16, 32000, 32
    logits = R.random_rows(rows, vocab, 13)
    for ld in (vocab + 1, vocab):
        view = _view(logits, ld)
        ids = R.pick_ids(logits, top, 2)
        a, b = _launch(view, ids, top), _launch(view, ids, top)
        assert _same_bits(a, b)
        for r in range(rows):
            alone = _launch(view[r:r + 1], ids[r:r + 1], top)
            assert _same_bits([x[0, r] for x in a], [x[0, 0] for x in alone]), (ld, r)


# ---- the engine ---------------------------------------------------------------------------------------------------------------------------
HD128 = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
             vocab_size=512, max_position_embeddings=512)
V = HD128['vocab_size']
T_MAX = 64
NEW = 20
KEYS = ('token_logprobs', 'ranks', 'top_ids', 'top_logprobs')


@functools.lru_cache(maxsize=None)
def _model():
    """the tiny model of the sampling tests: scales x 0.05 keep the logits finite"""
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
    gen = torch.Generator(device=DEV).manual_seed(170 + n)
    return tuple(torch.randint(1, V, (6 + 4 * i,), device=DEV, generator=gen) for i in range(n))


@functools.lru_cache(maxsize=None)
def _engine(batch=1, logprobs=None, logits_process=False):
    return D.DecodeEngine(_model(), t_max=T_MAX, batch=batch, logprobs=logprobs, logits_process=logits_process)


def _info_bits(info):
    return [_bits(info[k].cpu().numpy()) for k in KEYS]


def test_greedy_generation_records_what_it_chose():
    model, prompt = _model(), _prompts(1)[0][None]
    T = prompt.shape[1]
    plain = D.engine_generate(model, prompt, NEW, engine=_engine(), prefill='engine')
    seq, info = D.engine_generate(model, prompt, NEW, engine=_engine(logprobs=5), prefill='engine', logprobs=3)
    assert torch.equal(seq, plain) and isinstance(info, dict) and sorted(info) == sorted(KEYS)
    tokens = seq[0, T:]
    assert all(info[k].device == seq.device for k in KEYS)
    assert info['token_logprobs'].shape == (NEW,) and info['ranks'].shape == (NEW,) and info['top_ids'].shape == (NEW, 3) == info['top_logprobs'].shape
    assert info['token_logprobs'].dtype == torch.float32 and info['ranks'].dtype == torch.int32 and info['top_ids'].dtype == torch.int32
    assert (info['ranks'] == 0).all() and torch.equal(info['top_ids'][:, 0].long(), tokens)
    assert torch.equal(info['token_logprobs'].view(torch.int32), info['top_logprobs'][:, 0].contiguous().view(torch.int32))
    # a second engine is fed the same tokens through decode(): its logits rows through the restatement
    eng = _engine()
    with torch.no_grad():
        logits = eng.prefill(prompt[0], start=0)
        for n, tok in enumerate(tokens.tolist()):
            c, k, ti, tl = R.record(logits.reshape(-1).cpu().numpy(), tok, 3)
            assert k == int(info['ranks'][n]) and ti.tolist() == info['top_ids'][n].tolist(), n
            msg = R.close(info['token_logprobs'][n:n + 1].cpu().numpy(), [c]) or R.close(info['top_logprobs'][n].cpu().numpy(), tl)
            assert msg is None, (n, msg)
            logits = eng.decode(tok)[0]
    # K = 0: chosen and rank only, and the hf prefill route
    seq0, info0 = D.engine_generate(model, prompt, NEW, engine=_engine(logprobs=5), logprobs=0)
    assert info0['top_ids'].shape == (seq0.shape[1] - T, 0) and info0['token_logprobs'].shape == (seq0.shape[1] - T,)
    # engine=None: the driver builds an engine with the flag
    seq1, info1 = D.engine_generate(model, prompt, 4, t_max=T_MAX, logprobs=2)
    assert info1['top_ids'].shape == (4, 2) and (info1['ranks'] == 0).all() and torch.equal(info1['top_ids'][:, 0].long(), seq1[0, T:])


def test_sampling_draws_the_same_tokens_with_and_without_the_records():
    model, prompt = _model(), _prompts(1)[0][None]
    T = prompt.shape[1]
    sample = dict(temperature=1.5, top_k=50, top_p=0.95)
    torch.manual_seed(5)
    plain = D.engine_generate(model, prompt, NEW, engine=_engine(), prefill='engine', sample=sample)
    torch.manual_seed(5)
    seq, info = D.engine_generate(model, prompt, NEW, engine=_engine(logprobs=5), prefill='engine', sample=sample, logprobs=5)
    assert torch.equal(seq, plain)
    tokens, ranks = seq[0, T:], info['ranks'].long()
    print('ranks', ranks.tolist())
    assert (ranks >= 0).all() and (ranks > 0).any()
    inside = ranks < 5
    assert torch.equal(info['top_ids'][inside].gather(1, ranks[inside, None])[:, 0].long(), tokens[inside])
    assert (info['token_logprobs'] <= 0).all() and (info['top_logprobs'][:, :-1] >= info['top_logprobs'][:, 1:]).all()
    assert (info['token_logprobs'][~inside] <= info['top_logprobs'][~inside, -1]).all()


@pytest.mark.parametrize('batch', [1, 3])
def test_the_captured_step_and_the_eager_step_fill_bit_equal_records(batch):
    eng = D.DecodeEngine(_model(), t_max=T_MAX, batch=batch, logprobs=4)
    prompts = _prompts(batch)
    steps = 3
    with torch.no_grad():
        graph = eng.graph_for('greedy_rows')                                   # (before the prompts enter)
        first = eng.prefill_batch(list(prompts), starts=[0] * batch).argmax(dim=-1)
        pos0 = eng.pos.clone()
        bufs = (eng.stream_rows, eng.lp_chosen, eng.lp_rank, eng.lp_top_ids, eng.lp_top)

        def run(step):
            eng.pos.copy_(pos0)
            eng.ids.copy_(first)
            eng.stepc.zero_()
            for b in bufs:
                b.view(torch.uint8).fill_(0xA5)
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            assert int(eng.stepc) == steps
            return [b.clone() for b in bufs]
        eager, replayed = run(eng._greedy_rows_step), run(graph.replay)
    for a, b in zip(eager, replayed):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        assert (a[steps:].contiguous().view(torch.uint8) == 0xA5).all()        # nothing behind the steps that ran
    assert (eager[2][:steps] == 0).all() and torch.equal(eager[3][:steps, :, 0].long(), eager[0][:steps])


def test_a_batch_with_an_early_eos_cuts_the_records_with_the_tokens():
    model, prompts = _model(), list(_prompts(3))
    eng = _engine(batch=3, logprobs=2)
    seqs, infos = D.engine_generate_batch(model, prompts, NEW, engine=eng, logprobs=2)
    gens = [s[p.numel():] for s, p in zip(seqs, prompts)]
    plain = D.engine_generate_batch(model, prompts, NEW, engine=_engine(batch=3))
    assert isinstance(infos, list) and len(infos) == 3 and all(g.numel() == NEW for g in gens)
    assert all(torch.equal(a, b) for a, b in zip(seqs, plain))
    eos = int(gens[1][3])                                                      # row 1 ends after four tokens at the latest
    cut, cut_infos = D.engine_generate_batch(model, prompts, NEW, eos_token_id=eos, engine=eng, logprobs=2)
    lens = [c.numel() - p.numel() for c, p in zip(cut, prompts)]
    print('eos', eos, 'lengths', lens)
    assert 1 <= lens[1] <= 4 and int(cut[1][-1]) == eos
    for b in range(3):
        assert torch.equal(cut[b], seqs[b][:prompts[b].numel() + lens[b]])
        assert lens[b] == NEW or int(cut[b][-1]) == eos
        assert all(cut_infos[b][k].shape[0] == lens[b] for k in KEYS)
        assert all(np.array_equal(x, y[:lens[b]]) for x, y in zip(_info_bits(cut_infos[b]), _info_bits(infos[b])))
        assert torch.equal(cut_infos[b]['top_ids'][:, 0].long(), cut[b][prompts[b].numel():])
    built, built_infos = D.engine_generate_batch(model, prompts, 3, t_max=T_MAX, logprobs=1)       # engine=None: built with the flag
    assert all(torch.equal(a, b[:a.numel()]) for a, b in zip(built, seqs)) and all(i['top_logprobs'].shape == (3, 1) for i in built_infos)


def test_the_records_come_from_the_processed_logits():
    model, prompt = _model(), _prompts(1)[0][None]
    T = prompt.shape[1]
    eng = _engine(logprobs=5, logits_process=True)
    seq, info = D.engine_generate(model, prompt, NEW, engine=eng, prefill='engine', sample=dict(temperature=0), logprobs=5)
    t = int(seq[0, T])                                                         # the most probable first token: banned below
    assert int(info['top_ids'][0, 0]) == t
    seq, info = D.engine_generate(model, prompt, NEW, engine=eng, prefill='engine', sample=dict(temperature=0, logit_bias={t: NEG}), logprobs=5)
    assert (seq[0, T:] != t).all()
    assert torch.isfinite(info['top_logprobs']).all() and (info['top_ids'] != t).all()     # never ahead of a finite token: 511 of them are
    assert (info['ranks'] == 0).all()
    chosen, rank, top_ids, top_lp = eng.token_logprobs(eng.logits, torch.tensor([t], dtype=torch.int64, device=DEV), top=1)
    assert float(chosen[0]) == NEG and int(rank[0]) == V - 1 and int(top_ids[0, 0]) != t      # the last step's logits: t asked about


def test_value_errors():
    model, prompt = _model(), _prompts(1)[0][None]
    for kw in (dict(logprobs=33), dict(logprobs=-1), dict(logprobs=True), dict(logprobs=1.0), dict(logprobs=2, chunk=4),
               dict(logprobs=2, batch=2, batch_chunk=4), dict(logprobs=2, batch=2, beam_search=True)):
        with pytest.raises(ValueError, match='not built yet' if len(kw) > 1 else 'logprobs'):
            D.DecodeEngine(model, t_max=T_MAX, **kw)
    beam = D.DecodeEngine(model, t_max=T_MAX, batch=2, beam_search=True)
    for kw in (dict(logprobs=33), dict(logprobs=-1), dict(logprobs=True), dict(logprobs=1, speculate=dict(k=2)), dict(logprobs=1, engine=_engine()),
               dict(logprobs=3, engine=_engine(logprobs=2)), dict(logprobs=1, engine=beam)):
        with pytest.raises(ValueError, match='logprobs'):
            D.engine_generate(model, prompt, 4, **kw)
    prompts = list(_prompts(3))
    for kw in (dict(logprobs=33), dict(logprobs=1, speculate=dict(k=2)), dict(logprobs=1, engine=_engine(batch=3)),
               dict(logprobs=3, engine=_engine(batch=3, logprobs=2))):
        with pytest.raises(ValueError, match='logprobs'):
            D.engine_generate_batch(model, prompts, 4, **kw)
    eng = _engine(logprobs=2)
    good = torch.zeros((2, V), dtype=torch.float16, device=DEV)
    ids = torch.zeros(2, dtype=torch.int64, device=DEV)
    for logits, i, top in ((good.float(), ids, None), (good.t(), ids[:1].expand(V), None), (good.cpu(), ids, None), (good, ids.int(), None),
                           (good, ids[:1], None), (good, ids.cpu(), None), (good, ids, 33), (good, ids, -1), (good[:, :3], ids, 4),
                           (torch.zeros((129, 8), dtype=torch.float16, device=DEV), torch.zeros(129, dtype=torch.int64, device=DEV), 0)):
        with pytest.raises(ValueError, match='token_logprobs'):
            eng.token_logprobs(logits, i, top=top)
    out = eng.token_logprobs(good, ids)                                        # top = None: the engine's K; flat logits: lp = -log V
    assert out[2].shape == (2, 2) and out[2].tolist() == [[0, 1], [0, 1]] and abs(float(out[0][0]) + math.log(V)) < 1e-5
    assert _engine().token_logprobs(good[0], ids[:1])[2].shape == (1, 0)       # ... 0 on an engine without the flag
