"""GPU tests of gptq_logits_process_f16 (csrc/logits_process.hip) against the numpy restatement of its semantics (tests/logits_process_ref.py,
pinned to transformers' processors by tests/test_host_logits_process.py): BIT FOR BIT, logits and history, on logits at the scale an LM head
produces (sigma 3) with a few -inf and one -0 planted in every row.  Vocabularies that are no multiple of 32 with an odd leading dimension (a row
start is 2-byte aligned only), histories of 0 .. 2047 of 2048 tokens with heavy duplication and ids outside the vocabulary, every gen_start
regime, both sides of the min-new-tokens boundary, empty / single / full EOS and bias lists, R = 1 and R = 4 with and without `last`, per-sequence
settings at B = 16, idle sequences next to active ones."""
import numpy as np
import pytest
import torch

import logits_process_ref as R
from quant import _native

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T_HIST = 2048
INF = float('inf')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)


def _launch(logits, hist, t_hist, last, lens, len_add, gen_start, rp, pp, mn, eos=(), bias=(), pad=None):
    """the C entry on host arrays: logits fp16 [B, R, vocab] (stored with an ODD leading dimension), hist int32 [B, ld_hist], last int64 [B, R] or
    None.  Returns (logits, hist, the padding columns) afterwards."""
    B, Rr, V = logits.shape
    ld = V if V % 2 else V + 1
    buf = torch.full((B * Rr * ld + 1,), 77.0, dtype=torch.float16)
    rows = buf[1:].view(B * Rr, ld)                          # starts at byte 2: row starts are 2-byte aligned and no more
    rows[:, :V] = torch.from_numpy(logits.reshape(B * Rr, V))
    buf = buf.to(DEV)
    rows = buf[1:].view(B * Rr, ld)
    dev = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt).to(DEV)
    h = dev(hist, torch.int32)
    la = None if last is None else dev(last, torch.int64).reshape(-1)
    ln, gs = dev(lens, torch.int64), dev(gen_start, torch.int64)
    rpt, ppt, mnt = dev(rp, torch.float32), dev(pp, torch.float32), dev(mn, torch.int32)
    eo = dev(list(eos), torch.int32) if len(eos) else None
    bi = dev([v for v, _ in bias], torch.int32) if len(bias) else None
    bv = dev([x for _, x in bias], torch.float32) if len(bias) else None
    p = _native.ptr
    rc = _native.lib().gptq_logits_process_f16(rows.data_ptr(), ld, B, Rr, V, h.data_ptr(), h.stride(0), t_hist, p(la), ln.data_ptr(), len_add,
                                               gs.data_ptr(), rpt.data_ptr(), ppt.data_ptr(), mnt.data_ptr(), p(eo), len(eos), p(bi), p(bv),
                                               len(bias), _native.stream_ptr(torch.device(DEV)))
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = rows.cpu().numpy()
    return out[:, :V].reshape(B, Rr, V).copy(), h.cpu().numpy(), out[:, V:]


def _history(rng, B, V, pool=40):
    """[B, T_HIST] ids drawn from a pool of `pool` tokens per sequence (heavy duplication), a few of them outside [0, V)"""
    hist = np.empty((B, T_HIST), dtype=np.int32)
    for b in range(B):
        ids = rng.choice(V, size=min(pool, V), replace=False)
        hist[b] = rng.choice(ids, size=T_HIST)
        hist[b, rng.choice(T_HIST, size=24, replace=False)] = rng.choice([-5, V, V + 7, 2 ** 31 - 1, -2 ** 31], size=24)
        hist[b, :3] = [-1, V, ids[0]]                        # (out-of-range ids inside the shortest histories too)
    return hist


def _check(name, got, want):
    (gl, gh, pad), (wl, wh) = got, want
    assert np.array_equal(gh, wh), (name, 'hist', np.argwhere(gh != wh)[:8])
    bad = np.argwhere(_bits(gl) != _bits(wl))
    assert bad.size == 0, (name, 'logits', bad[:8], _bits(gl)[tuple(bad[0])], _bits(wl)[tuple(bad[0])])
    assert (pad == 77.0).all(), (name, 'padding column written')


LENS = [0, 1, 63, 64, 65, 2047]


@pytest.mark.parametrize('with_last', [True, False], ids=['last', 'nolast'])
@pytest.mark.parametrize('rows', [1, 4])
@pytest.mark.parametrize('vocab', [33, 1000, 32000, 32001])
def test_kernel_matches_the_restatement_bit_for_bit(vocab, rows, with_last):
    rng = np.random.default_rng(vocab * 10 + rows * 2 + with_last)
    B = len(LENS)
    logits = R.realistic_logits(rng, (B, rows, vocab))
    hist = _history(rng, B, vocab)
    last = rng.integers(0, vocab, size=(B, rows)) if with_last else None
    if with_last:
        last[2, 0] = vocab + 3                               # an out-of-range token this step consumed: appended, not penalised
        last[3, -1] = hist[3, 5]
    gen_start = [0, 0, 30, 64, 70, 1000]                     # 0; the middle; about n; above n; the middle
    rp = [1.3, 1.18, 0.9, 1.3, 1.18, 1.3]
    pp = [0.5, 0.0, 0.25, -0.5, 1.5, 0.5]
    mn = [0, 3, 40, 2, 1, 1100]
    in_s = int(hist[5, 100])
    eos = [2, vocab - 1, vocab + 4]
    bias = [(1, -INF), (in_s if 0 <= in_s < vocab and in_s not in (1, vocab - 2) else 3, 2.5), (vocab, 1.0), (vocab - 2, -3.25)]
    args = (logits, hist, T_HIST, last, LENS, 0, gen_start, rp, pp, mn, eos, bias)
    got, want = _launch(*args), R.process(*args)
    _check('v%d R%d' % (vocab, rows), got, want)
    # what the launch may touch: S, the bias list, the EOS list -- and, with `last`, hist[b, n_b + i] of the active rows
    changed = (_bits(got[0]) != _bits(logits)).reshape(B, rows, vocab)
    for b in range(B):
        allowed = set(int(t) for t in hist[b, :LENS[b] + rows]) | set(eos) | set(v for v, _ in bias)
        if with_last:
            allowed |= set(int(t) for t in last[b])
        assert set(np.flatnonzero(changed[b].any(0)).tolist()) <= allowed, b
    assert changed[2:].any(), 'the penalties changed nothing'
    if with_last:
        assert got[1][0, 0] == last[0, 0] and got[1][4, 65 + rows - 1] == last[4, rows - 1] and got[1][2, 63] == vocab + 3
        assert got[1][5, 2047] == last[5, 0]                 # n = 2048 = t_hist: the last position the history can hold
        assert np.array_equal(_bits(got[0][5, 1:]), _bits(logits[5, 1:]))            # ... and rows 1 .. of that sequence idle
        assert (got[1] != hist).sum() <= B * rows
    else:
        assert np.array_equal(got[1], hist)
    again = _launch(*args)                                   # the same input, the same bits
    assert np.array_equal(_bits(again[0]), _bits(got[0])) and np.array_equal(again[1], got[1])


@pytest.mark.parametrize('n_eos,n_bias', [(0, 0), (1, 1), (8, 256)])
def test_eos_and_bias_lists_of_every_size(n_eos, n_bias):
    rng = np.random.default_rng(n_eos * 1000 + n_bias)
    V, B = 1000, 3
    logits = R.realistic_logits(rng, (B, 1, V))
    hist = _history(rng, B, V)
    lens, gen_start = [64, 200, 65], [60, 0, 65]
    eos = ([7, V + 1, 0, 999, 500, 501, 502, 31][:n_eos]) if n_eos != 1 else [int(hist[0, 10]) % V]
    ids = rng.choice(V, size=n_bias, replace=False).tolist()
    vals = (3.0 * rng.standard_normal(n_bias)).astype(np.float32).tolist()
    if n_bias:
        ids[0] = int(hist[1, 20]) if 0 <= hist[1, 20] < V and int(hist[1, 20]) not in ids else ids[0]          # an id that is also in S
        vals[-1] = -INF
    if n_bias == 256:
        ids[5], vals[5] = V + 9, 1.0                         # out of range: ignored
    args = (logits, hist, T_HIST, None, lens, 0, gen_start, [1.3, 1.18, 1.0], [0.5, 0.0, 0.0], [5, 0, 1], eos, list(zip(ids, vals)))
    got, want = _launch(*args), R.process(*args)
    _check('eos %d bias %d' % (n_eos, n_bias), got, want)
    if n_eos:                                                # sequences 0 and 2 are inside their min_new_tokens, sequence 1 has none
        assert got[0][0, 0, eos[0]] == -INF and got[0][2, 0, eos[0]] == -INF


@pytest.mark.parametrize('with_last', [True, False], ids=['last', 'nolast'])
def test_min_new_tokens_on_both_sides_of_the_boundary(with_last):
    rng = np.random.default_rng(5)
    V, m = 1000, 6
    # n - gen_start = m - 1 (masked), m (not), and the same one row later for R = 2: row 0 masked, row 1 not
    n0 = [40, 40, 40]
    gen_start = [40 - (m - 1), 40 - m, 40 - (m - 1)]
    lens = [n - 1 for n in n0] if with_last else n0
    logits = R.realistic_logits(rng, (3, 2, V))
    logits[:, :, 17] = 1.5
    hist = _history(rng, 3, V)
    last = rng.integers(0, V, size=(3, 2)) if with_last else None
    args = (logits, hist, T_HIST, last, lens, 0, gen_start, [1.0] * 3, [0.0] * 3, [m, m, m], [17], ())
    got, want = _launch(*args), R.process(*args)
    _check('min_new', got, want)
    assert (got[0][:, :, 17] == -INF).tolist() == [[True, False], [False, False], [True, False]]


def test_every_sequence_of_a_batch_equals_its_own_launch():
    rng = np.random.default_rng(16)
    B, Rr, V = 16, 2, 1000
    logits = R.realistic_logits(rng, (B, Rr, V))
    hist = _history(rng, B, V)
    last = rng.integers(0, V, size=(B, Rr))
    lens = rng.integers(1, 300, size=B).tolist()
    lens[3], lens[9], lens[12] = 0, T_HIST + 1, T_HIST       # len_add = -1: n_b = -1 idle; n_b = 2048 idle; n_b = 2047: row 0 active, row 1 idle
    gen_start = [int(rng.integers(0, l + 2)) for l in lens]
    rp = rng.choice([1.0, 0.9, 1.18, 1.3, 2.0], size=B).tolist()
    pp = rng.choice([0.0, 0.5, -0.25, 1.0], size=B).tolist()
    mn = rng.integers(0, 300, size=B).tolist()
    eos, bias = [3, 998], [(11, -INF), (12, 4.0), (int(hist[0, 7]) % V if int(hist[0, 7]) % V not in (11, 12) else 13, -1.0)]
    args = (logits, hist, T_HIST, last, lens, -1, gen_start, rp, pp, mn, eos, bias)
    got, want = _launch(*args), R.process(*args)
    _check('B16', got, want)
    for b in (3, 9):                                         # idle sequences next to active ones: logits and history bit for bit
        assert np.array_equal(_bits(got[0][b]), _bits(logits[b])) and np.array_equal(got[1][b], hist[b])
    assert got[1][12, 2047] == last[12, 0] and np.array_equal(_bits(got[0][12, 1]), _bits(logits[12, 1]))
    for b in (0, 5, 12, 15):
        one = _launch(logits[b:b + 1], hist[b:b + 1], T_HIST, last[b:b + 1], lens[b:b + 1], -1, gen_start[b:b + 1], rp[b:b + 1], pp[b:b + 1],
                      mn[b:b + 1], eos, bias)
        assert np.array_equal(_bits(one[0][0]), _bits(got[0][b])) and np.array_equal(one[1][0], got[1][b]), b


def test_neutral_settings_leave_the_row_unchanged():
    rng = np.random.default_rng(3)
    B, V = 2, 32001
    logits = R.realistic_logits(rng, (B, 1, V))
    hist = _history(rng, B, V)
    last = rng.integers(0, V, size=(B, 1))
    got = _launch(logits, hist, T_HIST, last, [500, 2047], 0, [10, 10], [1.0, 1.0], [0.0, 0.0], [0, 0], [2], ())
    assert np.array_equal(_bits(got[0]), _bits(logits))
    assert got[1][0, 500] == last[0, 0] and got[1][1, 2047] == last[1, 0] and (got[1] != hist).sum() <= 2          # the append still happens
