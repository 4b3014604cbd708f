"""GPU tests of gptq_constrain_rows_f16 (csrc/constrain.hip) against the numpy restatement of its rules (tests/constrain_ref.py, pinned to
transformers' PrefixConstrainedLogitsProcessor by tests/test_host_constrain.py): BIT FOR BIT, logits and states, on logits at the scale an LM
head produces with NaN, +-inf and -0.0 planted in every row.  The shapes follow the kernel's geometry -- 1024 lanes, each holding 4 groups of
8 tokens in registers: lane i owns groups i, i + 1024, i + 2048, i + 3072, so one round covers 32 768 tokens and a larger vocabulary takes
further rounds from memory.  Vocabularies around the 8-element vector (1, 7, 8, 9); small ones in which only the first register group is live
(509, 512, 2049: a scalar head, a tail, both, neither); the production shape 32 000, whose last tokens lie in the fourth register group; 32 767,
32 768 and 32 777 around exactly one full round (from an offset base 32 777 is a head of 7, 4096 groups and a tail of 2; aligned, it is one
group of the second round and a tail of 1); 40 000 and 128 256 for the further rounds.  Every one with rows that are 16-byte aligned and with
rows that are 2-byte aligned only, whose class maps are aligned like their logits row in some rows and not in others (those go through the
scalar loop whole); 1 .. 16 384 classes (the LDS limit) with a padded table, 1 and 5 states, two class maps, 1, 3 and 16 rows, and every row
condition of the header next to ordinary rows."""
import numpy as np
import pytest
import torch

import constrain_ref as R
from quant import _native

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PAD = 77.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)


def _launch(logits, vocab, ld, off, nxt, n_states, n_classes, cls, ld_cls, map_of, state, last, lens, len_add, t_limit):
    """the C entry on host arrays.  logits fp16 [B, vocab] go into a buffer of rows of ld elements that starts `off` elements behind an aligned
    address, the class maps [n_maps, vocab] likewise (ld_cls); nxt int16 [rows, ld_next] as it is.  Returns (logits [B, vocab], state, whether
    anything outside the rows' first `vocab` elements was written)."""
    B = logits.shape[0]
    buf = torch.full((off + B * ld + 16,), PAD, dtype=torch.float16)
    buf[off:off + B * ld].view(B, ld)[:, :vocab] = torch.from_numpy(np.ascontiguousarray(logits))
    before = buf.clone()
    buf = buf.to(DEV)
    n_maps = cls.shape[0]
    cbuf = torch.full((off + n_maps * ld_cls + 16,), -9, dtype=torch.int16)
    cbuf[off:off + n_maps * ld_cls].view(n_maps, ld_cls)[:, :vocab] = torch.from_numpy(np.ascontiguousarray(cls))
    cbuf = cbuf.to(DEV)
    dev = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt).to(DEV)
    nx = torch.from_numpy(np.ascontiguousarray(nxt)).to(DEV)
    mp, st, ln = dev(map_of, torch.int32), dev(state, torch.int32), dev(lens, torch.int64)
    la = None if last is None else dev(last, torch.int64)
    rc = _native.lib().gptq_constrain_rows_f16(buf[off:].data_ptr(), ld, B, vocab, nx.data_ptr(), nx.stride(0), n_states, n_classes,
                                               cbuf[off:].data_ptr(), ld_cls, n_maps, mp.data_ptr(), st.data_ptr(), _native.ptr(la), ln.data_ptr(),
                                               len_add, t_limit, _native.stream_ptr(torch.device(DEV)))
    assert rc == 0, rc
    torch.cuda.synchronize()
    after = buf.cpu()
    inside = torch.zeros(after.shape, dtype=torch.bool)
    inside[off:off + B * ld].view(B, ld)[:, :vocab] = True
    stray = not torch.equal(after[~inside].view(torch.int16), before[~inside].view(torch.int16))
    return after[off:off + B * ld].view(B, ld)[:, :vocab].numpy().copy(), st.cpu().numpy(), stray


def _logits(rng, B, V):
    """sigma 3, and in every row NaN (a payload), +inf, -inf and -0.0 at random places"""
    x = (3.0 * rng.standard_normal((B, V))).astype(np.float16)
    for row in x.view(np.uint16):
        for bits in (0x7E01, 0xFE55, 0x7C00, 0xFC00, 0x8000):
            row[rng.integers(0, V, size=max(1, V // 64))] = bits
    return x


def _tables(rng, S, C, V, n_maps, ld_next):
    """random transitions with -1 on about a third, a few entries >= S (garbage: banned), classes with a few out of range; the padding
    columns C .. ld_next - 1 hold ALLOWED-looking entries, so a read past C would show"""
    nxt = rng.integers(0, S, size=(S + 2, ld_next)).astype(np.int16)            # (two rows behind n_states as well)
    live = nxt[:S, :C]
    live[rng.random(live.shape) < 0.35] = -1
    live[rng.random(live.shape) < 0.05] = S + 3
    live[rng.random(live.shape) < 0.02] = -5
    cls = rng.integers(0, C, size=(n_maps, V)).astype(np.int16)
    cls[:, rng.integers(0, V, size=max(1, V // 50))] = C                        # out of range on either side
    cls[:, rng.integers(0, V, size=max(1, V // 50))] = -7
    if V > 3:
        cls[:, -1], cls[:, 0] = C - 1, 0                                        # the last class and the first are in use
    return nxt, cls


def _run(name, rng, B, V, S, C, n_maps=2, aligned=True, ld_next=None, with_last=True, state=None, last=None, lens=None, t_limit=100, tables=None):
    ld_next = C + 5 if ld_next is None else ld_next
    nxt, cls = _tables(rng, S, C, V, n_maps, ld_next) if tables is None else tables
    logits = _logits(rng, B, V)
    map_of = np.arange(B) % n_maps
    state = rng.integers(0, S, size=B) if state is None else np.asarray(state)
    if last is None and with_last:
        last = rng.integers(0, V, size=B)
    lens = np.full(B, 5) if lens is None else np.asarray(lens)
    ld, ld_cls, off = (V, V, 0) if aligned else (V + 3, V + 3, 1)
    args = (nxt, S, C, cls)
    got = _launch(logits, V, ld, off, *args, ld_cls, map_of, state, last, lens, -1, t_limit)
    want_l, want_s = R.constrain_rows(logits, V, *args, map_of, state, last, lens, -1, t_limit)
    assert np.array_equal(got[1], want_s), (name, 'state', got[1], want_s)
    bad = np.argwhere(_bits(got[0]) != _bits(want_l))
    assert bad.size == 0, (name, 'logits', bad[:8], _bits(got[0])[tuple(bad[0])], _bits(want_l)[tuple(bad[0])])
    assert not got[2], (name, 'an element outside the rows was written')
    again = _launch(logits, V, ld, off, *args, ld_cls, map_of, state, last, lens, -1, t_limit)
    assert np.array_equal(_bits(again[0]), _bits(got[0])) and np.array_equal(again[1], got[1]), (name, 'a second launch differs')
    return logits, got, (nxt, cls, map_of, state, last)


@pytest.mark.parametrize('aligned', [True, False], ids=['ld=vocab', 'ld=vocab+3,offset'])
@pytest.mark.parametrize('vocab', [1, 7, 8, 9, 509, 512, 2049])
def test_vocabulary_sizes_and_row_strides(vocab, aligned):
    rng = np.random.default_rng(vocab * 2 + aligned)
    for with_last in (True, False):
        logits, got, (nxt, cls, map_of, state, last) = _run('V%d' % vocab, rng, 3, vocab, 5, 30, aligned=aligned, with_last=with_last)
        changed = (_bits(got[0]) != _bits(logits)).sum()
        print(vocab, aligned, with_last, 'state', state, '->', got[1], 'changed', changed)
        if not with_last:
            assert np.array_equal(got[1], state)
    if vocab >= 509:                                             # the mask acted, and left something: neither side is trivial
        assert 0 < changed < 3 * vocab


ROUND = 32768                                                    # tokens the kernel holds in registers: 1024 lanes x 4 groups x 8
GROUP = ROUND // 4                                               # ... and the tokens of one register group


@pytest.mark.parametrize('aligned', [True, False], ids=['ld=vocab', 'ld=vocab+3,offset'])
@pytest.mark.parametrize('vocab', [32000, 32767, 32768, 32777, 40000, 128256])
def test_every_register_group_and_further_rounds(vocab, aligned):
    """the vocabularies at which the fourth register group, exactly one full round and the rounds behind it are live.  Besides the random
    classes, class 0 is allowed and class 1 banned in every state, and they alternate over the first and the last 8 tokens (the scalar head
    and tail) and over 32 tokens around every boundary between two register groups and two rounds: an index slip there shows in a banned token
    that kept its bits or an allowed one that lost them."""
    rng = np.random.default_rng(vocab * 2 + aligned)
    S, C, B = 5, 30, 3
    nxt, cls = _tables(rng, S, C, vocab, 2, C + 5)
    nxt[:S, 0], nxt[:S, 1] = 1, -1
    cls[:, :8], cls[:, -8:] = [1, 0] * 4, [0, 1] * 4
    for k in range(GROUP, vocab - 8, GROUP):
        cls[:, k - 16:min(k + 16, vocab - 8)] = ([1, 0] * 16)[:min(k + 16, vocab - 8) - (k - 16)]
    for last in ([1, 1, 1], None):                               # token 1 is allowed everywhere: every row advances to state 1 and is masked
        logits, got, _ = _run('V%d' % vocab, rng, B, vocab, S, C, aligned=aligned, with_last=last is not None, state=[0, 3, 4], last=last,
                              tables=(nxt, cls))
        assert got[1].tolist() == ([1, 1, 1] if last else [0, 3, 4])
        out, was = _bits(got[0]), _bits(logits)
        assert (out[:, 0:8:2] == 0xFC00).all() and (out[:, -1:-8:-2] == 0xFC00).all()
        assert np.array_equal(out[:, 1:8:2], was[:, 1:8:2]) and np.array_equal(out[:, -2:-9:-2], was[:, -2:-9:-2])
        changed = out != was
        lo = 3 * GROUP + 16                                      # well inside the fourth register group, whatever the head
        assert changed[:, lo:min(vocab, ROUND)].any(axis=1).all() and not changed[:, lo:min(vocab, ROUND)].all(axis=1).any()
        for r in range(1, (vocab - 16) // ROUND + 1):            # ... and inside every further round
            part = changed[:, r * ROUND + 16:min(vocab, (r + 1) * ROUND)]
            assert part.any(axis=1).all() and not part.all(axis=1).any(), r
        print(vocab, aligned, last, 'changed', changed.sum(axis=1))


@pytest.mark.parametrize('classes', [1, 2, 300, 16384])
@pytest.mark.parametrize('states', [1, 5])
def test_classes_and_states(classes, states):
    rng = np.random.default_rng(classes + states)
    _run('C%d S%d' % (classes, states), rng, 3, 2049, states, classes)
    _run('C%d S%d nolast' % (classes, states), rng, 3, 2049, states, classes, with_last=False, aligned=False)
    if classes == 16384:                                         # every class in use at once: the whole staged row is read
        tables = _tables(rng, states, classes, 16400, 2, classes + 8)
        tables[1][0, :classes] = rng.permutation(classes)
        _run('C16384 all', rng, 2, 16400, states, classes, ld_next=classes + 8, tables=tables)


@pytest.mark.parametrize('batch', [1, 3, 16])
def test_batches_with_two_class_maps(batch):
    rng = np.random.default_rng(batch)
    _run('B%d' % batch, rng, batch, 509, 5, 300, n_maps=2)
    _run('B%d one map' % batch, rng, batch, 512, 5, 2, n_maps=1, aligned=False)


def _guaranteed_tables(rng, S, C, V):
    """tables in which class 0 is allowed everywhere (-> state 1 % S), class 1 banned everywhere, class 2 leads to a state >= S, and tokens 0,
    1, 2 have those classes; token 3 has a class >= C, token 4 a negative one"""
    nxt, cls = _tables(rng, S, C, V, 2, C + 5)
    nxt[:S, 0], nxt[:S, 1], nxt[:S, 2] = 1 % S, -1, S
    cls[:, :5] = [0, 1, 2, C + 9, -1]
    return nxt, cls


def test_row_conditions_next_to_ordinary_rows():
    rng = np.random.default_rng(11)
    S, C, V, B = 5, 40, 509, 16
    tables = _guaranteed_tables(rng, S, C, V)
    #        0   1   2  3  4  5  6  7  8        9   10      11 12 13 14 15
    state = [2, -1, -2, 3, 0, 1, 4, 2, 0,       3,  1,      S, 32767, 0, 4, 2]
    last = [0,   0,  0, 0, 0, 1, 2, 3, 4,      -1,  V, 2 ** 40, 0,    0, 0, 0]
    lens = [5,   5,  5, 0, 9, 5, 5, 5, 5,       5,  5,      5, 5,    8, 1, 5]
    # len_add -1, t_limit 7: row 3 idles below (n = -1), row 4 above (n = 8); row 13 (n = 7) and row 14 (n = 0) are the last that do not
    logits, got, _ = _run('rows', rng, B, V, S, C, state=state, last=last, lens=lens, t_limit=7, tables=tables)
    st = got[1].tolist()
    assert st[:5] == [1, -1, -2, 3, 0]                           # advanced; switched off twice; idle twice (not even the state moves)
    assert st[5:13] == [-2] * 8                                  # banned, a state >= S, two garbage classes, three garbage tokens, two garbage states
    assert st[13:] == [1, 1, 1]
    same = [bool(np.array_equal(_bits(got[0][b]), _bits(logits[b]))) for b in range(B)]
    assert same == [False] + [True] * 12 + [False] * 3, same     # every row but the ordinary ones keeps its bits
    # without `last`: nothing advances, and no state is written -- but a state outside the table still leaves
    logits, got, _ = _run('rows nolast', rng, B, V, S, C, state=state, with_last=False, lens=lens, t_limit=7, tables=tables)
    assert got[1].tolist() == state[:11] + [-2, -2] + state[13:]
    same = [bool(np.array_equal(_bits(got[0][b]), _bits(logits[b]))) for b in range(B)]
    assert same == [False, True, True, True, True] + [False] * 6 + [True, True] + [False] * 3, same


def test_allowed_special_values_keep_their_bits():
    rng = np.random.default_rng(13)
    S, C, V = 1, 2, 2049
    nxt = np.array([[0, -1]], dtype=np.int16)
    cls = (np.arange(V) % 3 == 0).astype(np.int16)[None]         # every third token is banned
    x = _logits(rng, 2, V)
    specials = [0x7E01, 0xFE55, 0x7C00, 0xFC00, 0x8000, 0x0000, 0x0001, 0xFBFF]
    x.view(np.uint16)[:, 1:1 + 3 * len(specials):3] = specials   # on allowed tokens
    x.view(np.uint16)[:, 0:3 * len(specials):3] = specials       # and on banned ones
    out, st, stray = _launch(x, V, V, 0, nxt, S, C, cls, V, [0, 0], [0, 0], None, [5, 5], -1, 100)
    ok = cls[0] == 0
    assert np.array_equal(_bits(out)[:, ok], _bits(x)[:, ok]) and (_bits(out)[:, ~ok] == 0xFC00).all() and not stray
    assert _bits(out)[0, 1:1 + 3 * len(specials):3].tolist() == specials
