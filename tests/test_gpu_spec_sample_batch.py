"""GPU tests of gptq_spec_sample_batch_f16 (csrc/spec_sample.hip) through the C ABI: B sequences of R rows in one launch.  Every sequence is a
window of the 16-row case of spec_sample_ref.gpu_case (tests/spec_sample_batch_cases.py), whose margins tests/test_host_spec_sample_batch.py
asserts on the CPU -- so per sequence the accept flags must be the float64 oracle's exactly and the tokens admissible -- and per sequence the
records, out and pos must equal a call of gptq_spec_sample_rows_f16 on that sequence's rows bit for bit."""
import numpy as np
import pytest
import torch

import spec_sample_batch_cases as C
from quant import _native

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T_MAX = 4096
SENTINEL = -0x5A5A5A5A5A5A5A5


def _dev(values, dtype):
    return torch.tensor(values, dtype=dtype).to(DEV)


def _odd(t):
    """the rows of t in a buffer whose rows are 2-byte aligned only (an odd leading dimension, an odd offset), NaN between the rows"""
    R, V = t.shape
    ld = V + 1 if V % 2 == 0 else V + 2
    buf = torch.full((R * ld + 1,), float('nan'), dtype=torch.float16, device=DEV)
    view = buf[1:].view(R, ld)[:, :V]
    view.copy_(t.to(DEV))
    assert view.data_ptr() % 4 == 2 and (view.stride(0) * 2) % 4 == 2
    return view


class Batch:
    """the device arrays of one batch of windows, packed [B, R] as the entry wants them"""

    def __init__(self, ws_list, with_q, odd=True):
        self.w = ws_list
        self.B, self.R, self.V = len(ws_list), len(ws_list[0]['ids']), ws_list[0]['P'].shape[1]
        put = _odd if odd else (lambda t: t.to(DEV).contiguous())
        self.P = put(torch.cat([w['P'] for w in ws_list]))
        self.Q = put(torch.cat([w['Q'] for w in ws_list])) if with_q else None
        cat = lambda n: sum((list(w[n]) for w in ws_list), [])
        self.ids, self.T, self.k, self.p = _dev(cat('ids'), torch.int64), _dev(cat('T'), torch.float32), _dev(cat('k'), torch.int32), _dev(cat('p'), torch.float32)
        self.ua, self.ud = _dev(cat('ua'), torch.float32), _dev(cat('ud'), torch.float32)

    def run(self, pos, out=None, ws=None, seqs=None, override=None):
        """one launch of the batch entry; returns (rc, out [B, R + 1], pos [B], ws [B, R + 1]) -- the tensors it ran on"""
        lib = _native.lib()
        B, R = self.B if seqs is None else seqs, self.R
        pos = _dev(list(pos), torch.int64) if not torch.is_tensor(pos) else pos
        out = torch.full((B, R + 1), SENTINEL, dtype=torch.int64, device=DEV) if out is None else out
        ws = torch.zeros((B, R + 1), dtype=torch.int64, device=DEV) if ws is None else ws
        a = dict(P=self.P.data_ptr(), ld=self.P.stride(0), Q=self.Q.data_ptr() if self.Q is not None else None,
                 ldq=self.Q.stride(0) if self.Q is not None else 0, seqs=B, rows=R, vocab=self.V, ids=self.ids.data_ptr(), T=self.T.data_ptr(),
                 k=self.k.data_ptr(), p=self.p.data_ptr(), ua=self.ua.data_ptr(), ud=self.ud.data_ptr(), pos=pos.data_ptr(), tm=T_MAX,
                 out=out.data_ptr(), ws=ws.data_ptr(), wb=ws.numel() * 8)
        a.update(override or {})
        rc = lib.gptq_spec_sample_batch_f16(a['P'], a['ld'], a['Q'], a['ldq'], a['seqs'], a['rows'], a['vocab'], a['ids'], a['T'], a['k'], a['p'],
                                            a['ua'], a['ud'], a['pos'], a['tm'], a['out'], a['ws'], a['wb'], _native.stream_ptr(torch.device(DEV)))
        return rc, out, pos, ws

    def single(self, b, pos):
        """gptq_spec_sample_rows_f16 on sequence b's rows of the SAME buffers: (out [R + 1], pos, ws [R + 1]) as lists"""
        lib = _native.lib()
        R = self.R
        s = slice(b * R, b * R + R)
        pos = _dev([pos], torch.int64)
        out = torch.full((R + 1,), SENTINEL, dtype=torch.int64, device=DEV)
        ws = torch.zeros(R + 1, dtype=torch.int64, device=DEV)
        Q = self.Q[b * (R - 1):] if self.Q is not None else None
        rc = lib.gptq_spec_sample_rows_f16(self.P[s].data_ptr(), self.P.stride(0), Q.data_ptr() if Q is not None else None,
                                           Q.stride(0) if Q is not None else 0, R, self.V, self.ids[s].data_ptr(), self.T[s].data_ptr(),
                                           self.k[s].data_ptr(), self.p[s].data_ptr(), self.ua[s].data_ptr(), self.ud[s].data_ptr(), pos.data_ptr(),
                                           out.data_ptr(), ws.data_ptr(), ws.numel() * 8, _native.stream_ptr(torch.device(DEV)))
        assert rc == 0, rc
        return out.tolist(), int(pos[0]), ws.tolist()


def _check_sequence(bt, b, out, pos, ws, pos0):
    """sequence b of a batch result (lists) against the old entry, bit for bit, and against the oracle: flags exactly, tokens admissible"""
    R, V, w = bt.R, bt.V, bt.w[b]
    assert (out, pos, ws) == bt.single(b, pos0), b
    assert ws[0] == 0                                          # the ticket put itself back
    rec = np.array(ws[1:], dtype=np.int64)
    flags, tokens = (rec >> 32).astype(bool), (rec & 0xFFFFFFFF).astype(np.int64)
    a, emitted, want_flags, want_tokens = C.oracle(w)
    assert flags.tolist() == want_flags, (b, flags, want_flags)
    ok = C.admissible(w, flags, tokens)
    assert ok.all(), (b, np.nonzero(~ok)[0], tokens, want_tokens)
    assert ((tokens >= 0) & (tokens < V)).all()
    assert out[0] == a and out[1:a + 1] == list(w['ids'][1:a + 1]) and out[a + 1:] == [int(tokens[a])] * (R + 1 - a - 1)
    assert pos == pos0 + a + 1
    if tokens.tolist() == want_tokens:
        assert out[1:a + 2] == emitted
    return a


@pytest.mark.parametrize('with_q', [False, True], ids=['point', 'draft'])
@pytest.mark.parametrize('R', C.ROWS)
@pytest.mark.parametrize('V', C.VOCABS)
def test_sequences_against_the_single_entry_and_the_oracle(V, R, with_q):
    B = 3
    bt = Batch(C.batch(V, R, with_q, B), with_q)
    pos0 = [100, 0, T_MAX - 1]                                 # (the edges of the active range are active)
    rc, out, pos, ws = bt.run(pos0)
    assert rc == 0, rc
    out, pos, ws = out.tolist(), pos.tolist(), ws.tolist()
    accepted = [_check_sequence(bt, b, out[b], pos[b], ws[b], pos0[b]) for b in range(B)]
    print('V %d R %d %s: accepted %s' % (V, R, 'draft' if with_q else 'point', accepted))

    # sequences 0 and B - 1 idle: their out, pos and workspace words keep the sentinel, the active one's bits do not move
    for idle_pos in ([-1, 100, T_MAX], [-(T_MAX + 1), 100, 1 << 40]):
        o2 = torch.full((B, R + 1), SENTINEL, dtype=torch.int64, device=DEV)
        w2 = torch.full((B, R + 1), SENTINEL, dtype=torch.int64, device=DEV)
        w2[1].zero_()
        rc, o2, p2, w2 = bt.run(idle_pos, out=o2, ws=w2)
        assert rc == 0, rc
        o2, p2, w2 = o2.tolist(), p2.tolist(), w2.tolist()
        for b in (0, B - 1):
            assert o2[b] == [SENTINEL] * (R + 1) and w2[b] == [SENTINEL] * (R + 1) and p2[b] == idle_pos[b], b
        assert (o2[1], p2[1], w2[1]) == bt.single(1, 100)


@pytest.mark.parametrize('with_q', [False, True], ids=['point', 'draft'])
def test_sixteen_sequences_of_eight_rows(with_q):
    """128 workgroups, the engine's largest step; every other sequence idles in a second launch"""
    V, R, B = 257, 8, 16
    bt = Batch(C.batch(V, R, with_q, B), with_q)
    pos0 = [10 * b for b in range(B)]
    rc, out, pos, ws = bt.run(pos0)
    assert rc == 0, rc
    out, pos, ws = out.tolist(), pos.tolist(), ws.tolist()
    for b in range(B):
        _check_sequence(bt, b, out[b], pos[b], ws[b], pos0[b])
    half = [p if b % 2 else -1 for b, p in enumerate(pos0)]
    rc, o2, p2, w2 = bt.run(half)
    assert rc == 0, rc
    o2, p2, w2 = o2.tolist(), p2.tolist(), w2.tolist()
    for b in range(B):
        if b % 2:
            assert (o2[b], p2[b], w2[b]) == (out[b], pos[b], ws[b]), b
        else:
            assert o2[b] == [SENTINEL] * (R + 1) and p2[b] == -1 and w2[b] == [0] * (R + 1), b


def test_fifty_calls_on_one_workspace_with_a_changing_idle_pattern():
    V, R, B, CALLS = 257, 5, 3, 50
    bt = Batch(C.batch(V, R, True, B), True)
    ws = torch.zeros((B, R + 1), dtype=torch.int64, device=DEV)
    out = torch.full((B, R + 1), SENTINEL, dtype=torch.int64, device=DEV)
    seen, patterns = {}, []
    for n in range(CALLS):
        active = [bool((n + 1) >> b & 1) for b in range(B)]    # every pattern of the three, the all-idle one included (n = 7, 15, ..)
        pos0 = [100 if act else (-1 if n % 2 else T_MAX) for act in active]
        rc, out, pos, ws = bt.run(pos0, out=out, ws=ws)
        assert rc == 0, rc
        patterns.append((active, out.clone(), pos, ws.clone()))
    torch.cuda.synchronize()
    assert any(not any(p[0]) for p in patterns) and any(all(p[0]) for p in patterns)
    before = ([[SENTINEL] * (R + 1)] * B, [[0] * (R + 1)] * B)
    for active, o, p, w in patterns:
        o, p, w = o.tolist(), p.tolist(), w.tolist()
        assert all(active[b] or (o[b], w[b]) == (before[0][b], before[1][b]) for b in range(B))     # an idle call leaves out and the words alone
        before = (o, w)
        assert all(w[b][0] == 0 for b in range(B))             # every ticket word is back at 0 (or never left it)
        for b in range(B):
            if active[b]:
                got = (o[b], p[b], w[b])
                assert seen.setdefault(b, got) == got, b     # equal inputs, equal bits, whoever else ran
            else:
                assert p[b] in (-1, T_MAX)
    for b in range(B):
        assert seen[b] == bt.single(b, 100)


def test_a_sequence_does_not_depend_on_its_neighbours():
    V, R, B = 257, 5, 3
    for with_q in (False, True):
        bt = Batch(C.batch(V, R, with_q, B), with_q)
        rc, out, pos, ws = bt.run([100] * B)
        assert rc == 0, rc
        base = (out.tolist(), pos.tolist(), ws.tolist())
        g = torch.Generator().manual_seed(11)
        bt.P[R:2 * R].copy_((torch.randn(R, V, generator=g) * 3).half())      # new target logits for sequence 1, a NaN among them
        bt.P[R + 1, 5] = float('nan')
        if with_q:
            bt.Q[R - 1:2 * (R - 1)].copy_((torch.randn(R - 1, V, generator=g) * 3).half())
        rc, out, pos, ws = bt.run([100] * B)
        assert rc == 0, rc
        new = (out.tolist(), pos.tolist(), ws.tolist())
        for b in (0, 2):
            assert all(n[b] == o[b] for n, o in zip(new, base)), b
        assert new[2][1] != base[2][1]                          # (and sequence 1 itself did change: its records)


@pytest.mark.parametrize('with_q', [False, True], ids=['point', 'draft'])
def test_one_sequence_through_the_new_entry_is_the_old_entry(with_q):
    for V, R in ((50, 2), (32001, 5), (257, 8)):
        for o in C.offsets(R, 3):
            bt = Batch([C.window(V, R, with_q, o)], with_q)
            rc, out, pos, ws = bt.run([7])
            assert rc == 0, rc
            assert (out[0].tolist(), int(pos[0]), ws[0].tolist()) == bt.single(0, 7), (V, R, o)
    # the old entry has no idle rule: a negative position runs (the new one would idle there)
    got = bt.single(0, -5)
    assert got[1] == -5 + got[0][0] + 1 and got[0][0] >= 0
    rc, out, pos, ws = bt.run([-5])
    assert rc == 0 and out[0].tolist() == [SENTINEL] * (bt.R + 1) and int(pos[0]) == -5


def test_error_codes_on_device_pointers():
    V, R, B = 50, 5, 3
    bt = Batch(C.batch(V, R, True, B), True, odd=False)
    run = lambda **kw: bt.run([100] * B, override=kw)[0]
    assert run() == 0
    for name in ('P', 'ids', 'T', 'k', 'p', 'ua', 'ud', 'pos', 'out', 'ws'):
        assert run(**{name: None}) == -4, name                                            # GPTQ_E_NULL
    assert run(Q=None) == 0                                                               # (no draft logits is a mode, not an error)
    for bad in (dict(seqs=0), dict(seqs=65536), dict(rows=1), dict(vocab=0), dict(ld=V - 1), dict(ldq=V - 1), dict(tm=0)):
        assert run(**bad) == -2, bad                                                      # GPTQ_E_SHAPE
    assert run(wb=B * (R + 1) * 8 - 1) == -5                                              # GPTQ_E_WORKSPACE
    assert run(P=bt.P.data_ptr() + 1) == -3 and run(Q=bt.Q.data_ptr() + 1) == -3          # GPTQ_E_ALIGN
    t = torch.zeros(8, dtype=torch.int64, device=DEV)
    for name, off in (('T', 2), ('k', 2), ('p', 2), ('ua', 2), ('ud', 2), ('ids', 4), ('pos', 4), ('out', 4), ('ws', 4)):
        assert run(**{name: t.data_ptr() + off}) == -3, name
    lib = _native.lib()
    assert lib.gptq_spec_sample_batch_workspace_bytes(B, R) == B * lib.gptq_spec_sample_workspace_bytes(R) == 144
