"""GPU tests of gptq_decode_attn_chunk_batch_f16 (csrc/chunk_attn.hip) through the C ABI: the chunk attention of tests/test_gpu_attn_chunk.py for
several sequences in the same two launches -- packed rows, one cache slot and one DEVICE position per sequence.  Method and constants of that file
(HEADS 3, T_MAX 1930, guard rows, NaN behind every chunk, the workspace filled with 0xA5; its helpers are imported, not copied), with guard rows
BETWEEN the slots as well (slot_stride > T_MAX * H).  The reference per sequence is the single-sequence entry on a copy of that slot: cache slots
and output rows must be bit-identical to it, and every sequence meets float64 under the op-level bar TOL."""
import numpy as np
import pytest
import torch

import test_gpu_attn_chunk as single
from quant import _native
from test_gpu_attn_chunk import BASE, DEV, GUARD, GUARD_BITS, H, HD, HEADS, NAN_BITS, SCALE, T_MAX
from util import rel_err, TOL

pytestmark = pytest.mark.gpu
SLOT_GUARD = 48                          # guard rows behind every slot: slot_stride = (T_MAX + SLOT_GUARD) * H
SLOT_ROWS = T_MAX + SLOT_GUARD
ROWS = 5


class Seq:
    """one sequence of a call: `p` is the position the call sees, `inputs` (p, rows) names the shared read-only inputs of test_gpu_attn_chunk
    (history below that p, NaN from p + rows on); extra > 0 appends that many random rows to qkv (rows that will not fit the slot)"""

    def __init__(self, p, inputs=None, extra=0, seed=0):
        self.p = p
        self.inputs = inputs if inputs is not None else (p, ROWS)
        qkv, self.kc, self.vc = single._inputs(*self.inputs)
        if extra:
            qkv = np.concatenate([qkv, np.random.default_rng(800 + seed).standard_normal((extra, 3 * H)).astype(np.float16)])
        self.qkv = qkv
        self.rows = qkv.shape[0]


def _workspace(seqs, rows):
    n = _native.lib().gptq_decode_attn_chunk_batch_workspace_bytes(seqs, rows, HEADS, HD, T_MAX)
    assert n > 0
    return torch.empty(n, dtype=torch.uint8, device=DEV).fill_(0xA5)       # pure scratch: no initialisation asked


def _slots(arrays):
    """the sequences' [T_MAX][H] caches as slots of ONE allocation: GUARD rows in front, SLOT_GUARD guard rows behind every slot, GUARD behind"""
    full = np.full((GUARD + len(arrays) * SLOT_ROWS + GUARD, H), GUARD_BITS, dtype=np.uint16)
    for b, a in enumerate(arrays):
        full[GUARD + b * SLOT_ROWS:GUARD + b * SLOT_ROWS + T_MAX] = a.view(np.uint16)
    return single._dev(full).view(torch.float16)


def _run(seqs, table=False, ldq=3 * H, ldo=H, ws=None):
    """one call on guarded allocations; returns the raw allocations as uint16 arrays on the host"""
    lib = _native.lib()
    B, rows = len(seqs), seqs[0].rows
    assert all(q.rows == rows for q in seqs)
    qf = np.full((B * rows, ldq), NAN_BITS, dtype=np.uint16)
    for b, q in enumerate(seqs):
        qf[b * rows:(b + 1) * rows, :3 * H] = q.qkv.view(np.uint16)
    qd = single._dev(qf).view(torch.float16)
    kd, vd = _slots([q.kc for q in seqs]), _slots([q.vc for q in seqs])
    od = single._guarded(np.full((B * rows, H), NAN_BITS, dtype=np.uint16).view(np.float16), cols=ldo)
    positions = [q.p for q in seqs]
    pos = torch.tensor(positions, dtype=torch.int64, device=DEV)
    ws = _workspace(B, rows) if ws is None else ws
    rc = lib.gptq_decode_attn_chunk_batch_f16(qd.data_ptr(), ldq, B, rows, pos.data_ptr(), kd[GUARD:].data_ptr(), vd[GUARD:].data_ptr(), SLOT_ROWS * H,
                                              od[GUARD:].data_ptr(), ldo, ws.data_ptr(), ws.numel(), HEADS, HD, T_MAX, BASE, SCALE,
                                              _native.ptr(single._rope_table() if table else None), torch.cuda.current_stream().cuda_stream)
    _native.check(rc, 'gptq_decode_attn_chunk_batch_f16')
    torch.cuda.synchronize()
    assert pos.tolist() == positions
    return dict(qkv=single._bits(qd), qkv_in=qf, kc=single._bits(kd), vc=single._bits(vd), out=single._bits(od), B=B, rows=rows)


def _slot(res, name, b):
    return res[name][GUARD + b * SLOT_ROWS:GUARD + b * SLOT_ROWS + T_MAX]


def _out(res, b):
    return res['out'][GUARD + b * res['rows']:GUARD + (b + 1) * res['rows'], :H]


def _check_guards(res):
    B, rows = res['B'], res['rows']
    for name in ('kc', 'vc'):
        a = res[name]
        assert (a[:GUARD] == GUARD_BITS).all() and (a[GUARD + B * SLOT_ROWS:] == GUARD_BITS).all(), name + ' guard rows written'
        for b in range(B):
            assert (a[GUARD + b * SLOT_ROWS + T_MAX:GUARD + (b + 1) * SLOT_ROWS] == GUARD_BITS).all(), '%s: guard rows behind slot %d written' % (name, b)
    o = res['out']
    assert (o[:GUARD] == GUARD_BITS).all() and (o[GUARD + B * rows:] == GUARD_BITS).all(), 'out guard rows written'
    assert (o[GUARD:GUARD + B * rows, H:] == NAN_BITS).all(), 'padding of the output rows written'
    assert np.array_equal(res['qkv'], res['qkv_in']), 'qkv was modified'


def _check_against_the_single_entry(res, seqs):
    """slot b and output rows b of the batch call: the bits a single-sequence call leaves on a copy of that slot (idle, skipped rows and NaN rows
    behind the chunk included: the single entry leaves them alone, so equality says the batch entry does too)"""
    for b, q in enumerate(seqs):
        ref = single._run(q.p, q.rows, q.qkv, q.kc, q.vc)
        assert np.array_equal(_slot(res, 'kc', b), ref['kc'][GUARD:GUARD + T_MAX]), 'k slot %d differs from the single-sequence entry' % b
        assert np.array_equal(_slot(res, 'vc', b), ref['vc'][GUARD:GUARD + T_MAX]), 'v slot %d differs from the single-sequence entry' % b
        assert np.array_equal(_out(res, b), ref['out'][GUARD:GUARD + q.rows, :H]), 'output rows of sequence %d differ from the single-sequence entry' % b


def _check_float64(res, seqs):
    """every served row against float64 on the fp16 values; rows beyond the chunk stay NaN in the cache, idle and skipped rows NaN in the output"""
    for b, q in enumerate(seqs):
        out = _out(res, b).view(np.float16)
        if not 0 <= q.p < T_MAX:                                 # idle: slot and output rows unchanged bit for bit
            assert np.array_equal(_slot(res, 'kc', b), q.kc.view(np.uint16)) and np.array_equal(_slot(res, 'vc', b), q.vc.view(np.uint16))
            assert (out.view(np.uint16) == NAN_BITS).all()
            continue
        fit = min(q.rows, T_MAX - q.p)
        assert (q.p, fit) == q.inputs, 'the shared reference belongs to another position'
        kc_ref, vc_ref, exact = single._reference(q.p, fit)
        assert np.array_equal(_slot(res, 'kc', b), kc_ref.view(np.uint16)) and np.array_equal(_slot(res, 'vc', b), vc_ref.view(np.uint16))
        assert (_slot(res, 'kc', b)[q.p + fit:] == NAN_BITS).all() and (_slot(res, 'vc', b)[q.p + fit:] == NAN_BITS).all()
        assert (out[fit:].view(np.uint16) == NAN_BITS).all(), 'a skipped row of sequence %d was written' % b
        assert np.isfinite(out[:fit].astype(np.float32)).all()
        err = rel_err(out[:fit], exact)
        print('sequence %d (p %d, %d of %d rows): rel err %.3e' % (b, q.p, fit, q.rows, err))
        assert err < TOL, (b, err)


def _check_everything(seqs):
    res = _run(seqs)
    _check_guards(res)
    _check_against_the_single_entry(res, seqs)
    _check_float64(res, seqs)
    # the table variant, and a second call on the SAME (now used) workspace: the same bits
    res_t = _run(seqs, table=True)
    ws = _workspace(len(seqs), seqs[0].rows)
    first, second = _run(seqs, ws=ws), _run(seqs, ws=ws)
    for name in ('out', 'kc', 'vc'):
        assert np.array_equal(res_t[name], res[name]), 'table variant differs in ' + name
        assert np.array_equal(first[name], res[name]) and np.array_equal(second[name], res[name]), 'a second call on the workspace differs in ' + name
    return res


def _mixed4():
    """one split, the most splits the rule chooses at T_MAX, the last position at which every row fits, and an idle sequence"""
    sp = single._split_positions(ROWS)
    assert min(sp) == 1 and max(sp) == _native.lib().gptq_decode_attn_chunk_splits(HEADS, HD, T_MAX, T_MAX)
    return [Seq(sp[1]), Seq(sp[max(sp)]), Seq(T_MAX - ROWS), Seq(-1, inputs=(200, ROWS))]


def test_four_sequences_one_split_most_splits_end_of_slot_and_idle():
    _check_everything(_mixed4())


def test_rows_that_do_not_fit_the_slot():
    """one of three sequences at T_MAX - 2 with 5 rows: its two fitting rows are served, three are skipped, nothing leaves the slot"""
    sp = single._split_positions(ROWS)
    seqs = [Seq(40), Seq(T_MAX - 2, inputs=(T_MAX - 2, 2), extra=ROWS - 2, seed=1), Seq(sp[2])]
    res = _check_everything(seqs)
    assert (_out(res, 1)[2:] == NAN_BITS).all() and not (_out(res, 1)[:2] == NAN_BITS).any()


def test_sixteen_sequences_of_eight_rows():
    """the 128-row limit at short mixed positions: tile edges (31 / 32 / 33), the split rule's tile (127 / 128 / 129), position 0"""
    seqs = [Seq(p, inputs=(p, 8)) for p in (0, 1, 2, 3, 5, 17, 31, 32, 33, 64, 100, 127, 128, 129, 200, 255)]
    _check_everything(seqs)


def test_one_sequence_is_the_single_entry():
    sp = single._split_positions(ROWS)
    for p in (sp[1], sp[max(sp)]):
        _check_everything([Seq(p)])


def test_positions_beyond_the_slot_idle():
    """no access outside a slot for any position value: T_MAX, beyond 2^31 and 2^40 idle like a negative one, next to a sequence that is served"""
    seqs = [Seq(T_MAX, inputs=(200, ROWS)), Seq(2 ** 31 + 5, inputs=(129, ROWS)), Seq(7), Seq(2 ** 40, inputs=(1, ROWS)),
            Seq(-2 ** 40, inputs=(127, ROWS))]
    _check_everything(seqs)


def test_strided_rows():
    seqs = _mixed4()
    base = _run(seqs)
    res = _run(seqs, ldq=3 * H + 64, ldo=H + 32)
    _check_guards(res)                                           # (the NaN padding of qkv and out rows included)
    for b in range(len(seqs)):
        assert np.array_equal(_out(res, b), _out(base, b))
    assert np.array_equal(res['kc'], base['kc']) and np.array_equal(res['vc'], base['vc'])


def test_neighbours_do_not_reach_a_sequence():
    """every other sequence gets other inputs and another position (another split count, idle, beyond the slot): sequence 0's bits do not move"""
    sp = single._split_positions(ROWS)
    first = Seq(sp[3])
    a = _run([first, Seq(sp[2]), Seq(129), Seq(sp[max(sp)])])
    b = _run([first, Seq(-1, inputs=(200, ROWS)), Seq(sp[max(sp)]), Seq(T_MAX - ROWS)])
    for name in ('kc', 'vc'):
        assert np.array_equal(_slot(a, name, 0), _slot(b, name, 0)), name
        assert not np.array_equal(_slot(a, name, 2), _slot(b, name, 2))
    assert np.array_equal(_out(a, 0), _out(b, 0))
    assert not (_out(a, 0) == NAN_BITS).any()
