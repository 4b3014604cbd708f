"""GPU tests of every place that computes the rotary embedding, each through the C ABI against the FLOAT64 rotation (tests/rope_cases.py:
exact_rope and the per-element bar assert_rope_close -- the judge tests/test_host_rope.py shows to reject a wrong base, position, sign,
pairing, batch row and fp16 trig), at three bases, at positions up to 4095 (32767 where there is no t_max), and at the head shapes that
reach every rope_kernel instance and every pass of its head loop.  Wherever the code promises bit-equality between two kernels it is
asserted as such.  No expectation here is produced by the project's own RoPE, except in those kernel-against-kernel comparisons.

Which rope_kernel instance a case launches (rope_launch, csrc/elementwise.hip): <8> when half % 8 == 0, the pointer is 16-byte aligned
and row_stride % 8 == 0 -- (2|32|33, 128), (3, 64), (5, 80); <2> when half % 2 == 0, pointer % 4 == 0, row_stride % 2 == 0 -- (4, 100)
(half = 50), and hd 128 at a pointer offset of 4 bytes; <1> otherwise -- (3, 10) (half = 5), and hd 128 at an offset of 2 bytes.

The share of outputs bit-equal to the faithful host oracle is PRINTED per kernel (and logged with GPTQ_TEST_ERRLOG): a measurement, not a
bar -- device and host expf may differ by an ulp, which at an angle of thousands of radians moves a result across an fp16 rounding
boundary.  Measured on the MI355X (share bit-equal to the oracle | worst err / bound of the judge):
    gptq_rope_f16, rope_kernel<8>   (2|32|33, 128), (3, 64), (5, 80)   99.54 .. 100 %   | 0.995 .. 0.999
    gptq_rope_f16, rope_kernel<2>   (4, 100); hd 128 at + 4 bytes      99.06 .. 99.98 % | 0.997 .. 0.998
    gptq_rope_f16, rope_kernel<1>   (3, 10); hd 128 at + 2 bytes       99.31 .. 100 %   | 0.992 .. 0.998
    gptq_decode_rope_kv_f16         positions 0 .. 4095                 99.83 .. 100 %   | 0.997 .. 0.998
    the fused decode / batch entries' K row, the prompt / chunk entries' K rows    99.84 .. 100 %   | 0.986 .. 0.997
    gptq_rope_table_f32             cos 0.43, sin 0.41 of its bound (the table holds fp32, no fp16 rounding)
Every bit-equality the code promises held: the three
rope_kernel instances, rope_kv against rope_kernel, every fused entry's cache rows against rope_kv, table against in-kernel trig.  The
attention outputs of the fused entries sit 2.4e-4 .. 8.6e-4 from float64 attention on exact_rope q and k (bar 1e-3).  At positions >= 2047 most of
that is the fp32 angle and not the attention kernels: the host oracle's rotation of the same qkv rows, put through the same float64
attention over a history of the same distribution, sits 1e-4 .. 8e-4 from it (1e-5 and less at positions <= 300)."""
import functools
import os

import numpy as np
import pytest
import torch

import quant
from quant import _native
from quant import decode as D
from oracle import oracle
from util import rel_err, within, TOL
import rope_cases as RC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
E_SHAPE, E_ALIGN = -2, -3          # GPTQ_E_SHAPE, GPTQ_E_ALIGN (include/gptq_mi355x.h)
NAN_BITS = 0x7E00                  # padding and guards: an fp16 NaN
HEADS, HD, T_MAX = 2, 128, 4096    # the decode-side entries (head_dim 128 only)
H = HEADS * HD
SCALE = float(1.0 / np.sqrt(HD))


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).to(DEV)


def _bits(t):
    return t.cpu().numpy().view(np.uint16)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _record(name, got, faithful, worst):
    """print (and log) the measured share of bit-equal outputs against the host oracle and the worst err / bound of the judge"""
    share = RC.bit_equal_share(got, faithful)
    print('%s: %.2f %% bit-equal to the host oracle, worst err/bound %.3f' % (name, 100.0 * share, worst))
    path = os.environ.get('GPTQ_TEST_ERRLOG')
    if path:
        with open(path, 'a') as f:
            f.write('%s_bit_equal_share %.4f (measured)\n' % (name, share))
    within(name + '_err_over_bound', worst, 1.0 + 1e-9)
    return share


def _oracle_rope(qkv, pos, base):
    """the faithful fp32 host restatement on a contiguous copy of qkv [bsz, seq, 3, heads, hd]"""
    ref = np.ascontiguousarray(qkv).copy()
    oracle.rope_(ref[:, :, :2], pos, base)
    return ref


# ---------------------------------------------------------------------------------------
# gptq_rope_f16 (rope_kernel<8|2|1>, csrc/elementwise.hip)
# ---------------------------------------------------------------------------------------
BSZ, SEQ = 3, 4
# every batch row at positions of its own (a kernel that takes row 0's would be caught on rows 1 and 2); all of RC.POSITIONS and RC.LONG_POSITIONS
OP_POS = np.array([[0, 1, 2, 17], [127, 128, 300, 2047], [4095, 8191, 32767, 5]], dtype=np.int64)
POS_LD = 8                         # the position_ids view is [3, 4] of a [3, 8] array: pos_batch_stride = 8 != seq
PAD = 8                            # halves of padding behind every row: row_stride = 3 heads hd + 8


def _padded(qkv, off=0):
    """qkv [bsz, seq, 3, heads, hd] laid out with PAD NaN halves behind every row, `off` halves into a flat NaN buffer (8 spare halves at
    the end).  Returns (flat uint16 host array, row stride)."""
    bsz, seq = qkv.shape[:2]
    W = int(np.prod(qkv.shape[2:]))
    ld = W + PAD
    flat = np.full(bsz * seq * ld + 8, NAN_BITS, dtype=np.uint16)
    rows = flat[off:off + bsz * seq * ld].reshape(bsz * seq, ld)
    rows[:, :W] = qkv.reshape(bsz * seq, W).view(np.uint16)
    return flat, ld


def _unpadded(flat, shape, off=0):
    bsz, seq = shape[:2]
    W = int(np.prod(shape[2:]))
    ld = W + PAD
    return np.ascontiguousarray(flat[off:off + bsz * seq * ld].reshape(bsz * seq, ld)[:, :W]).view(np.float16).reshape(shape)


def _check_untouched(flat_after, flat_before, shape, off=0):
    """everything but the q and k slots keeps its bits: the v slot, the padding of every row, the halves in front of and behind the rows"""
    bsz, seq, _, heads, hd = shape
    W, ld = 3 * heads * hd, 3 * heads * hd + PAD
    mask = np.ones(flat_before.shape, dtype=bool)
    rows = mask[off:off + bsz * seq * ld].reshape(bsz * seq, ld)
    rows[:, :2 * heads * hd] = False
    assert rows.shape == (bsz * seq, ld) and W + PAD == ld
    assert np.array_equal(flat_after[mask], flat_before[mask]), 'the v slot, the padding or a neighbour of the buffer was written'


def _rope_abi(buf, off, ld, pos_full, shape, base):
    bsz, seq, _, heads, hd = shape
    assert buf.data_ptr() % 16 == 0
    rc = _native.lib().gptq_rope_f16(buf.data_ptr() + 2 * off, ld, pos_full.data_ptr(), POS_LD, bsz, seq, heads, hd, float(base), _stream())
    torch.cuda.synchronize()
    return rc


def _pos_full():
    full = np.full((BSZ, POS_LD), 2 ** 40, dtype=np.int64)      # what lies behind the view would be loud
    full[:, :SEQ] = OP_POS
    return _dev(full)


@pytest.mark.parametrize('base', RC.BASES)
@pytest.mark.parametrize('heads,hd', RC.HEAD_SHAPES)
def test_rope_op_against_float64(heads, hd, base):
    shape = (BSZ, SEQ, 3, heads, hd)
    qkv = RC.qkv_inputs((BSZ, SEQ), heads, hd, 100 * heads + hd)
    flat, ld = _padded(qkv)
    pos_full = _pos_full()
    pos_view = pos_full[:, :SEQ]
    assert pos_view.stride(0) == POS_LD != SEQ
    # through the Python entry: a [bsz, seq, 2, heads, hd] view of rows wider than 3 heads hd
    buf = _dev(flat).view(torch.float16)
    rows = buf[:BSZ * SEQ * ld].view(BSZ, SEQ, ld)[:, :, :3 * heads * hd].view(BSZ, SEQ, 3, heads, hd)
    quant.fused_attn.hip_rotate_half_(rows[:, :, :2], pos_view, base)
    torch.cuda.synchronize()
    after = _bits(buf)
    _check_untouched(after, flat, shape)
    got = _unpadded(after, shape)
    worst = RC.assert_heads_close(got[:, :, :2], qkv[:, :, :2], OP_POS, hd, base, 'gptq_rope_f16 heads %d hd %d base %g' % (heads, hd, base))
    assert np.array_equal(got[0, 0].view(np.uint16), qkv[0, 0].view(np.uint16)), 'position 0 is not the identity'
    _record('rope_f16_h%d_hd%d_base%g' % (heads, hd, base), got[:, :, :2], _oracle_rope(qkv, OP_POS, base)[:, :, :2], worst)
    # ... and directly through the C ABI: the same bits
    buf2 = _dev(flat).view(torch.float16)
    assert _rope_abi(buf2, 0, ld, pos_full, shape, base) == 0
    assert np.array_equal(_bits(buf2), after)


@pytest.mark.parametrize('base', RC.BASES)
def test_rope_instances_agree_bit_for_bit(base):
    """hd 128 at a data pointer offset by 0, 4 and 2 bytes: rope_kernel<8>, <2> and <1> on the same values.  Their scalar arithmetic is the
    same, so are their bits; each is held to the judge, and nothing in front of, between or behind the rows is written."""
    heads, hd = 3, 128
    shape = (BSZ, SEQ, 3, heads, hd)
    qkv = RC.qkv_inputs((BSZ, SEQ), heads, hd, 31)
    pos_full = _pos_full()
    results = {}
    for vw, off in ((8, 0), (2, 2), (1, 1)):                     # offsets in halves
        flat, ld = _padded(qkv, off)
        assert ld % 8 == 0
        buf = _dev(flat).view(torch.float16)
        assert _rope_abi(buf, off, ld, pos_full, shape, base) == 0
        after = _bits(buf)
        _check_untouched(after, flat, shape, off)
        got = _unpadded(after, shape, off)
        worst = RC.assert_heads_close(got[:, :, :2], qkv[:, :, :2], OP_POS, hd, base, 'rope_kernel<%d> base %g' % (vw, base))
        _record('rope_kernel%d_base%g' % (vw, base), got[:, :, :2], _oracle_rope(qkv, OP_POS, base)[:, :, :2], worst)
        results[vw] = got
    assert np.array_equal(results[8].view(np.uint16), results[2].view(np.uint16)), '<8> and <2> differ'
    assert np.array_equal(results[8].view(np.uint16), results[1].view(np.uint16)), '<8> and <1> differ'


@pytest.mark.parametrize('base', (1e4, 5e5))
def test_rope_op_and_decode_rope_kv_agree_bit_for_bit(base):
    """heads 2, head_dim 128, t_max 64, positions 0, 1 and 63: the q and k rows gptq_rope_f16 rotates in place (rope_kernel<8>) against the q row
    gptq_decode_rope_kv_f16 rotates in place and the k row it appends to the cache -- both run the RoPE of csrc/attn_device.h under the same
    flags, so the bits are the same."""
    heads, hd, t_max = 2, 128, 64
    lib = _native.lib()
    for pos in (0, 1, 63):
        qkv = torch.from_numpy(RC.qkv_inputs((), heads, hd, 900 + pos)).to(DEV)                    # [3, heads, hd]
        p = torch.tensor([pos], dtype=torch.int64, device=DEV)
        op = qkv.clone()
        _native.check(lib.gptq_rope_f16(op.data_ptr(), 3 * heads * hd, p.data_ptr(), 1, 1, 1, heads, hd, float(base), _stream()), 'gptq_rope_f16')
        kv, kc, vc = qkv.clone(), torch.zeros((t_max, heads * hd), dtype=torch.float16, device=DEV), torch.zeros((t_max, heads * hd), dtype=torch.float16, device=DEV)
        _native.check(lib.gptq_decode_rope_kv_f16(kv.data_ptr(), p.data_ptr(), kc.data_ptr(), vc.data_ptr(), heads, hd, t_max, float(base), _stream()),
                      'gptq_decode_rope_kv_f16')
        torch.cuda.synchronize()
        assert torch.equal(op[0], kv[0]), 'q differs at position %d, base %g' % (pos, base)
        assert torch.equal(op[1].reshape(-1), kc[pos]), 'k differs at position %d, base %g' % (pos, base)
        assert torch.equal(op[2], qkv[2]) and torch.equal(vc[pos], qkv[2].reshape(-1)), 'v at position %d' % pos
        assert torch.equal(op[0], qkv[0]) == (pos == 0), 'position 0 is the identity, and only position 0'


def test_rope_op_refuses_a_half_beyond_256_columns():
    """hd 514: half = 257 is odd, so only the scalar instance could take it, and that serves half <= 256: GPTQ_E_SHAPE, nothing launched"""
    heads, hd = 1, 514
    shape = (BSZ, SEQ, 3, heads, hd)
    qkv = RC.qkv_inputs((BSZ, SEQ), heads, hd, 2)
    for off in (0, 1):
        flat, ld = _padded(qkv, off)
        buf = _dev(flat).view(torch.float16)
        assert _rope_abi(buf, off, ld, _pos_full(), shape, 1e4) == E_SHAPE
        assert np.array_equal(_bits(buf), flat)


# ---------------------------------------------------------------------------------------
# gptq_decode_rope_kv_f16 (rope_kv_kernel, csrc/decode_attn.hip)
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _history(qk_scale=1.0):
    """caches [T_MAX, H] fp16 (device; read-only: callers clone): keys 0.5 qk_scale N(0, 1), values N(0, 1)"""
    rng = np.random.default_rng(4096)
    kc = (rng.standard_normal((T_MAX, H)) * 0.5 * qk_scale).astype(np.float16)
    vc = rng.standard_normal((T_MAX, H)).astype(np.float16)
    return _dev(kc), _dev(vc)


def _rope_kv(qkv_row, pos, kc, vc, base):
    """one call on device tensors (qkv_row [3 H] rotated in place, the caches appended in place); pos a python int"""
    p = torch.tensor([pos], dtype=torch.int64, device=DEV)
    _native.check(_native.lib().gptq_decode_rope_kv_f16(qkv_row.data_ptr(), p.data_ptr(), kc.data_ptr(), vc.data_ptr(), HEADS, HD, T_MAX, float(base),
                                                        _stream()), 'gptq_decode_rope_kv_f16')
    torch.cuda.synchronize()
    assert int(p[0]) == pos


@pytest.mark.parametrize('base', RC.BASES)
def test_decode_rope_kv_against_float64(base):
    kc0, vc0 = _history()
    lib = _native.lib()
    qkv_all = RC.qkv_inputs((len(RC.POSITIONS),), HEADS, HD, 7)             # [P, 3, heads, hd]
    worst, got_all = 0.0, []
    for i, pos in enumerate(RC.POSITIONS):
        qkv = qkv_all[i]
        qd, kc, vc = _dev(qkv), kc0.clone(), vc0.clone()
        _rope_kv(qd, pos, kc, vc, base)
        got = qd.cpu().numpy()
        krow = kc[pos].cpu().numpy().reshape(HEADS, HD)
        p = np.array(pos)
        name = 'gptq_decode_rope_kv_f16 pos %d base %g' % (pos, base)
        worst = max(worst, RC.assert_heads_close(got[0], qkv[0], p, HD, base, name + ' q'), RC.assert_heads_close(krow, qkv[1], p, HD, base, name + ' k'))
        assert np.array_equal(got[1:].view(np.uint16), qkv[1:].view(np.uint16)), 'the k / v slots of qkv were written'
        assert np.array_equal(_bits(vc[pos]), qkv[2].reshape(-1).view(np.uint16)), 'the v row is not v'
        for c, c0 in ((kc, kc0), (vc, vc0)):
            assert torch.equal(c[:pos], c0[:pos]) and torch.equal(c[pos + 1:], c0[pos + 1:]), 'another cache row was written'
        if pos == 0:
            assert np.array_equal(got[0].view(np.uint16), qkv[0].view(np.uint16)) and np.array_equal(krow.view(np.uint16), qkv[1].view(np.uint16))
        # the q and k rows have the bits of gptq_rope_f16 on the same data (kernel against kernel: the promise "exactly like rope_kernel")
        od = _dev(qkv)
        pd = torch.tensor([pos], dtype=torch.int64, device=DEV)
        _native.check(lib.gptq_rope_f16(od.data_ptr(), 3 * H, pd.data_ptr(), 1, 1, 1, HEADS, HD, float(base), _stream()), 'gptq_rope_f16')
        torch.cuda.synchronize()
        op = od.cpu().numpy()
        assert np.array_equal(op[0].view(np.uint16), got[0].view(np.uint16)), 'q differs from gptq_rope_f16 at %d' % pos
        assert np.array_equal(op[1].view(np.uint16), krow.view(np.uint16)), 'k differs from gptq_rope_f16 at %d' % pos
        got_all.append(np.stack([got[0], krow]))
    ref = _oracle_rope(qkv_all[None], np.array([RC.POSITIONS], dtype=np.int64), base)[0, :, :2]
    _record('decode_rope_kv_base%g' % base, np.stack(got_all), ref, worst)


@pytest.mark.parametrize('pos', [-1, T_MAX, 2 ** 40])
def test_decode_rope_kv_position_outside_the_cache_writes_nothing(pos):
    kc0, vc0 = _history()
    qkv = RC.qkv_inputs((), HEADS, HD, 8)
    qd, kc, vc = _dev(qkv), kc0.clone(), vc0.clone()
    _rope_kv(qd, pos, kc, vc, 5e5)
    assert np.array_equal(_bits(qd), qkv.view(np.uint16)) and torch.equal(kc, kc0) and torch.equal(vc, vc0)


# ---------------------------------------------------------------------------------------
# gptq_rope_table_f32 (rope_table_kernel)
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table(base):
    tab = torch.full((T_MAX + 1, HD // 2, 2), float('nan'), dtype=torch.float32, device=DEV)     # (one guard row behind)
    _native.check(_native.lib().gptq_rope_table_f32(tab.data_ptr(), T_MAX, HD, float(base), _stream()), 'gptq_rope_table_f32')
    torch.cuda.synchronize()
    assert bool(torch.isnan(tab[T_MAX]).all()), 'the table kernel wrote behind t_max rows'
    return tab[:T_MAX]


@pytest.mark.parametrize('base', RC.BASES)
def test_rope_table_against_float64(base):
    """|cos - cos theta| and |sin - sin theta| <= rho_c theta + 2^-21 for every (pos < 4096, c < 64): the angle term of the bar with r = 1"""
    tab = _table(base).cpu().numpy().astype(np.float64)
    pos, c = np.arange(T_MAX)[:, None], np.arange(HD // 2)[None, :]
    t = RC.theta_of(pos, c, HD, base)
    rho = (4.0 * (2.0 * c * np.log(np.float64(np.float32(base))) / HD) + 3.0) * 2.0 ** -24
    bound = rho * t + 2.0 ** -21
    ec, es = np.abs(tab[:, :, 0] - np.cos(t)) / bound, np.abs(tab[:, :, 1] - np.sin(t)) / bound
    print('rope table base %g: worst err/bound cos %.3f sin %.3f' % (base, ec.max(), es.max()))
    assert ec.max() <= 1.0, (ec.max(), np.unravel_index(ec.argmax(), ec.shape))
    assert es.max() <= 1.0, (es.max(), np.unravel_index(es.argmax(), es.shape))
    assert np.array_equal(tab[0, :, 0], np.ones(HD // 2)) and not tab[0, :, 1].any()
    within('rope_table_base%g_err_over_bound' % base, max(ec.max(), es.max()), 1.0 + 1e-9)


def test_rope_table_argument_errors():
    lib = _native.lib()
    tab = torch.zeros((16, 64, 2), dtype=torch.float32, device=DEV)
    assert lib.gptq_rope_table_f32(tab.data_ptr(), 16, 64, 1e4, _stream()) == E_SHAPE
    assert lib.gptq_rope_table_f32(tab.data_ptr(), 16, 256, 1e4, _stream()) == E_SHAPE
    assert lib.gptq_rope_table_f32(tab.data_ptr() + 4, 15, 128, 1e4, _stream()) == E_ALIGN
    torch.cuda.synchronize()
    assert not bool(tab.any()), 'a refused call launched something'


# ---------------------------------------------------------------------------------------
# the fused consumers: the in-kernel rotation of attn_stream_kernel, prompt_rope_kv_kernel, chunk_rope_kv_kernel, with and without the table
# ---------------------------------------------------------------------------------------
ROWS = 5                           # rows of the prompt / chunk calls
QK_SCALE = 4.0                     # q and k scaled by 4: peaked logits, so the output depends visibly on how q was rotated
FUSED_BASES = (5e5, 1e6)           # (base 10000: tests/test_gpu_batch.py, test_gpu_prompt_attn.py, test_gpu_attn_chunk.py)
FUSED_POS = (1, 300, 2047, T_MAX - 1 - ROWS)


@functools.lru_cache(maxsize=None)
def _fused_inputs(p):
    """qkv [ROWS + 1, 3 H] fp16 with q and k scaled by QK_SCALE (read-only).  Rows 0 .. ROWS - 1: the chunk at positions p ..; row ROWS: the
    third sequence of the decode batch."""
    a = RC.qkv_inputs((ROWS + 1,), HEADS, HD, 500 + p).astype(np.float32)
    a[:, :2] *= QK_SCALE
    a = a.astype(np.float16).reshape(ROWS + 1, 3 * H)
    a.setflags(write=False)
    return a


def _exact_rows(qkv_rows, positions, base):
    """fp16(float64 rotation) of the q and k slots of qkv_rows [n, 3 H] at positions [n] -> q, k [n, heads, hd] fp16, v [n, H]"""
    a = qkv_rows.reshape(-1, 3, HEADS, HD)
    rot = RC.exact_rope_heads(a[:, :2], np.asarray(positions), HD, base).astype(np.float16)
    return rot[:, 0], rot[:, 1], qkv_rows[:, 2 * H:]


def _exact_chunk_attention(qkv_rows, p, base, kc_hist, vc_hist):
    """float64 causal attention of the rows at positions p .. p + n - 1 over [history below p | the rows' own keys], every q and k rotated by
    exact_rope (rounded to fp16 as the kernels store them), never by a kernel of the project -> [n, H]"""
    n = qkv_rows.shape[0]
    q, k, v = _exact_rows(qkv_rows, p + np.arange(n), base)
    K = np.concatenate([kc_hist[:p].reshape(p, HEADS, HD), k]).astype(np.float64)
    V = np.concatenate([vc_hist[:p].reshape(p, HEADS, HD), v.reshape(n, HEADS, HD)]).astype(np.float64)
    return np.stack([RC.exact_attention(q[r], K[:p + r + 1], V[:p + r + 1], SCALE).reshape(-1) for r in range(n)])


def _row_by_row(qkv_rows, p, base):
    """gptq_decode_rope_kv_f16 fed row by row (kernel against kernel: the caches every fused entry promises to reproduce bit for bit)"""
    kc0, vc0 = _history(QK_SCALE)
    kc, vc = kc0.clone(), vc0.clone()
    qd = _dev(qkv_rows)
    for r in range(qkv_rows.shape[0]):
        _rope_kv(qd[r], p + r, kc, vc, base)
    return kc, vc


def _check_appended_rows(kc, vc, qkv_rows, p, base, name):
    """the appended cache rows against the float64 rotation (the judge) and v"""
    n = qkv_rows.shape[0]
    a = qkv_rows.reshape(n, 3, HEADS, HD)
    got = kc[p:p + n].cpu().numpy().reshape(n, HEADS, HD)
    worst = RC.assert_heads_close(got, a[:, 1], p + np.arange(n), HD, base, name)
    assert np.array_equal(_bits(vc[p:p + n]), qkv_rows[:, 2 * H:].view(np.uint16)), name + ': v rows'
    return worst, got


def _attn_close(name, out, exact):
    out = np.asarray(out, dtype=np.float64)
    assert np.isfinite(out).all(), name
    err = rel_err(out, exact)
    print('%s: rel err %.3e against float64 attention with exact_rope q and k' % (name, err))
    within(name.replace(' ', '_'), err, TOL)


@pytest.mark.parametrize('p', FUSED_POS)
@pytest.mark.parametrize('base', FUSED_BASES)
def test_decode_entries_rotate_like_float64(base, p):
    """gptq_decode_attn_fused_f16, gptq_decode_attn_fused_table_f16 and gptq_decode_attn_batch_f16 (with and without the table; B = 3:
    positions p, idle, p + 3)"""
    lib = _native.lib()
    s = _stream()
    qkv = _fused_inputs(p)
    kc0, vc0 = _history(QK_SCALE)
    kh, vh = kc0.cpu().numpy(), vc0.cpu().numpy()
    tab = _table(base)
    ws_bytes = lib.gptq_decode_attn_workspace_bytes(HEADS, HD, T_MAX)
    pd = torch.tensor([p], dtype=torch.int64, device=DEV)
    kc_ref, vc_ref = _row_by_row(qkv[:1], p, base)
    exact = _exact_chunk_attention(qkv[:1], p, base, kh, vh)
    res = {}
    for table in (False, True):
        qd, kc, vc = _dev(qkv[:1]), kc0.clone(), vc0.clone()
        out = torch.full((1, H), float('nan'), dtype=torch.float16, device=DEV)
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
        if table:
            rc = lib.gptq_decode_attn_fused_table_f16(qd.data_ptr(), pd.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                      HEADS, HD, T_MAX, float(base), SCALE, tab.data_ptr(), s)
        else:
            rc = lib.gptq_decode_attn_fused_f16(qd.data_ptr(), pd.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                HEADS, HD, T_MAX, float(base), SCALE, s)
        _native.check(rc, 'gptq_decode_attn_fused%s_f16' % ('_table' if table else ''))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(qd), qkv[:1].view(np.uint16)), 'qkv was modified'
        assert torch.equal(kc, kc_ref) and torch.equal(vc, vc_ref), 'the appended row differs from gptq_decode_rope_kv_f16 (table %d)' % table
        res[table] = out.cpu().numpy()
    worst, krow = _check_appended_rows(kc, vc, qkv[:1], p, base, 'fused decode K row pos %d base %g' % (p, base))
    a = qkv[:1].reshape(1, 1, 3, HEADS, HD)
    _record('decode_attn_fused_k_pos%d_base%g' % (p, base), krow, _oracle_rope(a, np.array([[p]]), base)[0, :, 1], worst)
    assert np.array_equal(res[False].view(np.uint16), res[True].view(np.uint16)), 'table and in-kernel trig give different outputs'
    _attn_close('decode_attn_fused pos %d base %g' % (p, base), res[False], exact)

    # the batch entry: rows 0 and 2 active at p and p + 3 (qkv rows 0 and ROWS), row 1 idle
    B, pos = 3, [p, -1, p + 3]
    qb = np.stack([qkv[0], qkv[1], qkv[ROWS]])
    posd = torch.tensor(pos, dtype=torch.int64, device=DEV)
    wsb = lib.gptq_decode_attn_batch_workspace_bytes(B, HEADS, HD, T_MAX)
    ref2 = _row_by_row(qb[2:3], p + 3, base)
    exact2 = _exact_chunk_attention(qb[2:3], p + 3, base, kh, vh)
    resb = {}
    for table in (False, True):
        qd = _dev(qb)
        kb, vb = kc0[None].repeat(B, 1, 1), vc0[None].repeat(B, 1, 1)
        out = torch.full((B, H), float('nan'), dtype=torch.float16, device=DEV)
        ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
        rc = lib.gptq_decode_attn_batch_f16(qd.data_ptr(), 3 * H, posd.data_ptr(), kb.data_ptr(), vb.data_ptr(), out.data_ptr(), H, ws.data_ptr(), ws.numel(),
                                            B, HEADS, HD, T_MAX, float(base), SCALE, tab.data_ptr() if table else None, None, s)
        _native.check(rc, 'gptq_decode_attn_batch_f16')
        torch.cuda.synchronize()
        assert torch.equal(kb[0], kc_ref) and torch.equal(vb[0], vc_ref), 'batch row 0 (table %d)' % table
        assert torch.equal(kb[2], ref2[0]) and torch.equal(vb[2], ref2[1]), 'batch row 2 (table %d)' % table
        assert torch.equal(kb[1], kc0) and torch.equal(vb[1], vc0) and bool(torch.isnan(out[1]).all()), 'the idle row was touched'
        resb[table] = out.cpu().numpy()
    _check_appended_rows(kb[2], vb[2], qb[2:3], p + 3, base, 'batch decode K row pos %d base %g' % (p + 3, base))
    assert np.array_equal(resb[False][[0, 2]].view(np.uint16), resb[True][[0, 2]].view(np.uint16)), 'table and in-kernel trig give different outputs'
    _attn_close('decode_attn_batch row0 pos %d base %g' % (p, base), resb[False][0], exact[0])
    _attn_close('decode_attn_batch row2 pos %d base %g' % (p + 3, base), resb[False][2], exact2[0])


@pytest.mark.parametrize('p', FUSED_POS)
@pytest.mark.parametrize('base', FUSED_BASES)
def test_prompt_and_chunk_entries_rotate_like_float64(base, p):
    """gptq_prompt_attn_f16 (start a host value) and gptq_decode_attn_chunk_f16 (the position in device memory), ROWS rows at p .. p + ROWS - 1"""
    lib = _native.lib()
    s = _stream()
    qkv = _fused_inputs(p)[:ROWS]
    kc0, vc0 = _history(QK_SCALE)
    tab = _table(base)
    kc_ref, vc_ref = _row_by_row(qkv, p, base)
    exact = _exact_chunk_attention(qkv, p, base, kc0.cpu().numpy(), vc0.cpu().numpy())
    pd = torch.tensor([p], dtype=torch.int64, device=DEV)
    ws_p = torch.empty(lib.gptq_prompt_attn_workspace_bytes(ROWS, HEADS, HD, T_MAX), dtype=torch.uint8, device=DEV)
    ws_c = torch.empty(lib.gptq_decode_attn_chunk_workspace_bytes(ROWS, HEADS, HD, T_MAX), dtype=torch.uint8, device=DEV)
    assert ws_p.numel() > 0 and ws_c.numel() > 0
    outs = {}
    for entry in ('prompt', 'chunk'):
        for table in (False, True):
            qd, kc, vc = _dev(qkv), kc0.clone(), vc0.clone()
            out = torch.full((ROWS, H), float('nan'), dtype=torch.float16, device=DEV)
            t = tab.data_ptr() if table else None
            if entry == 'prompt':
                rc = lib.gptq_prompt_attn_f16(qd.data_ptr(), 3 * H, ROWS, p, kc.data_ptr(), vc.data_ptr(), out.data_ptr(), H, ws_p.data_ptr(), ws_p.numel(),
                                              HEADS, HD, T_MAX, float(base), SCALE, t, s)
            else:
                rc = lib.gptq_decode_attn_chunk_f16(qd.data_ptr(), 3 * H, ROWS, pd.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), H,
                                                    ws_c.data_ptr(), ws_c.numel(), HEADS, HD, T_MAX, float(base), SCALE, t, s)
            _native.check(rc, entry)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(qd), qkv.view(np.uint16)), 'qkv was modified'
            assert torch.equal(kc, kc_ref) and torch.equal(vc, vc_ref), '%s (table %d): the cache differs from gptq_decode_rope_kv_f16 fed row by row' % (entry, table)
            outs[entry, table] = out.cpu().numpy()
        assert np.array_equal(outs[entry, False].view(np.uint16), outs[entry, True].view(np.uint16)), entry + ': table and in-kernel trig give different outputs'
        _attn_close('%s_attn pos %d base %g' % (entry, p, base), outs[entry, False], exact)
    worst, krows = _check_appended_rows(kc, vc, qkv, p, base, 'prompt / chunk K rows pos %d base %g' % (p, base))
    a = qkv.reshape(1, ROWS, 3, HEADS, HD)
    _record('prompt_chunk_k_pos%d_base%g' % (p, base), krows, _oracle_rope(a, p + np.arange(ROWS)[None], base)[0, :, 1], worst)


# ---------------------------------------------------------------------------------------
# the engine: rope_theta reaches every regime, and the table is the one of that base
# ---------------------------------------------------------------------------------------
def test_engine_uses_the_models_rope_theta():
    from test_gpu_model import ENGINE_TOL, HD128, run_steps
    theta = 500000.0
    model = D.build_random_llama(DEV, seed=3, rope_theta=theta, **HD128)
    attns = [layer.self_attn for layer in model.model.layers]
    assert len(attns) == 2 and all(isinstance(a, quant.fused_attn.QuantLlamaAttention) and a.rope_theta == theta for a in attns)
    n, T, R = 20, 9, 4
    ids = torch.randint(0, HD128['vocab_size'], (1, n), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    expect = run_steps(model, ids, 1)[:, 0]                    # [n, vocab]: the module chain token by token
    expect_p = run_steps(model, ids, T)[:, 0]                  # [1 + n - T, vocab]: ... after a prompt of T tokens
    mx = np.abs(expect).max()

    def decode_all(eng, start=0):
        return np.stack([eng.decode(ids[0, i]).float().cpu().numpy()[0] for i in range(start, n)])
    got = {}
    for graph in (False, True):
        eng = D.DecodeEngine(model, t_max=64)
        assert all(L['theta'] == theta for L in eng.layers)
        if graph:
            eng.capture()
        got[graph] = decode_all(eng)
        within('rope_engine_decode_g%d' % graph, np.abs(got[graph] - expect).max() / mx, ENGINE_TOL)
        assert sorted(eng._rope_tabs) in ([theta], [])
    eng = D.DecodeEngine(model, t_max=64, chunk=R)
    first = eng.prefill(ids[0, :T], start=0).float().cpu().numpy().reshape(1, -1)
    rows = eng.verify(ids[0, T:T + R]).float().cpu().numpy()
    within('rope_engine_prefill', np.abs(first - expect_p[:1]).max() / mx, ENGINE_TOL)
    within('rope_engine_chunk', np.abs(rows - expect_p[1:1 + R]).max() / mx, ENGINE_TOL)
    eng.accept(R)
    rest = decode_all(eng, T + R)
    within('rope_engine_decode_after_chunk', np.abs(rest - expect_p[1 + R:]).max() / mx, ENGINE_TOL)
    # the same model object at the default base: another table, other logits -- by far more than the bar, or theta never reached a kernel
    try:
        for a in attns:
            a.rope_theta = 10000.0
        eng = D.DecodeEngine(model, t_max=64).capture()
        assert all(L['theta'] == 10000.0 for L in eng.layers)
        other = decode_all(eng)
    finally:
        for a in attns:
            a.rope_theta = theta
    assert np.abs(other[0] - got[True][0]).max() / mx < ENGINE_TOL      # position 0: no rotation, the same logits
    d = np.abs(other - got[True]).max() / mx
    print('engine at theta 1e4 against theta 5e5: %.3e of the largest logit (bar %.1e)' % (d, ENGINE_TOL))
    assert d > 10 * ENGINE_TOL, d
