"""The RoPE cases of tests/rope_cases.py, checked on the references alone (CPU): the faithful fp32 oracle and the reference kernel's own
goldens must sit inside the per-element bar (a condition on the BAR: a reference outside it would mean the derivation is wrong), and
each plausible wrong formula, rounded to fp16, must be rejected by the same judge the GPU tests use -- which is what shows that those
tests can see the base, the position, the pairing and the column."""
import numpy as np
import pytest

from oracle import oracle
from util import golden_names, load_golden
import rope_cases as RC

ALL_POS = RC.POSITIONS + RC.LONG_POSITIONS


def _rows(heads, hd, seed, positions=ALL_POS):
    """qkv [1, P, 3, heads, hd] with one row per position"""
    pos = np.array([positions], dtype=np.int64)
    return RC.qkv_inputs((1, len(positions)), heads, hd, seed), pos


@pytest.mark.parametrize('base', RC.BASES)
@pytest.mark.parametrize('heads,hd', RC.HEAD_SHAPES)
def test_oracle_is_inside_the_bar(heads, hd, base):
    qkv, pos = _rows(heads, hd, 1000 * heads + hd)
    got = qkv.copy()
    oracle.rope_(got[:, :, :2], pos, base)
    worst = RC.assert_heads_close(got[:, :, :2], qkv[:, :, :2], pos, hd, base, 'oracle hd %d base %g' % (hd, base))
    print('oracle heads %d hd %d base %g: worst err/bound %.3f' % (heads, hd, base, worst))
    assert np.array_equal(got[:, :, 2].view(np.uint16), qkv[:, :, 2].view(np.uint16))
    # position 0 is the identity, to the bit
    assert pos[0, 0] == 0 and np.array_equal(got[0, 0].view(np.uint16), qkv[0, 0].view(np.uint16))


def test_oracle_with_batch_rows_at_their_own_positions():
    pos = np.array([[0, 1, 2, 3], [300, 301, 302, 303], [4000, 4001, 4002, 4003]], dtype=np.int64)
    qkv = RC.qkv_inputs((3, 4), 2, 128, 5)
    got = qkv.copy()
    oracle.rope_(got[:, :, :2], pos, 5e5)
    RC.assert_heads_close(got[:, :, :2], qkv[:, :, :2], pos, 128, 5e5, 'oracle batch')


@pytest.mark.parametrize('name', golden_names('rope_'))
def test_reference_goldens_are_inside_the_bar(name):
    """the reference kernel's own output (base 10000): hd 128 at position 17, hd 64 at 0 .. 10, hd 32 at 2000 .. 2002"""
    f = load_golden(name)
    hd = f['qkv_in'].shape[-1]
    worst = RC.assert_heads_close(f['qkv_out'][:, :, :2], f['qkv_in'][:, :, :2], f['pos'], hd, 10000.0, name)
    print('%s: hd %d, worst err/bound %.3f' % (name, hd, worst))
    assert np.array_equal(f['qkv_out'][:, :, 2].view(np.uint16), f['qkv_in'][:, :, 2].view(np.uint16))


def _rejected(f, qk, pos, hd, base):
    """the wrong formula's fp16 result must fail the judge; returns (share beyond the bar, share beyond 10 x the bar)"""
    wrong = f(qk, pos, hd, base).astype(np.float16)
    with pytest.raises(AssertionError):
        RC.assert_heads_close(wrong, qk, pos, hd, base, f.__name__)
    return RC.share_beyond(wrong, qk, pos, hd, base), RC.share_beyond(wrong, qk, pos, hd, base, 10.0)


def _accepted(f, qk, pos, hd, base):
    RC.assert_heads_close(f(qk, pos, hd, base).astype(np.float16), qk, pos, hd, base, f.__name__)


# What hides each formula (kept here because the GPU cases are chosen around it):
#   every formula       position 0: the rotation is the identity whatever the frequency (pos + 1 and the pairing excepted: see below)
#   exponent c / hd     column 0 (both exponents are 0)
#   sine sign flipped   position 0 only; from 2047 on every element is off
#   pos + 1             nothing at the positions used; at position 0 it is the only formula that shows
#   base ignored        base 10000 itself -- the only base the suite used before -- and column 0 (frequency 1 for every base)
#   interleaved pairs   nothing but position 0
#   row 0's position    batches of one row, and rows that share row 0's positions (a [bsz, seq] batch whose rows all start at 0)
#   fp16 cos / sin      position 0 (cos = 1, sin = 0 are fp16 numbers), a max-normalised comparison at any position; beyond position 8191
#                       the bar's own angle term has grown past the fp16 rounding of the trig
@pytest.mark.parametrize('base', RC.BASES)
@pytest.mark.parametrize('heads,hd', [(2, 128), (4, 100), (3, 64)])
def test_wrong_formulas_are_rejected(heads, hd, base):
    qkv, _ = _rows(heads, hd, 77 + hd)
    for i, p in enumerate(ALL_POS):
        qk, pos = qkv[:, i:i + 1, :2], np.array([[p]], dtype=np.int64)
        RC.assert_heads_close(RC.exact_rope_heads(qk, pos, hd, base).astype(np.float16), qk, pos, hd, base, 'the right formula')
        for f in RC.WRONG_FORMULAS:
            hidden = (f is RC.rope_row0_position                                # one row: nothing to confuse
                      or (f is RC.rope_base_ignored and base == 1e4)
                      or (p == 0 and f is not RC.rope_pos_plus_one)
                      or (f is RC.rope_fp16_trig and p > 8191))
            if hidden:
                if not (f is RC.rope_fp16_trig and p > 8191):                   # (beyond 8191: may or may not show; nothing is claimed)
                    _accepted(f, qk, pos, hd, base)
                continue
            s1, s10 = _rejected(f, qk, pos, hd, base)
            print('hd %d base %g pos %5d %-24s %5.1f %% beyond the bar, %5.1f %% beyond 10 x' % (hd, base, p, f.__name__, 100 * s1, 100 * s10))
            # not a near miss: a wrong frequency, sign, position, base or pairing throws a quarter of the row or more beyond 10 x the bar (a kernel
            # with such a bug cannot pass by luck on a few elements); fp16 trig is half-ulp noise and shows at 1 x the bar only
            if f is RC.rope_fp16_trig:
                assert s1 >= 0.02, (f.__name__, p, s1)
            else:
                assert s10 >= 0.25, (f.__name__, p, s10)


@pytest.mark.parametrize('base', RC.BASES)
def test_row0_position_is_rejected_on_the_other_batch_rows(base):
    """the batch the GPU test uses: bsz 3, seq 4, every batch row at positions of its own"""
    hd = 128
    pos = np.array([[0, 1, 2, 3], [300, 301, 302, 303], [4092, 4093, 4094, 4095]], dtype=np.int64)
    qk = RC.qkv_inputs((3, 4), 2, hd, 9)[:, :, :2]
    wrong = RC.rope_row0_position(qk, pos, hd, base).astype(np.float16)
    RC.assert_heads_close(wrong[:1], qk[:1], pos[:1], hd, base, 'row 0 itself')
    for b in (1, 2):
        with pytest.raises(AssertionError):
            RC.assert_heads_close(wrong[b:b + 1], qk[b:b + 1], pos[b:b + 1], hd, base, 'row %d' % b)
        s10 = RC.share_beyond(wrong[b:b + 1], qk[b:b + 1], pos[b:b + 1], hd, base, 10.0)
        print('base %g batch row %d with row 0 positions: %.1f %% beyond 10 x the bar' % (base, b, 100 * s10))
        assert s10 >= 0.40
    with pytest.raises(AssertionError):
        RC.assert_heads_close(wrong, qk, pos, hd, base, 'the whole batch')


def test_the_bar_is_half_an_ulp_at_short_positions_and_elementwise():
    """at pos <= 300 the angle term typically adds a few per cent to half an fp16 spacing and never doubles it (so cos / sin rounded to fp16
    cannot pass), and an error of two spacings in ONE small element fails the judge whatever the largest element is"""
    hd, base = 128, 1e4
    qkv, _ = _rows(2, hd, 3, positions=(1, 17, 300))
    qk, pos = qkv[:, :, :2], np.array([[1, 17, 300]], dtype=np.int64)
    x, y, p, _ = RC._split(qk, pos, hd)
    exact = RC.exact_rope_heads(qk, pos, hd, base)
    _, bound = RC.rope_errors(exact, x, y, p, hd, base)
    half_ulp = 0.5 * RC.fp16_ulp(exact)
    big = np.abs(exact) >= 0.25
    ratio = bound[big] / half_ulp[big]
    print('bound / half ulp where |exact| >= 0.25: median %.4f, max %.4f' % (np.median(ratio), ratio.max()))
    assert np.median(ratio) < 1.10 and ratio.max() < 2.0        # (the maximum: position 300, column 0, a pair with r >> |exact|)
    good = exact.astype(np.float16)
    RC.assert_heads_close(good, qk, pos, hd, base, 'rounded once')
    i = np.unravel_index(np.argmin(np.where(np.abs(exact) > 2.0 ** -6, np.abs(exact), np.inf)), exact.shape)
    bad = good.copy()
    bad[i] = np.nextafter(np.nextafter(bad[i], np.float16(np.inf)), np.float16(np.inf))      # two spacings of a value of ~0.016
    assert abs(float(bad[i]) - float(good[i])) < 1e-4 * np.abs(exact).max()                      # (invisible to any max-normalised bar)
    with pytest.raises(AssertionError):
        RC.assert_heads_close(bad, qk, pos, hd, base, 'one small element off')
