"""The attention cases of tests/attn_cases.py, checked on the CPU alone: fp32 models of the kernels' rounding points must sit inside the
per-element bar on every case the GPU tests use (a condition on the BAR: a faithful model outside it would mean the derivation is wrong), every
plausible wrong formula must be thrown out by ten times the bar on the cases designated for it (which is what shows that the GPU tests can see
one key, one row, the split merge and the softmax scale), and every planted needle must hold the weight it is planted for.

Why the flat cases of the older files stay (test_flat_inputs_under_both_bars prints the figures): on N(0, 1) q / 0.5 N(0, 1) k every key weighs
about 1 / n, so A = sum w |v| is ~0.8 while |out| is ~1 / sqrt(n): the per-element bar, whose terms scale with A, is LOOSER there than the
max-normalised 1e-3 once n reaches the thousands -- a dropped middle key at 1930 keys costs 30 times the old bar and 2.3 times the new one
(at 384 keys 87 against 77, at 130 keys 300 against 850).  With a planted key it is the other way round: the old bar, normalised by the largest
output of ALL rows (3.4 in the start = 0 case, whose last row reaches 0.42), holds a deep row to about 1 % of its own size, the new one to an
fp16 half-spacing.  Each bar sees what the other cannot; both stay."""
import numpy as np
import pytest

import attn_cases as AC

TOL_OLD = 1e-3


def _apply(case):
    q_rot, K, V = AC.host_apply(case)
    return q_rot, K, V, AC.attention_stats(q_rot, K, V, case.start, case.scale)


def _prompt_cases():
    """(family, case) of tests/test_gpu_attn_cases.py, prompt entry"""
    out = []
    for start, rows in AC.PROMPT_SHAPES:
        for needle in AC.prompt_needles(start, rows):
            out.append((needle[0], AC.build_case(start, rows, AC.PROMPT_T_MAX, AC.PROMPT_HEADS, needle=needle)))
    for start, rows in AC.PROMPT_SINK_SHAPES:
        for amp in AC.SINK_AMPS:
            out.append(('sink %g' % amp, AC.build_case(start, rows, AC.PROMPT_T_MAX, AC.PROMPT_HEADS, needle=AC.sink_needle(start), amp=amp)))
    for start, rows in AC.PROMPT_SCALE_SHAPES:
        for scale in AC.SCALES:
            for needle, amp in AC.scale_patterns(start, rows):
                out.append(('scale', AC.build_case(start, rows, AC.PROMPT_T_MAX, AC.PROMPT_HEADS, scale=scale, needle=needle, amp=amp)))
    for start, rows, needle, amp in AC.prompt_segment_patterns():
        out.append(('segment', AC.build_case(start, rows, AC.PROMPT_T_MAX, AC.PROMPT_HEADS, needle=needle, amp=amp)))
    return out


def _chunk_cases():
    """(family, case, split ranges) of the chunk entry"""
    out = []

    def add(family, p, rows, **kw):
        out.append((family, AC.build_case(p, rows, AC.CHUNK_T_MAX, AC.CHUNK_HEADS, **kw), AC.split_ranges(p + rows, AC.chunk_cap(), AC.CHUNK_TPS)))

    for rows in AC.CHUNK_ROWS:
        pos = AC.chunk_positions(rows)
        for which in (('one', 'two', 'deep') if rows == 5 else ('deep',)):
            for needle in AC.chunk_needles(pos[which], rows):
                add(needle[0], pos[which], rows, needle=needle)
    p = AC.chunk_positions(5)['deep']
    for amp in AC.SINK_AMPS:
        add('sink %g' % amp, p, 5, needle=('history', 0), amp=amp)
    for which in ('one', 'deep'):
        p = AC.chunk_positions(5)[which]
        for scale in AC.SCALES:
            for needle, amp in AC.scale_patterns(p, 5):
                add('scale', p, 5, scale=scale, needle=needle, amp=amp)
    return out


def _decode_cases(tps):
    """(family, case, split ranges) of the streaming decode entries at a tokens-per-split target"""
    out = []
    cap = AC.grid_splits(AC.DECODE_HEADS, AC.DECODE_T_MAX)
    for pos in AC.DECODE_POSITIONS:
        ranges = AC.split_ranges(pos + 1, cap, tps)
        for needle in AC.decode_needles(pos, ranges):
            out.append((needle[0], AC.build_case(pos, 1, AC.DECODE_T_MAX, AC.DECODE_HEADS, needle=needle), ranges))
    for pos in AC.DECODE_SCALE_POSITIONS:
        ranges = AC.split_ranges(pos + 1, cap, tps)
        for scale in AC.SCALES:
            for needle, amp in AC.scale_patterns(pos, 1):
                out.append(('scale', AC.build_case(pos, 1, AC.DECODE_T_MAX, AC.DECODE_HEADS, scale=scale, needle=needle, amp=amp), ranges))
    return out


def _report(title, worst):
    for family in sorted(worst):
        print('%-8s %-10s worst err/bar %.3f' % (title, family, worst[family]))


def test_the_split_rule_port():
    """a few values of attn_split() worked out by hand from csrc/attn_split.h (the GPU tests compare the port with the library's own counts)"""
    assert AC.attn_split(6, 8, 768) == (1, 128)
    assert AC.attn_split(768, 8, 768) == (1, 768) and AC.attn_split(770, 8, 768) == (2, 512)
    assert AC.attn_split(2048, 8, 768) == (3, 768) and AC.attn_split(2048, 8, 128) == (8, 256)
    assert AC.attn_split(1930, 8, 256) == (8, 256) and AC.attn_split(300, 8, 256) == (2, 256)
    assert AC.split_ranges(300, 8, 256) == [(0, 256), (256, 300)]
    assert AC.grid_splits(3, 1930) == 8 and AC.grid_splits(4, 2048) == 8 and AC.grid_splits(4, 2048, 5) == 8 and AC.grid_splits(4, 384) == 3


def test_prompt_model_is_inside_the_bar():
    worst = {}
    for family, case in _prompt_cases():
        q_rot, K, V, st = _apply(case)
        got = AC.model_attention(q_rot, K, V, case.start, case.scale, 'prompt')
        r = AC.assert_attn_close(got, st, 'prompt', name='prompt model, ' + case.name)
        worst[family] = max(worst.get(family, 0.0), r)
    _report('prompt', worst)


def test_chunk_model_is_inside_the_bar():
    worst = {}
    for family, case, ranges in _chunk_cases():
        q_rot, K, V, st = _apply(case)
        got = AC.model_attention(q_rot, K, V, case.start, case.scale, 'chunk', ranges)
        r = AC.assert_attn_close(got, st, 'chunk', *AC.span_of(ranges), name='chunk model, ' + case.name)
        worst[family] = max(worst.get(family, 0.0), r)
    _report('chunk', worst)


@pytest.mark.parametrize('tps', [768, 128])
def test_stream_model_is_inside_the_bar(tps):
    worst = {}
    for family, case, ranges in _decode_cases(tps):
        q_rot, K, V, st = _apply(case)
        got = AC.model_attention(q_rot, K, V, case.start, case.scale, 'stream', ranges)
        r = AC.assert_attn_close(got, st, 'stream', *AC.span_of(ranges), name='stream model, ' + case.name)
        worst[family] = max(worst.get(family, 0.0), r)
    _report('stream', worst)


# ---------------------------------------------------------------------------------------
# Which cases are designated for which wrong formula (rows: the rows whose worst element must lie beyond 10 x the bar):
#   needle dropped / twice   every amp-8 needle case; every row that may see the needle and has another key beside it
#   scale ignored            the `scale` cases at 0.05 and 0.2 whose largest weight is at most 0.98 (at 0.0884 the formula IS the right one to
#                            1e-4, and a weight of ~1 does not move with the temperature), the flat ones among them up to 512 keys (see
#                            attn_cases.MAX_FLAT_KEYS_FOR_SCALE; the amp-8 pattern carries the deep positions); the case as a whole
#   causal, one short        chunk@j and self: row j loses its own key (position 0 keeps its only key)
#   causal, one long         chunk@j and self with j >= 1: row j - 1 gains the needle
#   alpha not on the acc     amp-8 needles behind the first tile of the kernel (prompt 64, chunk 32, streaming 128 keys): the maximum rises
#                            there and what was summed before is never scaled down; every row that may see the needle
#   splits, equal weights    amp-8 needles of the cases the kernel cuts into several splits; every row that may see the needle
#   stale new token          chunk@j and self: the rows that may see the needle
# ---------------------------------------------------------------------------------------
def _designated(f, case, st, ranges, tile):
    """rows (an index array) on which formula f must be rejected in this case; None: the case is not designated for f"""
    rows = np.arange(case.rows)
    needle8 = case.needle is not None and case.amp == AC.AMP
    sees = rows >= case.first_row if case.needle is not None else None
    several = (case.start + rows) >= 1                                     # the row has another key beside the last one
    kind = None if case.needle is None else case.needle[0]
    if f in (AC.attn_needle_dropped, AC.attn_needle_twice):
        return rows[sees & several] if needle8 else None
    if f is AC.attn_causal_one_short:
        return rows[case.first_row:case.first_row + 1] if needle8 and kind in ('chunk', 'self') and case.key > 0 else None
    if f is AC.attn_causal_one_long:
        return rows[case.first_row - 1:case.first_row] if needle8 and kind in ('chunk', 'self') and case.first_row >= 1 else None
    if f is AC.attn_alpha_not_on_acc:
        return rows[sees] if needle8 and case.key >= tile else None
    if f is AC.attn_splits_equal_weights:
        return rows[sees] if needle8 and len(ranges) > 1 else None
    if f is AC.attn_stale_new_token:
        return rows[sees] if needle8 and kind in ('chunk', 'self') else None
    raise AssertionError(f)


def _reject(cases, kernel, tile):
    """every designated (formula, case): the formula's float64 result, rounded to fp16, beyond 10 x the bar in every designated row"""
    least = {}
    for family, case, ranges in cases:
        q_rot, K, V, st = _apply(case)
        sk, sv = AC.stale_rows(case)
        ctx = dict(key=case.key, splits=ranges, tile=tile, stale_K=sk, stale_V=sv)
        for f in AC.WRONG_FORMULAS:
            if f is AC.attn_scale_ignored:
                if family != 'scale' or case.scale == AC.SCALE or st.w.max() > AC.MAX_WEIGHT_FOR_SCALE:
                    continue
                if case.needle is None and case.start + case.rows > AC.MAX_FLAT_KEYS_FOR_SCALE:
                    continue
                rows = None
            else:
                rows = _designated(f, case, st, ranges, tile)
                if rows is None or rows.size == 0:
                    continue
            wrong = f(q_rot, K, V, case.start, case.scale, ctx).astype(np.float16)
            ratio = AC.attn_ratio(wrong, st, kernel, *AC.span_of(ranges)).max(axis=(1, 2))          # per row
            r = float(ratio.max()) if rows is None else float(ratio[rows].min())
            assert r >= 10.0, (f.__name__, kernel, case.name, r)
            least[f.__name__] = min(least.get(f.__name__, np.inf), r)
    for name in sorted(least):
        print('%-8s %-28s least worst-element err/bar over its designated rows %.3g' % (kernel, name, least[name]))
    return least


def test_wrong_formulas_are_rejected_prompt():
    least = _reject([(fam, c, [(0, c.start + c.rows)]) for fam, c in _prompt_cases()], 'prompt', 64)
    assert set(least) == {f.__name__ for f in AC.WRONG_FORMULAS} - {'attn_splits_equal_weights'}


def test_wrong_formulas_are_rejected_chunk():
    least = _reject(_chunk_cases(), 'chunk', 32)
    assert set(least) == {f.__name__ for f in AC.WRONG_FORMULAS}


@pytest.mark.parametrize('tps', [768, 128])
def test_wrong_formulas_are_rejected_stream(tps):
    least = _reject(_decode_cases(tps), 'stream', 128)
    assert set(least) == {f.__name__ for f in AC.WRONG_FORMULAS} - {'attn_causal_one_long'}      # (one row: nothing beyond it)


def test_the_right_formula_rounded_once_is_accepted():
    for family, case in _prompt_cases()[::5]:
        q_rot, K, V, st = _apply(case)
        AC.assert_attn_close(AC.exact_attention(q_rot, K, V, case.start, case.scale).astype(np.float16), st, 'stream', name=case.name)


def test_needles_hold_their_weight():
    """at least 0.3 of the weight in every row that may see the needle, exactly 0 in every row that may not"""
    least = 1.0
    cases = [(f, c) for f, c in _prompt_cases()] + [(f, c) for f, c, _ in _chunk_cases() + _decode_cases(768) + _decode_cases(128)]
    for family, case in cases:
        if case.needle is None:
            continue
        st = _apply(case)[3]
        w = st.w[:, :, case.key]
        assert (w[:case.first_row] == 0.0).all(), case.name
        assert (w[case.first_row:] >= 0.3).all(), (case.name, float(w[case.first_row:].min()))
        if family.startswith('sink'):
            assert (w[case.first_row:] >= 0.97).all(), (case.name, float(w[case.first_row:].min()))
        least = min(least, float(w[case.first_row:].min()))
    print('least needle weight %.3f' % least)


def _flat_prompt_inputs(start, rows, t_max, H):
    """the generator of tests/test_gpu_prompt_attn.py::_inputs and tests/test_gpu_attn_chunk.py::_inputs, line by line"""
    rng = np.random.default_rng(1000 * start + rows)
    qkv = rng.standard_normal((rows, 3 * H)).astype(np.float32)
    kc = (rng.standard_normal((t_max, H)) * 0.5).astype(np.float16)
    vc = rng.standard_normal((t_max, H)).astype(np.float16)
    return qkv.astype(np.float16), kc, vc


@pytest.mark.parametrize('start,rows,t_max,heads,kind', [(0, 130, 384, 4, 'prompt'), (255, 129, 384, 4, 'prompt'), (1925, 5, 1930, 3, 'chunk')])
def test_flat_inputs_under_both_bars(start, rows, t_max, heads, kind):
    """the existing flat inputs with one middle key dropped: what that costs under max|err| / max|exact| < 1e-3 and under the per-element bar"""
    qkv, kc, vc = _flat_prompt_inputs(start, rows, t_max, heads * AC.HD)
    case = AC.Case(start, rows, t_max, heads, AC.SCALE, None, 0.0, qkv, kc, vc, None, None)
    q_rot, K, V, st = _apply(case)
    key = (start + rows) // 2
    wrong = AC.attn_needle_dropped(q_rot, K, V, start, case.scale, dict(key=key)).astype(np.float16)
    err = np.abs(wrong.astype(np.float64) - st.out)
    old = float(err.max() / np.abs(st.out).max() / TOL_OLD)
    ranges = AC.split_ranges(start + rows, 8, AC.CHUNK_TPS) if kind == 'chunk' else [(0, start + rows)]
    new = float(AC.attn_ratio(wrong, st, kind, *AC.span_of(ranges)).max())
    ours = AC.model_attention(q_rot, K, V, start, case.scale, kind, ranges)
    r_model = AC.assert_attn_close(ours, st, kind, *AC.span_of(ranges), name='model on flat inputs')
    deep = st.out[-1]
    print('flat (%d, %d) key %d dropped: %.2f x the old bar, %.2f x the new one; model %.3f; last row max|out| %.3f against %.3f overall'
          % (start, rows, key, old, new, r_model, np.abs(deep).max(), np.abs(st.out).max()))
    assert old > 1.0 or new > 1.0, 'a dropped key passes both bars'
    if kind == 'chunk':
        assert old > new, 'at ~2000 flat keys the max-normalised bar is the tighter one: the reason the flat cases stay'


def test_the_o_proj_bar_sees_a_lost_needle():
    """the bar of test_gpu_attn_cases.test_o_proj_record_merge -- y = x W is linear in the attention row, so B passes through as B |W|, plus the
    op-level 1e-3 max|y| for o_proj's own arithmetic -- on the host with an exact o_proj: the streaming model's row stays inside it, a dropped
    needle is thrown out by ten times the bar or more"""
    from oracle import oracle
    from util import TOL, make_random_layer
    H = AC.DECODE_HEADS * AC.HD
    L = make_random_layer(4, 128, H, H, seed=5)
    W = np.asarray(oracle.np_dequant(L['qweight'], L['qzeros'], L['scales'], L['g_idx'], L['bits'], faithful=False), dtype=np.float64)
    cap = AC.grid_splits(AC.DECODE_HEADS, AC.DECODE_T_MAX)
    least = np.inf
    for pos in AC.DECODE_POSITIONS:
        ranges = AC.split_ranges(pos + 1, cap, 128)
        for needle in (('self', 0), ('history', pos - 1), ('history', 0)):
            case = AC.build_case(pos, 1, AC.DECODE_T_MAX, AC.DECODE_HEADS, needle=needle)
            q_rot, K, V, st = _apply(case)
            exact = st.out.reshape(-1) @ W
            bar = AC.attn_bound(st, 'stream', *AC.span_of(ranges)).reshape(-1) @ np.abs(W) + TOL * np.abs(exact).max()
            good = AC.model_attention(q_rot, K, V, pos, case.scale, 'stream', ranges).astype(np.float64).reshape(-1) @ W
            wrong = AC.attn_needle_dropped(q_rot, K, V, pos, case.scale, dict(key=case.key)).astype(np.float16).astype(np.float64).reshape(-1) @ W
            assert (np.abs(good - exact) / bar).max() <= 1.0, case.name
            r = float((np.abs(wrong - exact) / bar).max())
            assert r >= 10.0, (case.name, r)
            least = min(least, r)
    print('o_proj bar: a dropped needle costs at least %.3g x the bar' % least)
