"""Attention cases shared by the host and GPU attention tests (plain numpy, no GPU): inputs with PLANTED keys, the float64 reference with
its weights, the per-element bar every attention kernel is held to, the formulas a kernel could compute instead without a flat-logit,
one-scale, max-normalised test noticing, and fp32 models of the kernels' rounding points.

The inputs.  Per head a direction u ~ N(0, 1)^128; the raw query of the row at position p is R(p)^-1 (u + 0.3 noise), so that every ROTATED
query is u plus noise whatever its position.  Background keys are 0.2 N(0, 1) (logit standard deviation ~0.2 at scale 1 / sqrt(128)), values
N(0, 1).  A needle is one key whose logit lies `amp` natural-log units above that background, with a value row drawn at 4 x the others, so
that a lost, doubled or leaked needle moves the output by order 1:
    ('history', t)  cache row t < start is amp / scale * u / |u|^2 plus background (the cache holds rotated keys)
    ('chunk', j)    the raw key of chunk row j is R(p_j)^-1 (amp / scale * u / |u|^2): the kernel's own RoPE and append produce the cache row;
                    rows r >= j see it, rows r < j must not
    ('self', r)     the raw key of row r is amp / scale * q_raw[r] / |q_raw[r]|^2: RoPE is orthogonal, the row's own key scores amp
                    (ONE row carries it: the keys of several such rows would score 0.92 amp against each other's queries and share the weight)
amp = 8 wherever a dropped key or the scale must show (the needle then holds 0.4 .. 0.98 of the weight up to 2048 keys); the `sink` family
puts amp = 12, 16, 20 on key 0, which drives every later weight of the row into and below the fp16 subnormal range of P.

The bar.  exact = sum_j w_j v_j in float64 on the fp16 values the kernel itself read (w = softmax(scale q . k) over the row's visible keys);
A = sum_j w_j |v_j|.  Rounding points, as read in csrc/decode_attn.hip, csrc/prompt_attn.hip, csrc/chunk_attn.hip, csrc/attn_device.h (the
last arriver's merge) and csrc/attn_split.h:

  score   every kernel forms p_j = exp2(s_j - m), s_j = fp32(q . k_j) * scale2, scale2 = fp32(scale * log2 e), m some running maximum.  m is
          the SAME number in the numerator and in l, and the rescale alpha multiplies both: their errors cancel.  What does not cancel is a
          relative error E_j of p_j:
            * the fp32 dot product of length 128: the products of two fp16 numbers are exact in fp32, every addition rounds; in ANY order
              (fma chains plus a DPP tree, or the MFMA's accumulator) at most 128 roundings of partial sums bounded by sum_i |q_i k_ji|:
              2^-17 a_j in logit units, a_j = scale * sum_i |q_i| |k_ji|;
            * scale2 itself (one product, the constant's own representation: 1.5 x 2^-24 relative, on a difference s_j - m of at most 2 L,
              L = max_j |logit_j| of the row), the product dot * scale2 (2^-24 L), the subtraction s_j - m (2^-24 x 2 L), for __expf the
              product with log2 e (2^-24 x 2 L): together 8 x 2^-24 L = 2^-21 L;
            * v_exp_f32: one ulp, 2^-23.
          E_j = 2^-17 a_j + 2^-21 L + 2^-23, and to first order  |d out| <= sum_j w_j E_j |v_j| + |out| sum_j w_j E_j.
  sums    l and the accumulator are fp32 sums of n non-negative (resp. n signed) terms: `depth` roundings along the longest chain, each 2^-24
          of a partial sum bounded by l (resp. by A l): 2 x depth x 2^-24 x A.  depth as the kernel's loops give it (per lane, rescales,
          the reductions behind the loop, the merge):  streaming decode kernel n / 16 + n / 128 + 16 (16 timesteps per pass of a workgroup);
          partial + combine pair 48 + n / 128;  prompt kernel n + n / 64 + 8 (the MFMA sums 16 keys per instruction: counted as one
          rounding per key);  chunk kernel 33 x ceil(n / 128) + 16 (a wave owns every fourth 32-key tile: 32 keys and one rescale per 128).
          With several splits n is the longest split's length (`span`): the chains of different splits only meet in the merge.
  P       the two MFMA kernels round p to fp16 before the second product, relative to the running maximum (<= the final one, and l >= 1
          in units of the final one): 2^-11 relative for a normal p, 2^-25 absolute for a subnormal one -- 2^-11 A + n 2^-25 max|v|; l is
          summed from the unrounded values, so there is no |out| term.  The streaming kernel and the partial / combine pair keep p in fp32.
  splits  with several splits every path but the fp32 partial / combine pair rounds each split's normalised row to fp16 before the merge
          (coefficients sum to 1): 2^-11 A + 2^-25.
  norm    v_rcp_f32 (one ulp) and the product behind it; in a merge exp2, two products, a sum of up to 8 and a reciprocal per coefficient
          (under 2^-20 relative each, on sum_s c_s |o_s| + |out| <= 2 A) and an fma chain of 8: 2^-18 A covers all of it.
  store   one rounding to fp16 of a value within the sum T of the terms above of exact: 1/2 ulp16(|exact| + T) (records merged in float64 on
          the host have no store of their own with several splits; the bar keeps the term, so it is the same for both).

Nothing in it is fitted to a kernel.  With a needle the bar is about one fp16 half-spacing of the output; on flat logits over thousands of keys
A >> |out| and it is LOOSER than the suite's max-normalised 1e-3 (tests/test_host_attn.py prints both): the planted cases are added next to the
flat ones, they do not replace them."""
import functools

import numpy as np

import rope_cases as RC
from util import fp16_ulp

HD = 128
BASE = 10000.0
NAN_BITS = 0x7E00
AMP = 8.0
SINK_AMPS = (12.0, 16.0, 20.0)
SCALES = (0.05, 0.0884, 0.2)
SCALE = 0.0884                       # the cases that do not vary it
MAX_WEIGHT_FOR_SCALE = 0.98          # a scale case is judged on the scale formula only if its largest weight stays below this ...
MAX_FLAT_KEYS_FOR_SCALE = 512        # ... and, if it is flat, only up to this many keys: there the output moves by ~ d(scale) / scale x 0.2 / sqrt(n)
                                     # while the bar stays ~2^-10 A (measured on the host at 1930 keys: 5 x the bar, seen but not tenfold)
MFMA_KINDS = ('prompt', 'chunk')
ATT_TILE = 128
ATT_MAX_SPLITS = 8

DEPTH = {
    'stream': lambda n: np.ceil(n / 16.0) + np.ceil(n / 128.0) + 16,
    'partial': lambda n: 48 + np.ceil(n / 128.0),
    'prompt': lambda n: n + np.ceil(n / 64.0) + 8,
    'chunk': lambda n: 33 * np.ceil(n / 128.0) + 16,
}


# ---------------------------------------------------------------------------------------
# the library's split rule (csrc/attn_split.h, csrc/decode_attn.hip): the GPU tests check this port against the library's own counts
# ---------------------------------------------------------------------------------------
def attn_split(length, cap, tps):
    """(active splits, timesteps per split) of a row that attends to `length` keys"""
    want = min(1 + sum(length > i * tps for i in range(1, ATT_MAX_SPLITS)), cap)
    per = -(-length // want)
    chunk = -(-per // ATT_TILE) * ATT_TILE
    return 1 + sum(i * chunk < length for i in range(1, ATT_MAX_SPLITS)), chunk


def split_ranges(length, cap, tps):
    nsp, chunk = attn_split(length, cap, tps)
    return [(s * chunk, min((s + 1) * chunk, length)) for s in range(nsp)]


def grid_splits(heads, t_max, batch=1):
    return min(min(max(256 // max(1, heads * batch), 1), ATT_MAX_SPLITS), -(-t_max // ATT_TILE))


def fixed_ranges(length, ts=128):
    """the partial + combine pair: splits of 128 timesteps whatever the length"""
    return [(t0, min(t0 + ts, length)) for t0 in range(0, length, ts)]


# ---------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------
def _unrotate(x, pos):
    """R(pos)^-1 x in float64: x [rows, heads, HD], pos [rows]"""
    return RC.exact_rope_heads(x, -np.asarray(pos, dtype=np.float64), HD, BASE)


def rotate(x, pos):
    return RC.exact_rope_heads(x, np.asarray(pos, dtype=np.float64), HD, BASE)


@functools.lru_cache(maxsize=16)
def _background(start, rows, t_max, heads, seed):
    rng = np.random.default_rng(seed)
    pos = start + np.arange(rows)
    u = rng.standard_normal((heads, HD))
    bg = dict(u=u,
              q_raw=_unrotate(u[None] + 0.3 * rng.standard_normal((rows, heads, HD)), pos).astype(np.float16),
              k_raw=(0.2 * rng.standard_normal((rows, heads, HD))).astype(np.float16),
              v_new=rng.standard_normal((rows, heads, HD)).astype(np.float16),
              kc=(0.2 * rng.standard_normal((t_max, heads, HD))).astype(np.float16),
              vc=rng.standard_normal((t_max, heads, HD)).astype(np.float16),
              needle_v=(4.0 * rng.standard_normal((heads, HD))).astype(np.float16))
    for a in bg.values():
        a.setflags(write=False)
    return bg


class Case:
    """qkv [rows, 3 H] fp16 (unrotated), kc / vc [t_max, H] fp16: the history below start, background values in rows start .. start + rows - 1
    (a stale cache: the call must overwrite them), NaN behind.  key: the needle's cache row (None: flat); first_row: the first chunk row
    that may see it."""

    def __init__(self, start, rows, t_max, heads, scale, needle, amp, qkv, kc, vc, key, first_row):
        self.start, self.rows, self.t_max, self.heads, self.scale, self.needle, self.amp = start, rows, t_max, heads, scale, needle, amp
        self.qkv, self.kc, self.vc, self.key, self.first_row = qkv, kc, vc, key, first_row
        for a in (qkv, kc, vc):
            a.setflags(write=False)

    @property
    def name(self):
        what = 'flat' if self.needle is None else '%s@%d amp %g' % (self.needle[0], self.needle[1], self.amp)
        return 'start %d rows %d scale %g %s' % (self.start, self.rows, self.scale, what)


def build_case(start, rows, t_max, heads, scale=SCALE, needle=None, amp=AMP, seed=None):
    seed = 7919 * start + 31 * rows + heads if seed is None else seed
    bg = _background(start, rows, t_max, heads, seed)
    assert 0 <= start and rows >= 1 and start + rows <= t_max
    q, k, v = bg['q_raw'], bg['k_raw'].copy(), bg['v_new'].copy()
    kc, vc = bg['kc'].copy(), bg['vc'].copy()
    u = bg['u']
    d = amp / scale * u / (u * u).sum(-1, keepdims=True)                  # scale * (u . d) = amp
    key = first_row = None
    if needle is not None:
        kind, i = needle
        if kind == 'history':
            assert 0 <= i < start, needle
            kc[i] = (d + kc[i].astype(np.float64)).astype(np.float16)
            vc[i] = bg['needle_v']
            key, first_row = i, 0
        elif kind == 'chunk':
            assert 0 <= i < rows, needle
            k[i] = _unrotate(d[None], [start + i])[0].astype(np.float16)
            v[i] = bg['needle_v']
            key, first_row = start + i, i
        elif kind == 'self':
            assert 0 <= i < rows, needle
            qi = q[i].astype(np.float64)
            k[i] = (amp / scale * qi / (qi * qi).sum(-1, keepdims=True)).astype(np.float16)
            v[i] = bg['needle_v']
            key, first_row = start + i, i
        else:
            raise ValueError(needle)
    nan = np.uint16(NAN_BITS).view(np.float16)
    kc[start + rows:] = nan
    vc[start + rows:] = nan
    H = heads * HD
    qkv = np.ascontiguousarray(np.stack([q, k, v], axis=1).reshape(rows, 3 * H))
    return Case(start, rows, t_max, heads, scale, needle, amp, qkv, kc.reshape(t_max, H), vc.reshape(t_max, H), key, first_row)


def host_apply(case):
    """what the call leaves, computed on the host (float64 rotation, one fp16 rounding): q_rot [rows, heads, HD], K / V [start + rows, heads, HD]
    fp16 -- the stand-in for the device's own values where there is no device"""
    c = case
    x = c.qkv.reshape(c.rows, 3, c.heads, HD)
    pos = c.start + np.arange(c.rows)
    n = c.start + c.rows
    K, V = c.kc[:n].reshape(n, c.heads, HD).copy(), c.vc[:n].reshape(n, c.heads, HD).copy()
    K[c.start:] = rotate(x[:, 1], pos).astype(np.float16)
    V[c.start:] = x[:, 2]
    return rotate(x[:, 0], pos).astype(np.float16), K, V


def stale_rows(case):
    """cache rows start .. start + rows - 1 as they were BEFORE the call: (K, V) [rows, heads, HD]"""
    c = case
    sl = slice(c.start, c.start + c.rows)
    return c.kc[sl].reshape(c.rows, c.heads, HD), c.vc[sl].reshape(c.rows, c.heads, HD)


# ---------------------------------------------------------------------------------------
# the float64 reference
# ---------------------------------------------------------------------------------------
def _qk(q, K):
    """sum_d q[r, h, d] K[n, h, d] -> [rows, heads, n] (batched matmul: einsum without BLAS is ten times slower)"""
    return np.matmul(q.transpose(1, 0, 2), K.transpose(1, 2, 0)).transpose(1, 0, 2)


def _wv(w, V):
    """sum_n w[r, h, n] V[n, h, d] -> [rows, heads, d]"""
    return np.matmul(w.transpose(1, 0, 2), V.transpose(1, 0, 2)).transpose(1, 0, 2)


def _logits(q_rot, K, start, scale):
    """float64 logits [rows, heads, n], -inf above each row's own position (row r sees keys 0 .. start + r)"""
    q, K = np.asarray(q_rot, dtype=np.float64), np.asarray(K, dtype=np.float64)
    x = _qk(q, K) * np.float64(np.float32(scale))
    hidden = np.arange(K.shape[0])[None, :] > (start + np.arange(q.shape[0]))[:, None]
    x[np.broadcast_to(hidden[:, None, :], x.shape)] = -np.inf
    return x


def _softmax(x):
    with np.errstate(invalid='ignore'):
        e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def exact_attention(q_rot, K, V, start, scale, ctx=None):
    """float64 causal softmax attention: q_rot [rows, heads, HD] rotated queries at positions start .., K / V [n, heads, HD] the caches after
    the append (n >= start + rows) -> [rows, heads, HD].  ctx is for the wrong formulas below (same signature)."""
    return _wv(_softmax(_logits(q_rot, K, start, scale)), np.asarray(V, dtype=np.float64))


class Stats:
    """the reference with what the bar needs: out, w [rows, heads, n], A = w @ |V|, S the score term, vmax and L per (row, head)"""


def attention_stats(q_rot, K, V, start, scale):
    st = Stats()
    q, K64, V64 = (np.asarray(t, dtype=np.float64) for t in (q_rot, K, V))
    x = _logits(q, K64, start, scale)
    seen = np.isfinite(x)
    st.w = _softmax(x)
    absV = np.abs(V64)
    st.out = _wv(st.w, V64)
    st.A = _wv(st.w, absV)
    st.L = np.where(seen, np.abs(x), 0.0).max(-1)
    a = _qk(np.abs(q), np.abs(K64)) * np.float64(np.float32(scale))
    wE = st.w * (2.0 ** -17 * a + (2.0 ** -21 * st.L + 2.0 ** -23)[..., None])
    st.S = _wv(wE, absV) + np.abs(st.out) * wE.sum(-1)[..., None]
    vabs = absV.max(-1)                                                       # [n, heads]
    st.vmax = np.where(seen, vabs.T[None], 0.0).max(-1)
    st.start = start
    return st


def attn_bound(st, kind, nsp=1, span=None):
    """the per-element bar of the module docstring: kind in DEPTH, nsp the number of splits whose fp16 rows were merged, span the longest
    split's length (None: one split, the row's own key count)"""
    n = (st.start + 1 + np.arange(st.out.shape[0], dtype=np.float64))[:, None, None]
    T = st.S + 2.0 * DEPTH[kind](n if span is None else np.minimum(n, span)) * 2.0 ** -24 * st.A + 2.0 ** -18 * st.A
    if kind in MFMA_KINDS:
        T = T + 2.0 ** -11 * st.A + n * 2.0 ** -25 * st.vmax[..., None]
    if nsp > 1 and kind != 'partial':
        T = T + 2.0 ** -11 * st.A + 2.0 ** -25
    return T + 0.5 * fp16_ulp(np.abs(st.out) + T)


def attn_ratio(got, st, kind, nsp=1, span=None):
    """err / bar per element, [rows, heads, HD]"""
    got = np.asarray(got, dtype=np.float64).reshape(st.out.shape)
    return np.abs(got - st.out) / attn_bound(st, kind, nsp, span)


def span_of(ranges):
    """(nsp, span) arguments of the bar for a list of split ranges"""
    return len(ranges), (max(t1 - t0 for t0, t1 in ranges) if len(ranges) > 1 else None)


def assert_attn_close(got, st, kind, nsp=1, span=None, name='', rows=None):
    """THE judge of the attention cases: every element of got (rows: of those rows only) within its own bar of the float64 result --
    elementwise, never normalised by a maximum.  Returns the worst err / bar."""
    got = np.asarray(got).reshape(st.out.shape)
    assert np.isfinite(got.astype(np.float64)).all(), (name, 'not finite')
    assert (np.abs(st.out).max(-1) >= 2.0 ** -10).all(), (name, 'a row below the floor of the bar')
    ratio = attn_ratio(got, st, kind, nsp, span)
    if rows is not None:
        ratio = ratio[rows]
    bad = ratio > 1.0
    if bad.any():
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError('%s: %d of %d elements (%.1f %%) beyond the bar, %.1f %% beyond 10 x; worst err/bar %.3g at (row, head, dim) %s'
                             % (name, int(bad.sum()), bad.size, 100.0 * bad.mean(), 100.0 * (ratio > 10.0).mean(), float(ratio[i]), i))
    return float(ratio.max())


# ---------------------------------------------------------------------------------------
# what a kernel could compute instead (float64; the signature of exact_attention; ctx: dict(key, splits, tile, stale_K, stale_V))
# ---------------------------------------------------------------------------------------
def _out(x, V):
    return _wv(_softmax(x), np.asarray(V, dtype=np.float64))


def attn_needle_dropped(q_rot, K, V, start, scale, ctx):
    x = _logits(q_rot, K, start, scale)
    only = np.isfinite(x).sum(-1) == 1                       # a row whose only key is the needle keeps it (an empty softmax is no formula)
    keep = x[:, :, ctx['key']].copy()
    x[:, :, ctx['key']] = np.where(only, keep, -np.inf)
    return _out(x, V)


def attn_needle_twice(q_rot, K, V, start, scale, ctx):
    x = _logits(q_rot, K, start, scale)
    x[:, :, ctx['key']] += np.log(2.0)
    return _out(x, V)


def attn_scale_ignored(q_rot, K, V, start, scale, ctx):
    return exact_attention(q_rot, K, V, start, 1.0 / np.sqrt(np.asarray(q_rot).shape[-1]))


def attn_causal_one_short(q_rot, K, V, start, scale, ctx):
    """row r stops at key start + r - 1 (the row at position 0 keeps its only key)"""
    x = _logits(q_rot, K, start, scale)
    for r in range(x.shape[0]):
        if start + r > 0:
            x[r, :, start + r] = -np.inf
    return _out(x, V)


def attn_causal_one_long(q_rot, K, V, start, scale, ctx):
    """row r also sees key start + r + 1 where the call has written one"""
    q = np.asarray(q_rot, dtype=np.float64)
    x = _logits(q, K, start, scale)
    full = _qk(q, np.asarray(K, dtype=np.float64)) * np.float64(np.float32(scale))
    for r in range(x.shape[0] - 1):
        x[r, :, start + r + 1] = full[r, :, start + r + 1]
    return _out(x, V)


def attn_alpha_not_on_acc(q_rot, K, V, start, scale, ctx):
    """online softmax over tiles of ctx['tile'] keys whose rescale reaches l but not the accumulator"""
    x = _logits(q_rot, K, start, scale)
    V = np.asarray(V, dtype=np.float64)
    rows, heads, n = x.shape
    M = np.full((rows, heads), -np.inf)
    l = np.zeros((rows, heads))
    acc = np.zeros((rows, heads, V.shape[-1]))
    with np.errstate(invalid='ignore'):
        for tb in range(0, n, ctx['tile']):
            sc = x[:, :, tb:tb + ctx['tile']]
            Mn = np.maximum(M, sc.max(-1))
            ref = np.where(np.isfinite(Mn), Mn, 0.0)
            alpha = np.exp(M - ref)
            p = np.exp(sc - ref[..., None])
            l = l * alpha + p.sum(-1)
            acc = acc + _wv(p, V[tb:tb + ctx['tile']])
            M = Mn
    return acc / l[..., None]


def attn_splits_equal_weights(q_rot, K, V, start, scale, ctx):
    """every split normalised against its own maximum, the merge forgets the maxima: c_s = den_s / sum den"""
    x = _logits(q_rot, K, start, scale)
    V = np.asarray(V, dtype=np.float64)
    num, den = 0.0, 0.0
    with np.errstate(invalid='ignore'):
        for t0, t1 in ctx['splits']:
            sc = x[:, :, t0:t1]
            m = sc.max(-1, keepdims=True)
            p = np.where(np.isfinite(m), np.exp(sc - np.where(np.isfinite(m), m, 0.0)), 0.0)
            num = num + _wv(p, V[t0:t1])
            den = den + p.sum(-1)
    return num / den[..., None]


def attn_stale_new_token(q_rot, K, V, start, scale, ctx):
    """the keys and values of the call's own rows read from the cache before the append"""
    K, V = np.array(K, dtype=np.float64), np.array(V, dtype=np.float64)
    rows = np.asarray(q_rot).shape[0]
    K[start:start + rows] = ctx['stale_K']
    V[start:start + rows] = ctx['stale_V']
    return exact_attention(q_rot, K, V, start, scale)


WRONG_FORMULAS = (attn_needle_dropped, attn_needle_twice, attn_scale_ignored, attn_causal_one_short, attn_causal_one_long, attn_alpha_not_on_acc,
                  attn_splits_equal_weights, attn_stale_new_token)


# ---------------------------------------------------------------------------------------
# fp32 models of the kernels' rounding points (numpy float32; the order of the sums is numpy's, the rounding points are the kernels')
# ---------------------------------------------------------------------------------------
M_FLOOR = np.float32(-1.0e30)


def model_attention(q_rot, K, V, start, scale, kind, splits=None):
    """prompt: one running maximum, 64-key tiles, p rounded to fp16 for the second product, l from the unrounded values, one fp16 store.
    chunk:  per split four waves over interleaved 32-key tiles, a maximum per wave, p rounded to fp16; the waves combined in fp32; with several
            splits fp16 records merged with c_s = 2^(M_s - max) den_s / sum.
    stream: as chunk with p kept in fp32.                                                            -> fp16 [rows, heads, HD]"""
    tile, waves, p16 = {'prompt': (64, 1, True), 'chunk': (32, 4, True), 'stream': (32, 4, False)}[kind]
    f32 = np.float32
    q, K32, V32 = (np.asarray(t, dtype=f32) for t in (q_rot, K, V))
    rows, heads, hd = q.shape
    n = K32.shape[0]
    splits = [(0, n)] if splits is None else splits
    scale2 = f32(f32(scale) * f32(1.44269504088896340736))
    s = (_qk(q, K32).astype(f32) * scale2).astype(f32)
    hidden = np.arange(n)[None, :] > (start + np.arange(rows))[:, None]
    s[np.broadcast_to(hidden[:, None, :], s.shape)] = -np.inf
    recs = []
    for t0, t1 in splits:
        Ms, ls, accs = [], [], []
        for w in range(waves):
            M = np.full((rows, heads), M_FLOOR, dtype=f32)
            l = np.zeros((rows, heads), dtype=f32)
            acc = np.zeros((rows, heads, hd), dtype=f32)
            for tb in range(t0 + w * tile, t1, waves * tile):
                te = min(tb + tile, t1)
                sc = s[:, :, tb:te]
                Mn = np.maximum(M, sc.max(-1))
                alpha = np.exp2(M - Mn).astype(f32)
                p = np.exp2(sc - Mn[..., None]).astype(f32)
                pv = p.astype(np.float16).astype(f32) if p16 else p
                l = (l * alpha + p.sum(-1, dtype=f32)).astype(f32)
                acc = (acc * alpha[..., None] + _wv(pv, V32[tb:te]).astype(f32)).astype(f32)
                M = Mn
            Ms.append(M), ls.append(l), accs.append(acc)
        Mx = np.maximum.reduce(Ms)
        den = np.zeros((rows, heads), dtype=f32)
        num = np.zeros((rows, heads, hd), dtype=f32)
        for M, l, acc in zip(Ms, ls, accs):
            e = np.exp2(M - Mx).astype(f32)
            den = (den + e * l).astype(f32)
            num = (num + e[..., None] * acc).astype(f32)
        with np.errstate(divide='ignore', invalid='ignore'):
            o = np.where(den[..., None] > 0, num / den[..., None], f32(0)).astype(f32)
        recs.append((Mx, den, o.astype(np.float16)))
    if len(recs) == 1:
        return recs[0][2]
    Mx = np.maximum.reduce([r[0] for r in recs])
    c = [(np.exp2(r[0] - Mx).astype(f32) * r[1]).astype(f32) for r in recs]
    D = np.add.reduce(c).astype(f32)
    out = np.zeros((rows, heads, hd), dtype=f32)
    for ci, r in zip(c, recs):
        out = (out + (ci / D).astype(f32)[..., None] * r[2].astype(f32)).astype(f32)
    return out.astype(np.float16)


# ---------------------------------------------------------------------------------------
# the cases of the GPU tests (tests/test_host_attn.py runs the models and the wrong formulas on the same lists)
# ---------------------------------------------------------------------------------------
PROMPT_T_MAX, PROMPT_HEADS = 384, 4
PROMPT_SHAPES = ((0, 65), (0, 130), (130, 70), (255, 129))
PROMPT_SINK_SHAPES = ((0, 130), (255, 129))
PROMPT_SCALE_SHAPES = ((0, 65), (255, 129))
PROMPT_SEGS = ((0, 1), (5, 1), (0, 65), (130, 70), (255, 129))           # SEGS of tests/test_gpu_prompt_attn_batch.py


def prompt_needles(start, rows):
    hist = sorted({t for t in (0, 63, 64, 127, 128, start - 1) if 0 <= t < start})
    chunk = sorted({j for j in (0, 31, 32, 63, 64, rows - 1) if 0 <= j < rows})
    return [('history', t) for t in hist] + [('chunk', j) for j in chunk] + [('self', rows - 1)]


def sink_needle(start):
    return ('history', 0) if start > 0 else ('chunk', 0)


def scale_patterns(start, rows):
    """one flat pattern and one amp-8 needle away from every edge: (needle, amp)"""
    n = start + rows
    mid = n // 2
    return [(None, AMP), (('history', mid) if mid < start else ('chunk', mid - start), AMP)]


def prompt_segment_patterns():
    """a different pattern per segment of the batch entry: (start, rows, needle, amp)"""
    return [(0, 1, None, AMP), (5, 1, ('history', 4), AMP), (0, 65, ('chunk', 32), AMP), (130, 70, ('history', 63), AMP),
            (255, 129, ('history', 0), 16.0)]


CHUNK_T_MAX, CHUNK_HEADS, CHUNK_TPS = 1930, 3, 256
CHUNK_ROWS = (1, 5, 16)


def chunk_cap():
    return grid_splits(CHUNK_HEADS, CHUNK_T_MAX)


def chunk_positions(rows):
    """{'one': a single split, 'two': two splits, 'deep': the maximum split count at T_MAX} -> p"""
    return {'one': 40, 'two': 300 - rows, 'deep': CHUNK_T_MAX - rows}


def chunk_needles(p, rows):
    sp = split_ranges(p + rows, chunk_cap(), CHUNK_TPS)
    keys = {0, 31, 32, p - 1}
    if len(sp) > 1:
        keys |= {sp[1][0], sp[1][1] - 1, sp[-1][0], sp[-1][1] - 1}
    hist = sorted(t for t in keys if 0 <= t < p)
    return [('history', t) for t in hist] + [('chunk', j) for j in sorted({0, rows - 1})] + [('self', rows - 1)]


DECODE_T_MAX, DECODE_HEADS = 2048, 4
DECODE_POSITIONS = (5, 129, 769, 1537, 2047)
DECODE_SCALE_POSITIONS = (5, 129, 2047)          # the tiny-context path, one split, the deepest position


def decode_needles(pos, ranges):
    """history needles on the first and last key of every split in `ranges`, at pos - 1 and at key 0, and the token's own key"""
    keys = {0, pos - 1}
    for t0, t1 in ranges:
        keys |= {t0, t1 - 1}
    return [('history', t) for t in sorted(k for k in keys if 0 <= k < pos)] + [('self', 0)]
