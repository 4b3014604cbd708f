"""RoPE cases shared by the host and GPU rope tests (plain numpy, no GPU): the float64 rotation, the per-element bar every kernel is
held to, the formulas a kernel could compute instead without a max-normalised test at base 10000 noticing, and the inputs.

The bar.  The reference kernel and every kernel here form the angle in fp32 as expf(c * inv_base) * pos with
inv_base = -2 logf(base) / hd, take fp32 cos / sin of it, rotate in fp32 and round once to fp16.  For an element of the pair (x, y) at
column c, with theta = pos * base ** (-2 c / hd) and r = hypot(x, y):

    |got - exact| <= 1/2 ulp16(exact) + (rho_c theta + 2^-21) r

    rho_c = (4 a_c + 3) 2^-24,  a_c = 2 c ln(base) / hd

* inv_base carries at most three fp32 roundings (logf, the product with -2, the division) and c * inv_base one more: a relative error
  of 4 x 2^-24 on an argument of magnitude a_c, i.e. an ABSOLUTE error 4 a_c 2^-24 of the exponent's argument, which expf turns into
  a RELATIVE error of the frequency;
* expf within one ulp, the rounding of its result's product with pos: + 3 x 2^-24 (one to spare);
* d(x cos t - y sin t) / dt is bounded by r, so an angle error of rho_c theta moves an output by at most rho_c theta r;
* fp32 cos / sin (about an ulp of a value <= 1), the two products and the sum: 2^-21 r covers them;
* one rounding to fp16: half a spacing of the result, 2^-24 (the subnormal spacing) at the least.

Nothing in it is fitted to a kernel.  At pos <= 300 the second term is a few per cent of the first: the bar is half an fp16 ulp.  At
position 4095 and column 0 (theta = 4095) it reaches (3 x 2^-24) x 4095 r = 7e-4 r: several fp16 ulps of a small element, which is
inherent to the reference's fp32 angle and not a property of any kernel here."""
import numpy as np

from util import fp16_ulp

POSITIONS = (0, 1, 2, 17, 127, 128, 300, 2047, 4095)
LONG_POSITIONS = (8191, 32767)          # entries without a t_max (gptq_rope_f16) only
BASES = (1e4, 5e5, 1e6)
# (heads, head_dim) of the op-level cases: 2 x heads head slots per row
#   (2, 128)   one pass of the 8-wide instance
#   (33, 128)  66 slots at 32 per pass: three passes, the last one ragged
#   (32, 128)  LLaMA-7B: two full passes
#   (3, 64)    the 8-wide instance with 4 column vectors per head
#   (5, 80)    5 column vectors per head: 256 threads are not a multiple of it
#   (4, 100)   OpenLLaMA-3B: half = 50, the 2-wide instance, 25 column vectors, idle tail threads
#   (3, 10)    half = 5: the scalar instance
HEAD_SHAPES = ((2, 128), (33, 128), (32, 128), (3, 64), (5, 80), (4, 100), (3, 10))


def qkv_inputs(shape, heads, hd, seed):
    """fp16 N(0, 1) [*shape, 3, heads, hd] from a seeded generator: q, k and v are separate draws (V is not K)"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(tuple(shape) + (3, heads, hd)).astype(np.float16)
    assert not np.array_equal(a[..., 1, :, :], a[..., 2, :, :])
    return a


def theta_of(pos, c, hd, base):
    """pos * base ** (-2 c / hd) in float64; base is the float32 the kernels receive"""
    b = np.float64(np.float32(base))
    return np.asarray(pos, dtype=np.float64) * b ** (-2.0 * np.asarray(c, dtype=np.float64) / hd)


def exact_rope(x, y, pos, c, hd, base):
    """float64 (ox, oy) of the pair (x, y) = columns (c, c + hd / 2) of a head at position pos (all arguments broadcast)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    t = theta_of(pos, c, hd, base)
    cs, sn = np.cos(t), np.sin(t)
    return x * cs - y * sn, x * sn + y * cs


def rope_bound(x, y, pos, c, hd, base, exact):
    """the per-element bar of the module docstring for an output whose float64 value is `exact`"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    a = 2.0 * np.asarray(c, dtype=np.float64) * np.log(np.float64(np.float32(base))) / hd
    rho = (4.0 * a + 3.0) * 2.0 ** -24
    t = np.abs(theta_of(pos, c, hd, base))
    return 0.5 * fp16_ulp(exact) + (rho * t + 2.0 ** -21) * np.hypot(x, y)


def _split(heads_in, pos, hd):
    """[..., hd] heads and positions of the leading dims -> x, y [..., half], pos [..., 1] (broadcast over trailing head dims), c [half]"""
    a = np.asarray(heads_in)
    assert a.shape[-1] == hd and hd % 2 == 0
    half = hd // 2
    p = np.asarray(pos, dtype=np.float64)
    assert p.shape == a.shape[:p.ndim], (p.shape, a.shape)
    p = p.reshape(p.shape + (1,) * (a.ndim - p.ndim))
    return a[..., :half].astype(np.float64), a[..., half:].astype(np.float64), p, np.arange(half)


def exact_rope_heads(heads_in, pos, hd, base):
    """float64 rotation of an array of heads [..., hd] (rotate-half pairing); pos has the array's leading dims (e.g. [bsz, seq] for
    [bsz, seq, 2, heads, hd])"""
    x, y, p, c = _split(heads_in, pos, hd)
    return np.concatenate(exact_rope(x, y, p, c, hd, base), axis=-1)


def rope_errors(got, x, y, pos, hd, base):
    """(|got - exact|, bound), each [..., hd]: got [..., hd] rotated heads, x / y [..., hd / 2] the unrotated halves, pos broadcastable
    against them"""
    c = np.arange(hd // 2)
    ox, oy = exact_rope(x, y, pos, c, hd, base)
    exact = np.concatenate([ox, oy], axis=-1)
    bound = np.concatenate([rope_bound(x, y, pos, c, hd, base, ox), rope_bound(x, y, pos, c, hd, base, oy)], axis=-1)
    return np.abs(np.asarray(got, dtype=np.float64) - exact), bound


def assert_rope_close(got, x, y, pos, hd, base, name=''):
    """THE judge of every rope test: each element of got [..., hd] within its own bar of the float64 rotation of (x, y) -- elementwise,
    never normalised by a maximum.  Returns the worst err / bound."""
    got = np.asarray(got)
    assert np.isfinite(got.astype(np.float64)).all(), (name, 'not finite')
    err, bound = rope_errors(got, x, y, pos, hd, base)
    ratio = err / bound
    bad = ratio > 1.0
    if bad.any():
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError('%s: %d of %d elements (%.1f %%) beyond the bar, %.1f %% beyond 10 x; worst err/bound %.3g at %s (err %.3e, bound %.3e)'
                             % (name, int(bad.sum()), bad.size, 100.0 * bad.mean(), 100.0 * (ratio > 10.0).mean(), float(ratio[i]), i,
                                float(err[i]), float(bound[i])))
    return float(ratio.max())


def assert_heads_close(got, heads_in, pos, hd, base, name=''):
    """assert_rope_close for arrays of heads [..., hd] with pos over their leading dims"""
    x, y, p, _ = _split(heads_in, pos, hd)
    return assert_rope_close(got, x, y, p, hd, base, name)


def share_beyond(got, heads_in, pos, hd, base, factor=1.0):
    """share of the elements of got further than factor x the bar from the float64 rotation"""
    x, y, p, _ = _split(heads_in, pos, hd)
    err, bound = rope_errors(got, x, y, p, hd, base)
    return float((err > factor * bound).mean())


# ---------------------------------------------------------------------------------------
# what a kernel could compute instead (float64; the signature of exact_rope_heads)
# ---------------------------------------------------------------------------------------
def rope_exponent_c_over_hd(heads_in, pos, hd, base):
    x, y, p, c = _split(heads_in, pos, hd)
    return np.concatenate(exact_rope(x, y, p, c / 2.0, hd, base), axis=-1)


def rope_sine_flipped(heads_in, pos, hd, base):
    x, y, p, c = _split(heads_in, pos, hd)
    return np.concatenate(exact_rope(x, y, -p, c, hd, base), axis=-1)


def rope_pos_plus_one(heads_in, pos, hd, base):
    return exact_rope_heads(heads_in, np.asarray(pos) + 1, hd, base)


def rope_base_ignored(heads_in, pos, hd, base):
    return exact_rope_heads(heads_in, pos, hd, 10000.0)


def rope_interleaved(heads_in, pos, hd, base):
    """pairs (2c, 2c + 1) instead of (c, c + hd / 2)"""
    a = np.asarray(heads_in, dtype=np.float64)
    p = _split(heads_in, pos, hd)[2]
    ox, oy = exact_rope(a[..., 0::2], a[..., 1::2], p, np.arange(hd // 2), hd, base)
    out = np.empty_like(a)
    out[..., 0::2], out[..., 1::2] = ox, oy
    return out


def rope_row0_position(heads_in, pos, hd, base):
    """every batch row takes the positions of batch row 0 (pos [bsz, seq]); a 1-D pos: every row takes pos[0]"""
    p = np.asarray(pos)
    return exact_rope_heads(heads_in, np.broadcast_to(p[:1], p.shape), hd, base)


def rope_fp16_trig(heads_in, pos, hd, base):
    """cos / sin rounded to fp16 before the multiply"""
    x, y, p, c = _split(heads_in, pos, hd)
    t = theta_of(p, c, hd, base)
    cs, sn = np.cos(t).astype(np.float16).astype(np.float64), np.sin(t).astype(np.float16).astype(np.float64)
    return np.concatenate([x * cs - y * sn, x * sn + y * cs], axis=-1)


WRONG_FORMULAS = (rope_exponent_c_over_hd, rope_sine_flipped, rope_pos_plus_one, rope_base_ignored, rope_interleaved, rope_row0_position,
                  rope_fp16_trig)


def bit_equal_share(a, b):
    """share of fp16 elements with the same bits (a measurement, never a bar: device and host expf may differ by an ulp)"""
    a, b = np.ascontiguousarray(a, dtype=np.float16), np.ascontiguousarray(b, dtype=np.float16)
    return float((a.view(np.uint16) == b.view(np.uint16)).mean())


def exact_attention(q_rot, K, V, scale):
    """float64 softmax attention of ONE query per head: q_rot [heads, hd], K / V [n, heads, hd] -> [heads, hd]"""
    q, K, V = (np.asarray(t, dtype=np.float64) for t in (q_rot, K, V))
    s = np.einsum('hd,nhd->hn', q, K) * scale
    s -= s.max(axis=1, keepdims=True)
    e = np.exp(s)
    return np.einsum('hn,nhd->hd', e / e.sum(axis=1, keepdims=True), V)
