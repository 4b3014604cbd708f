"""Every kernel family of the stripe16 matmul path (csrc/stripe_mm.inc, csrc/stripe_kernel.inc) on data where the answer is EXACT.

The parity tests hold these kernels to 1e-3 against the oracle, or compare them with themselves: a wrong magic-offset class for one pair of one
bit width fails them, but two roundings of an epilogue in the wrong order can stay under the bar.  Here the data (util.exact_domain_case: power-of-two
scales, integer x) makes every product and every partial sum, in any order, exact in fp32, so the only roundings left are the one or two fp16
roundings of the epilogue and the result is known bit for bit:
  * one weight set: y == fp16(float64 result), rounded once; with a bias (ldb == 0) or a residual row (ldb != 0) b: fp16(float32(h) + float32(b)) of
    that rounded h;
  * a gate | up pair: SiLU runs on __expf under fast-math, so the bar of test_stripe_mm_fused_mlp against oracle.fused_mlp and the float64 result,
    plus bit equality of two runs.
One case per kernel family the two dispatch ladders can reach; each is placed by the ladder's own predicates, which are fixed numbers (256 CUs,
cw = ceil(N / 16 / 256) rounds of stripes, tm = ceil(M / 16) row tiles) and stand as a comment beside the case.  The cases are placed by that
arithmetic ALONE: the C ABI has no entry that tells which kernel a launch took, so nothing here asserts that the named kernel ran -- whoever changes a
ladder moves these cases with it, or they silently test another route (their assertions hold on every route).  K is five row blocks (640 for 3 / 4 / 8
bits, 1280 for 2 bits) unless the route needs a long K.  A K that is no multiple of the row block (672 for 4 bits) has no stripe16 image at all -- pinned
by test_ragged_k_has_no_image -- so the 4-bit instances of `stripe_mm3w4` cannot be reached: with an image, x is aligned for the loader / consumer
kernel, whose predicate covers theirs; the 3-bit case runs that kernel.
The whole file: 56 cases, 8.7 s on an MI355X (import and library load included; the slowest case, the pair as two launches on N = 12288, 0.9 s)."""
import numpy as np
import pytest
import torch

import quant
from quant import quant_linear as QL
from quant import _native
from quant.layer import prepared
from oracle import oracle
from util import TOL, exact_domain_case, rel_err, assert_not_worse_than_reference

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _x_max(bits):
    return 1 if bits == 8 else 4          # 8-bit fields reach 255: |x| <= 1 keeps the sums inside the exact range (exact_domain_case asserts it)


def _k5(bits):
    return 1280 if bits == 2 else 640     # five row blocks (BK = 256 / 128 / 128 / 64 k)


def _sets(Ls):
    return [(L['qweight'], L['scales'], L['qzeros'], L['g_idx']) for L in Ls]


def _once(x, L):
    """fp16(float64 result): the one rounding"""
    return oracle.matmul248_exact(x, L['qweight'], L['scales'], L['qzeros'], L['g_idx'], int(L['bits'])).astype(np.float16)


def _plus(h, b):
    """the second rounding: fp16(float32(h) + float32(b)) on the rounded h"""
    return (h.astype(np.float32) + np.asarray(b, dtype=np.float16).astype(np.float32)).astype(np.float16)


def _eighths(rng, shape):
    return (rng.integers(-16, 17, size=shape) / 8.0).astype(np.float16)


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    bad = a.view(np.uint16) != b.view(np.uint16)
    print('%s: %d of %d elements differ' % (what, int(bad.sum()), bad.size))
    assert not bad.any(), (what, int(bad.sum()), a[bad][:4], b[bad][:4])


def _pair_bar(c, c2, x, Ls, bits, what):
    sets = _sets(Ls)
    ref = oracle.fused_mlp(x, sets[0], sets[1], bits)
    print('%s: rel err %.3e' % (what, rel_err(c, ref)))
    assert rel_err(c, ref) < TOL
    assert_not_worse_than_reference(c, ref, oracle.fused_mlp_exact(x, sets[0], sets[1], bits))
    _same_bits(c, c2, what + ' (second run)')


def _tiles(x, L, bias=None):
    """gptq_stripe_matmul_f16: the ladder of stripe_mm_dispatch (M <= 128) / stripe_gemm_dispatch (above)"""
    y = QL.matmul248(dev(x), dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), dev(L['g_idx']), int(L['bits']), 2 ** int(L['bits']) - 1,
                     bias=None if bias is None else dev(bias), family='stripe_mm')
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _tiles_pair(x, Ls, bits, gs):
    gate, up = (tuple(dev(t) for t in s) for s in _sets(Ls))
    c = quant.fused_mlp.fused_gate_up(dev(x), gate, up, bits, gs, family='stripe_mm')
    torch.cuda.synchronize()
    return c.cpu().numpy()


TILE_CASES = [
    # bits, gs, K, N, M, split_k (None: the ladder decides), route and the predicate that places the case there
    (4, 128, 640, 8192, 17, None),     # stripe_mmr C = 2: cw == 2, 2 <= tm <= 8, K <= 8192, one set
    (4, 128, 640, 8192, 128, None),    # stripe_mmr C = 2, eight row tiles (row halves): tm == 8, K <= 6144
    (4, 128, 640, 12288, 40, None),    # stripe_mmr C = 3: cw == 3, tm == 3
    (4, 128, 6272, 3584, 17, None),    # stripe_mmr in four K slices + mmr_combine: 192 < 224 stripes <= 256, 6144 < K <= 16384, tm == 2
    (3, 128, 640, 8192, 40, None),     # stripe_mm3w4 C = 2 (3 bits have no loader / consumer kernel): cw == 2, 3 <= tm <= 6, K <= 6144
    (4, 128, 640, 8192, 5, None),      # stripe_mm3c C = 2: cw == 2, tm == 1 (the loader / consumer kernel starts at tm == 2)
    (4, 128, 640, 8192, 16, None),     # stripe_mm3c C = 2, a full row tile
    (4, 128, 640, 512, 17, None),      # stripe_mm3: 32 stripes <= 256 and K <= 6144 (one round, short K), tm == 2
    (4, 128, 640, 512, 100, None),     # stripe_mm3, seven row tiles (the PFL instance)
    (8, 64, 640, 8192, 9, None),       # stripe_mm1 <1, 1, 2>: 8 bits (no C-stripe routes), 512 stripes > 256 so not stripe_mm3, tm == 1 and stripes <= 1024
    (4, 128, 640, 512, 16, 0),         # stripe_mm1: gptq_set_split_k(0) asks for the single launch, tm == 1
    (4, 128, 640, 512, 40, 0),         # stripe_mm2 <3, 1>: gptq_set_split_k(0), tm == 3
    (4, 128, 640, 512, 17, 0),         # stripe_mm2 <2, 1>: gptq_set_split_k(0), tm == 2
    (4, 128, 640, 512, 64, 0),         # stripe_mm2 <4, 1>: gptq_set_split_k(0), tm == 4
    (4, 128, 640, 512, 16, 4),         # stripe_mm_kernel <1, 1, false> + stripe_mm_reduce_kernel: gptq_set_split_k(4) -> three slices of two row blocks
    (4, 32, 640, 512, 16, None),       # stripe_mm_kernel <1, 1, true> (prescale) + reduce: the group (32) is smaller than the row block (128)
    (2, 128, 1280, 512, 16, None),     # ... prescale, 2 bits: the group (128) is smaller than the 2-bit row block (256)
    (3, 32, 640, 512, 16, None),       # ... prescale, 3 bits at groupsize 32
    (3, 128, 640, 512, 16, 4),         # stripe_mm_kernel <1, 1, false>, 3 bits at groupsize 128 (the group IS the row block: no prescale), forced slices
    (8, 64, 640, 8192, 80, None),      # stripe_gemm_kernel <1, 4> in K slices + reduce: tm == 5 and 512 stripes (not one round), ten row blocks >= 8
    (4, 128, 640, 512, 129, None),     # stripe_gemm_kernel <1, 4>, 128-row tiles: M > 128; 4 column groups x 2 row tiles: r4 == r8 == 1
    (4, 128, 640, 11008, 300, None),   # stripe_gemm_kernel <1, 8>, 256-row tiles (prescaled operands): 86 groups x 3 tiles = 2 rounds against 86 x 2 = 1: 7 r8 < 4 r4
]


@pytest.mark.parametrize('bits,gs,K,N,M,split_k', TILE_CASES)
def test_tile_routes_one_set(bits, gs, K, N, M, split_k):
    """y == fp16(float64 result) bit for bit, and with a bias the second rounding on the rounded value, on every tile route of one weight set"""
    (L,), x = exact_domain_case(bits, gs, K, N, M, seed=N + M, x_max=_x_max(bits))
    bias = _eighths(np.random.default_rng(M), N)
    lib = _native.lib()
    prev = lib.gptq_set_split_k(split_k) if split_k is not None else None
    try:
        y = _tiles(x, L)
        yb = _tiles(x, L, bias)
    finally:
        if split_k is not None:
            lib.gptq_set_split_k(prev)
    h = _once(x, L)
    _same_bits(y, h, 'plain')
    _same_bits(yb, _plus(h, bias[None, :]), 'bias')


PAIR_CASES = [
    (4, 128, 640, 8192, 40),       # stripe_mmr pair (consumers split by set), C = 2: cw == 2, tm == 3, K <= 6144
    (4, 128, 640, 12288, 128),     # stripe_mmr pair, C = 3 and tm == 8: TWO launches of the four-tile instance, rows 0 .. 63 and 64 .. 127
    (4, 128, 640, 8192, 9),        # stripe_mm3c pair (gate and up take turns), C = 2: cw == 2, tm == 1
    (4, 128, 640, 512, 20),        # stripe_mm3 pair: one round, short K, tm == 2
    (4, 128, 640, 512, 130),       # stripe_gemm_kernel <2, 4>: M > 128, 8 column groups of four stripes
]


@pytest.mark.parametrize('bits,gs,K,N,M', PAIR_CASES)
def test_tile_routes_pair(bits, gs, K, N, M):
    Ls, x = exact_domain_case(bits, gs, K, N, M, nsets=2, seed=N + M)
    _pair_bar(_tiles_pair(x, Ls, bits, gs), _tiles_pair(x, Ls, bits, gs), x, Ls, bits, 'pair')


def test_ragged_k_has_no_image():
    """K = 672 is no multiple of the 4-bit row block (128 k): the layer has no stripe16 image, so no kernel of this file ever sees a ragged K"""
    assert _native.lib().gptq_stripe_bytes(672, 512, 4, 32, 1) == 0
    assert _native.lib().gptq_stripe_bytes(640, 512, 4, 32, 1) > 0


# ---- the decode launches (csrc/stripe_kernel.inc) through gptq_stripe_matvec_f16 / gptq_layer_decode_f16 ----

def _image(Ls, bits, gs, K, N, bias=None):
    sets = tuple(tuple(dev(t) for t in s) for s in _sets(Ls))
    return prepared(sets, None if bias is None else dev(bias), bits, gs, K, N), sets


def _matvec(pl, x, K, N, bits, gs, nsets, bias=None):
    out = torch.full((x.shape[0], N), float('nan'), dtype=torch.float16, device=DEV)
    QL.stripe_matvec(dev(x), pl.stripe, out, K, N, bits, gs, nsets=nsets, bias=None if bias is None else dev(bias))
    torch.cuda.synchronize()
    return out.cpu().numpy()


DECODE_CASES = [(bits, 128 if bits != 8 else 64, _k5(bits), 512, M, 1) for bits in (2, 3, 4, 8) for M in (1, 4, 8)] + [   # stripe_gemv_kernel: 32 stripes, MR = 1 / 4 / 8
    # (5 .. 8 rows of 3 / 4 / 8 bits: stripe_mf8_ok -> stripe_gemvc_kernel <C = 1, MF>; 2 bits keep the 4x4x4 row groups of stripe_gemv_kernel)
    (4, 128, 9344, 512, 5, 1),      # stripe_gemv2p_kernel <MF>: 9216 < NU 8 BK (NU = 10: 10240) <= 12288 -- the shortest K is 73 row blocks; eight rows of it do not fit LDS
    (4, 128, 9344, 512, 8, 1),
    (4, 128, 640, 8192, 2, 1),      # 512 stripes are NOT more than 512: stripe_gemv_kernel, MR = 4
    (4, 128, 640, 12288, 2, 1),     # stripe_gemvc_kernel C = 3, MR = 4: 768 stripes > 512, c == 3
    (4, 128, 640, 12288, 4, 1),
    (4, 128, 640, 8192, 9, 1),      # stripe_gemvc_kernel <MF, MR = 16> (deferred epilogue), C = 2: 9 .. 16 rows, K <= 4096
    (4, 128, 640, 8192, 16, 1),
    (4, 128, 640, 12288, 9, 1),     # ... C = 3
    (4, 128, 640, 12288, 16, 1),
    (4, 128, 640, 12288, 4, 2),     # pairs: stripe_gemvc_kernel C = 3, MR = 4
    (4, 128, 640, 8192, 2, 2),      # stripe_gemv_kernel pair, MR = 4
    (4, 128, 640, 8192, 9, 2),      # stripe_gemvc_kernel <MF, MR = 16> pair, C = 2
    (4, 128, 640, 12288, 16, 2),    # ... C = 3
]


@pytest.mark.parametrize('bits,gs,K,N,M,nsets', DECODE_CASES)
def test_decode_routes(bits, gs, K, N, M, nsets):
    Ls, x = exact_domain_case(bits, gs, K, N, M, nsets=nsets, seed=N + M + bits, x_max=_x_max(bits))
    pl, _keep = _image(Ls, bits, gs, K, N)
    y = _matvec(pl, x, K, N, bits, gs, nsets)
    if nsets == 2:
        _pair_bar(y, _matvec(pl, x, K, N, bits, gs, nsets), x, Ls, bits, 'decode pair')
        return
    h = _once(x, Ls[0])
    _same_bits(y, h, 'plain')
    bias = _eighths(np.random.default_rng(M), N)
    _same_bits(_matvec(pl, x, K, N, bits, gs, 1, bias), _plus(h, bias[None, :]), 'bias')


def test_decode_act_order():
    """stripe_gemv_kernel <XPERM>: the image of the group-sorted rows, x gathered through the permutation (one row; no fused norm: rsqrt is not exact)"""
    bits, gs, K, N = 4, 128, 640, 512
    (L,), x = exact_domain_case(bits, gs, K, N, 1, act_order=True, seed=5)
    y = QL.matmul248(dev(x), dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), dev(L['g_idx']), bits, 15, family='stripe')
    torch.cuda.synchronize()
    _same_bits(y.cpu().numpy(), _once(x, L), 'act-order')


@pytest.mark.parametrize('M', [4, 40])      # stripe_gemv_kernel MR = 4 (bias_pre read through ldb); 16-row tiles (finish_tile's ldb != 0 branch)
def test_residual_row(M):
    """gptq_layer_decode_f16 with a residual and no norm: y == fp16(float32(fp16(sum)) + float32(residual)), on a decode kernel and on a tile kernel"""
    bits, gs, K, N = 4, 128, 640, 512
    (L,), x = exact_domain_case(bits, gs, K, N, M, seed=40 + M)
    res = _eighths(np.random.default_rng(M), (M, N))
    pl, _keep = _image([L], bits, gs, K, N)
    lib = _native.lib()
    s = _native.stream_ptr(torch.device(DEV))
    ws = _native.layer_workspace(torch.device(DEV), s)
    scratch = torch.empty(max(lib.gptq_layer_decode_scratch_bytes(pl.handle, M), 256), dtype=torch.uint8, device=DEV)
    xd, rd = dev(x), dev(res)
    y = torch.full((M, N), float('nan'), dtype=torch.float16, device=DEV)
    rc = lib.gptq_layer_decode_f16(pl.handle, xd.data_ptr(), xd.stride(0), y.data_ptr(), y.stride(0), M, None, 1e-6, rd.data_ptr(), rd.stride(0), ws.data_ptr(),
                                   ws.numel(), scratch.data_ptr(), scratch.numel(), s)
    _native.check(rc, 'gptq_layer_decode_f16')
    torch.cuda.synchronize()
    _same_bits(y.cpu().numpy(), _plus(_once(x, L), res), 'residual')
