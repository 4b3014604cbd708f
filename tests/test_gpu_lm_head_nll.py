"""GPU tests of gptq_lm_head_nll_f16 (csrc/gemm8.hip, cross-entropy epilogue): the LM head of many rows that never writes the logits.

Reference: float64 on the same fp16 inputs, z64 = x64 . W64^T (+ bias), nll64 = logsumexp(z64) - z64[target].
Bar: |nll - nll64| <= 2e-3 max(1, max_n |z64|) per row, the same for lse: the project's op bar of 1e-3 on the logits (tests/util.py TOL), carried
through log-sum-exp (1-Lipschitz in the max norm) and the target logit (the same error once more).  The fp16-logit route itself (a float32 product
rounded to fp16) stays at <= 0.28 of this bar on these shapes and activation kinds (checked on the CPU, 33 x 256 x 1000 .. 300 x 256 x 2049).
Not worse than the plain route: per row, the distance from nll64 may exceed that of torch's own fp16 route (matmul -> fp16 -> fp32 cross-entropy)
by at most 2^-10 max(1, max |z64|): one fp16 spacing at the row's largest logit, plus order noise."""
import functools
import math

import pytest
import torch

from quant import _native
from util import activations

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAR = 2e-3
SLACK = 2.0 ** -10
KINDS = ('outliers', 'massive_row', 'tiny')
SIGMAS = (0.02, 0.1, 0.3)
MS, NS, KS = (1, 33, 193, 257), (257, 513, 1000, 2049), (128, 384)
IGNORE = -100


def _cases():
    """every M, N, K, kind and sigma appears; padded rows (ldx = K + 8, ldw = K + 16) in a third of the cases; 24 cases, not the cross product"""
    out = []
    for im, M in enumerate(MS):
        for jn, N in enumerate(NS):
            i = len(out)
            out.append((M, N, KS[(im + jn) % 2], KINDS[(im + 2 * jn) % 3], SIGMAS[(2 * im + jn) % 3], i % 3 == 0))
    for i, (M, N) in enumerate([(257, 2049), (1, 257), (193, 1000), (33, 513), (257, 257), (1, 2049), (33, 1000), (193, 2049)]):
        out.append((M, N, KS[i % 2], KINDS[i % 3], SIGMAS[(i + 1) % 3], i % 2 == 1))
    return out


def _padded(t, ld):
    """the same values as rows of a wider allocation (row stride ld elements)"""
    buf = torch.zeros((t.shape[0], ld), dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def _inputs(M, N, K, kind, sigma, pad, seed, bias=False):
    x = torch.from_numpy(activations(kind, M, K, seed)).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(1000 + seed)
    W = (sigma * torch.randn((N, K), device=DEV, generator=g)).half()
    b = None
    if bias:
        b = (sigma * math.sqrt(K) * torch.randn(N, device=DEV, generator=g)).half()      # of the logits' own magnitude
    if pad:
        x, W = _padded(x, K + 8), _padded(W, K + 16)
    return x, W, b


def _targets(M, N, seed, bad=False):
    """random targets with, as far as M rows allow, column 0, column N - 1, both sides of the first tile seam, one ignored row (and one = N)"""
    g = torch.Generator(device=DEV).manual_seed(2000 + seed)
    t = torch.randint(0, N, (M,), device=DEV, generator=g)
    special = [0, N - 1, 255, 256, IGNORE] + ([N] if bad else [])
    if M == 1:
        t[0] = special[seed % 4]
    else:
        rows = torch.randperm(M, device=DEV, generator=g)[:len(special)].tolist()
        for r, v in zip(rows, special):
            t[r] = v
    return t


def _run(x, W, b, t, want_lse=True, want_arg=True, fill=None):
    """one call of the entry -> (nll, lse or None, argmax or None); fill: the byte the workspace and the outputs hold before the call"""
    lib = _native.lib()
    M, K = x.shape
    N = W.shape[0]
    need = lib.gptq_lm_head_nll_workspace_bytes(M, N)
    assert need >= M * ((N + 255) // 256) * 16
    byte = 0 if fill is None else fill
    ws = torch.full((need,), byte, dtype=torch.uint8, device=DEV)
    outs = torch.full((3, M, 4), byte, dtype=torch.uint8, device=DEV)
    nll, lse, arg = outs[0].view(torch.float32).view(M), outs[1].view(torch.float32).view(M), outs[2].view(torch.int32).view(M)
    rc = lib.gptq_lm_head_nll_f16(x.data_ptr(), x.stride(0), W.data_ptr(), W.stride(0), _native.ptr(b), t.data_ptr(), nll.data_ptr(),
                                  lse.data_ptr() if want_lse else None, arg.data_ptr() if want_arg else None, M, N, K, ws.data_ptr(), ws.numel(),
                                  torch.cuda.current_stream().cuda_stream)
    _native.check(rc, 'gptq_lm_head_nll_f16')
    torch.cuda.synchronize()
    return nll, (lse if want_lse else None), (arg if want_arg else None)


def _reference(x, W, b, t):
    """float64 on the same fp16 inputs: z64, lse64, nll64 (ignored rows 0, out-of-range rows NaN), and the nll of torch's own fp16 route"""
    N = W.shape[0]
    z = x.double() @ W.double().t()
    z16 = torch.matmul(x, W.t())
    if b is not None:
        z = z + b.double()
        z16 = z16 + b
    lse = torch.logsumexp(z, dim=1)
    ok = (t >= 0) & (t < N)
    tc = t.clamp(0, N - 1)
    nll = lse - z.gather(1, tc[:, None])[:, 0]
    nll = torch.where(t < 0, torch.zeros_like(nll), torch.where(ok, nll, torch.full_like(nll, float('nan'))))
    z32 = z16.float()
    plain = torch.logsumexp(z32, dim=1) - z32.gather(1, tc[:, None])[:, 0]
    return z, lse, nll, plain.double()


def _check(x, W, b, t, name):
    N = W.shape[0]
    nll, lse, arg = _run(x, W, b, t)
    z, lse64, nll64, plain = _reference(x, W, b, t)
    zmax = z.abs().max(dim=1).values.clamp(min=1.0)
    live = (t >= 0) & (t < N)
    e_nll = (nll.double() - nll64).abs()[live]
    e_lse = (lse.double() - lse64).abs()
    e_plain = (plain - nll64).abs()[live]
    print('%s: max |z| %.3g, nll err %.3e of bar, lse err %.3e of bar, excess over the plain route %.3e of slack' % (
        name, float(zmax.max()), float((e_nll / (BAR * zmax[live])).max()) if live.any() else 0.0, float((e_lse / (BAR * zmax)).max()),
        float(((e_nll - e_plain) / (SLACK * zmax[live])).max()) if live.any() else 0.0))
    assert bool((e_nll <= BAR * zmax[live]).all()), name
    assert bool((e_lse <= BAR * zmax).all()), name
    assert bool((e_nll <= e_plain + SLACK * zmax[live]).all()), name
    assert bool((nll[t < 0] == 0.0).all()), name                                # an ignored row: 0.0 exactly
    assert bool(torch.isnan(nll[t >= N]).all()), name                           # a target past the head: NaN, the other rows unaffected
    assert bool(torch.isfinite(nll[live]).all()), name
    assert bool(((arg >= 0) & (arg < N)).all()), name
    zarg = z.gather(1, arg.long()[:, None])[:, 0]
    assert bool((zarg >= z.max(dim=1).values - BAR * zmax).all()), name
    return nll, lse, arg


@pytest.mark.parametrize('M,N,K,kind,sigma,pad', _cases())
def test_lm_head_nll_against_float64(M, N, K, kind, sigma, pad):
    seed = M + N + K
    x, W, b = _inputs(M, N, K, kind, sigma, pad, seed)
    _check(x, W, b, _targets(M, N, seed), 'M %d N %d K %d %s sigma %g%s' % (M, N, K, kind, sigma, ' padded' if pad else ''))


def test_lm_head_nll_cases_cover_every_value():
    cs = _cases()
    assert len(cs) == len(set(cs)) == 24
    assert {c[0] for c in cs} == set(MS) and {c[1] for c in cs} == set(NS) and {c[2] for c in cs} == set(KS)
    assert {c[3] for c in cs} == set(KINDS) and {c[4] for c in cs} == set(SIGMAS) and any(c[5] for c in cs) and not all(c[5] for c in cs)


def test_lm_head_nll_target_past_the_head_gives_nan():
    M, N, K = 33, 1000, 128
    x, W, b = _inputs(M, N, K, 'outliers', 0.1, True, 7)
    t = _targets(M, N, 7, bad=True)
    assert int((t == N).sum()) == 1 and int((t == IGNORE).sum()) == 1
    nll, lse, arg = _check(x, W, b, t, 'target = N')
    good = t.clone()
    good[t == N] = 3
    nll2, lse2, arg2 = _run(x, W, b, good)
    keep = t != N
    assert torch.equal(nll[keep].view(torch.int32), nll2[keep].view(torch.int32))          # the other rows: the same bits
    assert torch.equal(lse.view(torch.int32), lse2.view(torch.int32)) and torch.equal(arg, arg2)


def test_lm_head_nll_bias():
    for (M, N, K, pad) in ((33, 1000, 128, False), (193, 2049, 384, True)):
        x, W, b = _inputs(M, N, K, 'outliers', 0.1, pad, 11, bias=True)
        _check(x, W, b, _targets(M, N, 11), 'bias M %d N %d K %d' % (M, N, K))


def test_lm_head_nll_zero_rows():
    """an all-zero x row: every logit is 0, so nll = lse = log N and the first column wins -- padded columns must not reach the sum"""
    for N in (257, 1000, 2049):
        M, K = 33, 128
        x, W, _ = _inputs(M, N, K, 'outliers', 0.3, False, 5)
        x[3].zero_()
        x[32].zero_()
        t = _targets(M, N, 5)
        t[3], t[32] = N - 1, 17
        nll, lse, arg = _run(x, W, None, t)
        for r in (3, 32):
            assert abs(float(lse[r]) - math.log(N)) <= 1e-6 * math.log(N), (N, r, float(lse[r]))
            assert abs(float(nll[r]) - math.log(N)) <= 1e-6 * math.log(N), (N, r, float(nll[r]))
            assert int(arg[r]) == 0, (N, r, int(arg[r]))


def test_lm_head_nll_planted_winners():
    """one weight row scaled up along a row of x: that column is returned exactly, at the first and last column and on both sides of a tile seam"""
    M, N, K, sigma = 33, 1000, 384, 0.05
    x, W, _ = _inputs(M, N, K, 'massive_row', sigma, False, 13)                  # ordinary rows (the massive one is row 16): nearly orthogonal
    plant = {2: 0, 9: 255, 17: 256, 30: N - 1}
    for r, c in plant.items():
        v = x[r].float()
        W[c] = (10.0 * sigma * v / v.norm()).half()
    nll, lse, arg = _check(x, W, None, _targets(M, N, 13), 'planted winners')
    z = x.double() @ W.double().t()
    for r, c in plant.items():
        top2 = torch.topk(z[r], 2).values
        assert int(torch.argmax(z[r])) == c and float(top2[0] - top2[1]) > 10 * BAR * float(z[r].abs().max())      # a clear winner
        assert int(arg[r]) == c, (r, c, int(arg[r]))


def test_lm_head_nll_workspace_independence():
    M, N, K = 193, 2049, 128
    x, W, b = _inputs(M, N, K, 'massive_row', 0.1, False, 17)
    t = _targets(M, N, 17)
    clean = _run(x, W, b, t)
    first = _run(x, W, b, t, fill=0xFF)
    second = _run(x, W, b, t, fill=0xFF)
    for a, c, d in zip(clean, first, second):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)) and torch.equal(c.view(torch.int32), d.view(torch.int32))


def test_lm_head_nll_row_independence():
    """a row's bits depend neither on M nor on the row's place: row r of an M = 257 call, alone (M = 1), and at another position of an M = 33 call"""
    M, N, K = 257, 1000, 384
    x, W, b = _inputs(M, N, K, 'outliers', 0.1, True, 19)
    t = _targets(M, N, 19)
    small = torch.from_numpy(activations('outliers', 33, K, 23)).to(DEV)
    ts = _targets(33, N, 23)
    places = ((5, 20), (200, 0), (256, 32))                                     # (row of the large call, its row in the M = 33 call)
    t[5], t[200], t[256] = 255, 256, N - 1
    nll, lse, arg = _run(x, W, b, t)
    for r, at in places:
        alone = _run(x[r:r + 1].contiguous(), W, b, t[r:r + 1].clone())
        xs, t2 = small.clone(), ts.clone()
        xs[at], t2[at] = x[r], t[r]
        moved = _run(xs, W, b, t2)
        for full, a, m in zip((nll, lse, arg), alone, moved):
            assert torch.equal(full[r:r + 1].view(torch.int32), a.view(torch.int32)), r
            assert torch.equal(full[r:r + 1].view(torch.int32), m[at:at + 1].view(torch.int32)), (r, at)


def test_lm_head_nll_optional_outputs():
    M, N, K = 33, 513, 128
    x, W, b = _inputs(M, N, K, 'tiny', 0.3, False, 29)
    t = _targets(M, N, 29)
    nll = _run(x, W, b, t)[0]
    for want_lse, want_arg in ((False, False), (True, False), (False, True)):
        got = _run(x, W, b, t, want_lse=want_lse, want_arg=want_arg)
        assert got[1] is (None if not want_lse else got[1]) and torch.equal(got[0].view(torch.int32), nll.view(torch.int32))
