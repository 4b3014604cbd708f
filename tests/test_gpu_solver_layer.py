"""GPU tests of gptq_solver_layer_f32 (csrc/gptq_solver.hip): the GPTQ solve step of a whole layer in one launch -- per 128-column block the
grid fit, the column loop and the trailing update on the fp32 matrix instruction -- and of its dispatch in GPTQ.fasterquant.  A tile is 16
rows and a strip of the trailing update 32 columns: rows 1 / 33 / 40 / 72 / 130 are no multiple of the tile, 384 columns are three blocks (the
update of block 0 has 8 strips, that of block 1 four), 512 give the first update exactly one strip per wave."""
import numpy as np
import pytest
import torch

import gptq as product_gptq
import quant
from quant import _native

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def solve(W, Hinv, gs, maxq, sym, fit, scale=None, zero=None):
    """one call of the entry on fresh device copies: (Q, scale, zero, loss_rows, W afterwards), all on the CPU"""
    rows, cols = W.shape
    ng = -(-cols // gs)
    Wd, Hd = W.to(DEV).contiguous(), Hinv.to(DEV).contiguous()
    sd = torch.zeros((rows, ng), device=DEV) if scale is None else scale.to(DEV).contiguous()
    zd = torch.zeros((rows, ng), device=DEV) if zero is None else zero.to(DEV).contiguous()
    Q, loss = torch.full((rows, cols), 99.0, device=DEV), torch.full((rows,), 99.0, device=DEV)
    rc = _native.lib().gptq_solver_layer_f32(Wd.data_ptr(), cols, Hd.data_ptr(), cols, rows, cols, gs, maxq, int(sym), int(fit), sd.data_ptr(),
                                             zd.data_ptr(), ng, Q.data_ptr(), cols, loss.data_ptr(), _native.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    return Q.cpu(), sd.cpu(), zd.cpu(), loss.cpu(), Wd.cpu()


@pytest.mark.parametrize('rows', [1, 40, 72])
def test_exact_against_float64(rows):
    """W = integers / 64, Hinv unit upper triangular with three +-1 per row anywhere to the right, grid (0.125, 8): every fp32 operation is
    exact, so any summation order gives the bits of the float64 loop below (the reference's column loop and per-block trailing update)"""
    cols, maxq, sc, zp = 384, 15, 0.125, 8.0
    rng = np.random.default_rng(rows)
    W = rng.integers(-64, 65, (rows, cols)) / 64.0
    Hinv = np.eye(cols)
    for i in range(cols - 1):
        right = rng.choice(np.arange(i + 1, cols), min(3, cols - 1 - i), replace=False)
        Hinv[i, right] = rng.choice([-1.0, 1.0], len(right))
    Wr, Qr, loss = W.copy(), np.zeros((rows, cols)), np.zeros(rows)
    for i1 in range(0, cols, 128):
        W1, Err = Wr[:, i1:i1 + 128].copy(), np.zeros((rows, 128))
        for i in range(128):
            w, d = W1[:, i], Hinv[i1 + i, i1 + i]
            q = sc * (np.clip(np.rint(w / sc) + zp, 0, maxq) - zp)
            Qr[:, i1 + i], Err[:, i] = q, (w - q) / d
            loss += (w - q) ** 2 / d ** 2 * 0.5
            W1[:, i:] -= np.outer(Err[:, i], Hinv[i1 + i, i1 + i:i1 + 128])
        Wr[:, i1 + 128:] -= Err @ Hinv[i1:i1 + 128, i1 + 128:]
    grid = torch.full((rows, 1), sc), torch.full((rows, 1), zp)
    Q, _, _, lr, Wa = solve(torch.from_numpy(W).float(), torch.from_numpy(Hinv).float(), cols, maxq, False, False, *grid)
    assert np.array_equal(Q.numpy(), Qr), int((Q.numpy() != Qr).sum())
    assert np.array_equal(Wa.numpy(), Wr) and np.array_equal(lr.numpy(), loss)


def _levels(Q, scale, zero, g_idx):
    return np.rint(Q / scale[:, g_idx]) + zero[:, g_idx]


def _layer(rows, cols, seed):
    """(W, H, n) as test_gpu_solver_block_kernel_is_bit_exact_given_the_reference_inverse_factor builds them"""
    from oracle import gptq_solver as G
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((rows, cols)) * 0.05).astype(np.float32)
    mix = (rng.standard_normal((cols, cols)) * 0.1 + np.eye(cols)).astype(np.float32)
    X = (rng.standard_normal((512, cols)).astype(np.float32) @ mix) * np.exp(rng.standard_normal(cols) * 0.5).astype(np.float32)
    H, n = G.hessian_add_batch(np.zeros((cols, cols), np.float32), 0, X[None])
    return W, H, n


def _fasterquant(W, H, n, bits, sym=False, mse=False, perchannel=True, **kw):
    layer = torch.nn.Linear(W.shape[1], W.shape[0], bias=False)
    layer.weight.data = torch.from_numpy(W).clone()
    layer = layer.to(DEV)
    g = product_gptq.GPTQ(layer)
    g.quantizer.configure(bits, perchannel=perchannel, sym=sym, mse=mse)
    g.H, g.nsamples = torch.from_numpy(H).to(DEV), n
    scale, zero, g_idx, err = g.fasterquant(percdamp=0.01, name='t', **kw)
    return layer.weight.data.float().cpu().numpy(), scale.cpu().numpy(), zero.cpu().numpy(), g_idx.cpu().numpy(), err


@pytest.mark.parametrize('rows,cols,bits,gs,act,sym', [(72, 384, 4, 128, False, False), (40, 384, 4, 32, True, False), (33, 256, 3, 256, False, False),
                                                        (64, 384, 2, 192, False, True), (16, 256, 8, -1, False, False), (130, 512, 4, 64, True, False)])
def test_fasterquant_against_the_cpu_restatement(monkeypatch, rows, cols, bits, gs, act, sym):
    """only the solver differs: the inverse factor is the oracle's on both sides.  The bounds are those of test_gpu_gptq_solver_vs_cpu_restatement
    for the same quantity; the parent route (_solve_blocks) is run on the same inputs and printed next to the new one."""
    from oracle import gptq_solver as G
    W, H, n = _layer(rows, cols, rows * 7 + cols + bits)
    monkeypatch.setattr(product_gptq, '_inverse_factor',
                        lambda hess, percdamp: torch.from_numpy(G.inverse_factor(hess.cpu().numpy(), percdamp)).to(hess.device).contiguous())
    Qo, so, zo, go, eo = G.fasterquant(W, H, bits, 128, 0.01, gs, act, sym)

    def shares(tag):
        Q, scale, zero, g_idx, err = _fasterquant(W, H, n, bits, sym, blocksize=128, groupsize=gs, actorder=act)
        assert np.array_equal(g_idx, go)
        first = -(-128 // (cols if gs == -1 else gs))             # groups that start in block 0 are fitted to the untouched W: the oracle's bits
        assert np.array_equal(scale[:, :first], so[:, :first]) and np.array_equal(zero[:, :first], zo[:, :first])
        moved = np.mean(np.abs(scale - so) / so > 1e-4)
        flipped = np.mean(_levels(Q, scale, zero, g_idx) != _levels(Qo, so, zo, go))
        print('%s %dx%d b%d g%d act%d sym%d: grids moved %.2e, levels flipped %.2e, loss %.6g vs %.6g' % (tag, rows, cols, bits, gs, act, sym, moved,
                                                                                                       flipped, err, eo))
        return moved, flipped, err
    moved, flipped, err = shares('layer ')
    quantizer = quant.Quantizer()
    quantizer.configure(bits, perchannel=True, sym=sym, mse=False)
    monkeypatch.setattr(product_gptq, '_solve_layer', lambda W_, Hinv, g, maxq, sym_, fit, sa, za, Q, lr: product_gptq._solve_blocks(
        W_, Hinv, quantizer, 128, g if fit else -1, g, maxq, sa, za, Q, lr))
    shares('parent')
    assert moved < 0.02 and flipped < 0.02
    assert abs(err - eo) / eo < 2e-3


def test_rows_are_independent_and_calls_repeat():
    W, H, _ = _layer(72, 384, 5)
    H = torch.from_numpy(H)
    H.diagonal().add_(0.01 * H.diagonal().mean())
    Hinv = torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(H)), upper=True).contiguous()
    W = torch.from_numpy(W)
    full = solve(W, Hinv, 128, 15, False, True)
    part = solve(W[40:], Hinv, 128, 15, False, True)
    again = solve(W, Hinv, 128, 15, False, True)
    assert bool((full[1] > 0).all())
    for f, p, a in zip(full[:4], part[:4], again[:4]):
        assert torch.equal(f[40:], p) and torch.equal(f, a)


def _raise(*a, **k):
    raise AssertionError('this route must not be taken')


def test_dispatch_takes_the_layer_kernel(monkeypatch):
    monkeypatch.setattr(quant.Quantizer, 'find_params', _raise)
    monkeypatch.setattr(product_gptq, '_solve_blocks', _raise)
    W, H, n = _layer(64, 384, 1)
    Q, scale, zero, g_idx, err = _fasterquant(W, H, n, 4, blocksize=128, groupsize=128)
    assert scale.shape == (64, 3) and bool((scale > 0).all()) and err > 0 and np.isfinite(Q).all()


@pytest.mark.parametrize('cols,mse,blocksize,perchannel', [(384, False, 64, True), (200, False, 128, True), (384, True, 128, True), (384, False, 128, False)])
def test_dispatch_keeps_the_block_route(monkeypatch, cols, mse, blocksize, perchannel):
    monkeypatch.setattr(product_gptq, '_solve_layer', _raise)
    W, H, n = _layer(64, cols, 2)
    Q, scale, zero, g_idx, err = _fasterquant(W, H, n, 4, mse=mse, perchannel=perchannel, blocksize=blocksize, groupsize=-1 if cols == 200 else 128)
    assert err > 0 and np.isfinite(Q).all()
    assert perchannel or bool((scale == scale[:1]).all() and (zero == zero[:1]).all())   # per-tensor: all rows share one grid per group
