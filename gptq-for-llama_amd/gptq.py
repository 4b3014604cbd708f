"""GPTQ solver for MI355X -- same surface as the reference's ``gptq.py`` (``GPTQ(layer)``, ``add_batch``,
``fasterquant`` -> ``(scale, zero, g_idx, error)``, ``free``, ``Observer``), so ``llama.py:95-166`` can drive it
unchanged.  It is the caller that produces the integer weights ``QuantLinear.pack`` packs.

What runs where:
  * Hessian accumulation (reference gptq.py:71-96): fp16 activations of an ``nn.Linear`` whose width is a multiple of 8 -- what
    ``llama.py``'s hooks deliver -- take ONE hand-written HIP launch per calibration batch (``gptq_hessian_update_f16``,
    csrc/hessian.hip): H <- n/(n+b) H + 2/(n+b) X^T X in place, exact fp16 products on the matrix core, only the tiles on and above
    the diagonal computed and mirrored (H is bit-symmetric), no upcast or transposed copy of X.  Every other input (fp32 or bf16
    activations, Conv2d / Conv1D layers, odd widths) keeps the reference's route: one fp32 GEMM per batch (torch).
  * damping (torch, one line) + Hinv = chol(chol_inv(chol(H)), upper) (gptq.py:157-163): for a width that is a multiple of 128 (every
    LLaMA / OPT / NeoX linear) one hand-written HIP sweep (``gptq_hinv_factor_f32``, csrc/hinv_factor.hip) instead of the three library
    factorisations: the damped Hessian is factored from the last column backwards, A = R R^T, and Hinv = R^-1 -- the same matrix, from
    2/3 n^3 flops on the fp32 matrix instruction, with no dense inverse in between.  A pivot that is not positive raises
    ``torch.linalg.LinAlgError`` like the library.  Other widths keep torch.linalg (rocSOLVER).
  * the solve step (gptq.py:171-208), ``blocksize`` 128, a width that is a multiple of 128, a min/max quantiser (``mse=False``; per-channel when there are groups) -- every
    LLaMA / OPT / NeoX linear as ``llama.py`` quantises it: ONE hand-written HIP launch for the layer (``_solve_layer`` ->
    ``gptq_solver_layer_f32``, csrc/gptq_solver.hip).  A workgroup owns 16 weight rows and walks the blocks: per block it fits the grids
    of the groups that start there to W as it stands then (where the reference fits them, gptq.py:181-183; ``sym`` as upstream), runs the
    column loop below, keeps Err1 in LDS and applies W[:, i2:] -= Err1 . Hinv[i1:i2, i2:] (gptq.py:204) on the fp32 matrix instruction.
  * every other call (other block sizes, other widths, ``mse=True`` whose search stays in torch, and groups with ``perchannel=False``,
    where all weight rows share one grid per group while the kernel fits one per row) keeps ``_solve_blocks``: per block the
    grids with ``quant.Quantizer.find_params`` on the global W (torch), the sequential quantise / error-feedback loop over the columns
    (gptq.py:177-199; ~10 dependent torch launches per column in the reference) as ONE hand-written HIP launch
    (``gptq_solver_block_f32``: a wave per weight row, the block's columns in registers, the reference's fp32 operations one by one --
    the same device function the layer kernel calls), and the trailing update as one GEMM (torch / hipBLASLt).
There is no CPU path: the layer must live on a ROCm device (the CPU restatement used for parity and as the
reported-only baseline is oracle/gptq_solver.py, which this module never imports).
"""
import math
import time

import torch
import torch.nn as nn

import quant
from quant import _native

try:  # transformers is only needed to recognise Conv1D layers (OPT / GPT-2 style checkpoints)
    import transformers
    _Conv1D = transformers.Conv1D
except Exception:  # pragma: no cover
    _Conv1D = ()

KERNEL_MAX_BLOCK = 128   # columns the block kernel keeps in registers (two per lane)
LAYER_BLOCK = 128        # block edge of the one-launch layer solver: it serves blocksize 128 on widths that are multiples of it
FACTOR_BLOCK = 128       # block edge of the inverse-factor sweep: it serves widths that are multiples of it


class Observer:
    """keeps the ``topk`` layers with the largest quantisation error (reference gptq.py:15-53)."""

    def __init__(self, topk=32):
        self.loss_list = []
        self.topk = topk

    def submit(self, name, layerid, gptq, error):
        item = (name, layerid, {'gptq': gptq, 'error': error})
        if len(self.loss_list) < self.topk:
            self.loss_list.append(item)
            return
        worst = min(range(len(self.loss_list)), key=lambda i: self.loss_list[i][2]['error'])
        if self.loss_list[worst][2]['error'] < error:
            self.loss_list[worst] = item

    def print(self):
        self.loss_list.sort(key=lambda it: it[2]['error'], reverse=True)
        for name, layerid, info in self.loss_list:
            print('%-32s %.6f' % ('%s.%d' % (name, layerid), info['error']))
        print()

    def items(self):
        return self.loss_list


def _weight_matrix(layer):
    """[out_features, in_features] view of the layer's weight, as the reference flattens it (gptq.py:60-65)."""
    W = layer.weight.data.clone()
    if isinstance(layer, nn.Conv2d):
        W = W.flatten(1)
    if _Conv1D and isinstance(layer, _Conv1D):
        W = W.t()
    return W


def _inverse_factor(hess, percdamp):
    """upper Cholesky factor U of (H + percdamp * mean(diag H) * I)^-1 (reference gptq.py:157-163); ``hess`` is damped in place, as upstream.
    A ROCm fp32 Hessian whose width is a multiple of 128 takes the HIP sweep (``gptq_hinv_factor_f32``: A = R R^T from the last column
    backwards, U = R^-1); every other input the reference's three library factorisations."""
    hess.diagonal().add_(percdamp * hess.diagonal().mean())
    n = hess.shape[0]
    if not (hess.is_cuda and hess.dtype == torch.float32 and hess.dim() == 2 and n >= FACTOR_BLOCK and n % FACTOR_BLOCK == 0):
        lower = torch.linalg.cholesky(hess)
        return torch.linalg.cholesky(torch.cholesky_inverse(lower), upper=True).contiguous()
    # the sweep destroys its input (it is the storage of R): it works on a copy, so a caller that keeps the damped Hessian (observe=True
    # leaves it in GPTQ.H) still holds it afterwards, as with the library route.  One n^2 copy against 2/3 n^3 flops.
    work = hess.clone(memory_format=torch.contiguous_format)
    factor = torch.zeros((n, n), device=hess.device, dtype=torch.float32)
    info = torch.zeros(1, device=hess.device, dtype=torch.int32)
    with _native.on_device(hess.device):
        rc = _native.lib().gptq_hinv_factor_f32(work.data_ptr(), n, n, factor.data_ptr(), n, info.data_ptr(), _native.stream_ptr(hess.device))
    _native.check(rc, 'gptq_hinv_factor_f32')
    bad = int(info.item())                                  # read once, behind the whole sweep
    if bad:
        raise torch.linalg.LinAlgError('gptq_hinv_factor_f32: the damped Hessian is not positive definite (the pivot of column %d is not '
                                       'positive)' % (bad - 1))
    return factor


def _solve_blocks(W, Hinv, quantizer, blocksize, groupsize, gs, maxq, scale_all, zero_all, Q, loss_rows):
    """the solve step block by block from the host (reference gptq.py:171-208): per block the grids of the groups that start in it
    (``quantizer.find_params``, torch), ONE launch of the column loop (``gptq_solver_block_f32``) and one library GEMM for the trailing
    update.  Serves every block size, every width and ``mse=True``.  ``W`` is updated in place."""
    lib = _native.lib()
    rows, cols = W.shape
    n_groups = scale_all.shape[1]
    Err = torch.empty((rows, KERNEL_MAX_BLOCK), device=W.device)
    stream = _native.stream_ptr(W.device)
    for i1 in range(0, cols, blocksize):
        i2 = min(i1 + blocksize, cols)
        if groupsize != -1:
            # grids of the groups that START inside this block, fitted to W as it is now (gptq.py:181-183)
            first = -(-i1 // gs) * gs
            for c in range(first, i2, gs):
                quantizer.find_params(W[:, c:c + gs], weight=True)
                scale_all[:, c // gs] = quantizer.scale.reshape(-1)
                zero_all[:, c // gs] = quantizer.zero.reshape(-1)
        for j1 in range(i1, i2, KERNEL_MAX_BLOCK):   # the kernel keeps <= 128 columns in registers
            j2 = min(j1 + KERNEL_MAX_BLOCK, i2)
            rc = lib.gptq_solver_block_f32(W.data_ptr(), cols, Hinv.data_ptr(), cols, rows, cols, j1, j2 - j1, gs, maxq,
                                           scale_all.data_ptr(), zero_all.data_ptr(), n_groups, Q.data_ptr(), cols,
                                           Err.data_ptr(), KERNEL_MAX_BLOCK, loss_rows.data_ptr(), stream)
            _native.check(rc, 'gptq_solver_block_f32')
            if j2 < cols:
                W[:, j2:] -= Err[:, :j2 - j1].matmul(Hinv[j1:j2, j2:])


def _solve_layer(W, Hinv, gs, maxq, sym, fit, scale_all, zero_all, Q, loss_rows):
    """the same solve step in ONE launch (``gptq_solver_layer_f32``): 128-column blocks, the min/max grid fitted in the kernel when ``fit``
    (``scale_all`` / ``zero_all`` are then outputs), Err1 in LDS, the trailing update on the fp32 matrix instruction.  ``W`` is destroyed."""
    rows, cols = W.shape
    rc = _native.lib().gptq_solver_layer_f32(W.data_ptr(), cols, Hinv.data_ptr(), cols, rows, cols, gs, maxq, int(sym), int(fit),
                                             scale_all.data_ptr(), zero_all.data_ptr(), scale_all.shape[1], Q.data_ptr(), cols,
                                             loss_rows.data_ptr(), _native.stream_ptr(W.device))
    _native.check(rc, 'gptq_solver_layer_f32')


class GPTQ:

    def __init__(self, layer, observe=False):
        self.layer = layer
        self.dev = self.layer.weight.device
        W = _weight_matrix(layer)
        self.rows, self.columns = W.shape[0], W.shape[1]
        self.H = torch.zeros((self.columns, self.columns), device=self.dev)
        self.nsamples = 0
        self.quantizer = quant.Quantizer()
        self.observe = observe
        self.inp1 = self.out1 = None

    # -----------------------------------------------------------------------------------------
    def add_batch(self, inp, out):
        """H <- running mean of 2 X X^T over the calibration samples (reference gptq.py:71-96)."""
        if self.observe:
            self.inp1, self.out1 = inp, out
        else:
            self.inp1 = self.out1 = None
        if inp.dim() == 2:
            inp = inp.unsqueeze(0)
        batch = inp.shape[0]
        if isinstance(self.layer, nn.Conv2d):
            unfold = nn.Unfold(self.layer.kernel_size, dilation=self.layer.dilation, padding=self.layer.padding, stride=self.layer.stride)
            inp = unfold(inp).permute([1, 0, 2]).flatten(1)
        else:
            if inp.dim() == 3:
                inp = inp.reshape((-1, inp.shape[-1]))
            if (isinstance(self.layer, nn.Linear) and inp.dtype == torch.float16 and inp.is_cuda and inp.dim() == 2
                    and inp.shape[0] > 0 and inp.shape[1] % 8 == 0):
                self._add_batch_native(inp, batch)
                return
            inp = inp.t()
        self.H *= self.nsamples / (self.nsamples + batch)
        self.nsamples += batch
        x = math.sqrt(2 / self.nsamples) * inp.float()
        self.H.addmm_(x, x.t())

    def _add_batch_native(self, x, batch):
        """the same running mean in one launch: H <- n/(n+b) H + 2/(n+b) X^T X on the fp16 rows x [tokens, columns]"""
        x = x.contiguous()
        n = self.nsamples
        with _native.on_device(self.dev):
            rc = _native.lib().gptq_hessian_update_f16(x.data_ptr(), x.shape[1], x.shape[0], x.shape[1], self.H.data_ptr(), self.columns,
                                                       n / (n + batch), 2 / (n + batch), _native.stream_ptr(self.dev))
        _native.check(rc, 'gptq_hessian_update_f16')
        self.nsamples = n + batch

    # -----------------------------------------------------------------------------------------
    def _report(self, name, q_weight, weight_error, seconds):
        """assign the quantised weight and print one progress line (reference print_loss, gptq.py:98-126)."""
        self.layer.weight.data = q_weight.reshape(self.layer.weight.shape).to(self.layer.weight.data.dtype)
        fp_snr = q_snr = '-'
        if self.inp1 is not None:
            q8 = quant.Quantizer()
            q8.configure(8, perchannel=False, sym=True, mse=False)
            q8.find_params(self.inp1)
            q_out = self.layer(q8.quantize(self.inp1).type(torch.float16))

            def snr(pred, real):
                pred, real = pred.float().flatten(1), real.float().flatten(1)
                return float((((pred - real) ** 2).sum(-1) / (real ** 2).sum(-1)).mean())
            q_snr = '%.4g' % snr(q_out, self.out1)
            fp_snr = '%.4g' % snr(self.layer(self.inp1), self.out1)
        print('| %-16s | %12.4f | %10s | %10s | %8.3f |' % (name, weight_error, fp_snr, q_snr, seconds))

    def fasterquant(self, blocksize=128, percdamp=.01, groupsize=-1, actorder=False, name=''):
        if self.dev.type != 'cuda':
            raise RuntimeError('GPTQ.fasterquant: layer is on %s -- the MI355X solver has no CPU path' % self.dev)
        _native.lib()
        self.layer.to(self.dev)
        W = _weight_matrix(self.layer).float().contiguous()
        tick = time.time()
        if int(self.quantizer.maxq) < 0:
            raise NotImplementedError('ternary grids (trits) are not supported by the HIP block solver')
        maxq = int(self.quantizer.maxq)
        # one launch for the layer where the kernel serves it: its blocks are 128 columns and its grid fit is the min/max rule, one grid
        # per weight row and group (perchannel=True; a per-tensor quantiser shares one grid per group among all rows and keeps the block route)
        layer_route = (maxq > 0 and blocksize == LAYER_BLOCK and self.columns % LAYER_BLOCK == 0 and not self.quantizer.mse
                       and (groupsize == -1 or self.quantizer.perchannel))

        # whole-row grid; the only one without groups (gptq.py:139-140).  With groups every grid is fitted again per group, in the kernel
        # on the layer route: nothing reads this one
        if not self.quantizer.ready() and not (layer_route and groupsize != -1):
            self.quantizer.find_params(W, weight=True)

        hess = self.H
        if not self.observe:
            del self.H
        never_seen = hess.diagonal() == 0                   # input features no calibration token activated (gptq.py:145-147)
        hess.diagonal()[never_seen] = 1
        W[:, never_seen] = 0

        order = None
        if actorder:                                        # most sensitive input features first (gptq.py:149-152)
            order = torch.argsort(hess.diagonal(), descending=True)
            W = W[:, order].contiguous()
            hess = hess[order][:, order]
        rows, cols = self.rows, self.columns
        Hinv = _inverse_factor(hess, percdamp)
        del hess

        gs = cols if groupsize == -1 else groupsize
        n_groups = (cols + gs - 1) // gs
        scale_all = torch.zeros((rows, n_groups), device=self.dev)
        zero_all = torch.zeros((rows, n_groups), device=self.dev)
        if groupsize == -1:
            scale_all[:, 0] = self.quantizer.scale.reshape(-1)
            zero_all[:, 0] = self.quantizer.zero.reshape(-1)
        Q = torch.zeros_like(W)
        loss_rows = torch.zeros(rows, device=self.dev)
        with torch.cuda.device(self.dev):
            if layer_route:
                _solve_layer(W, Hinv, gs, maxq, bool(self.quantizer.sym), groupsize != -1, scale_all, zero_all, Q, loss_rows)
                if groupsize != -1:                         # the quantiser is left as the last per-group fit leaves it
                    self.quantizer.maxq = self.quantizer.maxq.to(self.dev)
                    self.quantizer.scale, self.quantizer.zero = scale_all[:, -1:].clone(), zero_all[:, -1:].clone()
            else:
                _solve_blocks(W, Hinv, self.quantizer, blocksize, groupsize, gs, maxq, scale_all, zero_all, Q, loss_rows)
            torch.cuda.synchronize()
        error = float(loss_rows.double().sum().item())

        g_idx = (torch.arange(cols, device=self.dev) // gs).to(torch.int32)
        if order is not None:                               # back to the checkpoint's column order (gptq.py:212-215)
            restore = torch.argsort(order)
            Q, g_idx = Q[:, restore], g_idx[restore]
        if _Conv1D and isinstance(self.layer, _Conv1D):
            Q = Q.t()
        self._report(name, Q, error, time.time() - tick)
        return scale_all, zero_all, g_idx, error

    def free(self):
        self.inp1 = self.out1 = None
        self.H = None
        self.Losses = None
        self.Trace = None
        torch.cuda.empty_cache()
