"""The solve step of GPTQ.fasterquant: one launch for the layer (gptq._solve_layer -> gptq_solver_layer_f32, csrc/gptq_solver.hip) against the
parent commit's route (gptq._solve_blocks as kept in the tree: per block the torch grid fits, one block-kernel launch and one library GEMM), on
the same damped Hessian (add_batch on 2 x 2048 random fp16 tokens) and the same inverse factor, 4096 x 4096 and 4096 x 11008 -> 4-bit g128.

  solve:       the solve step alone, each route on a fresh copy of W (the copy and the output buffers are outside the events)
  fasterquant: the whole call with the dispatch as shipped and with the layer route switched off (gptq.LAYER_BLOCK = -1: the parent's code path)
Device events, both routes warmed up, REPEATS alternating repeats in one process, medians and max - min spreads, raw repeats printed.
    python tools/bench_solver.py [--markdown FILE]          # the tables
    python tools/bench_solver.py --once N new|parent        # two whole calls at width N on one route, for a kernel trace"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'gptq-for-llama_amd')]
os.environ.setdefault('OMP_NUM_THREADS', '16')
REPEATS, TOKENS, WIDTHS, ROWS, BITS, GS = 11, 2048, (4096, 11008), 4096, 4, 128


def setup(n):
    import torch
    import torch.nn as nn
    import gptq
    layer = nn.Linear(n, ROWS, bias=False).half().to('cuda:0')
    g = gptq.GPTQ(layer)
    gen = torch.Generator(device='cuda:0').manual_seed(n)
    for _ in range(2):
        g.add_batch((torch.randn((1, TOKENS, n), device='cuda:0', generator=gen) * 0.5).half(), None)
    return layer, g.H


def quantise(layer, weight, H, shipped, block=None):
    """one whole fasterquant on a restored layer: (ms, loss); shipped False takes the parent's code path"""
    import torch
    import gptq
    layer.weight.data = weight.clone()
    g = gptq.GPTQ(layer)
    g.quantizer.configure(BITS, perchannel=True, sym=False, mse=False)
    g.H, g.nsamples = H.clone(), 2
    gptq.LAYER_BLOCK = block if shipped else -1
    try:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        err = g.fasterquant(blocksize=128, percdamp=0.01, groupsize=GS, name='%s %d' % ('new' if shipped else 'parent', layer.in_features))[3]
        e1.record()
        torch.cuda.synchronize()
    finally:
        gptq.LAYER_BLOCK = block                                  # the product constant is restored whatever the call did
    return e0.elapsed_time(e1), err


def measure(n):
    import torch
    import gptq
    import quant
    layer, H = setup(n)
    weight, block = layer.weight.data.clone(), gptq.LAYER_BLOCK
    Hinv = gptq._inverse_factor(H.clone(), 0.01)
    quantizer = quant.Quantizer()
    quantizer.configure(BITS, perchannel=True, sym=False, mse=False)
    maxq, ng = int(quantizer.maxq), n // GS
    solve, total, loss, solve_loss = ({'new': [], 'parent': []} for _ in range(4))
    for rep in range(-2, REPEATS):                                # two warm-up rounds
        for name in ('new', 'parent'):
            W = weight.float().contiguous()
            sa, za = torch.zeros((ROWS, ng), device='cuda:0'), torch.zeros((ROWS, ng), device='cuda:0')
            Q, lr = torch.zeros_like(W), torch.zeros(ROWS, device='cuda:0')
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            if name == 'new':
                gptq._solve_layer(W, Hinv, GS, maxq, False, True, sa, za, Q, lr)
            else:
                gptq._solve_blocks(W, Hinv, quantizer, 128, GS, GS, maxq, sa, za, Q, lr)
            e1.record()
            torch.cuda.synchronize()
            if rep >= 0:
                solve[name].append(e0.elapsed_time(e1))
                solve_loss[name] = float(lr.double().sum().item())
        for name in ('new', 'parent'):
            t, err = quantise(layer, weight, H, name == 'new', block)
            if rep >= 0:
                total[name].append(t)
                loss[name] = err
    return dict(n=n, rows=ROWS, solve_ms=solve, fasterquant_ms=total, solve_loss=solve_loss, loss=loss)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    if '--once' in sys.argv:
        import gptq
        n, route = int(sys.argv[sys.argv.index('--once') + 1]), sys.argv[sys.argv.index('--once') + 2]
        layer, H = setup(n)
        weight = layer.weight.data.clone()
        for _ in range(2):
            quantise(layer, weight, H, route == 'new', gptq.LAYER_BLOCK)
        return 0
    results = []
    for n in WIDTHS:
        print('n %d ...' % n, flush=True)
        results.append(measure(n))
        print('RESULT ' + json.dumps(results[-1]), flush=True)
    cell = lambda v: '%.2f (%.2f)' % (_median(v), max(v) - min(v))
    lines = ['### %d x n -> %d-bit g%d, damped Hessian of 2 x %d fp16 tokens: the layer launch against the parent route (`_solve_blocks`); ms, median '
             '(max - min) of %d alternating repeats, device events' % (ROWS, BITS, GS, TOKENS, REPEATS), '',
             '| n | solve new | solve parent | ratio | every new repeat below every parent repeat | fasterquant new | fasterquant parent | ratio | '
             'loss new | loss parent |', '|---|---|---|---|---|---|---|---|---|---|']
    for r in results:
        s, t = r['solve_ms'], r['fasterquant_ms']
        lines.append('| %d | %s | %s | %.2f | %s | %s | %s | %.2f | %.6g | %.6g |' % (
            r['n'], cell(s['new']), cell(s['parent']), _median(s['parent']) / _median(s['new']), 'yes' if max(s['new']) < min(s['parent']) else '**NO**',
            cell(t['new']), cell(t['parent']), _median(t['parent']) / _median(t['new']), r['loss']['new'], r['loss']['parent']))
    lines += ['', '### Raw repeats', '', '```'] + [json.dumps(r) for r in results] + ['```', '']
    text = '\n'.join(lines)
    print(text)
    if '--markdown' in sys.argv:
        with open(sys.argv[sys.argv.index('--markdown') + 1], 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
