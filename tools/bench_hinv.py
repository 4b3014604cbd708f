"""The inverse Hessian factor of GPTQ.fasterquant: the HIP sweep (gptq_hinv_factor_f32, csrc/hinv_factor.hip) against the parent commit's three
library factorisations (restated here), on the same damped Hessian (add_batch on 2 x 2048 random fp16 tokens), at n = 4096 and n = 11008.

  factor:      gptq._inverse_factor alone, each route on a fresh copy of the damped Hessian (the copy is outside the events)
  fasterquant: the whole call on a rows x n layer -> 4-bit g128 (4096 x 4096 and 4096 x 11008), with gptq._inverse_factor as shipped and
               replaced by the parent's; the time inside _inverse_factor is taken by events in the same runs, "rest" is the difference
               (grid fits, block kernel, trailing GEMMs, Python)
Device events, both routes warmed up, REPEATS alternating repeats in one process, medians and max - min spreads, raw repeats printed.
    python tools/bench_hinv.py [--markdown FILE]        # the tables
    python tools/bench_hinv.py --once N                 # one warm sweep at width N, for a kernel trace"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'gptq-for-llama_amd')]
os.environ.setdefault('OMP_NUM_THREADS', '16')
REPEATS, TOKENS, WIDTHS, ROWS = 21, 2048, (4096, 11008), 4096


def parent_route(hess, percdamp):
    import torch
    hess.diagonal().add_(percdamp * hess.diagonal().mean())
    lower = torch.linalg.cholesky(hess)
    return torch.linalg.cholesky(torch.cholesky_inverse(lower), upper=True).contiguous()


def hessian(n, layer):
    import torch
    import gptq
    g = gptq.GPTQ(layer)
    gen = torch.Generator(device='cuda:0').manual_seed(n)
    for _ in range(2):
        g.add_batch((torch.randn((1, TOKENS, n), device='cuda:0', generator=gen) * 0.5).half(), None)
    return g.H


def _events():
    import torch
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def measure(n):
    import torch
    import torch.nn as nn
    import gptq
    layer = nn.Linear(n, ROWS, bias=False).half().to('cuda:0')
    weight = layer.weight.data.clone()
    H = hessian(n, layer)
    shipped = gptq._inverse_factor
    routes = {'new': shipped, 'parent': parent_route}
    factor, total, inside, loss, spans = ({k: [] for k in routes} for _ in range(5))

    def timed_factor(f):
        def inner(hess, percdamp):
            e0, e1 = _events()
            e0.record()
            out = f(hess, percdamp)
            e1.record()
            spans.setdefault('last', []).append((e0, e1))
            return out
        return inner

    def quantise(name):
        layer.weight.data = weight.clone()
        g = gptq.GPTQ(layer)
        g.quantizer.configure(4, perchannel=True, sym=False, mse=False)
        g.H, g.nsamples = H.clone(), 2
        gptq._inverse_factor = timed_factor(routes[name])
        e0, e1 = _events()
        torch.cuda.synchronize()
        e0.record()
        err = g.fasterquant(blocksize=128, percdamp=0.01, groupsize=128, name='%s %d' % (name, n))[3]
        e1.record()
        torch.cuda.synchronize()
        gptq._inverse_factor = shipped
        f0, f1 = spans.pop('last')[0]
        return e0.elapsed_time(e1), f0.elapsed_time(f1), err

    for rep in range(-2, REPEATS):                                # two warm-up rounds
        for name, f in routes.items():
            work = H.clone()
            e0, e1 = _events()
            torch.cuda.synchronize()
            e0.record()
            out = f(work, 0.01)
            e1.record()
            torch.cuda.synchronize()
            if rep >= 0:
                factor[name].append(e0.elapsed_time(e1))
            if rep == -2:
                spans[name] = out
        for name in routes:
            t, fi, err = quantise(name)
            if rep >= 0:
                total[name].append(t)
                inside[name].append(fi)
                loss[name] = err
    diff = float((spans['new'] - spans['parent']).abs().max() / spans['parent'].abs().max())
    return dict(n=n, rows=ROWS, factor_ms=factor, fasterquant_ms=total, inside_factor_ms=inside, loss=loss, rel_diff=diff)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    if '--once' in sys.argv:
        import torch
        import torch.nn as nn
        import gptq
        n = int(sys.argv[sys.argv.index('--once') + 1])
        H = hessian(n, nn.Linear(n, 8, bias=False).half().to('cuda:0'))
        for _ in range(2):
            gptq._inverse_factor(H.clone(), 0.01)
        torch.cuda.synchronize()
        return 0
    results = []
    for n in WIDTHS:
        print('n %d ...' % n, flush=True)
        results.append(measure(n))
        print('RESULT ' + json.dumps(results[-1]), flush=True)
    cell = lambda v: '%.2f (%.2f)' % (_median(v), max(v) - min(v))
    lines = ['### `_inverse_factor` alone on the damped Hessian of 2 x %d fp16 tokens: HIP sweep against the parent\'s three library calls; ms, median '
             '(max - min) of %d alternating repeats, device events; TFLOP/s = 2/3 n^3 over the sweep' % (TOKENS, REPEATS), '',
             '| n | new ms | parent ms | ratio | new TFLOP/s | faster beyond both spreads | max abs diff / max abs U |', '|---|---|---|---|---|---|---|']
    for r in results:
        f = r['factor_ms']
        lines.append('| %d | %s | %s | %.2f | %.1f | %s | %.2e |' % (
            r['n'], cell(f['new']), cell(f['parent']), _median(f['parent']) / _median(f['new']), 2 / 3 * r['n'] ** 3 / _median(f['new']) / 1e9,
            'yes' if max(f['new']) < min(f['parent']) else '**NO**', r['rel_diff']))
    lines += ['', '### Whole `fasterquant`, %d x n -> 4-bit g128: where the time goes, parent route and new route; ms, median (max - min)' % ROWS, '',
              '| n | route | fasterquant | inside `_inverse_factor` | share | rest (grid fits, block kernel, trailing GEMM, Python) | loss |',
              '|---|---|---|---|---|---|---|']
    for r in results:
        for name in ('parent', 'new'):
            t, fi = r['fasterquant_ms'][name], r['inside_factor_ms'][name]
            lines.append('| %d | %s | %s | %s | %.0f %% | %.2f | %.6g |' % (r['n'], name, cell(t), cell(fi), 100 * _median(fi) / _median(t),
                                                                         _median(t) - _median(fi), r['loss'][name]))
    lines += ['', '### Raw repeats', '', '```'] + [json.dumps(r) for r in results] + ['```', '']
    text = '\n'.join(lines)
    print(text)
    if '--markdown' in sys.argv:
        with open(sys.argv[sys.argv.index('--markdown') + 1], 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
