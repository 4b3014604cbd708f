"""GPTQ.add_batch on fp16 activations: the native Hessian launch (gptq_hessian_update_f16, csrc/hessian.hip) against the parent commit's route
on the SAME tensor (x.float(), scale, transpose, fp32 addmm_ -- restated here, since the class no longer takes it for fp16 input).

  T = 2048 tokens per calibration batch (the reference's seqlen), K = 4096 and K = 11008 (the two widths of the 7B shape's linears).
  "one call": us per add_batch, the median of windows of INNER calls; "128 calls": ms for 128 consecutive calls (one linear's calibration set).
  The running mean keeps H bounded, so the calls of a window are what a quantisation run issues.

Device events around a synchronised window, both routes warmed up, REPEATS repeats with the routes alternating in one process, medians and
max - min spreads (raw repeats printed too).  Also printed: max|H_native - H_parent| / max|H| after the windows (same batches, same count).
    python tools/bench_hessian.py [--markdown FILE]"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'gptq-for-llama_amd')]
os.environ.setdefault('OMP_NUM_THREADS', '16')
REPEATS, INNER, CALLS = 7, 16, 128
TOKENS, WIDTHS = 2048, (4096, 11008)


def _timed(fn, inner):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0                       # us per window


def measure(K):
    import torch
    import torch.nn as nn
    import gptq
    dev = torch.device('cuda:0')
    layer = nn.Linear(K, 8, bias=False).half().to(dev)        # add_batch only looks at the layer's type and width
    gen = torch.Generator(device=dev).manual_seed(K)
    x = (torch.randn((1, TOKENS, K), device=dev, generator=gen) * 0.5).half()
    native, parent = gptq.GPTQ(layer), gptq.GPTQ(layer)

    def parent_route():                                       # gptq.py:94-113 of the parent commit, on the fp16 tensor
        g, batch = parent, x.shape[0]
        inp = x.reshape((-1, x.shape[-1])).t()
        g.H *= g.nsamples / (g.nsamples + batch)
        g.nsamples += batch
        xs = math.sqrt(2 / g.nsamples) * inp.float()
        g.H.addmm_(xs, xs.t())
    routes = {'native': lambda: native.add_batch(x, None), 'parent': parent_route}
    for f in routes.values():
        for _ in range(8):
            f()
    one, many = {n: [] for n in routes}, {n: [] for n in routes}
    for _ in range(REPEATS):                                  # alternating
        for name, f in routes.items():
            one[name].append(_timed(f, INNER) / INNER)
        for name, f in routes.items():
            many[name].append(_timed(f, CALLS) / 1000.0)
    torch.cuda.synchronize()
    assert native.nsamples == parent.nsamples
    diff = float((native.H - parent.H).abs().max() / parent.H.abs().max())
    return dict(K=K, tokens=TOKENS, us_per_call=one, ms_per_128_calls=many, rel_diff=diff, symmetric=bool(torch.equal(native.H, native.H.t())))


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    results = []
    for K in WIDTHS:
        print('K %d ...' % K, flush=True)
        results.append(measure(K))
        print('RESULT ' + json.dumps(results[-1]), flush=True)
    cell = lambda v: '%.1f (%.1f)' % (_median(v), max(v) - min(v))
    lines = ['### GPTQ.add_batch on a [1, %d, K] fp16 batch: native launch against the parent commit\'s route (upcast, scale, fp32 addmm_); median '
             '(max - min) of %d alternating repeats, device events; TFLOP/s = K (K + 1) T over the native call' % (TOKENS, REPEATS), '',
             '| K | native us / call | parent us / call | ratio | native ms / 128 calls | parent ms / 128 calls | ratio | native TFLOP/s | '
             'faster beyond the spread | max abs diff / max abs H | H bit-symmetric |', '|---|---|---|---|---|---|---|---|---|---|---|']
    for r in results:
        u, m = r['us_per_call'], r['ms_per_128_calls']
        faster = all(max(a['native']) < min(a['parent']) for a in (u, m))
        lines.append('| %d | %s | %s | %.2f | %s | %s | %.2f | %.0f | %s | %.2e | %s |' % (
            r['K'], cell(u['native']), cell(u['parent']), _median(u['parent']) / _median(u['native']), cell(m['native']), cell(m['parent']),
            _median(m['parent']) / _median(m['native']), r['K'] * (r['K'] + 1) * r['tokens'] / _median(u['native']) / 1e6,
            'yes' if faster else '**NO**', r['rel_diff'], 'yes' if r['symmetric'] else '**NO**'))
    lines += ['', '### Raw repeats', '', '```'] + [json.dumps(r) for r in results] + ['```', '']
    text = '\n'.join(lines)
    print(text)
    if '--markdown' in sys.argv:
        with open(sys.argv[sys.argv.index('--markdown') + 1], 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
