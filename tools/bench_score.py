"""Scoring token sequences: what the fused LM head + cross-entropy (gptq_lm_head_nll_f16, csrc/gemm8.hip) and DecodeEngine.score cost.

  table 1, the op: one gptq_lm_head_nll_f16 call (nll only) against the materialising route -- torch.matmul to fp16 logits, then
           F.cross_entropy(logits.float(), targets, reduction='none') -- at M in {128, 512, 2047}, N = 32000, K = 4096: time, peak memory above
           the inputs (torch.cuda.max_memory_allocated over one call), achieved FLOP/s of the fused call from 2 M N K and its share of the
           2.5 PFLOP/s dense fp16 peak, and the largest difference of the two results.
  table 2, the engine, 7B-shaped random model (build_random_llama), T in {128, 512, 2047}: DecodeEngine.score(ids) against the module chain
           (model(ids).logits with the engine hook disabled + the same cross-entropy) and against prefill(ids) alone (what scoring all rows
           costs on top of the prompt pass).

Device events around a synchronised window, every shape warmed up, REPEATS repeats with the candidates alternating in one process, medians and
max - min spreads (raw repeats printed too).  Every table is a child process under its own `timeout`; at most 16 CPU threads.
    python tools/bench_score.py [--markdown FILE] [--only op|engine]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'gptq-for-llama_amd')]
os.environ.setdefault('OMP_NUM_THREADS', '16')
REPEATS = 7
ROWS = (128, 512, 2047)
N, K = 32000, 4096
PEAK_FLOPS = 2.5e15
STEP_TIMEOUT = {'op': 300, 'engine': 900}


def _timed(fn, inner):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / inner          # us per call


def _peak(fn, dev):
    """peak bytes one call allocates above what is resident before it (the call's result included)"""
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    del out
    return peak


def step_op(M):
    import torch
    import torch.nn.functional as F
    from quant import _native
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lib, dev = _native.lib(), torch.device('cuda:0')
    s = _native.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(M)
    x = torch.randn((M, K), device=dev, generator=g).half()
    W = (0.02 * torch.randn((N, K), device=dev, generator=g)).half()
    t = torch.randint(0, N, (M,), device=dev, generator=g)
    need = lib.gptq_lm_head_nll_workspace_bytes(M, N)

    def fused():                                         # allocates its workspace and its output, like a first call would
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        nll = torch.empty(M, dtype=torch.float32, device=dev)
        rc = lib.gptq_lm_head_nll_f16(x.data_ptr(), K, W.data_ptr(), K, None, t.data_ptr(), nll.data_ptr(), None, None, M, N, K, ws.data_ptr(), need, s)
        assert rc == 0, rc
        return nll

    def materialised():
        return F.cross_entropy(torch.matmul(x, W.t()).float(), t, reduction='none')

    for f in (fused, materialised):
        for _ in range(3):
            f()
    diff = float((fused().double() - materialised().double()).abs().max())
    res = dict(step='op', M=M, workspace_bytes=need, fused_peak_bytes=_peak(fused, dev), materialised_peak_bytes=_peak(materialised, dev), max_abs_diff=diff)
    inner = max(5, min(50, int(20000 / M)))
    a, b = [], []
    for _ in range(REPEATS):                             # alternating
        a.append(_timed(fused, inner))
        b.append(_timed(materialised, inner))
    res.update(inner=inner, fused_us=a, materialised_us=b)
    return res


def engine_setup():
    import torch
    from quant import decode as D
    torch.set_num_threads(min(16, torch.get_num_threads()))
    model = D.build_random_llama('cuda:0', seed=0)
    return model, D.DecodeEngine(model, t_max=2048)


def step_engine(T, model, eng):
    import torch
    import torch.nn.functional as F
    dev = torch.device('cuda:0')
    ids = torch.randint(0, model.config.vocab_size, (T,), device=dev, generator=torch.Generator(device=dev).manual_seed(T))

    def score():
        return eng.score(ids)

    def prefill():
        return eng.prefill(ids, start=0)

    def chain():
        model._gptq_engine_disabled = True
        try:
            with torch.no_grad():
                logits = model(ids[None]).logits[0]
        finally:
            model._gptq_engine_disabled = False
        return F.cross_entropy(logits[:-1].float(), ids[1:], reduction='none')

    for f in (score, prefill, chain):
        for _ in range(2):
            f()
    res = dict(step='engine', T=T, max_abs_diff=float((score().double() - chain().double()).abs().max()),
               score_peak_bytes=_peak(score, dev), chain_peak_bytes=_peak(chain, dev), prefill_peak_bytes=_peak(prefill, dev))
    a, b, c = [], [], []
    for _ in range(REPEATS):
        a.append(_timed(score, 1) / 1000.0)
        b.append(_timed(chain, 1) / 1000.0)
        c.append(_timed(prefill, 1) / 1000.0)
    res.update(score_ms=a, chain_ms=b, prefill_ms=c)
    return res


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _spread(v):
    return max(v) - min(v)


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == '--step':
        setup = engine_setup() if sys.argv[2] == 'engine' else ()
        for m in ROWS:
            print('%s %d ...' % (sys.argv[2], m), flush=True)
            r = (step_op if sys.argv[2] == 'op' else step_engine)(m, *setup)
            print('RESULT ' + json.dumps(r), flush=True)
        return 0
    kinds = [sys.argv[sys.argv.index('--only') + 1]] if '--only' in sys.argv else ['op', 'engine']
    results = []
    for kind in kinds:
        cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT[kind]), sys.executable, os.path.abspath(__file__), '--step', kind]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
        for line in p.stdout:                            # streamed: a long step still shows progress
            print(line.rstrip(), flush=True)
            if line.startswith('RESULT '):
                results.append(json.loads(line[7:]))
        if p.wait() != 0:                                # a fault, an abort or a time limit: nothing more is started on the GPU
            print('step %s ended with status %d: stopping' % (kind, p.returncode))
            return 1
    MiB = 2.0 ** 20
    lines = ['### The op: N = %d, K = %d (median of %d alternating repeats, device events; spread = max - min)' % (N, K, REPEATS), '',
             '| M | fused us | spread | materialised us | spread | materialised / fused | fused TFLOP/s | of 2.5 PFLOP/s | fused peak MiB (workspace) | materialised peak MiB | max abs difference of nll |',
             '|---|---|---|---|---|---|---|---|---|---|---|']
    for r in results:
        if r['step'] == 'op':
            a, b = _median(r['fused_us']), _median(r['materialised_us'])
            fl = 2.0 * r['M'] * N * K / (a * 1e-6)
            lines.append('| %d | %.1f | %.1f | %.1f | %.1f | %.2f | %.0f | %.1f %% | %.2f (%.2f) | %.1f | %.2e |' % (
                r['M'], a, _spread(r['fused_us']), b, _spread(r['materialised_us']), b / a, fl / 1e12, 100 * fl / PEAK_FLOPS,
                r['fused_peak_bytes'] / MiB, r['workspace_bytes'] / MiB, r['materialised_peak_bytes'] / MiB, r['max_abs_diff']))
    lines += ['', '### The engine: 7B-shaped random model, DecodeEngine(t_max=2048) (median of %d alternating repeats)' % REPEATS, '',
              '| T | score ms | spread | module chain + cross-entropy ms | spread | chain / score | prefill alone ms | spread | score - prefill ms | score peak MiB | chain peak MiB | prefill peak MiB | max abs difference of nll |',
              '|---|---|---|---|---|---|---|---|---|---|---|---|---|']
    for r in results:
        if r['step'] == 'engine':
            a, b, c = _median(r['score_ms']), _median(r['chain_ms']), _median(r['prefill_ms'])
            lines.append('| %d | %.2f | %.2f | %.2f | %.2f | %.2f | %.2f | %.2f | %.2f | %.1f | %.1f | %.1f | %.2e |' % (
                r['T'], a, _spread(r['score_ms']), b, _spread(r['chain_ms']), b / a, c, _spread(r['prefill_ms']), a - c,
                r['score_peak_bytes'] / MiB, r['chain_peak_bytes'] / MiB, r['prefill_peak_bytes'] / MiB, r['max_abs_diff']))
    lines += ['', '### Raw repeats', '', '```'] + [json.dumps(r) for r in results] + ['```', '']
    text = '\n'.join(lines)
    print(text)
    if '--markdown' in sys.argv:
        with open(sys.argv[sys.argv.index('--markdown') + 1], 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
