"""Sampling in the engine: what gptq_sample_rows_f16 (csrc/sample.hip) and the native sampling graph cost.

  table 1, the op: one gptq_sample_rows_f16 launch on [rows, 32000] fp16 logits (randn * 2.5, every row its own), rows in {1, 4, 16}, with the
           reference script's setting (temperature 0.8, top-k off, top-p 0.95: llama_inference.py:119-127) and with top-k 50 added; next to it
           torch.argmax(logits, -1) -- what the greedy graph runs in its place -- and the parent's sampling tail on the same logits (fp32 copy,
           HF's warpers, softmax, torch.multinomial: DecodeEngine._sample_rows_step without the decode step).
  table 2, the engine, 7B-shaped random model with the finite-logits initialisation of bench.py's sampling leg (scales x 0.05), batch 1 and 16,
           a 16-token prompt per row: seconds per replay of the three self-feeding graphs of ONE engine from the same state -- greedy
           (capture_greedy_rows), native sampling (capture_sample_native) and the parent's sampling tail (capture_sample_rows with HF's warpers)
           -- and tokens/s of engine_generate(prefill='engine') / engine_generate_batch end to end, greedy and sample=dict(temperature=0.8,
           top_p=0.95).

Device events around a synchronised window, everything warmed up, REPEATS repeats with the candidates alternating in one process, medians and
max - min spreads (raw repeats printed too).  Every table is a child process under its own `timeout`; at most 16 CPU threads.
    python tools/bench_sample.py [--markdown FILE] [--only op|engine]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'gptq-for-llama_amd')]
os.environ.setdefault('OMP_NUM_THREADS', '16')
REPEATS = 7
VOCAB = 32000
SCRIPT = dict(temperature=0.8, top_p=0.95)           # llama_inference.py:119-127
STEPS = 128
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


def _warpers(top_k=0):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    w = [TemperatureLogitsWarper(SCRIPT['temperature'])]
    if top_k:
        w.append(TopKLogitsWarper(top_k=top_k, min_tokens_to_keep=1))
    return w + [TopPLogitsWarper(top_p=SCRIPT['top_p'], min_tokens_to_keep=1)]


def step_op(rows):
    import torch
    from quant import _native
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lib, dev = _native.lib(), torch.device('cuda:0')
    s = _native.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(rows)
    logits = (torch.randn((rows, VOCAB), device=dev, generator=g) * 2.5).half()
    u = torch.rand(rows, device=dev, generator=g)
    T = torch.full((rows,), SCRIPT['temperature'], device=dev)
    p = torch.full((rows,), SCRIPT['top_p'], device=dev)
    k0, k50 = torch.zeros(rows, dtype=torch.int32, device=dev), torch.full((rows,), 50, dtype=torch.int32, device=dev)
    out = torch.empty(rows, dtype=torch.int64, device=dev)

    def native(k):
        def run():
            rc = lib.gptq_sample_rows_f16(logits.data_ptr(), VOCAB, rows, VOCAB, u.data_ptr(), T.data_ptr(), k.data_ptr(), p.data_ptr(), out.data_ptr(), s)
            assert rc == 0, rc
        return run

    def tail(warpers):
        def run():
            scores = logits.to(copy=True, dtype=torch.float32)
            for w in warpers:
                scores = w(None, scores)
            out.copy_(torch.multinomial(torch.nn.functional.softmax(scores, dim=-1), num_samples=1).squeeze(1))
        return run

    def argmax():
        torch.argmax(logits, dim=-1, out=out)
    cands = dict(native=native(k0), native_k50=native(k50), argmax=argmax, hf_tail=tail(_warpers()), hf_tail_k50=tail(_warpers(50)))
    for f in cands.values():
        for _ in range(5):
            f()
    times = {name: [] for name in cands}
    for _ in range(REPEATS):                             # alternating
        for name, f in cands.items():
            times[name].append(_timed(f, 200))
    return dict(step='op', rows=rows, inner=200, us=times)


def engine_setup():
    import torch
    from quant import decode as D
    torch.set_num_threads(min(16, torch.get_num_threads()))
    fill = D.fill_random_quant_

    def small(layer, gen):                               # bench.py's sampling leg: finite logits
        fill(layer, gen)
        layer.scales.mul_(0.05)
    D.fill_random_quant_ = small
    try:
        return (D.build_random_llama('cuda:0', seed=0),)
    finally:
        D.fill_random_quant_ = fill


def step_engine(batch, model):
    import time
    import torch
    from quant import decode as D
    dev = torch.device('cuda:0')
    eng = D.DecodeEngine(model, t_max=2048, batch=batch)
    gen = torch.Generator(device=dev).manual_seed(batch)
    prompts = [torch.randint(1, VOCAB, (16,), device=dev, generator=gen) for _ in range(batch)]
    logits = eng.prefill_batch(prompts)
    finite = bool(torch.isfinite(logits.float()).all())
    eng.set_sampling(**SCRIPT)
    eng.ids.copy_(torch.argmax(logits, dim=-1))
    pos0, ids0 = eng.pos.clone(), eng.ids.clone()
    graphs = dict(greedy=eng.capture_greedy_rows().greedy_rows_graph, native=eng.capture_sample_native(),
                  hf_tail=eng.capture_sample_rows('bench', _warpers()))

    def replays(g):
        def run():
            g.replay()
        return run

    def timed_graph(g):
        eng.pos.copy_(pos0); eng.ids.copy_(ids0); eng.stepc.zero_()     # every candidate from the same state: the same context lengths
        return _timed(replays(g), STEPS)
    torch.manual_seed(0)
    for g in graphs.values():
        timed_graph(g)
    times = {name: [] for name in graphs}
    for _ in range(REPEATS):
        for name, g in graphs.items():
            times[name].append(timed_graph(g))
    res = dict(step='engine', batch=batch, logits_finite=finite, steps=STEPS, us_per_replay=times)

    # end to end: tokens/s of the public entry points, (t(STEPS + 1 tokens) - t(1 token)) / STEPS as benchmark_generate measures model.generate
    one = D.DecodeEngine(model, t_max=2048).capture() if batch == 1 else None

    def generate(n, sample):
        torch.manual_seed(0); torch.cuda.synchronize(); t0 = time.perf_counter()
        if batch == 1:
            D.engine_generate(model, prompts[0][None], n, engine=one, prefill='engine', sample=sample)
        else:
            D.engine_generate_batch(model, prompts, n, engine=eng, sample=sample)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    rates = dict(greedy=[], sampled=[])
    for sample in (None, SCRIPT):
        generate(4, sample)
    for _ in range(REPEATS):
        for name, sample in (('greedy', None), ('sampled', SCRIPT)):
            rates[name].append(batch * STEPS / (generate(STEPS + 1, sample) - generate(1, sample)))
    res['tokens_per_s'] = rates
    return res


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _spread(v):
    return max(v) - min(v)


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == '--step':
        kind = sys.argv[2]
        setup = engine_setup() if kind == 'engine' else ()
        for n in ((1, 4, 16) if kind == 'op' else (1, 16)):
            print('%s %d ...' % (kind, n), flush=True)
            r = (step_op if kind == 'op' else step_engine)(n, *setup)
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
    cell = lambda v: '%.1f (%.1f)' % (_median(v), _spread(v))
    lines = ['### The op: [rows, %d] fp16 logits, us per call: median (max - min) of %d alternating repeats of 200 calls, device events' % (VOCAB, REPEATS), '',
             '| rows | native, T 0.8 / top-p 0.95 | native, + top-k 50 | torch.argmax | parent\'s tail (HF warpers + multinomial) | parent\'s tail, + top-k 50 |',
             '|---|---|---|---|---|---|']
    for r in results:
        if r['step'] == 'op':
            t = r['us']
            lines.append('| %d | %s | %s | %s | %s | %s |' % (r['rows'], cell(t['native']), cell(t['native_k50']), cell(t['argmax']), cell(t['hf_tail']),
                                                             cell(t['hf_tail_k50'])))
    lines += ['', '### The engine: 7B-shaped random model (scales x 0.05), 16-token prompts, %d steps: median (max - min) of %d alternating repeats' % (STEPS, REPEATS), '',
              '| batch | greedy graph us / replay | native sampling graph | parent\'s sampling graph | native - greedy | parent - native | greedy tok/s end to end | sampled tok/s end to end |',
              '|---|---|---|---|---|---|---|---|']
    for r in results:
        if r['step'] == 'engine':
            t, q = r['us_per_replay'], r['tokens_per_s']
            lines.append('| %d | %s | %s | %s | %.1f | %.1f | %s | %s |' % (
                r['batch'], cell(t['greedy']), cell(t['native']), cell(t['hf_tail']), _median(t['native']) - _median(t['greedy']),
                _median(t['hf_tail']) - _median(t['native']), cell(q['greedy']), cell(q['sampled'])))
    lines += ['', '### Raw repeats', '', '```'] + [json.dumps(r) for r in results] + ['```', '']
    text = '\n'.join(lines)
    print(text)
    if '--markdown' in sys.argv:
        with open(sys.argv[sys.argv.index('--markdown') + 1], 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
