"""Beam search in the engine: what gptq_beam_select_f16 and gptq_kv_reorder_f16 (csrc/beam.hip) cost, what the beam step costs next to the
greedy step of the same engine, and engine_generate_beam against the only route the parent commit has for beams.

  table 1, select: one call (two launches) on [N, 32000] fp16 logits (randn * 3), N in {4, 8, 16}; the state advances from t = 5 through the
           200 calls of a window (no EOS, t_cap 2048: never done) and is put back between windows.
  table 2, reorder: the 7B cache shape (32 layers, H = 4096, t_max 2048), N = 4, len in {16, 512, 2047}, parent (1, 2, 3, 0) (every row changes)
           and the identity; achieved bytes/s from 2 (k, v) x changed rows x layers x len x H x 2 B read and the same written.
  table 3, the step: 7B-shaped random model (scales x 0.05: finite logits), DecodeEngine(batch=4, beam_search=True): us per replay of the
           capture_beam_step graph against the same engine's capture_greedy_rows graph at 16 / 512 / 2027 tokens of context, 16 replays a window.
  table 4, end to end: engine_generate_beam(num_beams=4), a 16-token prompt + 128 tokens, against model.generate(num_beams=4,
           max_new_tokens=128) through the installed hook (which switches itself off for beams: the eager module chain), alternating in one
           process; tokens of the best hypothesis per second, (t(129 tokens) - t(1 token)) / 128.

Device events around a synchronised window (wall clock end to end), everything warmed up, REPEATS alternating repeats, medians and max - min
spreads (raw repeats printed too).  Every table is a child process under its own `timeout`; at most 16 CPU threads.
    python tools/bench_beam.py [--markdown FILE] [--only select|reorder|engine]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'gptq-for-llama_amd')]
os.environ.setdefault('OMP_NUM_THREADS', '16')
REPEATS = 5
VOCAB = 32000
T_MAX = 2048
LAYERS, H = 32, 4096
WINDOW = 16
NEW = 128
STEP_TIMEOUT = {'select': 200, 'reorder': 200, 'engine': 900}


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


def step_select():
    import numpy as np
    import torch
    from quant import _native, decode as D
    lib, dev = _native.lib(), torch.device('cuda:0')
    s = _native.stream_ptr(dev)
    cands = {}
    for N in (4, 8, 16):
        g = torch.Generator(device=dev).manual_seed(N)
        logits = (torch.randn((N, VOCAB), device=dev, generator=g) * 3).half()
        w = np.zeros(lib.gptq_beam_state_bytes(N, T_MAX) // 4, dtype=np.int32)
        f = w.view(np.float32)
        w[D.BEAM_W_EOS], w[D.BEAM_W_MAX_NEW], w[D.BEAM_W_T_CAP], w[D.BEAM_W_BEAMS], w[D.BEAM_W_T], w[D.BEAM_W_OPEN] = -1, T_MAX, T_MAX, N, 5, 1
        f[D.BEAM_W_LP] = 1.0
        f[D.BEAM_W_SCORE:D.BEAM_W_SCORE + 16] = -np.arange(16) * 0.25 - 1
        f[D.BEAM_W_POOL:D.BEAM_W_CAND:5] = D.BEAM_DEAD
        start = torch.from_numpy(w).to(dev)
        state = start.clone()

        def run(N=N, logits=logits, state=state):
            rc = lib.gptq_beam_select_f16(logits.data_ptr(), VOCAB, N, VOCAB, state.data_ptr(), s)
            assert rc == 0, rc
        cands['N%d' % N] = (run, state, start)
    for run, state, start in cands.values():
        for _ in range(5):
            run()
    times = {name: [] for name in cands}
    for _ in range(REPEATS):
        for name, (run, state, start) in cands.items():
            state.copy_(start)                               # outside the window: t = 5 again, so no call of the window reaches t_cap
            times[name].append(_timed(run, 200))
    torch.cuda.synchronize()
    for name, (run, state, start) in cands.items():
        assert int(state[D.BEAM_W_T]) == 205 and not int(state[D.BEAM_W_DONE]) and not int(state[D.BEAM_W_STATUS]), name
    return dict(step='select', us=times)


def step_reorder():
    import torch
    from quant import _native
    lib, dev = _native.lib(), torch.device('cuda:0')
    s = _native.stream_ptr(dev)
    N = 4
    k = torch.zeros((LAYERS, N, T_MAX, H), dtype=torch.float16, device=dev)
    v = torch.zeros_like(k)
    parents = dict(all=torch.tensor([1, 2, 3, 0], dtype=torch.int32, device=dev), identity=torch.arange(N, dtype=torch.int32, device=dev))
    cands = {}
    for name, par in parents.items():
        for n in (16, 512, 2047):
            ln = torch.tensor([n], dtype=torch.int64, device=dev)

            def run(par=par, ln=ln):
                rc = lib.gptq_kv_reorder_f16(k.data_ptr(), v.data_ptr(), LAYERS, N, T_MAX, H, k.stride(0), par.data_ptr(), ln.data_ptr(), s)
                assert rc == 0, rc
            cands['%s_%d' % (name, n)] = run
    for fn in cands.values():
        for _ in range(3):
            fn()
    times = {name: [] for name in cands}
    for _ in range(REPEATS):
        for name, fn in cands.items():
            times[name].append(_timed(fn, 20))
    return dict(step='reorder', us=times, bytes_each_way={str(n): 2 * N * LAYERS * n * H * 2 for n in (16, 512, 2047)})


def step_engine():
    import time
    import torch
    from quant import decode as D
    torch.set_num_threads(min(16, torch.get_num_threads()))
    fill = D.fill_random_quant_

    def small(layer, gen):                               # bench.py's sampling leg: finite logits
        fill(layer, gen)
        layer.scales.mul_(0.05)
    D.fill_random_quant_ = small
    try:
        model = D.build_random_llama('cuda:0', seed=0)
    finally:
        D.fill_random_quant_ = fill
    dev = torch.device('cuda:0')
    N = 4
    eng = D.DecodeEngine(model, t_max=T_MAX, batch=N, beam_search=True)
    eng.graph_for('beam')
    eng.graph_for('greedy_rows')
    gen = torch.Generator(device=dev).manual_seed(1)
    prompt = torch.randint(1, VOCAB, (1, 16), device=dev, generator=gen)

    def window(kind, ctx):
        eng.set_beam_search(T_MAX)
        eng.pos.fill_(ctx)
        eng.ids.copy_(prompt[0, :N])
        eng.stepc.zero_()
        return _timed((eng.beam_graph if kind == 'beam' else eng.greedy_rows_graph).replay, WINDOW)
    cands = [(kind, ctx) for ctx in (16, 512, 2027) for kind in ('greedy', 'beam')]
    for c in cands:
        window(*c)
    times = {'%s_%d' % c: [] for c in cands}
    for _ in range(REPEATS):
        for c in cands:
            times['%s_%d' % c].append(window(*c))
    res = dict(step='engine', window=WINDOW, us_per_replay=times)

    def engine_route(n):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        seqs, _ = D.engine_generate_beam(model, prompt, n, num_beams=N, engine=eng)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, seqs[0].numel() - prompt.shape[1]

    def hf_route(n):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        with torch.no_grad():
            out = model.generate(prompt, do_sample=False, num_beams=N, max_new_tokens=n, pad_token_id=0)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out.shape[1] - prompt.shape[1]
    routes = dict(engine=engine_route, hf=hf_route)
    rates = {name: [] for name in routes}
    for fn in routes.values():
        fn(4)
    for _ in range(REPEATS):
        for name, fn in routes.items():
            (tn, got), (t1, _) = fn(NEW + 1), fn(1)
            assert got == NEW + 1, (name, got)
            rates[name].append(NEW / (tn - t1))
    res['tokens_per_s'] = rates
    return res


STEPS = dict(select=step_select, reorder=step_reorder, engine=step_engine)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == '--step':
        print('%s ...' % sys.argv[2], flush=True)
        print('RESULT ' + json.dumps(STEPS[sys.argv[2]]()), flush=True)
        return 0
    kinds = [sys.argv[sys.argv.index('--only') + 1]] if '--only' in sys.argv else list(STEPS)
    results = {}
    for kind in kinds:
        cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT[kind]), sys.executable, os.path.abspath(__file__), '--step', kind]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
        for line in p.stdout:                            # streamed: a long step still shows progress
            print(line.rstrip(), flush=True)
            if line.startswith('RESULT '):
                results[kind] = json.loads(line[7:])
        if p.wait() != 0:                                # a fault, an abort or a time limit: nothing more is started on the GPU
            print('step %s ended with status %d: stopping' % (kind, p.returncode))
            return 1
    cell = lambda v: '%.1f (%.1f)' % (_median(v), max(v) - min(v))
    head = 'median (max - min) of %d alternating repeats' % REPEATS
    lines = []
    if 'select' in results:
        t = results['select']['us']
        lines += ['### gptq_beam_select_f16 on [N, %d] fp16 logits, us per call (two launches), 200 consecutive steps of one search a window: %s' % (
            VOCAB, head), '', '| N | us per call |', '|---|---|']
        lines += ['| %d | %s |' % (N, cell(t['N%d' % N])) for N in (4, 8, 16)]
    if 'reorder' in results:
        r = results['reorder']
        lines += ['', '### gptq_kv_reorder_f16, 32 layers, H = 4096, t_max 2048, N = 4: us per launch and achieved GB/s (read + write) where every '
                  'row changes; the identity step: %s' % head, '', '| len | all rows change, us | GB/s | identity, us |', '|---|---|---|---|']
        for n in (16, 512, 2047):
            us = _median(r['us']['all_%d' % n])
            lines.append('| %d | %s | %.0f | %s |' % (n, cell(r['us']['all_%d' % n]), 2 * r['bytes_each_way'][str(n)] / us / 1e3,
                                                     cell(r['us']['identity_%d' % n])))
    if 'engine' in results:
        r = results['engine']
        t, q = r['us_per_replay'], r['tokens_per_s']
        lines += ['', '### The step: 7B-shaped random model, batch 4, us per replay over %d replays: %s' % (r['window'], head), '',
                  '| context | capture_greedy_rows | capture_beam_step | beam / greedy |', '|---|---|---|---|']
        for ctx in (16, 512, 2027):
            g, b = t['greedy_%d' % ctx], t['beam_%d' % ctx]
            lines.append('| %d | %s | %s | %.3f |' % (ctx, cell(g), cell(b), _median(b) / _median(g)))
        lines += ['', '### End to end: 4 beams, 16 + %d tokens, tokens of the best hypothesis per second: %s' % (NEW, head), '',
                  '| model.generate(num_beams=4) through the hook (the parent\'s route) | engine_generate_beam | engine / parent |', '|---|---|---|',
                  '| %s | %s | %.2f |' % (cell(q['hf']), cell(q['engine']), _median(q['engine']) / _median(q['hf']))]
    lines += ['', '### Raw repeats', '', '```'] + [json.dumps(r) for r in results.values()] + ['```', '']
    text = '\n'.join(lines)
    print(text)
    if '--markdown' in sys.argv:
        with open(sys.argv[sys.argv.index('--markdown') + 1], 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
