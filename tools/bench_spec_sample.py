"""Speculative sampling: what gptq_spec_sample_rows_f16 (csrc/spec_sample.hip), the verify-sample graph and engine_generate(speculate=dict(sample=...))
cost.

  table 1, the kernel: one launch on R = 5 rows of [32000] fp16 logits (randn * 2.5; draft rows = target + randn * 0.7), the reference script's
           setting (temperature 0.8, top-p 0.95), with and without draft logits, on the ACCEPT path (every draft is the target row's likeliest
           token, u_accept = 0: two selects with draft logits, no residual) and on the REJECT path (every draft lies outside the target's kept set:
           the residual sum and the draw on top); next to gptq_sample_rows_f16 on the same 5 rows in the same run.  The expectation to confirm or
           refute: <= 2 x that kernel.
  table 2, the step: 7B-shaped random model (finite logits: scales x 0.05), DecodeEngine(chunk=5), us per replay of the verify-greedy graph and of
           the verify-sample graph without / with draft logits, at 16 / 512 / 1024 / 2027 tokens of context (the position is put back in front of
           every replay, in all three).
  table 3, generation: engine_generate, 16 + 256 tokens, k = 4, tokens/s of the sample= route (capture_sample_native) under the script's setting,
           of speculate=dict(sample=...) with the prompt-lookup draft under the same setting, and with an oracle draft.  A random draw has no
           oracle, so that leg adds top_k = 1 (deterministic: every draft is accepted) -- the ceiling of the verify-sample path, not a
           like-for-like setting.

Device events around a synchronised window, everything warmed up, REPEATS repeats with the candidates alternating in one process, medians and
max - min spreads.  Every table is a child process under its own `timeout`; at most 16 CPU threads.
    python tools/bench_spec_sample.py [--markdown FILE] [--only kernel|step|generate]"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'gptq-for-llama_amd')]
os.environ.setdefault('OMP_NUM_THREADS', '16')
REPEATS = 7
VOCAB, R, K = 32000, 5, 4
SCRIPT = dict(temperature=0.8, top_p=0.95)           # llama_inference.py:119-127
CONTEXTS = (16, 512, 1024, 2027)
PROMPT, NEW = 16, 256
STEP_TIMEOUT = {'kernel': 300, 'step': 900, 'generate': 900}


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


def _alternate(cands, inner):
    for f in cands.values():
        for _ in range(3):
            f()
    times = {name: [] for name in cands}
    for _ in range(REPEATS):
        for name, f in cands.items():
            times[name].append(_timed(f, inner))
    return times


def step_kernel():
    import torch
    from quant import _native
    lib, dev = _native.lib(), torch.device('cuda:0')
    s = _native.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(R)
    P = (torch.randn((R, VOCAB), device=dev, generator=g) * 2.5).half()
    Q = (P.float() + torch.randn((R, VOCAB), device=dev, generator=g) * 0.7).half()[:R - 1].contiguous()
    T, p = torch.full((R,), SCRIPT['temperature'], device=dev), torch.full((R,), SCRIPT['top_p'], device=dev)
    k = torch.zeros(R, dtype=torch.int32, device=dev)
    ud = torch.rand(R, device=dev, generator=g)
    ua = torch.zeros(R, device=dev)
    first = torch.zeros(1, dtype=torch.int64, device=dev)
    ids_acc = torch.cat([first, torch.argmax(P[:R - 1], dim=-1)])          # p(d) > 0 and u_accept = 0: every row accepts
    ids_rej = torch.cat([first, torch.argmin(P[:R - 1], dim=-1)])          # outside the kept set: every row rejects
    pos, out = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(R + 1, dtype=torch.int64, device=dev)
    ws = torch.zeros(lib.gptq_spec_sample_workspace_bytes(R) // 8, dtype=torch.int64, device=dev)
    ids_out = torch.empty(R, dtype=torch.int64, device=dev)

    def spec(q, ids):
        def run():
            rc = lib.gptq_spec_sample_rows_f16(P.data_ptr(), VOCAB, q.data_ptr() if q is not None else None, VOCAB if q is not None else 0, R, VOCAB,
                                               ids.data_ptr(), T.data_ptr(), k.data_ptr(), p.data_ptr(), ua.data_ptr(), ud.data_ptr(), pos.data_ptr(),
                                               out.data_ptr(), ws.data_ptr(), ws.numel() * 8, s)
            assert rc == 0, rc
        return run

    def sample():
        rc = lib.gptq_sample_rows_f16(P.data_ptr(), VOCAB, R, VOCAB, ud.data_ptr(), T.data_ptr(), k.data_ptr(), p.data_ptr(), ids_out.data_ptr(), s)
        assert rc == 0, rc
    cands = dict(sample_rows=sample, point_accept=spec(None, ids_acc), point_reject=spec(None, ids_rej), draft_accept=spec(Q, ids_acc),
                 draft_reject=spec(Q, ids_rej))
    times = _alternate(cands, 200)
    spec(Q, ids_acc)()
    accepted = int(out[0])
    spec(Q, ids_rej)()
    return dict(step='kernel', us=times, accepted_on_accept_path=accepted, accepted_on_reject_path=int(out[0]))


def _model():
    from quant import decode as D
    fill = D.fill_random_quant_

    def small(layer, gen):                               # bench.py's sampling leg: finite logits
        fill(layer, gen)
        layer.scales.mul_(0.05)
    D.fill_random_quant_ = small
    try:
        return D.build_random_llama('cuda:0', seed=0)
    finally:
        D.fill_random_quant_ = fill


def step_step():
    import torch
    from quant import decode as D
    eng = D.DecodeEngine(_model(), t_max=2048, chunk=R)
    eng.set_sampling(**SCRIPT)
    eng.capture_verify_greedy()
    gs, gq = eng.capture_verify_sample(False), eng.capture_verify_sample(True)
    eng.chunk_ids.copy_(torch.randint(1, VOCAB, (R,), device='cuda:0'))
    eng.chunk_draft_logits.copy_((torch.randn((R - 1, eng.chunk_logits.shape[1]), device='cuda:0') * 2.5).half())
    rows = []
    for ctx in CONTEXTS:
        def at(graph):
            def run():
                eng.pos.fill_(ctx)
                graph.replay()
            return run
        rows.append(dict(context=ctx, us=_alternate(dict(verify_greedy=at(eng.verify_graph), verify_sample=at(gs), verify_sample_draft=at(gq)), 20)))
    return dict(step='step', rows=rows)


def step_generate():
    import time
    import torch
    from quant import decode as D
    model = _model()
    prompt = torch.randint(1, VOCAB, (1, PROMPT), device='cuda:0', generator=torch.Generator(device='cuda:0').manual_seed(1))
    plain = D.DecodeEngine(model, t_max=2048).capture()
    spec = D.DecodeEngine(model, t_max=2048, chunk=R)
    det = dict(SCRIPT, top_k=1)
    known = D.engine_generate(model, prompt, NEW, engine=spec, prefill='engine', speculate=dict(k=K, sample=det))[0].tolist()
    oracle = lambda toks, k: (known[len(toks):len(toks) + k] + [0] * k)[:k]
    legs = dict(sample_route=lambda: D.engine_generate(model, prompt, NEW, engine=plain, prefill='engine', sample=SCRIPT),
                spec_lookup=lambda: D.engine_generate(model, prompt, NEW, engine=spec, prefill='engine', speculate=dict(k=K, sample=SCRIPT)),
                spec_oracle_topk1=lambda: D.engine_generate(model, prompt, NEW, engine=spec, prefill='engine',
                                                            speculate=dict(k=K, sample=det, draft=oracle)))
    rates, stats = {n: [] for n in legs}, {}
    for f in legs.values():
        f()
    for rep in range(REPEATS):
        for name, f in legs.items():
            torch.manual_seed(rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            rates[name].append(NEW / (time.perf_counter() - t0))
            if name != 'sample_route':
                st = spec.spec_stats
                stats[name] = dict(steps=st['steps'], mean_accepted=sum(st['accepted']) / max(1, st['steps']))
    return dict(step='generate', tok_s=rates, stats=stats)


def _med(v):
    return '%.1f (±%.1f)' % (statistics.median(v), (max(v) - min(v)) / 2)


def markdown(results):
    out = ['# Speculative sampling: `gptq_spec_sample_rows_f16`, the verify-sample graph, generation', '',
           'Written by `python tools/bench_spec_sample.py --markdown profiles/spec_sample/README.md`; medians (± half the max − min spread) of %d '
           'alternating repeats.' % REPEATS, '']
    for r in results:
        if r['step'] == 'kernel':
            base = statistics.median(r['us']['sample_rows'])
            out += ['## Kernel, R = 5, vocab 32 000 (µs per launch)', '', '| launch | µs | × `gptq_sample_rows_f16` (5 rows) |', '|---|---|---|']
            out += ['| %s | %s | %.2f |' % (n, _med(v), statistics.median(v) / base) for n, v in r['us'].items()]
            out += ['', 'accepted rows on the accept path: %d of 4, on the reject path: %d' % (r['accepted_on_accept_path'], r['accepted_on_reject_path']), '']
        if r['step'] == 'step':
            out += ['## Verify step, 7B shape, R = 5 (µs per replay)', '', '| context | verify-greedy | verify-sample | verify-sample + draft logits |', '|---|---|---|---|']
            out += ['| %d | %s | %s | %s |' % (x['context'], _med(x['us']['verify_greedy']), _med(x['us']['verify_sample']), _med(x['us']['verify_sample_draft']))
                    for x in r['rows']]
            out += ['']
        if r['step'] == 'generate':
            out += ['## `engine_generate`, 16 + 256 tokens, k = 4 (tokens/s)', '', '| route | tok/s | steps, mean accepted |', '|---|---|---|']
            out += ['| %s | %s | %s |' % (n, _med(v), '%(steps)d, %(mean_accepted).2f' % r['stats'][n] if n in r['stats'] else '') for n, v in r['tok_s'].items()]
            out += ['']
    return '\n'.join(out)


def main(argv):
    if len(argv) > 1 and argv[1] == '--child':
        import torch
        torch.set_num_threads(min(16, torch.get_num_threads()))
        with torch.no_grad():
            print('RESULT ' + json.dumps({'kernel': step_kernel, 'step': step_step, 'generate': step_generate}[argv[2]]()), flush=True)
        return 0
    only = argv[argv.index('--only') + 1] if '--only' in argv else None
    results = []
    for step in ('kernel', 'step', 'generate'):
        if only and step != only:
            continue
        cp = subprocess.run(['timeout', '-k', '10', str(STEP_TIMEOUT[step]), sys.executable, os.path.abspath(__file__), '--child', step],
                            stdout=subprocess.PIPE, text=True)
        if cp.returncode != 0:                              # nothing more is started on the GPU behind a step that failed
            print('step %s ended with status %d' % (step, cp.returncode), file=sys.stderr)
            return cp.returncode
        results.append(json.loads([l for l in cp.stdout.splitlines() if l.startswith('RESULT ')][-1][7:]))
        print(json.dumps(results[-1]), flush=True)
    text = markdown(results)
    print(text)
    if '--markdown' in argv:
        path = argv[argv.index('--markdown') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
