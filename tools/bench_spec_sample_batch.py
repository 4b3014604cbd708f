"""Batched speculative sampling: what gptq_spec_sample_batch_f16 (csrc/spec_sample.hip), the verify-sample-batch graph and
engine_generate_batch(speculate=dict(sample=...)) cost.

  table 1, the kernel: R = 5 rows of [32000] fp16 logits per sequence (randn * 2.5; draft rows = target + randn * 0.7), the reference script's
           setting (temperature 0.8, top-p 0.95), B in {1, 4, 16} sequences, on the ACCEPT path (every draft is the target row's likeliest token,
           u_accept = 0) and on the REJECT path (every draft lies outside the target's kept set), without / with draft logits: ONE launch of
           gptq_spec_sample_batch_f16 against a loop of B launches of gptq_spec_sample_rows_f16 on the same rows (the only way before), each
           candidate captured as a graph of INNER calls, so the figures are device time per call.  The criterion: not slower than the loop at
           every point (B R <= 128 workgroups fit the chip at once).  The results of the two are compared bit for bit as well.
  table 2, the step: 7B-shaped random model (finite logits: scales x 0.05), DecodeEngine(batch=4, batch_chunk=5, spec_sample=True), us per replay
           of the verify-greedy-batch graph and of the verify-sample-batch graph without / with draft logits at 16 / 512 / 2027 tokens (the
           positions are put back in front of every replay, in all three).  Reported, no bar.
  table 3, generation: engine_generate_batch, 4 x (16 + 256) tokens, k = 4, aggregate tokens/s of the sample= route (capture_sample_native) under
           the script's setting, of speculate=dict(sample=...) with the prompt-lookup draft under the same setting, and with an oracle draft under
           top_k = 1 (a random draw has no oracle: the ceiling of the path, not a like-for-like setting); --draft-model adds a two-layer random
           draft model of the same vocabulary (nothing of its drafts can be expected to be accepted: the cost of the route).

Device events around a synchronised window (table 3: wall time around a synchronised call), everything warmed up, REPEATS repeats with the
candidates alternating in one process, medians and max - min spreads.  Every table is a child process under its own `timeout`; at most 16 CPU
threads.
    python tools/bench_spec_sample_batch.py [--markdown FILE] [--only kernel|step|generate] [--draft-model]"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'gptq-for-llama_amd')]
os.environ.setdefault('OMP_NUM_THREADS', '16')
REPEATS = 7
INNER = 16
VOCAB, R, K = 32000, 5, 4
SEQS = (1, 4, 16)
BATCH = 4
SCRIPT = dict(temperature=0.8, top_p=0.95)           # llama_inference.py:119-127
CONTEXTS = (16, 512, 2027)
PROMPT, NEW = 16, 256
STEP_TIMEOUT = {'kernel': 300, 'step': 900, 'generate': 1100}


def _timed(fn, inner):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / inner          # us per call


def _graph_of(call, n):
    """a graph of n calls (one eager warm-up call first)"""
    import torch
    call(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s = torch.cuda.current_stream().cuda_stream
        for _ in range(n):
            call(s)
    return g


def step_kernel():
    import torch
    from quant import _native
    lib, dev = _native.lib(), torch.device('cuda:0')
    ALWAYS = 1 << 40                                      # t_max of the batch entry: every position of the run is active
    cases = []
    for B in SEQS:
        M = B * R
        g = torch.Generator(device=dev).manual_seed(B)
        P = (torch.randn((M, VOCAB), device=dev, generator=g) * 2.5).half()
        Q = (P.float() + torch.randn((M, VOCAB), device=dev, generator=g) * 0.7).half().view(B, R, VOCAB)[:, :R - 1].reshape(B * (R - 1), VOCAB).contiguous()
        T, p = torch.full((M,), SCRIPT['temperature'], device=dev), torch.full((M,), SCRIPT['top_p'], device=dev)
        k = torch.zeros(M, dtype=torch.int32, device=dev)
        ud, ua = torch.rand(M, device=dev, generator=g), torch.zeros(M, device=dev)
        ids_acc = torch.roll(torch.argmax(P, dim=-1).view(B, R), 1, dims=1).contiguous().view(-1)     # ids[b, i + 1] = argmax of row i: accepted
        ids_rej = torch.roll(torch.argmin(P, dim=-1).view(B, R), 1, dims=1).contiguous().view(-1)     # outside the kept set: rejected
        pos, out = torch.zeros(B, dtype=torch.int64, device=dev), torch.zeros((B, R + 1), dtype=torch.int64, device=dev)
        ws = torch.zeros(lib.gptq_spec_sample_batch_workspace_bytes(B, R) // 8, dtype=torch.int64, device=dev)
        pos1, out1, ws1 = torch.zeros_like(pos), torch.zeros_like(out), torch.zeros_like(ws)

        for path, ids in (('accept', ids_acc), ('reject', ids_rej)):
            for q in (None, Q):
                qp, ldq = (q.data_ptr(), VOCAB) if q is not None else (None, 0)

                def batch(s):
                    rc = lib.gptq_spec_sample_batch_f16(P.data_ptr(), VOCAB, qp, ldq, B, R, VOCAB, ids.data_ptr(), T.data_ptr(), k.data_ptr(), p.data_ptr(),
                                                        ua.data_ptr(), ud.data_ptr(), pos.data_ptr(), ALWAYS, out.data_ptr(), ws.data_ptr(), ws.numel() * 8, s)
                    assert rc == 0, rc

                def loop(s):
                    for b in range(B):
                        o = b * R
                        rc = lib.gptq_spec_sample_rows_f16(P[o:].data_ptr(), VOCAB, q[b * (R - 1):].data_ptr() if q is not None else None, ldq, R, VOCAB,
                                                           ids[o:].data_ptr(), T[o:].data_ptr(), k[o:].data_ptr(), p[o:].data_ptr(), ua[o:].data_ptr(),
                                                           ud[o:].data_ptr(), pos1[b:].data_ptr(), out1[b].data_ptr(), ws1[b * (R + 1):].data_ptr(),
                                                           (R + 1) * 8, s)
                        assert rc == 0, rc
                graphs = dict(batch=_graph_of(batch, INNER), loop=_graph_of(loop, INNER))
                for gr in graphs.values():
                    gr.replay()
                times = {name: [] for name in graphs}
                for _ in range(REPEATS):                  # alternating
                    for name, gr in graphs.items():
                        times[name].append(_timed(gr.replay, INNER))
                torch.cuda.synchronize()
                same = bool(torch.equal(out, out1) and torch.equal(pos, pos1) and torch.equal(ws, ws1))
                cases.append(dict(seqs=B, path=path, draft_logits=q is not None, us=times, accepted=out[:, 0].tolist(), same_bits_as_the_loop=same))
                del graphs
    return dict(step='kernel', rows=R, inner=INNER, cases=cases)


def _model(seed=0, **kw):
    from quant import decode as D
    fill = D.fill_random_quant_

    def small(layer, gen):                               # bench.py's sampling leg: finite logits
        fill(layer, gen)
        layer.scales.mul_(0.05)
    D.fill_random_quant_ = small
    try:
        return D.build_random_llama('cuda:0', seed=seed, **kw)
    finally:
        D.fill_random_quant_ = fill


def step_step():
    import torch
    from quant import decode as D
    eng = D.DecodeEngine(_model(), t_max=2048, batch=BATCH, batch_chunk=R, spec_sample=True)
    eng.set_sampling(**SCRIPT)
    eng.capture_verify_greedy_batch()
    gs, gq = eng.capture_verify_sample_batch(False), eng.capture_verify_sample_batch(True)
    eng.chunk_ids.copy_(torch.randint(1, VOCAB, (BATCH, R), device='cuda:0'))
    eng.chunk_draft_logits.copy_((torch.randn(tuple(eng.chunk_draft_logits.shape), device='cuda:0') * 2.5).half())
    rows = []
    for ctx in CONTEXTS:
        def at(graph):
            def run():
                for _ in range(INNER):
                    eng.pos.fill_(ctx)
                    graph.replay()
            return lambda: _timed(run, INNER)
        cands = dict(verify_greedy=at(eng.verify_graph), verify_sample=at(gs), verify_sample_draft=at(gq))
        for f in cands.values():
            f()
        times = {name: [] for name in cands}
        for _ in range(REPEATS):
            for name, f in cands.items():
                times[name].append(f())
        rows.append(dict(context=ctx, us=times))
    return dict(step='step', batch=BATCH, rows_per_sequence=R, rows=rows)


def step_generate(draft_model):
    import time
    import torch
    from quant import decode as D
    model = _model()
    dev = 'cuda:0'
    prompts = [torch.randint(1, VOCAB, (PROMPT,), device=dev, generator=torch.Generator(device=dev).manual_seed(b)) for b in range(BATCH)]
    heads = [p.tolist() for p in prompts]
    plain = D.DecodeEngine(model, t_max=2048, batch=BATCH)
    spec = D.DecodeEngine(model, t_max=2048, batch=BATCH, batch_chunk=R, spec_sample=True)
    det = dict(SCRIPT, top_k=1)
    gen = lambda **kw: D.engine_generate_batch(model, prompts, NEW, **kw)
    known = [o.tolist() for o in gen(engine=spec, speculate=dict(k=K, sample=det))]

    def oracle(toks, k):
        f = next(s for s, h in zip(known, heads) if toks[:PROMPT] == h)
        return (f[len(toks):len(toks) + k] + [0] * k)[:k]
    legs = dict(sample_route=lambda: gen(engine=plain, sample=SCRIPT), spec_lookup=lambda: gen(engine=spec, speculate=dict(k=K, sample=SCRIPT)),
                spec_oracle_topk1=lambda: gen(engine=spec, speculate=dict(k=K, sample=det, draft=oracle)))
    if draft_model:
        small = _model(seed=1, num_hidden_layers=2)
        legs['spec_draft_model'] = lambda: gen(engine=spec, speculate=dict(k=K, sample=SCRIPT, draft_model=small))
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
            rates[name].append(BATCH * NEW / (time.perf_counter() - t0))
            if name != 'sample_route':
                st = spec.spec_stats
                stats[name] = dict(steps=st['steps'], mean_accepted=[round(sum(a) / max(1, len(a)), 2) for a in st['accepted']])
    return dict(step='generate', batch=BATCH, tok_s=rates, stats=stats, draft_model_measured=bool(draft_model))


def _med(v):
    return '%.1f (±%.1f)' % (statistics.median(v), (max(v) - min(v)) / 2)


def markdown(results, argv):
    out = ['# Batched speculative sampling: `gptq_spec_sample_batch_f16`, the verify-sample-batch graph, generation', '',
           'Written by `python %s`; medians (± half the max − min spread) of %d alternating repeats.' % (
               ' '.join(['tools/bench_spec_sample_batch.py'] + argv[1:]), REPEATS), '']
    for r in results:
        if r['step'] == 'kernel':
            out += ['## Kernel, R = 5, vocab 32 000: one launch for B sequences against a loop of B `gptq_spec_sample_rows_f16` launches '
                    '(µs per call, graphs of %d calls)' % r['inner'], '',
                    '| B | path | draft logits | batch launch | loop of B launches | loop / batch | same bits | not slower than the loop |', '|---|---|---|---|---|---|---|---|']
            for c in r['cases']:
                b, l = c['us']['batch'], c['us']['loop']
                ok = statistics.median(b) <= statistics.median(l) + max(max(b) - min(b), max(l) - min(l))
                out.append('| %d | %s | %s | %s | %s | %.2f | %s | %s |' % (c['seqs'], c['path'], 'yes' if c['draft_logits'] else 'no', _med(b), _med(l),
                                                                          statistics.median(l) / statistics.median(b),
                                                                          'yes' if c['same_bits_as_the_loop'] else 'NO', 'yes' if ok else 'NO'))
            out += ['', '"not slower": the batch median is at most the loop median plus the larger max − min spread of the two.']
            late = ['B = %d, %s path, %s draft logits: %+.2f µs' % (c['seqs'], c['path'], 'with' if c['draft_logits'] else 'without',
                                                                  statistics.median(c['us']['batch']) - statistics.median(c['us']['loop']))
                    for c in r['cases'] if statistics.median(c['us']['batch']) > statistics.median(c['us']['loop'])]
            if late:
                out += ['Points where the batch launch is the slower one (batch − loop): ' + '; '.join(late) + '.  At B = 1 the loop IS the same kernel '
                        'launched without the idle rule, so the difference is what the rule costs: one load of `pos[b]` in front of everything else '
                        'a workgroup does.  No counters were collected.']
            out += ['']
        if r['step'] == 'step':
            out += ['## Verify step, 7B shape, B = %d, R = %d (µs per replay, each including a `pos.fill_`)' % (r['batch'], r['rows_per_sequence']), '',
                    '| context | verify-greedy-batch | verify-sample-batch | verify-sample-batch + draft logits |', '|---|---|---|---|']
            out += ['| %d | %s | %s | %s |' % (x['context'], _med(x['us']['verify_greedy']), _med(x['us']['verify_sample']), _med(x['us']['verify_sample_draft']))
                    for x in r['rows']]
            out += ['']
        if r['step'] == 'generate':
            out += ['## `engine_generate_batch`, %d × (16 + 256) tokens, k = 4 (aggregate tokens/s, prefill included)' % r['batch'], '',
                    '| route | tok/s | steps, mean accepted per sequence |', '|---|---|---|']
            out += ['| %s | %s | %s |' % (n, _med(v), '%d, %r' % (r['stats'][n]['steps'], r['stats'][n]['mean_accepted']) if n in r['stats'] else '')
                    for n, v in r['tok_s'].items()]
            if not r['draft_model_measured']:
                out += ['| spec_draft_model | not measured | |']
            out += ['']
    out += ['## Raw repeats', '', '```'] + [json.dumps(r) for r in results] + ['```']
    return '\n'.join(out)


def main(argv):
    if len(argv) > 1 and argv[1] == '--child':
        import torch
        torch.set_num_threads(min(16, torch.get_num_threads()))
        with torch.no_grad():
            fn = {'kernel': step_kernel, 'step': step_step, 'generate': lambda: step_generate('--draft-model' in argv)}[argv[2]]
            print('RESULT ' + json.dumps(fn()), flush=True)
        return 0
    only = argv[argv.index('--only') + 1] if '--only' in argv else None
    results = []
    for step in ('kernel', 'step', 'generate'):
        if only and step != only:
            continue
        cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT[step]), sys.executable, os.path.abspath(__file__), '--child', step]
        cp = subprocess.run(cmd + (['--draft-model'] if '--draft-model' in argv else []), stdout=subprocess.PIPE, text=True)
        if cp.returncode != 0:                              # nothing more is started on the GPU behind a step that failed
            print('step %s ended with status %d' % (step, cp.returncode), file=sys.stderr)
            return cp.returncode
        results.append(json.loads([l for l in cp.stdout.splitlines() if l.startswith('RESULT ')][-1][7:]))
        print(json.dumps(results[-1]), flush=True)
    text = markdown(results, [a for a in argv if a != '--markdown' and not a.endswith('.md')])
    print(text)
    if '--markdown' in argv:
        path = argv[argv.index('--markdown') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
