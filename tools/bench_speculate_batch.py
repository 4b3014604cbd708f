"""Batched speculative decoding in the engine: what verifying R tokens of B sequences per step costs and what it can buy.

  table a, the attention call alone, 32 heads, t_max 2048, R = 5 rows of B in {4, 16} sequences, every sequence at position p in {16, 512, 2042}:
           gptq_decode_attn_chunk_batch_f16 (csrc/chunk_attn.hip: two launches for all sequences) against a loop of B calls of
           gptq_decode_attn_chunk_f16 on the same slots (2 B launches: the only way to do it before).  Each candidate is captured as a graph of
           INNER calls (a call of the loop candidate = its B calls), so the figures are device time per call without the host's launch cost.
  table b, step graphs of ONE engine DecodeEngine(batch=4, batch_chunk=5) on the 7B-shaped random model: the verify-greedy-batch graph
           (capture_verify_greedy_batch: 20 rows through every layer, accept rule on the device) against the decode step graph of the same
           engine (4 rows), from 16 / 512 / 2027 tokens on.  c = t_verify / t_step: speculation pays when a step emits more than c tokens per
           sequence on average, i.e. accepts more than c - 1 drafts.  The drafts are random ids (nothing is accepted: every replay advances every
           position by one, like the decode step).
  table c, end to end: engine_generate_batch, 4 prompts of 16 tokens + 256 new tokens each, k = 4, aggregate tokens/s of plain greedy against two
           synthetic drafts that bound every real one -- an ORACLE that replays a previous run (the ceiling) and an ADVERSARIAL draft,
           (greedy token + 1) % vocab (nothing accepted: the worst-case overhead).  Real acceptance rates need real text and a real checkpoint.

Device events around a synchronised window (table c: wall time around a synchronised call), everything warmed up, REPEATS repeats with the
candidates alternating in one process, medians and max - min spreads (raw repeats printed too).  The attention table and the two engine tables
are child processes under their own `timeout`; at most 16 CPU threads.
    python tools/bench_speculate_batch.py [--markdown FILE] [--only attn|engine]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'gptq-for-llama_amd')]
os.environ.setdefault('OMP_NUM_THREADS', '16')
REPEATS = 7
HEADS, HD, T_MAX = 32, 128, 2048
H = HEADS * HD
INNER = 16
ROWS = 5
ATTN_SEQS = (4, 16)
ATTN_POSITIONS = (16, 512, 2042)
BATCH = 4
STEP_CONTEXTS = (16, 512, 2027)
NEW, PROMPT, K = 256, 16, 4
STEP_TIMEOUT = {'attn': 300, 'engine': 900}


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


def step_attn(B):
    import numpy as np
    import torch
    from quant import _native
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lib, dev, R = _native.lib(), torch.device('cuda:0'), ROWS
    gen = torch.Generator(device=dev).manual_seed(B)
    f16 = dict(dtype=torch.float16, device=dev)
    qkv = torch.randn((B * R, 3 * H), generator=gen, **f16)
    kc = torch.randn((B, T_MAX, H), generator=gen, **f16) * 0.5
    vc = torch.randn((B, T_MAX, H), generator=gen, **f16)
    out = torch.zeros((B * R, H), **f16)
    tab = torch.empty((T_MAX, HD // 2, 2), dtype=torch.float32, device=dev)
    assert lib.gptq_rope_table_f32(tab.data_ptr(), T_MAX, HD, 10000.0, _native.stream_ptr(dev)) == 0
    ws_b = torch.zeros(lib.gptq_decode_attn_chunk_batch_workspace_bytes(B, R, HEADS, HD, T_MAX), dtype=torch.uint8, device=dev)
    ws_1 = torch.zeros(lib.gptq_decode_attn_chunk_workspace_bytes(R, HEADS, HD, T_MAX), dtype=torch.uint8, device=dev)
    scale = float(1.0 / np.sqrt(HD))
    res = []
    for p in ATTN_POSITIONS:
        pos = torch.full((B,), p, dtype=torch.int64, device=dev)

        def batch(s):
            rc = lib.gptq_decode_attn_chunk_batch_f16(qkv.data_ptr(), 3 * H, B, R, pos.data_ptr(), kc.data_ptr(), vc.data_ptr(), T_MAX * H, out.data_ptr(),
                                                      H, ws_b.data_ptr(), ws_b.numel(), HEADS, HD, T_MAX, 10000.0, scale, tab.data_ptr(), s)
            assert rc == 0, rc

        def loop(s):
            for b in range(B):
                rc = lib.gptq_decode_attn_chunk_f16(qkv[b * R:].data_ptr(), 3 * H, R, pos[b:].data_ptr(), kc[b].data_ptr(), vc[b].data_ptr(),
                                                    out[b * R:].data_ptr(), H, ws_1.data_ptr(), ws_1.numel(), HEADS, HD, T_MAX, 10000.0, scale,
                                                    tab.data_ptr(), s)
                assert rc == 0, rc
        loop(_native.stream_ptr(dev))
        torch.cuda.synchronize()
        expect = out.clone()
        out.zero_()
        batch(_native.stream_ptr(dev))
        torch.cuda.synchronize()
        same = bool(torch.equal(out.view(torch.int16), expect.view(torch.int16)))
        graphs = dict(batch=_graph_of(batch, INNER), loop=_graph_of(loop, INNER))
        for g in graphs.values():
            g.replay()
        times = {name: [] for name in graphs}
        for _ in range(REPEATS):                         # alternating
            for name, g in graphs.items():
                times[name].append(_timed(g.replay, INNER))
        res.append(dict(p=p, us=times, splits=lib.gptq_decode_attn_chunk_splits(HEADS, HD, T_MAX, p + R), same_bits_as_the_loop=same))
        del graphs
    return dict(step='attn', seqs=B, rows=R, inner=INNER, cases=res)


def model_setup():
    import torch
    from quant import decode as D
    torch.set_num_threads(min(16, torch.get_num_threads()))
    fill = D.fill_random_quant_

    def small(layer, gen):                               # bench.py's sampling leg: finite logits
        fill(layer, gen)
        layer.scales.mul_(0.05)
    D.fill_random_quant_ = small
    try:
        return D.build_random_llama('cuda:0', seed=0)
    finally:
        D.fill_random_quant_ = fill


def step_steps(model, eng):
    import torch
    dev, B, R = torch.device('cuda:0'), BATCH, ROWS
    gen = torch.Generator(device=dev).manual_seed(R)
    eng.kcb.normal_(0, 0.5, generator=gen)
    eng.vcb.normal_(0, 0.5, generator=gen)
    eng.pos.zero_()
    eng.capture()
    eng.capture_verify_greedy_batch()
    vocab = model.config.vocab_size
    ids1 = torch.randint(1, vocab, (B,), device=dev, generator=gen)
    idsR = torch.randint(1, vocab, (B, R), device=dev, generator=gen)
    res = []
    for ctx in STEP_CONTEXTS:
        start = min(ctx, T_MAX - R - INNER)              # INNER replays, one position each, the chunk still fits at the last

        def run_verify():
            eng.pos.fill_(start); eng.chunk_ids.copy_(idsR)
            return _timed(lambda: [eng.verify_batch_graph.replay() for _ in range(INNER)], INNER)

        def run_decode():
            eng.pos.fill_(start); eng.ids.copy_(ids1)
            return _timed(lambda: [eng.graph.replay() for _ in range(INNER)], INNER)
        cands = dict(verify=run_verify, decode=run_decode)
        for f in cands.values():
            f()
        eng.pos.fill_(start); eng.chunk_ids.copy_(idsR)
        eng.verify_batch_graph.replay()
        accepted = eng.verify_out[:, 0].tolist()
        times = {name: [] for name in cands}
        for _ in range(REPEATS):
            for name, f in cands.items():
                times[name].append(f())
        res.append(dict(start=start, us=times, accepted_by_the_random_draft=accepted))
    return dict(step='steps', batch=B, rows=R, inner=INNER, cases=res)


def step_e2e(model, eng):
    import time
    import torch
    from quant import decode as D
    dev, B = torch.device('cuda:0'), BATCH
    vocab = model.config.vocab_size
    prompts = [torch.randint(1, vocab, (PROMPT,), device=dev, generator=torch.Generator(device=dev).manual_seed(b)) for b in range(B)]
    heads = [p.tolist() for p in prompts]

    def plain(n=NEW):
        return D.engine_generate_batch(model, prompts, n, engine=eng)

    def spec(draft, n=NEW):
        return D.engine_generate_batch(model, prompts, n, engine=eng, speculate=dict(k=K, draft=draft))

    def by_prompt(seqs):
        """drafts are asked per sequence, without its index: the known sequence that starts with the same prompt"""
        return lambda toks: next(s for s, h in zip(seqs, heads) if toks[:PROMPT] == h)
    greedy = [g.tolist() for g in plain()]
    # the oracle replays a previous run.  A verify step and a decode step round differently, so a near tie can send the speculative run down
    # another (equally greedy) path than the plain one: the oracle is then refined with the speculative run's own output
    known = greedy
    for _ in range(4):
        oracle = (lambda find: (lambda toks, k: (find(toks)[len(toks):len(toks) + k] + [0] * k)[:k]))(by_prompt([list(s) for s in known]))
        out = spec(oracle)
        st = eng.spec_stats
        known = [o.tolist() for o in out]
        if all(a == K for acc in st['accepted'] for a in acc[:-1]):
            break
    oracle_stats = dict(st)
    find = by_prompt(greedy)
    adversarial = lambda toks, k: [((find(toks)[len(toks) + j] if len(toks) + j < PROMPT + NEW else 0) + 1) % vocab for j in range(k)]
    adv_out = spec(adversarial)
    adv_stats = dict(eng.spec_stats)
    agree = dict(oracle=[sum(int(a == b) for a, b in zip(o.tolist(), g)) - PROMPT for o, g in zip(out, greedy)],
                 adversarial=[sum(int(a == b) for a, b in zip(o.tolist(), g)) - PROMPT for o, g in zip(adv_out, greedy)])

    def rate(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn(NEW)
        torch.cuda.synchronize(); tn = time.perf_counter() - t0
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn(1)
        torch.cuda.synchronize(); t1 = time.perf_counter() - t0
        return B * (NEW - 1) / (tn - t1)                 # decode part only, all sequences together
    cands = dict(greedy=plain, oracle=lambda n: spec(oracle, n), adversarial=lambda n: spec(adversarial, n))
    for f in cands.values():
        f(8)
    rates = {name: [] for name in cands}
    for _ in range(REPEATS):
        for name, f in cands.items():
            rates[name].append(rate(f))
    summary = lambda s: dict(steps=s['steps'], emitted=s['emitted'], mean_accepted_per_step=[sum(a) / max(1, len(a)) for a in s['accepted']])
    return dict(step='e2e', batch=B, prompt=PROMPT, new=NEW, k=K, tokens_per_s=rates, oracle=summary(oracle_stats), adversarial=summary(adv_stats),
                tokens_equal_to_plain_greedy_of_256=agree)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _spread(v):
    return max(v) - min(v)


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == '--step':
        kind = sys.argv[2]
        if kind == 'attn':
            for B in ATTN_SEQS:
                print('attn %d ...' % B, flush=True)
                print('RESULT ' + json.dumps(step_attn(B)), flush=True)
            return 0
        from quant import decode as D
        model = model_setup()
        eng = D.DecodeEngine(model, t_max=T_MAX, batch=BATCH, batch_chunk=ROWS)
        for name, fn in (('steps', step_steps), ('e2e', step_e2e)):
            print('%s ...' % name, flush=True)
            print('RESULT ' + json.dumps(fn(model, eng)), flush=True)
        return 0
    kinds = [sys.argv[sys.argv.index('--only') + 1]] if '--only' in sys.argv else ['attn', 'engine']
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

    def verdict(ours, other):
        """not slower, with the margin of the larger max - min spread of the two"""
        return 'yes' if _median(ours) <= _median(other) + max(_spread(ours), _spread(other)) else 'NO'
    lines = []
    if any(r['step'] == 'attn' for r in results):
        lines += ['### (a) The attention call alone: %d heads, t_max %d, R = %d, us per call: median (max - min) of %d alternating repeats of a graph of %d calls' % (
                      HEADS, T_MAX, ROWS, REPEATS, INNER), '',
                  '| sequences B | position p (all) | splits | gptq_decode_attn_chunk_batch_f16 (2 launches) | B x gptq_decode_attn_chunk_f16 (2 B launches) | loop / batch | same bits | not slower than the loop |',
                  '|---|---|---|---|---|---|---|---|']
        for r in results:
            if r['step'] == 'attn':
                for c in r['cases']:
                    t = c['us']
                    lines.append('| %d | %d | %d | %s | %s | %.2f | %s | %s |' % (
                        r['seqs'], c['p'], c['splits'], cell(t['batch']), cell(t['loop']), _median(t['loop']) / _median(t['batch']),
                        'yes' if c['same_bits_as_the_loop'] else 'NO', verdict(t['batch'], t['loop'])))
        lines.append('')
    for r in results:
        if r['step'] == 'steps':
            lines += ['### (b) Step graphs, 7B-shaped random model (scales x 0.05), DecodeEngine(batch=%d, batch_chunk=%d), us per replay: median (max - min) of %d alternating repeats of %d replays' % (
                          r['batch'], r['rows'], REPEATS, INNER), '',
                      '| first position | verify-greedy-batch graph (%d rows) | decode step graph (%d rows) | c = verify / decode | speculation pays above this many accepted drafts per step and sequence (c - 1) |' % (
                          r['batch'] * r['rows'], r['batch']), '|---|---|---|---|---|']
            for c in r['cases']:
                t = c['us']
                ratio = _median(t['verify']) / _median(t['decode'])
                lines.append('| %d | %s | %s | %.3f | %.2f |' % (c['start'], cell(t['verify']), cell(t['decode']), ratio, ratio - 1))
            lines.append('')
        if r['step'] == 'e2e':
            q = r['tokens_per_s']
            row = lambda s: '%d | %r | %s' % (s['steps'], s['emitted'], ', '.join('%.2f' % m for m in s['mean_accepted_per_step']))
            lines += ['### (c) End to end: engine_generate_batch, %d prompts x %d tokens + %d new tokens each, k = %d, aggregate tokens/s of the decode part: median (max - min) of %d alternating repeats' % (
                          r['batch'], r['prompt'], r['new'], r['k'], REPEATS), '',
                      '| draft | tokens/s | vs plain greedy | verify steps | tokens from verify steps per sequence | mean accepted drafts per step, per sequence |',
                      '|---|---|---|---|---|---|',
                      '| none (plain greedy engine_generate_batch) | %s | 1.00 | | | |' % cell(q['greedy']),
                      '| oracle (replays a previous run: the ceiling) | %s | %.2f | %s |' % (cell(q['oracle']), _median(q['oracle']) / _median(q['greedy']), row(r['oracle'])),
                      '| adversarial ((greedy + 1) %% vocab: the worst case) | %s | %.2f | %s |' % (
                          cell(q['adversarial']), _median(q['adversarial']) / _median(q['greedy']), row(r['adversarial'])), '']
    lines += ['### Raw repeats', '', '```'] + [json.dumps(r) for r in results] + ['```', '']
    text = '\n'.join(lines)
    print(text)
    if '--markdown' in sys.argv:
        with open(sys.argv[sys.argv.index('--markdown') + 1], 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
