"""Speculative decoding in the engine: what the multi-token verify step costs and what it can buy.

  table 1, the attention call alone, 32 heads, t_max 2048, R rows in {2, 4, 5, 8, 16} at position p in {16, 512, 1024, 2047 - R}:
           gptq_decode_attn_chunk_f16 (csrc/chunk_attn.hip: position on the device, the history streamed once for all rows) against
           gptq_prompt_attn_f16 with the same rows and start = p (the only way to do it before; start is a host value) and against
           gptq_decode_attn_batch_f16 at batch R with every row at position p (R slots: it reads R times the K / V).  Each candidate is captured as
           a graph of INNER calls, so the figures are device time per call without the host's launch cost.
  table 2, step graphs of ONE engine per R in {2, 4, 5, 8} on the 7B-shaped random model: the verify-greedy graph (capture_verify_greedy: R rows
           through every layer, accept rule on the device) against the single-token greedy graph of the same engine and against the step graph of
           DecodeEngine(batch=R), at the same contexts.  c_R = t_verify(R) / t_step(1): speculation pays when the mean number of tokens a step
           emits exceeds c_R.  The drafts are random ids (nothing is accepted: every replay advances the position by one, like the others).
  table 3, end to end: engine_generate(prefill='engine'), 16-token prompt + 256 new tokens, k = 4, tokens/s of plain greedy against two synthetic
           drafts that bound every real one -- an ORACLE that replays a previous run (full acceptance: the ceiling) and an ADVERSARIAL draft,
           (greedy token + 1) % vocab (nothing accepted: the worst-case overhead).  Real acceptance rates depend on real text and a real checkpoint,
           which a random model cannot give: only these bounds are reported.  The default draft (prompt_lookup_draft, host code) runs too, for its
           host cost per step -- its acceptance on a random model (whose greedy output may simply repeat itself) means nothing -- next to the time of one lookup over 2 048 random ids.

Device events around a synchronised window (table 3: wall time around a synchronised call), everything warmed up, REPEATS repeats with the
candidates alternating in one process, medians and max - min spreads (raw repeats printed too).  Every table is a child process under its own
`timeout`; at most 16 CPU threads.
    python tools/bench_speculate.py [--markdown FILE] [--only attn|steps|e2e]"""
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
ATTN_ROWS = (2, 4, 5, 8, 16)
STEP_ROWS = (2, 4, 5, 8)
CONTEXTS = (16, 512, 1024, 2047)
NEW, PROMPT, K = 256, 16, 4
STEP_TIMEOUT = {'attn': 300, 'steps': 900, 'e2e': 600}


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


def step_attn(R):
    import numpy as np
    import torch
    from quant import _native
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lib, dev = _native.lib(), torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(R)
    f16 = dict(dtype=torch.float16, device=dev)
    qkv = torch.randn((R, 3 * H), generator=gen, **f16)
    kc = torch.randn((R, T_MAX, H), generator=gen, **f16) * 0.5           # slot 0: the one sequence; all R slots: the batch candidate
    vc = torch.randn((R, T_MAX, H), generator=gen, **f16)
    out = torch.zeros((R, H), **f16)
    tab = torch.empty((T_MAX, HD // 2, 2), dtype=torch.float32, device=dev)
    assert lib.gptq_rope_table_f32(tab.data_ptr(), T_MAX, HD, 10000.0, _native.stream_ptr(dev)) == 0
    ws_c = torch.zeros(lib.gptq_decode_attn_chunk_workspace_bytes(R, HEADS, HD, T_MAX), dtype=torch.uint8, device=dev)
    ws_p = torch.zeros(lib.gptq_prompt_attn_workspace_bytes(R, HEADS, HD, T_MAX), dtype=torch.uint8, device=dev)
    ws_b = torch.zeros(lib.gptq_decode_attn_batch_workspace_bytes(R, HEADS, HD, T_MAX), dtype=torch.uint8, device=dev)
    scale = float(1.0 / np.sqrt(HD))
    res = []
    for ctx in CONTEXTS:
        p = min(ctx, 2047 - R)
        pos1 = torch.full((1,), p, dtype=torch.int64, device=dev)
        posR = torch.full((R,), p, dtype=torch.int64, device=dev)

        def chunk(s):
            rc = lib.gptq_decode_attn_chunk_f16(qkv.data_ptr(), 3 * H, R, pos1.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), H, ws_c.data_ptr(),
                                                ws_c.numel(), HEADS, HD, T_MAX, 10000.0, scale, tab.data_ptr(), s)
            assert rc == 0, rc

        def prompt(s):
            rc = lib.gptq_prompt_attn_f16(qkv.data_ptr(), 3 * H, R, p, kc.data_ptr(), vc.data_ptr(), out.data_ptr(), H, ws_p.data_ptr(), ws_p.numel(),
                                          HEADS, HD, T_MAX, 10000.0, scale, tab.data_ptr(), s)
            assert rc == 0, rc

        def batch(s):
            rc = lib.gptq_decode_attn_batch_f16(qkv.data_ptr(), 3 * H, posR.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), H, ws_b.data_ptr(),
                                                ws_b.numel(), R, HEADS, HD, T_MAX, 10000.0, scale, tab.data_ptr(), None, s)
            assert rc == 0, rc
        graphs = dict(chunk=_graph_of(chunk, INNER), prompt=_graph_of(prompt, INNER), batch=_graph_of(batch, INNER))
        for g in graphs.values():
            g.replay()
        times = {name: [] for name in graphs}
        for _ in range(REPEATS):                         # alternating
            for name, g in graphs.items():
                times[name].append(_timed(g.replay, INNER))
        res.append(dict(p=p, us=times, splits=lib.gptq_decode_attn_chunk_splits(HEADS, HD, T_MAX, p + R)))
        del graphs
    return dict(step='attn', rows=R, inner=INNER, cases=res)


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
        return (D.build_random_llama('cuda:0', seed=0),)
    finally:
        D.fill_random_quant_ = fill


def step_steps(R, model):
    import torch
    from quant import decode as D
    dev = torch.device('cuda:0')
    eng = D.DecodeEngine(model, t_max=T_MAX, chunk=R)
    wide = D.DecodeEngine(model, t_max=T_MAX, batch=R)
    gen = torch.Generator(device=dev).manual_seed(R)
    for e in (eng, wide):
        e.kcb.normal_(0, 0.5, generator=gen)
        e.vcb.normal_(0, 0.5, generator=gen)
    eng.pos.zero_()
    eng.capture_greedy()
    eng.capture_verify_greedy()
    wide.capture()
    vocab = model.config.vocab_size
    ids1 = torch.randint(1, vocab, (1,), device=dev, generator=gen)
    idsR = torch.randint(1, vocab, (R,), device=dev, generator=gen)
    res = []
    for ctx in CONTEXTS:
        start = min(ctx, T_MAX - R - INNER)              # INNER replays, one position each, the chunk still fits at the last

        def run_verify():
            eng.pos.fill_(start); eng.chunk_ids.copy_(idsR)
            return _timed(lambda: [eng.verify_graph.replay() for _ in range(INNER)], INNER)

        def run_single():
            eng.pos.fill_(start); eng.ids.copy_(ids1)
            return _timed(lambda: [eng.greedy_graph.replay() for _ in range(INNER)], INNER)

        def run_batch():
            wide.pos.fill_(start); wide.ids.copy_(idsR)
            return _timed(lambda: [wide.graph.replay() for _ in range(INNER)], INNER)
        cands = dict(verify=run_verify, single=run_single, batch=run_batch)
        for f in cands.values():
            f()
        eng.pos.fill_(start); eng.chunk_ids.copy_(idsR)
        eng.verify_graph.replay()
        accepted = int(eng.verify_out[0])
        times = {name: [] for name in cands}
        for _ in range(REPEATS):
            for name, f in cands.items():
                times[name].append(f())
        res.append(dict(start=start, us=times, accepted_by_the_random_draft=accepted))
    return dict(step='steps', rows=R, inner=INNER, cases=res)


def step_e2e(_, model):
    import time
    import torch
    from quant import decode as D
    dev = torch.device('cuda:0')
    vocab = model.config.vocab_size
    plain_eng = D.DecodeEngine(model, t_max=T_MAX).capture()
    eng = D.DecodeEngine(model, t_max=T_MAX, chunk=K + 1)
    prompt = torch.randint(1, vocab, (1, PROMPT), device=dev, generator=torch.Generator(device=dev).manual_seed(0))

    def plain(n=NEW):
        return D.engine_generate(model, prompt, n, engine=plain_eng, prefill='engine')

    def spec(draft, n=NEW):
        return D.engine_generate(model, prompt, n, engine=eng, prefill='engine', speculate=dict(k=K, draft=draft))
    greedy = plain()
    # the oracle replays a previous run.  A verify step and a single step round differently, so a near tie can send the speculative run down
    # another (equally greedy) path than the plain one: the oracle is then refined with the speculative run's own output
    known = greedy[0].tolist()
    for _ in range(4):
        oracle = (lambda kn: (lambda toks, k: (kn[len(toks):len(toks) + k] + [0] * k)[:k]))(list(known))
        out = spec(oracle)
        st = eng.spec_stats
        known = out[0].tolist()
        if all(a == K for a in st['accepted'][:-1]):
            break
    oracle_stats = dict(st)
    gl = greedy[0].tolist()
    adversarial = lambda toks, k: [((gl[len(toks) + j] if len(toks) + j < len(gl) else 0) + 1) % vocab for j in range(k)]
    adv_out = spec(adversarial)
    adv_stats = dict(eng.spec_stats)
    agree = dict(oracle=sum(int(a == b) for a, b in zip(out[0].tolist(), gl)) - PROMPT, adversarial=sum(int(a == b) for a, b in zip(adv_out[0].tolist(), gl)) - PROMPT)

    def rate(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn(NEW)
        torch.cuda.synchronize(); tn = time.perf_counter() - t0
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn(1)
        torch.cuda.synchronize(); t1 = time.perf_counter() - t0
        return (NEW - 1) / (tn - t1)                     # decode part only, as benchmark_generate measures model.generate
    spec(None)
    lookup_stats = dict(eng.spec_stats)
    cands = dict(greedy=plain, oracle=lambda n: spec(oracle, n), adversarial=lambda n: spec(adversarial, n), lookup=lambda n: spec(None, n))
    for f in cands.values():
        f(8)
    rates = {name: [] for name in cands}
    for _ in range(REPEATS):
        for name, f in cands.items():
            rates[name].append(rate(f))
    mean = lambda s: s['emitted'] / max(1, s['steps'])
    long_ids = torch.randint(1, vocab, (2048,), generator=torch.Generator().manual_seed(1)).tolist()
    t0 = time.perf_counter()
    for _ in range(100):
        D.prompt_lookup_draft(long_ids, K)
    lookup_us = (time.perf_counter() - t0) / 100 * 1e6
    return dict(step='e2e', prompt=PROMPT, new=NEW, k=K, tokens_per_s=rates,
                oracle=dict(steps=oracle_stats['steps'], emitted=oracle_stats['emitted'], mean_emitted_per_step=mean(oracle_stats)),
                adversarial=dict(steps=adv_stats['steps'], emitted=adv_stats['emitted'], mean_emitted_per_step=mean(adv_stats)),
                lookup=dict(steps=lookup_stats['steps'], emitted=lookup_stats['emitted'], mean_emitted_per_step=mean(lookup_stats)),
                prompt_lookup_draft_us_at_2048_random_ids=lookup_us,
                tokens_equal_to_plain_greedy_of_256=agree)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _spread(v):
    return max(v) - min(v)


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == '--step':
        kind = sys.argv[2]
        setup = model_setup() if kind != 'attn' else ()
        for n in dict(attn=ATTN_ROWS, steps=STEP_ROWS, e2e=(K,))[kind]:
            print('%s %d ...' % (kind, n), flush=True)
            r = dict(attn=step_attn, steps=step_steps, e2e=step_e2e)[kind](n, *setup)
            print('RESULT ' + json.dumps(r), flush=True)
        return 0
    kinds = [sys.argv[sys.argv.index('--only') + 1]] if '--only' in sys.argv else ['attn', 'steps', 'e2e']
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
        lines += ['### The attention call alone: %d heads, t_max %d, us per call: median (max - min) of %d alternating repeats of a graph of %d calls' % (
                      HEADS, T_MAX, REPEATS, INNER), '',
                  '| rows R | position p | splits | gptq_decode_attn_chunk_f16 | gptq_prompt_attn_f16 (start = p) | gptq_decode_attn_batch_f16 (batch R) | prompt / chunk | batch / chunk | not slower than prompt |',
                  '|---|---|---|---|---|---|---|---|---|']
        for r in results:
            if r['step'] == 'attn':
                for c in r['cases']:
                    t = c['us']
                    lines.append('| %d | %d | %d | %s | %s | %s | %.2f | %.2f | %s |' % (
                        r['rows'], c['p'], c['splits'], cell(t['chunk']), cell(t['prompt']), cell(t['batch']), _median(t['prompt']) / _median(t['chunk']),
                        _median(t['batch']) / _median(t['chunk']), verdict(t['chunk'], t['prompt']) if c['p'] >= 512 else '(p < 512: not a criterion) ' + verdict(t['chunk'], t['prompt'])))
        lines.append('')
    if any(r['step'] == 'steps' for r in results):
        lines += ['### Step graphs, 7B-shaped random model (scales x 0.05), us per replay: median (max - min) of %d alternating repeats of %d replays' % (REPEATS, INNER), '',
                  '| rows R | first position | verify-greedy graph (R rows) | single-token greedy graph | DecodeEngine(batch=R) step graph | c_R = verify / single | verify / batch | not slower than batch=R |',
                  '|---|---|---|---|---|---|---|---|']
        for r in results:
            if r['step'] == 'steps':
                for c in r['cases']:
                    t = c['us']
                    lines.append('| %d | %d | %s | %s | %s | %.3f | %.3f | %s |' % (
                        r['rows'], c['start'], cell(t['verify']), cell(t['single']), cell(t['batch']), _median(t['verify']) / _median(t['single']),
                        _median(t['verify']) / _median(t['batch']), verdict(t['verify'], t['batch'])))
        lines.append('')
    for r in results:
        if r['step'] == 'e2e':
            q = r['tokens_per_s']
            lines += ['### End to end: engine_generate(prefill=\'engine\'), %d-token prompt + %d new tokens, k = %d, tokens/s of the decode part: median (max - min) of %d alternating repeats' % (
                          r['prompt'], r['new'], r['k'], REPEATS), '',
                      '| draft | tokens/s | vs plain greedy | verify steps | tokens from verify steps | mean tokens per step |', '|---|---|---|---|---|---|',
                      '| none (plain greedy engine_generate) | %s | 1.00 | | | |' % cell(q['greedy']),
                      '| oracle (replays a previous run: the ceiling) | %s | %.2f | %d | %d | %.2f |' % (
                          cell(q['oracle']), _median(q['oracle']) / _median(q['greedy']), r['oracle']['steps'], r['oracle']['emitted'], r['oracle']['mean_emitted_per_step']),
                      '| adversarial ((greedy + 1) %% vocab: the worst case) | %s | %.2f | %d | %d | %.2f |' % (
                          cell(q['adversarial']), _median(q['adversarial']) / _median(q['greedy']), r['adversarial']['steps'], r['adversarial']['emitted'],
                          r['adversarial']['mean_emitted_per_step']),
                      '| prompt lookup (the default draft; its acceptance on a random model says nothing about real text) | %s | %.2f | %d | %d | %.2f |' % (
                          cell(q['lookup']), _median(q['lookup']) / _median(q['greedy']), r['lookup']['steps'], r['lookup']['emitted'],
                          r['lookup']['mean_emitted_per_step']), '',
                      'One `prompt_lookup_draft(tokens, %d)` over 2 048 random ids (nothing matches: the longest scan): %.0f us of host time.' % (
                          r['k'], r['prompt_lookup_draft_us_at_2048_random_ids']), '']
    lines += ['### Raw repeats', '', '```'] + [json.dumps(r) for r in results] + ['```', '']
    text = '\n'.join(lines)
    print(text)
    if '--markdown' in sys.argv:
        with open(sys.argv[sys.argv.index('--markdown') + 1], 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
