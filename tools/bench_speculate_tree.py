"""Tree speculative decoding: what the tree entries cost next to the chain's (method and helpers of tools/bench_speculate.py: device events around
a synchronised window, graphs of INNER calls, REPEATS alternating repeats, medians and max - min spreads; every table a child process under its own
`timeout`).

  attn     gptq_decode_attn_tree_f16 at the CHAIN mask against gptq_decode_attn_chunk_f16 (whose kernels are the parent commit's instructions),
           32 heads, R = 5 / 16 at p = 16 / 512 / 2030, the chunk entry captured TWICE so that its own run-to-run spread stands next to the difference.
  steps    7B-shaped random model: the verify-tree-greedy graph at R = 8 / 16 (a star of random ids: nothing is accepted, a replay advances one
           position) against the verify-greedy graph at R = 5 and the single-token greedy graph: c = t_tree(R) / t_token.
  compact  gptq_kv_tree_compact_f16 alone on the 7B cache (32 layers x 4096): a = 0, a = 4 and a = 7 with every row moving, a = 15 (a chain).
  e2e      engine_generate, 16 + 256 tokens: plain greedy, the chain oracle (k = 4), a tree with a wrong first branch of 3 and the truth as its
           second (k = 7), an adversarial star (k = 7), and prompt_lookup_tree_draft -- whose acceptance on a random model says nothing.
    python tools/bench_speculate_tree.py [--markdown FILE] [--only attn|steps|compact|e2e]"""
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_speculate import HD, HEADS, H, INNER, REPEATS, T_MAX, _graph_of, _median, _spread, _timed, model_setup   # noqa: E402

NEW, PROMPT = 256, 16
STEP_TIMEOUT = dict(attn=240, steps=600, compact=240, e2e=600)


def step_attn():
    import numpy as np
    import torch
    from quant import _native
    lib, dev = _native.lib(), torch.device('cuda:0')
    res = []
    for R in (5, 16):
        gen = torch.Generator(device=dev).manual_seed(R)
        f16 = dict(dtype=torch.float16, device=dev)
        qkv, out = torch.randn((R, 3 * H), generator=gen, **f16), torch.zeros((R, H), **f16)
        kc, vc = torch.randn((T_MAX, H), generator=gen, **f16) * 0.5, torch.randn((T_MAX, H), generator=gen, **f16)
        ws = torch.zeros(lib.gptq_decode_attn_chunk_workspace_bytes(R, HEADS, HD, T_MAX), dtype=torch.uint8, device=dev)
        anc = torch.tensor([(2 << r) - 1 for r in range(16)], dtype=torch.int32, device=dev)
        scale = float(1.0 / np.sqrt(HD))
        for p in (16, 512, 2030):
            pos = torch.full((1,), p, dtype=torch.int64, device=dev)
            tail = (kc.data_ptr(), vc.data_ptr(), out.data_ptr(), H, ws.data_ptr(), ws.numel(), HEADS, HD, T_MAX, 10000.0, scale, None)

            def chunk(s):
                assert lib.gptq_decode_attn_chunk_f16(qkv.data_ptr(), 3 * H, R, pos.data_ptr(), *tail, s) == 0

            def tree(s):
                assert lib.gptq_decode_attn_tree_f16(qkv.data_ptr(), 3 * H, R, pos.data_ptr(), anc.data_ptr(), *tail, s) == 0
            graphs = dict(chunk=_graph_of(chunk, INNER), chunk_again=_graph_of(chunk, INNER), tree=_graph_of(tree, INNER))
            times = {name: [] for name in graphs}
            for _ in range(REPEATS + 1):
                for name, g in graphs.items():
                    times[name].append(_timed(g.replay, INNER))
            res.append(dict(rows=R, p=p, us={k: v[1:] for k, v in times.items()}))
    return dict(step='attn', cases=res)


def step_steps():
    import torch
    from quant import decode as D
    model, dev = model_setup()[0], torch.device('cuda:0')
    vocab, res = model.config.vocab_size, []
    engines = [('chain R = 5', D.DecodeEngine(model, t_max=T_MAX, chunk=5))] + [
        ('tree R = %d' % R, D.DecodeEngine(model, t_max=T_MAX, chunk=R, tree=True)) for R in (8, 16)]
    gen = torch.Generator(device=dev).manual_seed(0)
    for _, e in engines:
        e.kcb.normal_(0, 0.5, generator=gen)
        e.vcb.normal_(0, 0.5, generator=gen)
        e.pos.zero_()
        (e.capture_verify_tree_greedy if e.tree else e.capture_verify_greedy)()
    single = engines[0][1].capture_greedy()
    for start in (16, 512, T_MAX - 16 - INNER):
        def run(e, graph, ids):
            e.pos.fill_(start)
            ids.copy_(torch.randint(1, vocab, ids.shape, device=dev, generator=gen))
            return _timed(lambda: [graph.replay() for _ in range(INNER)], INNER)
        cands = {name: (lambda e=e: run(e, e.tree_graph if e.tree else e.verify_graph, e.chunk_ids)) for name, e in engines}
        cands['token step'] = lambda: run(single, single.greedy_graph, single.ids)
        times = {name: [] for name in cands}
        for _ in range(REPEATS + 1):
            for name, f in cands.items():
                times[name].append(f())
        res.append(dict(start=start, us={k: v[1:] for k, v in times.items()}))
    return dict(step='steps', cases=res)


def step_compact():
    import torch
    from quant import _native
    lib, dev, layers, p = _native.lib(), torch.device('cuda:0'), 32, 1000
    kc, vc = (torch.zeros((layers, T_MAX, H), dtype=torch.float16, device=dev) for _ in range(2))
    us = {}
    for name, path in (('a = 0', [0]), ('a = 4, 4 rows move', [0, 2, 4, 6, 8]), ('a = 7, 7 rows move', list(range(0, 16, 2))), ('a = 15, a chain', list(range(16)))):
        a = len(path) - 1
        pos, acc = torch.tensor([p + a + 1], device=dev), torch.tensor([a], device=dev)
        pd = torch.tensor(path + [-1] * (16 - len(path)), dtype=torch.int32, device=dev)

        def call(s):
            assert lib.gptq_kv_tree_compact_f16(kc.data_ptr(), vc.data_ptr(), layers, T_MAX, H, T_MAX * H, pos.data_ptr(), acc.data_ptr(), pd.data_ptr(), s) == 0
        g = _graph_of(call, INNER)
        us[name] = [_timed(g.replay, INNER) for _ in range(REPEATS + 1)][1:]
    return dict(step='compact', us=us)


def step_e2e():
    import time
    import torch
    from quant import decode as D
    model, dev = model_setup()[0], torch.device('cuda:0')
    vocab = model.config.vocab_size
    plain_eng = D.DecodeEngine(model, t_max=T_MAX).capture()
    chain_eng, tree_eng = D.DecodeEngine(model, t_max=T_MAX, chunk=5), D.DecodeEngine(model, t_max=T_MAX, chunk=8, tree=True)
    prompt = torch.randint(1, vocab, (1, PROMPT), device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    known = D.engine_generate(model, prompt, NEW, engine=plain_eng, prefill='engine')[0].tolist()
    nxt = lambda toks, n: (known[len(toks):len(toks) + n] + [0] * n)[:n]
    second = lambda toks, k: ([(nxt(toks, 1)[0] + 1) % vocab, 1, 2] + nxt(toks, k - 3), [0, 1, 2, 0] + list(range(4, k)))
    star = lambda toks, k: ([(nxt(toks, 1)[0] + 1 + j) % vocab for j in range(k)], [0] * k)
    runs = {'plain greedy': lambda n: D.engine_generate(model, prompt, n, engine=plain_eng, prefill='engine'),
            'chain oracle, k = 4': lambda n: D.engine_generate(model, prompt, n, engine=chain_eng, prefill='engine', speculate=dict(k=4, draft=nxt))}
    for name, draft in (('tree, truth on the second branch, k = 7', second), ('tree, adversarial star, k = 7', star), ('tree, prompt lookup, k = 7', None)):
        runs[name] = lambda n, d=draft: D.engine_generate(model, prompt, n, engine=tree_eng, prefill='engine', speculate=dict(k=7, tree=dict(width=3), draft=d))

    def rate(fn):                                            # the decode part only, as tools/bench_speculate.py
        t = []
        for n in (NEW, 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn(n)
            torch.cuda.synchronize(); t.append(time.perf_counter() - t0)
        return (NEW - 1) / (t[0] - t[1])
    stats, rates = {}, {name: [] for name in runs}
    for name, f in runs.items():
        f(NEW)
        e = chain_eng if 'chain' in name else tree_eng
        stats[name] = None if 'plain' in name else dict(steps=e.spec_stats['steps'], emitted=e.spec_stats['emitted'])
    for _ in range(REPEATS):
        for name, f in runs.items():
            rates[name].append(rate(f))
    return dict(step='e2e', tokens_per_s=rates, stats=stats)


def main():
    steps = dict(attn=step_attn, steps=step_steps, compact=step_compact, e2e=step_e2e)
    if len(sys.argv) >= 3 and sys.argv[1] == '--step':
        print('RESULT ' + json.dumps(steps[sys.argv[2]]()), flush=True)
        return 0
    results = []
    for kind in ([sys.argv[sys.argv.index('--only') + 1]] if '--only' in sys.argv else list(steps)):
        p = subprocess.run(['timeout', '-k', '10', str(STEP_TIMEOUT[kind]), sys.executable, os.path.abspath(__file__), '--step', kind],
                           stdout=subprocess.PIPE, text=True)
        results += [json.loads(line[7:]) for line in p.stdout.splitlines() if line.startswith('RESULT ')]
        if p.returncode != 0:                                # a fault, an abort or a time limit: nothing more is started on the GPU
            print('step %s ended with status %d: stopping' % (kind, p.returncode))
            return 1
    cell = lambda v: '%.1f (%.1f)' % (_median(v), _spread(v))
    lines = []
    for r in results:
        if r['step'] == 'attn':
            lines += ['### The tree entry at a chain mask against the chunk entry, %d heads, us per call: median (max - min) of %d repeats' % (HEADS, REPEATS), '',
                      '| rows | p | chunk | chunk, a second graph | tree, chain mask | tree - chunk | within the chunk entry\'s spread |', '|---|---|---|---|---|---|---|']
            for c in r['cases']:
                t = c['us']
                d = _median(t['tree']) - _median(t['chunk'])
                bar = max(_spread(t['chunk']), _spread(t['chunk_again']), abs(_median(t['chunk']) - _median(t['chunk_again'])))
                lines.append('| %d | %d | %s | %s | %s | %+.2f | %s |' % (c['rows'], c['p'], cell(t['chunk']), cell(t['chunk_again']), cell(t['tree']), d,
                                                                         'yes' if d <= bar else 'NO (spread %.2f)' % bar))
        if r['step'] == 'steps':
            names = list(r['cases'][0]['us'])
            lines += ['', '### Verify graphs, 7B-shaped random model, us per replay: median (max - min); c = graph / token step', '',
                      '| first position | ' + ' | '.join(names) + ' | ' + ' | '.join('c, ' + n for n in names[:-1]) + ' |', '|---' * (2 * len(names)) + '|']
            for c in r['cases']:
                t = c['us']
                lines.append('| %d | ' % c['start'] + ' | '.join(cell(t[n]) for n in names) + ' | ' +
                             ' | '.join('%.2f' % (_median(t[n]) / _median(t['token step'])) for n in names[:-1]) + ' |')
        if r['step'] == 'compact':
            lines += ['', '### gptq_kv_tree_compact_f16 alone, 32 layers x 4096, us per launch: median (max - min)', '', '| accept | us |', '|---|---|']
            lines += ['| %s | %s |' % (k, cell(v)) for k, v in r['us'].items()]
        if r['step'] == 'e2e':
            q = r['tokens_per_s']
            lines += ['', '### engine_generate, %d + %d tokens, tokens/s of the decode part: median (max - min)' % (PROMPT, NEW), '',
                      '| run | tokens/s | vs plain greedy | verify steps | tokens from them |', '|---|---|---|---|---|']
            for k, v in q.items():
                s = r['stats'][k] or dict(steps=0, emitted=0)
                lines.append('| %s | %s | %.2f | %d | %d |' % (k, cell(v), _median(v) / _median(q['plain greedy']), s['steps'], s['emitted']))
    lines += ['', '### Raw repeats', '', '```'] + [json.dumps(r) for r in results] + ['```', '']
    text = '\n'.join(lines)
    print(text)
    if '--markdown' in sys.argv:
        with open(sys.argv[sys.argv.index('--markdown') + 1], 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
