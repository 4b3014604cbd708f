"""The fp8 KV cache (DecodeEngine(kv_cache='fp8'), csrc/decode_attn_kv8.hip) against the fp16 cache: what the narrower cache buys and costs.

  table 1, the op: gptq_decode_attn_batch_kv8_f16 against gptq_decode_attn_batch_f16 (the yardstick), 32 heads of 128, t_max 2048, B in {1, 4,
           16} rows at contexts of 16 / 512 / 2047 tokens.  A call rotates through LAYERS cache allocations the way a decode step walks its
           layers, so that no call finds its rows in a cache level the one before filled.  us per call and achieved bytes/s (K and V rows
           read, exponents included).
  table 2, the engine: us per replay of the capture_greedy_rows graph of the 7B-shaped random model (scales x 0.05), both cache kinds from the
           same positions, 16 steps ending at the context; --parent DIR (a built checkout of the parent commit) measures the fp16 engine
           there as well, in a process of its own that imports that tree: the flag off must be the parent's step.
  table 3, engine_generate_batch at 16 x (16 + 256) tokens, tok/s; accuracy of fp8 against fp16 on the 7B-shaped and the tiny random model
           (max|dlogit| / max|logit| over teacher-forced steps, greedy-token agreement); cache memory of both kinds.

Device events around a synchronised window, everything warmed up, REPEATS repeats with the candidates alternating in one process, medians and
max - min spreads (raw repeats printed too).  Every table is a child process under its own `timeout`; at most 16 CPU threads.
    python tools/bench_kv_fp8.py [--markdown FILE] [--only op|engine|generate] [--parent DIR]"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = sys.argv[sys.argv.index('--root') + 1] if '--root' in sys.argv else HERE       # (the tree a child step imports)
sys.path[:0] = [ROOT, os.path.join(ROOT, 'gptq-for-llama_amd')]
os.environ.setdefault('OMP_NUM_THREADS', '16')
REPEATS = 7
HEADS, HD, T_MAX = 32, 128, 2048
BATCHES, CONTEXTS = (1, 4, 16), (16, 512, 2047)
STEPS = 16
NEW = 256
STEP_TIMEOUT = {'op': 300, 'engine': 700, 'parent': 500, 'generate': 700}


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


def _random_fp8_(q, e):
    """finite e4m3 bytes of magnitude 0.25 .. 1 with random signs, exponents -1"""
    import torch
    q.copy_(torch.randint(0x28, 0x38, q.shape, device=q.device, dtype=torch.uint8) + 0x80 * torch.randint(0, 2, q.shape, device=q.device, dtype=torch.uint8))
    e.fill_(-1)


def step_op(B):
    import torch
    from quant import _native
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lib, dev = _native.lib(), torch.device('cuda:0')
    s = _native.stream_ptr(dev)
    H, scale = HEADS * HD, 1.0 / HD ** 0.5
    layers = 4 if B == 16 else 8                          # fp16 at B = 16, 2047 tokens: 4 x 537 MB walked per round
    g = torch.Generator(device=dev).manual_seed(B)
    qkv = (torch.randn((B, 3 * H), device=dev, generator=g) * 0.5).half()
    out = torch.zeros((B, H), dtype=torch.float16, device=dev)
    ws = torch.zeros(lib.gptq_decode_attn_batch_workspace_bytes(B, HEADS, HD, T_MAX), dtype=torch.uint8, device=dev)
    kc, vc = (torch.empty((layers, B, T_MAX, H), dtype=torch.float16, device=dev).normal_(0, 0.5) for _ in range(2))
    k8, v8 = (torch.empty((layers, B, T_MAX, H), dtype=torch.uint8, device=dev) for _ in range(2))
    ke, ve = (torch.empty((layers, B, T_MAX, HEADS), dtype=torch.int8, device=dev) for _ in range(2))
    _random_fp8_(k8, ke)
    _random_fp8_(v8, ve)
    pos = torch.zeros(B, dtype=torch.int64, device=dev)
    turn = [0]

    def fp16():
        li = turn[0] = (turn[0] + 1) % layers
        rc = lib.gptq_decode_attn_batch_f16(qkv.data_ptr(), 3 * H, pos.data_ptr(), kc[li].data_ptr(), vc[li].data_ptr(), out.data_ptr(), H, ws.data_ptr(),
                                            ws.numel(), B, HEADS, HD, T_MAX, 10000.0, scale, None, None, s)
        assert rc == 0, rc

    def fp8():
        li = turn[0] = (turn[0] + 1) % layers
        rc = lib.gptq_decode_attn_batch_kv8_f16(qkv.data_ptr(), 3 * H, pos.data_ptr(), k8[li].data_ptr(), v8[li].data_ptr(), ke[li].data_ptr(),
                                                ve[li].data_ptr(), out.data_ptr(), H, ws.data_ptr(), ws.numel(), B, HEADS, HD, T_MAX, 10000.0, scale,
                                                None, None, 0, s)
        assert rc == 0, rc
    cands = {'fp16': fp16, 'fp8': fp8}
    res = []
    for ctx in CONTEXTS:
        pos.fill_(ctx - 1)                                # the call attends to ctx rows: ctx - 1 of the cache and the new token
        for f in cands.values():
            for _ in range(2 * layers):
                f()
        times = {name: [] for name in cands}
        for _ in range(REPEATS):                          # alternating
            for name, f in cands.items():
                times[name].append(_timed(f, 25 * layers))
        res.append(dict(step='op', B=B, context=ctx, inner=25 * layers, layers=layers, us=times,
                        bytes=dict(fp16=B * (ctx - 1) * H * 2 * 2, fp8=B * (ctx - 1) * (H + HEADS) * 2)))
    return res


def engine_setup(tiny=False):
    import torch
    from quant import decode as D
    torch.set_num_threads(min(16, torch.get_num_threads()))
    fill = D.fill_random_quant_

    def small(layer, gen):                               # bench.py's sampling leg: finite logits
        fill(layer, gen)
        layer.scales.mul_(0.05)
    D.fill_random_quant_ = small
    try:
        if tiny:
            return D.build_random_llama('cuda:0', seed=3, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                                        num_key_value_heads=2, vocab_size=512, max_position_embeddings=512)
        return D.build_random_llama('cuda:0', seed=0)
    finally:
        D.fill_random_quant_ = fill


def step_engine(model, kinds):
    """kinds ('fp16',): the fp16 engine alone, through nothing this commit added (what a checkout of the parent can run)"""
    import torch
    from quant import decode as D
    dev = torch.device('cuda:0')
    res = []
    for B in BATCHES:
        engines = {}
        for kind in kinds:
            eng = D.DecodeEngine(model, t_max=T_MAX, batch=B, **({} if kind == 'fp16' else dict(kv_cache=kind)))
            eng.capture_greedy_rows()
            if kind == 'fp16':
                eng.kcb.normal_(0, 0.5)
                eng.vcb.normal_(0, 0.5)
            else:
                _random_fp8_(eng.k8b, eng.kexpb)
                _random_fp8_(eng.v8b, eng.vexpb)
            engines[kind] = eng
        ids = torch.randint(1, model.config.vocab_size, (B,), device=dev, generator=torch.Generator(device=dev).manual_seed(B))

        def timed(kind, ctx):
            eng = engines[kind]
            eng.pos.fill_(ctx - STEPS)
            eng.ids.copy_(ids)
            eng.stepc.zero_()
            return _timed(eng.greedy_rows_graph.replay, STEPS)
        for ctx in CONTEXTS:
            for kind in kinds:
                timed(kind, ctx)
            times = {kind: [] for kind in kinds}
            for _ in range(REPEATS):
                for kind in kinds:
                    times[kind].append(timed(kind, ctx))
            res.append(dict(step='engine' if len(kinds) > 1 else 'parent', B=B, context=ctx, steps=STEPS, us_per_replay=times))
        del engines, eng
        torch.cuda.empty_cache()
    return res


def step_generate(model):
    import time
    import torch
    from quant import decode as D
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(1)
    vocab = model.config.vocab_size
    prompts = [torch.randint(1, vocab, (16,), device=dev, generator=gen) for _ in range(16)]
    kinds = ('fp16', 'fp8')
    engines = {k: D.DecodeEngine(model, t_max=T_MAX, batch=16, kv_cache=k) for k in kinds}
    cache = {}
    for k, e in engines.items():
        names = ('kcb', 'vcb') if k == 'fp16' else ('k8b', 'v8b', 'kexpb', 'vexpb', 'kst', 'vst')
        cache[k] = sum(getattr(e, n).numel() * getattr(e, n).element_size() for n in names)

    def generate(k, n):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = D.engine_generate_batch(model, prompts, n, engine=engines[k], kv_cache=k)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    for k in kinds:
        generate(k, 4)
    rates = {k: [] for k in kinds}
    for _ in range(5):
        for k in kinds:
            rates[k].append(16 * NEW / (generate(k, NEW + 1)[0] - generate(k, 1)[0]))
    res = [dict(step='generate', new=NEW, tokens_per_s=rates, cache_bytes=cache, t_max=T_MAX, batch=16)]
    del engines
    torch.cuda.empty_cache()
    # accuracy: teacher-forced tokens (the fp16 engine's greedy ones) through both engines, 3 prompts of 16 tokens + 64 steps
    for name, m in (('7B-shaped', model), ('tiny', engine_setup(tiny=True))):
        v = m.config.vocab_size
        ps = [torch.randint(3, v, (16,), device=dev, generator=gen) for _ in range(3)]
        t_max = 128
        e16, e8 = D.DecodeEngine(m, t_max=t_max, batch=3), D.DecodeEngine(m, t_max=t_max, batch=3, kv_cache='fp8')
        with torch.no_grad():
            l16, l8 = e16.prefill_batch(ps).float().clone(), e8.prefill_batch(ps).float().clone()
            worst, scale, agree, n = 0.0, 0.0, 0, 0
            for _ in range(64):
                worst, scale = max(worst, float((l8 - l16).abs().max())), max(scale, float(l16.abs().max()))
                tok = l16.argmax(dim=-1)
                agree += int((l8.argmax(dim=-1) == tok).sum())
                n += 3
                l16, l8 = e16.decode(tok).float().clone(), e8.decode(tok).float().clone()
        res.append(dict(step='accuracy', model=name, steps=64, rows=3, max_dlogit_over_max_logit=worst / scale, greedy_agreement=agree / n))
    return res


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _spread(v):
    return max(v) - min(v)


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == '--step':
        kind = sys.argv[2]
        if kind == 'op':
            for B in BATCHES:
                print('op B %d ...' % B, flush=True)
                for r in step_op(B):
                    print('RESULT ' + json.dumps(r), flush=True)
        else:
            print('%s ...' % kind, flush=True)
            model = engine_setup()
            rows = step_generate(model) if kind == 'generate' else step_engine(model, ('fp16', 'fp8') if kind == 'engine' else ('fp16',))
            for r in rows:
                print('RESULT ' + json.dumps(r), flush=True)
        return 0
    kinds = [sys.argv[sys.argv.index('--only') + 1]] if '--only' in sys.argv else ['op', 'engine', 'generate']
    parent = os.path.abspath(sys.argv[sys.argv.index('--parent') + 1]) if '--parent' in sys.argv else None
    if parent is not None and 'engine' in kinds:
        kinds.insert(kinds.index('engine') + 1, 'parent')
    results = []
    for kind in kinds:
        cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT[kind]), sys.executable, os.path.abspath(__file__), '--step', kind]
        if kind == 'parent':
            cmd += ['--root', parent]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
        for line in p.stdout:                            # streamed: a long step still shows progress
            print(line.rstrip(), flush=True)
            if line.startswith('RESULT '):
                results.append(json.loads(line[7:]))
        if p.wait() != 0:                                # a fault, an abort or a time limit: nothing more is started on the GPU
            print('step %s ended with status %d: stopping' % (kind, p.returncode))
            return 1
    cell = lambda v: '%.1f (%.1f)' % (_median(v), _spread(v))
    lines = []
    ops = [r for r in results if r['step'] == 'op']
    if ops:
        lines += ['### The attention call: %d heads of %d, t_max %d, us: median (max - min) of %d alternating repeats, device events; TB/s = K / V '
                  'bytes of the context over the median' % (HEADS, HD, T_MAX, REPEATS), '',
                  '| B | context | fp16 us | fp8 us | fp8 / fp16 | fp16 TB/s | fp8 TB/s |', '|---|---|---|---|---|---|---|']
        for r in ops:
            u, b = r['us'], r['bytes']
            lines.append('| %d | %d | %s | %s | %.3f | %.2f | %.2f |' % (r['B'], r['context'], cell(u['fp16']), cell(u['fp8']),
                                                                     _median(u['fp8']) / _median(u['fp16']), b['fp16'] / _median(u['fp16']) / 1e6,
                                                                     b['fp8'] / _median(u['fp8']) / 1e6))
    eng = [r for r in results if r['step'] == 'engine']
    par = {(r['B'], r['context']): r for r in results if r['step'] == 'parent'}
    if eng:
        lines += ['', '### The engine step: 7B-shaped random model, capture_greedy_rows, us / replay over %d steps ending at the context: median (max - '
                  'min) of %d alternating repeats' % (STEPS, REPEATS), '',
                  '| B | context | fp16 | fp8 | fp8 / fp16 | fp16 on the parent commit |', '|---|---|---|---|---|---|']
        for r in eng:
            t = r['us_per_replay']
            p = par.get((r['B'], r['context']))
            lines.append('| %d | %d | %s | %s | %.3f | %s |' % (r['B'], r['context'], cell(t['fp16']), cell(t['fp8']), _median(t['fp8']) / _median(t['fp16']),
                                                              cell(p['us_per_replay']['fp16']) if p else 'not measured'))
    for r in results:
        if r['step'] == 'generate':
            q, c = r['tokens_per_s'], r['cache_bytes']
            lines += ['', '### engine_generate_batch, 16 x (16 + %d) tokens, tok/s: median (max - min) of 5 alternating repeats; cache memory at batch %d, '
                      't_max %d' % (r['new'], r['batch'], r['t_max']), '', '| | fp16 | fp8 | fp8 / fp16 |', '|---|---|---|---|',
                      '| tok/s | %s | %s | %.3f |' % (cell(q['fp16']), cell(q['fp8']), _median(q['fp8']) / _median(q['fp16'])),
                      '| cache, MiB (fp8: bytes + exponents + one layer of fp16 staging) | %.0f | %.0f | %.3f |' % (
                          c['fp16'] / 2 ** 20, c['fp8'] / 2 ** 20, c['fp8'] / c['fp16'])]
    acc = [r for r in results if r['step'] == 'accuracy']
    if acc:
        lines += ['', '### fp8 against fp16 on the same teacher-forced tokens (3 rows, 16-token prompts + 64 steps)', '',
                  '| model | max abs dlogit / max abs logit | greedy-token agreement |', '|---|---|---|']
        lines += ['| %s | %.4f | %.3f |' % (r['model'], r['max_dlogit_over_max_logit'], r['greedy_agreement']) for r in acc]
    lines += ['', '### Raw repeats', '', '```'] + [json.dumps(r) for r in results] + ['```', '']
    text = '\n'.join(lines)
    print(text)
    if '--markdown' in sys.argv:
        with open(sys.argv[sys.argv.index('--markdown') + 1], 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
