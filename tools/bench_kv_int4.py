"""The int4 KV cache (DecodeEngine(kv_cache='int4'), csrc/decode_attn_kv4.hip) against the fp16 and the fp8 cache.

  table 1, the op: gptq_decode_attn_batch_kv4_f16 against gptq_decode_attn_batch_f16 (the yardstick) and gptq_decode_attn_batch_kv8_f16 on the
           same positions, 32 heads of 128, t_max 2048, B in {1, 4, 16} rows at contexts of 16 / 512 / 2047 tokens.  A call rotates through
           LAYERS cache allocations the way a decode step walks its layers.  us per call and achieved bytes/s (K and V rows read, metadata
           included).  The yardstick is timed TWICE per repeat (fp16, fp16'): the distance between its two medians is what a ratio can mean.
  table 2, the engine: us per replay of the capture_greedy_rows graph of the 7B-shaped random model (scales x 0.05), the three cache kinds from
           the same positions, 16 steps ending at the context.
  table 3, cache memory allocated at batch 16, t_max 2048 (staging included), and int4 against fp16 on the same teacher-forced tokens.

The method and the helpers are tools/bench_kv_fp8.py's: device events around a synchronised window, everything warmed up, REPEATS repeats with
the candidates alternating in one process, medians and max - min spreads (raw repeats printed too).  Every table is a child process under its
own `timeout`; at most 16 CPU threads.
    python tools/bench_kv_int4.py [--markdown FILE] [--only op|engine|memory]"""
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_kv_fp8 as F            # noqa: E402  (also puts the package on sys.path)

REPEATS, HEADS, HD, T_MAX, BATCHES, CONTEXTS, STEPS = F.REPEATS, F.HEADS, F.HD, F.T_MAX, F.BATCHES, F.CONTEXTS, F.STEPS
STEP_TIMEOUT = {'op': 300, 'engine': 800, 'memory': 500}
KINDS = ('fp16', 'fp8', 'int4')


def _random_int4_(q, m):
    """random codes, d = 1 / 16, m = -0.5: values in [-0.5, 0.44]"""
    import torch
    q.copy_(torch.randint(0, 256, q.shape, device=q.device, dtype=torch.uint8))
    m[..., 0], m[..., 1] = 1.0 / 16, -0.5


def step_op(B):
    import torch
    from quant import _native
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lib, dev = _native.lib(), torch.device('cuda:0')
    s = _native.stream_ptr(dev)
    H, scale = HEADS * HD, 1.0 / HD ** 0.5
    layers = 4 if B == 16 else 8
    g = torch.Generator(device=dev).manual_seed(B)
    qkv = (torch.randn((B, 3 * H), device=dev, generator=g) * 0.5).half()
    out = torch.zeros((B, H), dtype=torch.float16, device=dev)
    ws = torch.zeros(lib.gptq_decode_attn_batch_workspace_bytes(B, HEADS, HD, T_MAX), dtype=torch.uint8, device=dev)
    kc, vc = (torch.empty((layers, B, T_MAX, H), dtype=torch.float16, device=dev).normal_(0, 0.5) for _ in range(2))
    k8, v8 = (torch.empty((layers, B, T_MAX, H), dtype=torch.uint8, device=dev) for _ in range(2))
    ke, ve = (torch.empty((layers, B, T_MAX, HEADS), dtype=torch.int8, device=dev) for _ in range(2))
    k4, v4 = (torch.empty((layers, B, T_MAX, H // 2), dtype=torch.uint8, device=dev) for _ in range(2))
    km, vm = (torch.empty((layers, B, T_MAX, HEADS, 4, 2), dtype=torch.float16, device=dev) for _ in range(2))
    F._random_fp8_(k8, ke)
    F._random_fp8_(v8, ve)
    _random_int4_(k4, km)
    _random_int4_(v4, vm)
    pos = torch.zeros(B, dtype=torch.int64, device=dev)
    turn = [0]

    def fp16():
        li = turn[0] = (turn[0] + 1) % layers
        rc = lib.gptq_decode_attn_batch_f16(qkv.data_ptr(), 3 * H, pos.data_ptr(), kc[li].data_ptr(), vc[li].data_ptr(), out.data_ptr(), H, ws.data_ptr(),
                                            ws.numel(), B, HEADS, HD, T_MAX, 10000.0, scale, None, None, s)
        assert rc == 0, rc

    def quant(entry, k, v, ka, va):
        def call():
            li = turn[0] = (turn[0] + 1) % layers
            rc = entry(qkv.data_ptr(), 3 * H, pos.data_ptr(), k[li].data_ptr(), v[li].data_ptr(), ka[li].data_ptr(), va[li].data_ptr(), out.data_ptr(), H,
                       ws.data_ptr(), ws.numel(), B, HEADS, HD, T_MAX, 10000.0, scale, None, None, 0, s)
            assert rc == 0, rc
        return call
    cands = {'fp16': fp16, 'fp8': quant(lib.gptq_decode_attn_batch_kv8_f16, k8, v8, ke, ve),
             'int4': quant(lib.gptq_decode_attn_batch_kv4_f16, k4, v4, km, vm), "fp16'": fp16}
    res = []
    for ctx in CONTEXTS:
        pos.fill_(ctx - 1)                                # the call attends to ctx rows: ctx - 1 of the cache and the new token
        for f in cands.values():
            for _ in range(2 * layers):
                f()
        times = {name: [] for name in cands}
        for _ in range(REPEATS):                          # alternating
            for name, f in cands.items():
                times[name].append(F._timed(f, 25 * layers))
        n = B * (ctx - 1) * HEADS * 2
        res.append(dict(step='op', B=B, context=ctx, inner=25 * layers, layers=layers, us=times, bytes=dict(fp16=n * 256, fp8=n * 129, int4=n * 80)))
    return res


def _randomise(eng, kind):
    if kind == 'fp16':
        eng.kcb.normal_(0, 0.5)
        eng.vcb.normal_(0, 0.5)
    elif kind == 'fp8':
        F._random_fp8_(eng.k8b, eng.kexpb)
        F._random_fp8_(eng.v8b, eng.vexpb)
    else:
        _random_int4_(eng.k4b, eng.kmetab)
        _random_int4_(eng.v4b, eng.vmetab)


def step_engine(model):
    import torch
    from quant import decode as D
    dev = torch.device('cuda:0')
    res = []
    for B in BATCHES:
        engines = {}
        for kind in KINDS:
            eng = engines[kind] = D.DecodeEngine(model, t_max=T_MAX, batch=B, kv_cache=kind)
            eng.capture_greedy_rows()
            _randomise(eng, kind)
        ids = torch.randint(1, model.config.vocab_size, (B,), device=dev, generator=torch.Generator(device=dev).manual_seed(B))

        def timed(kind, ctx):
            eng = engines[kind]
            eng.pos.fill_(ctx - STEPS)
            eng.ids.copy_(ids)
            eng.stepc.zero_()
            return F._timed(eng.greedy_rows_graph.replay, STEPS)
        for ctx in CONTEXTS:
            for kind in KINDS:
                timed(kind, ctx)
            times = {kind: [] for kind in KINDS}
            for _ in range(REPEATS):
                for kind in KINDS:
                    times[kind].append(timed(kind, ctx))
            res.append(dict(step='engine', B=B, context=ctx, steps=STEPS, us_per_replay=times))
        del engines, eng
        torch.cuda.empty_cache()
    return res


def step_memory(model):
    import torch
    from quant import decode as D
    dev = torch.device('cuda:0')
    cache = {}
    for kind in KINDS:
        base = torch.cuda.memory_allocated()
        eng = D.DecodeEngine(model, t_max=T_MAX, batch=16, kv_cache=kind)
        names = ('kcb', 'vcb') if kind == 'fp16' else tuple(n for g in D.KV_QUANT[kind]['arrays'] for n in g[0]) + ('kst', 'vst')
        cache[kind] = dict(arrays=sum(getattr(eng, n).numel() * getattr(eng, n).element_size() for n in names),
                           engine=torch.cuda.memory_allocated() - base)
        del eng
        torch.cuda.empty_cache()
    res = [dict(step='memory', batch=16, t_max=T_MAX, bytes=cache)]
    gen = torch.Generator(device=dev).manual_seed(1)
    for name, m in (('7B-shaped', model), ('tiny', F.engine_setup(tiny=True))):      # teacher-forced: the fp16 engine's greedy tokens
        ps = [torch.randint(3, m.config.vocab_size, (16,), device=dev, generator=gen) for _ in range(3)]
        e16, e4 = D.DecodeEngine(m, t_max=128, batch=3), D.DecodeEngine(m, t_max=128, batch=3, kv_cache='int4')
        with torch.no_grad():
            l16, l4 = e16.prefill_batch(ps).float().clone(), e4.prefill_batch(ps).float().clone()
            worst, scale, agree, n = 0.0, 0.0, 0, 0
            for _ in range(64):
                worst, scale = max(worst, float((l4 - l16).abs().max())), max(scale, float(l16.abs().max()))
                tok = l16.argmax(dim=-1)
                agree += int((l4.argmax(dim=-1) == tok).sum())
                n += 3
                l16, l4 = e16.decode(tok).float().clone(), e4.decode(tok).float().clone()
        res.append(dict(step='accuracy', model=name, steps=64, rows=3, max_dlogit_over_max_logit=worst / scale, greedy_agreement=agree / n))
    return res


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == '--step':
        kind = sys.argv[2]
        print('%s ...' % kind, flush=True)
        if kind == 'op':
            rows = [r for B in BATCHES for r in step_op(B)]
        else:
            rows = (step_engine if kind == 'engine' else step_memory)(F.engine_setup())
        for r in rows:
            print('RESULT ' + json.dumps(r), flush=True)
        return 0
    kinds = [sys.argv[sys.argv.index('--only') + 1]] if '--only' in sys.argv else ['op', 'engine', 'memory']
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
    med = F._median
    cell = lambda v: '%.1f (%.1f)' % (med(v), F._spread(v))
    lines = []
    ops = [r for r in results if r['step'] == 'op']
    if ops:
        lines += ['### The attention call: %d heads of %d, t_max %d, us: median (max - min) of %d alternating repeats, device events; TB/s = K / V '
                  "bytes of the context over the median; fp16' = the yardstick timed a second time in the same rotation" % (HEADS, HD, T_MAX, REPEATS),
                  '', "| B | context | fp16 us | fp16' us | fp8 us | int4 us | int4 / fp16 | int4 / fp8 | fp16 TB/s | fp8 TB/s | int4 TB/s |",
                  '|---|---|---|---|---|---|---|---|---|---|---|']
        for r in ops:
            u, b = r['us'], r['bytes']
            lines.append('| %d | %d | %s | %s | %s | %s | %.3f | %.3f | %.2f | %.2f | %.2f |' % (
                r['B'], r['context'], cell(u['fp16']), cell(u["fp16'"]), cell(u['fp8']), cell(u['int4']), med(u['int4']) / med(u['fp16']),
                med(u['int4']) / med(u['fp8']), *[b[k] / med(u[k]) / 1e6 for k in KINDS]))
    eng = [r for r in results if r['step'] == 'engine']
    if eng:
        lines += ['', '### The engine step: 7B-shaped random model, capture_greedy_rows, us / replay over %d steps ending at the context: median (max - '
                  'min) of %d alternating repeats' % (STEPS, REPEATS), '',
                  '| B | context | fp16 | fp8 | int4 | int4 / fp16 | int4 / fp8 |', '|---|---|---|---|---|---|---|']
        for r in eng:
            t = r['us_per_replay']
            lines.append('| %d | %d | %s | %s | %s | %.3f | %.3f |' % (r['B'], r['context'], cell(t['fp16']), cell(t['fp8']), cell(t['int4']),
                                                                   med(t['int4']) / med(t['fp16']), med(t['int4']) / med(t['fp8'])))
    for r in results:
        if r['step'] == 'memory':
            c = r['bytes']
            lines += ['', '### Cache memory at batch %d, t_max %d, MiB: the cache arrays (quantised kinds: with one layer of fp16 staging) and everything '
                      'the engine allocated' % (r['batch'], r['t_max']), '', '| | fp16 | fp8 | int4 |', '|---|---|---|---|',
                      '| cache arrays | %s |' % ' | '.join('%.0f' % (c[k]['arrays'] / 2 ** 20) for k in KINDS),
                      '| engine, all allocations | %s |' % ' | '.join('%.0f' % (c[k]['engine'] / 2 ** 20) for k in KINDS)]
    acc = [r for r in results if r['step'] == 'accuracy']
    if acc:
        lines += ['', '### int4 against fp16 on the same teacher-forced tokens (3 rows, 16-token prompts + 64 steps)', '',
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
