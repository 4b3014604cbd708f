"""Constrained decoding in the engine: what gptq_constrain_rows_f16 (csrc/constrain.hip) and the constraint launch inside the native sampling
graph cost.

  table 1, the op: one launch on [B, 32000] fp16 logits (randn * 2.5), with `last`, B in {1, 16}, all rows constrained, 64 states, C in {2,
           300, 16384} classes, about half of the classes banned in every state; the token consumed is a self loop, so the state -- and the
           work -- is the same at every call.  The launch works in place and skips the store of a group of 8 that is banned already, so
           every timed call is preceded by a device copy that puts fresh logits back; the copy alone is timed next to it and subtracted.
  table 2, the engine, 7B-shaped random model with the finite-logits initialisation of bench.py's sampling leg (scales x 0.05), batch 1, a
           16-token prompt: us per replay of the capture_sample_native graph of an engine built with constrain=True under a 64-state, 300-class
           automaton against the same graph of an engine without the flag, both from the same state; and tokens/s of
           engine_generate(prefill='engine', sample=...) at 16 + 256 tokens with and without constrain=.
           --parent DIR (a built checkout of the parent commit) measures the flag-off pair there as well, in a process of its own that
           imports that tree: the flag off must be the parent's step.

Device events around a synchronised window, everything warmed up, REPEATS repeats with the candidates alternating in one process, medians and
max - min spreads (raw repeats printed too).  Every table is a child process under its own `timeout`; at most 16 CPU threads.
    python tools/bench_constrain.py [--markdown FILE] [--only op|engine] [--parent DIR]"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = sys.argv[sys.argv.index('--root') + 1] if '--root' in sys.argv else HERE       # (the tree a child step imports)
sys.path[:0] = [ROOT, os.path.join(ROOT, 'gptq-for-llama_amd')]
os.environ.setdefault('OMP_NUM_THREADS', '16')
REPEATS = 7
VOCAB = 32000
T_MAX = 2048
STATES = 64
SCRIPT = dict(temperature=0.8, top_p=0.95)           # llama_inference.py:119-127
STEPS = 128
NEW = 256
STEP_TIMEOUT = {'op': 300, 'engine': 600, 'parent': 600}


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


def _tables(rng, classes, vocab=VOCAB, states=STATES):
    """(next int16 [S, C], cls int16 [V]): about half of the classes banned per state, class 0 a self loop everywhere"""
    import numpy as np
    nxt = rng.integers(0, states, size=(states, classes)).astype(np.int16)
    nxt[rng.random(nxt.shape) < 0.5] = -1
    nxt[:, 0] = np.arange(states)
    cls = rng.integers(0, classes, size=vocab).astype(np.int16)
    cls[0] = 0
    return nxt, cls


def step_op(B, classes):
    import numpy as np
    import torch
    from quant import _native
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lib, dev = _native.lib(), torch.device('cuda:0')
    s = _native.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(B)
    rng = np.random.default_rng(classes)
    fresh = (torch.randn((B, VOCAB), device=dev, generator=g) * 2.5).half()
    logits = fresh.clone()
    nxt, cls = _tables(rng, classes)
    nx, cl = torch.from_numpy(nxt).to(dev), torch.from_numpy(np.repeat(cls[None], B, axis=0).copy()).to(dev)
    map_of = torch.arange(B, dtype=torch.int32, device=dev)
    state = torch.from_numpy(rng.integers(0, STATES, size=B).astype(np.int32)).to(dev)
    last = torch.zeros(B, dtype=torch.int64, device=dev)                       # token 0: class 0, the self loop
    ln = torch.full((B,), 16, dtype=torch.int64, device=dev)

    def launch():
        rc = lib.gptq_constrain_rows_f16(logits.data_ptr(), VOCAB, B, VOCAB, nx.data_ptr(), classes, STATES, classes, cl.data_ptr(), VOCAB, B,
                                         map_of.data_ptr(), state.data_ptr(), last.data_ptr(), ln.data_ptr(), 0, T_MAX, s)
        assert rc == 0, rc

    def both():
        logits.copy_(fresh)
        launch()
    cands = {'copy': lambda: logits.copy_(fresh), 'copy+launch': both, 'launch, already masked': launch}
    for f in cands.values():
        for _ in range(5):
            f()
    assert int(state.min()) >= 0 and bool(torch.isinf(logits).any())
    times = {name: [] for name in cands}
    for _ in range(REPEATS):                             # alternating
        for name, f in cands.items():
            times[name].append(_timed(f, 200))
    return dict(step='op', B=B, classes=classes, inner=200, us=times)


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
        return D.build_random_llama('cuda:0', seed=0)
    finally:
        D.fill_random_quant_ = fill


def step_engine(model, with_flag):
    """with_flag False: the flag-off engine alone, through nothing this commit added (what a checkout of the parent can run)"""
    import time
    import numpy as np
    import torch
    from quant import decode as D
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(1)
    prompt = torch.randint(1, VOCAB, (16,), device=dev, generator=gen)
    engines = dict(off=D.DecodeEngine(model, t_max=T_MAX).capture())
    dfa = None
    if with_flag:
        from quant.constrain import TokenDFA
        nxt, cls = _tables(np.random.default_rng(0), 300, vocab=model.lm_head.weight.shape[0])
        dfa = TokenDFA.from_table(nxt[:, cls])
        engines['on'] = D.DecodeEngine(model, t_max=T_MAX, constrain=True).capture()
    state = {}
    for name, eng in engines.items():
        eng.set_sampling(**SCRIPT)
        if name == 'on':
            eng.set_constraint(dfa)
        eng.capture_sample_native()
        logits = eng.prefill(prompt, start=0)
        eng.ids.copy_(torch.argmax(logits if name == 'off' else eng.constrain_logits(logits.to(torch.float16).contiguous()), dim=-1).reshape(1))
        state[name] = (eng.pos.clone(), eng.ids.clone()) + ((eng.c_state.clone(),) if name == 'on' else ())

    def timed_graph(name):
        eng = engines[name]
        eng.pos.copy_(state[name][0]); eng.ids.copy_(state[name][1]); eng.stepc.zero_()     # from the same state: the same context lengths
        if name == 'on':
            eng.c_state.copy_(state[name][2])
        return _timed(eng.sample_native_graph.replay, STEPS)
    torch.manual_seed(0)
    for name in engines:
        timed_graph(name)
    if with_flag:
        assert int(engines['on'].c_state[0]) >= 0        # the row is still inside its automaton: every replay did the whole work
    times = {name: [] for name in engines}
    for _ in range(REPEATS):
        for name in engines:
            times[name].append(timed_graph(name))
    res = dict(step='engine' if with_flag else 'parent', steps=STEPS, us_per_replay=times, classes=None if dfa is None else dfa.n_classes,
               states=None if dfa is None else dfa.n_states)

    # end to end: tokens/s of engine_generate, (t(NEW + 1 tokens) - t(1 token)) / NEW as benchmark_generate measures model.generate
    def generate(name, n):
        kw = dict(constrain=dfa) if name == 'on' else {}
        torch.manual_seed(0); torch.cuda.synchronize(); t0 = time.perf_counter()
        D.engine_generate(model, prompt[None], n, engine=engines[name], prefill='engine', sample=SCRIPT, **kw)      # (no eos_token_id: all NEW tokens)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    rates = {name: [] for name in engines}
    for name in engines:
        generate(name, 4)
    for _ in range(REPEATS):
        for name in engines:
            rates[name].append(NEW / (generate(name, NEW + 1) - generate(name, 1)))
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
        if kind == 'op':
            for B in (1, 16):
                for classes in (2, 300, 16384):
                    print('op B %d C %d ...' % (B, classes), flush=True)
                    print('RESULT ' + json.dumps(step_op(B, classes)), flush=True)
        else:
            print('%s ...' % kind, flush=True)
            print('RESULT ' + json.dumps(step_engine(engine_setup(), kind == 'engine')), flush=True)
        return 0
    kinds = [sys.argv[sys.argv.index('--only') + 1]] if '--only' in sys.argv else ['op', 'engine']
    parent = os.path.abspath(sys.argv[sys.argv.index('--parent') + 1]) if '--parent' in sys.argv else None
    if parent is not None and 'engine' in kinds:
        kinds.append('parent')
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
    lines = ['### The op: [B, %d] fp16 logits, %d states, all rows constrained, us: median (max - min) of %d alternating repeats of 200 calls, '
             'device events' % (VOCAB, STATES, REPEATS), '',
             '| B | classes | copy of fresh logits | copy + launch | launch = the difference | launch on logits masked already |', '|---|---|---|---|---|---|']
    for r in results:
        if r['step'] == 'op':
            u = r['us']
            lines.append('| %d | %d | %s | %s | %.1f | %s |' % (r['B'], r['classes'], cell(u['copy']), cell(u['copy+launch']),
                                                                _median(u['copy+launch']) - _median(u['copy']), cell(u['launch, already masked'])))
    for r in results:
        if r['step'] == 'engine':
            t, q = r['us_per_replay'], r['tokens_per_s']
            lines += ['', '### The engine: 7B-shaped random model (scales x 0.05), batch 1, a 16-token prompt, an automaton of %d states and %d '
                      'classes: median (max - min) of %d alternating repeats' % (r['states'], r['classes'], REPEATS), '',
                      '| | flag off | constrain=True | on - off | on / off |', '|---|---|---|---|---|',
                      '| capture_sample_native, us / replay over %d steps | %s | %s | %.1f | %.4f |' % (
                          r['steps'], cell(t['off']), cell(t['on']), _median(t['on']) - _median(t['off']), _median(t['on']) / _median(t['off'])),
                      '| engine_generate, 16 + %d tokens, tok/s | %s | %s | %.1f | %.4f |' % (
                          NEW, cell(q['off']), cell(q['on']), _median(q['on']) - _median(q['off']), _median(q['on']) / _median(q['off']))]
        if r['step'] == 'parent':
            lines += ['', '### The parent commit, the same two measurements in a process of its own', '', '| | parent |', '|---|---|',
                      '| capture_sample_native, us / replay over %d steps | %s |' % (r['steps'], cell(r['us_per_replay']['off'])),
                      '| engine_generate, 16 + %d tokens, tok/s | %s |' % (NEW, cell(r['tokens_per_s']['off']))]
    lines += ['', '### Raw repeats', '', '```'] + [json.dumps(r) for r in results] + ['```', '']
    text = '\n'.join(lines)
    print(text)
    if '--markdown' in sys.argv:
        with open(sys.argv[sys.argv.index('--markdown') + 1], 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
