"""Logit processors in the engine: what gptq_logits_process_f16 (csrc/logits_process.hip) and the process launch inside the native sampling
graph cost.

  table 1, the op: one launch on [B, 32000] fp16 logits (randn * 2.5), R = 1 with `last`, B in {1, 4, 16}, a history of 16 / 512 / 2047 of 2048
           tokens drawn uniformly from the vocabulary (nearly all distinct: the most read-modify-writes a history of that length can ask for),
           repetition_penalty 1.18, presence_penalty 0.5, min_new_tokens on with one eos id, two bias entries.  The launch works in place, so
           the logits drift from call to call; the work per call -- bitmap clear, history scan, one RMW per distinct token -- does not.
  table 2, the engine, 7B-shaped random model with the finite-logits initialisation of bench.py's sampling leg (scales x 0.05), batch 1, a
           16-token prompt: us per replay of the capture_sample_native graph of an engine built with logits_process=True against the same
           graph of an engine without the flag (the parent's step: the baseline), both from the same state; and tokens/s of
           engine_generate(prefill='engine', sample=...) at 16 + 256 tokens with and without the processor keys.

Device events around a synchronised window, everything warmed up, REPEATS repeats with the candidates alternating in one process, medians and
max - min spreads (raw repeats printed too).  Every table is a child process under its own `timeout`; at most 16 CPU threads.
    python tools/bench_logits_process.py [--markdown FILE] [--only op|engine]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'gptq-for-llama_amd')]
os.environ.setdefault('OMP_NUM_THREADS', '16')
REPEATS = 7
VOCAB = 32000
T_HIST = 2048
SCRIPT = dict(temperature=0.8, top_p=0.95)           # llama_inference.py:119-127
PROCESS = dict(repetition_penalty=1.18, presence_penalty=0.5, min_new_tokens=8, logit_bias={5: -float('inf'), 6: 1.5})
EOS = 2
STEPS = 128
NEW = 256
STEP_TIMEOUT = {'op': 300, 'engine': 600}


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


def step_op(B):
    import torch
    from quant import _native
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lib, dev = _native.lib(), torch.device('cuda:0')
    s = _native.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(B)
    logits = (torch.randn((B, VOCAB), device=dev, generator=g) * 2.5).half()
    hist = torch.randint(0, VOCAB, (B, T_HIST), device=dev, generator=g).int()
    last = torch.randint(0, VOCAB, (B,), device=dev, generator=g)
    gen_start = torch.full((B,), 8, dtype=torch.int64, device=dev)
    rp, pp = torch.full((B,), 1.18, device=dev), torch.full((B,), 0.5, device=dev)
    mn = torch.full((B,), 4096, dtype=torch.int32, device=dev)
    eos = torch.tensor([EOS], dtype=torch.int32, device=dev)
    bias_ids, bias_vals = torch.tensor([5, 6], dtype=torch.int32, device=dev), torch.tensor([-float('inf'), 1.5], device=dev)

    def launch(n):
        ln = torch.full((B,), n, dtype=torch.int64, device=dev)

        def run():
            rc = lib.gptq_logits_process_f16(logits.data_ptr(), VOCAB, B, 1, VOCAB, hist.data_ptr(), T_HIST, T_HIST, last.data_ptr(), ln.data_ptr(), 0,
                                             gen_start.data_ptr(), rp.data_ptr(), pp.data_ptr(), mn.data_ptr(), eos.data_ptr(), 1,
                                             bias_ids.data_ptr(), bias_vals.data_ptr(), 2, s)
            assert rc == 0, rc
        return run
    cands = {'n%d' % n: launch(n) for n in (16, 512, 2047)}
    for f in cands.values():
        for _ in range(5):
            f()
    times = {name: [] for name in cands}
    for _ in range(REPEATS):                             # alternating
        for name, f in cands.items():
            times[name].append(_timed(f, 200))
    return dict(step='op', B=B, inner=200, us=times)


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


def step_engine(model):
    import time
    import torch
    from quant import decode as D
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(1)
    prompt = torch.randint(1, VOCAB, (16,), device=dev, generator=gen)
    engines = dict(off=D.DecodeEngine(model, t_max=T_HIST).capture(), on=D.DecodeEngine(model, t_max=T_HIST, logits_process=True).capture())
    state = {}
    for name, eng in engines.items():
        eng.set_sampling(**SCRIPT)
        if name == 'on':
            eng.set_logits_process(eos_token_id=EOS, **PROCESS)
        eng.capture_sample_native()
        logits = eng.prefill(prompt, start=0)
        eng.ids.copy_(torch.argmax(logits, dim=-1).reshape(1))
        state[name] = (eng.pos.clone(), eng.ids.clone())

    def timed_graph(name):
        eng = engines[name]
        eng.pos.copy_(state[name][0]); eng.ids.copy_(state[name][1]); eng.stepc.zero_()     # from the same state: the same context lengths
        return _timed(eng.sample_native_graph.replay, STEPS)
    torch.manual_seed(0)
    for name in engines:
        timed_graph(name)
    times = {name: [] for name in engines}
    for _ in range(REPEATS):
        for name in engines:
            times[name].append(timed_graph(name))
    res = dict(step='engine', steps=STEPS, us_per_replay=times)

    # end to end: tokens/s of engine_generate, (t(NEW + 1 tokens) - t(1 token)) / NEW as benchmark_generate measures model.generate
    def generate(name, n):
        sample = dict(SCRIPT, **PROCESS) if name == 'on' else SCRIPT
        torch.manual_seed(0); torch.cuda.synchronize(); t0 = time.perf_counter()
        D.engine_generate(model, prompt[None], n, engine=engines[name], prefill='engine', sample=sample)      # (no eos_token_id: all NEW tokens)
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
            for B in (1, 4, 16):
                print('op %d ...' % B, flush=True)
                print('RESULT ' + json.dumps(step_op(B)), flush=True)
        else:
            print('engine ...', flush=True)
            print('RESULT ' + json.dumps(step_engine(engine_setup())), flush=True)
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
    lines = ['### The op: [B, %d] fp16 logits, R = 1, us per launch: median (max - min) of %d alternating repeats of 200 launches, device events' % (
        VOCAB, REPEATS), '', '| B | history 16 | history 512 | history 2047 |', '|---|---|---|---|']
    for r in results:
        if r['step'] == 'op':
            lines.append('| %d | %s | %s | %s |' % (r['B'], cell(r['us']['n16']), cell(r['us']['n512']), cell(r['us']['n2047'])))
    for r in results:
        if r['step'] == 'engine':
            t, q = r['us_per_replay'], r['tokens_per_s']
            lines += ['', '### The engine: 7B-shaped random model (scales x 0.05), batch 1, a 16-token prompt: median (max - min) of %d alternating '
                      'repeats' % REPEATS, '', '| | flag off (the parent\'s step) | logits_process=True | on - off | on / off |', '|---|---|---|---|---|',
                      '| capture_sample_native, us / replay over %d steps | %s | %s | %.1f | %.4f |' % (
                          r['steps'], cell(t['off']), cell(t['on']), _median(t['on']) - _median(t['off']), _median(t['on']) / _median(t['off'])),
                      '| engine_generate, 16 + %d tokens, tok/s | %s | %s | %.1f | %.4f |' % (
                          NEW, cell(q['off']), cell(q['on']), _median(q['on']) - _median(q['off']), _median(q['on']) / _median(q['off']))]
    lines += ['', '### Raw repeats', '', '```'] + [json.dumps(r) for r in results] + ['```', '']
    text = '\n'.join(lines)
    print(text)
    if '--markdown' in sys.argv:
        with open(sys.argv[sys.argv.index('--markdown') + 1], 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
