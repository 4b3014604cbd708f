"""Token log-probabilities in the engine: what gptq_logprobs_rows_f16 (csrc/logprobs.hip) and the record launch inside the self-feeding graphs
cost.

  table 1, the op: one launch on [B, 32000] fp16 logits (randn * 2.5), B in {1, 16}, top K in {0, 5, 32}, the chosen ids random, the slot read
           from a device counter as the engine's launch does (a ring of 2049 slots).
  table 2, the engine, 7B-shaped random model with the finite-logits initialisation of bench.py's sampling leg (scales x 0.05), batch 1, a
           16-token prompt: us per replay of the capture_sample_native graph of an engine built with logprobs=5 against the same graph of an
           engine without the flag (the parent's step: the baseline), both from the same state; and tokens/s of
           engine_generate(prefill='engine', sample=...) at 16 + 256 tokens with logprobs=5 and without.

Device events around a synchronised window, everything warmed up, REPEATS repeats with the candidates alternating in one process, medians and
max - min spreads (raw repeats printed too).  Every table is a child process under its own `timeout`; at most 16 CPU threads.
    python tools/bench_logprobs.py [--markdown FILE] [--only op|engine]          (FILE defaults to profiles/logprobs/README.md)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'gptq-for-llama_amd')]
os.environ.setdefault('OMP_NUM_THREADS', '16')
REPEATS = 7
VOCAB = 32000
T_MAX = 2048
SCRIPT = dict(temperature=0.8, top_p=0.95)           # llama_inference.py:119-127
K = 5
STEPS = 128
NEW = 256
STEP_TIMEOUT = {'op': 300, 'engine': 600}
BEAM_SELECT_US = 29.0                                # README: gptq_beam_select_f16 at N = 4, two launches


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
    ids = torch.randint(0, VOCAB, (B,), device=dev, generator=g)
    step = torch.tensor([7], dtype=torch.int64, device=dev)
    steps = T_MAX + 1

    def launch(top):
        chosen = torch.zeros((steps, B), dtype=torch.float32, device=dev)
        rank = torch.zeros((steps, B), dtype=torch.int32, device=dev)
        top_ids = torch.zeros((steps, B, max(top, 1)), dtype=torch.int32, device=dev)
        top_lp = torch.zeros((steps, B, max(top, 1)), dtype=torch.float32, device=dev)

        def run():
            rc = lib.gptq_logprobs_rows_f16(logits.data_ptr(), VOCAB, B, VOCAB, ids.data_ptr(), top, step.data_ptr(), steps, chosen.data_ptr(),
                                            rank.data_ptr(), top_ids.data_ptr(), top_lp.data_ptr(), s)
            assert rc == 0, rc
        return run
    cands = {'k%d' % top: launch(top) for top in (0, 5, 32)}
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
    engines = dict(off=D.DecodeEngine(model, t_max=T_MAX).capture(), on=D.DecodeEngine(model, t_max=T_MAX, logprobs=K).capture())
    state = {}
    for name, eng in engines.items():
        eng.set_sampling(**SCRIPT)
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
        torch.manual_seed(0); torch.cuda.synchronize(); t0 = time.perf_counter()
        D.engine_generate(model, prompt[None], n, engine=engines[name], prefill='engine', sample=SCRIPT,        # (no eos_token_id: all NEW tokens)
                          logprobs=K if name == 'on' else None)
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
    lines = ['# Token log-probabilities in the engine: `gptq_logprobs_rows_f16`, the record launch of the self-feeding step, '
             '`engine_generate(logprobs=K)`', '', 'Written by `tools/bench_logprobs.py` on one MI355X.', '',
             '### The op: [B, %d] fp16 logits, us per launch: median (max - min) of %d alternating repeats of 200 launches, device events' % (
                 VOCAB, REPEATS), '', '| B | K = 0 | K = 5 | K = 32 |', '|---|---|---|---|']
    ops = [r for r in results if r['step'] == 'op']
    for r in ops:
        lines.append('| %d | %s | %s | %s |' % (r['B'], cell(r['us']['k0']), cell(r['us']['k5']), cell(r['us']['k32'])))
    if ops:
        worst = max(_median(v) for r in ops for v in r['us'].values())
        lines += ['', 'The expectation was a launch below the two launches of `gptq_beam_select_f16` at N = 4 (%.1f us, README): the slowest cell '
                  'here is %.1f us -- %s.' % (BEAM_SELECT_US, worst, 'confirmed' if worst < BEAM_SELECT_US else 'REFUTED')]
    for r in results:
        if r['step'] == 'engine':
            t, q = r['us_per_replay'], r['tokens_per_s']
            lines += ['', '### The engine: 7B-shaped random model (scales x 0.05), batch 1, a 16-token prompt: median (max - min) of %d alternating '
                      'repeats' % REPEATS, '', '| | flag off (the parent\'s step) | logprobs=%d | on - off | on / off |' % K, '|---|---|---|---|---|',
                      '| capture_sample_native, us / replay over %d steps | %s | %s | %.1f | %.4f |' % (
                          r['steps'], cell(t['off']), cell(t['on']), _median(t['on']) - _median(t['off']), _median(t['on']) / _median(t['off'])),
                      '| engine_generate, 16 + %d tokens, tok/s | %s | %s | %.1f | %.4f |' % (
                          NEW, cell(q['off']), cell(q['on']), _median(q['on']) - _median(q['off']), _median(q['on']) / _median(q['off'])),
                      '', 'The step ratio of the logit processors, for comparison: 1.0035 x (profiles/logits_process/README.md).']
    lines += ['', '### Raw repeats', '', '```'] + [json.dumps(r) for r in results] + ['```', '']
    text = '\n'.join(lines)
    print(text)
    out = sys.argv[sys.argv.index('--markdown') + 1] if '--markdown' in sys.argv else os.path.join(ROOT, 'profiles', 'logprobs', 'README.md')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
