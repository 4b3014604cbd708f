"""Prompt attention and engine-native prefill: what they cost next to the route they replace.

  table 1, the kernel alone: gptq_prompt_attn_f16 (RoPE + cache append + causal attention, csrc/prompt_attn.hip) against the gptq_rope_f16 launch
           plus F.scaled_dot_product_attention(is_causal=True) of QuantLlamaAttention.forward, same fp16 inputs, 32 heads, start = 0.
           FLOPs counted: 2 T^2 128 heads (the causal half of 4 T^2 128 heads).
  table 2, time to first token on the 7B-shaped random model: DecodeEngine.prefill against the route of engine_generate(prefill='hf') (module
           chain into a DynamicCache, copy into the engine's cache), with the peak memory of each.

Device events, warm-up, REPEATS repeats of both sides interleaved in one process, medians (raw repeats printed too).  Every GPU step is a child
process under its own `timeout`; at most 16 CPU threads.
    python tools/bench_prompt_attn.py [--markdown FILE]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'gptq-for-llama_amd')]
os.environ.setdefault('OMP_NUM_THREADS', '16')
REPEATS = 7
HEADS, HD = 32, 128
STEPS = [('kernel', [128, 512, 1024, 2047]), ('ttft', [16, 128, 512, 2047])]       # one child process per table (the model is built once)
STEP_TIMEOUT = {'kernel': 240, 'ttft': 600}


def _timed(fn, inner):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / inner          # us per call


def step_kernel(T):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from quant import _native, fused_attn
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lib, dev = _native.lib(), torch.device('cuda:0')
    H, t_max = HEADS * HD, 2048
    s = _native.stream_ptr(dev)
    qkv = torch.randn((T, 3 * H), device=dev).half()
    kc, vc = torch.zeros((t_max, H), dtype=torch.float16, device=dev), torch.zeros((t_max, H), dtype=torch.float16, device=dev)
    out = torch.empty((T, H), dtype=torch.float16, device=dev)
    ws = torch.empty(lib.gptq_prompt_attn_workspace_bytes(T, HEADS, HD, t_max), dtype=torch.uint8, device=dev)
    tab = torch.empty((t_max, HD // 2, 2), dtype=torch.float32, device=dev)
    _native.check(lib.gptq_rope_table_f32(tab.data_ptr(), t_max, HD, 10000.0, s), 'rope_table')
    scale = float(1.0 / np.sqrt(HD))
    pos = torch.arange(T, device=dev).view(1, T)
    work = qkv.clone()

    def ours():
        rc = lib.gptq_prompt_attn_f16(qkv.data_ptr(), 3 * H, T, 0, kc.data_ptr(), vc.data_ptr(), out.data_ptr(), H, ws.data_ptr(), ws.numel(), HEADS, HD,
                                      t_max, 10000.0, scale, tab.data_ptr(), s)
        assert rc == 0, rc

    def sdpa():                                          # QuantLlamaAttention.forward between qkv_proj and o_proj (the in-place RoPE needs its own qkv)
        v5 = work.view(1, T, 3, HEADS, HD)
        fused_attn.hip_rotate_half_(v5[:, :, :2], pos)
        q, k, v = (v5[:, :, i].transpose(1, 2) for i in range(3))
        return F.scaled_dot_product_attention(q, k, v, is_causal=T > 1).transpose(1, 2).reshape(1, T, H)

    inner = max(4, min(200, int(2e5 / T)))
    for f in (ours, sdpa):
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(REPEATS):                             # interleaved
        a.append(_timed(ours, inner))
        b.append(_timed(sdpa, inner))
    flop = 2.0 * T * T * HD * HEADS
    return dict(step='kernel', T=T, inner=inner, ours_us=a, sdpa_us=b, flop=flop)


def ttft_setup():
    import torch
    from quant import decode as D
    torch.set_num_threads(min(16, torch.get_num_threads()))
    model = D.build_random_llama('cuda:0', seed=0)
    return model, D.DecodeEngine(model, t_max=2048)


def step_ttft(T, model, eng):
    import torch
    from quant import decode as D
    from transformers.cache_utils import DynamicCache
    dev = torch.device('cuda:0')
    ids = torch.randint(0, model.config.vocab_size, (1, T), device=dev, generator=torch.Generator(device=dev).manual_seed(T))

    def engine():
        return eng.prefill(ids[0], start=0).argmax()

    def hf():                                            # engine_generate(prefill='hf'): module chain, DynamicCache, copy
        with torch.no_grad():
            cache = DynamicCache(config=model.config)
            out = model(ids, past_key_values=cache, use_cache=True)
            for li in range(len(eng.layers)):
                k, v = D._cache_layer_kv(cache, li)
                eng.kc[li, :T].copy_(k[0].transpose(0, 1).reshape(T, -1))
                eng.vc[li, :T].copy_(v[0].transpose(0, 1).reshape(T, -1))
            eng.pos.fill_(T)
            return out.logits[0, -1].argmax()

    res = dict(step='ttft', T=T)
    for name, f in (('engine', engine), ('hf', hf)):
        for _ in range(2):
            f()
        torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    for name, f in (('engine', engine), ('hf', hf)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        f()
        torch.cuda.synchronize()
        res[name + '_peak_MiB'] = round(torch.cuda.max_memory_allocated(dev) / 2**20, 1)
    res['resident_MiB'] = round(base / 2**20, 1)
    a, b = [], []
    for _ in range(REPEATS):
        a.append(_timed(engine, 1) / 1000.0)
        b.append(_timed(hf, 1) / 1000.0)
    res['engine_ms'], res['hf_ms'] = a, b
    return res


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == '--step':
        setup = ttft_setup() if sys.argv[2] == 'ttft' else ()
        for T in sys.argv[3].split(','):
            print('%s T=%s ...' % (sys.argv[2], T), flush=True)
            r = (step_kernel if sys.argv[2] == 'kernel' else step_ttft)(int(T), *setup)
            print('RESULT ' + json.dumps(r), flush=True)
        return 0
    results = []
    for kind, Ts in STEPS:
        cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT[kind]), sys.executable, os.path.abspath(__file__), '--step', kind, ','.join(map(str, Ts))]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
        for line in p.stdout:                            # streamed: a long step still shows progress
            print(line.rstrip(), flush=True)
            if line.startswith('RESULT '):
                results.append(json.loads(line[7:]))
        if p.wait() != 0:                                # a fault, an abort or a time limit: nothing more is started on the GPU
            print('step %s ended with status %d: stopping' % (kind, p.returncode))
            return 1
    lines = ['### Kernel alone (32 heads, start = 0; median of %d interleaved repeats, device events)' % REPEATS, '',
             '| T | gptq_prompt_attn_f16 us | TFLOP/s | gptq_rope_f16 + SDPA us | TFLOP/s | ratio (SDPA / ours) |', '|---|---|---|---|---|---|']
    for r in results:
        if r['step'] == 'kernel':
            a, b = _median(r['ours_us']), _median(r['sdpa_us'])
            lines.append('| %d | %.1f | %.1f | %.1f | %.1f | %.2f |' % (r['T'], a, r['flop'] / a / 1e6, b, r['flop'] / b / 1e6, b / a))
    lines += ['', '### Time to first token, 7B-shaped random model (median of %d interleaved repeats)' % REPEATS, '',
              "| T | eng.prefill ms | prefill='hf' route ms | hf spread (max - min) ms | engine peak MiB | hf peak MiB |", '|---|---|---|---|---|---|']
    for r in results:
        if r['step'] == 'ttft':
            lines.append('| %d | %.2f | %.2f | %.2f | %.1f | %.1f |' % (r['T'], _median(r['engine_ms']), _median(r['hf_ms']), max(r['hf_ms']) - min(r['hf_ms']),
                                                                      r['engine_peak_MiB'], r['hf_peak_MiB']))
    lines += ['', '### Raw repeats', '', '```'] + [json.dumps(r) for r in results] + ['```', '']
    text = '\n'.join(lines)
    print(text)
    if '--markdown' in sys.argv:
        with open(sys.argv[sys.argv.index('--markdown') + 1], 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
