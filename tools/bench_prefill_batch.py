"""Batched prompt prefill: what one packed pass costs next to the per-sequence loop it replaces.

  table 1, the kernel alone: ONE gptq_prompt_attn_batch_f16 call (B segments of one packed qkv, csrc/prompt_attn.hip) against B calls of
           gptq_prompt_attn_f16 on the same rows and cache slices, 32 heads, start = 0, {cos, sin} from the table.
  table 2, time from ids to all first tokens on the 7B-shaped random model: DecodeEngine.prefill_batch against a loop of
           prefill(row=b, start=0) over the same prompts on the same DecodeEngine(batch=16), with the peak memory of each.
  cells:   B in {4, 16} x T in {16, 128, 512} (equal lengths) and one ragged batch: one prompt of 2047 tokens and fifteen of 16.

Device events, warm-up, REPEATS repeats of both sides interleaved in one process, medians (raw repeats printed too).  Every table is a child
process under its own `timeout`; at most 16 CPU threads.
    python tools/bench_prefill_batch.py [--markdown FILE]
    python tools/bench_prefill_batch.py --compare-lib OTHER.so     # gptq_prompt_attn_f16 of this tree's library against another build's, bit by bit"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'gptq-for-llama_amd')]
os.environ.setdefault('OMP_NUM_THREADS', '16')
REPEATS = 7
HEADS, HD, T_MAX = 32, 128, 2048
RAGGED = [2047] + [16] * 15
CELLS = [[T] * B for B in (4, 16) for T in (16, 128, 512)] + [RAGGED]
STEP_TIMEOUT = {'kernel': 240, 'ttft': 900}
# the cases of tests/test_gpu_prompt_attn.py (start, rows, t_max) for --compare-lib
CASES = [(0, 1, 384), (5, 1, 384), (0, 17, 384), (0, 64, 384), (0, 65, 384), (0, 130, 384), (130, 70, 384), (255, 129, 384), (150, 50, 200)]


def _label(lens):
    return '%d x %d' % (len(lens), lens[0]) if len(set(lens)) == 1 else ' + '.join('%d x %d' % (lens.count(t), t) for t in sorted(set(lens), reverse=True))


def _timed(fn, inner):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / inner          # us per call


def step_kernel(lens):
    import numpy as np
    import torch
    from quant import _native
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lib, dev = _native.lib(), torch.device('cuda:0')
    H, B, total = HEADS * HD, len(lens), sum(lens)
    s = _native.stream_ptr(dev)
    qkv = torch.randn((total, 3 * H), device=dev).half()
    kc = torch.zeros((B, T_MAX, H), dtype=torch.float16, device=dev)
    vc = torch.zeros((B, T_MAX, H), dtype=torch.float16, device=dev)
    out = torch.empty((total, H), dtype=torch.float16, device=dev)
    ws = torch.empty(lib.gptq_prompt_attn_workspace_bytes(total, HEADS, HD, T_MAX), dtype=torch.uint8, device=dev)
    tab = torch.empty((T_MAX, HD // 2, 2), dtype=torch.float32, device=dev)
    _native.check(lib.gptq_rope_table_f32(tab.data_ptr(), T_MAX, HD, 10000.0, s), 'rope_table')
    scale = float(1.0 / np.sqrt(HD))
    offs = [sum(lens[:i]) for i in range(B)]
    segs = (_native.PromptSeg * B)(*[_native.PromptSeg(offs[i], lens[i], 0, i) for i in range(B)])

    def packed():
        rc = lib.gptq_prompt_attn_batch_f16(qkv.data_ptr(), 3 * H, total, segs, B, kc.data_ptr(), vc.data_ptr(), T_MAX * H, out.data_ptr(), H,
                                            ws.data_ptr(), ws.numel(), HEADS, HD, T_MAX, 10000.0, scale, tab.data_ptr(), s)
        assert rc == 0, rc

    def loop():
        for i in range(B):
            rc = lib.gptq_prompt_attn_f16(qkv[offs[i]:].data_ptr(), 3 * H, lens[i], 0, kc[i].data_ptr(), vc[i].data_ptr(), out[offs[i]:].data_ptr(), H,
                                          ws.data_ptr(), ws.numel(), HEADS, HD, T_MAX, 10000.0, scale, tab.data_ptr(), s)
            assert rc == 0, rc

    inner = max(4, min(100, int(2e5 / total)))
    for f in (packed, loop):
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(REPEATS):                             # interleaved
        a.append(_timed(packed, inner))
        b.append(_timed(loop, inner))
    return dict(step='kernel', lens=lens, inner=inner, packed_us=a, loop_us=b)


def ttft_setup():
    import torch
    from quant import decode as D
    torch.set_num_threads(min(16, torch.get_num_threads()))
    model = D.build_random_llama('cuda:0', seed=0)
    return model, D.DecodeEngine(model, t_max=T_MAX, batch=16)


def step_ttft(lens, model, eng):
    import torch
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(sum(lens))
    prompts = [torch.randint(0, model.config.vocab_size, (t,), device=dev, generator=gen) for t in lens]
    B = len(lens)

    def packed():
        return eng.prefill_batch(prompts).argmax(dim=-1)

    def loop():                                          # the route before prefill_batch: one pass over the weights per prompt
        for b in range(B):
            eng.prefill(prompts[b], row=b, start=0)
        return eng.logits[:B].argmax(dim=-1)

    res = dict(step='ttft', lens=lens)
    eng._prefill_bufs = None                             # every cell pays for its own buffers: the peaks are those of this cell
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    for name, f in (('loop', loop), ('packed', packed)):             # (the loop first: its buffers are the smaller ones)
        eng._prefill_bufs = None
        torch.cuda.empty_cache()
        f()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        f()
        torch.cuda.synchronize()
        res[name + '_peak_MiB'] = round(torch.cuda.max_memory_allocated(dev) / 2**20, 1)
    res['resident_MiB'] = round(base / 2**20, 1)
    agree = int((packed() == loop()).sum())
    res['first_tokens_equal'] = '%d of %d' % (agree, B)
    a, b = [], []
    for _ in range(REPEATS):
        a.append(_timed(packed, 1) / 1000.0)
        b.append(_timed(loop, 1) / 1000.0)
    res['packed_ms'], res['loop_ms'] = a, b
    return res


def hash_lib(path):
    """sha256 of the output rows and both caches gptq_prompt_attn_f16 of the library at `path` leaves for every case of CASES"""
    import hashlib
    import numpy as np
    import torch
    heads, H, dev = 4, 4 * HD, 'cuda:0'
    lib = ctypes.CDLL(path)
    c_void_p, c_int, c_int64, c_float = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    lib.gptq_prompt_attn_f16.argtypes = [c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, ctypes.c_size_t, c_int, c_int,
                                         c_int, c_float, c_float, c_void_p, c_void_p]
    res = {}
    for start, rows, t_max in CASES:
        rng = np.random.default_rng(1000 * start + rows)
        qkv = torch.from_numpy(rng.standard_normal((rows, 3 * H)).astype(np.float16)).to(dev)
        kc = (rng.standard_normal((t_max, H)) * 0.5).astype(np.float16)
        vc = rng.standard_normal((t_max, H)).astype(np.float16)
        kc[start + rows:] = np.nan
        vc[start + rows:] = np.nan
        kc, vc = torch.from_numpy(kc).to(dev), torch.from_numpy(vc).to(dev)
        out = torch.zeros((rows, H), dtype=torch.float16, device=dev)
        ws = torch.empty(rows * H * 2 + 256, dtype=torch.uint8, device=dev)
        rc = lib.gptq_prompt_attn_f16(qkv.data_ptr(), 3 * H, rows, start, kc.data_ptr(), vc.data_ptr(), out.data_ptr(), H, ws.data_ptr(), ws.numel(),
                                      heads, HD, t_max, 10000.0, float(1.0 / np.sqrt(HD)), None, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out.float()).all())
        res['%d,%d,%d' % (start, rows, t_max)] = [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in (out, kc, vc)]
    return res


def compare_lib(other):
    """gptq_prompt_attn_f16 of this tree's library against the one at `other` (the parent commit's build), each in a process of its own:
    output and cache bits of CASES"""
    from quant import _native
    got = []
    for path in (_native.LIB_PATH, os.path.abspath(other)):
        cmd = ['timeout', '-k', '10', '120', sys.executable, os.path.abspath(__file__), '--hash-lib', path]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                            # a fault, an abort or a time limit: nothing more is started on the GPU
            print('%s ended with status %d: stopping' % (path, p.returncode))
            return 1
        got.append(json.loads([l for l in p.stdout.splitlines() if l.startswith('RESULT ')][-1][7:]))
    ok = True
    for start, rows, t_max in CASES:
        key = '%d,%d,%d' % (start, rows, t_max)
        same = [a == b for a, b in zip(got[0][key], got[1][key])]
        ok = ok and all(same)
        print('(start %3d, rows %3d, t_max %d): out %s, k cache %s, v cache %s' % ((start, rows, t_max) + tuple('equal' if x else 'DIFFERS' for x in same)))
    print('gptq_prompt_attn_f16: %s' % ('all bits agree' if ok else 'BITS DIFFER'))
    return 0 if ok else 1


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == '--compare-lib':
        return compare_lib(sys.argv[2])
    if len(sys.argv) >= 3 and sys.argv[1] == '--hash-lib':
        print('RESULT ' + json.dumps(hash_lib(sys.argv[2])), flush=True)
        return 0
    if len(sys.argv) >= 3 and sys.argv[1] == '--step':
        setup = ttft_setup() if sys.argv[2] == 'ttft' else ()
        for lens in CELLS:
            print('%s %s ...' % (sys.argv[2], _label(lens)), flush=True)
            r = (step_kernel if sys.argv[2] == 'kernel' else step_ttft)(lens, *setup)
            print('RESULT ' + json.dumps(r), flush=True)
        return 0
    results = []
    for kind in ('kernel', 'ttft'):
        cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT[kind]), sys.executable, os.path.abspath(__file__), '--step', kind]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
        for line in p.stdout:                            # streamed: a long step still shows progress
            print(line.rstrip(), flush=True)
            if line.startswith('RESULT '):
                results.append(json.loads(line[7:]))
        if p.wait() != 0:                                # a fault, an abort or a time limit: nothing more is started on the GPU
            print('step %s ended with status %d: stopping' % (kind, p.returncode))
            return 1
    lines = ['### Kernel alone (32 heads, start = 0; median of %d interleaved repeats, device events)' % REPEATS, '',
             '| prompts x tokens | packed rows | one gptq_prompt_attn_batch_f16 us | B x gptq_prompt_attn_f16 us | loop spread (max - min) us | ratio (loop / packed) |',
             '|---|---|---|---|---|---|']
    for r in results:
        if r['step'] == 'kernel':
            a, b = _median(r['packed_us']), _median(r['loop_us'])
            lines.append('| %s | %d | %.1f | %.1f | %.1f | %.2f |' % (_label(r['lens']), sum(r['lens']), a, b, max(r['loop_us']) - min(r['loop_us']), b / a))
    lines += ['', '### Ids to all first tokens, 7B-shaped random model, DecodeEngine(batch=16) (median of %d interleaved repeats)' % REPEATS, '',
              '| prompts x tokens | prefill_batch ms | loop of prefill ms | loop spread (max - min) ms | ratio (loop / packed) | packed peak MiB | loop peak MiB | first tokens equal |',
              '|---|---|---|---|---|---|---|---|']
    for r in results:
        if r['step'] == 'ttft':
            a, b = _median(r['packed_ms']), _median(r['loop_ms'])
            lines.append('| %s | %.2f | %.2f | %.2f | %.2f | %.1f | %.1f | %s |' % (_label(r['lens']), a, b, max(r['loop_ms']) - min(r['loop_ms']), b / a,
                                                                                  r['packed_peak_MiB'], r['loop_peak_MiB'], r['first_tokens_equal']))
    lines += ['', '### Raw repeats', '', '```'] + [json.dumps(r) for r in results] + ['```', '']
    text = '\n'.join(lines)
    print(text)
    if '--markdown' in sys.argv:
        with open(sys.argv[sys.argv.index('--markdown') + 1], 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
