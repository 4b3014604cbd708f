#!/usr/bin/env python
"""Measure the grouped-query decode attention (csrc/decode_attn_gqa.hip) and the engine on a grouped-query model; writes profiles/gqa/.

  attention   gptq_decode_attn_batch_gqa_f16 at 32 query heads, G = 4 and 8, B = 1 / 4 / 16, 16 / 512 / 2047 tokens, against
              gptq_decode_attn_batch_f16 on 32 full K/V heads (the same query work on G x the cache bytes).  Each figure is the time per call of a
              captured graph of CALLS calls, the median of REPS replays, taken in the order yardstick, grouped, yardstick: the distance between the
              two yardstick figures is the spread a difference has to exceed.  The yardstick runs on the grouped inputs with every K/V head
              repeated G times, and the two outputs are compared at every size that is timed.
  engine      a Llama-3-8B-shaped random model (32 heads on 8 K/V heads): the captured greedy-rows step at three depths, and engine_generate
              tok/s against model.generate on the eager module chain (the hook switched off).

    python tools/bench_gqa.py [--skip-engine] [--out profiles/gqa]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'gptq-for-llama_amd'))

import torch  # noqa: E402

from quant import _native  # noqa: E402
from quant import decode as D  # noqa: E402

DEV = 'cuda:0'
HD, T_MAX, HEADS = 128, 2048, 32
CALLS, REPS = 20, 15


def graph_time_us(call):
    """median microseconds per call of a captured graph of CALLS calls"""
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            call()
    g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1000.0 / CALLS)
    return statistics.median(times)


def attention_rows():
    lib = _native.lib()
    f16 = dict(dtype=torch.float16, device=DEV)
    rows = []
    for G in (4, 8):
        kv = HEADS // G
        for B in (1, 4, 16):
            H, KV = HEADS * HD, kv * HD
            # the yardstick's inputs are the grouped ones with every K/V head repeated G times: both entries must compute the same rows
            rep = lambda t: t.unflatten(-1, (kv, 1, HD)).expand(*t.shape[:-1], kv, G, HD).reshape(*t.shape[:-1], H)
            qkv_gqa = torch.randn((B, H + 2 * KV), **f16)
            qkv_gqa[:, H:H + KV] *= 0.2
            qkv_full = torch.cat([qkv_gqa[:, :H], rep(qkv_gqa[:, H:H + KV]), rep(qkv_gqa[:, H + KV:])], 1)
            kg, vg = (0.2 * torch.randn((B, T_MAX, KV), **f16), torch.randn((B, T_MAX, KV), **f16))
            kf, vf = rep(kg), rep(vg)
            out, out_g = torch.zeros((B, H), **f16), torch.zeros((B, H), **f16)
            nb_f = lib.gptq_decode_attn_batch_workspace_bytes(B, HEADS, HD, T_MAX)
            nb_g = lib.gptq_decode_attn_batch_gqa_workspace_bytes(B, HEADS, kv, HD, T_MAX)
            ws_f, ws_g = torch.zeros(nb_f, dtype=torch.uint8, device=DEV), torch.zeros(nb_g, dtype=torch.uint8, device=DEV)
            for tokens in (16, 512, 2047):
                pos = torch.full((B,), tokens - 1, dtype=torch.int64, device=DEV)

                def full():
                    s = torch.cuda.current_stream().cuda_stream
                    _native.check(lib.gptq_decode_attn_batch_f16(qkv_full.data_ptr(), 3 * H, pos.data_ptr(), kf.data_ptr(), vf.data_ptr(), out.data_ptr(), H,
                                                                 ws_f.data_ptr(), nb_f, B, HEADS, HD, T_MAX, 10000.0, 0.0884, None, None, s), 'batch_f16')

                def gqa():
                    s = torch.cuda.current_stream().cuda_stream
                    _native.check(lib.gptq_decode_attn_batch_gqa_f16(qkv_gqa.data_ptr(), H + 2 * KV, pos.data_ptr(), kg.data_ptr(), vg.data_ptr(), out_g.data_ptr(),
                                                                     H, ws_g.data_ptr(), nb_g, B, HEADS, kv, HD, T_MAX, 10000.0, 0.0884, None, None, s), 'gqa')
                y1, g, y2 = graph_time_us(full), graph_time_us(gqa), graph_time_us(full)
                torch.cuda.synchronize()
                diff = float((out_g.float() - out.float()).abs().max())          # two fp16 roundings of the same rows: a few fp16 ulps of |out| <= ~1
                if not diff < 1e-3:
                    sys.exit('bench_gqa: the grouped entry and the yardstick disagree by %g at G=%d B=%d tokens=%d' % (diff, G, B, tokens))
                row = dict(G=G, B=B, tokens=tokens, yardstick_us=[round(y1, 2), round(y2, 2)], gqa_us=round(g, 2), spread_us=round(abs(y1 - y2), 2),
                           not_slower=bool(g <= max(y1, y2) + abs(y1 - y2)), max_abs_diff=diff)
                print(json.dumps(row), flush=True)
                rows.append(row)
            del kf, vf, kg, vg
            torch.cuda.empty_cache()
    return rows


def engine_rows():
    cfg = dict(hidden_size=4096, intermediate_size=14336, num_hidden_layers=32, num_attention_heads=32, num_key_value_heads=8, vocab_size=128256,
               max_position_embeddings=8192)
    model = D.build_random_llama(DEV, bits=4, groupsize=128, seed=0, fused=True, **cfg)
    res = dict(model='Llama-3-8B shape, random 4-bit g128 weights')
    eng = D.DecodeEngine(model, t_max=T_MAX)
    with torch.no_grad():
        g = eng.graph_for('greedy_rows')
        steps = {}
        for depth in (16, 512, 2000):
            eng.pos.fill_(depth)
            for _ in range(3):
                g.replay()
            torch.cuda.synchronize()
            eng.pos.fill_(depth)
            t0 = time.perf_counter()
            for _ in range(32):
                g.replay()
            torch.cuda.synchronize()
            steps[depth] = round((time.perf_counter() - t0) / 32 * 1e6, 1)
        res['greedy_rows_step_us_at_depth'] = steps
        ids = torch.randint(1, 1000, (1, 16), device=DEV)
        new = 128
        for name, run in (('engine_generate', lambda: D.engine_generate(model, ids, new, engine=eng)),
                          ('eager_chain_generate', lambda: model.generate(ids, do_sample=False, max_new_tokens=new, min_new_tokens=new, pad_token_id=0,
                                                                          attention_mask=torch.ones_like(ids)))):
            model._gptq_engine_disabled = name.startswith('eager')
            try:
                rates = []
                for _ in range(3):                      # the first run warms up
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run()
                    torch.cuda.synchronize()
                    rates.append(new / (time.perf_counter() - t0))
            finally:
                model._gptq_engine_disabled = False
            res[name + '_tok_s'] = [round(r, 1) for r in rates[1:]]
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gqa'))
    ap.add_argument('--skip-engine', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_gqa: no GPU (a CPU run measures nothing)')
    os.makedirs(a.out, exist_ok=True)
    res = dict(device=torch.cuda.get_device_name(0), calls_per_graph=CALLS, replays=REPS, attention=attention_rows())
    if not a.skip_engine:
        res['engine'] = engine_rows()
    with open(os.path.join(a.out, 'bench_gqa.json'), 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
