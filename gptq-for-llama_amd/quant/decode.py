"""Decode-latency harness for the drop-in modules: the measurement protocol of the reference's
``benchmark()`` (llama.py:385-438) on a random-init LLaMA-shaped model (no network, no
checkpoint): one token per step with a KV cache, a device sync per step, the median step time.

``build_random_llama`` goes through exactly the module surgery the reference's ``load_quant``
performs (llama_inference.py:27-72): ``make_quant_linear`` on every decoder linear (lm_head stays
fp16, :46-48), then ``make_quant_attn``, ``make_quant_norm``, ``make_fused_mlp``.  The packed
buffers are filled with the synthetic distribution of SURVEY 8(d) directly on the GPU.
"""
import functools
import math
import time

import numpy as np
import os
import torch

from . import fused_attn, fused_mlp, quant_linear, triton_norm

LLAMA_7B = dict(hidden_size=4096, intermediate_size=11008, num_hidden_layers=32, num_attention_heads=32,
                num_key_value_heads=32, vocab_size=32000, max_position_embeddings=2048, rms_norm_eps=1e-6)


def find_layers(module, layers=(torch.nn.Linear,), name=''):
    """same contract as the reference's utils/modelutils.py:7-13 (exact type match)."""
    if type(module) in layers:
        return {name: module}
    res = {}
    for name1, child in module.named_children():
        res.update(find_layers(child, layers=layers, name=name + '.' + name1 if name != '' else name1))
    return res


def fill_random_quant_(layer, gen):
    """uniform int32 bit patterns, scales ~ U(0.001, 0.011) fp16, trivial g_idx."""
    dev = layer.qweight.device
    layer.qweight.copy_(torch.randint(-2**31, 2**31 - 1, layer.qweight.shape, dtype=torch.int32, device=dev, generator=gen))
    layer.qzeros.copy_(torch.randint(-2**31, 2**31 - 1, layer.qzeros.shape, dtype=torch.int32, device=dev, generator=gen))
    layer.scales.copy_((torch.rand(layer.scales.shape, device=dev, generator=gen) * 0.01 + 0.001).half())
    gs = layer.groupsize if layer.groupsize != -1 else layer.infeatures
    layer.g_idx.copy_((torch.arange(layer.infeatures, device=dev) // gs).to(torch.int32))
    if layer.bias is not None:
        layer.bias.zero_()


def build_random_llama(dev='cuda:0', bits=4, groupsize=128, seed=0, fused=True, act_order=False, **overrides):
    """random-init LLaMA (7B shape by default) with every decoder linear replaced by a QuantLinear
    holding random packed weights, then fused attention / norm / MLP like load_quant().
    act_order: every linear gets a non-trivial g_idx of the shape gptq.py:210-216 produces (exactly `groupsize`
    members per group); linears that share their input (q/k/v, gate/up) share the permutation, as in a real
    --act-order checkpoint (same input => same Hessian diagonal)."""
    from transformers import LlamaConfig, LlamaForCausalLM
    from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding

    cfg = dict(LLAMA_7B)
    cfg.update(overrides)
    config = LlamaConfig(**cfg)
    with torch.device('meta'):
        model = LlamaForCausalLM(config)
    model = model.half().eval()
    layers = find_layers(model)
    for name in ['lm_head']:
        layers.pop(name, None)
    with torch.device('meta'):
        quant_linear.make_quant_linear(model, layers, bits, groupsize)
    model = model.to_empty(device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    with torch.no_grad():
        for _, m in model.named_modules():
            if isinstance(m, quant_linear.QuantLinear):
                fill_random_quant_(m, gen)
        if act_order:
            for layer in model.model.layers:
                K = layer.self_attn.q_proj.infeatures
                gs = groupsize if groupsize != -1 else K

                def random_g_idx(k):
                    inv = torch.argsort(torch.randperm(k, device=dev, generator=gen))
                    return (torch.arange(k, device=dev) // (groupsize if groupsize != -1 else k))[inv].to(torch.int32)
                shared = random_g_idx(K)
                for m in (layer.self_attn.q_proj, layer.self_attn.k_proj, layer.self_attn.v_proj, layer.mlp.gate_proj, layer.mlp.up_proj):
                    m.g_idx.copy_(shared)
                layer.self_attn.o_proj.g_idx.copy_(random_g_idx(layer.self_attn.o_proj.infeatures))
                layer.mlp.down_proj.g_idx.copy_(random_g_idx(layer.mlp.down_proj.infeatures))
        for name, p in model.named_parameters():
            if p.dim() == 1:
                p.fill_(1.0)                                  # RMSNorm weights
            else:
                p.copy_((torch.randn(p.shape, device=dev, generator=gen) * 0.02).to(p.dtype))
    model.model.rotary_emb = LlamaRotaryEmbedding(config, device=dev)
    if fused:
        fused_attn.make_quant_attn(model)
        triton_norm.make_quant_norm(model)
        fused_mlp.make_fused_mlp(model)
    model.seqlen = 2048     # reference sets this on the model (llama.py:23)
    return model


def benchmark_decode(model, tokens=64, seed=0, engine_hook=True):
    """llama.py:385-438: feed ``input_ids[:, i:i+1]`` with the growing cache, sync after every
    step, report the median (and peak memory).  Returns a dict.  engine_hook=False switches the transparent
    decode engine of quant/engine_hook.py off for this run (the module chain launch by launch)."""
    from transformers.cache_utils import DynamicCache
    model._gptq_engine_disabled = not engine_hook

    dev = next(model.parameters()).device
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    vocab = model.config.vocab_size
    input_ids = torch.randint(0, vocab, (1, tokens), device=dev, generator=gen)
    cache = DynamicCache(config=model.config)
    times = []
    torch.cuda.reset_peak_memory_stats(dev)
    with torch.no_grad():
        for i in range(tokens):
            torch.cuda.synchronize(dev)
            tick = time.perf_counter()
            out = model(input_ids[:, i:i + 1], past_key_values=cache, use_cache=True)
            torch.cuda.synchronize(dev)
            times.append(time.perf_counter() - tick)
            del out
    model._gptq_engine_disabled = False
    med = float(np.median(times[2:])) if len(times) > 4 else float(np.median(times))
    return {'protocol': 'llama.py:385-438 (one token per step, KV cache, sync per step, median)',
            'mode': 'model(input_ids[:, i:i+1], past_key_values=cache) on the drop-in modules, ' +
                    ('decode engine hook (quant/engine_hook.py)' if engine_hook else 'eager module chain'),
            'tokens': tokens, 'median_s_per_token': round(med, 6), 'tokens_per_s': round(1.0 / med, 1),
            'max_memory_MiB': round(torch.cuda.max_memory_allocated(dev) / 1024 / 1024, 1)}


def benchmark_generate(model, prompt_len=16, new_tokens=128, seed=0, batch=1, left_pad=False):
    """``model.generate(input_ids, do_sample=False, max_new_tokens=...)`` as llama_inference.py:119-127 calls it (greedy here
    so that runs are comparable), wall time of the decode part: (t(new_tokens) - t(1 new token)) / (new_tokens - 1).
    batch > 1: that many prompts at once; left_pad: rows of different lengths, left-padded with an attention mask (what a tokenizer
    with padding_side='left' hands to generate); tokens_per_s is the aggregate over the rows."""
    dev = next(model.parameters()).device
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    ids = torch.randint(1, model.config.vocab_size, (batch, prompt_len), device=dev, generator=gen)
    mask = torch.ones_like(ids)
    if left_pad:
        for b in range(batch):
            n = (3 * b + 2) % max(prompt_len - 1, 1) if b < batch - 1 or batch == 1 else 0
            ids[b, :n] = 0
            mask[b, :n] = 0

    def run(n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        with torch.no_grad():
            out = model.generate(ids, attention_mask=mask, do_sample=False, max_new_tokens=n, min_new_tokens=n, pad_token_id=0)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out
    run(4)                                   # warm-up: engine build + graph capture happen here
    t1, _ = run(1)
    tn, out = run(new_tokens)
    per_step = (tn - t1) / (new_tokens - 1)
    from .engine_hook import engine_steps
    return {'call': 'model.generate(input_ids[%d, %d]%s, do_sample=False, max_new_tokens=%d) (llama_inference.py:119-127)' % (
                batch, prompt_len, ', left-padded attention_mask' if left_pad else '', new_tokens),
            'generated': int(out.shape[1] - prompt_len), 's_per_token': round(per_step / batch, 6), 's_per_step': round(per_step, 6),
            'tokens_per_s': round(batch / per_step, 1), 'engine_steps_total': engine_steps(model)}


# ----------------------------------------------------------------------------------------------
# Graph-captured decode engine: the same arithmetic as one HF decoder step
# through the drop-in modules, but issued as a flat list of C-ABI launches on static buffers --
# 10 launches per layer (RMSNorm, qkv GEMV, RoPE+KV append, attention x2, o_proj GEMV + residual,
# RMSNorm, fused gate/up, down GEMV + residual) -- so that ONE hipGraph replay is one token.
# The position lives in device memory and is advanced inside the graph.
# ----------------------------------------------------------------------------------------------
ROPE_TABLE = os.environ.get('GPTQ_ROPE_TABLE', '1') != '0'
# round 6: the batch-1 attention launch leaves its split records to o_proj's decode kernel (gptq_decode_attn_split_f16 + gptq_layer_decode_attn_f16)
# instead of merging them itself; 0: the self-merging launch of rounds 2-5 (A/B runs, and what every other configuration takes anyway)
ATTN_RECORDS = os.environ.get('GPTQ_ATTN_RECORDS', '1') != '0'
LM_HEAD_KERNEL = os.environ.get('GPTQ_LM_HEAD_KERNEL', '1') != '0'   # 0: final norm + torch.matmul (hipBLASLt) as in rounds 1-3 (A/B runs)


MAX_BATCH = 16         # rows of a decode batch one engine serves (the LM head kernel and the decode kernel's row groups end there)
MAX_CHUNK_ROWS = 128   # rows of a batched verify step (batch x batch_chunk): what gptq_layer_decode_f16 and the batched chunk attention take
MAX_PROCESS_EOS, MAX_PROCESS_BIAS, MAX_PROCESS_VOCAB = 8, 256, 131072      # GPTQ_LOGITS_PROCESS_MAX_EOS / _BIAS / _VOCAB
MAX_BEAMS = 16         # GPTQ_BEAM_MAX_BEAMS
MAX_CONSTRAIN_STATES, MAX_CONSTRAIN_CLASSES = 32767, 16384                 # GPTQ_CONSTRAIN_MAX_STATES / _CLASSES
BEAM_DEAD = -1e9
MAX_LOGPROBS, MAX_LOGPROBS_ROWS = 32, 128      # GPTQ_LOGPROBS_MAX_TOP, the rows of one gptq_logprobs_rows_f16 launch
# gptq_beam_select_f16's state block in 4-byte words (gptq_mi355x.h "beam search")
(BEAM_W_EOS, BEAM_W_MAX_NEW, BEAM_W_LP, BEAM_W_ES, BEAM_W_T_CAP, BEAM_W_BEAMS, BEAM_W_T, BEAM_W_OPEN, BEAM_W_DONE, BEAM_W_STATUS) = range(10)
BEAM_W_SCORE, BEAM_W_PARENT, BEAM_W_TOKEN, BEAM_W_POOL, BEAM_W_CAND, BEAM_W_REC, BEAM_W_TABLES = 16, 32, 48, 80, 160, 288, 1376


def lm_head_logits(eng, x, logits, s, h=None):
    """shared by DecodeEngine and TPDecodeEngine: logits[B, rows] = lm_head(rmsnorm(x[B, hidden])) (+ lm_head.bias).  The hand-written
    launch needs an fp16 [rows, hidden] weight with unit column stride whose shape matches the logits buffer (a resized head would write
    past it: ADVICE r4) -- anything else, or GPTQ_LM_HEAD_KERNEL=0, takes the stand-alone norm + torch.matmul.
    h: the [B, hidden] scratch of the stand-alone norm (default eng.h)."""
    h = eng.h if h is None else h
    W = eng.lm_head
    bias = getattr(eng, 'lm_head_bias', None)
    B = x.shape[0]
    ok = (LM_HEAD_KERNEL and W.dtype == torch.float16 and W.dim() == 2 and W.stride(1) == 1 and W.stride(0) % 8 == 0 and W.shape[1] % 8 == 0 and
          W.shape[1] == x.shape[1] and W.shape[0] == logits.shape[-1] and B <= MAX_BATCH and (bias is None or bias.dtype == torch.float16))
    if ok:
        nw = eng.final_norm if eng.fuse_norm else None
        if nw is None:
            eng._norm_rows(x, eng.final_norm, h, s)
        src = x if nw is not None else h
        rc = eng.lib.gptq_dense_matmat_f16(src.data_ptr(), src.stride(0), W.data_ptr(), W.stride(0), eng.native.ptr(bias), logits.data_ptr(),
                                           logits.stride(0), B, W.shape[0], W.shape[1], eng.native.ptr(nw), eng.eps, s)
        if rc != -6:
            eng.native.check(rc, 'gptq_dense_matmat_f16')
            return
    eng._norm_rows(x, eng.final_norm, h, s)
    if bias is not None:
        torch.addmm(bias, h, W.t(), out=logits)
    else:
        torch.matmul(h, W.t(), out=logits)


class DecodeEngine:

    def __init__(self, model, t_max=2048, fuse_norm=True, fuse_attn=True, batch=1, chunk=0, batch_chunk=0, spec_sample=False, logits_process=False, beam_search=False,
                 logprobs=None, constrain=None, kv_cache='fp16'):
        """kv_cache = 'fp8' keeps the K/V cache in the FP8 format of gptq_mi355x.h "fp8 KV cache": k8b / v8b uint8 [layers, B, t_max, H] (OCP
        e4m3fn bytes) with kexpb / vexpb int8 [layers, B, t_max, heads] (one power-of-two exponent per token and head) -- half the bytes a decode
        step streams at depth, half the memory; kcb / vcb do not exist.  Every batch size, 1 included, steps through _step_rows with
        gptq_decode_attn_batch_kv8_f16, which rotates, quantises, attends to and appends the new token in one launch; the batch-1 route whose
        attention records are merged by o_proj's kernel is not built for fp8 (profiles/kv_fp8/README.md has what that costs at short context).
        prefill / prefill_batch run the fp16 prompt attention on ONE layer's worth of fp16 staging (kst / vst [B, t_max, H]) -- the prompt
        attends to its unquantised rows -- and gptq_kv8_store_f16 converts the rows they appended, layer by layer.  Everything behind the logits
        (greedy, sampling, processors, log-probabilities, constraints, every capture helper) is unchanged.  ValueError('... not built yet')
        before anything is allocated: together with chunk, batch_chunk, beam_search or fuse_attn=False; and, before anything changes, from
        prefill / prefill_batch with a start other than 0 or a prompt that needs more than one max_rows pass, and from score / score_batch.
        'fp16' (the default) allocates and launches exactly what it always did.
        constrain = True (dict(states=4096, classes=1024)) or a dict of those two capacities adds CONSTRAINED DECODING for regular languages
        (gptq_constrain_rows_f16, gptq_mi355x.h "constrained decoding"; quant/constrain.py builds the automata): c_next int16 [states, classes]
        filled with -1, c_cls int16 [B, vocab] -- one class-map slot per row --, c_map int32 [B], c_state int32 [B], all -1 (unconstrained).  One
        more launch per step, directly behind the processors' and ahead of the draw: it advances every row's state by the token the step
        consumed and sets the logits of the tokens the new state bans to -inf (set_constraint, reset_constraint, constrain_logits).  Every
        pointer and capacity is fixed here: a captured graph serves any automaton set later.  None (the default) allocates nothing and adds no
        launch.  ValueError together with chunk, batch_chunk or beam_search: constraints under speculation (a verify step has R rows per
        sequence and needs the state chain per row) and for beams are not built yet.
        logprobs = K (0 .. 32) makes every self-feeding step (capture_greedy_rows, capture_sample_native, capture_sample_rows) RECORD the
        log-probability of the token it chose, that token's rank and the row's K most probable tokens (gptq_logprobs_rows_f16, gptq_mi355x.h
        "token log-probabilities": one more launch per step, no host round trip): lp_chosen float [t_max + 1, B], lp_rank int32 [t_max + 1, B],
        lp_top_ids int32 / lp_top float [t_max + 1, B, K]; row n belongs to row n of stream_rows.  The logits are the ones the draw sees:
        behind the logit processors when logits_process is on, BEFORE temperature / top-k / top-p -- the model's distribution, not the
        warped one.  The batch-1 capture_greedy graph records nothing.  None (the default) allocates nothing and adds no launch.  ValueError
        for K outside 0 .. 32 and together with chunk, batch_chunk or beam_search (not built yet).  token_logprobs() is the eager entry.
        beam_search = True (with batch = N, 2 .. 16) makes the N rows the running beams of ONE beam search (HF's rule: gptq_mi355x.h "beam
        search"): the state block of gptq_beam_select_f16 -- set_beam_search, beam_select, beam_begin, capture_beam_step, beam_result,
        engine_generate_beam.  False (the default) allocates nothing and those calls raise.  ValueError together with logits_process, chunk or
        batch_chunk.
        logits_process = True adds the LOGIT PROCESSORS (gptq_logits_process_f16: repetition / presence penalty, logit bias, the
        min-new-tokens EOS mask) to every step: hist int32 [B, t_max] -- hist[b, p] = the token row b consumed at position p, kept by the prompt
        calls and by the process launch itself --, gen_start int64 [B], rep_penalty / presence_penalty float [B], min_new int32 [B], eos_ids
        int32 [8], bias_ids / bias_vals [256] with their counts on the host (set_logits_process, set_history, process_logits).  decode(token)
        and every self-feeding step then return / draw from PROCESSED logits.  False (the default) allocates nothing and changes no step.
        ValueError together with chunk / batch_chunk: processors under speculation are not built yet (the kernel takes R > 1 rows already).
        chunk = R or batch_chunk = R (2 .. 16) adds the VERIFY step of speculative decoding: R consecutive tokens of each of the B = batch
        sequences -- the last accepted token and R - 1 drafts -- go through every layer at M = B R in one pass over the weights; attention by
        gptq_decode_attn_chunk_batch_f16 -- two launches for all sequences -- on every sequence's own cache slice and position.  It is ONE
        mechanism (_chunk_buffers, _step_chunk, _verify_greedy_step, one graph) with two entry points that differ in the shapes they show:
        chunk = R needs batch 1: verify / accept / capture_verify_greedy / verify_sample, engine_generate(speculate=...); chunk_ids [R] and
        verify_out [R + 1] are row 0 of the [1, .] buffers.
        batch_chunk = R needs batch B >= 2 with B R <= 128: verify_batch / accept_batch / capture_verify_greedy_batch,
        engine_generate_batch(speculate=...); chunk_ids [B, R], verify_out [B, R + 1].
        0 for both (the default) allocates nothing and changes nothing; NotImplementedError when a layer has no decode route for B R rows.
        spec_sample = True (with batch_chunk = R) adds speculative SAMPLING for the B sequences: the [B R] settings and uniforms, the draft
        logits rows and the workspace of gptq_spec_sample_batch_f16 -- verify_sample_batch / capture_verify_sample_batch,
        engine_generate_batch(speculate=dict(sample=..., draft_model=...)).  A chunk engine always has them (its B = 1 case); a batch_chunk
        engine without the flag allocates nothing of it and refuses those calls.  ValueError without chunk rows.
        batch (round 5): rows of a decode BATCH -- B sequences advance by one token per step, every row with its own position and its
        own slice of the K/V cache (the reference's one kernel serves any batch, quant_linear.py:263-269; HF generate drives it with
        [B, 1] steps).  The linears run at M = B through gptq_layer_decode_f16 (norm and residual inside the decode kernel's launch up to
        four rows, 16-row MFMA tiles above), attention through gptq_decode_attn_batch_f16, the LM head through gptq_dense_matmat_f16:
        still ONE hipGraph replay per step."""
        from . import _native
        # act-order layers fed by one of the engine's own launches (o_proj <- attention, down_proj <- gate/up + SiLU) get their input written in THEIR
        # sorted order by the producer (round 5) and run the trivial kernel; GPTQ_PRODUCER_PERM=0: the in-kernel gather of round 3 / 4 (A/B)
        self.producer_perm = os.environ.get('GPTQ_PRODUCER_PERM', '1') != '0'
        self.batch = int(batch)
        if not 1 <= self.batch <= MAX_BATCH:
            raise NotImplementedError('DecodeEngine: batch must be 1 .. %d' % MAX_BATCH)
        self.chunk = int(chunk)
        if self.chunk != 0 and (not 2 <= self.chunk <= MAX_BATCH or self.batch != 1):
            raise ValueError('DecodeEngine: chunk must be 0 or 2 .. %d, and needs batch 1' % MAX_BATCH)
        self.batch_chunk = int(batch_chunk)
        if self.batch_chunk != 0 and (self.batch < 2 or not 2 <= self.batch_chunk <= MAX_BATCH or self.batch * self.batch_chunk > MAX_CHUNK_ROWS):
            raise ValueError('DecodeEngine: batch_chunk must be 0 or 2 .. %d, and needs batch >= 2 with batch x batch_chunk <= %d' % (
                MAX_BATCH, MAX_CHUNK_ROWS))
        if spec_sample and not (self.chunk or self.batch_chunk):
            raise ValueError('DecodeEngine: spec_sample needs batch_chunk = R (a chunk engine always samples speculatively)')
        self.spec_sample = bool(spec_sample or self.chunk)
        self.logits_process = bool(logits_process)
        if self.logits_process and (self.chunk or self.batch_chunk):
            raise ValueError('DecodeEngine: logits_process together with chunk / batch_chunk is not built yet (processors under speculation)')
        self.beam_search = bool(beam_search)
        if self.beam_search and (self.logits_process or self.chunk or self.batch_chunk or not 2 <= self.batch <= MAX_BEAMS):
            raise ValueError('DecodeEngine: beam_search needs batch = 2 .. %d beams and combines with neither logits_process, chunk nor batch_chunk'
                             % MAX_BEAMS)
        if logprobs is not None:
            if isinstance(logprobs, bool) or not isinstance(logprobs, int) or not 0 <= logprobs <= MAX_LOGPROBS:
                raise ValueError('DecodeEngine: logprobs must be None or an int in 0 .. %d, not %r' % (MAX_LOGPROBS, logprobs))
            if self.chunk or self.batch_chunk or self.beam_search:
                raise ValueError('DecodeEngine: logprobs together with chunk / batch_chunk / beam_search is not built yet (records of a verify '
                                 'step, of a beam)')
        self.logprobs = logprobs
        if constrain is None or constrain is False:
            self.constrain = None
        else:
            cap = dict(states=4096, classes=1024)
            if constrain is not True:
                if not isinstance(constrain, dict) or set(constrain) - set(cap):
                    raise ValueError('DecodeEngine: constrain must be None, True or a dict with the keys states, classes, not %r' % (constrain,))
                cap.update(constrain)
            for k, most in (('states', MAX_CONSTRAIN_STATES), ('classes', MAX_CONSTRAIN_CLASSES)):
                if isinstance(cap[k], bool) or not isinstance(cap[k], int) or not 1 <= cap[k] <= most:
                    raise ValueError('DecodeEngine: constrain %s must be an int in 1 .. %d, not %r' % (k, most, cap[k]))
            if self.chunk or self.batch_chunk or self.beam_search:
                raise ValueError('DecodeEngine: constrain together with chunk / batch_chunk / beam_search is not built yet (the state chain of a '
                                 'verify step, of a beam)')
            self.constrain = cap
        self.fuse_norm, self.fuse_attn = bool(fuse_norm), bool(fuse_attn)
        if kv_cache not in ('fp16', 'fp8'):
            raise ValueError("DecodeEngine: kv_cache must be 'fp16' or 'fp8', not %r" % (kv_cache,))
        self.kv_cache = kv_cache
        if kv_cache == 'fp8' and (self.chunk or self.batch_chunk or self.beam_search or not self.fuse_attn):
            raise ValueError("DecodeEngine: kv_cache='fp8' together with chunk / batch_chunk / beam_search / fuse_attn=False is not built yet (the "
                             "fp8 cache has the fused decode attention and the prompt store, nothing else)")
        self.native = _native
        self.lib = _native.lib()
        self.model = model
        cfg = model.config
        dev = next(model.parameters()).device
        self.dev = dev
        self.t_max = int(t_max)
        self.hidden = cfg.hidden_size
        self.heads = cfg.num_attention_heads
        self.head_dim = self.hidden // self.heads
        self.scale = 1.0 / float(np.sqrt(self.head_dim))
        self.eps = float(cfg.rms_norm_eps)
        if self.head_dim != 128:
            raise NotImplementedError('DecodeEngine: head_dim must be 128')
        self.embed = model.model.embed_tokens.weight
        self.lm_head = model.lm_head.weight
        self.lm_head_bias = getattr(model.lm_head, 'bias', None)
        self.final_norm = model.model.norm.weight
        self.layers = []
        for layer in model.model.layers:
            attn, mlp = layer.self_attn, layer.mlp
            if not isinstance(attn, fused_attn.QuantLlamaAttention) or not isinstance(mlp, fused_mlp.QuantLlamaMLP):
                raise RuntimeError('DecodeEngine needs make_quant_attn / make_fused_mlp applied first')
            gpack, upack = self._pack_pair(mlp)
            self.layers.append(dict(
                ln1=layer.input_layernorm.weight, ln2=layer.post_attention_layernorm.weight,
                qkv=self._pack(attn.qkv_proj), o=self._pack(attn.o_proj), down=self._pack(mlp.down_proj),
                gate=gpack, up=upack, theta=float(attn.rope_theta)))
        H, I, B = self.hidden, cfg.intermediate_size, self.batch
        f16 = dict(dtype=torch.float16, device=dev)
        self.ids = torch.zeros(B, dtype=torch.int64, device=dev)
        self.pos = torch.zeros(B, dtype=torch.int64, device=dev)       # per row: tokens consumed so far = the position of the next one
        self.x = torch.zeros((B, H), **f16)
        self.x2 = torch.zeros((B, H), **f16)
        self.h = torch.zeros((B, H), **f16)
        self.qkvb = torch.zeros((B, 3 * H), **f16)
        self.ab = torch.zeros((B, H), **f16)
        self.cb = torch.zeros((B, I), **f16)
        # sized from the head itself (a resized / padded lm_head has rows != config.vocab_size: ADVICE r4)
        self.logits = torch.zeros((B, self.lm_head.shape[0]), **f16)
        self.stream_out = torch.zeros(self.t_max + 1, dtype=torch.int64, device=dev)   # greedy mode (batch 1): token chosen after position p
        self.greedy_graph = None
        self.greedy_rows_graph, self.stream_rows, self.stepc, self.sample_graphs = None, None, None, {}
        self.lp_chosen, self.lp_rank, self.lp_top_ids, self.lp_top = None, None, None, None      # with logprobs: allocated next to stream_rows
        if self.logprobs is not None and self.logits.shape[1] < max(self.logprobs, 1):
            raise ValueError('DecodeEngine: logprobs = %d needs a vocabulary of at least that many tokens' % self.logprobs)
        # gptq_sample_rows_f16: the uniforms and every row's (temperature, top_k, top_p), read by the kernel at every replay (set_sampling)
        self.u = torch.zeros(B, dtype=torch.float32, device=dev)
        self.temperature = torch.ones(B, dtype=torch.float32, device=dev)
        self.top_k = torch.zeros(B, dtype=torch.int32, device=dev)
        self.top_p = torch.ones(B, dtype=torch.float32, device=dev)
        self.sample_native_graph = None
        if self.logits_process:
            # gptq_logits_process_f16: the rows' token history and settings, read by the kernel at every replay (set_logits_process)
            if self.logits.shape[1] > MAX_PROCESS_VOCAB:
                raise NotImplementedError('DecodeEngine: logits_process takes vocabularies up to %d' % MAX_PROCESS_VOCAB)
            self.hist = torch.zeros((B, self.t_max), dtype=torch.int32, device=dev)
            self.gen_start = torch.zeros(B, dtype=torch.int64, device=dev)
            self.rep_penalty = torch.ones(B, dtype=torch.float32, device=dev)
            self.presence_penalty = torch.zeros(B, dtype=torch.float32, device=dev)
            self.min_new = torch.zeros(B, dtype=torch.int32, device=dev)
            self.eos_ids = torch.zeros(MAX_PROCESS_EOS, dtype=torch.int32, device=dev)
            self.bias_ids = torch.zeros(MAX_PROCESS_BIAS, dtype=torch.int32, device=dev)
            self.bias_vals = torch.zeros(MAX_PROCESS_BIAS, dtype=torch.float32, device=dev)
            self.n_eos, self.n_bias = 0, 0                  # launch arguments: a captured step holds the counts it was captured with
        if self.constrain is not None:
            # gptq_constrain_rows_f16: the stacked automata, every row's class map and state, read by the kernel at every replay (set_constraint)
            self.c_next = torch.full((self.constrain['states'], self.constrain['classes']), -1, dtype=torch.int16, device=dev)
            self.c_cls = torch.zeros((B, self.logits.shape[1]), dtype=torch.int16, device=dev)
            self.c_map = torch.arange(B, dtype=torch.int32, device=dev)
            self.c_state = torch.full((B,), -1, dtype=torch.int32, device=dev)
            self._c_dfas, self._c_start = [None] * B, [-1] * B       # the rows' automata and start states, as set_constraint left them
        nl = len(self.layers)
        if self.kv_cache == 'fp8':
            u8, i8 = dict(dtype=torch.uint8, device=dev), dict(dtype=torch.int8, device=dev)
            self.k8b, self.v8b = torch.zeros((nl, B, self.t_max, H), **u8), torch.zeros((nl, B, self.t_max, H), **u8)      # e4m3fn bytes
            self.kexpb, self.vexpb = torch.zeros((nl, B, self.t_max, self.heads), **i8), torch.zeros((nl, B, self.t_max, self.heads), **i8)
            self.kst, self.vst = torch.zeros((B, self.t_max, H), **f16), torch.zeros((B, self.t_max, H), **f16)          # ONE layer of fp16 staging
        else:
            self.kcb = torch.zeros((nl, B, self.t_max, H), **f16)          # [layer][row][t][heads * head_dim]
            self.vcb = torch.zeros((nl, B, self.t_max, H), **f16)
            self.kc, self.vc = self.kcb[:, 0], self.vcb[:, 0]              # row 0 = THE cache of a batch-1 engine ([layer][t][H] views)
        self.attn_ws = torch.zeros(self.lib.gptq_decode_attn_batch_workspace_bytes(B, self.heads, self.head_dim, self.t_max),
                                   dtype=torch.uint8, device=dev)
        self.ws = _native.workspace(dev)
        self.graph = None
        self.beam_graph = None
        if self.beam_search:
            # gptq_beam_select_f16's ONE state block (int32 words, gptq_mi355x.h): settings, scores, the step's parents and tokens, the pool, the
            # back-pointer tables of t_max steps
            if self.logits.shape[1] < 2 * B:
                raise ValueError('DecodeEngine: beam_search with %d beams needs a vocabulary of at least %d' % (B, 2 * B))
            nbytes = self.lib.gptq_beam_state_bytes(B, self.t_max)
            if nbytes != 4 * (BEAM_W_TABLES + 2 * self.t_max * B):
                raise RuntimeError('DecodeEngine: the library lays the beam state block out differently from BEAM_W_* (%d bytes)' % nbytes)
            self.beam_state = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)
            self.beam_parent = self.beam_state[BEAM_W_PARENT:BEAM_W_PARENT + B]
            self.beam_token = self.beam_state[BEAM_W_TOKEN:BEAM_W_TOKEN + 2 * B].view(torch.int64)
            self.set_beam_search(self.t_max)
        self.scratch = None
        self._rope_tabs, self._prefill_bufs, self._nll_ws = {}, None, None      # filled on first use: _rope_table, _prefill_buffers, _nll_rows
        # batch 1: the attention's splits are merged by o_proj's decode kernel when every o_proj can (trivial g_idx, an image, no bias next to the residual)
        self.attn_records = bool(ATTN_RECORDS and self.fuse_attn and B == 1 and self.kv_cache == 'fp16' and all(
            L['o']['st'] is not None and L['o']['bias'] is None and
            self.lib.gptq_layer_decode_attn_supported(L['o']['_keep'].handle, 1, self.heads, self.head_dim) == 1 for L in self.layers))
        if B > 1 or self.kv_cache == 'fp8':                        # (an fp8 engine steps through _step_rows at every batch size)
            self.scratch = self._rows_scratch('batch', (B,))
        self.verify_graph, self.verify_sample_graphs, self.spec_stats = None, {}, None
        self.draft_graph, self._draft_engine = None, None          # capture_draft_step (a draft engine) / (draft model, its engine) of a target engine
        self.chunk_rows = self.chunk or self.batch_chunk           # R of the verify step, whichever argument asked for it (0: none)
        if self.chunk_rows:
            self._chunk_buffers()

    verify_batch_graph = property(lambda self: self.verify_graph, doc='the ONE verify-greedy graph under the name capture_verify_greedy_batch stores it')

    # -- weights: the engine reads the SAME derived copy as the modules -------------------------------------------------------
    # Every linear is taken from quant/layer.py prepared() with exactly the arguments the module's own forward uses, so the eager
    # path (prefill, anything the hook declines) and the engine share ONE PreparedLayer: one stripe16 image per layer next to the
    # checkpoint buffers -- not the three or four copies of round 3 (module image + the engine's own stripe_copy of every linear +
    # single-set images of gate and up next to the pair's).
    def _from_prepared(self, pl, qweight, scales, qzeros, g_idx, bits, gs, K, N, bias):
        gi = None
        if pl.kind != 0 and g_idx is not None and qweight is not None:
            gi = quant_linear._int32c(g_idx[:K])
        st = pl.stripe
        srt = None
        if st is None and gi is not None and bits in (2, 4, 8):      # no image (GPTQ_STRIPE=0, odd shapes): the sorted-copy kernels
            srt = quant_linear.act_order_sorted(quant_linear._int32c(qweight), gi, K, gs, bits)
        released = qweight is None or qweight.shape[0] == 0
        return dict(qw=None if released else quant_linear._int32c(qweight), sc=None if released else scales,
                    qz=None if released else quant_linear._int32c(qzeros), gi=gi, bits=bits, gs=gs, K=K, N=N, bias=bias, srt=srt, st=st,
                    perm=pl.perm16 if st is not None else None, invperm=pl.invperm32 if st is not None else None, _keep=pl)

    def _pack_raw(self, qweight, scales, qzeros, g_idx, bits, groupsize, K, N, bias=None):
        from .layer import prepared
        gs = groupsize if groupsize != -1 else K
        pl = prepared(((qweight, scales, qzeros, g_idx),), bias, bits, gs, K, N, sort=quant_linear.ACT_ORDER_SORT)
        return self._from_prepared(pl, qweight, scales, qzeros, g_idx, bits, gs, K, N, bias)

    def _pack(self, ql):
        if getattr(ql, '_released', None) is not None:   # memory mode: the PreparedLayer's image is all there is -- and all the decode kernels need
            return self._from_prepared(ql._released, None, None, None, None, ql.bits, ql.groupsize, ql.infeatures, ql.outfeatures, ql.bias)
        return self._pack_raw(ql.qweight, ql.scales, ql.qzeros, ql.g_idx, ql.bits, ql.groupsize, ql.infeatures, ql.outfeatures, ql.bias)

    def _pack_pair(self, mlp):
        """gate and up of a QuantLlamaMLP: ONE PreparedLayer of the pair (the one mlp.hip_llama_mlp uses) -- its image holds both sets,
        of the group-sorted rows when the two share an act-order permutation."""
        from .layer import prepared
        K, N, bits = mlp.infeatures, mlp.intermediate_size, mlp.bits
        gs = mlp.groupsize if mlp.groupsize != -1 else K
        if getattr(mlp, '_released', None) is not None:
            pl = mlp._released
            g = self._from_prepared(pl, None, None, None, None, bits, gs, K, N, None)
            u = dict(g)
        else:
            gate = (mlp.gate_proj_qweight, mlp.gate_proj_scales, mlp.gate_proj_qzeros, mlp.gate_proj_g_idx)
            up = (mlp.up_proj_qweight, mlp.up_proj_scales, mlp.up_proj_qzeros, mlp.up_proj_g_idx)
            pl = prepared((gate, up), None, bits, gs, K, N, sort=quant_linear.ACT_ORDER_SORT)
            g = self._from_prepared(pl, *gate, bits, gs, K, N, None)
            u = self._from_prepared(pl, *up, bits, gs, K, N, None)
        g['st2'], g['perm2'] = pl.stripe, (pl.perm16 if pl.stripe is not None else None)
        g['st'] = u['st'] = None          # the pair's image is not a single-set image
        g['perm'] = u['perm'] = None
        g['pair_sorted'] = False
        if g['st2'] is None and g['gi'] is not None and u['gi'] is not None and bits in (2, 4, 8):
            # no image: gate and up share their input, hence (normally) their act-order permutation -- checked ONCE here
            for w in (g, u):
                w['srt'] = quant_linear.act_order_sorted(w['qw'], w['gi'], K, gs, bits)
            g['pair_sorted'] = g['srt'] is not None and u['srt'] is not None and bool(torch.equal(g['srt'][1], u['srt'][1]))
        return g, u

    def _rows_scratch(self, what, rows):
        """the scratch of gptq_layer_decode_f16 for every row count in `rows`; NotImplementedError unless every layer has a stripe16 route for
        rows[0] (what: 'batch' or 'chunk', for the message)"""
        M, need = rows[0], 256
        for L in self.layers:
            for w in (L['qkv'], L['o'], L['gate'], L['down']):
                pl = w['_keep']
                route = self.lib.gptq_layer_route_for(pl.handle, M)
                if route not in (1, 2) and not (pl.kind == 1 and route > 0):     # stripe decode kernel / 16-row tiles on the image
                    raise NotImplementedError('DecodeEngine(%s=%d): a layer has no stripe16 route for %d rows (route %d)' % (what, M, M, route))
                need = max([need] + [self.lib.gptq_layer_decode_scratch_bytes(pl.handle, m) for m in rows])
        return torch.empty(need, dtype=torch.uint8, device=self.dev)

    # -- launches ------------------------------------------------------------------------------
    def _gemv(self, x, w, y, s, residual=None, x_sorted=False):
        """x_sorted: x was written in this layer's group-sorted order by its producer -- no gather (the image IS the sorted rows)"""
        if w['bias'] is not None and residual is not None:
            # one add slot per launch: the bias rides in the matvec, the residual is a second launch (gptq_layer_decode_f16 does both)
            if self.scratch is None:
                self.scratch = torch.empty(max(256, self.lib.gptq_layer_decode_scratch_bytes(w['_keep'].handle, 1)), dtype=torch.uint8, device=self.dev)
            return self._lin(w, x, y, s, self.native.layer_workspace(self.dev, s), residual=residual)
        b = residual if residual is not None else w['bias']
        ptr = self.native.ptr
        if w['st'] is not None:       # stripe16: no K split, no workspace (act-order: x gathered through perm in the kernel)
            quant_linear.stripe_matvec(x, w['st'], y, w['K'], w['N'], w['bits'], w['gs'], bias=b, perm=None if x_sorted else w['perm'])
            return
        if w['srt'] is not None:      # act-order layer: group-sorted copy + fused x gather
            qs, perm = w['srt']
            rc = self.lib.gptq_matmul248_sorted_f16(x.data_ptr(), w['K'], perm.data_ptr(), qs.data_ptr(), w['sc'].data_ptr(),
                                                    w['qz'].data_ptr(), ptr(b), y.data_ptr(), w['N'], 1, w['K'], w['N'], w['bits'],
                                                    w['gs'], self.ws.data_ptr(), self.ws.numel(), s)
            self.native.check(rc, 'gptq_matmul248_sorted_f16')
            return
        rc = self.lib.gptq_matmul248_f16(x.data_ptr(), w['K'], w['qw'].data_ptr(), w['sc'].data_ptr(), w['qz'].data_ptr(), ptr(w['gi']),
                                         ptr(b), y.data_ptr(), w['N'], 1, w['K'], w['N'], w['bits'], w['gs'], self.ws.data_ptr(),
                                         self.ws.numel(), s)
        self.native.check(rc, 'gptq_matmul248_f16')

    def _norm_rows(self, x, w, y, s):
        rc = self.lib.gptq_rmsnorm_f16(x.data_ptr(), x.stride(0), w.data_ptr(), y.data_ptr(), y.stride(0), x.shape[0], self.hidden, self.eps, s)
        self.native.check(rc, 'gptq_rmsnorm_f16')

    def _norm_gemv(self, x, nw, w, y, s):
        """y = QuantLinear(rmsnorm(x)): one launch when the fused kernel serves the shape, else two."""
        ptr = self.native.ptr
        if self.fuse_norm and w['st'] is not None:      # RMSNorm fused into the staging of x (every workgroup sees all of x)
            quant_linear.stripe_matvec(x, w['st'], y, w['K'], w['N'], w['bits'], w['gs'], bias=w['bias'], norm_weight=nw, eps=self.eps, perm=w['perm'])
            return
        if self.fuse_norm and w['bias'] is None and w['srt'] is not None:      # act-order: norm + gather + GEMV in one launch
            qs, perm = w['srt']
            rc = self.lib.gptq_rmsnorm_sorted_f16(x.data_ptr(), nw.data_ptr(), self.eps, perm.data_ptr(), qs.data_ptr(), w['sc'].data_ptr(),
                                                  w['qz'].data_ptr(), None, None, None, None, y.data_ptr(), w['K'], w['N'], w['bits'],
                                                  w['gs'], self.ws.data_ptr(), self.ws.numel(), s)
            if rc != -6:
                self.native.check(rc, 'gptq_rmsnorm_sorted_f16')
                return
        if self.fuse_norm and w['bias'] is None and w['srt'] is None:
            rc = self.lib.gptq_rmsnorm_matmul248_f16(x.data_ptr(), nw.data_ptr(), self.eps, w['qw'].data_ptr(), w['sc'].data_ptr(),
                                                     w['qz'].data_ptr(), ptr(w['gi']), None, y.data_ptr(), w['K'], w['N'], w['bits'],
                                                     w['gs'], self.ws.data_ptr(), self.ws.numel(), s)
            if rc != -6:   # GPTQ_E_VARIANT: shape needs the generic kernels
                self.native.check(rc, 'gptq_rmsnorm_matmul248_f16')
                return
        self._norm_rows(x, nw, self.h, s)
        self._gemv(self.h, w, y, s)

    def _norm_mlp(self, x, nw, g, u, c, s, out_perm=None):
        """out_perm: store column n of silu(gate) * up at out_perm[n] (down_proj's sorted order); only the stripe16 pair kernel does that"""
        ptr = self.native.ptr
        if g.get('st2') is not None:
            perm = g['perm2']
            if self.fuse_norm:
                quant_linear.stripe_matvec(x, g['st2'], c, g['K'], g['N'], g['bits'], g['gs'], nsets=2, norm_weight=nw, eps=self.eps, perm=perm, out_perm=out_perm)
            else:
                self._norm_rows(x, nw, self.h, s)
                quant_linear.stripe_matvec(self.h, g['st2'], c, g['K'], g['N'], g['bits'], g['gs'], nsets=2, perm=perm, out_perm=out_perm)
            return
        assert out_perm is None
        if g.get('pair_sorted') and self.fuse_norm:
            rc = self.lib.gptq_rmsnorm_sorted_f16(x.data_ptr(), nw.data_ptr(), self.eps, g['srt'][1].data_ptr(), g['srt'][0].data_ptr(),
                                                  g['sc'].data_ptr(), g['qz'].data_ptr(), u['srt'][0].data_ptr(), u['sc'].data_ptr(),
                                                  u['qz'].data_ptr(), None, c.data_ptr(), g['K'], g['N'], g['bits'], g['gs'],
                                                  self.ws.data_ptr(), self.ws.numel(), s)
            if rc != -6:
                self.native.check(rc, 'gptq_rmsnorm_sorted_f16')
                return
        if g.get('pair_sorted'):
            # act-order MLP: gate and up share the permutation of their common input -> sorted fused kernel
            self._norm_rows(x, nw, self.h, s)
            rc = self.lib.gptq_fused_mlp_sorted_f16(self.h.data_ptr(), g['K'], g['srt'][1].data_ptr(), g['srt'][0].data_ptr(),
                                                    g['sc'].data_ptr(), g['qz'].data_ptr(), u['srt'][0].data_ptr(), u['sc'].data_ptr(),
                                                    u['qz'].data_ptr(), c.data_ptr(), g['N'], 1, g['K'], g['N'], g['bits'], g['gs'],
                                                    self.ws.data_ptr(), self.ws.numel(), s)
            if rc != -6:
                self.native.check(rc, 'gptq_fused_mlp_sorted_f16')
                return
        if self.fuse_norm:
            rc = self.lib.gptq_rmsnorm_fused_mlp_f16(x.data_ptr(), nw.data_ptr(), self.eps, g['qw'].data_ptr(), g['sc'].data_ptr(),
                                                     g['qz'].data_ptr(), ptr(g['gi']), u['qw'].data_ptr(), u['sc'].data_ptr(),
                                                     u['qz'].data_ptr(), ptr(u['gi']), c.data_ptr(), g['K'], g['N'], g['bits'], g['gs'],
                                                     self.ws.data_ptr(), self.ws.numel(), s)
            if rc != -6:
                self.native.check(rc, 'gptq_rmsnorm_fused_mlp_f16')
                return
        self._norm_rows(x, nw, self.h, s)
        rc = self.lib.gptq_fused_mlp_f16(self.h.data_ptr(), g['K'], g['qw'].data_ptr(), g['sc'].data_ptr(), g['qz'].data_ptr(), ptr(g['gi']),
                                         u['qw'].data_ptr(), u['sc'].data_ptr(), u['qz'].data_ptr(), ptr(u['gi']), c.data_ptr(), g['N'], 1,
                                         g['K'], g['N'], g['bits'], g['gs'], self.ws.data_ptr(), self.ws.numel(), s)
        self.native.check(rc, 'gptq_fused_mlp_f16')

    def _rope_table(self, theta, s):
        """{cos, sin}[t_max][head_dim / 2] fp32 per rope base (one for a LLaMA), filled once by the kernel that would otherwise
        evaluate them per token and head.  GPTQ_ROPE_TABLE=0: compute in the attention kernel (A/B runs)."""
        if not ROPE_TABLE:
            return None
        tabs = self._rope_tabs
        t = tabs.get(float(theta))
        if t is None:
            t = torch.empty((self.t_max, self.head_dim // 2, 2), dtype=torch.float32, device=self.dev)
            self.native.check(self.lib.gptq_rope_table_f32(t.data_ptr(), self.t_max, self.head_dim, float(theta), s), 'gptq_rope_table_f32')
            tabs[float(theta)] = t
        return t

    # -- a decode batch: every linear is ONE gptq_layer_decode_f16 (y = residual + layer(rmsnorm(x)), M = batch) ------------------------
    def _lin(self, w, x, y, s, lws, norm=None, residual=None):
        pl = w['_keep']
        ptr = self.native.ptr
        rc = self.lib.gptq_layer_decode_f16(pl.handle, x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), x.shape[0], ptr(norm), self.eps,
                                            ptr(residual), residual.stride(0) if residual is not None else 0, lws.data_ptr(), lws.numel(),
                                            self.scratch.data_ptr(), self.scratch.numel(), s)
        self.native.check(rc, 'gptq_layer_decode_f16')

    def _lin_next_norm(self, w, x, y, s, lws, residual, next_norm, h):
        """y = residual + layer(x) and, when the launch that combines this batch's K slices can do it for free, h = rmsnorm(y) * next_norm
        (gptq_layer_decode_next_norm_f16) -- returns whether h was written (decided on the host, per shape and batch: the same in every replay)"""
        import ctypes
        pl = w['_keep']
        done = ctypes.c_int(0)
        rc = self.lib.gptq_layer_decode_next_norm_f16(pl.handle, x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), x.shape[0], None, self.eps,
                                                      residual.data_ptr(), residual.stride(0), next_norm.data_ptr(), self.eps, h.data_ptr(), h.stride(0),
                                                      ctypes.byref(done), lws.data_ptr(), lws.numel(), self.scratch.data_ptr(), self.scratch.numel(), s)
        self.native.check(rc, 'gptq_layer_decode_next_norm_f16')
        return bool(done.value)

    def _step_rows(self, bufs, ids, attn, logits):
        """one decode step at M = len(ids) rows on the [M, .] activations `bufs` (x, x2, h, qkv, ab, cb): every linear is ONE _lin /
        _lin_next_norm launch, attention is the caller's attn(li, L, qkv, ab, tab, s), the LM head writes `logits`.  Does not advance pos."""
        s = self.native.stream_ptr(self.dev)
        lws = self.native.layer_workspace(self.dev, s)
        x, x2, h, qkvb, ab, cb = (bufs[k] for k in ('x', 'x2', 'h', 'qkv', 'ab', 'cb'))
        torch.index_select(self.embed, 0, ids, out=x)
        normed = False          # h holds rmsnorm(x) * ln1 of this block already (written by the previous block's down_proj: round 6)
        for li, L in enumerate(self.layers):
            if normed:
                self._lin(L['qkv'], h, qkvb, s, lws)
            elif self.fuse_norm:
                self._lin(L['qkv'], x, qkvb, s, lws, norm=L['ln1'])                             # qkv = qkv_proj(rmsnorm(x))
            else:
                self._norm_rows(x, L['ln1'], h, s)
                self._lin(L['qkv'], h, qkvb, s, lws)
            attn(li, L, qkvb, ab, self._rope_table(L['theta'], s), s)
            self._lin(L['o'], ab, x2, s, lws, residual=x)                                       # x2 = x + o_proj(attn)
            if self.fuse_norm:
                self._lin(L['gate'], x2, cb, s, lws, norm=L['ln2'])                             # c = silu(gate(h)) * up(h), h = rmsnorm(x2)
            else:
                self._norm_rows(x2, L['ln2'], h, s)
                self._lin(L['gate'], h, cb, s, lws)
            if self.fuse_norm and li + 1 < len(self.layers):                                    # x = x2 + down(c) (+ the next block's input norm)
                normed = self._lin_next_norm(L['down'], cb, x, s, lws, x2, self.layers[li + 1]['ln1'], h)
            else:
                self._lin(L['down'], cb, x, s, lws, residual=x2)
                normed = False
        lm_head_logits(self, x, logits, s, h)

    def _step_batch(self):
        """a decode batch: _step_rows at M = batch, gptq_decode_attn_batch_f16 on every row's own cache slice and position (an fp8 engine:
        gptq_decode_attn_batch_kv8_f16 on its bytes and exponents, at every batch size)"""
        def attn8(li, L, qkvb, ab, tab, s):
            rc = self.lib.gptq_decode_attn_batch_kv8_f16(qkvb.data_ptr(), qkvb.stride(0), self.pos.data_ptr(), self.k8b[li].data_ptr(),
                                                         self.v8b[li].data_ptr(), self.kexpb[li].data_ptr(), self.vexpb[li].data_ptr(),
                                                         ab.data_ptr(), ab.stride(0), self.attn_ws.data_ptr(), self.attn_ws.numel(), self.batch,
                                                         self.heads, self.head_dim, self.t_max, L['theta'], self.scale, self.native.ptr(tab), None,
                                                         0, s)
            self.native.check(rc, 'gptq_decode_attn_batch_kv8_f16')

        def attn(li, L, qkvb, ab, tab, s):
            rc = self.lib.gptq_decode_attn_batch_f16(qkvb.data_ptr(), qkvb.stride(0), self.pos.data_ptr(), self.kcb[li].data_ptr(),
                                                     self.vcb[li].data_ptr(), ab.data_ptr(), ab.stride(0), self.attn_ws.data_ptr(),
                                                     self.attn_ws.numel(), self.batch, self.heads, self.head_dim, self.t_max, L['theta'],
                                                     self.scale, self.native.ptr(tab), None, s)
            self.native.check(rc, 'gptq_decode_attn_batch_f16')
        self._step_rows(dict(x=self.x, x2=self.x2, h=self.h, qkv=self.qkvb, ab=self.ab, cb=self.cb), self.ids,
                        attn8 if self.kv_cache == 'fp8' else attn, self.logits)
        self.pos.add_(1)

    def _step(self):
        if self.batch > 1 or self.kv_cache == 'fp8':
            return self._step_batch()
        lib, ptr = self.lib, self.native.ptr
        s = torch.cuda.current_stream(self.dev).cuda_stream
        torch.index_select(self.embed, 0, self.ids, out=self.x)
        scale = self.scale
        for li, L in enumerate(self.layers):
            self._norm_gemv(self.x, L['ln1'], L['qkv'], self.qkvb, s)       # qkv = qkv_proj(rmsnorm(x))
            # producer-side permutation: o_proj / down_proj of an act-order checkpoint read x in their sorted order -- written that way by the attention /
            # gate-up launch when those are the stripe16 kernels (else: the in-kernel gather)
            # (a consumer with a bias AND a residual goes through gptq_layer_decode_f16, which gathers x itself: no producer-side order for it -- ADVICE r5)
            o_inv = L['o'].get('invperm') if (self.producer_perm and self.fuse_attn and L['o']['st'] is not None and L['o']['bias'] is None) else None
            d_inv = L['down'].get('invperm') if (self.producer_perm and L['gate'].get('st2') is not None and L['down']['st'] is not None and
                                                 L['down']['bias'] is None) else None
            if self.attn_records:
                tab = self._rope_table(L['theta'], s)
                rc = lib.gptq_decode_attn_split_f16(self.qkvb.data_ptr(), self.qkvb.stride(0), self.pos.data_ptr(), self.kc[li].data_ptr(),
                                                    self.vc[li].data_ptr(), self.attn_ws.data_ptr(), self.attn_ws.numel(), 1, self.heads, self.head_dim,
                                                    self.t_max, L['theta'], scale, ptr(tab), 0, s)
                self.native.check(rc, 'gptq_decode_attn_split_f16')
                rc = lib.gptq_layer_decode_attn_f16(L['o']['_keep'].handle, self.attn_ws.data_ptr(), self.attn_ws.numel(), self.pos.data_ptr(), 1,
                                                    self.heads, self.head_dim, self.t_max, 0, self.x2.data_ptr(), self.x2.stride(0), self.x.data_ptr(),
                                                    self.x.stride(0), s)                                   # x2 = x + o_proj(merge(records))
                self.native.check(rc, 'gptq_layer_decode_attn_f16')
            elif self.fuse_attn:
                tab = self._rope_table(L['theta'], s)
                if o_inv is not None:
                    rc = lib.gptq_decode_attn_batch_f16(self.qkvb.data_ptr(), self.qkvb.stride(0), self.pos.data_ptr(), self.kc[li].data_ptr(),
                                                        self.vc[li].data_ptr(), self.ab.data_ptr(), self.ab.stride(0), self.attn_ws.data_ptr(),
                                                        self.attn_ws.numel(), 1, self.heads, self.head_dim, self.t_max, L['theta'], scale,
                                                        self.native.ptr(tab), o_inv.data_ptr(), s)
                elif tab is not None:
                    rc = lib.gptq_decode_attn_fused_table_f16(self.qkvb.data_ptr(), self.pos.data_ptr(), self.kc[li].data_ptr(),
                                                              self.vc[li].data_ptr(), self.ab.data_ptr(), self.attn_ws.data_ptr(),
                                                              self.attn_ws.numel(), self.heads, self.head_dim, self.t_max, L['theta'], scale,
                                                              tab.data_ptr(), s)
                else:
                    rc = lib.gptq_decode_attn_fused_f16(self.qkvb.data_ptr(), self.pos.data_ptr(), self.kc[li].data_ptr(),
                                                        self.vc[li].data_ptr(), self.ab.data_ptr(), self.attn_ws.data_ptr(),
                                                        self.attn_ws.numel(), self.heads, self.head_dim, self.t_max, L['theta'], scale, s)
                self.native.check(rc, 'gptq_decode_attn_fused_f16')
            else:
                rc = lib.gptq_decode_rope_kv_f16(self.qkvb.data_ptr(), self.pos.data_ptr(), self.kc[li].data_ptr(),
                                                 self.vc[li].data_ptr(), self.heads, self.head_dim, self.t_max, L['theta'], s)
                self.native.check(rc, 'gptq_decode_rope_kv_f16')
                rc = lib.gptq_decode_attn_f16(self.qkvb.data_ptr(), self.kc[li].data_ptr(), self.vc[li].data_ptr(), self.pos.data_ptr(),
                                              self.ab.data_ptr(), self.attn_ws.data_ptr(), self.attn_ws.numel(), self.heads,
                                              self.head_dim, self.t_max, scale, s)
                self.native.check(rc, 'gptq_decode_attn_f16')
            if not self.attn_records:
                self._gemv(self.ab, L['o'], self.x2, s, residual=self.x, x_sorted=o_inv is not None)    # x2 = x + o_proj(attn)
            self._norm_mlp(self.x2, L['ln2'], L['gate'], L['up'], self.cb, s, out_perm=d_inv)
            self._gemv(self.cb, L['down'], self.x, s, residual=self.x2, x_sorted=d_inv is not None)     # x = x2 + down(silu(gate) * up)
        self._lm_head(s)
        self.pos.add_(1)

    def _lm_head(self, s):
        """logits = lm_head(rmsnorm(x)): the model's final norm and its dense fp16 LM head in ONE hand-written launch (gptq_dense_matmat_f16,
        csrc/dense_gemv.hip: one pass over the weight for all rows of a batch); a head the kernel does not take (odd strides, dtypes) goes
        through the stand-alone norm + torch.matmul."""
        lm_head_logits(self, self.x, self.logits, s)

    def reset(self):
        self.pos.zero_()

    def _greedy_step(self):
        """one decode step whose argmax becomes the next input token, entirely on the device: ids <- argmax(logits),
        and the choice is appended to stream_out[pos] (pos = number of tokens consumed so far)."""
        self._step()                                   # consumes self.ids, advances pos
        self._process_step()
        self._constrain_step()
        torch.argmax(self.logits, dim=-1, out=self.ids)
        self.stream_out.index_copy_(0, self.pos, self.ids)

    def _capture(self, step, state, keep_rng=False):
        """warm up once (module loads, workspaces), then capture step() into ONE hipGraph and return it.  The tensors of `state` -- what the step
        advances -- get their present values back behind the warm-up run and behind the capture; keep_rng: torch's CUDA generator, which a
        sampling step draws from, is put back where it was as well"""
        with torch.no_grad(), torch.cuda.device(self.dev):
            rng = torch.cuda.get_rng_state(self.dev) if keep_rng else None
            saved = [t.clone() for t in state]

            def restore():
                for t, t0 in zip(state, saved):
                    t.copy_(t0)
            step()
            torch.cuda.synchronize(self.dev)
            restore()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
            restore()
            if keep_rng:
                torch.cuda.synchronize(self.dev)
                torch.cuda.set_rng_state(rng, self.dev)
        return g

    def capture_greedy(self):
        """capture the self-feeding greedy step (engine_generate): a replay needs no host input at all."""
        self.greedy_graph = self._capture(self._greedy_step, (self.pos, self.ids) + self._constrain_state())
        return self

    def _stream_buffers(self):
        """stream_rows / stepc of the self-feeding steps, allocated on first use"""
        if self.stream_rows is None:
            self.stream_rows = torch.zeros((self.t_max + 1, self.batch), dtype=torch.int64, device=self.dev)
            self.stepc = torch.zeros(1, dtype=torch.int64, device=self.dev)
            if self.logprobs is not None:                  # the record ring of _logprobs_step: row n belongs to row n of stream_rows
                n, B, K = self.t_max + 1, self.batch, self.logprobs
                self.lp_chosen = torch.zeros((n, B), dtype=torch.float32, device=self.dev)
                self.lp_rank = torch.zeros((n, B), dtype=torch.int32, device=self.dev)
                self.lp_top_ids = torch.zeros((n, B, K), dtype=torch.int32, device=self.dev)
                self.lp_top = torch.zeros((n, B, K), dtype=torch.float32, device=self.dev)

    def _logprobs_launch(self, logits, ids, top, step, steps, chosen, rank, top_ids, top_logprobs):
        n = logits.shape[0]
        with self.native.on_device(self.dev):
            rc = self.lib.gptq_logprobs_rows_f16(logits.data_ptr(), logits.stride(0) if n > 1 else logits.shape[1], n, logits.shape[1], ids.data_ptr(),
                                                 top, self.native.ptr(step), steps, chosen.data_ptr(), rank.data_ptr(),
                                                 top_ids.data_ptr() if top else None, top_logprobs.data_ptr() if top else None,
                                                 self.native.stream_ptr(self.dev))
        self.native.check(rc, 'gptq_logprobs_rows_f16')

    def _logprobs_step(self):
        """behind choose(): the record of the tokens in self.ids under self.logits -- the logits the draw saw: behind the processors, before
        temperature / top-k / top-p -- into row stepc of the lp_* buffers, ONE launch that reads the step counter on the device and draws no
        random numbers.  Nothing without the flag."""
        if self.logprobs is not None:
            self._logprobs_launch(self.logits, self.ids, self.logprobs, self.stepc, self.t_max + 1, self.lp_chosen, self.lp_rank, self.lp_top_ids,
                                  self.lp_top)

    def token_logprobs(self, logits, ids, top=None):
        """the eager entry of gptq_logprobs_rows_f16, on any engine: for each row of `logits` ([n, vocab] or [vocab] fp16 on the engine's device,
        unit column stride, n <= 128) and its token ids[r] (int64 [n] on the device) -> (chosen float [n]: the token's log-probability, rank
        int32 [n]: its 0-based place among the row's tokens by (logit descending, id ascending), top_ids int32 [n, top], top_logprobs float
        [n, top]: the row's first `top` tokens), new tensors.  top: 0 .. 32; None: the engine's logprobs setting (0 without one).  What the
        drivers use for the first token of a generation, from the prompt's logits; decode()'s logits are as good.  A row with a NaN or +inf
        or of -inf only, and an id outside the vocabulary, give NaN and rank -1 (gptq_mi355x.h "token log-probabilities")."""
        what = 'DecodeEngine.token_logprobs'
        if top is None:
            top = self.logprobs or 0
        if isinstance(top, bool) or not isinstance(top, int) or not 0 <= top <= MAX_LOGPROBS:
            raise ValueError('%s: top must be None or an int in 0 .. %d, not %r' % (what, MAX_LOGPROBS, top))
        if logits.dim() == 1:
            logits = logits.unsqueeze(0)
        n = logits.shape[0] if logits.dim() == 2 else 0
        if not 1 <= n <= MAX_LOGPROBS_ROWS or logits.dtype != torch.float16 or logits.device != self.ids.device or logits.stride(1) != 1 or \
                logits.shape[1] < max(top, 1):
            raise ValueError('%s: logits must be fp16 [n <= %d, vocab >= %d] with unit column stride on %s' % (
                what, MAX_LOGPROBS_ROWS, max(top, 1), self.dev))
        if not torch.is_tensor(ids) or ids.dtype != torch.int64 or ids.device != self.ids.device or ids.shape != (n,) or not ids.is_contiguous():
            raise ValueError('%s: ids must be a contiguous int64 [%d] on %s' % (what, n, self.dev))
        dev = self.ids.device
        chosen = torch.empty(n, dtype=torch.float32, device=dev)
        rank = torch.empty(n, dtype=torch.int32, device=dev)
        top_ids = torch.empty((n, top), dtype=torch.int32, device=dev)
        top_logprobs = torch.empty((n, top), dtype=torch.float32, device=dev)
        self._logprobs_launch(logits, ids, top, None, 1, chosen, rank, top_ids, top_logprobs)
        return chosen, rank, top_ids, top_logprobs

    def _capture_rows(self, step, keep_rng=False):
        """_capture for the steps that append to stream_rows: the step counter starts at 0, and is 0 again afterwards"""
        self._stream_buffers()
        self.stepc.zero_()
        return self._capture(step, (self.pos, self.ids, self.stepc) + self._constrain_state(), keep_rng)

    def _self_feeding_step(self, choose):
        """THE self-feeding step, for any batch: one decode step, the processors and the constraint (nothing without their flags), choose() puts every row's next input
        token into self.ids, the logprobs record of the choices (nothing without the flag), and the choices of step n become row n of stream_rows
        (n = stepc, a device counter the step advances itself)"""
        self._stream_buffers()
        self._step()
        self._process_step()
        self._constrain_step()
        choose()
        self._logprobs_step()
        self.stream_rows.index_copy_(0, self.stepc, self.ids.unsqueeze(0))
        self.stepc.add_(1)

    def _greedy_rows_step(self):
        """the self-feeding greedy step: every row's argmax becomes its next input token"""
        self._self_feeding_step(lambda: torch.argmax(self.logits, dim=-1, out=self.ids))

    def capture_greedy_rows(self):
        """capture _greedy_rows_step (quant/engine_hook.py _greedy_fast: greedy model.generate without a host round trip per token)"""
        self.greedy_rows_graph = self._capture_rows(self._greedy_rows_step)
        return self

    def _sample_rows_step(self, warpers):
        """the self-feeding SAMPLING step: HF's own arithmetic on the step's logits (generation/utils.py `_sample`: fp32 copy, the warpers in HF's order,
        softmax, torch.multinomial) -- inside the graph, where the default generator's Philox offset advances per replay exactly as per eager call"""
        def choose():
            scores = self.logits.to(copy=True, dtype=torch.float32)
            for w in warpers:
                scores = w(None, scores)
            probs = torch.nn.functional.softmax(scores, dim=-1)
            self.ids.copy_(torch.multinomial(probs, num_samples=1).squeeze(1))
        self._self_feeding_step(choose)

    def capture_sample_rows(self, key, warpers):
        """capture _sample_rows_step for one (temperature, top_k, top_p) setting; the generator's state is put back behind the warm-up run"""
        g = self._capture_rows(lambda: self._sample_rows_step(warpers), keep_rng=True)
        self.sample_graphs = {key: g}              # (one setting at a time: a graph holds the temporaries of a vocabulary-sized sort per row)
        return g

    def _per_row(self, what, name, v, ok):
        """a setting of the rows -- a scalar for all or one value per row -- as a list of `batch` numbers that ok() accepts; `what` opens the
        ValueError's message"""
        B = self.batch
        vals = [v] * B if not isinstance(v, (list, tuple)) and not torch.is_tensor(v) else [x for x in (v.tolist() if torch.is_tensor(v) else v)]
        if len(vals) != B:
            raise ValueError('%s: %s has %d values for a batch of %d' % (what, name, len(vals), B))
        for x in vals:
            if isinstance(x, bool) or not isinstance(x, (int, float)) or not ok(x):
                raise ValueError('%s: %s = %r' % (what, name, x))
        return vals

    # -- sampling of the engine's own: gptq_sample_rows_f16 (csrc/sample.hip) with every row's setting in device memory --------------------
    def set_sampling(self, temperature=1.0, top_k=0, top_p=1.0):
        """the rows' sampling settings: a scalar for all rows or one value per row.  temperature 0 makes a row greedy, top_k 0 and top_p 1 switch
        the filter off.  Only the static device buffers change: a captured graph (capture_sample_native) serves the new setting at its next
        replay.  An engine that samples speculatively (chunk=R, or batch_chunk=R with spec_sample) also gets sequence b's setting in rows
        b R .. b R + R - 1 of its verify step (capture_verify_sample / _batch: those rows are consecutive tokens of sequence b).  ValueError
        for a temperature that is negative or not finite, a negative top_k, a top_p outside (0, 1]."""
        B = self.batch
        per_row = functools.partial(self._per_row, 'DecodeEngine.set_sampling')
        t = per_row('temperature', temperature, lambda x: math.isfinite(x) and x >= 0)
        k = per_row('top_k', top_k, lambda x: float(x).is_integer() and 0 <= x < 2 ** 31)
        p = per_row('top_p', top_p, lambda x: 0 < x <= 1)
        with torch.no_grad():
            self.temperature.copy_(torch.tensor(t, dtype=torch.float32))
            self.top_k.copy_(torch.tensor([int(x) for x in k], dtype=torch.int32))
            self.top_p.copy_(torch.tensor(p, dtype=torch.float32))
            if self.spec_sample:                     # the R rows of sequence b in a verify step decode that sequence: row b's setting
                R = self.chunk_rows
                self.chunk_temperature.view(B, R).copy_(self.temperature.unsqueeze(1).expand(B, R))
                self.chunk_top_k.view(B, R).copy_(self.top_k.unsqueeze(1).expand(B, R))
                self.chunk_top_p.view(B, R).copy_(self.top_p.unsqueeze(1).expand(B, R))
        return self

    def sample_logits(self, logits, out=None, u=None):
        """one token id per row of `logits` ([n, vocab] or [vocab] fp16 on the engine's device, unit column stride, n <= batch) drawn by
        gptq_sample_rows_f16 under the settings of rows 0 .. n - 1 (set_sampling).  u: n float32 uniforms in [0, 1) on the device -- with a
        given u nothing random happens; None draws them from torch's CUDA generator.  out: int64 [n] on the device (default: a new tensor)."""
        if logits.dim() == 1:
            logits = logits.unsqueeze(0)
        n = logits.shape[0] if logits.dim() == 2 else 0
        if not 1 <= n <= self.batch or logits.dtype != torch.float16 or logits.device != self.ids.device or logits.stride(1) != 1 or logits.shape[1] < 1:
            raise ValueError('DecodeEngine.sample_logits: logits must be fp16 [n <= %d, vocab] with unit column stride on %s' % (self.batch, self.dev))
        if u is None:
            u = torch.rand(n, dtype=torch.float32, device=self.ids.device)
        if out is None:
            out = torch.empty(n, dtype=torch.int64, device=self.ids.device)
        for name, t, dt in (('u', u, torch.float32), ('out', out, torch.int64)):
            if t.dtype != dt or t.device != self.ids.device or t.shape != (n,) or not t.is_contiguous():
                raise ValueError('DecodeEngine.sample_logits: %s must be a contiguous %s [%d] on %s' % (name, dt, n, self.dev))
        with self.native.on_device(self.dev):
            rc = self.lib.gptq_sample_rows_f16(logits.data_ptr(), logits.stride(0) if n > 1 else logits.shape[1], n, logits.shape[1], u.data_ptr(),
                                               self.temperature.data_ptr(), self.top_k.data_ptr(), self.top_p.data_ptr(), out.data_ptr(),
                                               self.native.stream_ptr(self.dev))
        self.native.check(rc, 'gptq_sample_rows_f16')
        return out

    def _sample_native_step(self):
        """the self-feeding sampling step of the engine's own, for ANY batch: one decode step, fresh uniforms from torch's CUDA generator (inside a
        graph its Philox offset advances per replay exactly as per eager call), ONE launch that draws every row's next token under that row's
        setting, and the bookkeeping of _self_feeding_step.  With logits_process the ONE process launch sits between the step and the uniforms:
        the row's token history -- the token just consumed included, appended by that launch -- edits self.logits in place before the draw;
        temperature 0 (set_sampling) makes this graph the greedy step under the processors."""
        def choose():
            self.u.uniform_()
            self.sample_logits(self.logits, out=self.ids, u=self.u)
        self._self_feeding_step(choose)

    def capture_sample_native(self):
        """capture _sample_native_step ONCE: the settings are device buffers the kernel reads at every replay, so set_sampling never re-captures.
        The generator's state is put back behind the warm-up run, as capture_sample_rows does."""
        self.sample_native_graph = self._capture_rows(self._sample_native_step, keep_rng=True)
        return self.sample_native_graph

    # -- logit processors: gptq_logits_process_f16 (csrc/logits_process.hip) on the rows' token history, every setting in device memory ---------
    def _need_logits_process(self, what):
        if not self.logits_process:
            raise ValueError('DecodeEngine.%s: the engine was built without logits_process=True' % what)

    def set_logits_process(self, repetition_penalty=1.0, presence_penalty=0.0, min_new_tokens=0, eos_token_id=None, logit_bias=None):
        """the rows' processor settings.  repetition_penalty (finite, > 0; 1 is off: HF's rule, the prompt counts), presence_penalty (finite;
        subtracted once from every token GENERATED so far) and min_new_tokens (an int >= 0: no eos token before that many generated ones) are
        a scalar for all rows or one value per row.  eos_token_id: None, an int or up to 8 ints -- what min_new_tokens masks.  logit_bias:
        None or {id: value} of at most 256 distinct ids in [0, vocab), values finite or -inf (-inf bans the token); added AFTER the
        penalties, shared by all rows.  Every call sets all five.  Only the static device buffers change -- a captured step serves the new
        values at its next replay -- EXCEPT the two list lengths, which are launch arguments: a call that changes the number of eos ids or of
        bias entries drops the captured self-feeding graphs (capture_sample_native, capture_greedy, capture_greedy_rows,
        capture_sample_rows), which are captured again at their next use.  ValueError before anything changes."""
        self._need_logits_process('set_logits_process')
        V = self.logits.shape[1]
        per_row = functools.partial(self._per_row, 'DecodeEngine.set_logits_process')
        rp = per_row('repetition_penalty', repetition_penalty, lambda x: math.isfinite(x) and x > 0)
        pp = per_row('presence_penalty', presence_penalty, math.isfinite)
        mn = per_row('min_new_tokens', min_new_tokens, lambda x: float(x).is_integer() and 0 <= x < 2 ** 31)
        eos = [] if eos_token_id is None else (eos_token_id.tolist() if torch.is_tensor(eos_token_id) else eos_token_id)
        eos = list(eos) if isinstance(eos, (list, tuple)) else [eos]
        if len(eos) > MAX_PROCESS_EOS or any(isinstance(e, bool) or not isinstance(e, int) or not -2 ** 31 <= e < 2 ** 31 for e in eos):
            raise ValueError('DecodeEngine.set_logits_process: eos_token_id must be an int or up to %d ints, not %r' % (MAX_PROCESS_EOS, eos_token_id))
        pairs = [] if logit_bias is None else (list(logit_bias.items()) if isinstance(logit_bias, dict) else logit_bias)
        if not isinstance(pairs, (list, tuple)) or len(pairs) > MAX_PROCESS_BIAS or any(not isinstance(e, (list, tuple)) or len(e) != 2 for e in pairs):
            raise ValueError('DecodeEngine.set_logits_process: logit_bias must be a dict {id: value} (or a list of (id, value) pairs) of at most '
                             '%d entries' % MAX_PROCESS_BIAS)
        ids, bias = [], {}
        for k, x in pairs:
            if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < V:
                raise ValueError('DecodeEngine.set_logits_process: logit_bias id %r outside [0, %d)' % (k, V))
            if isinstance(x, bool) or not isinstance(x, (int, float)) or not (math.isfinite(x) or x == -math.inf):
                raise ValueError('DecodeEngine.set_logits_process: logit_bias[%d] = %r must be finite or -inf' % (k, x))
            if k in bias:                                    # (the kernel gives every entry its own thread: one entry per token)
                raise ValueError('DecodeEngine.set_logits_process: logit_bias id %d is listed twice' % k)
            ids.append(k)
            bias[k] = x
        with torch.no_grad():
            self.rep_penalty.copy_(torch.tensor(rp, dtype=torch.float32))
            self.presence_penalty.copy_(torch.tensor(pp, dtype=torch.float32))
            self.min_new.copy_(torch.tensor([int(x) for x in mn], dtype=torch.int32))
            if eos:
                self.eos_ids[:len(eos)].copy_(torch.tensor(eos, dtype=torch.int32))
            if ids:
                self.bias_ids[:len(ids)].copy_(torch.tensor(ids, dtype=torch.int32))
                self.bias_vals[:len(ids)].copy_(torch.tensor([float(bias[k]) for k in ids], dtype=torch.float32))
        if (len(eos), len(ids)) != (self.n_eos, self.n_bias):
            self.n_eos, self.n_bias = len(eos), len(ids)
            self.sample_native_graph, self.greedy_graph, self.greedy_rows_graph, self.sample_graphs = None, None, None, {}
        return self

    def _write_history(self, row, start, ids):
        """hist[row, start : start + T] = ids and gen_start[row] = start + T: what every prompt path does behind its layers"""
        T = int(ids.numel())
        self.hist[row, start:start + T].copy_(ids.reshape(-1))
        self.gen_start[row:row + 1].fill_(start + T)

    def set_history(self, row, ids, gen_start=None):
        """for callers that fill cache row `row` by other means than prefill / prefill_batch / decode: ids (1-D, T <= t_max) are the tokens at
        positions 0 .. T - 1 of that row, gen_start (default T) the first position that counts as generated.  pos is not touched."""
        self._need_logits_process('set_history')
        row, T = int(row), int(ids.numel())
        if not 0 <= row < self.batch or ids.dim() != 1 or not 1 <= T <= self.t_max:
            raise ValueError('DecodeEngine.set_history: needs a row of the batch of %d and 1 .. %d ids' % (self.batch, self.t_max))
        with torch.no_grad():
            self._write_history(row, 0, ids)
            if gen_start is not None:
                self.gen_start[row:row + 1].fill_(int(gen_start))
        return self

    def _process_launch(self, logits, n, last, len_add):
        with self.native.on_device(self.dev):
            rc = self.lib.gptq_logits_process_f16(
                logits.data_ptr(), logits.stride(0) if n > 1 else logits.shape[1], n, 1, logits.shape[1], self.hist.data_ptr(), self.hist.stride(0),
                self.t_max, self.native.ptr(last), self.pos.data_ptr(), len_add, self.gen_start.data_ptr(), self.rep_penalty.data_ptr(),
                self.presence_penalty.data_ptr(), self.min_new.data_ptr(), self.eos_ids.data_ptr(), self.n_eos, self.bias_ids.data_ptr(),
                self.bias_vals.data_ptr(), self.n_bias, self.native.stream_ptr(self.dev))
        self.native.check(rc, 'gptq_logits_process_f16')

    def _process_step(self):
        """behind _step() (pos is advanced already: len_add = -1): the processors on self.logits under every row's history INCLUDING the token
        this step consumed (self.ids), which the same launch appends to hist.  A row idling at a negative position, or past the cache, is
        left alone.  Nothing without the flag."""
        if self.logits_process:
            self._process_launch(self.logits, self.batch, self.ids, -1)

    def process_logits(self, logits, last=None):
        """the eager counterpart of sample_logits: rows 0 .. n - 1 of `logits` ([n, vocab] or [vocab] fp16 on the engine's device, unit column
        stride, n <= batch) IN PLACE under those rows' settings (set_logits_process) and their history hist[b, 0 : pos[b]] -- what the first
        token after a prompt needs.  last: int64 [n] on the device, tokens consumed at positions pos[b] that hist does not hold yet: they
        count, and are appended at hist[b, pos[b]].  Returns logits."""
        self._need_logits_process('process_logits')
        rows = logits.unsqueeze(0) if logits.dim() == 1 else logits
        n = rows.shape[0] if rows.dim() == 2 else 0
        if not 1 <= n <= self.batch or rows.dtype != torch.float16 or rows.device != self.ids.device or rows.stride(1) != 1 or \
                not 1 <= rows.shape[1] <= MAX_PROCESS_VOCAB:
            raise ValueError('DecodeEngine.process_logits: logits must be fp16 [n <= %d, vocab] with unit column stride on %s' % (self.batch, self.dev))
        if last is not None and (last.dtype != torch.int64 or last.device != self.ids.device or last.shape != (n,) or not last.is_contiguous()):
            raise ValueError('DecodeEngine.process_logits: last must be a contiguous int64 [%d] on %s' % (n, self.dev))
        self._process_launch(rows, n, last, 0)
        return logits

    # -- constrained decoding: gptq_constrain_rows_f16 (csrc/constrain.hip) on the rows' automaton states, every table in device memory ----------
    def _need_constrain(self, what):
        if self.constrain is None:
            raise ValueError('DecodeEngine.%s: the engine was built without constrain=' % what)

    def _constrain_state(self):
        """what a capture must put back behind its warm-up run and behind the capture itself: both run the step, and the step moves c_state"""
        return () if self.constrain is None else (self.c_state,)

    def set_constraint(self, dfa):
        """the rows' automata: a quant.constrain.TokenDFA, None (unconstrained), or a list of `batch` of either -- it may differ per row.  The
        automata are stacked into c_next, each at a state offset, their transitions shifted on upload, so c_state holds absolute indices; rows
        that pass the same object share its states and its class map.  Every row is put to its automaton's start (None: -1).  Only the static
        device buffers change: a captured graph serves the new automata at its next replay, and no graph is dropped.  ValueError before
        anything changes when the automata do not fit the capacities or a vocabulary differs from the head's."""
        from .constrain import TokenDFA
        self._need_constrain('set_constraint')
        what, B, V = 'DecodeEngine.set_constraint', self.batch, self.logits.shape[1]
        dfas = list(dfa) if isinstance(dfa, (list, tuple)) else [dfa] * B
        if len(dfas) != B or any(d is not None and not isinstance(d, TokenDFA) for d in dfas):
            raise ValueError('%s: needs a TokenDFA, None or a list of %d of either' % (what, B))
        distinct = []
        for d in dfas:
            if d is not None and not any(d is e for e in distinct):
                distinct.append(d)
        for d in distinct:
            if d.vocab != V:
                raise ValueError('%s: an automaton over %d tokens for a head of %d' % (what, d.vocab, V))
        states, classes = sum(d.n_states for d in distinct), max([d.n_classes for d in distinct] + [1])
        if states > self.constrain['states'] or classes > self.constrain['classes']:
            raise ValueError('%s: the automata need %d states and %d classes, the engine was built for %d and %d' % (
                what, states, classes, self.constrain['states'], self.constrain['classes']))
        with torch.no_grad():
            offset, first_row, start, maps = 0, {}, [], []
            self.c_next.fill_(-1)
            for b, d in enumerate(dfas):
                if d is None:
                    start.append(-1)
                    maps.append(b)
                    continue
                if id(d) not in first_row:                           # its states at `offset`, its class map in the slot of its first row
                    nxt = d.next.astype(np.int32)
                    nxt[nxt >= 0] += offset
                    self.c_next[offset:offset + d.n_states, :d.n_classes].copy_(torch.from_numpy(nxt.astype(np.int16)))
                    self.c_cls[b].copy_(torch.from_numpy(d.cls.copy()))        # (a copy: the automaton's arrays are read-only)
                    first_row[id(d)] = (b, offset)
                    offset += d.n_states
                maps.append(first_row[id(d)][0])
                start.append(first_row[id(d)][1])
            self.c_map.copy_(torch.tensor(maps, dtype=torch.int32))
            self._c_dfas, self._c_start = dfas, start
            self.c_state.copy_(torch.tensor(start, dtype=torch.int32))
        return self

    def reset_constraint(self, rows=None):
        """the rows (None: all; an int or a list of ints) back to the start states of their automata"""
        self._need_constrain('reset_constraint')
        rows = range(self.batch) if rows is None else ([rows] if isinstance(rows, int) else list(rows))
        if any(isinstance(r, bool) or not isinstance(r, int) or not 0 <= r < self.batch for r in rows):
            raise ValueError('DecodeEngine.reset_constraint: rows must lie in the batch of %d' % self.batch)
        state = self.c_state.tolist()
        for r in rows:
            state[r] = self._c_start[r]
        with torch.no_grad():
            self.c_state.copy_(torch.tensor(state, dtype=torch.int32))
        return self

    def _constrain_launch(self, logits, n, last, len_add):
        with self.native.on_device(self.dev):
            rc = self.lib.gptq_constrain_rows_f16(
                logits.data_ptr(), logits.stride(0) if n > 1 else logits.shape[1], n, logits.shape[1], self.c_next.data_ptr(), self.c_next.stride(0),
                self.c_next.shape[0], self.c_next.shape[1], self.c_cls.data_ptr(), self.c_cls.stride(0), self.batch, self.c_map.data_ptr(),
                self.c_state.data_ptr(), self.native.ptr(last), self.pos.data_ptr(), len_add, self.t_max - (0 if last is None else 1),
                self.native.stream_ptr(self.dev))
        self.native.check(rc, 'gptq_constrain_rows_f16')

    def _constrain_step(self):
        """behind _process_step() (pos is advanced already: len_add = -1): every row's state advances by the token this step consumed (self.ids)
        and self.logits is masked under the new state, in ONE launch -- the processors act first, then the mask.  A row idling at a negative
        position, or past the cache, is left alone, as the processors leave it.  Nothing without the flag."""
        if self.constrain is not None:
            self._constrain_launch(self.logits, self.batch, self.ids, -1)

    def constrain_logits(self, logits, last=None):
        """the eager entry, with the shape rules of process_logits: rows 0 .. n - 1 of `logits` ([n, vocab] or [vocab] fp16 on the engine's
        device, unit column stride, n <= batch) are masked IN PLACE under those rows' states -- what the first token after a prompt needs.
        last: int64 [n] on the device, tokens the rows consume first: the states advance by them, and a token its state bans puts the row at
        -2 (it has left its automaton: its logits are left alone from then on).  Returns logits."""
        self._need_constrain('constrain_logits')
        rows = logits.unsqueeze(0) if logits.dim() == 1 else logits
        n = rows.shape[0] if rows.dim() == 2 else 0
        if not 1 <= n <= self.batch or rows.dtype != torch.float16 or rows.device != self.ids.device or rows.stride(1) != 1 or \
                rows.shape[1] != self.logits.shape[1]:
            raise ValueError('DecodeEngine.constrain_logits: logits must be fp16 [n <= %d, vocab] with unit column stride on %s' % (self.batch, self.dev))
        if last is not None and (last.dtype != torch.int64 or last.device != self.ids.device or last.shape != (n,) or not last.is_contiguous()):
            raise ValueError('DecodeEngine.constrain_logits: last must be a contiguous int64 [%d] on %s' % (n, self.dev))
        self._constrain_launch(rows, n, last, 0)
        return logits

    # -- beam search: the N rows are the running beams; gptq_beam_select_f16 + gptq_kv_reorder_f16 (csrc/beam.hip) behind the batch step ---------
    def _need_beam_search(self, what):
        if not self.beam_search:
            raise ValueError('DecodeEngine.%s: the engine was built without beam_search=True' % what)

    def set_beam_search(self, max_new_tokens, eos_token_id=None, length_penalty=1.0, early_stopping=False):
        """the settings of the next search, and its state put back to the start: scores [0, DEAD ..], an empty pool, t = 0, open, not done.
        Only the device block changes: a captured beam step serves the new search at its next replay.  ValueError: max_new_tokens outside
        1 .. t_max; more than one EOS id, or one outside the vocabulary; a length_penalty that is not finite; early_stopping other than
        False, True or 'never'."""
        self._need_beam_search('set_beam_search')
        what = 'DecodeEngine.set_beam_search'
        if isinstance(max_new_tokens, bool) or not isinstance(max_new_tokens, int) or not 1 <= max_new_tokens <= self.t_max:
            raise ValueError('%s: max_new_tokens = %r must be 1 .. %d' % (what, max_new_tokens, self.t_max))
        if isinstance(eos_token_id, (list, tuple)):
            if len(eos_token_id) > 1:
                raise ValueError('%s: beam search takes one EOS id, not %r' % (what, eos_token_id))
            eos_token_id = eos_token_id[0] if eos_token_id else None
        if eos_token_id is not None and (isinstance(eos_token_id, bool) or not isinstance(eos_token_id, int) or
                                         not 0 <= eos_token_id < self.logits.shape[1]):
            raise ValueError('%s: eos_token_id = %r outside [0, %d)' % (what, eos_token_id, self.logits.shape[1]))
        if isinstance(length_penalty, bool) or not isinstance(length_penalty, (int, float)) or not math.isfinite(length_penalty):
            raise ValueError('%s: length_penalty = %r' % (what, length_penalty))
        modes = [m for m, v in ((0, False), (1, True), (2, 'never')) if early_stopping is v or (isinstance(v, str) and early_stopping == v)]
        if not modes:
            raise ValueError("%s: early_stopping = %r must be False, True or 'never'" % (what, early_stopping))
        B = self.batch
        w = np.zeros(BEAM_W_TABLES, dtype=np.int32)
        f = w.view(np.float32)
        w[BEAM_W_EOS], w[BEAM_W_MAX_NEW], w[BEAM_W_ES] = -1 if eos_token_id is None else eos_token_id, max_new_tokens, modes[0]
        f[BEAM_W_LP] = length_penalty
        w[BEAM_W_T_CAP], w[BEAM_W_BEAMS], w[BEAM_W_OPEN] = self.t_max, B, 1
        f[BEAM_W_SCORE:BEAM_W_SCORE + MAX_BEAMS] = BEAM_DEAD
        f[BEAM_W_SCORE] = 0.0
        f[BEAM_W_POOL:BEAM_W_CAND:5] = BEAM_DEAD
        with torch.no_grad():
            self.beam_state.zero_()
            self.beam_state[:BEAM_W_TABLES].copy_(torch.from_numpy(w))
        return self

    def beam_select(self, logits):
        """one beam step (gptq_beam_select_f16) on `logits`, any fp16 [N, vocab] tensor with unit column stride on the engine's device: the
        state block advances -- scores, beam_parent (int32 [N]), beam_token (int64 [N]), pool, tables, flags"""
        self._need_beam_search('beam_select')
        B = self.batch
        if logits.dim() != 2 or logits.shape[0] != B or logits.dtype != torch.float16 or logits.device != self.ids.device or \
                logits.stride(1) != 1 or logits.shape[1] < 2 * B or logits.stride(0) < logits.shape[1]:
            raise ValueError('DecodeEngine.beam_select: logits must be fp16 [%d, vocab >= %d] with unit column stride on %s' % (B, 2 * B, self.dev))
        with self.native.on_device(self.dev):
            rc = self.lib.gptq_beam_select_f16(logits.data_ptr(), logits.stride(0), B, logits.shape[1], self.beam_state.data_ptr(),
                                               self.native.stream_ptr(self.dev))
        self.native.check(rc, 'gptq_beam_select_f16')

    def _beam_reorder(self):
        """cache row b continues row beam_parent[b] at positions [0, pos[0]) (gptq_kv_reorder_f16: in place, every layer, both caches)"""
        with self.native.on_device(self.dev):
            rc = self.lib.gptq_kv_reorder_f16(self.kcb.data_ptr(), self.vcb.data_ptr(), self.kcb.shape[0], self.batch, self.t_max, self.hidden,
                                              self.kcb.stride(0), self.beam_parent.data_ptr(), self.pos.data_ptr(),
                                              self.native.stream_ptr(self.dev))
        self.native.check(rc, 'gptq_kv_reorder_f16')

    def _beam_advance(self, logits):
        self.beam_select(logits)
        self._beam_reorder()
        self.ids.copy_(self.beam_token)

    def beam_begin(self, first_logits):
        """the first step of a search whose prompt sits in cache row 0 (prefill; pos[0] = its length): the one row of prompt logits stands for all
        N beams -- only beam 0 is alive --, select, the reorder replicates row 0's prompt into every row, ids <- the N first tokens"""
        self._need_beam_search('beam_begin')
        with torch.no_grad():
            rows = first_logits.reshape(1, -1).to(device=self.dev, dtype=torch.float16).expand(self.batch, -1).contiguous()
            self.pos.copy_(self.pos[:1].clone().expand(self.batch))
            self._beam_advance(rows)

    def _beam_step(self):
        """one step of the search: the batch step on the beams' tokens, select on its logits, the reorder, ids <- the step's tokens"""
        self._step()
        self._beam_advance(self.logits)

    def capture_beam_step(self):
        """capture _beam_step ONCE: settings and state are device memory, so set_beam_search never re-captures"""
        self._need_beam_search('capture_beam_step')
        self.beam_graph = self._capture(self._beam_step, (self.pos, self.ids, self.beam_state))
        return self.beam_graph

    def beam_result(self, num_return_sequences=1):
        """the best finished hypotheses of the pool, best first: (list of 1-D int64 tensors -- the tokens, a closing EOS included --, float32
        scores: HF's sequences_scores).  One download of the state block; the tokens come from the back-pointer tables."""
        self._need_beam_search('beam_result')
        B, T = self.batch, self.t_max
        if not 1 <= num_return_sequences <= B:
            raise ValueError('DecodeEngine.beam_result: num_return_sequences = %r for %d beams' % (num_return_sequences, B))
        w = self.beam_state.cpu().numpy()
        parent_at = w[BEAM_W_TABLES:BEAM_W_TABLES + T * B].reshape(T, B)
        token_at = w[BEAM_W_TABLES + T * B:BEAM_W_TABLES + 2 * T * B].reshape(T, B)
        seqs, scores = [], []
        for i in range(num_return_sequences):
            e = w[BEAM_W_POOL + 5 * i:BEAM_W_POOL + 5 * i + 5]
            if not e[1]:
                raise RuntimeError('DecodeEngine.beam_result: the pool holds %d finished hypotheses, %d were asked for' % (i, num_return_sequences))
            step, beam = int(e[2]), int(e[3])
            toks = [0] * step + [int(e[4])]
            for u in range(step - 1, -1, -1):
                toks[u], beam = int(token_at[u, beam]), int(parent_at[u, beam])
            seqs.append(torch.tensor(toks, dtype=torch.int64))
            scores.append(e[:1].view(np.float32)[0])
        return seqs, torch.tensor(np.array(scores, dtype=np.float32))

    def capture(self):
        """warm up once (module loads, workspace), then capture one decode step into a hipGraph."""
        self.reset()
        self.graph = self._capture(self._step, (self.pos,))
        return self

    # -- a prompt: T tokens of ONE row at M = T, attention by gptq_prompt_attn_f16 on the row's own cache slice -----------------------
    def _prefill_buffers(self, T):
        """activation buffers for M = T rows: allocated on first use, grown when a longer prompt arrives, kept"""
        pb = self._prefill_bufs
        if pb is None or pb['x'].shape[0] < T:
            H, I = self.hidden, self.cb.shape[1]
            f16 = dict(dtype=torch.float16, device=self.dev)
            pb = dict(x=torch.empty((T, H), **f16), x2=torch.empty((T, H), **f16), h=torch.empty((T, H), **f16), qkv=torch.empty((T, 3 * H), **f16),
                      ab=torch.empty((T, H), **f16), cb=torch.empty((T, I), **f16),
                      ws=torch.empty(max(256, self.lib.gptq_prompt_attn_workspace_bytes(T, self.heads, self.head_dim, self.t_max)),
                                     dtype=torch.uint8, device=self.dev))
            self._prefill_bufs = pb
        return pb

    def _prompt_layers(self, ids, attn, s):
        """every layer at M = len(ids) packed rows on the first M rows of the prefill buffers (_prefill_buffers has been called): embedding,
        then per layer norm -> qkv -> the caller's attn(li, L, qkv, ab, ws, tab) (RoPE + cache append + causal attention) -> o_proj -> add ->
        norm -> gate/up -> down -> add.  Returns (x, h): the last block's output and an [M, hidden] scratch."""
        pb, M = self._prefill_bufs, int(ids.numel())
        x, x2, h, qkv, ab, cb = (pb[k][:M] for k in ('x', 'x2', 'h', 'qkv', 'ab', 'cb'))
        torch.index_select(self.embed, 0, ids, out=x)

        def add_rows(y, r):
            self.native.check(self.lib.gptq_add_rows_f16(y.data_ptr(), y.stride(0), r.data_ptr(), r.stride(0), M, self.hidden, s), 'gptq_add_rows_f16')
        for li, L in enumerate(self.layers):
            self._norm_rows(x, L['ln1'], h, s)
            L['qkv']['_keep'].forward(h, qkv)                                       # qkv = qkv_proj(rmsnorm(x))
            attn(li, L, qkv, ab, pb['ws'], self._rope_table(L['theta'], s))
            L['o']['_keep'].forward(ab, x2)
            add_rows(x2, x)                                                         # x2 = x + o_proj(attn)
            self._norm_rows(x2, L['ln2'], h, s)
            L['gate']['_keep'].forward(h, cb)                                       # c = silu(gate(h)) * up(h): the pair's PreparedLayer
            L['down']['_keep'].forward(cb, x)
            add_rows(x, x2)                                                         # x = x2 + down(c)
        return x, h

    def _head_rows(self, last, rows, pos, s):
        """the end of every prompt call: logits[rows] = lm_head(rmsnorm(last)) and pos[rows] = pos; returns those rows of the static logits buffer.
        rows an int (prefill, score): the one row is written in place; a list: one LM head launch for all of them, then scattered."""
        if isinstance(rows, int):
            lm_head_logits(self, last, self.logits[rows:rows + 1], s)
            self.pos[rows:rows + 1].fill_(pos)
            return self.logits[rows]
        rows_t = torch.tensor(rows, dtype=torch.int64, device=self.dev)
        logits = torch.empty((len(rows), self.logits.shape[1]), dtype=torch.float16, device=self.dev)
        lm_head_logits(self, last, logits, s)
        self.logits.index_copy_(0, rows_t, logits)
        self.pos.index_copy_(0, rows_t, torch.tensor(pos, dtype=torch.int64, device=self.dev))
        return self.logits[rows_t]

    def _kv8_store(self, li, table, nseq, s):
        """an fp8 engine: the rows of the segments `table` (a PromptSeg array: rows start .. start + rows - 1 of cache row slot) of the fp16 staging
        cache kst / vst -> layer li of the fp8 cache (gptq_kv8_store_f16, one launch)"""
        with self.native.on_device(self.dev):
            rc = self.lib.gptq_kv8_store_f16(self.kst.data_ptr(), self.vst.data_ptr(), self.kst.stride(0), table, nseq, self.k8b[li].data_ptr(),
                                             self.v8b[li].data_ptr(), self.kexpb[li].data_ptr(), self.vexpb[li].data_ptr(), self.heads,
                                             self.head_dim, self.t_max, s)
        self.native.check(rc, 'gptq_kv8_store_f16')

    def prefill(self, input_ids, row=0, start=None):
        """Feed T tokens of ONE sequence (input_ids: int64, 1-D or [1, T]) into cache row `row` at positions start .. start + T - 1 and return
        the logits after the last of them (self.logits[row], the static buffer: clone it to keep it -- the contract of decode()).
        start=None continues at self.pos[row]; start=0 begins a new sequence in that row.  Every layer runs at M = T through the engine's own
        launches: gptq_rmsnorm_f16, the layer's PreparedLayer (gptq_layer_forward: the derived copy the modules and the decode step share; any
        bit width, act-order included), gptq_prompt_attn_f16 (RoPE + cache append + causal attention on kcb[li, row] / vcb[li, row]),
        gptq_add_rows_f16; only the last row goes through the LM head.  Nothing of `transformers` is involved; not graph-captured."""
        ids = input_ids.reshape(-1) if (input_ids.dim() == 1 or (input_ids.dim() == 2 and input_ids.shape[0] == 1)) else None
        if ids is None or ids.numel() == 0:
            raise ValueError('DecodeEngine.prefill: input_ids must be a non-empty 1-D or [1, T] tensor')
        row = int(row)
        if not 0 <= row < self.batch:
            raise ValueError('DecodeEngine.prefill: row %d outside the batch of %d' % (row, self.batch))
        T = int(ids.numel())
        start = int(self.pos[row]) if start is None else int(start)
        if start < 0 or start + T > self.t_max:
            raise ValueError('DecodeEngine.prefill: positions %d .. %d do not fit the engine cache (%d)' % (start, start + T - 1, self.t_max))
        fp8 = self.kv_cache == 'fp8'
        if fp8 and start != 0:
            raise ValueError("DecodeEngine.prefill: start = %d on a kv_cache='fp8' engine is not built yet (the prompt attention reads fp16 rows: "
                             "only a whole prompt from position 0)" % start)
        with torch.no_grad(), torch.cuda.device(self.dev):
            s = self.native.stream_ptr(self.dev)
            self._prefill_buffers(T)
            table = (self.native.PromptSeg * 1)(self.native.PromptSeg(0, T, start, row)) if fp8 else None

            def attn(li, L, qkv, ab, ws, tab):
                kc, vc = (self.kst[row], self.vst[row]) if fp8 else (self.kcb[li, row], self.vcb[li, row])
                rc = self.lib.gptq_prompt_attn_f16(qkv.data_ptr(), qkv.stride(0), T, start, kc.data_ptr(), vc.data_ptr(),
                                                   ab.data_ptr(), ab.stride(0), ws.data_ptr(), ws.numel(), self.heads, self.head_dim, self.t_max,
                                                   L['theta'], self.scale, self.native.ptr(tab), s)
                self.native.check(rc, 'gptq_prompt_attn_f16')
                if fp8:
                    self._kv8_store(li, table, 1, s)
            ids = ids.to(device=self.dev, dtype=torch.int64)
            x, _ = self._prompt_layers(ids, attn, s)
            if self.logits_process:
                self._write_history(row, start, ids)
            return self._head_rows(x[T - 1:T], row, start + T, s)

    def _packed(self, what, prompts, rows, starts, max_rows, score=False, one_row=False):
        """prefill_batch (`what`: the public method, for the messages), score and score_batch: prompts[i] enters cache row rows[i] at starts[i] ..,
        all prompts packed into one activation, in passes of at most max_rows packed rows with ONE segment per prompt and pass; the last row
        of every prompt goes through _head_rows (one_row: the in-place form of prefill).  score: the ids are range-checked on the host, and
        behind every pass the final norm and _nll_rows run over all its rows -- the targets are the packed ids shifted by one, so the last row
        of a pass is scored against the first token of the next, and the last row of every prompt gives 0.  Validates everything (ValueError)
        before the first launch.  Returns (logits[rows], nll [sum T] float32 or None, offs, lens)."""
        n = len(prompts)
        if not 1 <= n <= self.batch:
            raise ValueError('DecodeEngine.%s: %d prompts for an engine of batch %d' % (what, n, self.batch))
        if any((not torch.is_tensor(p)) or p.dim() != 1 or p.numel() == 0 for p in prompts):
            raise ValueError('DecodeEngine.%s: every prompt must be a non-empty 1-D tensor of ids' % what)
        rows = list(range(n)) if rows is None else [int(r) for r in rows]
        if len(rows) != n or len(set(rows)) != n or any(not 0 <= r < self.batch for r in rows):
            raise ValueError('DecodeEngine.%s: rows %r must be %d distinct rows of the batch of %d' % (what, rows, n, self.batch))
        starts = [0] * n if starts is None else list(starts)
        if len(starts) != n:
            raise ValueError('DecodeEngine.%s: %d starts for %d prompts' % (what, len(starts), n))
        if any(st is None for st in starts):
            pos = self.pos.tolist()
            starts = [pos[r] if st is None else st for st, r in zip(starts, rows)]
        starts = [int(st) for st in starts]
        lens = [int(p.numel()) for p in prompts]
        for st, T in zip(starts, lens):
            if st < 0 or st + T > self.t_max:
                raise ValueError('DecodeEngine.%s: positions %d .. %d do not fit the engine cache (%d)' % (what, st, st + T - 1, self.t_max))
        max_rows = int(max_rows)
        if max_rows < 1:
            raise ValueError('DecodeEngine.%s: max_rows must be positive' % what)
        total = sum(lens)
        offs = [sum(lens[:i]) for i in range(n)]                                    # first packed row of prompt i
        fp8 = self.kv_cache == 'fp8'
        if fp8 and (score or any(st != 0 for st in starts) or total > max_rows):
            raise ValueError("DecodeEngine.%s on a kv_cache='fp8' engine is not built yet: %s" % (what, (
                'scoring' if score else 'a start other than 0' if any(st != 0 for st in starts) else
                '%d packed rows need more than one pass of max_rows = %d' % (total, max_rows)) +
                ' (the prompt attention reads fp16 rows: only whole prompts from position 0 in one pass)'))
        if score:
            vocab = min(self.embed.shape[0], self.lm_head.shape[0])
            host = torch.cat([p.detach().reshape(-1).to(device='cpu', dtype=torch.int64) for p in prompts])      # a copy, not a launch
            if int(host.min()) < 0 or int(host.max()) >= vocab:
                raise ValueError('DecodeEngine.%s: token ids must lie in [0, %d)' % (what, vocab))
            shifted = torch.full((total,), -100, dtype=torch.int64)                 # target of packed row r: the next id of the SAME prompt
            for o, T in zip(offs, lens):
                shifted[o:o + T - 1] = host[o + 1:o + T]
        with torch.no_grad(), torch.cuda.device(self.dev):
            s = self.native.stream_ptr(self.dev)
            self._prefill_buffers(min(total, max_rows))
            nll = None
            if score:
                ids, targets = host.to(self.dev), shifted.to(self.dev)
                nll = torch.empty(total, dtype=torch.float32, device=self.dev)
            else:
                ids = torch.cat([p.to(device=self.dev, dtype=torch.int64) for p in prompts])
            last = torch.empty((n, self.hidden), dtype=torch.float16, device=self.dev)      # the final hidden row of every prompt
            slot_stride = self.kst.stride(0) if fp8 else self.kcb.stride(1)
            for p0 in range(0, total, max_rows):
                M = min(total, p0 + max_rows) - p0
                # the part of every prompt inside packed rows [p0, p0 + M): ONE segment per prompt and pass (never two of the same cache row)
                segs, ends = [], []
                for i in range(n):
                    lo, hi = max(offs[i], p0), min(offs[i] + lens[i], p0 + M)
                    if lo < hi:
                        segs.append(self.native.PromptSeg(lo - p0, hi - lo, starts[i] + lo - offs[i], rows[i]))
                        if hi == offs[i] + lens[i]:
                            ends.append((i, hi - 1 - p0))
                table = (self.native.PromptSeg * len(segs))(*segs)

                def attn(li, L, qkv, ab, ws, tab):
                    kc, vc = (self.kst, self.vst) if fp8 else (self.kcb[li], self.vcb[li])
                    rc = self.lib.gptq_prompt_attn_batch_f16(qkv.data_ptr(), qkv.stride(0), M, table, len(segs), kc.data_ptr(),
                                                             vc.data_ptr(), slot_stride, ab.data_ptr(), ab.stride(0), ws.data_ptr(),
                                                             ws.numel(), self.heads, self.head_dim, self.t_max, L['theta'], self.scale,
                                                             self.native.ptr(tab), s)
                    self.native.check(rc, 'gptq_prompt_attn_batch_f16')
                    if fp8:
                        self._kv8_store(li, table, len(segs), s)
                x, h = self._prompt_layers(ids[p0:p0 + M], attn, s)
                if ends:
                    dst = torch.tensor([i for i, _ in ends], dtype=torch.int64, device=self.dev)
                    src = torch.tensor([r for _, r in ends], dtype=torch.int64, device=self.dev)
                    last.index_copy_(0, dst, x.index_select(0, src))
                if score:
                    self._norm_rows(x, self.final_norm, h, s)                       # all rows: the model's final norm in front of the head
                    self._nll_rows(h, targets[p0:p0 + M], nll[p0:p0 + M], s)
            new_pos = [st + T for st, T in zip(starts, lens)]
            if self.logits_process:
                for i in range(n):
                    self._write_history(rows[i], starts[i], ids[offs[i]:offs[i] + lens[i]])
            logits = self._head_rows(last, rows[0], new_pos[0], s) if one_row else self._head_rows(last, rows, new_pos, s)
        return logits, nll, offs, lens

    def prefill_batch(self, prompts, rows=None, starts=None, max_rows=4096):
        """Feed SEVERAL prompts at once: prompts[i] (1-D int64 ids, any length >= 1, 1 <= len(prompts) <= batch) goes into cache row rows[i]
        (default 0 .. n - 1; distinct) at positions starts[i] .. starts[i] + T_i - 1 (default 0; a None entry continues at self.pos[row]).
        Returns self.logits[rows]: the logits after each prompt's last token (the static buffer's rows, as prefill's).  All prompts are packed
        into one [sum T, hidden] activation and every layer runs ONCE at M = sum T through the launches of prefill -- gptq_rmsnorm_f16, the
        layer's PreparedLayer, gptq_add_rows_f16 -- with gptq_prompt_attn_batch_f16 (one segment per prompt, two launches) on kcb[li] / vcb[li];
        the last row of each prompt is gathered and the LM head runs once for those rows.  Above max_rows packed rows the work is done in
        passes of at most max_rows (the buffers grow to min(sum T, max_rows) rows and are shared with prefill); a prompt that straddles a pass
        boundary continues in the next pass at its advanced position.  Cache rows and positions of engine rows not named stay as they are.
        ValueError before anything is launched: an empty prompt, duplicate rows, a row outside the batch, positions beyond t_max.  Not
        graph-captured; nothing of `transformers` is involved.  Measured against a loop of prefill: profiles/prefill_batch/README.md."""
        return self._packed('prefill_batch', prompts, rows, starts, max_rows)[0]

    # -- scoring: how likely was the prompt?  The launches of prefill / prefill_batch, then the LM head of EVERY row with the cross-entropy inside ---
    def _nll_rows(self, h, targets, nll, s):
        """nll[m] = -log softmax(lm_head(h[m]))[targets[m]] for the already normalised rows h; a negative target gives 0.  gptq_lm_head_nll_f16
        (csrc/gemm8.hip: the tile GEMM with a cross-entropy epilogue -- the [M, vocab] logits never exist); a head the kernel declines (rc -6:
        hidden % 128 != 0; non-fp16, non-unit stride, misaligned) goes through torch.matmul + log_softmax in row chunks whose temporaries
        (fp16 logits + their fp32 log-softmax) stay under 64 MiB."""
        W, bias = self.lm_head, self.lm_head_bias
        M, N = h.shape[0], W.shape[0]
        ok = (W.dtype == torch.float16 and W.dim() == 2 and W.stride(1) == 1 and W.stride(0) % 8 == 0 and W.shape[1] == h.shape[1] and
              W.data_ptr() % 16 == 0 and (bias is None or (bias.dtype == torch.float16 and bias.is_contiguous() and bias.data_ptr() % 8 == 0)))
        if ok:
            need = self.lib.gptq_lm_head_nll_workspace_bytes(M, N)
            ws = self._nll_ws
            if ws is None or ws.numel() < need:
                ws = self._nll_ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.dev)
            rc = self.lib.gptq_lm_head_nll_f16(h.data_ptr(), h.stride(0), W.data_ptr(), W.stride(0), self.native.ptr(bias), targets.data_ptr(),
                                               nll.data_ptr(), None, None, M, N, W.shape[1], ws.data_ptr(), ws.numel(), s)
            if rc != -6:
                self.native.check(rc, 'gptq_lm_head_nll_f16')
                return
        chunk = max(1, (64 << 20) // (6 * N))
        for r0 in range(0, M, chunk):
            hc, tc = h[r0:r0 + chunk].to(W.dtype), targets[r0:r0 + chunk]
            z = torch.matmul(hc, W.t()) if bias is None else torch.addmm(bias, hc, W.t())
            picked = torch.log_softmax(z.float(), dim=-1).gather(1, tc.clamp(min=0)[:, None])[:, 0]
            nll[r0:r0 + chunk] = torch.where(tc < 0, torch.zeros_like(picked), -picked)

    def score(self, input_ids, row=0, start=0, max_rows=4096):
        """nll [T - 1] (float32, on the device): nll[t] = -log p(input_ids[t + 1] | input_ids[: t + 1]) -- what the reference's evaluation sums
        (llama.py:241-258: lm_head over all rows, shifted labels, CrossEntropyLoss), as the fp32 cross-entropy of the fp16 logits.  Runs the
        launches of prefill on cache row `row` from position `start` (None: continue at self.pos[row]), then the final norm and
        gptq_lm_head_nll_f16 over all rows; sequences longer than max_rows go in passes.  Afterwards the engine is in exactly the state
        prefill(input_ids, row, start) leaves -- cache rows, pos[row], logits[row] after the last token -- so a caller can score a prompt and go
        on generating.  T == 1 returns an empty tensor.  ValueError before anything is launched: an id outside [0, vocab), and every case
        prefill refuses."""
        ids = input_ids.reshape(-1) if (torch.is_tensor(input_ids) and (input_ids.dim() == 1 or (input_ids.dim() == 2 and input_ids.shape[0] == 1))) else None
        if ids is None or ids.numel() == 0:
            raise ValueError('DecodeEngine.score: input_ids must be a non-empty 1-D or [1, T] tensor')
        if not 0 <= int(row) < self.batch:
            raise ValueError('DecodeEngine.score: row %d outside the batch of %d' % (int(row), self.batch))
        _, nll, _, lens = self._packed('score', [ids], [row], [start], max_rows, score=True, one_row=True)
        return nll[:lens[0] - 1]

    def score_batch(self, prompts, rows=None, max_rows=4096):
        """score for SEVERAL prompts at once, with the packing of prefill_batch: one activation, one segment per prompt, every prompt from
        position 0 of its cache row (rows[i], default 0 .. n - 1), ONE gptq_lm_head_nll_f16 call per pass over all packed rows.  Returns a list
        of [T_i - 1] float32 tensors (views of one buffer) and leaves the state prefill_batch(prompts, rows) leaves.  ValueError as
        prefill_batch, and for an id outside [0, vocab)."""
        _, nll, offs, lens = self._packed('score_batch', prompts, rows, None, max_rows, score=True)
        return [nll[o:o + T - 1] for o, T in zip(offs, lens)]

    # -- speculative decoding: R consecutive tokens of EACH of the B sequences per step.  ONE mechanism: chunk = R is its B = 1 case (chunk_ids [R],
    # -- verify_out [R + 1]: row 0), batch_chunk = R the B >= 2 one (chunk_ids [B, R], verify_out [B, R + 1]); the public pairs differ in shapes only
    def _chunk_buffers(self):
        """[B R, .] activations, chunk_ids, chunk_logits [B R, vocab], the attention workspace, verify_out and the decode kernels' scratch for
        M = B R (and M = B: the plain step shares it); every layer must have a route for B R rows"""
        B, R, H, dev = self.batch, self.chunk_rows, self.hidden, self.dev
        M = B * R
        self.scratch = self._rows_scratch('chunk' if self.chunk else 'batch_chunk', (M, B))
        f16 = dict(dtype=torch.float16, device=dev)
        self.chunk_logits = torch.zeros((M, self.lm_head.shape[0]), **f16)
        self.chunk_bufs = dict(x=torch.zeros((M, H), **f16), x2=torch.zeros((M, H), **f16), h=torch.zeros((M, H), **f16),
                               qkv=torch.zeros((M, 3 * H), **f16), ab=torch.zeros((M, H), **f16), cb=torch.zeros((M, self.cb.shape[1]), **f16))
        self.chunk_attn_ws = torch.zeros(self.lib.gptq_decode_attn_chunk_batch_workspace_bytes(B, R, self.heads, self.head_dim, self.t_max),
                                         dtype=torch.uint8, device=dev)
        # the verify-greedy graph's result, read by the host in ONE copy per step: row b = [a_b, am_b[0 .. R - 1]]
        ids, out = torch.zeros((B, R), dtype=torch.int64, device=dev), torch.zeros((B, R + 1), dtype=torch.int64, device=dev)
        self.chunk_ids, self.verify_out = (ids[0], out[0]) if self.chunk else (ids, out)
        if not self.spec_sample:
            return
        # speculative sampling (gptq_spec_sample_batch_f16): the B R rows' setting (set_sampling: sequence b's in its R rows), their uniforms, the
        # draft model's logits rows [B (R - 1), vocab], and the kernel's workspace, per sequence [ticket, R records] -- zero once, a ticket
        # puts itself back
        f32 = dict(dtype=torch.float32, device=dev)
        self.chunk_temperature, self.chunk_top_p = torch.ones(M, **f32), torch.ones(M, **f32)
        self.chunk_top_k = torch.zeros(M, dtype=torch.int32, device=dev)
        self.chunk_u_accept, self.chunk_u_draw = torch.zeros(M, **f32), torch.zeros(M, **f32)
        self.chunk_draft_logits = torch.zeros((B * (R - 1), self.lm_head.shape[0]), **f16)
        self.spec_ws = torch.zeros(self.lib.gptq_spec_sample_batch_workspace_bytes(B, R) // 8, dtype=torch.int64, device=dev)

    def _step_chunk(self):
        """_step_rows at M = B R: row b R + r is token r of sequence b (chunk_ids[b, r] at position pos[b] + r); gptq_decode_attn_chunk_batch_f16 on
        kcb[li] / vcb[li] with pos as the DEVICE positions (pos[b] < 0: sequence b idles), the LM head for B R rows into chunk_logits (above 16
        rows: the stand-alone norm + the library matmul of lm_head_logits).  Does not advance pos."""
        slot_stride = self.kcb.stride(1)

        def attn(li, L, qkvb, ab, tab, s):
            rc = self.lib.gptq_decode_attn_chunk_batch_f16(qkvb.data_ptr(), qkvb.stride(0), self.batch, self.chunk_rows, self.pos.data_ptr(),
                                                           self.kcb[li].data_ptr(), self.vcb[li].data_ptr(), slot_stride, ab.data_ptr(), ab.stride(0),
                                                           self.chunk_attn_ws.data_ptr(), self.chunk_attn_ws.numel(), self.heads, self.head_dim,
                                                           self.t_max, L['theta'], self.scale, self.native.ptr(tab), s)
            self.native.check(rc, 'gptq_decode_attn_chunk_batch_f16')
        self._step_rows(self.chunk_bufs, self.chunk_ids.view(-1), attn, self.chunk_logits)

    def _need_chunk(self, what, batched=False):
        if not (self.batch_chunk if batched else self.chunk):
            raise ValueError('DecodeEngine.%s: the engine was built without %s=R' % (what, 'batch_chunk' if batched else 'chunk'))

    def _chunks_fit(self, what, active=None):
        """ValueError unless positions pos[b] .. pos[b] + R - 1 fit the cache for every sequence b -- of `active` (a list of B flags) when given,
        which exempts the others, wherever their positions are"""
        R = self.chunk_rows
        for b, p in enumerate(self.pos.tolist()):
            if (active is None or active[b]) and not 0 <= p <= self.t_max - R:
                raise ValueError('DecodeEngine.%s: positions %d .. %d of sequence %d do not fit the engine cache (%d)' % (what, p, p + R - 1, b, self.t_max))

    def _verify_rows(self, what, tokens):
        """verify and verify_batch: tokens is a list of B entries, entry b the 1 .. R ids of sequence b -- short ones are padded with copies of
        their last id -- or None for a sequence that idles: its position holds the kernel's idle mark (-1) during the step and comes back behind
        it.  Everything is checked (ValueError) before the upload of chunk_ids and the step."""
        B, R = self.batch, self.chunk_rows
        if not isinstance(tokens, (list, tuple)) or len(tokens) != B:
            raise ValueError('DecodeEngine.%s: tokens must be a list of %d entries (ids or None)' % (what, B))
        rows = []
        for t in tokens:
            if t is not None:
                t = [int(x) for x in (t.reshape(-1).tolist() if torch.is_tensor(t) else list(t))]
                if not 1 <= len(t) <= R:
                    raise ValueError('DecodeEngine.%s: 1 .. %d tokens per sequence, not %d' % (what, R, len(t)))
                t = t + [t[-1]] * (R - len(t))
            rows.append(t)
        self._chunks_fit(what, [t is not None for t in rows])
        with torch.no_grad(), torch.cuda.device(self.dev):
            self.chunk_ids.view(B, R).copy_(torch.tensor([t if t is not None else [0] * R for t in rows], dtype=torch.int64))
            idle = any(t is None for t in rows)
            if idle:
                pos = self.pos.clone()
                self.pos.masked_fill_(torch.tensor([t is None for t in rows]).to(self.dev), -1)
            self._step_chunk()
            if idle:
                self.pos.copy_(pos)

    def _accept_rows(self, what, ns, least):
        """accept and accept_batch: pos[b] += ns[b] for B counts in least .. R, checked (ValueError) before anything changes"""
        ns = [int(n) for n in ns] if isinstance(ns, (list, tuple)) else None
        if ns is None or len(ns) != self.batch or any(not least <= n <= self.chunk_rows for n in ns):
            raise ValueError('DecodeEngine.%s: needs %d counts in %d .. %d' % (what, self.batch, least, self.chunk_rows))
        for b, (p, n) in enumerate(zip(self.pos.tolist(), ns)):
            if n and p + n > self.t_max:
                raise ValueError('DecodeEngine.%s: position %d of sequence %d beyond the engine cache (%d)' % (what, p + n, b, self.t_max))
        self.pos.add_(torch.tensor(ns, dtype=torch.int64).to(self.dev))
        return self

    def verify(self, tokens):
        """chunk = R.  tokens: 1-D, 1 .. R ids -- the last accepted token followed by the drafts -- fed at positions pos .. pos + n - 1.  Returns
        chunk_logits[:n] (the static buffer: clone it to keep it): row i is the distribution after tokens[:i + 1].  Fewer than R tokens are padded
        with copies of the last one (their rows are computed and dropped).  pos is unchanged: accept(n) advances it.  Cache rows pos .. pos + R - 1
        are written; what lies beyond the accepted ones is stale by contract and overwritten by the next step.  ValueError, with nothing
        launched, when the chunk does not fit the cache."""
        self._need_chunk('verify')
        t = torch.as_tensor(tokens).reshape(-1)
        self._verify_rows('verify', [t])
        return self.chunk_logits[:int(t.numel())]

    def verify_batch(self, tokens):
        """batch_chunk = R.  tokens: a list of B entries, entry b what verify takes for sequence b, or None for a sequence that idles (nothing of
        its cache slot is read or written).  Returns chunk_logits viewed [B, R, vocab] (the static buffer: clone it to keep it): row [b, i] is the
        distribution after entry b's first i + 1 tokens; rows behind a short entry and the rows of an idle sequence mean nothing.  pos is
        unchanged: accept_batch advances it.  ValueError, with nothing launched, when an active sequence's chunk does not fit the cache."""
        self._need_chunk('verify_batch', batched=True)
        self._verify_rows('verify_batch', tokens)
        return self.chunk_logits.view(self.batch, self.batch_chunk, -1)

    def accept(self, n):
        """pos += n (1 .. R): the first n tokens of the last verify stay in the cache, the rest is stale"""
        self._need_chunk('accept')
        return self._accept_rows('accept', [n], 1)

    def accept_batch(self, ns):
        """pos[b] += ns[b]: accept per sequence; 0 for a sequence that idled"""
        self._need_chunk('accept_batch', batched=True)
        return self._accept_rows('accept_batch', ns, 0)

    def _verify_greedy_step(self):
        """_step_chunk and the greedy accept rule per sequence, entirely on the device: am = argmax of every row, a_b = the length of the longest
        prefix of sequence b's drafts with am[b, i] == chunk_ids[b, i + 1]; verify_out[b] = [a_b, am[b, 0 .. R - 1]] (the tokens a step emits are
        am[b, 0 .. a_b]); pos[b] += a_b + 1 -- with B >= 2 for the active sequences (0 <= pos[b] < t_max) only: an idle position stays as it is"""
        B, R = self.batch, self.chunk_rows
        self._step_chunk()
        am = torch.argmax(self.chunk_logits, dim=-1).view(B, R)
        ok = (am[:, :-1] == self.chunk_ids.view(B, R)[:, 1:]).to(torch.int64)
        a = torch.cumprod(ok, dim=1).sum(dim=1)
        out = self.verify_out.view(B, R + 1)
        out[:, 0].copy_(a)
        out[:, 1:].copy_(am)
        if B == 1:
            # nothing ever idles the one sequence of a chunk engine, and the mask's five element-wise nodes were measured: 9 us per replay of
            # the 7B-shaped verify graph on average, outside the spread of its repeats at 10 of 16 points (profiles/speculate/README.md)
            self.pos.add_(a + 1)
        else:
            active = ((self.pos >= 0) & (self.pos < self.t_max)).to(torch.int64)
            self.pos.add_((a + 1) * active)

    def _capture_verify(self, what, step, batched=False, keep_rng=False):
        """the ONE capture of the verify steps, which advance pos and are fed new chunk_ids behind the warm-up run.  ValueError for an engine of
        the other kind, or when the warm-up chunk does not fit the cache -- batched: an ACTIVE sequence's (0 <= pos[b] < t_max) only"""
        self._need_chunk(what, batched)
        self._chunks_fit(what, [0 <= p < self.t_max for p in self.pos.tolist()] if batched else None)
        return self._capture(step, (self.pos, self.chunk_ids), keep_rng)

    def capture_verify_greedy(self):
        """chunk = R.  Capture _verify_greedy_step into ONE hipGraph (verify_graph): a replay verifies chunk_ids at the device position and
        advances it by what was accepted; the host uploads chunk_ids and downloads verify_out once per step.  The capture runs the step once for
        real at the current position: cache rows pos .. pos + R - 1 of every layer are overwritten (rows at and beyond pos are stale by contract,
        so the history below pos is intact) and pos, chunk_ids are put back.  ValueError when the warm-up chunk does not fit the cache: capture
        earlier in the sequence, or before the prompt (engine_generate captures at pos = 0, in front of the prefill)."""
        self.verify_graph = self._capture_verify('capture_verify_greedy', self._verify_greedy_step)
        return self

    def capture_verify_greedy_batch(self):
        """batch_chunk = R.  capture_verify_greedy for the B sequences -- the same step, the same stored graph (verify_batch_graph reads it) --
        where only an active sequence's warm-up chunk has to fit; engine_generate_batch captures at pos = 0, in front of the prefill."""
        self.verify_graph = self._capture_verify('capture_verify_greedy_batch', self._verify_greedy_step, batched=True)
        return self

    # -- speculative SAMPLING: the verify step followed by the accept / resample rule of gptq_spec_sample_batch_f16 (csrc/spec_sample.hip), for the
    # -- B sequences in one launch; the chunk engine is its B = 1 case -----------------------------------------------------------------------
    def _need_spec_sample(self, what, batched):
        self._need_chunk(what, batched)
        if not self.spec_sample:
            raise ValueError('DecodeEngine.%s: the engine was built without spec_sample=True' % what)

    def _spec_sample_rows(self, draft_logits):
        """the kernel on chunk_logits / chunk_ids under the chunk rows' setting and the uniforms in chunk_u_accept / chunk_u_draw, for every active
        sequence b (0 <= pos[b] < t_max): verify_out[b] = [a_b, d_0 .. d_{a_b - 1}, t_a, ..] and pos[b] += a_b + 1, in one launch"""
        dl = self.chunk_draft_logits if draft_logits else None
        with self.native.on_device(self.dev):
            rc = self.lib.gptq_spec_sample_batch_f16(self.chunk_logits.data_ptr(), self.chunk_logits.stride(0), dl.data_ptr() if draft_logits else None,
                                                     dl.stride(0) if draft_logits else 0, self.batch, self.chunk_rows, self.chunk_logits.shape[1],
                                                     self.chunk_ids.data_ptr(), self.chunk_temperature.data_ptr(), self.chunk_top_k.data_ptr(),
                                                     self.chunk_top_p.data_ptr(), self.chunk_u_accept.data_ptr(), self.chunk_u_draw.data_ptr(),
                                                     self.pos.data_ptr(), self.t_max, self.verify_out.data_ptr(), self.spec_ws.data_ptr(),
                                                     self.spec_ws.numel() * 8, self.native.stream_ptr(self.dev))
        self.native.check(rc, 'gptq_spec_sample_batch_f16')

    def _verify_sample_step(self, draft_logits=False):
        """_step_chunk, fresh uniforms from torch's CUDA generator (inside a graph its Philox offset advances per replay as per eager call), the
        accept / resample launch"""
        self._step_chunk()
        self.chunk_u_accept.uniform_()
        self.chunk_u_draw.uniform_()
        self._spec_sample_rows(draft_logits)

    def _verify_sample_rows(self, what, tokens, draft_logits, u_accept, u_draw):
        """verify_sample and verify_sample_batch: tokens a list of B entries (2 .. R ids, or None: the sequence idles under the mark -1 and gets its
        position back), draft_logits None or a list of B fp16 [n_b - 1, vocab] tensors, the uniforms None or float32 [B, R].  Everything is checked
        (ValueError) before anything is uploaded or launched.  Returns one (a_b, tokens_b) per sequence, None for an idle one."""
        B, R, V = self.batch, self.chunk_rows, self.chunk_logits.shape[1]
        if not isinstance(tokens, (list, tuple)) or len(tokens) != B:
            raise ValueError('DecodeEngine.%s: tokens must be a list of %d entries (ids or None)' % (what, B))
        rows = []
        for t in tokens:
            if t is not None:
                t = [int(x) for x in (t.reshape(-1).tolist() if torch.is_tensor(t) else list(t))]
                if not 2 <= len(t) <= R:
                    raise ValueError('DecodeEngine.%s: 2 .. %d tokens per sequence, not %d' % (what, R, len(t)))
            rows.append(t)
        if draft_logits is not None:
            if not isinstance(draft_logits, (list, tuple)) or len(draft_logits) != B:
                raise ValueError('DecodeEngine.%s: draft_logits must be None or a list of %d tensors' % (what, B))
            for t, dl in zip(rows, draft_logits):
                if t is not None and (not torch.is_tensor(dl) or dl.shape != (len(t) - 1, V) or dl.dtype != torch.float16):
                    raise ValueError('DecodeEngine.%s: draft_logits must be fp16 [%d, %d]' % (what, len(t) - 1, V))
        for name, u in (('u_accept', u_accept), ('u_draw', u_draw)):
            if u is not None and (not torch.is_tensor(u) or u.dtype != torch.float32 or u.shape != (B, R)):
                raise ValueError('DecodeEngine.%s: %s must be float32 %s' % (what, name, [B, R] if self.batch_chunk else [R]))
        active = [t is not None for t in rows]
        self._chunks_fit(what, active)
        pos = self.pos.tolist()
        with torch.no_grad(), torch.cuda.device(self.dev):
            self.chunk_ids.view(B, R).copy_(torch.tensor([t + [t[-1]] * (R - len(t)) if t is not None else [0] * R for t in rows], dtype=torch.int64))
            if draft_logits is not None:
                rows_q = self.chunk_draft_logits.view(B, R - 1, V)
                for b, t in enumerate(rows):
                    if t is not None:
                        n = len(t)
                        rows_q[b, :n - 1].copy_(draft_logits[b])
                        if n < R:                                # a padding row's draft is a point mass: -inf everywhere but at the token
                            rows_q[b, n - 1:].fill_(float('-inf'))
                            rows_q[b, n - 1:, t[-1]] = 0.0
            if not all(active):
                self.pos.masked_fill_(torch.tensor([not x for x in active]).to(self.dev), -1)
            self._step_chunk()
            for buf, u in ((self.chunk_u_accept, u_accept), (self.chunk_u_draw, u_draw)):
                if u is None:
                    buf.uniform_()
                else:
                    buf.copy_(u.reshape(-1))
            self._spec_sample_rows(draft_logits is not None)
            res = self.verify_out.view(B, R + 1).tolist()
            out = []
            for b, t in enumerate(rows):
                if t is not None:
                    a = min(res[b][0], len(t) - 1)               # (padding rows do not count; their tokens are dropped)
                    out.append((a, res[b][1:a + 2]))
                    pos[b] += a + 1
                else:
                    out.append(None)
            if not all(active) or any(t is not None and o[0] < r[0] for t, o, r in zip(rows, out, res)):
                self.pos.copy_(torch.tensor(pos, dtype=torch.int64))
        return out

    def verify_sample(self, tokens, draft_logits=None, u_accept=None, u_draw=None):
        """Speculative sampling of one step, eagerly.  tokens: 1-D, 2 .. R ids -- the last accepted token followed by the drafts, fed at positions
        pos .. pos + n - 1 and padded as verify pads (a step of fewer than R tokens runs as R rows; the copies of the last draft behind it can only
        be accepted after it, and what they emit is dropped).  draft_logits: [n - 1, vocab] fp16 rows the drafts were drawn from under the engine's
        setting (set_sampling), None: every draft is a point mass.  u_accept / u_draw: float32 [R] on the device; None draws them from torch's CUDA
        generator.  Returns (a, tokens): a accepted drafts and the a + 1 ids the step emits (a list of ints); pos has advanced by a + 1."""
        self._need_spec_sample('verify_sample', False)
        row = lambda u: u.unsqueeze(0) if torch.is_tensor(u) and u.dim() == 1 else u
        return self._verify_sample_rows('verify_sample', [torch.as_tensor(tokens)], None if draft_logits is None else [draft_logits], row(u_accept),
                                        row(u_draw))[0]

    def verify_sample_batch(self, tokens, draft_logits=None, u_accept=None, u_draw=None):
        """batch_chunk = R with spec_sample.  verify_sample for the B sequences in ONE step: tokens a list of B entries, entry b what verify_sample
        takes for sequence b (2 .. R ids, padded alike) or None for a sequence that idles (nothing of its cache slot, its position or its row of
        verify_out changes).  draft_logits: None, or a list of B fp16 tensors [n_b - 1, vocab] (an idle sequence's entry is ignored) under the
        sequences' own settings.  u_accept / u_draw: float32 [B, R] on the device; None draws them from torch's CUDA generator.  Returns a list of
        B entries (a_b, tokens_b), None for an idle sequence; pos[b] has advanced by a_b + 1.  ValueError, with nothing uploaded or launched: an
        engine without spec_sample, a wrong count or shape, an active chunk that does not fit the cache."""
        self._need_spec_sample('verify_sample_batch', True)
        return self._verify_sample_rows('verify_sample_batch', tokens, draft_logits, u_accept, u_draw)

    def capture_verify_sample(self, draft_logits=False):
        """capture _verify_sample_step into ONE hipGraph: a replay verifies chunk_ids (and, draft_logits=True, reads the static chunk_draft_logits)
        at the device position, draws fresh uniforms, and leaves [a, tokens] in verify_out with pos advanced.  One capture serves every setting
        (set_sampling).  The generator's state is put back behind the warm-up run, as capture_sample_native does; the cache contract and the
        ValueError are capture_verify_greedy's."""
        g = self._capture_verify('capture_verify_sample', lambda: self._verify_sample_step(bool(draft_logits)), keep_rng=True)
        self.verify_sample_graphs[bool(draft_logits)] = g
        return g

    def capture_verify_sample_batch(self, draft_logits=False):
        """batch_chunk = R with spec_sample.  capture_verify_sample for the B sequences -- the same step, the same verify_sample_graphs -- under
        the cache contract of capture_verify_greedy_batch: only an active sequence's warm-up chunk has to fit, an idle position stays."""
        self._need_spec_sample('capture_verify_sample_batch', True)
        g = self._capture_verify('capture_verify_sample_batch', lambda: self._verify_sample_step(bool(draft_logits)), batched=True, keep_rng=True)
        self.verify_sample_graphs[bool(draft_logits)] = g
        return g

    def _draft_step(self, target):
        """the self-feeding sampling step of a DRAFT engine in front of `target` (a speculative-sampling engine of the same batch B and
        vocabulary): as _sample_native_step, and the step's [B, vocab] logits -- what the tokens were drawn from -- go into draft row stepc of
        every sequence of target.chunk_draft_logits.  (A draft engine has no processors: _self_feeding_step's process call does nothing here.)"""
        def choose():
            B, V = self.logits.shape
            target.chunk_draft_logits.view(B, -1, V).index_copy_(1, self.stepc, self.logits.unsqueeze(1))
            self.u.uniform_()
            self.sample_logits(self.logits, out=self.ids, u=self.u)
        self._self_feeding_step(choose)

    def capture_draft_step(self, target):
        """capture _draft_step once for `target`: at most R - 1 replays (R the target's chunk rows) between two resets of stepc.  ValueError for
        a target that does not sample speculatively, or of another batch, vocabulary or device."""
        if (not getattr(target, 'spec_sample', False) or self.batch != target.batch or target.chunk_draft_logits.shape[1] != self.logits.shape[1] or
                target.dev != self.dev):
            raise ValueError('DecodeEngine.capture_draft_step: needs a target engine with speculative sampling, of the same batch and vocabulary, '
                             'on one device')
        self.draft_graph = self._capture_rows(lambda: self._draft_step(target), keep_rng=True)
        return self.draft_graph

    def graph_for(self, kind, draft_logits=False):
        """THE place that hands out the graphs of the generation drivers: the captured graph of `kind` -- 'greedy' (batch 1: capture_greedy),
        'greedy_rows', 'sample_native', 'verify_greedy', 'verify_sample' (draft_logits: the one that reads the draft model's logits rows), 'beam' --,
        captured by the public capture_* method on first use.  A capture warms up with a real step, which writes the cache rows at pos: pos is
        put to 0 first, so that the step fits whatever an earlier sequence left there.  A driver therefore asks for EVERY graph it will need
        BEFORE its prompt enters the cache: behind a prompt, the warm-up step at position 0 would overwrite the prompt's first cache row, and
        this method must not be called there."""
        with_q = bool(draft_logits)
        held, capture = {
            'greedy': (lambda: self.greedy_graph, self.capture_greedy),
            'greedy_rows': (lambda: self.greedy_rows_graph, self.capture_greedy_rows),
            'sample_native': (lambda: self.sample_native_graph, self.capture_sample_native),
            'verify_greedy': (lambda: self.verify_graph, self.capture_verify_greedy_batch if self.batch_chunk else self.capture_verify_greedy),
            'verify_sample': (lambda: self.verify_sample_graphs.get(with_q), lambda: (
                self.capture_verify_sample_batch if self.batch_chunk else self.capture_verify_sample)(draft_logits=with_q)),
            'beam': (lambda: self.beam_graph, self.capture_beam_step),
        }[kind]
        if held() is None:
            self.pos.zero_()
            capture()
        return held()

    def decode(self, token):
        """one token per row in ([batch] ids), logits [batch, vocab] out (the static buffer: clone it to keep it).  An engine built with
        logits_process=True returns the PROCESSED logits (set_logits_process) and appends the tokens to its history; one built with constrain
        advances the rows' automata by the tokens and returns the logits MASKED under the new states (set_constraint)."""
        if torch.is_tensor(token):
            self.ids.copy_(token.reshape(self.batch))
        else:
            self.ids.fill_(int(token))
        with torch.no_grad():
            if self.graph is not None:
                self.graph.replay()
            else:
                self._step()
            self._process_step()
            self._constrain_step()
        return self.logits


def perplexity(model, input_ids, seqlen=2048, engine=None, batch=1):
    """The reference's quality gate (llama_eval, llama.py:173-261) on the engine: input_ids (any shape; the caller brings the ids -- no dataset,
    tokenizer or network here) is cut into numel // seqlen segments of seqlen tokens (llama.py:178), every segment is scored from position 0
    (DecodeEngine.score; batch > 1: score_batch, `batch` segments per call) and the results are
        nll_sum, tokens   sum and number of the per-token negative log-likelihoods (seqlen - 1 targets per segment),
        ppl               exp(nll_sum / tokens),
        ppl_reference     the reference's own figure: per segment the MEAN over its seqlen - 1 targets (CrossEntropyLoss, llama.py:254-255)
                          times seqlen (llama.py:256), summed and divided by nsamples * seqlen before the exp (llama.py:258) -- it weighs
                          every segment's mean as if the segment had seqlen targets.
    engine=None builds a DecodeEngine(model, t_max=seqlen, batch=batch)."""
    ids = input_ids.reshape(-1)
    seqlen, batch = int(seqlen), int(batch)
    nsamples = ids.numel() // seqlen
    if seqlen < 2 or nsamples < 1:
        raise ValueError('perplexity: needs seqlen >= 2 and at least seqlen ids')
    if engine is None:
        engine = DecodeEngine(model, t_max=seqlen, batch=batch)
    if batch < 1 or batch > engine.batch:
        raise ValueError('perplexity: batch %d for an engine of batch %d' % (batch, engine.batch))
    segments = [ids[i * seqlen:(i + 1) * seqlen] for i in range(nsamples)]
    sums = []
    for i in range(0, nsamples, batch):
        group = segments[i:i + batch]
        nlls = [engine.score(group[0], row=0, start=0)] if batch == 1 else engine.score_batch(group)
        sums.extend(v.double().sum() for v in nlls)
    sums = torch.stack(sums).cpu()                                     # [nsamples] float64
    tokens = nsamples * (seqlen - 1)
    nll_sum = float(sums.sum())
    reference = float((sums / (seqlen - 1) * seqlen).sum() / (nsamples * seqlen))
    return dict(nll_sum=nll_sum, tokens=tokens, ppl=math.exp(nll_sum / tokens), ppl_reference=math.exp(reference))


def _cache_layer_kv(cache, li):
    """(keys, values) [1, heads, T, head_dim] of layer li from a transformers cache (5.x: cache.layers[li].keys)."""
    layers = getattr(cache, 'layers', None)
    if layers is not None and hasattr(layers[li], 'keys'):
        return layers[li].keys, layers[li].values
    kv = cache[li]
    return kv[0], kv[1]


def _prompt_into_engine(model, input_ids, eng, prefill):
    """the prompt of engine_generate ([1, T] ids) into the engine's cache, pos = T; returns the logits after its last token.  'engine':
    DecodeEngine.prefill; 'hf': once through the HF model (the drop-in modules' prefill path), its KV cache copied into the engine's"""
    T = input_ids.shape[1]
    if prefill == 'engine':
        return eng.prefill(input_ids[0], start=0)
    from transformers.cache_utils import DynamicCache
    cache = DynamicCache(config=model.config)
    out = model(input_ids, past_key_values=cache, use_cache=True)
    fp8 = eng.kv_cache == 'fp8'
    if fp8:                                                      # the module cache goes through the staging layer, as the engine's own prefill does
        table, s = (eng.native.PromptSeg * 1)(eng.native.PromptSeg(0, T, 0, 0)), eng.native.stream_ptr(eng.dev)
    for li in range(len(eng.layers)):
        k, v = _cache_layer_kv(cache, li)
        kc, vc = (eng.kst[0], eng.vst[0]) if fp8 else (eng.kc[li], eng.vc[li])
        kc[:T].copy_(k[0].transpose(0, 1).reshape(T, -1))
        vc[:T].copy_(v[0].transpose(0, 1).reshape(T, -1))
        if fp8:
            eng._kv8_store(li, table, 1, s)
    eng.pos.fill_(T)
    if eng.logits_process:
        eng.set_history(0, input_ids[0])
    return out.logits[0, -1]


def _cut_after_eos(gen, eos_token_id):
    """the 1-D id tensor gen up to and including its first eos_token_id (None, or not there: all of it)"""
    if eos_token_id is not None:
        at = (gen == eos_token_id).nonzero()
        if at.numel():
            return gen[:int(at[0]) + 1]
    return gen


def _sampling_settings(what, sample):
    """the `sample` argument of engine_generate / engine_generate_batch as keywords of DecodeEngine.set_sampling (which validates the values)"""
    if not isinstance(sample, dict):
        raise ValueError('%s: sample must be None or a dict with the keys temperature, top_k, top_p' % what)
    unknown = sorted(set(sample) - {'temperature', 'top_k', 'top_p'} - set(_PROCESS_NEUTRAL))
    if unknown:
        raise ValueError('%s: unknown sampling keys %r' % (what, unknown))
    return {k: v for k, v in sample.items() if k not in _PROCESS_NEUTRAL}


_PROCESS_NEUTRAL = dict(repetition_penalty=1.0, presence_penalty=0.0, min_new_tokens=0, logit_bias=None)


def _process_settings(sample):
    """the logit-processor keys of the `sample` argument as keywords of DecodeEngine.set_logits_process (which validates the values), or None
    when every one of them is absent or neutral (1.0, 0.0, 0, None / empty -- also as one neutral value per prompt): then nothing is processed"""
    def neutral(k, v):
        if k == 'logit_bias':
            return v is None or (isinstance(v, (dict, list, tuple)) and len(v) == 0)
        vals = v.tolist() if torch.is_tensor(v) else v
        vals = list(vals) if isinstance(vals, (list, tuple)) else [vals]
        return all(isinstance(x, (int, float)) and not isinstance(x, bool) and x == _PROCESS_NEUTRAL[k] for x in vals)
    keys = {k: sample[k] for k in _PROCESS_NEUTRAL if k in sample}
    return None if all(neutral(k, v) for k, v in keys.items()) else keys


def prompt_lookup_draft(tokens, k, max_ngram=3):
    """Draft k tokens for speculative decoding from the sequence itself (prompt lookup): find the MOST RECENT earlier occurrence of the last n
    tokens, trying n = max_ngram down to 1, and propose the tokens that followed it; when that run ends before k tokens (the match sits near the
    end) the lookup continues from the sequence extended by the proposal; without any match the last token is repeated.  Pure host code:
    tokens is a list or a numpy array of ids, the result a list of exactly k ints."""
    seq = list(tokens) if isinstance(tokens, list) else [int(t) for t in (tokens.tolist() if hasattr(tokens, 'tolist') else tokens)]
    k, max_ngram = int(k), int(max_ngram)
    if not seq or k < 0 or max_ngram < 1:
        raise ValueError('prompt_lookup_draft: needs a non-empty sequence, k >= 0 and max_ngram >= 1')
    out = []
    while len(out) < k:
        L = len(seq)
        rev = seq[::-1]                                          # rev[j] = seq[L - 1 - j]: list.index walks it at C speed
        last, nmax = rev[0], min(max_ngram, L - 1)
        # ONE pass over the earlier occurrences of the last token, most recent first: at each, how many tokens in front of it agree with the
        # tail; the first occurrence that reaches n tokens is the most recent match of the n-gram.  It ends at the first full-length match.
        best_n, best_j, j = 0, 0, 0
        while best_n < nmax:
            try:
                j = rev.index(last, j + 1)
            except ValueError:
                break
            n = 1
            while n < nmax and j + n < L and rev[j + n] == rev[n]:
                n += 1
            if n > best_n:
                best_n, best_j = n, j
        run = seq[L - best_j:L - best_j + (k - len(out))] if best_n else [last]
        out.extend(run)
        seq.extend(run)
    return out


def _speculate_settings(speculate, what='engine_generate'):
    """the `speculate` argument of `what` (engine_generate / engine_generate_batch): (k, max_ngram, draft) -- every key optional"""
    if not isinstance(speculate, dict):
        raise ValueError('%s: speculate must be None or a dict with the keys k, max_ngram, draft' % what)
    unknown = sorted(set(speculate) - {'k', 'max_ngram', 'draft', 'sample', 'draft_model'})
    if unknown:
        raise ValueError('%s: unknown speculation keys %r' % (what, unknown))
    k, max_ngram, draft = speculate.get('k', 4), speculate.get('max_ngram', 3), speculate.get('draft')
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_BATCH - 1:
        raise ValueError('%s: speculate k must be 1 .. %d, not %r' % (what, MAX_BATCH - 1, k))
    if isinstance(max_ngram, bool) or not isinstance(max_ngram, int) or max_ngram < 1:
        raise ValueError('%s: speculate max_ngram must be a positive int, not %r' % (what, max_ngram))
    if draft is not None and not callable(draft):
        raise ValueError('%s: speculate draft must be a callable (tokens_so_far, k) -> k ids' % what)
    return k, max_ngram, draft


def _speculate_sampling(speculate, model, what):
    """the keys of `speculate` that ask for speculative SAMPLING and for a draft MODEL: (sampling settings or None, draft model or None)"""
    sample, draft_model = speculate.get('sample'), speculate.get('draft_model')
    settings = None if sample is None else _sampling_settings(what, sample)
    if sample is not None and _process_settings(sample) is not None:
        raise ValueError('%s: logit processors (%s) under speculate= are not built yet: the verify step does not apply them' % (
            what, ', '.join(sorted(_PROCESS_NEUTRAL))))
    if draft_model is not None:
        if speculate.get('draft') is not None:
            raise ValueError('%s: speculate takes draft or draft_model, not both' % what)
        dv, tv = getattr(getattr(draft_model, 'config', None), 'vocab_size', None), model.config.vocab_size
        if dv != tv:
            raise ValueError('%s: the draft model has a vocabulary of %r tokens, the model one of %d' % (what, dv, tv))
    return settings, draft_model


def _generation_settings(what, model, sample, speculate, engine):
    """what the arguments sample= / speculate= / engine= of `what` (engine_generate / engine_generate_batch) ask for, validated ONCE for both:
    (sampling settings or None, processor settings or None, (k, max_ngram, draft, sampling settings or None, draft model or None) or None)"""
    settings = None if sample is None else _sampling_settings(what, sample)
    proc = None if sample is None else _process_settings(sample)
    spec = None
    if speculate is not None:
        if sample is not None:
            raise ValueError('%s: speculate and the sample argument exclude each other (speculative sampling: the key sample inside '
                             'speculate)' % what)
        spec = _speculate_settings(speculate, what) + _speculate_sampling(speculate, model, what)
    if engine is not None and proc is not None and not engine.logits_process:
        raise ValueError('%s: %s need an engine built with logits_process=True' % (what, ', '.join(sorted(proc))))
    return settings, proc, spec


def _draft_model_engine(eng, draft_model, settings):
    """the engine of the draft model that belongs to the target engine `eng`, of its batch: built and captured once (plain step, draft step), kept
    on eng"""
    kept = eng._draft_engine
    if kept is None or kept[0] is not draft_model:
        deng = DecodeEngine(draft_model, t_max=eng.t_max, batch=eng.batch).capture()
        deng.capture_draft_step(eng)
        kept = eng._draft_engine = (draft_model, deng)
    deng = kept[1]
    deng.set_sampling(**(settings if settings is not None else dict(temperature=0)))
    return deng


def _cut(tokens, left, eos_token_id):
    """the first `left` ids of the list `tokens`, up to and including the first eos_token_id: (those ids, whether the eos is among them)"""
    tokens = tokens[:left]
    if eos_token_id is not None and eos_token_id in tokens:
        return tokens[:tokens.index(eos_token_id) + 1], True
    return tokens, False


def _host_drafts(what, eng, k, max_ngram, draft):
    """the HOST draft source of _generate_speculative: draft(tokens_so_far: list[int], k) -> k ids for every active sequence (default:
    prompt_lookup_draft), behind the sequence's last token; ONE upload of chunk_ids for all sequences"""
    if draft is None:
        draft = lambda toks, m: prompt_lookup_draft(toks, m, max_ngram)

    def fill(seqs, done):
        ids = []
        for seq, idle in zip(seqs, done):
            d = [0] * k if idle else [int(t) for t in draft(seq, k)]     # (the draft reads the list, it must not change it)
            if len(d) != k:
                raise ValueError('%s: the draft returned %d ids for k = %d' % (what, len(d), k))
            ids.append([0 if idle else seq[-1]] + d)
        eng.chunk_ids.view(len(seqs), k + 1).copy_(torch.tensor(ids, dtype=torch.int64))
    return fill


def _model_drafts(eng, deng, k, lens):
    """the draft-MODEL source of _generate_speculative: the draft engine `deng` of the target's batch holds prompt b (lens[b] tokens) in cache row b.
    Per step, the sequences whose last step accepted all k drafts first consume the one token they have not seen (d_k) in a plain step, the
    others idling far below position 0; then every active sequence is put at its last token, and k replays of the captured draft step consume it
    and d_1 .. d_{k-1} and draw d_1 .. d_k -- chunk_ids[:, 1:] and the rows of chunk_draft_logits are written on the device.  Finished
    sequences idle throughout."""
    n = len(lens)
    valid = list(lens)                                           # deng's position behind its last drafts: row b's cache is seq b's up to there at most
    far = -(eng.t_max + 1)                                       # (a step adds 1 to every position: still negative after the k draft steps)

    def fill(seqs, done):
        L = [len(seq) for seq in seqs]
        seen = [min(l - 1, v) for l, v in zip(L, valid)]         # tokens of seq b it has consumed; behind a rejection its later rows are stale
        unseen = [not d and sn < l - 1 for d, sn, l in zip(done, seen, L)]
        if any(unseen):
            deng.pos.copy_(torch.tensor([sn if u else far for sn, u in zip(seen, unseen)], dtype=torch.int64))
            deng.decode(torch.tensor([seq[sn] if u else 0 for seq, sn, u in zip(seqs, seen, unseen)], dtype=torch.int64))
        last = torch.tensor([0 if d else seq[-1] for seq, d in zip(seqs, done)], dtype=torch.int64)
        deng.pos.copy_(torch.tensor([far if d else l - 1 for l, d in zip(L, done)], dtype=torch.int64))
        deng.ids.copy_(last)
        deng.stepc.zero_()
        for _ in range(k):
            deng.draft_graph.replay()
        ids = eng.chunk_ids.view(n, k + 1)
        ids[:, 0].copy_(last)
        ids[:, 1:].copy_(deng.stream_rows[:k].t())
        for b in range(n):
            if not done[b]:
                valid[b] = L[b] + k - 1
    return fill


def _self_feeding_tail(eng, graph, first, n, eos=None, record=None):
    """THE tail loop of every generation driver.  graph: a captured self-feeding step of `eng`; first: the B tokens chosen behind the prompts
    (int64 on the device), which the first replay consumes; n >= 1: tokens wanted per row, `first` included; eos: None, an id or a list of
    ids.  Replays in bursts of min(16, what remains) -- the host looks at the stream between bursts only -- until n tokens per row exist or
    every row has shown an eos.  record = (buffer [., B], the row the first replay writes): where the step keeps its choices; None: stream_rows
    from row 0, with stepc put to 0.  Returns the stream [done, B] with `first` in front: done - 1 replays have run."""
    if record is None:
        eng.stepc.zero_()
        record = (eng.stream_rows, 0)
    rows, r0 = record
    eng.ids.copy_(first)
    eos_t = None if eos is None else torch.tensor(eos, dtype=torch.int64, device=first.device).reshape(-1)
    hit = None if eos_t is None else torch.isin(first, eos_t)
    done = 1
    while done < n and not (hit is not None and bool(hit.all())):
        burst = min(16, n - done)
        for _ in range(burst):
            graph.replay()
        if hit is not None:
            hit = hit | torch.isin(rows[r0 + done - 1:r0 + done - 1 + burst], eos_t).any(dim=0)
        done += burst
    return torch.cat([first.unsqueeze(0), rows[r0:r0 + done - 1]])


def _generate_speculative(eng, prompts, first, max_new_tokens, eos_token_id, k, graph, drafts, finish):
    """The ONE speculative loop, for n >= 1 sequences: engine_generate(speculate=...) is n = 1 on a chunk engine, engine_generate_batch(speculate=...)
    n >= 2 on a batch_chunk engine.  prompts: n id lists already in the engine's cache; first: the token chosen behind each.  Per step: who is
    active -- a sequence that hit its eos or its length idles (position -1) --; drafts(seqs, done) puts chunk_ids on the device (_host_drafts /
    _model_drafts); ONE replay of `graph` (verify-greedy or verify-sample); ONE download of verify_out; every active sequence appends its
    a_b + 1 tokens, cut at its length and its eos.  It ends when no active sequence has two tokens left or an active chunk no longer fits the
    cache; finish(seqs, left) -> one id list per sequence then runs the caller's single-step graph for what remains and leaves the positions.
    Returns (generated ids per sequence, dict(steps, emitted=[per sequence], accepted=[per sequence: per step]))."""
    n, R = len(prompts), k + 1
    seqs = [p + [f] for p, f in zip(prompts, first)]             # every token so far; the last one is not in the cache yet: pos = len - 1
    gens = [[f] for f in first]
    done = [(eos_token_id is not None and f == eos_token_id) or max_new_tokens <= 1 for f in first]
    accepted, steps = [[] for _ in range(n)], 0
    marked = [False] * n                                         # sequences whose device position holds the idle mark
    while True:
        active = [b for b in range(n) if not done[b]]
        if not active or all(max_new_tokens - len(gens[b]) < 2 for b in active) or any(len(seqs[b]) - 1 + R > eng.t_max for b in active):
            break
        for b in range(n):
            if done[b] and not marked[b]:
                eng.pos[b:b + 1].fill_(-1)
                marked[b] = True
        drafts(seqs, done)
        graph.replay()
        res = eng.verify_out.view(n, R + 1).tolist()             # one copy per step: row b = [a_b, the a_b + 1 tokens of its step, ...]
        steps += 1
        for b in active:
            a = res[b][0]
            new, hit = _cut(res[b][1:a + 2], max_new_tokens - len(gens[b]), eos_token_id)
            accepted[b].append(a)
            gens[b].extend(new)
            seqs[b].extend(new)
            done[b] = hit or len(gens[b]) >= max_new_tokens
    stats = dict(steps=steps, emitted=[len(g) - 1 for g in gens], accepted=accepted)
    left = [0 if done[b] else max_new_tokens - len(gens[b]) for b in range(n)]
    for b, tail in enumerate(finish(seqs, left)):
        gens[b].extend(_cut(tail, left[b], eos_token_id)[0])
    return gens, stats


def _speculate_rows(what, eng, prompts, into, max_new_tokens, eos_token_id, k, max_ngram, draft, settings, draft_model):
    """_generate_rows with speculation: what _generate_speculative needs for the n sequences of a chunk (n = 1) or batch_chunk engine.
    settings None: the verify-greedy graph, the first tokens by argmax, the capture_greedy_rows graph for the tail.  settings (one value for all
    or one per prompt): the verify-sample graph -- with the draft model's logits rows when a draft model is given, point-mass drafts otherwise
    --, the first tokens by sample_logits, the tail by the capture_sample_native graph.
    draft_model: _model_drafts on a DecodeEngine of this batch, under the same settings (greedily without them); else _host_drafts.
    Afterwards every position is that of the sequence's last token, the one not consumed yet, and eng.spec_stats describes the run."""
    n = len(prompts)
    if settings is None:
        graph, tail = eng.graph_for('verify_greedy'), eng.graph_for('greedy_rows')
    else:
        eng.set_sampling(**settings)                             # (validates before anything changes)
        graph, tail = eng.graph_for('verify_sample', draft_logits=draft_model is not None), eng.graph_for('sample_native')
    deng = None if draft_model is None else _draft_model_engine(eng, draft_model, settings)
    logits = into(eng)
    first = (logits.argmax(dim=-1) if settings is None else eng.sample_logits(logits.to(torch.float16).contiguous())).tolist()
    if deng is not None:
        into(deng)
        drafts = _model_drafts(eng, deng, k, [int(p.numel()) for p in prompts])
    else:
        drafts = _host_drafts(what, eng, k, max_ngram, draft)

    def finish(seqs, left):
        if max(left) <= 0:
            return [[]] * n
        far = -(eng.t_max + 1)                                   # (a step adds 1 to every position: still negative after the tail)
        eng.pos.copy_(torch.tensor([len(s) - 1 if m else far for s, m in zip(seqs, left)], dtype=torch.int64))
        last = torch.tensor([s[-1] if m else 0 for s, m in zip(seqs, left)], dtype=torch.int64, device=eng.dev)
        return _self_feeding_tail(eng, tail, last, max(left) + 1)[1:].t().tolist()      # [row][step]: no eos, the exact count
    gens, eng.spec_stats = _generate_speculative(eng, [[int(t) for t in p.tolist()] for p in prompts], first, max_new_tokens, eos_token_id, k,
                                                 graph, drafts, finish)
    eng.pos.copy_(torch.tensor([p.numel() + len(g) - 1 for p, g in zip(prompts, gens)], dtype=torch.int64))
    return [torch.tensor(g, dtype=torch.int64) for g in gens]


def _logprobs_setting(what, logprobs, speculate, engine):
    """the logprobs= argument of `what` (engine_generate / engine_generate_batch), validated: None or K in 0 .. 32; ValueError under speculate=,
    and for an engine passed in that has beam search, no logprobs flag or a smaller one"""
    if logprobs is None:
        return None
    if isinstance(logprobs, bool) or not isinstance(logprobs, int) or not 0 <= logprobs <= MAX_LOGPROBS:
        raise ValueError('%s: logprobs must be None or an int in 0 .. %d, not %r' % (what, MAX_LOGPROBS, logprobs))
    if speculate is not None:
        raise ValueError('%s: logprobs together with speculate is not built yet (records of a verify step)' % what)
    if engine is not None:
        if engine.beam_search:
            raise ValueError('%s: logprobs on a beam-search engine is not built yet' % what)
        if engine.logprobs is None or engine.logprobs < logprobs:
            raise ValueError('%s: logprobs = %d needs an engine built with logprobs >= %d (this one: %r)' % (what, logprobs, logprobs, engine.logprobs))
    return logprobs


def _constrain_setting(what, constrain, n, speculate, engine):
    """the constrain= argument of `what` (engine_generate / engine_generate_batch), validated: None, or one automaton (or None) per prompt.
    ValueError under speculate= and for an engine passed in without the flag"""
    if constrain is None:
        return None
    from .constrain import TokenDFA
    dfas = list(constrain) if isinstance(constrain, (list, tuple)) else [constrain] * n
    if len(dfas) != n or any(d is not None and not isinstance(d, TokenDFA) for d in dfas):
        raise ValueError('%s: constrain must be a TokenDFA or a list of %d of them (None: that prompt is unconstrained)' % (what, n))
    if speculate is not None:
        raise ValueError('%s: constrain together with speculate is not built yet (a verify step needs the state chain per row)' % what)
    if engine is not None and engine.constrain is None:
        raise ValueError('%s: constrain needs an engine built with constrain=' % what)
    return dfas


def _kv_cache_setting(what, kv_cache, speculate, engine):
    """the kv_cache= argument of `what` (engine_generate / engine_generate_batch), validated: 'fp16' or 'fp8'; ValueError for 'fp8' under
    speculate= and for an engine passed in of the other kind"""
    if kv_cache not in ('fp16', 'fp8'):
        raise ValueError("%s: kv_cache must be 'fp16' or 'fp8', not %r" % (what, kv_cache))
    if kv_cache == 'fp8' and speculate is not None:
        raise ValueError("%s: kv_cache='fp8' together with speculate is not built yet (the verify step's chunk attention reads an fp16 cache)" % what)
    if engine is not None and engine.kv_cache != kv_cache:
        raise ValueError('%s: kv_cache=%r for an engine built with kv_cache=%r' % (what, kv_cache, engine.kv_cache))


def _constrain_capacity(dfas):
    """the constrain= argument of a DecodeEngine that holds exactly these automata (None: no flag)"""
    if dfas is None:
        return None
    distinct = {id(d): d for d in dfas if d is not None}.values()
    return dict(states=max(1, sum(d.n_states for d in distinct)), classes=max([d.n_classes for d in distinct] + [1]))


def _generate_rows(what, eng, prompts, into, max_new_tokens, eos_token_id, settings, proc, spec, one_prompt=False, logprobs=None, dfas=None):
    """THE generation driver behind engine_generate (one prompt) and engine_generate_batch: prompts are n = eng.batch 1-D id tensors,
    into(engine) puts them into that engine's cache from position 0 and returns the [n, vocab] logits behind their last tokens.  In this order:
    the settings go into the engine; every graph the run will need is taken from graph_for, while no prompt is in the cache yet; the prompts
    enter; the processors act on the first logits; the first tokens come from argmax or sample_logits; _self_feeding_tail makes the others.
    Returns the generated ids of every row, cut after its first eos; with logprobs = K, (those, one info dict per row: the records of
    DecodeEngine.token_logprobs for the first token and of the step's own launch for the others, cut alike).
    one_prompt: the greedy tail of ONE prompt replays the capture_greedy graph, which records into stream_out[pos]: one element-wise node less
    per step than the rows graph, a difference that was measured (profiles/generate_drivers/README.md)."""
    with torch.no_grad():
        if spec is not None:
            return _speculate_rows(what, eng, prompts, into, max_new_tokens, eos_token_id, *spec)
        record = None
        if eng.constrain is not None:                            # (an engine passed in with the flag, no automata: its rows are unconstrained)
            eng.set_constraint(dfas)                             # validates before anything changes; every row at its start state
        if settings is not None:
            eng.set_sampling(**settings)
            if eng.logits_process:                               # (an engine passed in with the flag, neutral keys: its processors are switched off)
                eng.set_logits_process(eos_token_id=eos_token_id, **(proc or {}))
            graph = eng.graph_for('sample_native')
        elif one_prompt and eng.logprobs is None:                # (the capture_greedy graph records no logprobs)
            graph = eng.graph_for('greedy')
            record = (eng.stream_out.unsqueeze(1), int(prompts[0].numel()) + 1)      # stream_out[p] = the token chosen after p consumed ones
        else:
            graph = eng.graph_for('greedy_rows')
        logits = into(eng)
        if dfas is not None:                                     # the first token under the start states (behind the processors, ahead of the draw)
            logits = logits.to(torch.float16).contiguous()
        if settings is None:
            if dfas is not None:
                eng.constrain_logits(logits)
            first = logits.argmax(dim=-1)
        else:
            logits = logits.to(torch.float16).contiguous()
            if eng.logits_process:
                eng.process_logits(logits)
            if dfas is not None:
                eng.constrain_logits(logits)
            first = eng.sample_logits(logits)
        if logprobs is not None:                                 # the first token's record, from the logits it was drawn from
            head = eng.token_logprobs(logits.to(torch.float16).contiguous(), first, top=logprobs)
        gen = _self_feeding_tail(eng, graph, first, max_new_tokens, eos_token_id, record).t()      # [row][step]
        if dfas is not None:                                     # ONE look at the states: a row that consumed a token its state bans is at -2
            left = [b for b, s in enumerate(eng.c_state.tolist()) if s == -2]
            if left:
                raise RuntimeError('%s: row %s left its automaton: every token its state allows was banned by another setting (logit_bias, '
                                   'min_new_tokens), so the draw fell on a banned one' % (what, ', '.join(str(b) for b in left)))
        gens = [_cut_after_eos(g, eos_token_id) for g in gen]
        if logprobs is None:
            return gens
        # replay n wrote row n of the lp_* buffers, as of stream_rows: [first, rows 0 .. done - 2], cut where the tokens are cut
        done = gen.shape[1]
        tails = (eng.lp_chosen, eng.lp_rank, eng.lp_top_ids[:, :, :logprobs], eng.lp_top[:, :, :logprobs])
        full = [torch.cat([h.unsqueeze(0), t[:done - 1]]) for h, t in zip(head, tails)]              # [step][row] (, K)
        keys = ('token_logprobs', 'ranks', 'top_ids', 'top_logprobs')
        return gens, [{k: f[:g.numel(), b].clone() for k, f in zip(keys, full)} for b, g in enumerate(gens)]


def engine_generate(model, input_ids, max_new_tokens, eos_token_id=None, engine=None, t_max=2048, prefill='hf', sample=None, speculate=None,
                    logprobs=None, constrain=None, kv_cache='fp16'):
    """Generation for ONE prompt ([1, T] ids) on the DecodeEngine: the prompt enters the engine's static cache, the first token is chosen from
    its logits, and every further token is ONE hipGraph replay of a self-feeding step; the host looks at the stream every 16 tokens only.
    Returns the full sequence [1, prompt + generated], cut after the first eos_token_id.  The reference equivalent is
    ``model.generate(input_ids, do_sample=False, max_new_tokens=...)`` through llama_inference.py:109-115.
    prefill='hf' (the default): the prompt goes through the HF model once (the drop-in modules' prefill path: MFMA GEMMs, fused MLP
    epilogue) and its KV cache is copied into the engine's.  'engine': DecodeEngine.prefill instead (the engine's own launches with the
    hand-written causal attention kernel straight into its cache: no HF module chain, no DynamicCache, no copy) -- it reaches the first token
    sooner at every measured length (profiles/prompt_attn/README.md: 2.1 / 4.2 / 9.5 / 29.0 ms against 7.9 / 8.3 / 12.2 / 38.1 at 16, 128,
    512 and 2047 tokens of the 7B shape).
    engine=None builds a DecodeEngine for the call (t_max; chunk = k + 1 under speculate; logits_process when a processor is asked for).
    sample=dict(temperature=..., top_k=..., top_p=...) (every key optional: DecodeEngine.set_sampling) SAMPLES, as the reference's script does
    (llama_inference.py:119-127): the first token by DecodeEngine.sample_logits, the others by the capture_sample_native graph; the draws
    follow torch.manual_seed, temperature 0 gives the greedy tokens.  The settings STAY in the engine's buffers afterwards.
    The same dict takes the LOGIT PROCESSORS repetition_penalty, presence_penalty, min_new_tokens and logit_bias
    (DecodeEngine.set_logits_process; eos_token_id of this call is what min_new_tokens masks).  The prompt counts for repetition_penalty (HF's
    rule), only generated tokens for presence_penalty; they act before temperature, top-k and top-p: process_logits ahead of the first draw,
    one more launch per step of the native graph.  They need an engine with logits_process=True.  All neutral (1.0, 0.0, 0, None) is exactly
    the call without the keys: the same tokens for a seed and no process launch.
    speculate=dict(k=4, max_ngram=3, draft=None) (every key optional) decodes SPECULATIVELY, greedy: per step a draft of k tokens -- from
    draft(tokens_so_far: list[int], k) -> k ids, by default prompt_lookup_draft -- goes through the model together with the last token as ONE
    replay of the capture_verify_greedy graph (an engine with chunk = k + 1: one pass over the weights), which accepts the longest prefix the
    greedy rule agrees with and emits one token more; the host reads (accepted, tokens) in one copy per step.  Where fewer than 2 tokens remain
    or the chunk no longer fits the cache, the single-step graph finishes.  Same return value and eos semantics (the tokens are the greedy
    ones up to the near ties that any change of the arithmetic's row count moves); eng.spec_stats = dict(steps, emitted, accepted=[per step])
    describes the last run, and eng.pos is the position of the last token.
    speculate=dict(..., sample=dict(temperature, top_k, top_p)) SAMPLES speculatively: the capture_verify_sample graph applies the accept /
    resample rule of gptq_spec_sample_rows_f16 on the device, so the emitted tokens are distributed exactly as engine_generate(sample=...) draws
    them, whatever the draft; drafts from prompt lookup or `draft` count as point masses.  A processor key in there is a ValueError:
    processors under speculation are not built yet.  speculate=dict(..., draft_model=<fused model of the same vocabulary>) drafts with a MODEL:
    a DecodeEngine of its own (kept on the engine) draws the k tokens under the same setting and hands its logits rows to the verify step;
    without `sample` it drafts greedily and the verify-greedy graph checks it.
    logprobs = K (0 .. 32; None, the default: the call as it always was) returns (sequences, info): info is a dict on the device of the returned
    ids with, for the n generated tokens -- the first one included, cut after the first eos exactly as the tokens are, the eos entry kept --,
    token_logprobs float [n] (the log-probability of each token), ranks int32 [n] (its 0-based place among the vocabulary by (logit
    descending, id ascending)), top_ids int32 [n, K] and top_logprobs float [n, K] (the K most probable tokens of each step):
    gptq_logprobs_rows_f16, one more launch per step of the captured graph (DecodeEngine(logprobs=K)).  The probabilities are the MODEL's,
    from the logits the draw sees: behind the logit processors, before temperature / top-k / top-p.  Greedy, sample= and the processor keys
    all record; an engine passed in must have been built with logprobs >= K.
    constrain = a quant.constrain.TokenDFA (from_regex, from_sequences, from_table) makes the GENERATED tokens a word of its language -- the
    prompt is not part of the constrained text --: DecodeEngine.set_constraint puts the row at the start state, constrain_logits masks the first
    logits behind the processors and ahead of argmax / sample_logits, and every replay of the usual graphs advances the state by the token it
    consumes and masks its logits in one more launch (gptq_constrain_rows_f16).  An automaton whose accepting states lead eos to a FINAL state
    that allows only eos (from_regex, from_sequences) emits eos there, and the sequence is cut as always when that is eos_token_id.
    engine=None builds the engine with capacities taken from the automaton; an engine passed in must have been built with constrain= and hold
    it.  With logprobs, the records are those of the constrained distribution: banned tokens have -inf.  After the run the states are read
    once: RuntimeError naming the row that left its automaton (-2) -- the CALLER's error: logit_bias or min_new_tokens banned every token its
    state allowed, so the draw fell on a banned one.  None (the default) is exactly the call without the argument -- and on an engine passed
    in that was built with constrain= it means UNCONSTRAINED: the call replaces whatever automata an earlier set_constraint left on that
    engine by none (every row at -1), as the processor keys left out switch the processors off; set them again afterwards, or pass them
    here.  ValueError together with speculate= (not built yet) and for an engine without the flag.
    ValueError: logprobs together with speculate, on a beam-search engine, outside 0 .. 32, or on an engine built with a smaller K or none;
    speculate together with the sample ARGUMENT; k outside 1 .. 15; an engine passed in whose chunk is not k + 1 or whose batch is
    not 1; unknown keys; draft together with draft_model; a draft model of another vocabulary size; a prompt that is not [1, T]; prompt +
    max_new_tokens beyond the cache."""
    what = 'engine_generate'
    if prefill not in ('hf', 'engine'):
        raise ValueError("engine_generate: prefill must be 'hf' or 'engine', not %r" % (prefill,))
    settings, proc, spec = _generation_settings(what, model, sample, speculate, engine)
    logprobs = _logprobs_setting(what, logprobs, speculate, engine)
    dfas = _constrain_setting(what, constrain, 1, speculate, engine)
    _kv_cache_setting(what, kv_cache, speculate, engine)
    if spec is not None and engine is not None and (engine.batch != 1 or engine.chunk != spec[0] + 1):
        raise ValueError('engine_generate: speculate k = %d needs an engine of batch 1 with chunk = %d (this one: batch %d, chunk %d)' % (
            spec[0], spec[0] + 1, engine.batch, engine.chunk))
    if input_ids.dim() != 2 or input_ids.shape[0] != 1:
        raise ValueError('engine_generate: batch 1 only')
    if engine is not None:
        eng = engine
    elif spec is not None:
        eng = DecodeEngine(model, t_max=t_max, chunk=spec[0] + 1)
    else:
        eng = DecodeEngine(model, t_max=t_max, logits_process=proc is not None, logprobs=logprobs, constrain=_constrain_capacity(dfas),
                           kv_cache=kv_cache)
    if input_ids.shape[1] + max_new_tokens > eng.t_max:
        raise ValueError('engine_generate: prompt + max_new_tokens exceeds the engine cache (%d)' % eng.t_max)
    if settings is not None and eng.batch != 1:
        raise ValueError('engine_generate: sampling needs an engine of batch 1')

    def into(e):                                                 # (a draft model's engine takes the prompt by its own prefill)
        return _prompt_into_engine(model, input_ids, e, prefill if e is eng else 'engine').reshape(1, -1)
    out = _generate_rows(what, eng, [input_ids[0]], into, max_new_tokens, eos_token_id, settings, proc, spec, one_prompt=True, logprobs=logprobs,
                         dfas=dfas)
    gen = (out if logprobs is None else out[0])[0]
    if spec is not None:                                         # one sequence: emitted as an int, accepted as the flat per-step list
        eng.spec_stats = dict(eng.spec_stats, emitted=eng.spec_stats['emitted'][0], accepted=eng.spec_stats['accepted'][0])
    seq = torch.cat([input_ids[0], gen.to(device=input_ids.device, dtype=input_ids.dtype)]).unsqueeze(0)
    if logprobs is None:
        return seq
    return seq, {k: v.to(input_ids.device) for k, v in out[1][0].items()}


def engine_generate_batch(model, prompts, max_new_tokens, eos_token_id=None, engine=None, t_max=2048, sample=None, speculate=None, logprobs=None,
                          constrain=None, kv_cache='fp16'):
    """engine_generate for a LIST of prompts of different lengths (1-D id tensors): the same driver, arguments and ValueErrors, and what differs:
    all prompts enter through ONE DecodeEngine.prefill_batch (there is no prefill= route: nothing of `transformers` is involved, and the
    prompts are pad-free, so every row's history is its own prompt and tokens); a step is one replay for all rows, and a row that has emitted
    its eos keeps stepping and disturbs no other row.  Returns a list of 1-D tensors, prompt + generated, each cut after its first
    eos_token_id.  engine.batch must equal len(prompts) (engine=None builds one of that batch); max(T) + max_new_tokens <= t_max.
    sample=: every value a scalar for all rows or one value per prompt (logit_bias: one dict for all); a row with temperature 0 stays greedy.
    speculate=: at least two prompts, on an engine with batch = len(prompts) and batch_chunk = k + 1 (one pass over the weights at M = batch
    x (k + 1) per step: capture_verify_greedy_batch); a sequence that has hit its eos or its length idles; where no active sequence has two
    tokens left, or an active chunk no longer fits the cache, the single-step graph finishes all rows.  eng.spec_stats = dict(steps,
    emitted=[per sequence], accepted=[per sequence: per step]).  The keys sample / draft_model in there need an engine built with
    spec_sample=True (capture_verify_sample_batch: gptq_spec_sample_batch_f16 on all sequences in one launch).
    logprobs = K: returns (list of sequences, list of info dicts), one dict per prompt as engine_generate's, each as long as that row's generated
    tokens.
    constrain = one TokenDFA for all prompts or a list with one per prompt, None for a prompt that stays unconstrained: rows that pass the same
    object share its states.  A row that has reached its FINAL state keeps emitting eos and disturbs no other row.  As in engine_generate,
    the call REPLACES the automata of an engine passed in, also by none where constrain is None.
    kv_cache = 'fp8': as in engine_generate (the prompts enter through prefill_batch's fp16 staging and gptq_kv8_store_f16).
    ValueError also: an engine passed in whose batch is not len(prompts) or whose batch_chunk is not k + 1, or that lacks spec_sample where it
    is needed; an empty list or prompt; max_new_tokens below 1."""
    what = 'engine_generate_batch'
    settings, proc, spec = _generation_settings(what, model, sample, speculate, engine)
    logprobs = _logprobs_setting(what, logprobs, speculate, engine)
    dfas = _constrain_setting(what, constrain, len(prompts), speculate, engine)
    _kv_cache_setting(what, kv_cache, speculate, engine)
    sampled = spec is not None and (spec[3] is not None or spec[4] is not None)
    if sampled and engine is not None and not engine.spec_sample:
        raise ValueError('engine_generate_batch: speculate with sample or draft_model needs an engine built with spec_sample=True')
    n = len(prompts)
    if n < 1 or any((not torch.is_tensor(p)) or p.dim() != 1 or p.numel() == 0 for p in prompts):
        raise ValueError('engine_generate_batch: prompts must be a non-empty list of non-empty 1-D id tensors')
    max_new_tokens = int(max_new_tokens)
    if max_new_tokens < 1:
        raise ValueError('engine_generate_batch: max_new_tokens must be positive')
    if spec is not None and engine is not None and (engine.batch != n or engine.batch_chunk != spec[0] + 1):
        raise ValueError('engine_generate_batch: speculate k = %d for %d prompts needs an engine of batch %d with batch_chunk = %d (this one: batch '
                         '%d, batch_chunk %d)' % (spec[0], n, n, spec[0] + 1, engine.batch, engine.batch_chunk))
    if engine is not None:
        eng = engine
    elif spec is not None:
        eng = DecodeEngine(model, t_max=t_max, batch=n, batch_chunk=spec[0] + 1, spec_sample=sampled)
    else:
        eng = DecodeEngine(model, t_max=t_max, batch=n, logits_process=proc is not None, logprobs=logprobs, constrain=_constrain_capacity(dfas),
                           kv_cache=kv_cache)
    if eng.batch != n:
        raise ValueError('engine_generate_batch: %d prompts for an engine of batch %d' % (n, eng.batch))
    if max(int(p.numel()) for p in prompts) + max_new_tokens > eng.t_max:
        raise ValueError('engine_generate_batch: prompt + max_new_tokens exceeds the engine cache (%d)' % eng.t_max)
    out = _generate_rows(what, eng, prompts, lambda e: e.prefill_batch(prompts, starts=[0] * n), max_new_tokens, eos_token_id, settings, proc, spec,
                         logprobs=logprobs, dfas=dfas)
    gens = out if logprobs is None else out[0]
    seqs = [torch.cat([p, g.to(device=p.device, dtype=p.dtype)]) for p, g in zip(prompts, gens)]
    if logprobs is None:
        return seqs
    return seqs, [{k: v.to(p.device) for k, v in info.items()} for p, info in zip(prompts, out[1])]


def engine_generate_beam(model, input_ids, max_new_tokens, num_beams=4, eos_token_id=None, length_penalty=1.0, early_stopping=False,
                         num_return_sequences=1, engine=None, t_max=2048, prefill='engine', constrain=None):
    """Beam search for ONE prompt ([1, T] ids) on the DecodeEngine, by HF's rule (`generate(num_beams=N, do_sample=False)` with at most one EOS id
    and no logit processors; gptq_mi355x.h "beam search"): the prompt enters cache row 0 (prefill: 'engine' or 'hf', as engine_generate), beam_begin
    chooses the N first tokens and replicates the prompt's cache rows, and every further step is ONE replay of the capture_beam_step graph -- the
    batch step at M = N, the select, the in-place cache reorder -- behind which the host reads the 4-byte `done` flag.  Returns (sequences, scores):
    the num_return_sequences best hypotheses, best first, each a 1-D tensor prompt + tokens (a closing EOS included), and their float32
    length-penalised scores (HF's sequences_scores).  engine=None builds DecodeEngine(model, t_max, batch=num_beams, beam_search=True).
    ValueError: a prompt that is not [1, T]; num_beams outside 2 .. 16; an engine whose batch is not num_beams or that lacks beam_search;
    num_return_sequences outside 1 .. num_beams; more than one EOS id; prompt + max_new_tokens beyond the cache; a vocabulary below 2 num_beams;
    a row of logits that was not finite (the state's status word) -- raised after the run; constrain= other than None: constraints for beams
    are not built yet (a beam's state would have to move with its cache row)."""
    what = 'engine_generate_beam'
    if constrain is not None:
        raise ValueError('%s: constrain together with beam search is not built yet' % what)
    if prefill not in ('hf', 'engine'):
        raise ValueError("%s: prefill must be 'hf' or 'engine', not %r" % (what, prefill))
    if input_ids.dim() != 2 or input_ids.shape[0] != 1 or input_ids.shape[1] < 1:
        raise ValueError('%s: one prompt [1, T] only' % what)
    if isinstance(num_beams, bool) or not isinstance(num_beams, int) or not 2 <= num_beams <= MAX_BEAMS:
        raise ValueError('%s: num_beams = %r must be 2 .. %d' % (what, num_beams, MAX_BEAMS))
    if engine is not None and (engine.batch != num_beams or not engine.beam_search):
        raise ValueError('%s: needs an engine of batch %d built with beam_search=True' % (what, num_beams))
    if isinstance(num_return_sequences, bool) or not isinstance(num_return_sequences, int) or not 1 <= num_return_sequences <= num_beams:
        raise ValueError('%s: num_return_sequences = %r for %d beams' % (what, num_return_sequences, num_beams))
    max_new_tokens = int(max_new_tokens)
    if max_new_tokens < 1:
        raise ValueError('%s: max_new_tokens must be positive' % what)
    if model.lm_head.weight.shape[0] < 2 * num_beams:
        raise ValueError('%s: %d beams need a vocabulary of at least %d' % (what, num_beams, 2 * num_beams))
    eng = engine if engine is not None else DecodeEngine(model, t_max=t_max, batch=num_beams, beam_search=True)
    if input_ids.shape[1] + max_new_tokens > eng.t_max:
        raise ValueError('%s: prompt + max_new_tokens exceeds the engine cache (%d)' % (what, eng.t_max))
    with torch.no_grad():
        graph = eng.graph_for('beam')                            # (before the prompt: a capture warms up with a real step)
        eng.set_beam_search(max_new_tokens, eos_token_id, length_penalty, early_stopping)
        eng.beam_begin(_prompt_into_engine(model, input_ids, eng, prefill))
        done = eng.beam_state[BEAM_W_DONE:BEAM_W_DONE + 1]
        while not int(done):
            graph.replay()
        if int(eng.beam_state[BEAM_W_STATUS]):
            raise ValueError('%s: a row of logits was not finite, or the state block was not set up (status %d)' % (
                what, int(eng.beam_state[BEAM_W_STATUS])))
        seqs, scores = eng.beam_result(num_return_sequences)
    return [torch.cat([input_ids[0], g.to(device=input_ids.device, dtype=input_ids.dtype)]) for g in seqs], scores


def benchmark_decode_engine(model, tokens=64, t_max=2048, seed=0, graph=True, fuse_norm=True, fuse_attn=True, start_pos=0, batch=1):
    """the llama.py:385-438 protocol on the DecodeEngine (hipGraph replay per token).  batch > 1: B sequences advance together, one
    replay per step; tokens_per_s is the aggregate (B tokens per step)."""
    dev = next(model.parameters()).device
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    eng = DecodeEngine(model, t_max=t_max, fuse_norm=fuse_norm, fuse_attn=fuse_attn, batch=batch)
    if graph:
        eng.capture()
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    input_ids = torch.randint(0, model.config.vocab_size, (batch, tokens), device=dev, generator=gen)
    times = []
    eng.reset()
    if start_pos:      # decode at depth: pretend start_pos tokens are already cached (random K/V rows)
        eng.kcb.normal_(0, 0.5)
        eng.vcb.normal_(0, 0.5)
        eng.pos.fill_(int(start_pos))
    for i in range(tokens):
        torch.cuda.synchronize(dev)
        tick = time.perf_counter()
        eng.decode(input_ids[:, i])
        torch.cuda.synchronize(dev)
        times.append(time.perf_counter() - tick)
    med = float(np.median(times[2:])) if len(times) > 4 else float(np.median(times))
    res = {'protocol': 'llama.py:385-438 (one token per step, KV cache, sync per step, median)',
           'mode': 'DecodeEngine, %s' % ('one hipGraph replay per token' if graph else 'eager launches'), 'tokens': tokens,
           't_max': t_max, 'start_pos': start_pos, 'fused_norm': fuse_norm, 'fused_attention': fuse_attn,
           # per layer: [norm,] qkv, [rope+append, attention partial, merge | one fused launch], o+residual, [norm,] gate/up, down+residual
           'launches_per_token': (9 - 2 * int(fuse_norm) - 2 * int(fuse_attn)) * len(eng.layers) + 4, 'median_s_per_token': round(med, 6),
           'tokens_per_s': round(batch / med, 1),
           # the llama.py:426-438 figure: peak bytes in use by tensors while decoding (model + derived copies + KV cache of t_max + engine buffers)
           'max_memory_MiB': round(torch.cuda.max_memory_allocated(dev) / 1024 / 1024, 1)}
    if batch > 1:
        res['batch'] = batch
        res['mode'] = 'DecodeEngine(batch=%d), %s' % (batch, 'one hipGraph replay per step' if graph else 'eager launches')
        res['median_s_per_step'] = res.pop('median_s_per_token')
        res.pop('launches_per_token')
    return res


def benchmark_decode_engine_context(model, contexts=(512, 1024, 2047), tokens=16, t_max=2048, batch=1, seed=0):
    """the same protocol at DEPTH: for every entry of `contexts` the engine's rows pretend to hold context - tokens cached tokens (random K / V
    rows) and decode `tokens` more, so the median step sees ~context tokens of history -- the regime of the reference's own measurement, which
    steps through --benchmark 2048 tokens and prints the median (llama.py:385-438; README.md:161).  ONE engine / graph for all depths."""
    dev = next(model.parameters()).device
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    eng = DecodeEngine(model, t_max=t_max, batch=batch).capture()
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    input_ids = torch.randint(0, model.config.vocab_size, (batch, tokens), device=dev, generator=gen)
    eng.kcb.normal_(0, 0.5)
    eng.vcb.normal_(0, 0.5)
    out = {}
    for ctx in contexts:
        start = max(0, min(int(ctx), t_max) - tokens)
        eng.pos.fill_(start)
        times = []
        for i in range(tokens):
            torch.cuda.synchronize(dev)
            tick = time.perf_counter()
            eng.decode(input_ids[:, i])
            torch.cuda.synchronize(dev)
            times.append(time.perf_counter() - tick)
        med = float(np.median(times[2:]))
        out['ctx%d' % ctx] = {'positions': [start, start + tokens - 1], 'median_s_per_step': round(med, 6), 'tokens_per_s': round(batch / med, 1)}
    out['protocol'] = 'llama.py:385-438 at depth: rows start with (context - %d) cached tokens, %d steps, sync per step, median' % (tokens, tokens)
    out['batch'] = batch
    out['attention'] = 'split records merged by o_proj' if eng.attn_records else 'self-merging launch'
    return out
