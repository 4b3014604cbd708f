"""The engines choose the right norm weight and the right eps.  build_random_llama fills every norm weight with exactly 1.0 and
leaves rms_norm_eps at 1e-6 next to embeddings of std 0.02: exchanging input_layernorm and post_attention_layernorm, taking another
layer's weight, skipping the final norm's weight or hard-coding eps in a layer loop passes every other model-level test.  Here every
norm weight is drawn on its own (log-uniform 0.5 .. 2), the embeddings are scaled to std 1e-3 (var = 1e-6: the size of eps) and
rms_norm_eps is 1e-5 -- identically on the fused model, the unfused model and (through dense_twin) the stock HF twin, whose norm is
HF's own LlamaRMSNorm.  Every engine entry is compared with the module chain AND with the twin; how far a twin with exchanged weights,
a dropped final weight or eps = 1e-6 sits from the right one is measured on the twin alone (test_the_twin_can_see_...)."""
import functools
import math
import os
import zlib

import numpy as np
import pytest
import torch

from quant import decode as D
from util import within
from test_gpu_model import ENGINE_TOL, HOOK_TOL, TWIN_TOL, HD128, TINY, dense_twin, run_steps, _spawn

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 1e-5
CFG = dict(HD128, rms_norm_eps=EPS)
CFG_TINY = dict(TINY, rms_norm_eps=EPS)
CFG_TP = dict(HD128, num_attention_heads=4, num_key_value_heads=4, hidden_size=512, intermediate_size=1024, rms_norm_eps=EPS)
VOCAB = HD128['vocab_size']
NORM_SEED = 1
# The bars are the ones in force in tests/test_gpu_model.py.  Observed on the MI355X (GPTQ_TEST_ERRLOG), against the module chain / the twin:
#   ENGINE_TOL 2.7e-3  decode b1 8.7e-4 / 1.2e-3 (the same bits for fuse x graph); b4 worst row 2.2e-3, p95 8.3e-4 / 1.1e-3; b16 p95 8.9e-4,
#                      worst row 1.8e-3 (TWIN_TOL, as tests/test_gpu_batch.py) / 6.3e-3 (twin noise 1.4e-2); act-order w4 8.7e-4 / 8.7e-4,
#                      w3 8.4e-4 / 8.4e-4; two tensor-parallel ranks 6.3e-4 / 8.4e-4
#   HOOK_TOL 2e-2      prefill 8.4e-4 / 1.6e-3; prefill_batch rows 8.1e-4 .. 1.2e-3 / 9.4e-4 .. 4.4e-3; score 2.4e-4 / 8.7e-4 (of 2 x the bar);
#                      verify 0 (the module chain takes the same launches at three rows) / 1.1e-3; generate 1.6e-3 / 6.5e-3
#   TWIN_TOL 1.2e-2    the twin columns above; the module chain on the head_dim 64 model 1.0e-3
#   the twin with exchanged ln1 / ln2 of layer 0: 1.47, with the final weight set to 1: 0.45, with eps = 1e-6: 1.36 (needed: > 0.12)


def randomize_norms_(model, seed):
    """every 1-D parameter (the norm weights) log-uniform in 0.5 .. 2, a separate draw per norm (seeded by its name: the same values on
    the fused model, the unfused model and the twin)"""
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.dim() == 1:
                g = torch.Generator().manual_seed(seed * 1000003 + zlib.crc32(name.encode()))
                u = torch.rand(p.shape, generator=g, dtype=torch.float64)
                p.copy_(torch.exp(math.log(0.5) + u * math.log(4.0)).to(p.dtype))
    return model


def scale_embeddings_(model, factor):
    with torch.no_grad():
        model.model.embed_tokens.weight.mul_(factor)
    return model


def prepare_(model):
    return scale_embeddings_(randomize_norms_(model, NORM_SEED), 0.05)


def _cfg(name):
    return {'hd128': CFG, 'tiny': CFG_TINY, 'tp': CFG_TP}[name]


@functools.lru_cache(maxsize=None)
def fused_model(seed=3, bits=4, act=False, cfg='hd128'):
    return prepare_(D.build_random_llama(DEV, bits=bits, groupsize=128, seed=seed, fused=True, act_order=act, **_cfg(cfg)))


@functools.lru_cache(maxsize=None)
def twin_model(seed=3, bits=4, act=False, cfg='hd128'):
    unfused = prepare_(D.build_random_llama(DEV, bits=bits, groupsize=128, seed=seed, fused=False, act_order=act, **_cfg(cfg)))
    twin = dense_twin(unfused, _cfg(cfg))
    assert float(twin.model.embed_tokens.weight.float().std()) < 2e-3 and twin.model.norm.variance_epsilon == EPS
    assert not torch.equal(twin.model.layers[0].input_layernorm.weight, twin.model.layers[0].post_attention_layernorm.weight)
    assert torch.equal(twin.model.layers[1].input_layernorm.weight, fused_model(seed, bits, act, cfg).model.layers[1].input_layernorm.weight)
    return twin


def ids_for(shape, seed):
    return torch.randint(0, VOCAB, shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def twin_steps(twin, ids, prefill):
    """(the twin's fp16 logits, the bar against them): TWIN_TOL, raised -- as test_tiny_llama_batched_decode_matches_dense_twin raises it --
    to the twin's own distance from its fp32 copy on the same tokens (a measurement of the reference only)"""
    c = run_steps(twin, ids, prefill)
    exact = run_steps(twin.float(), ids, prefill)
    twin.half()
    noise = np.abs(c - exact).max() / np.abs(c).max()
    return c, max(TWIN_TOL, float(noise))


def against_both(name, got, model, twin, ids, prefill, tol):
    """got [steps, B, vocab] against the module chain (tol) and against the dense twin (TWIN_TOL or its own fp16 noise)"""
    expect = run_steps(model, ids, prefill)
    assert np.isfinite(got).all() and got.shape == expect.shape, (got.shape, expect.shape)
    within(name + '_chain', np.abs(got - expect).max() / np.abs(expect).max(), tol)
    c, bar = twin_steps(twin, ids, prefill)
    within(name + '_twin', np.abs(got - c).max() / np.abs(c).max(), bar)
    return expect


# ---------------------------------------------------------------------------------------
# the reference can see what these tests are for
# ---------------------------------------------------------------------------------------
def test_the_twin_can_see_exchanged_weights_a_dropped_final_weight_and_the_other_eps():
    """computed on the stock HF twin, never on an engine: with layer 0's two norm weights exchanged, with the final norm's weight set to 1,
    with eps = 1e-6 instead of 1e-5, the twin's logits move by more than 10 x the bar the engines are held to against it"""
    import copy
    twin = twin_model()
    ids = ids_for((1, 10), 99)
    right, bar = twin_steps(twin, ids, 1)
    scale = np.abs(right).max()

    def distance(change):
        wrong = copy.deepcopy(twin)
        with torch.no_grad():
            change(wrong)
        return float(np.abs(run_steps(wrong, ids, 1) - right).max() / scale)

    def exchange(m):
        a, b = m.model.layers[0].input_layernorm.weight, m.model.layers[0].post_attention_layernorm.weight
        t = a.clone()
        a.copy_(b)
        b.copy_(t)

    def other_eps(m):
        from transformers.models.llama.modeling_llama import LlamaRMSNorm
        for mod in m.modules():
            if isinstance(mod, LlamaRMSNorm):
                mod.variance_epsilon = 1e-6

    for name, change in (('exchange_ln1_ln2', exchange), ('final_weight_one', lambda m: m.model.norm.weight.fill_(1.0)), ('eps_1e-6', other_eps)):
        d = distance(change)
        print('twin sensitivity %s: %.3e (bar %.3e)' % (name, d, bar))
        path = os.environ.get('GPTQ_TEST_ERRLOG')
        if path:
            with open(path, 'a') as f:
                f.write('twin_sensitivity_%s %.3e > %.1e\n' % (name, d, 10 * bar))
        assert d > 10 * bar, (name, d, bar)


def test_module_chain_matches_the_twin():
    """the expectation of every test below, itself against the twin: the drop-in modules (HIP RMSNorm at M = batch x T rows, fused qkv /
    MLP) on a batch of three, head_dim 64 (no engine serves that: the module chain alone)"""
    q, twin = fused_model(seed=7, cfg='tiny'), twin_model(seed=7, cfg='tiny')
    ids = ids_for((3, 8), 102)
    a = run_steps(q, ids, 5)
    c, bar = twin_steps(twin, ids, 5)
    assert np.isfinite(a).all() and a.shape == c.shape
    within('norm_chain_tiny_twin', np.abs(a - c).max() / np.abs(c).max(), bar)


# ---------------------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('fuse', [False, True])
@pytest.mark.parametrize('graph', [False, True])
def test_decode_batch1(graph, fuse):
    q, twin = fused_model(), twin_model()
    ids = ids_for((1, 10), 99)
    eng = D.DecodeEngine(q, t_max=64, fuse_norm=fuse, fuse_attn=fuse)
    assert eng.eps == EPS
    if graph:
        eng.capture()
    got = np.stack([eng.decode(ids[0, i]).float().cpu().numpy()[0] for i in range(ids.shape[1])])[:, None, :]
    against_both('norm_engine_b1_g%d_f%d' % (graph, fuse), got, q, twin, ids, 1, ENGINE_TOL)


@pytest.mark.parametrize('B', [4, 16])
def test_decode_batch(B):
    q, twin = fused_model(seed=3 + B), twin_model(seed=3 + B)
    ids = ids_for((B, 9), B)
    eng = D.DecodeEngine(q, t_max=64, batch=B).capture()
    got = np.stack([eng.decode(ids[:, i]).float().cpu().numpy() for i in range(ids.shape[1])])
    expect = run_steps(q, ids, 1)
    err = np.abs(got - expect).max(axis=2) / np.abs(expect).max()
    # as test_batched_decode_engine_matches_the_module_chain: the bulk of the (step, row) pairs to the engine bar, the worst row of a
    # 16-row batch to the twin bar
    within('norm_engine_b%d_p95' % B, np.quantile(err, 0.95), ENGINE_TOL)
    within('norm_engine_b%d_chain' % B, err.max(), ENGINE_TOL if B <= 8 else TWIN_TOL)
    c, bar = twin_steps(twin, ids, 1)
    within('norm_engine_b%d_twin' % B, np.abs(got - c).max() / np.abs(c).max(), bar)


@pytest.mark.parametrize('bits', [4, 3])
def test_decode_act_order(bits):
    """an --act-order model: x and the norm weight go through the permutation together.  The seeds are chosen on the REFERENCE alone: the
    twin's own fp16 - fp32 distance on these tokens has to be below TWIN_TOL / 4 for the twin to be a yardstick at all (asserted below).
    Measured on the MI355X for the 4-bit model, seeds 4 .. 8: 8.8e-3, 3.1e-3, 8.1e-4, 2.0e-3, 1.1e-3 -- seed 6 is the first one admitted
    (seed 4, the seed of test_decode_engine_act_order_checkpoint: engine 1.22e-2 from the fp16 twin, 3.4e-3 from its fp32 copy, 1.9e-3 from
    the module chain: the twin's noise, not the engine's).  3-bit keeps seed 5 (twin noise 7.0e-4)."""
    seed = 6 if bits == 4 else 5
    q, twin = fused_model(seed=seed, bits=bits, act=True), twin_model(seed=seed, bits=bits, act=True)
    ids = ids_for((1, 8), 7)
    c = run_steps(twin, ids, 1)
    noise = np.abs(c - run_steps(twin.float(), ids, 1)).max() / np.abs(c).max()
    twin.half()
    assert noise < TWIN_TOL / 4, noise
    eng = D.DecodeEngine(q, t_max=64).capture()
    assert all(L['qkv']['perm'] is not None and L['gate']['perm2'] is not None for L in eng.layers)
    got = np.stack([eng.decode(ids[0, i]).float().cpu().numpy()[0] for i in range(ids.shape[1])])[:, None, :]
    against_both('norm_engine_act_order_w%d' % bits, got, q, twin, ids, 1, ENGINE_TOL)


# ---------------------------------------------------------------------------------------
# prompts
# ---------------------------------------------------------------------------------------
def test_prefill():
    q, twin = fused_model(), twin_model()
    T = 9
    ids = ids_for((1, T + 4), 109)
    eng = D.DecodeEngine(q, t_max=64)
    got = [eng.prefill(ids[0, :T], start=0).float().cpu().numpy().reshape(-1)]
    got += [eng.decode(ids[0, i]).float().cpu().numpy()[0] for i in range(T, T + 4)]
    against_both('norm_engine_prefill', np.stack(got)[:, None, :], q, twin, ids, T, HOOK_TOL)


def test_prefill_batch():
    q, twin = fused_model(), twin_model()
    lens = [5, 9, 3, 7]
    prompts = [ids_for((1, n + 1), 200 + r) for r, n in enumerate(lens)]
    eng = D.DecodeEngine(q, t_max=64, batch=4)
    first = eng.prefill_batch([p[0, :n] for p, n in zip(prompts, lens)]).float().cpu().numpy()
    second = eng.decode(torch.stack([p[0, n] for p, n in zip(prompts, lens)])).float().cpu().numpy()
    for r, (p, n) in enumerate(zip(prompts, lens)):
        got = np.stack([first[r], second[r]])[:, None, :]
        against_both('norm_engine_prefill_batch_row%d' % r, got, q, twin, p, n, HOOK_TOL)


def test_score():
    q, twin = fused_model(), twin_model()
    ids = ids_for((24,), 71)
    got = D.DecodeEngine(q, t_max=64).score(ids).double()

    def nll_of(model, dtype):
        model._gptq_engine_disabled = True
        try:
            with torch.no_grad():
                z = model(ids[None]).logits[0, :-1].double()
        finally:
            model._gptq_engine_disabled = False
        return torch.logsumexp(z, dim=1) - z.gather(1, ids[1:, None])[:, 0], z

    want, z = nll_of(q, torch.float16)
    # a logit error of HOOK_TOL max|z| moves logsumexp and the target's logit by that much each (tests/test_gpu_score.py)
    within('norm_engine_score_chain', float(((got - want).abs() / z.abs().max(dim=1).values).max()), 2 * HOOK_TOL)
    wt, zt = nll_of(twin, torch.float16)
    we, ze = nll_of(twin.float(), torch.float32)
    twin.half()
    noise = float((zt - ze).abs().max() / zt.abs().max())
    within('norm_engine_score_twin', float(((got - wt).abs() / zt.abs().max(dim=1).values).max()), 2 * max(TWIN_TOL, noise))


def test_verify():
    q, twin = fused_model(), twin_model()
    T = 3
    ids = ids_for((1, 2 * T), 303)
    eng = D.DecodeEngine(q, t_max=64, chunk=T)
    first = eng.prefill(ids[0, :T], start=0).float().cpu().numpy().reshape(-1)
    rows = eng.verify(ids[0, T:2 * T]).float().cpu().numpy()
    assert rows.shape == (T, VOCAB)
    against_both('norm_engine_verify', np.concatenate([first[None], rows])[:, None, :], q, twin, ids, T, HOOK_TOL)


def test_generate_through_the_engine_hook():
    from quant.engine_hook import engine_steps
    q, twin = fused_model(seed=11), twin_model(seed=11)
    ids = ids_for((1, 7), 2)
    n = 12
    before = engine_steps(q)
    with torch.no_grad():
        out = q.generate(ids, do_sample=False, max_new_tokens=n, min_new_tokens=n, return_dict_in_generate=True, output_logits=True)
    assert engine_steps(q) == before + n - 1
    got = torch.stack([l[0].float() for l in out.logits]).cpu().numpy()[:, None, :]
    seq = out.sequences[:, :ids.shape[1] + n - 1]                  # teacher-forced on the tokens the hook chose
    against_both('norm_engine_hook_generate', got, q, twin, seq, ids.shape[1], HOOK_TOL)


# ---------------------------------------------------------------------------------------
# tensor parallel
# ---------------------------------------------------------------------------------------
def _tp_norm_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from quant.tp_decode import TPDecodeEngine
        torch.cuda.set_device(0)
        model = fused_model(seed=21, cfg='tp')
        ids = ids_for((1, 9), 5)
        eng = TPDecodeEngine(model, t_max=64).capture()
        got = np.stack([eng.decode(ids[0, i]).float().cpu().numpy()[0] for i in range(9)])[:, None, :]
        ok = eng.status() == 0
        try:
            if rank == 0:
                against_both('norm_engine_tp2', got, model, twin_model(seed=21, cfg='tp'), ids, 1, ENGINE_TOL)
            else:
                expect = run_steps(model, ids, 1)
                assert np.abs(got - expect).max() / np.abs(expect).max() < ENGINE_TOL
        except AssertionError as e:
            print('rank %d: %r' % (rank, e), flush=True)
            ok = False
        t = torch.tensor([1 if ok else 0])
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        if rank == 0:
            ret.put(int(t.item()))
    finally:
        dist.destroy_process_group()


def test_tensor_parallel_engine_two_ranks_one_gpu():
    _spawn(_tp_norm_worker, 2)
