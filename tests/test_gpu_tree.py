"""GPU tests of tree speculative decoding: gptq_decode_attn_tree_f16, gptq_tree_accept_greedy, gptq_kv_tree_compact_f16 through the C ABI, and
DecodeEngine(chunk=R, tree=True).  Method of tests/test_gpu_attn_chunk.py: float64 on the fp16 values, the op-level bar TOL per row, NaN sentinels."""
import functools

import numpy as np
import pytest
import torch

from quant import _native
from quant import decode as D
from util import rel_err, TOL

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HEADS, HD, T_MAX, BASE = 2, 128, 640, 10000.0
H = HEADS * HD
SCALE = float(1.0 / np.sqrt(HD))
NAN = np.uint16(0x7E00).view(np.float16)
BRANCHES = [-1, 0, 1, 2, 3, 4, 5, 6, 0, 8, 9, 10, 11, 12, 13]                  # two branches of depth 7: leaves 7 and 14
TREES = dict(chain=[-1, 0, 1, 2, 3], chain16=[-1] + list(range(15)), star=[-1] + [0] * 15, branches=BRANCHES, irregular=[-1, 0, 0, 1, 1, 2, 0, 4, 4, 5, 7, 7, 3, 10, 12, 9],
             single=[-1])


def _anc(parents):
    anc = [1] * 16
    for r in range(1, len(parents)):
        anc[r] = anc[parents[r]] | (1 << r)
    return anc


_dev = lambda a: torch.from_numpy(np.array(a, order='C')).to(DEV)
_bits = lambda t: t.cpu().numpy().view(np.uint16)


def _position(p, rows):
    """'split2' / 'split0': a position the library cuts into two splits / the most it can choose at T_MAX; 'end': the last one that fits"""
    if not isinstance(p, str):
        return p
    count = lambda q: _native.lib().gptq_decode_attn_chunk_splits(HEADS, HD, T_MAX, q + rows)
    want = int(p[5:] if p != 'end' else 0) or count(T_MAX - rows)
    assert want >= 2
    return T_MAX - rows if p == 'end' else next(q for q in range(3, T_MAX - rows, 61) if count(q) == want)


@functools.lru_cache(maxsize=None)
def _inputs(p, rows):
    rng = np.random.default_rng(1000 * p + rows)
    qkv = rng.standard_normal((rows, 3 * H)).astype(np.float16)
    kc = (rng.standard_normal((T_MAX, H)) * 0.5).astype(np.float16)
    vc = rng.standard_normal((T_MAX, H)).astype(np.float16)
    kc[p:], vc[p:] = NAN, NAN                                      # the sentinel: a row at or beyond p that is read shows, one that is written too
    return qkv, kc, vc


def _call(entry, p, rows, qkv, kc, vc, anc=None):
    lib, s = _native.lib(), torch.cuda.current_stream().cuda_stream
    qd, kd, vd = _dev(qkv), _dev(kc), _dev(vc)
    od = torch.full((rows, H), float('nan'), dtype=torch.float16, device=DEV)
    pos = torch.tensor([p], dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.gptq_decode_attn_chunk_workspace_bytes(rows, HEADS, HD, T_MAX), dtype=torch.uint8, device=DEV).fill_(0xA5)
    ad = None if anc is None else _dev(np.array(anc, dtype=np.uint32).view(np.int32))
    extra = () if anc is None else (ad.data_ptr(),)
    rc = getattr(lib, entry)(qd.data_ptr(), 3 * H, rows, pos.data_ptr(), *extra, kd.data_ptr(), vd.data_ptr(), od.data_ptr(), H, ws.data_ptr(),
                             ws.numel(), HEADS, HD, T_MAX, BASE, SCALE, None, s)
    _native.check(rc, entry)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(qd), qkv.view(np.uint16)), 'qkv was modified'
    return _bits(od), _bits(kd), _bits(vd)


_tree = lambda p, parents, qkv, kc, vc: _call('gptq_decode_attn_tree_f16', p, len(parents), qkv, kc, vc, _anc(parents))


def _rotated(qkv, p, depth):
    # gptq_decode_rope_kv_f16 per node at position p + its depth: the rotated q rows and the k rows it appends
    lib, s = _native.lib(), torch.cuda.current_stream().cuda_stream
    qd = _dev(qkv)
    kd, vd = torch.zeros((T_MAX, H), dtype=torch.float16, device=DEV), torch.zeros((T_MAX, H), dtype=torch.float16, device=DEV)
    k = []
    for r, d in enumerate(depth):
        pos = torch.tensor([p + d], dtype=torch.int64, device=DEV)
        _native.check(lib.gptq_decode_rope_kv_f16(qd[r].data_ptr(), pos.data_ptr(), kd.data_ptr(), vd.data_ptr(), HEADS, HD, T_MAX, BASE, s), 'rope_kv')
        k.append(kd[p + d].clone())
    return qd.cpu().numpy()[:, :H], torch.stack(k).cpu().numpy()


@pytest.mark.parametrize('p', [0, 3, 31, 40, 'split2', 'split0', 'end'])
@pytest.mark.parametrize('tree', sorted(TREES))
def test_tree_attn_against_float64(tree, p):
    parents, rows, anc = TREES[tree], len(TREES[tree]), _anc(TREES[tree])
    p = _position(p, rows)
    qkv, kc, vc = _inputs(p, rows)
    out, kb, vb = _tree(p, parents, qkv, kc, vc)
    q_rot, k_rot = _rotated(qkv, p, [bin(a).count('1') - 1 for a in anc[:rows]])
    for name, got, old, new in (('k', kb, kc, k_rot), ('v', vb, vc, qkv[:, 2 * H:])):
        assert np.array_equal(got[p:p + rows], new.view(np.uint16)), name + ' rows of the nodes'
        assert np.array_equal(got[:p], old.view(np.uint16)[:p]) and np.array_equal(got[p + rows:], old.view(np.uint16)[p + rows:]), name + ' outside'
    kf, vf = kb.view(np.float16).astype(np.float64), vb.view(np.float16).astype(np.float64)
    for r in range(rows):
        keys = list(range(p)) + [p + j for j in range(rows) if anc[r] >> j & 1]
        for h in range(HEADS):
            c = slice(h * HD, (h + 1) * HD)
            sc = (kf[keys, c] @ q_rot[r, c].astype(np.float64)) * SCALE
            e = np.exp(sc - sc.max())
            err = rel_err(out[r, c].view(np.float16), (e / e.sum()) @ vf[keys, c])
            assert err < TOL, (r, h, err)
    again = _tree(p, parents, qkv, kc, vc)
    assert all(np.array_equal(a, b) for a, b in zip(again, (out, kb, vb))), 'two calls differ'
    if tree.startswith('chain'):                     # a chain is the chunk entry: output and caches bit for bit, at one split and at several
        assert all(np.array_equal(a, b) for a, b in zip(again, _call('gptq_decode_attn_chunk_f16', p, rows, qkv, kc, vc))), 'chain != chunk entry'


@pytest.mark.parametrize('p', [40, 'split0'])
@pytest.mark.parametrize('leaf', [7, 14])
def test_non_ancestors_do_not_reach_a_row(leaf, p):
    rows, anc = len(BRANCHES), _anc(BRANCHES)
    p = _position(p, rows)
    qkv, kc, vc = _inputs(p, rows)
    base = _tree(p, BRANCHES, qkv, kc, vc)[0]
    others = [j for j in range(rows) if not anc[leaf] >> j & 1]
    for fill in (np.random.default_rng(5).standard_normal((len(others), 3 * H)).astype(np.float16) * 4, NAN):
        qkv2 = qkv.copy()
        qkv2[others] = fill
        assert np.array_equal(_tree(p, BRANCHES, qkv2, kc, vc)[0][leaf], base[leaf])


@pytest.mark.parametrize('p', [-1, T_MAX, 2 ** 40, T_MAX - 3])
def test_tree_attn_bounds(p):
    """idle positions touch nothing; at T_MAX - 3 nodes 0 .. 2 of the star are served as the 3-node star is, the others skipped"""
    rows, fit = 16, max(0, min(16, T_MAX - p)) if p >= 0 else 0
    qkv, kc, vc = _inputs(T_MAX - 3, rows)
    out, kb, vb = _tree(p, TREES['star'], qkv, kc, vc)
    assert (out[fit:] == 0x7E00).all(), 'a skipped row was written'
    if not fit:
        assert np.array_equal(kb, kc.view(np.uint16)) and np.array_equal(vb, vc.view(np.uint16))
        return
    for a, b in zip((out[:fit], kb, vb), _tree(p, TREES['star'][:fit], qkv[:fit], kc, vc)):
        assert np.array_equal(a, b)


def _walk(tok, parents, best):
    path, nxt = [], [0]
    while nxt:
        path.append(nxt[0])
        nxt = [c for c in range(len(tok)) if parents[c] == path[-1] and tok[c] == best[path[-1]]]
    return path


@pytest.mark.parametrize('case', ['second_branch', 'chain', 'none'])
def test_accept_and_compaction(case):
    """the truth on BRANCHES' second branch (nodes 8 .. 11 accepted, 12 refused), a chain accepted whole, nothing accepted; two layers"""
    lib, s = _native.lib(), torch.cuda.current_stream().cuda_stream
    parents = BRANCHES if case != 'chain' else [-1] + list(range(14))
    rows, p, layers = len(parents), 37, 2
    tok, best = [100 + r for r in range(rows)], [0] * rows
    if case == 'second_branch':
        best[0], best[8], best[9], best[10], best[11] = tok[8], tok[9], tok[10], tok[11], 7
    elif case == 'chain':
        best = tok[1:] + [7]
    path = _walk(tok, parents, best)
    a, pos = len(path) - 1, torch.tensor([p], dtype=torch.int64, device=DEV)
    assert a == dict(second_branch=4, chain=14, none=0)[case]
    out, pd = torch.zeros(rows + 1, dtype=torch.int64, device=DEV), torch.zeros(16, dtype=torch.int32, device=DEV)
    args = [_dev(np.array(tok, dtype=np.int64)), _dev(np.array(parents, dtype=np.int32)), _dev(np.array(best, dtype=np.int64))]
    _native.check(lib.gptq_tree_accept_greedy(*(t.data_ptr() for t in args), rows, pos.data_ptr(), out.data_ptr(), pd.data_ptr(), s), 'accept')
    assert pd.tolist() == path + [-1] * (16 - len(path)) and int(pos[0]) == p + a + 1
    assert out.tolist() == [a] + [best[n] for n in path] + [best[path[-1]]] * (rows - len(path))
    qkv, kc, vc = _inputs(p, rows)
    trees = [_tree(p, parents, np.roll(qkv, li, axis=1), kc, vc) for li in range(layers)]
    kd, vd = (_dev(np.stack([t[i] for t in trees]).view(np.int16)) for i in (1, 2))
    if case != 'second_branch':
        kd[:, p + 1], vd[:, p + 1] = 0x5A5A, 0x5A5A                # a chain or an empty accept stores nothing: a copy of row p + 1 onto itself would show
    before = (_bits(kd).copy(), _bits(vd).copy())
    _native.check(lib.gptq_kv_tree_compact_f16(kd.data_ptr(), vd.data_ptr(), layers, T_MAX, H, T_MAX * H, pos.data_ptr(), out.data_ptr(), pd.data_ptr(), s), 'compact')
    torch.cuda.synchronize()
    if case != 'second_branch':
        assert np.array_equal(_bits(kd), before[0]) and np.array_equal(_bits(vd), before[1])
        return
    for li in range(layers):
        _, kr, vr = _call('gptq_decode_attn_chunk_f16', p, a + 1, np.roll(qkv, li, axis=1)[path], kc, vc)
        for got, ref, old in ((_bits(kd)[li], kr, before[0][li]), (_bits(vd)[li], vr, before[1][li])):
            assert np.array_equal(got[:p + a + 1], ref[:p + a + 1]) and np.array_equal(got[p + a + 1:], old[p + a + 1:])


# ---- the engine, on the model of tests/test_gpu_speculate.py ---------------------------------------------------------------------------------------
TINY = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2, vocab_size=512, max_position_embeddings=512)
E_T_MAX, R, NEW, HOOK_TOL = 160, 8, 24, 2e-2


@functools.lru_cache(maxsize=None)
def _engines():
    model = D.build_random_llama(DEV, seed=3, **TINY)
    return model, D.DecodeEngine(model, t_max=E_T_MAX).capture(), D.DecodeEngine(model, t_max=E_T_MAX, chunk=R, tree=True)


@pytest.mark.parametrize('draft', ['lookup', 'oracle', 'adversarial'])
def test_generate_with_a_tree(draft):
    """the rule of tests/test_gpu_speculate.py: every token within HOOK_TOL of the plain engine's teacher-forced maximum, at most one off its argmax"""
    (model, plain_eng, eng), T = _engines(), 24
    prompt = torch.randint(0, 512, (1, 6), device=DEV, generator=torch.Generator(device=DEV).manual_seed(77)).repeat(1, 4)   # repeated n-grams
    known = D.engine_generate(model, prompt, max_new_tokens=NEW, engine=plain_eng, prefill='engine')[0].tolist()

    def truth_second(toks, k):        # a wrong first branch of 3, the true continuation as the second branch
        t = (known[len(toks):len(toks) + k - 3] + [0] * k)[:k - 3]
        return [(t[0] + 1) % 512, 1, 2] + t, [0, 1, 2, 0] + list(range(4, k))
    wrong = lambda toks, k: ([(known[min(len(toks), len(known) - 1)] + 1 + j) % 512 for j in range(k)], [0] * k)
    spec = dict(k=R - 1, tree=dict(width=3), draft=dict(lookup=None, oracle=truth_second, adversarial=wrong)[draft])
    got = D.engine_generate(model, prompt, max_new_tokens=NEW, engine=eng, prefill='engine', speculate=spec)
    st = eng.spec_stats
    assert got.shape == (1, T + NEW) and int(eng.pos[0]) == T + NEW - 1
    ref = [plain_eng.prefill(got[0, :T], start=0).float().cpu().numpy()] + [plain_eng.decode(t).float().cpu().numpy()[0] for t in got[0, T:-1]]
    gen = got[0, T:].tolist()
    assert all(r[t] >= r.max() - HOOK_TOL * np.abs(r).max() for r, t in zip(ref, gen))
    assert sum(int(t != int(r.argmax())) for r, t in zip(ref, gen)) <= 1
    if draft == 'oracle':
        assert sum(1 for a in st['accepted'] if a != R - 4) <= 1, st        # the second branch, whole, but for one near tie at most
    if draft == 'adversarial':
        assert all(a == 0 for a in st['accepted']), st


def test_graph_and_eager_verify_agree_and_the_flag_is_opt_in():
    model, plain_eng, eng = _engines()
    assert not any(hasattr(plain_eng, n) for n in ('tree_anc', 'tree_tok', 'tree_parent', 'tree_path'))
    with pytest.raises(ValueError):
        D.DecodeEngine(model, t_max=E_T_MAX, tree=True)
    graph = eng.graph_for('verify_tree_greedy')
    eng.prefill(torch.arange(40, device=DEV) % 7, start=0)
    start, res = (eng.kc.clone(), eng.vc.clone()), []
    for run in (lambda: (eng.verify_tree(), eng.accept_tree()), graph.replay, graph.replay):
        eng.kc.copy_(start[0]); eng.vc.copy_(start[1]); eng.pos.fill_(40)
        eng.set_tree([5, 9, 3, 9, 4, 1], [-1, 0, 0, 1, 2, 2])
        run()
        res.append([t.clone() for t in (eng.verify_out, eng.tree_path, eng.pos, eng.chunk_logits, eng.kc, eng.vc)])
    assert all(torch.equal(a, b) for other in res[1:] for a, b in zip(res[0], other))
