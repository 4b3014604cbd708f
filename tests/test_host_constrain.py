"""CPU-side tests of constrained decoding (quant/constrain.py, include/gptq_mi355x.h "constrained decoding"): the regex compiler against Python's
own `re` over every short string, the token automaton against the byte level on a synthetic vocabulary, compression, the constructors'
errors, the mask rule (tests/constrain_ref.py) against transformers' PrefixConstrainedLogitsProcessor, and every rule of
gptq_constrain_rows_f16's host validation on fake aligned pointers: nothing is launched, no device is needed."""
import itertools
import re

import numpy as np
import pytest
import torch

import constrain_ref as R
from quant import _native
from quant.constrain import TokenDFA, llama_vocab_bytes, regex_byte_dfa

E_SHAPE, E_ALIGN, E_NULL = -2, -3, -4

# (pattern, alphabet): together they use every construct of the dialect
PATTERNS = [
    (r'a(b|c)*d', b'abcdx\n'),
    (r'\d+\.\d{2}', b'019.a '),
    (r'[a-c]{2,4}x?', b'abcdx-'),
    (r'[^a\d]+', b'ab1_ \n'),
    (r'(?:ab|a)(?:b|bc)?c*', b'abcd(?'),
    (r'\w+\s\W\S\D', b'a_ 1-\n'),
    (r'.{1,3}\n?', b'a\n.x\r\t'),
    (r'\x41[\x42-\x44]\t\r\n*', b'ABD\t\r\n'),
    (r'(a|b|)c{2,}', b'abcd{}'),
    (r'\{\d\}|\[\]|\(\)\*\+\?|\.\|\^\$', b'{}[]1a'),
    (r'[]a-][\]\\^-]?', b']a-\\^b'),
    (r'a{,2}b{2}(c{1,}|d)', b'abcd{,'),
    (r'[\d\s]-[\w.][\D\S][\W5]', b'1 -a.5'),
    (r'ab{c|}a{1|x{}', b'abc{}|'),
    (r'', b'ab'),
]

UNSUPPORTED = [r'^a', r'a$', r'\bfoo', r'\Aa', r'a\Z', r'a\B', r'(a)\1', r'(?=a)a', r'(?!a)b', r'(?<=a)b', r'(?<!a)b', r'a*?', r'a+?', r'a??',
               r'a{1,2}?', r'a*+', r'a++', r'a?+', r'(?i)a', r'(?i:a)', r'(?P<n>a)', r'a**', r'*a', r'(+a)', r'a|*', r'{2}', r'(a', r'a)', r'[a',
               r'[b-a]', r'[\d-z]', r'\q', r'\x4', r'[\b]', r'a{3,2}', 'a\\', r'a{5000}']


def _all_strings(alphabet, max_len):
    """every string over the alphabet up to max_len, per length: uint8 [n, L]"""
    a = np.frombuffer(alphabet, dtype=np.uint8)
    for L in range(max_len + 1):
        idx = np.indices((len(a),) * L).reshape(L, -1).T if L else np.zeros((1, 0), dtype=np.int64)
        yield a[idx]


def _dfa_accepts(trans, accept, strings):
    ext = np.vstack([np.where(trans < 0, trans.shape[0], trans), np.full((1, 256), trans.shape[0])])
    cur = np.zeros(strings.shape[0], dtype=np.int64)
    for p in range(strings.shape[1]):
        cur = ext[cur, strings[:, p]]
    return np.append(accept, False)[cur]


# ---- 1. the regex against Python's re ----
@pytest.mark.parametrize('pattern,alphabet', PATTERNS)
def test_byte_dfa_accepts_exactly_what_re_fullmatch_accepts(pattern, alphabet):
    trans, accept = regex_byte_dfa(pattern)
    rx = re.compile(pattern.encode())
    n_match = 0
    for strings in _all_strings(alphabet, 6):
        ours = _dfa_accepts(trans, accept, strings)
        want = np.array([rx.fullmatch(s.tobytes()) is not None for s in strings])
        bad = np.flatnonzero(ours != want)
        assert bad.size == 0, (pattern, strings[bad[0]].tobytes(), bool(want[bad[0]]))
        n_match += int(want.sum())
    assert n_match > 0, pattern                                 # the alphabet can spell the language


def test_unsupported_constructs_raise_naming_the_offset():
    for pattern in UNSUPPORTED:
        with pytest.raises(ValueError, match='offset'):
            regex_byte_dfa(pattern)
    with pytest.raises(ValueError, match='pattern must be a str'):
        TokenDFA.from_regex(b'a', [b'a', None], 1)


# ---- 2. the token level, on a synthetic vocabulary ----
TOKEN_PATTERNS = [(r'a(b|c)*d', b'abcdx\n'), (r'\d+\.\d{2}', b'019.a '), (r'[a-c]{2,4}x?', b'abcdx-'), (r'(?:ab|a)(?:b|bc)?c*', b'abcd(?')]


def _vocabulary(alphabet, seed, n=300):
    """every single byte of the alphabet, random strings of 2 .. 5 bytes, duplicates, None and b'' entries; the last id is eos"""
    rng = np.random.default_rng(seed)
    texts = [bytes([b]) for b in alphabet]
    while len(texts) < n - 40:
        texts.append(bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=rng.integers(2, 6)).tolist()))
    texts += [texts[i] for i in rng.integers(0, len(texts), size=30)]             # duplicates
    texts += [None] * 5 + [b''] * 4
    order = rng.permutation(len(texts))
    return [texts[i] for i in order] + [b'</s>'], len(texts)                      # (the eos token's own text never counts)


def _segmentations(s, by_text, max_len=5):
    if not s:
        yield []
        return
    for k in range(1, min(max_len, len(s)) + 1):
        ids = by_text.get(s[:k])
        if ids:
            for rest in _segmentations(s[k:], by_text, max_len):
                yield [ids] + rest


@pytest.fixture(scope='module', params=range(len(TOKEN_PATTERNS)))
def token_case(request):
    pattern, alphabet = TOKEN_PATTERNS[request.param]
    vocab, eos = _vocabulary(alphabet, seed=request.param)
    return pattern, alphabet, vocab, eos, TokenDFA.from_regex(pattern, vocab, eos)


def test_every_segmentation_of_every_match_walks_to_an_eos(token_case):
    pattern, alphabet, vocab, eos, dfa = token_case
    assert dfa.vocab == len(vocab) and dfa.next.dtype == np.int16 and dfa.cls.dtype == np.int16
    by_text = {}
    for v, t in enumerate(vocab[:-1]):
        if t:
            by_text.setdefault(t, []).append(v)
    assert max(len(ids) for ids in by_text.values()) > 1
    rx = re.compile(pattern.encode())
    n_seg = 0
    for strings in _all_strings(alphabet, 6):
        for s in strings:
            text = s.tobytes()
            matches = rx.fullmatch(text) is not None
            for k, seg in enumerate(_segmentations(text, by_text)):
                tokens = [ids[(k + j) % len(ids)] for j, ids in enumerate(seg)]    # (duplicates take turns)
                state = dfa.walk(tokens)
                if matches:
                    assert state >= 0 and dfa.allowed(state)[eos], (pattern, text, tokens)
                    n_seg += 1
                else:                                             # a text outside the language: dead, or alive without eos
                    assert state < 0 or not dfa.allowed(state)[eos], (pattern, text, tokens)
    assert n_seg > 50


def test_random_walks_spell_matching_texts(token_case):
    pattern, _, vocab, eos, dfa = token_case
    rx = re.compile(pattern.encode())
    rng = np.random.default_rng(7)
    final = dfa.step(dfa.walk([]), eos) if dfa.allowed(0)[eos] else None
    for _ in range(200):
        state, text = 0, b''
        for step in range(400):
            ok = dfa.allowed(state)
            assert ok.any()
            if ok[eos] and (rng.random() < 0.3 or step > 40):
                state = dfa.step(state, eos)
                break
            choices = np.flatnonzero(ok)
            choices = choices[choices != eos]
            if choices.size == 0:
                assert ok[eos]
                state = dfa.step(state, eos)
                break
            t = int(rng.choice(choices))
            assert vocab[t]                                      # None and b'' are never allowed
            text += vocab[t]
            state = dfa.step(state, t)
            assert state >= 0
        else:
            raise AssertionError('no end within 400 tokens')
        assert rx.fullmatch(text) is not None, (pattern, text)
        assert final is None or state == final
        assert dfa.allowed(state).sum() == 1 and dfa.step(state, eos) == state   # FINAL allows only eos -> FINAL


def test_every_state_allows_a_token_and_reaches_final(token_case):
    _, _, _, eos, dfa = token_case
    table = dfa.dense()
    assert table.shape == (dfa.n_states, dfa.vocab) and (table >= 0).any(axis=1).all() and table.max() < dfa.n_states
    finals = [s for s in range(dfa.n_states) if table[s, eos] == s]
    assert len(finals) == 1
    good = np.zeros(dfa.n_states, dtype=bool)
    good[finals[0]] = True
    for _ in range(dfa.n_states):
        good |= np.append(good, False)[table].any(axis=1)
    assert good.all()
    reach, stack = {0}, [0]                                     # ... and every state is reachable from the start
    while stack:
        for t in set(table[stack.pop()].tolist()) - {-1}:
            if t not in reach:
                reach.add(t)
                stack.append(t)
    assert len(reach) == dfa.n_states


# ---- 3. compression and sequences ----
def _random_table(rng, S, V, n_cols):
    cols = rng.integers(-1, S, size=(S, n_cols))
    cols[np.arange(S), rng.integers(0, n_cols, size=S)] = (np.arange(S) + 1) % S  # a cycle: every state reachable, every state allows a token
    return cols[:, rng.integers(0, n_cols, size=V)], cols


def test_dense_of_the_compressed_automaton_is_the_table():
    rng = np.random.default_rng(3)
    for S, V, n_cols in ((1, 5, 2), (6, 40, 7), (9, 500, 30)):
        table, cols = _random_table(rng, S, V, n_cols)
        dfa = TokenDFA.from_table(table)
        assert dfa.n_states == S and dfa.vocab == V
        assert np.array_equal(dfa.dense(), table)
        assert dfa.n_classes == len({table[:, v].tobytes() for v in range(V)}) <= n_cols
        for s in range(S):
            assert np.array_equal(dfa.allowed(s), table[s] >= 0)
        assert dfa.step(0, 3) == table[0, 3] and dfa.step(0, V) == -1 and dfa.step(-1, 0) == -1
    with pytest.raises(AttributeError):
        dfa.vocab = 3
    with pytest.raises(ValueError):
        dfa.next[0, 0] = 0


def test_from_table_renumbers_from_the_start_and_drops_unreachable_states():
    #         tok0 tok1 tok2
    table = [[1, -1, -1],        # 0: unreachable from 2
             [-1, 3, -1],        # 1
             [-1, 1, 3],         # 2: the start
             [-1, -1, 3],        # 3
             [-1, -1, -1]]       # 4: unreachable, allows nothing -- and is dropped, so it does not count
    dfa = TokenDFA.from_table(table, start=2)
    assert dfa.n_states == 3                                    # 2 -> 0, 1 -> 1, 3 -> 2
    assert dfa.dense().tolist() == [[-1, 1, 2], [-1, 2, -1], [-1, -1, 2]]
    assert dfa.n_classes == 3 and dfa.walk([1, 1, 2, 2]) == 2 and dfa.walk([1, 0]) == -1


def test_from_sequences_accepts_exactly_its_sequences():
    V, eos = 6, 5
    seqs = [[0, 1], [0, 1, 2], [3], [4, 4, 0], [0, 1]]
    dfa = TokenDFA.from_sequences(seqs, V, eos)
    want = {tuple(s) for s in seqs}
    for L in range(0, 5):
        for cand in itertools.product(range(V - 1), repeat=L):
            state = dfa.walk(list(cand))
            accepted = state >= 0 and bool(dfa.allowed(state)[eos])
            assert accepted == (cand in want), cand
    final = dfa.walk([3, eos])
    assert dfa.allowed(final).tolist() == [False] * 5 + [True] and dfa.step(final, eos) == final
    assert dfa.walk([3, eos, eos, eos]) == final and dfa.walk([eos]) == -1
    assert TokenDFA.from_sequences([[]], V, eos).allowed(0).tolist() == [False] * 5 + [True]      # the empty sequence: eos at once


# ---- 4. the constructors' errors ----
def test_from_table_errors():
    for bad in ([[2, 0], [0, 1]], [[-2, 0], [0, 1]], [[0.5, 0], [0, 1]], [0, 1], [[]]):
        with pytest.raises(ValueError):
            TokenDFA.from_table(np.array(bad))
    with pytest.raises(ValueError):
        TokenDFA.from_table([[0, 1], [1, 0]], start=2)
    with pytest.raises(ValueError, match='state 1 allows no token'):
        TokenDFA.from_table([[0, 1], [-1, -1]])
    TokenDFA.from_table([[0, -1], [-1, -1]])                    # the empty state is not reachable: fine
    chain = np.minimum(np.arange(32768) + 1, 32767).reshape(-1, 1)
    with pytest.raises(ValueError, match='more than 32767'):
        TokenDFA.from_table(chain)
    assert TokenDFA.from_table(chain[:32767].clip(max=32766)).n_states == 32767
    S, V = 15, 16385                                            # 16385 distinct columns: bit s of v + 1 decides whether state s allows token v
    bits = ((np.arange(1, V + 1)[None, :] >> np.arange(S)[:, None]) & 1).astype(bool)
    wide = np.where(bits, ((np.arange(S) + 1) % S)[:, None], -1)
    with pytest.raises(ValueError, match='more than 16384'):
        TokenDFA.from_table(wide)
    assert TokenDFA.from_table(wide[:, 2:]).n_classes == 16383


def test_from_sequences_and_from_regex_errors():
    with pytest.raises(ValueError):
        TokenDFA.from_sequences([], 4, 3)
    with pytest.raises(ValueError):
        TokenDFA.from_sequences([[0, 3]], 4, 3)                 # eos inside a sequence
    with pytest.raises(ValueError):
        TokenDFA.from_sequences([[4]], 4, 3)
    with pytest.raises(ValueError):
        TokenDFA.from_sequences([[0]], 4, 4)
    vocab = [b'a', b'b', b'ab', None]
    with pytest.raises(ValueError, match='max_states'):
        TokenDFA.from_regex(r'a{50}', vocab, 3, max_states=10)
    assert TokenDFA.from_regex(r'a{50}', vocab, 3, max_states=52).n_states == 52
    with pytest.raises(ValueError, match='empty'):
        TokenDFA.from_regex(r'[^\x00-\xff]', vocab, 3)          # no byte at all
    with pytest.raises(ValueError, match='empty'):
        TokenDFA.from_regex(r'abc', vocab, 3)                   # a language this vocabulary cannot spell
    with pytest.raises(ValueError):
        TokenDFA.from_regex(r'a', vocab, 4)
    with pytest.raises(ValueError):
        TokenDFA.from_regex(r'a', ['a', b'b'], 1)               # a str where bytes belong


def test_dead_ends_are_cut_at_the_token_level():
    # 'ab' can be spelled, 'ac' cannot finish (no token holds a 'c'): the state behind 'a' stays, but only through 'b'
    dfa = TokenDFA.from_regex(r'ab|ac|x', [b'a', b'b', b'ab', b'x', None], 4)
    assert dfa.allowed(0).tolist() == [True, False, True, True, False]
    assert dfa.allowed(dfa.step(0, 0)).tolist() == [False, True, False, False, False]
    dfa = TokenDFA.from_regex(r'ac|x', [b'a', b'b', b'ab', b'x', None], 4)
    assert dfa.allowed(0).tolist() == [False, False, False, True, False]          # 'a' leads to a dead end: banned at the start


# ---- 5. the mask rule against transformers ----
def test_mask_rule_is_hfs_prefix_constrained_processor():
    """Bit for bit against PrefixConstrainedLogitsProcessor driven by walk / allowed -- with two differences the kernel's rule states, each
    checked on its own: HF ADDS 0 or -inf, so a NaN or a +inf on a banned token gives NaN there (here: 0xFC00, the token is banned) and a -0.0
    on an allowed token becomes +0.0 there (here: the bits are kept).  Everything else, -inf, +inf and NaN on allowed tokens included, has
    equal bits."""
    from transformers import PrefixConstrainedLogitsProcessor
    rng = np.random.default_rng(5)
    V, eos = 400, 399
    vocab = [bytes(rng.choice(np.frombuffer(b'0123456789.-e', dtype=np.uint8), size=rng.integers(1, 4)).tolist()) for _ in range(V - 1)] + [None]
    dfa = TokenDFA.from_regex(r'-?\d+(\.\d+)?(e-?\d+)?', vocab, eos)
    prefixes = [[]]
    while len(prefixes) < 6:                                    # a few prefixes of different lengths, by a seeded walk
        p, state = [], 0
        for _ in range(rng.integers(1, 6)):
            t = int(rng.choice(np.flatnonzero(dfa.allowed(state))))
            if t == eos:
                break
            p.append(t)
            state = dfa.step(state, t)
        prefixes.append(p)
    for prefix in prefixes:
        state = dfa.walk(prefix)
        ok = dfa.allowed(state)
        logits = (3.0 * rng.standard_normal(V)).astype(np.float16)
        plant = np.concatenate([rng.choice(np.flatnonzero(ok), 4, replace=False), rng.choice(np.flatnonzero(~ok), 4, replace=False)])
        for at, bits in zip(plant, (0x7E00, 0x8000, 0xFC00, 0x7C00) * 2):        # NaN, -0.0, -inf, +inf: on allowed AND on banned tokens
            logits.view(np.uint16)[at] = bits
        fn = lambda batch_id, sent: np.flatnonzero(dfa.allowed(dfa.walk(sent.tolist()))).tolist()
        hf = PrefixConstrainedLogitsProcessor(fn, num_beams=1)(torch.tensor([prefix], dtype=torch.int64),
                                                               torch.from_numpy(logits.astype(np.float32))[None].clone())
        hf = hf[0].numpy().astype(np.float16).view(np.uint16)
        ours, st = R.constrain_dfa(logits[None], dfa, [state])
        ours = ours[0].view(np.uint16)
        before = logits.view(np.uint16)
        assert st.tolist() == [state]                           # no token consumed: the state stays
        nan_banned = ~ok & (np.isnan(logits) | (before == 0x7C00))
        zero_allowed = ok & (before == 0x8000)
        assert nan_banned.sum() == 2 and zero_allowed.sum() == 1
        assert np.isnan(hf.view(np.float16)[nan_banned]).all() and (ours[nan_banned] == 0xFC00).all()
        assert (hf[zero_allowed] == 0x0000).all() and (ours[zero_allowed] == 0x8000).all()
        rest = ~(nan_banned | zero_allowed)
        assert np.array_equal(hf[rest], ours[rest])
        assert np.array_equal(ours[ok], before[ok]) and (ours[~ok] == 0xFC00).all()            # exactly the banned positions change
        # ... and with the last token of the prefix consumed by the same call
        if prefix:
            ours2, st2 = R.constrain_dfa(logits[None], dfa, [dfa.walk(prefix[:-1])], last=[prefix[-1]])
            assert st2.tolist() == [state] and np.array_equal(ours2.view(np.uint16)[0], ours)


def test_restatement_rules_by_hand():
    nxt = np.array([[1, -1, 0], [-1, 1, 7]], dtype=np.int16)   # 2 states, 3 classes; the 7 is garbage (>= n_states)
    cls = np.array([[0, 1, 2, 5, -3]], dtype=np.int16)         # ... as are the classes 5 and -3
    logits = np.arange(1, 13, dtype=np.float16).reshape(2, 6)  # ld = 6 > vocab = 5
    inf = -np.inf
    out, st = R.constrain_rows(logits, 5, nxt, 2, 3, cls, [0, 0], [0, 1], None, [0, 0], 0, 0)
    assert out.tolist() == [[1, inf, 3, inf, inf, 6], [inf, 8, inf, inf, inf, 12]] and st.tolist() == [0, 1]
    out, st = R.constrain_rows(logits, 5, nxt, 2, 3, cls, [0, 0], [0, 1], [0, 2], [0, 0], 0, 0)
    assert st.tolist() == [1, -2] and out[0].tolist() == [inf, 2, inf, inf, inf, 6] and out[1].tolist() == logits[1].tolist()
    for last in ([1, 3], [-1, 5], [4, 2 ** 40]):               # banned, out of range, a garbage class
        out, st = R.constrain_rows(logits, 5, nxt, 2, 3, cls, [0, 0], [0, 0], last, [0, 0], 0, 0)
        assert st.tolist() == [-2, -2] and np.array_equal(out, logits)
    out, st = R.constrain_rows(logits, 5, nxt, 2, 3, cls, [0, 1], [2, 0], None, [0, 0], 0, 0)       # a state, a map outside the tables
    assert st.tolist() == [-2, -2] and np.array_equal(out, logits)
    out, st = R.constrain_rows(logits, 5, nxt, 2, 3, cls, [0, 0], [-1, -2], [0, 0], [0, 0], 0, 0)   # switched off
    assert st.tolist() == [-1, -2] and np.array_equal(out, logits)
    out, st = R.constrain_rows(logits, 5, nxt, 2, 3, cls, [0, 0], [0, 0], [0, 0], [0, 9], -1, 7)    # idle on both sides
    assert st.tolist() == [0, 0] and np.array_equal(out, logits)


# ---- 6. the C entry's validation, on fake pointers ----
_PTRS = dict(logits=4096, next=8192, cls=12288, map_of=16384, state=20480, last=24576, len=28672)


def _call(lib, ld=1000, seqs=2, vocab=1000, ld_next=300, n_states=5, n_classes=300, ld_cls=1000, n_maps=2, len_add=-1, t_limit=63, **ptrs):
    p = dict(_PTRS, **ptrs)
    return lib.gptq_constrain_rows_f16(p['logits'], ld, seqs, vocab, p['next'], ld_next, n_states, n_classes, p['cls'], ld_cls, n_maps,
                                       p['map_of'], p['state'], p['last'], p['len'], len_add, t_limit, None)


def test_symbol_is_exported_and_bound():
    lib = _native.lib()
    assert hasattr(lib, 'gptq_constrain_rows_f16') and 'gptq_constrain_rows_f16' in _native.EXPORTS
    assert len(lib.gptq_constrain_rows_f16.argtypes) == 18


def test_null_rules():
    lib = _native.lib()
    for name in ('logits', 'next', 'cls', 'map_of', 'state', 'len'):
        assert _call(lib, **{name: None}) == E_NULL, name
    assert _call(lib, next=None, vocab=0) == E_NULL                            # NULL is reported before any shape rule
    assert _call(lib, len=None, state=20480 + 2) == E_NULL                     # ... and before any alignment rule
    assert _call(lib, last=None, seqs=0) == E_SHAPE                            # `last` may be NULL: this reaches the shape rules


def test_shape_rules():
    lib = _native.lib()
    for kw in (dict(seqs=0), dict(seqs=65536), dict(vocab=0, ld=0), dict(ld=999), dict(n_states=0), dict(n_states=32768), dict(n_classes=0),
               dict(n_classes=16385, ld_next=16385), dict(ld_next=299), dict(ld_cls=999), dict(n_maps=0)):
        assert _call(lib, **kw) == E_SHAPE, kw
    assert _call(lib, seqs=0, map_of=16384 + 2) == E_SHAPE                     # shape before alignment


def test_alignment_rules():
    lib = _native.lib()
    for name in ('logits', 'next', 'cls'):
        assert _call(lib, **{name: _PTRS[name] + 1}) == E_ALIGN, name          # fp16 rows and int16 tables: 2 bytes, nothing more
    for name in ('map_of', 'state'):
        assert _call(lib, **{name: _PTRS[name] + 2}) == E_ALIGN, name          # int32 arrays: 4 bytes
    for name in ('last', 'len'):
        assert _call(lib, **{name: _PTRS[name] + 4}) == E_ALIGN, name          # int64 arrays: 8 bytes


# ---- 7. llama_vocab_bytes ----
def test_llama_vocab_bytes_on_hand_made_pieces():
    pieces = ['<unk>', '<s>', '</s>', '<0x0A>', '<0xff>', '▁the', 'ing', '▁', '▁▁', 'é', '<0x4G>', None, '<0x41>x']
    out = llama_vocab_bytes(pieces, special_ids=(0, 1, 2))
    assert out == [None, None, None, b'\n', b'\xff', b' the', b'ing', b' ', b'  ', 'é'.encode(), b'<0x4G>', None, b'<0x41>x']
    assert llama_vocab_bytes(pieces)[:3] == [b'<unk>', b'<s>', b'</s>'] and llama_vocab_bytes([]) == []
    dfa = TokenDFA.from_regex(r' the(ing)*\n', out, 2)         # and it feeds from_regex as it is
    assert dfa.walk([5, 6, 6, 3, 2]) >= 0 and dfa.walk([6]) == -1
