"""CPU-side tests of the speculative-decoding pieces that need no GPU: prompt_lookup_draft (quant/decode.py: the default draft source of
engine_generate(speculate=...)), the speculate settings, and the C entry's host-side validation."""
import numpy as np
import pytest

from quant import _native
from quant.decode import _speculate_settings, prompt_lookup_draft


def test_longest_ngram_first():
    # the 1-gram [2] last occurred in front of 9, the 2-gram [1, 2] in front of 8, the 3-gram [7, 1, 2] in front of 5: the longest match decides
    seq = [7, 1, 2, 5, 6, 1, 2, 8, 3, 2, 9, 7, 1, 2]
    assert prompt_lookup_draft(seq, 1, max_ngram=3) == [5]
    assert prompt_lookup_draft(seq, 1, max_ngram=2) == [8]
    assert prompt_lookup_draft(seq, 1, max_ngram=1) == [9]


def test_most_recent_occurrence():
    seq = [1, 2, 10, 4, 1, 2, 20, 4, 1, 2]
    assert prompt_lookup_draft(seq, 2, max_ngram=2) == [20, 4]
    assert prompt_lookup_draft(seq, 3, max_ngram=3) == [20, 4, 1]          # [4, 1, 2] matched once, at 3 .. 5


def test_continuation_past_the_end_of_the_match():
    # [1, 2] matched at 0: only [3, 1, 2] follows inside the sequence; the lookup goes on from [.., 3, 1, 2] and finds [3, 1, 2] -> [3, 1]
    assert prompt_lookup_draft([1, 2, 3, 1, 2], 5) == [3, 1, 2, 3, 1]
    assert prompt_lookup_draft([4, 4], 6) == [4] * 6


def test_no_match_repeats_the_last_token():
    assert prompt_lookup_draft([1, 2, 3], 3) == [3, 3, 3]
    assert prompt_lookup_draft([5], 2) == [5, 5]


@pytest.mark.parametrize('k', [0, 1, 4, 15])
def test_always_k_ids(k):
    rng = np.random.default_rng(k)
    for n in (1, 2, 3, 17, 200):
        seq = rng.integers(0, 5, size=n)
        for arg in (seq, seq.tolist()):                                    # numpy or list in, list of ints out
            d = prompt_lookup_draft(arg, k)
            assert isinstance(d, list) and len(d) == k and all(isinstance(t, int) and 0 <= t < 5 for t in d)


def test_sequence_shorter_than_the_ngram():
    assert prompt_lookup_draft([9, 9], 2, max_ngram=3) == [9, 9]           # only the 1-gram can match
    assert prompt_lookup_draft([3, 8], 2, max_ngram=5) == [8, 8]
    assert prompt_lookup_draft([6, 3, 6], 2, max_ngram=3) == [3, 6]


def test_max_ngram_one():
    assert prompt_lookup_draft([7, 1, 7, 2, 7], 2, max_ngram=1) == [2, 7]


def test_bad_arguments():
    for args in (([], 2), ([1], -1), ([1], 2, 0)):
        with pytest.raises(ValueError):
            prompt_lookup_draft(*args)


def test_speculate_settings():
    assert _speculate_settings({}) == (4, 3, None)
    f = lambda toks, k: [0] * k
    assert _speculate_settings(dict(k=15, max_ngram=1, draft=f)) == (15, 1, f)
    for bad in (dict(k=0), dict(k=16), dict(k=True), dict(k=2.0), dict(max_ngram=0), dict(draft=3), dict(depth=2), [4]):
        with pytest.raises(ValueError):
            _speculate_settings(bad)


def test_chunk_attention_entry_is_exported_and_validates_on_the_host():
    lib = _native.lib()
    for name in ('gptq_decode_attn_chunk_f16', 'gptq_decode_attn_chunk_workspace_bytes', 'gptq_decode_attn_chunk_splits'):
        assert hasattr(lib, name) and name in _native.EXPORTS
    assert len(lib.gptq_decode_attn_chunk_f16.argtypes) == 17
    need = lib.gptq_decode_attn_chunk_workspace_bytes(5, 32, 128, 2048)
    assert 0 < need < (1 << 20) and need % 16 == 0
    assert lib.gptq_decode_attn_chunk_workspace_bytes(5, 32, 64, 2048) == 0 and lib.gptq_decode_attn_chunk_workspace_bytes(17, 32, 128, 2048) == 0
    # the split rule at the 7B shape: one workgroup per head for short contexts, one per CU (32 heads x 8) at 2 047 tokens
    assert lib.gptq_decode_attn_chunk_splits(32, 128, 2048, 200) == 1
    assert lib.gptq_decode_attn_chunk_splits(32, 128, 2048, 300) == 2
    assert lib.gptq_decode_attn_chunk_splits(32, 128, 2048, 2047) == 8
    assert lib.gptq_decode_attn_chunk_splits(64, 128, 2048, 2047) == 4         # heads x splits <= 256
    assert lib.gptq_decode_attn_chunk_splits(32, 128, 2048, 0) == -2 and lib.gptq_decode_attn_chunk_splits(32, 128, 2048, 2049) == -2
    P = 4096                                                                   # any aligned non-NULL address: nothing is launched
    ok = dict(qkv=P, ldq=3 * 4096, rows=5, pos=P, k=P, v=P, out=P, ldo=4096, ws=P, wb=need)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gptq_decode_attn_chunk_f16(a['qkv'], a['ldq'], a['rows'], a['pos'], a['k'], a['v'], a['out'], a['ldo'], a['ws'], a['wb'], 32,
                                              a.get('hd', 128), 2048, 10000.0, 0.088, None, None)
    for name in ('qkv', 'pos', 'k', 'v', 'out', 'ws'):
        assert call(**{name: None}) == -4, name                                # GPTQ_E_NULL
    for kw in (dict(rows=0), dict(rows=17), dict(hd=64), dict(ldq=3 * 4096 - 8), dict(ldo=4088), dict(wb=need - 1)):
        assert call(**kw) == -2, kw                                            # GPTQ_E_SHAPE
    for kw in (dict(qkv=P + 8), dict(pos=P + 4), dict(k=P + 2), dict(v=P + 8), dict(out=P + 8), dict(ws=P + 8), dict(ldq=3 * 4096 + 4), dict(ldo=4100)):
        assert call(**kw) == -3, kw                                            # GPTQ_E_ALIGN
