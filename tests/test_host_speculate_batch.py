"""CPU-side tests of batched speculative decoding: the C entry gptq_decode_attn_chunk_batch_f16 (csrc/chunk_attn.hip) is exported, bound and
validates its arguments on the host before anything is launched, its workspace function answers 0 for the shapes it does not serve, and the
speculate settings engine_generate_batch shares with engine_generate are what they were."""
import pytest

from quant import _native
from quant.decode import _speculate_settings

E_SHAPE, E_ALIGN, E_NULL = -2, -3, -4          # GPTQ_E_SHAPE, GPTQ_E_ALIGN, GPTQ_E_NULL (include/gptq_mi355x.h)
HEADS, HD, T_MAX = 32, 128, 2048
H = HEADS * HD


def test_both_symbols_are_exported_and_bound():
    lib = _native.lib()
    for name in ('gptq_decode_attn_chunk_batch_f16', 'gptq_decode_attn_chunk_batch_workspace_bytes'):
        assert hasattr(lib, name) and name in _native.EXPORTS
    assert len(lib.gptq_decode_attn_chunk_batch_f16.argtypes) == 19
    assert len(lib.gptq_decode_attn_chunk_batch_workspace_bytes.argtypes) == 5


def test_workspace_bytes():
    ws = _native.lib().gptq_decode_attn_chunk_batch_workspace_bytes
    need = ws(4, 5, HEADS, HD, T_MAX)
    assert need > 0 and need % 16 == 0
    assert ws(4, 5, HEADS, 64, T_MAX) == 0                     # head_dim 64
    assert ws(17, 5, HEADS, HD, T_MAX) == 0 and ws(0, 5, HEADS, HD, T_MAX) == 0
    assert ws(4, 17, HEADS, HD, T_MAX) == 0 and ws(4, 0, HEADS, HD, T_MAX) == 0
    assert ws(16, 9, HEADS, HD, T_MAX) == 0 and ws(9, 15, HEADS, HD, T_MAX) == 0      # seqs x rows > 128
    assert ws(16, 8, HEADS, HD, T_MAX) > 0                     # ... and the limit itself is served
    assert ws(4, 5, 0, HD, T_MAX) == 0 and ws(4, 5, HEADS, HD, 0) == 0
    # one sequence: the size of the single-sequence entry (which keeps its own); more sequences need more, never less than B times the records
    single = _native.lib().gptq_decode_attn_chunk_workspace_bytes
    for rows in (1, 5, 16):
        assert ws(1, rows, HEADS, HD, T_MAX) == single(rows, HEADS, HD, T_MAX)
    assert need > single(5, HEADS, HD, T_MAX)


def test_every_validation_rule_on_the_host():
    lib = _native.lib()
    seqs, rows = 4, 5
    need = lib.gptq_decode_attn_chunk_batch_workspace_bytes(seqs, rows, HEADS, HD, T_MAX)
    P = 4096                                                   # any aligned non-NULL address: nothing is launched
    stride = T_MAX * H
    ok = dict(qkv=P, ldq=3 * H, seqs=seqs, rows=rows, pos=P, k=P, v=P, stride=stride, out=P, ldo=H, ws=P, wb=need, heads=HEADS, hd=HD, tm=T_MAX,
              tab=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gptq_decode_attn_chunk_batch_f16(a['qkv'], a['ldq'], a['seqs'], a['rows'], a['pos'], a['k'], a['v'], a['stride'], a['out'], a['ldo'],
                                                    a['ws'], a['wb'], a['heads'], a['hd'], a['tm'], 10000.0, 0.088, a['tab'], None)
    for name in ('qkv', 'pos', 'k', 'v', 'out', 'ws'):
        assert call(**{name: None}) == E_NULL, name
    for kw in (dict(seqs=0), dict(seqs=17), dict(seqs=-1), dict(rows=0), dict(rows=17), dict(rows=-2),
               dict(seqs=16, rows=9), dict(seqs=9, rows=15),                          # seqs x rows > 128 (with a workspace that would do)
               dict(hd=64), dict(hd=256), dict(heads=0), dict(heads=-1), dict(tm=0), dict(tm=-5),
               dict(ldq=3 * H - 8), dict(ldo=H - 8), dict(stride=stride - 8), dict(stride=0),
               dict(wb=need - 1), dict(wb=0)):
        big = dict(wb=1 << 40) if 'seqs' in kw and 'rows' in kw else {}
        assert call(**dict(big, **kw)) == E_SHAPE, kw
    for kw in (dict(qkv=P + 8), dict(k=P + 8), dict(v=P + 2), dict(out=P + 8), dict(ws=P + 8), dict(pos=P + 4), dict(tab=P + 4),
               dict(ldq=3 * H + 4), dict(ldo=H + 4), dict(stride=stride + 4)):
        assert call(**kw) == E_ALIGN, kw
    # the largest request is refused for its workspace, not for its shape: 16 x 8 rows with the workspace of 4 x 5
    assert call(seqs=16, rows=8) == E_SHAPE
    assert lib.gptq_decode_attn_chunk_batch_workspace_bytes(16, 8, HEADS, HD, T_MAX) > need


def test_speculate_settings_are_unchanged():
    assert _speculate_settings({}) == (4, 3, None)
    f = lambda toks, k: [0] * k
    assert _speculate_settings(dict(k=15, max_ngram=1, draft=f)) == (15, 1, f)
    for bad in (dict(k=0), dict(k=16), dict(k=True), dict(k=2.0), dict(max_ngram=0), dict(draft=3), dict(depth=2), [4]):
        with pytest.raises(ValueError):
            _speculate_settings(bad)
