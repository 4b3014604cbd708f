"""gptq_decode_attn_batch_gqa_f16 and its workspace query without a GPU: the symbols, their bindings, and the validation that returns before any
launch (the pointers of the bad calls are never dereferenced)."""
import os
import re

import pytest

from quant import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('gptq_decode_attn_batch_gqa_f16', 'gptq_decode_attn_batch_gqa_workspace_bytes')
P = 0x10000                                   # a 16-byte aligned address nobody reads
HD = 128
GOOD = dict(qkv=P, ldq=(8 + 2 * 2) * HD, pos=P, kc=P, vc=P, out=P, ldo=8 * HD, ws=P, ws_bytes=1 << 30, batch=3, heads=8, kv_heads=2, hd=HD, t_max=384,
            base=10000.0, scale=0.0884, table=None, perm=None, stream=None)
E_SHAPE, E_ALIGN, E_NULL, E_WORKSPACE = -2, -3, -4, -5


@pytest.mark.parametrize('name', NAMES)
def test_symbols_are_exported_bound_and_declared(name):
    hdr = open(os.path.join(ROOT, 'include', 'gptq_mi355x.h')).read()
    decl = re.search(r'(?:int|size_t) %s\(([^;]*)\);' % name, hdr)
    assert decl and name in _native.EXPORTS and hasattr(_native.lib(), name)
    assert len(decl.group(1).split(',')) == len(getattr(_native.lib(), name).argtypes) == (len(GOOD) if name == NAMES[0] else 5)


BAD = [(dict(hd=64), E_SHAPE), (dict(kv_heads=0), E_SHAPE), (dict(kv_heads=3), E_SHAPE), (dict(kv_heads=8), E_SHAPE),       # G = 1: the ungrouped entry's
       (dict(heads=34, kv_heads=2, ldq=38 * HD, ldo=34 * HD), E_SHAPE),                                                     # G = 17
       (dict(batch=0), E_SHAPE), (dict(batch=17), E_SHAPE), (dict(t_max=0), E_SHAPE), (dict(ldq=12 * HD - 8), E_SHAPE), (dict(ldo=8 * HD - 8), E_SHAPE),
       (dict(qkv=None), E_NULL), (dict(pos=None), E_NULL), (dict(kc=None), E_NULL), (dict(vc=None), E_NULL), (dict(out=None), E_NULL),
       (dict(ws=None), E_NULL), (dict(qkv=None, hd=64), E_NULL),                                                            # NULL is reported first
       (dict(qkv=P + 8), E_ALIGN), (dict(kc=P + 8), E_ALIGN), (dict(vc=P + 4), E_ALIGN), (dict(out=P + 2), E_ALIGN), (dict(ws=P + 8), E_ALIGN),
       (dict(pos=P + 4), E_ALIGN), (dict(table=P + 4), E_ALIGN), (dict(perm=P + 2), E_ALIGN), (dict(ldq=12 * HD + 4), E_ALIGN),
       (dict(ldo=8 * HD + 4), E_ALIGN), (dict(hd=64, qkv=P + 2), E_SHAPE),                                                  # SHAPE before ALIGN
       (dict(ws_bytes=0), E_WORKSPACE)]


@pytest.mark.parametrize('bad,code', BAD)
def test_bad_calls_are_refused_before_the_launch(bad, code):
    assert _native.lib().gptq_decode_attn_batch_gqa_f16(*{**GOOD, **bad}.values()) == code


def test_workspace_query():
    lib = _native.lib()
    need = lib.gptq_decode_attn_batch_gqa_workspace_bytes(3, 8, 2, HD, 384)
    assert need > 0 and lib.gptq_decode_attn_batch_gqa_f16(*{**GOOD, 'ws_bytes': need - 1}.values()) == E_WORKSPACE
    for G in range(2, 17):                                        # every group size 2 .. 16, 7 included
        assert lib.gptq_decode_attn_batch_gqa_workspace_bytes(1, 2 * G, 2, HD, 64) > 0, G
    for args in ((1, 8, 8, HD, 64), (1, 34, 2, HD, 64), (1, 8, 3, HD, 64), (1, 8, 2, 64, 64), (17, 8, 2, HD, 64), (1, 8, 2, HD, 0)):
        assert lib.gptq_decode_attn_batch_gqa_workspace_bytes(*args) == 0, args
