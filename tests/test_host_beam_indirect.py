"""CPU-side tests of the beam cache indirection (include/gptq_mi355x.h): the four symbols are exported, bound and declared, and the NULL / shape /
alignment / workspace rules return their codes on fake pointers (nothing is launched), NULL before shape before alignment."""
import os

from quant import _native

E_SHAPE, E_ALIGN, E_NULL, E_WORKSPACE = -2, -3, -4, -5


def test_symbols_are_exported_bound_and_declared():
    lib = _native.lib()
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'gptq_mi355x.h')).read()
    for name, nargs in (('gptq_beam_src_update_u8', 7), ('gptq_decode_attn_beam_ws_bytes', 3), ('gptq_decode_attn_beam_splits', 4),
                        ('gptq_decode_attn_beam_f16', 21)):
        assert hasattr(lib, name) and name in _native.EXPORTS and name + '(' in header
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert lib.gptq_decode_attn_beam_ws_bytes(4, 32, 2048) > 0
    assert [lib.gptq_decode_attn_beam_ws_bytes(*a) for a in ((0, 32, 2048), (17, 32, 2048), (4, 0, 2048), (4, 32, 0))] == [0] * 4
    assert lib.gptq_decode_attn_beam_splits(32, 128, 2048, 1) == 1 and lib.gptq_decode_attn_beam_splits(32, 128, 2048, 2048) == 8
    assert [lib.gptq_decode_attn_beam_splits(*a) for a in ((32, 64, 2048, 5), (32, 128, 2048, 0), (32, 128, 2048, 2049))] == [E_SHAPE] * 3


def test_src_update_validation():
    def call(src=4096, beams=4, t_max=64, parent=8192, len_=16384, common=32768):
        return _native.lib().gptq_beam_src_update_u8(src, beams, t_max, parent, len_, common, None)
    assert [call(**{name: None, 'beams': 0}) for name in ('src', 'parent', 'len_', 'common')] == [E_NULL] * 4
    assert [call(**kw) for kw in (dict(beams=0), dict(beams=17), dict(t_max=0), dict(beams=17, parent=8194))] == [E_SHAPE] * 4
    assert [call(**kw) for kw in (dict(parent=8194), dict(len_=16388), dict(common=32770))] == [E_ALIGN] * 3


def test_attention_validation():
    lib = _native.lib()

    def call(**kw):
        a = dict(qkv=1 << 20, ldq=3 * 384, beams=4, pos=8192, k=2 << 20, v=3 << 20, stride=64 * 384, src=4096, common=16384, out=4 << 20, ldo=384,
                 perm=None, ws=5 << 20, ws_bytes=1 << 30, heads=3, hd=128, t_max=64, tab=None)
        a.update(kw)
        return lib.gptq_decode_attn_beam_f16(a['qkv'], a['ldq'], a['beams'], a['pos'], a['k'], a['v'], a['stride'], a['src'], a['common'], a['out'],
                                             a['ldo'], a['perm'], a['ws'], a['ws_bytes'], a['heads'], a['hd'], a['t_max'], 1e4, 0.0884, a['tab'], None)
    assert [call(**{name: None, 'beams': 0}) for name in ('qkv', 'pos', 'k', 'v', 'src', 'common', 'out', 'ws')] == [E_NULL] * 8
    for kw in (dict(beams=0), dict(beams=17, out=(4 << 20) + 8), dict(heads=0), dict(hd=64), dict(t_max=0), dict(ldq=3 * 384 - 8), dict(ldo=376),
               dict(stride=64 * 384 - 8)):
        assert call(**kw) == E_SHAPE, kw
    for kw in (dict(qkv=(1 << 20) + 8), dict(pos=8196), dict(k=(2 << 20) + 8), dict(v=(3 << 20) + 8), dict(ws=(5 << 20) + 8), dict(tab=4100),
               dict(common=16386), dict(perm=4098), dict(ldq=3 * 384 + 4), dict(ldo=388), dict(stride=64 * 384 + 4), dict(out=(4 << 20) + 8)):
        assert call(**kw) == E_ALIGN, kw
    assert call(ws_bytes=lib.gptq_decode_attn_beam_ws_bytes(4, 3, 64) - 1) == E_WORKSPACE
