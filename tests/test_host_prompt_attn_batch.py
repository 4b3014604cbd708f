"""CPU-side tests of gptq_prompt_attn_batch_f16 (include/gptq_mi355x.h "prompt prefill"): the symbol is exported and bound with its segment
struct, and every rule of the host validation returns its code on fake aligned pointers -- nothing is launched, no device is needed."""
import ctypes

from quant import _native

HEADS, HD, T_MAX = 4, 128, 384
H = HEADS * HD
E_SHAPE, E_ALIGN, E_NULL, E_WORKSPACE = -2, -3, -4, -5
GOOD = [(0, 8, 0, 0), (8, 5, 10, 2), (16, 1, 383, 1)]      # (row0, rows, start, slot)
TOTAL = 20


def _table(segs):
    return (_native.PromptSeg * max(1, len(segs)))(*[_native.PromptSeg(*s) for s in segs])


def _call(lib, segs=GOOD, nseq=None, qkv=4096, ldq=3 * H, total=TOTAL, kc=4096, vc=4096, stride=T_MAX * H, out=4096, ldo=H, ws=4096,
          ws_bytes=1 << 30, heads=HEADS, hd=HD, t_max=T_MAX, table=None):
    """fake, aligned, non-NULL "device pointers": every failing case below is refused before anything is launched"""
    tab = None if segs is None else _table(segs)
    n = (0 if segs is None else len(segs)) if nseq is None else nseq
    return lib.gptq_prompt_attn_batch_f16(qkv, ldq, total, tab, n, kc, vc, stride, out, ldo, ws, ws_bytes, heads, hd, t_max, 10000.0, 0.088,
                                          table, None)


def test_prompt_attn_batch_symbol_is_exported_and_bound():
    lib = _native.lib()
    assert hasattr(lib, 'gptq_prompt_attn_batch_f16')
    assert 'gptq_prompt_attn_batch_f16' in _native.EXPORTS
    assert lib.gptq_prompt_attn_batch_f16.argtypes is not None and len(lib.gptq_prompt_attn_batch_f16.argtypes) == 19
    assert _native.PROMPT_ATTN_MAX_SEQS == 16
    assert ctypes.sizeof(_native.PromptSeg) == 16                  # four int32: 16 of them are the 256 bytes of the launch arguments
    assert [f[0] for f in _native.PromptSeg._fields_] == ['row0', 'rows', 'start', 'slot']


def test_prompt_attn_batch_shape_rules():
    lib = _native.lib()
    assert _call(lib, segs=[], nseq=0) == E_SHAPE                  # nseq outside 1 .. 16
    assert _call(lib, nseq=-1) == E_SHAPE
    seventeen = [(i, 1, 0, i) for i in range(17)]
    assert _call(lib, segs=seventeen, stride=T_MAX * H) == E_SHAPE
    assert _call(lib, hd=64) == E_SHAPE
    assert _call(lib, hd=256) == E_SHAPE
    assert _call(lib, heads=0) == E_SHAPE
    assert _call(lib, heads=-2) == E_SHAPE
    assert _call(lib, segs=[(0, 0, 0, 0)]) == E_SHAPE              # rows <= 0
    assert _call(lib, segs=[(0, 8, 0, 0), (8, -1, 0, 1)]) == E_SHAPE
    assert _call(lib, segs=[(0, 8, -1, 0)]) == E_SHAPE             # start < 0
    assert _call(lib, segs=[(0, 8, T_MAX - 7, 0)]) == E_SHAPE      # start + rows = t_max + 1
    assert _call(lib, segs=[(0, 8, T_MAX - 8, 0)], ws_bytes=0) == E_WORKSPACE    # start + rows = t_max passes the shape rules
    assert _call(lib, segs=[(0, 8, 0, -1)]) == E_SHAPE             # slot < 0
    assert _call(lib, stride=T_MAX * H - 8) == E_SHAPE             # slices would overlap
    assert _call(lib, segs=[(-1, 8, 0, 0)]) == E_SHAPE             # row range outside [0, total_rows)
    assert _call(lib, segs=[(13, 8, 0, 0)]) == E_SHAPE             # 13 + 8 > 20
    assert _call(lib, total=0) == E_SHAPE
    assert _call(lib, segs=[(0, 8, 0, 0), (7, 5, 0, 1)]) == E_SHAPE            # row ranges overlap
    assert _call(lib, segs=[(4, 2, 0, 0), (0, 12, 0, 1)]) == E_SHAPE           # one inside the other, either order
    assert _call(lib, segs=[(0, 8, 0, 2), (8, 5, 10, 2)]) == E_SHAPE           # the same slot twice: one would read what the other writes
    assert _call(lib, segs=[(0, 8, 0, 1), (8, 5, 8, 3), (13, 1, 0, 1)]) == E_SHAPE
    assert _call(lib, ldq=3 * H - 8) == E_SHAPE
    assert _call(lib, ldo=H - 8) == E_SHAPE


def test_prompt_attn_batch_null_align_and_workspace():
    lib = _native.lib()
    for name in ('qkv', 'kc', 'vc', 'out', 'ws'):
        assert _call(lib, **{name: None}) == E_NULL, name
    assert _call(lib, segs=None, nseq=3) == E_NULL                 # segs = NULL
    assert _call(lib, qkv=4096 + 2) == E_ALIGN
    assert _call(lib, kc=4096 + 8) == E_ALIGN
    assert _call(lib, ldq=3 * H + 4) == E_ALIGN
    assert _call(lib, ldo=H + 4) == E_ALIGN
    assert _call(lib, stride=T_MAX * H + 4) == E_ALIGN             # a slice must begin on 16 bytes
    assert _call(lib, table=4096 + 4) == E_ALIGN
    # the workspace is that of the single-sequence entry for total_rows: one fp16 copy of the rotated q, no query of its own
    need = lib.gptq_prompt_attn_workspace_bytes(TOTAL, HEADS, HD, T_MAX)
    assert need >= TOTAL * H * 2
    assert _call(lib, ws_bytes=need - 1) == E_WORKSPACE
    assert _call(lib, ws_bytes=0) == E_WORKSPACE
    # the packed rows of a batch may outnumber one sequence's cache rows
    big = lib.gptq_prompt_attn_workspace_bytes(16 * T_MAX, HEADS, HD, T_MAX)
    assert 16 * T_MAX * H * 2 <= big <= 16 * T_MAX * H * 2 + 4096
    full = [(i * T_MAX, T_MAX, 0, 15 - i) for i in range(16)]
    assert _call(lib, segs=full, total=16 * T_MAX, ws_bytes=big - 1) == E_WORKSPACE
