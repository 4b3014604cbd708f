"""CPU-side tests of gptq_lm_head_nll_f16 (include/gptq_mi355x.h "scoring"): the symbol is exported and bound, every rule of the host validation
returns its code on fake aligned pointers -- nothing is launched, no device is needed -- and the workspace query covers one 16-byte record per
row and 256-column tile."""
from quant import _native

E_SHAPE, E_ALIGN, E_NULL, E_WORKSPACE, E_VARIANT = -2, -3, -4, -5, -6
M, N, K = 33, 1000, 256
REC = 16          # bytes of a record {max, sumexp, argidx, z_target}


def _call(lib, x=4096, ldx=K, w=8192, ldw=K, bias=None, targets=4096, nll=4096, lse=4096, argmax=4096, m=M, n=N, k=K, ws=4096, ws_bytes=1 << 30):
    """fake, aligned, non-NULL "device pointers": every failing case below is refused before anything is launched"""
    return lib.gptq_lm_head_nll_f16(x, ldx, w, ldw, bias, targets, nll, lse, argmax, m, n, k, ws, ws_bytes, None)


def test_lm_head_nll_symbol_is_exported_and_bound():
    lib = _native.lib()
    for name, nargs in (('gptq_lm_head_nll_f16', 15), ('gptq_lm_head_nll_workspace_bytes', 2)):
        assert hasattr(lib, name)
        assert name in _native.EXPORTS
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == nargs


def test_lm_head_nll_null_rules():
    lib = _native.lib()
    for name in ('x', 'w', 'targets', 'nll', 'ws'):
        assert _call(lib, **{name: None}) == E_NULL, name
    # the optional outputs and the bias may be NULL: the call then gets as far as the workspace rule
    assert _call(lib, lse=None, argmax=None, bias=None, ws_bytes=0) == E_WORKSPACE
    # NULL is reported before any shape rule
    assert _call(lib, x=None, n=0) == E_NULL


def test_lm_head_nll_shape_rules():
    lib = _native.lib()
    assert _call(lib, m=-1) == E_SHAPE
    assert _call(lib, n=0) == E_SHAPE
    assert _call(lib, n=-5) == E_SHAPE
    assert _call(lib, k=0) == E_SHAPE
    assert _call(lib, k=-128) == E_SHAPE
    assert _call(lib, ldx=K - 8) == E_SHAPE
    assert _call(lib, ldw=K - 8) == E_SHAPE
    assert _call(lib, ldx=K + 8, ldw=K + 16, ws_bytes=0) == E_WORKSPACE        # padded rows pass the shape and alignment rules
    assert _call(lib, n=1, ws_bytes=0) == E_WORKSPACE                          # any N >= 1
    assert _call(lib, n=32001, ws_bytes=0) == E_WORKSPACE


def test_lm_head_nll_alignment_rules():
    lib = _native.lib()
    assert _call(lib, x=4096 + 8) == E_ALIGN                                   # x, weight: 16 bytes (the rules of the tile GEMM)
    assert _call(lib, w=8192 + 8) == E_ALIGN
    assert _call(lib, ldx=K + 4) == E_ALIGN                                    # rows must begin on 16 bytes
    assert _call(lib, ldw=K + 4) == E_ALIGN
    assert _call(lib, bias=4096 + 4) == E_ALIGN                                # bias: 8 bytes
    assert _call(lib, bias=4096 + 8, ws_bytes=0) == E_WORKSPACE
    assert _call(lib, targets=4096 + 4) == E_ALIGN                             # int64 targets: 8 bytes
    assert _call(lib, nll=4096 + 2) == E_ALIGN                                 # float / int outputs: 4 bytes
    assert _call(lib, lse=4096 + 2) == E_ALIGN
    assert _call(lib, argmax=4096 + 1) == E_ALIGN
    assert _call(lib, nll=4096 + 4, lse=4096 + 4, argmax=4096 + 4, ws_bytes=0) == E_WORKSPACE
    assert _call(lib, ws=4096 + 8) == E_ALIGN                                  # 16-byte records


def test_lm_head_nll_workspace_variant_and_empty():
    lib = _native.lib()
    need = lib.gptq_lm_head_nll_workspace_bytes(M, N)
    assert need >= M * ((N + 255) // 256) * REC
    assert _call(lib, ws_bytes=need - 1) == E_WORKSPACE
    assert _call(lib, ws_bytes=0) == E_WORKSPACE
    # K % 128 != 0: declined (the caller falls back), after every other rule
    assert _call(lib, k=192, ldx=192, ldw=192) == E_VARIANT
    assert _call(lib, k=200, ldx=200, ldw=200) == E_VARIANT
    assert _call(lib, k=192, ldx=192, ldw=192, ws_bytes=0) == E_WORKSPACE
    assert _call(lib, k=192, ldx=192, ldw=192, x=None) == E_NULL
    # no rows: nothing to do, nothing launched (the pointers are fake)
    assert _call(lib, m=0, ws_bytes=0) == 0
    assert _call(lib, m=0, k=192, ldx=192, ldw=192) == E_VARIANT


def test_lm_head_nll_workspace_query():
    lib = _native.lib()
    q = lib.gptq_lm_head_nll_workspace_bytes
    assert q(1, 1) > 0
    for m in (1, 33, 257, 2047):
        for n in (1, 256, 257, 1000, 2049, 32000, 32001):
            assert q(m, n) >= m * ((n + 255) // 256) * REC, (m, n)
            assert q(m + 1, n) >= q(m, n) and q(m, n + 1) >= q(m, n) and q(m, n + 256) > q(m, n), (m, n)
    # records only: about 4 MB at 2047 x 32000, never the logits
    assert q(2047, 32000) <= 2047 * 125 * REC + 4096
