"""CPU-side tests of the prompt-attention entries (gptq_prompt_attn_f16, include/gptq_mi355x.h "prompt prefill"): the symbols are
exported and bound, argument validation and the workspace formula are host logic -- nothing is launched, no device is needed."""
from quant import _native

HEADS, HD, T_MAX = 4, 128, 384
H = HEADS * HD


def _call(lib, qkv=4096, ldq=3 * H, rows=8, start=0, kc=4096, vc=4096, out=4096, ldo=H, ws=4096, ws_bytes=1 << 30, heads=HEADS, hd=HD,
          t_max=T_MAX, table=None):
    """fake, aligned, non-NULL "device pointers": every case below is refused before anything is launched"""
    return lib.gptq_prompt_attn_f16(qkv, ldq, rows, start, kc, vc, out, ldo, ws, ws_bytes, heads, hd, t_max, 10000.0, 0.088, table, None)


def test_prompt_attn_symbols_are_exported_and_bound():
    lib = _native.lib()
    for name in ('gptq_prompt_attn_f16', 'gptq_prompt_attn_workspace_bytes'):
        assert hasattr(lib, name), name
        assert name in _native.EXPORTS, name
    assert lib.gptq_prompt_attn_f16.argtypes is not None and len(lib.gptq_prompt_attn_f16.argtypes) == 17


def test_prompt_attn_validation_needs_no_gpu():
    lib = _native.lib()
    E_SHAPE, E_ALIGN, E_NULL, E_WORKSPACE = -2, -3, -4, -5
    assert _call(lib, hd=64) == E_SHAPE                         # head_dim != 128
    assert _call(lib, hd=256) == E_SHAPE
    assert _call(lib, rows=0) == E_SHAPE
    assert _call(lib, rows=-3) == E_SHAPE
    assert _call(lib, heads=0) == E_SHAPE
    assert _call(lib, start=-1) == E_SHAPE
    assert _call(lib, rows=8, start=T_MAX - 7) == E_SHAPE       # start + rows > t_max
    assert _call(lib, rows=T_MAX + 1) == E_SHAPE
    assert _call(lib, ldq=3 * H - 8) == E_SHAPE                 # ldq < 3 heads 128
    assert _call(lib, ldo=H - 8) == E_SHAPE                     # ldo < heads 128
    # NULL pointers, alignment and the workspace: the codes of the neighbouring decode-attention entries
    for name in ('qkv', 'kc', 'vc', 'out', 'ws'):
        assert _call(lib, **{name: None}) == E_NULL, name
    assert _call(lib, qkv=4096 + 2) == E_ALIGN
    assert _call(lib, ldq=3 * H + 4) == E_ALIGN
    need = lib.gptq_prompt_attn_workspace_bytes(8, HEADS, HD, T_MAX)
    assert need >= 8 * H * 2
    assert _call(lib, ws_bytes=need - 1) == E_WORKSPACE
    assert _call(lib, ws_bytes=0) == E_WORKSPACE


def test_prompt_attn_workspace_is_one_copy_of_q():
    lib = _native.lib()
    # at most one fp16 copy of the rotated q plus 4 KiB: no term in rows^2 or rows * t_max
    assert lib.gptq_prompt_attn_workspace_bytes(2047, 32, 128, 2048) <= 2047 * 32 * 128 * 2 + 4096
    assert lib.gptq_prompt_attn_workspace_bytes(2047, 32, 128, 1 << 20) == lib.gptq_prompt_attn_workspace_bytes(2047, 32, 128, 2048)
    assert lib.gptq_prompt_attn_workspace_bytes(16, 32, 64, 2048) == 0      # head_dim != 128
    assert lib.gptq_prompt_attn_workspace_bytes(16, 32, 256, 2048) == 0
