"""GPU parity tests: the HIP path (through the drop-in Python surface -> C ABI) against
(a) the golden fixtures recorded from the reference's own kernels, (b) the CPU oracle on seeded
inputs, incl. the full LLaMA-7B shapes, and (c) size-independent properties.
Tolerance (SURVEY 0.6 / BASELINE north_star): max|y - y_ref| / max|y_ref| < 1e-3."""
import numpy as np
import pytest
import torch

import quant
from quant import quant_linear as QL
from quant import _native
from oracle import oracle
from util import TOL, golden_names, load_golden, make_random_layer, rel_err, assert_not_worse_than_reference

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def hip_forward(x, L, bias=None, family=None):
    out = QL.matmul248(dev(x), dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), dev(L['g_idx']), int(L['bits']),
                       2**int(L['bits']) - 1, bias=None if bias is None else dev(bias), family=family)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def oracle_forward(x, L, bias=None):
    return oracle.matmul248(x, L['qweight'], L['scales'], L['qzeros'], L['g_idx'], int(L['bits']), bias=bias)


def exact_forward(x, L, bias=None):
    """float64 result (weights never rounded); + bias.  With a bias the kernels round twice -- fp16(fp16(acc) + bias), reference
    quant_linear.py:376 -- and a 1-ulp flip of the FIRST rounding against the reference-faithful oracle can survive as up to 2 ulp of
    the sum; the op-level bar (1e-3, max-normalised) is therefore held against THIS result for every call that carries a bias."""
    e = oracle.matmul248_exact(x, L['qweight'], L['scales'], L['qzeros'], L['g_idx'], int(L['bits']))
    return e if bias is None else e + np.asarray(bias, dtype=np.float64)


def check_forward(x, L, bias=None, family=None):
    y = hip_forward(x, L, bias, family)
    ref = oracle_forward(x, L, bias)
    assert y.shape == ref.shape
    assert np.isfinite(y.astype(np.float32)).all()
    bar = ref if bias is None else exact_forward(x, L, bias)
    assert rel_err(y, bar) < TOL, rel_err(y, bar)
    return y, ref


def test_native_library_loaded():
    L = _native.lib()
    assert L.gptq_query(0) == 1
    assert torch.cuda.get_device_properties(0).gcnArchName.startswith('gfx950')


@pytest.mark.parametrize('name', golden_names('pack_') + golden_names('fwd_'))
def test_forward_vs_reference_kernel_golden(name):
    f = load_golden(name)
    y = hip_forward(f['x'], f)
    assert rel_err(y, f['y']) < TOL
    ye = oracle.matmul248_exact(f['x'], f['qweight'], f['scales'], f['qzeros'], f['g_idx'], int(f['bits']))
    assert rel_err(y, ye) < TOL


def test_bias_golden():
    f = load_golden('pack_w4gall_sym_bias.npz')
    y = hip_forward(f['x'], f, bias=f['bias'])
    ref = oracle_forward(f['x'], f, bias=f['bias'])
    assert rel_err(y, ref) < TOL


@pytest.mark.parametrize('name', golden_names('mlp_'))
def test_fused_mlp_vs_reference_kernel_golden(name):
    f = load_golden(name)
    bits = int(f['gate_bits'])
    gs = int(f['gate_groupsize'])
    K = f['x'].shape[1]
    gs = K if gs == -1 else gs
    gate = tuple(dev(f['gate_' + k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    up = tuple(dev(f['up_' + k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    c = quant.fused_mlp.fused_gate_up(dev(f['x']), gate, up, bits, gs).cpu().numpy()
    assert rel_err(c, f['c']) < TOL


@pytest.mark.parametrize('name', golden_names('bwd_'))
def test_backward_vs_reference_kernel_golden(name):
    f = load_golden(name)
    bits = int(f['bits'])
    dx = QL.transpose_matmul248(dev(f['dy']), dev(f['qweight']), dev(f['scales']), dev(f['qzeros']), dev(f['g_idx']), bits,
                                2**bits - 1).cpu().numpy()
    assert rel_err(dx, f['dx']) < TOL


@pytest.mark.parametrize('name', golden_names('norm_'))
def test_rmsnorm_vs_reference_kernel_golden(name):
    f = load_golden(name)
    y = quant.triton_norm.rms_norm(dev(f['x']), dev(f['w']), float(f['eps'])).cpu().numpy()
    assert rel_err(y, f['y']) < TOL


@pytest.mark.parametrize('name', golden_names('rope_'))
def test_rope_vs_reference_kernel_golden(name):
    f = load_golden(name)
    qkv = dev(f['qkv_in'])
    quant.fused_attn.hip_rotate_half_(qkv[:, :, :2], dev(f['pos']))
    out = qkv.cpu().numpy()
    assert np.array_equal(out[:, :, 2].view(np.uint16), f['qkv_out'][:, :, 2].view(np.uint16))
    assert np.abs(out.astype(np.float32) - f['qkv_out'].astype(np.float32)).max() < 4e-3
    assert rel_err(out, f['qkv_out']) < TOL


@pytest.mark.parametrize('bits,gs', [(2, 128), (2, 32), (4, 128), (4, 64), (4, 32), (4, -1), (8, 128), (8, 32), (8, -1)])
@pytest.mark.parametrize('variant', [0, 1, 2])
@pytest.mark.parametrize('M', [1, 3])
def test_gemv_every_variant(bits, gs, variant, M):
    """the rowwave GEMV with U = 8, 4, 2 packed rows in flight per wave, forced through the ABI
    (M > 1 = one launch per row); a variant whose U does not divide the group is refused."""
    K, N = 1024, 512
    L = make_random_layer(bits, gs, K, N, seed=bits * 10 + variant)
    x = np.random.default_rng(M).standard_normal((M, K)).astype(np.float16)
    U = 8 >> variant
    rows, rpg = K * bits // 32, (K if gs == -1 else gs) * bits // 32
    lib = _native.lib()
    lib.gptq_set_gemv_variant(variant)
    try:
        if rows % U == 0 and (gs == -1 or rpg % U == 0):
            check_forward(x, L, family='gemv')
        else:
            with pytest.raises(RuntimeError):
                hip_forward(x, L, family='gemv')
    finally:
        lib.gptq_set_gemv_variant(-1)


@pytest.mark.parametrize('K,N', [(1024, 288), (1056, 256), (96, 32), (2080, 800)])
@pytest.mark.parametrize('bits,gs', [(4, 32), (4, -1), (8, 32), (2, 32)])
def test_gemv_ragged_shapes(K, N, bits, gs):
    """N not a multiple of the 256-column tile, K not a multiple of the 4*U-row chunk."""
    L = make_random_layer(bits, gs, K, N, seed=K + N + bits)
    x = np.random.default_rng(K).standard_normal((1, K)).astype(np.float16)
    check_forward(x, L, family='gemv')
    bias = np.random.default_rng(N).standard_normal(N).astype(np.float16)
    check_forward(x, L, bias=bias)


@pytest.mark.parametrize('split_k', [1, 2, 3, 8, 32, 128])
@pytest.mark.parametrize('variant', [0, 1, 2])
def test_gemv_split_k(split_k, variant):
    """K slices combined through fp32 partials summed in slice order by the last arriver; run twice: the last arriver
    must leave the arrival counts zeroed for the next launch, and the result is bit-reproducible."""
    L = make_random_layer(4, 128, 2048, 512, seed=7)
    x = np.random.default_rng(3).standard_normal((2, 2048)).astype(np.float16)
    lib = _native.lib()
    lib.gptq_set_gemv_variant(variant)
    lib.gptq_set_split_k(split_k)
    try:
        y1, _ = check_forward(x, L, family='gemv')
        y2, _ = check_forward(x, L, family='gemv')
        # the combine sums in slice order whatever the arrival order: bit-identical run to run
        assert np.array_equal(y1.view(np.uint16), y2.view(np.uint16))
    finally:
        lib.gptq_set_gemv_variant(-1)
        lib.gptq_set_split_k(-1)


@pytest.mark.parametrize('bits,gs', [(4, 128), (4, 32), (4, -1), (2, 64), (2, 128), (8, 128), (8, 32)])
@pytest.mark.parametrize('M', [5, 16, 17, 33, 64])
def test_skinny_mfma(bits, gs, M):
    L = make_random_layer(bits, gs, 1024, 256, seed=bits + M)
    x = np.random.default_rng(M).standard_normal((M, 1024)).astype(np.float16)
    check_forward(x, L, family='skinny')
    check_forward(x, L)      # built-in dispatch


@pytest.mark.parametrize('bits,gs,act', [(4, 128, False), (4, 32, False), (4, -1, False), (4, 128, True), (3, -1, False), (8, 32, False), (2, 64, True)])
def test_dequantize_is_bit_exact_with_the_reference_weight(bits, gs, act):
    """gptq_dequant_f16 == the weight the reference kernel forms on the fly (oracle.dequant, faithful)."""
    K, N = 512, 288 if bits != 3 else 320
    L = make_random_layer(bits, gs, K, N, act_order=act, seed=bits + K)
    W = QL.dequantize(dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), dev(L['g_idx']), bits).cpu().numpy()
    ref = oracle.dequant(L['qweight'], L['qzeros'], L['scales'], L['g_idx'], bits, faithful=True).astype(np.float16)
    assert np.array_equal(W.view(np.uint16), ref.view(np.uint16))


@pytest.mark.parametrize('M', [65, 100, 700])
def test_mid_m_route(M):
    """above the weight-streaming kernels, below a GPU full of 256 x 256 tiles (gptq_layer_forward: 16-row MFMA tiles up to 128
    rows, then dequantise once + dense product): same answer as the ABI's own kernels for that M."""
    L = make_random_layer(4, 128, 1024, 512, seed=M)
    x = np.random.default_rng(M).standard_normal((M, 1024)).astype(np.float16)
    bias = np.random.default_rng(1).standard_normal(512).astype(np.float16)
    y, _ = check_forward(x, L, bias=bias)
    y_abi, _ = check_forward(x, L, bias=bias, family='abi')
    assert rel_err(y, y_abi) < TOL


def test_dequantize_into_a_strided_view_and_silu_mul():
    """the two kernels of the prefill route next to the library GEMM: gptq_dequant_ld_f16 writes gate | up side by side into ONE
    [K, 2N] matrix (bit-exact halves, nothing outside them), gptq_silu_mul_f16 = fp16(silu(fp32 g) * fp32 u) on strided halves."""
    import torch
    K, N = 512, 288
    A, B = make_random_layer(4, 128, K, N, seed=1), make_random_layer(2, 64, K, N, act_order=True, seed=2)
    W = torch.full((K, 2 * N + 8), 7.0, dtype=torch.float16, device='cuda:0')
    QL.dequantize(dev(A['qweight']), dev(A['scales']), dev(A['qzeros']), dev(A['g_idx']), 4, out=W[:, :N])
    QL.dequantize(dev(B['qweight']), dev(B['scales']), dev(B['qzeros']), dev(B['g_idx']), 2, out=W[:, N:2 * N])
    Wn = W.cpu().numpy()
    for L, bits, sl in ((A, 4, slice(0, N)), (B, 2, slice(N, 2 * N))):
        ref = oracle.dequant(L['qweight'], L['qzeros'], L['scales'], L['g_idx'], bits, faithful=True).astype(np.float16)
        assert np.array_equal(np.ascontiguousarray(Wn[:, sl]).view(np.uint16), ref.view(np.uint16))
    assert (Wn[:, 2 * N:] == 7.0).all()
    with pytest.raises(RuntimeError):
        QL.dequantize(dev(A['qweight']), dev(A['scales']), dev(A['qzeros']), dev(A['g_idx']), 4, out=W[:, :N + 8])
    rng = np.random.default_rng(3)
    for M in (1, 37, 300):
        y = (rng.standard_normal((M, 2 * N)) * 3).astype(np.float16)
        dy = dev(y)
        c = QL.silu_mul(dy[:, :N], dy[:, N:]).cpu().numpy()
        g, u = y[:, :N].astype(np.float32), y[:, N:].astype(np.float32)
        ref = (g / (1.0 + np.exp(-g)) * u).astype(np.float16)
        assert rel_err(c, ref) < 1e-3 and np.abs(c.astype(np.float32) - ref.astype(np.float32)).max() <= 2 * np.spacing(np.abs(ref).max().astype(np.float16))
    assert _native.lib().gptq_silu_mul_f16(dy.data_ptr(), 2 * N, dy.data_ptr(), 2 * N, dy.data_ptr(), 2 * N, 4, N + 4, None) == -2      # N % 8


@pytest.mark.parametrize('route', ['auto', 'library', 'own'])
@pytest.mark.parametrize('bits,gs,act,M,K,N', [(4, 128, False, 4096, 4096, 4096), (4, 128, True, 2100, 1024, 4096), (3, -1, False, 700, 512, 320),
                                               (2, 64, False, 300, 1024, 512), (8, 128, False, 8192, 512, 4096)])
def test_prefill_routes_vs_oracle(route, bits, gs, act, M, K, N, monkeypatch):
    """the built-in dispatch above the streaming kernels under every setting of GPTQ_PREFILL: 'auto' (default) and 'own' = the tile GEMM of
    csrc/gemm8.hip wherever it can run (K % 128 == 0; round 3's 'auto' still used hipBLASLt below one full round of tiles); 'library' =
    hipBLASLt for every dense product (the reported ceiling); against the CPU oracle on sampled rows."""
    monkeypatch.setattr(QL, 'PREFILL_ROUTE', route)
    lib = _native.lib()
    QL._apply_prefill_route()
    if route != 'library' and K % 128 == 0:
        assert lib.gptq_prefill_route_for(M, K, N, 1, 0) == 1         # round 4: 'auto' never hands a K % 128 == 0 product to the library
    if route == 'library':
        assert lib.gptq_prefill_route_for(M, K, N, 1, 0) == 0
    L = make_random_layer(bits, gs, K, N, act_order=act, seed=M + K + bits)
    rng = np.random.default_rng(17)
    x = rng.standard_normal((M, K)).astype(np.float16)
    bias = rng.standard_normal(N).astype(np.float16) if bits == 8 else None
    y = hip_forward(x, L, bias=bias)
    rows = np.unique(np.concatenate([np.arange(0, M, max(M // 24, 1)), [M - 1, 63, 64, 255, 256]]))
    ref = oracle_forward(x[rows], L, bias=bias)
    assert rel_err(y[rows], ref) < TOL, rel_err(y[rows], ref)
    monkeypatch.setattr(QL, 'PREFILL_ROUTE', 'auto')
    QL._apply_prefill_route()


@pytest.mark.parametrize('route', ['library', 'own'])
@pytest.mark.parametrize('bits,gs,act,M', [(4, 128, False, 1000), (4, 128, True, 300), (2, 64, False, 200), (3, -1, False, 129), (8, 32, False, 333),
                                           (4, 128, False, 8192 + 77)])
def test_fused_mlp_prefill_routes(bits, gs, act, M, route, monkeypatch):
    """fused_gate_up above the streaming kernels (gptq_prefill_fused_mlp_f16), both engines: 'own' = gate and up stacked as ONE
    [2N, K] operand of the tile GEMM, SiLU on the fp32 accumulators in its epilogue; 'library' = gate | up in one [K, 2N] matrix,
    one hipBLASLt GEMM with FP32 output per chunk of 8192 rows (last case: a ragged second chunk), silu * mul on the fp32 products
    as its own pass.  Every width, act-order included, against the fused oracle at the op-level bar (1e-3: no rounding of gate / up
    before the activation on either route -- reference fused_mlp.py:160-165)."""
    monkeypatch.setattr(QL, 'PREFILL_ROUTE', route)
    K, N = 512, 320 if bits == 3 else 288
    A = make_random_layer(bits, gs, K, N, act_order=act, seed=M)
    B = make_random_layer(bits, gs, K, N, act_order=act, seed=M + 1)
    if act:
        B['g_idx'] = A['g_idx']         # not required on this route, but what a real MLP has; the oracle takes either
    x = (np.random.default_rng(M).standard_normal((M, K)) * 0.5).astype(np.float16)
    gate = tuple(dev(A[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    up = tuple(dev(B[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    c = quant.fused_mlp.fused_gate_up(dev(x), gate, up, bits, gs if gs != -1 else K).cpu().numpy()
    rows = np.arange(M) if M <= 1000 else np.unique(np.concatenate([np.arange(0, M, 257), [8191, 8192, M - 1]]))
    ref = oracle.fused_mlp(x[rows], (A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), bits)
    assert rel_err(c[rows], ref) < TOL, rel_err(c[rows], ref)
    monkeypatch.setattr(QL, 'PREFILL_ROUTE', 'auto')
    QL._apply_prefill_route()


@pytest.mark.parametrize('bits,gs,act,M,K,N', [(4, 128, False, 3072, 1024, 4096), (4, 128, True, 2100, 1024, 768), (8, 128, False, 577, 512, 4096),
                                               (4, 128, False, 191, 512, 320), (4, 128, False, 193, 512, 320), (3, -1, False, 700, 512, 320)])
def test_gemm8_tile_rows_same_bits(bits, gs, act, M, K, N):
    """Round 5: the tile GEMM's 192-row workgroup tile (csrc/gemm8.hip XH = 48) against the 256-row one -- every accumulator
    sums the same products in the same K order, so the outputs are the SAME BITS (plain with bias, and the gate/up pair with SiLU on the fp32
    sums), and the 192-row result meets the oracle on sampled rows.  Row counts around the tile edges (191, 193: one / two tiles; 577: a ragged
    fourth tile; 3072 = 16 x 192 = 12 x 256); the per-launch choice (gptq_set_gemm8_tile(0)) is one of the two."""
    lib = _native.lib()
    L = make_random_layer(bits, gs, K, N, act_order=act, seed=M + bits)
    U = make_random_layer(bits, gs, K, N, act_order=act, seed=M + bits + 1)
    if act:
        U['g_idx'] = L['g_idx']
    rng = np.random.default_rng(M)
    x = (rng.standard_normal((M, K)) * 0.5).astype(np.float16)
    bias = rng.standard_normal(N).astype(np.float16) if bits == 8 else None
    gate = tuple(dev(L[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    up = tuple(dev(U[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    prev_rows = lib.gptq_set_stripe_gemm_max_rows(0)          # the dense route for every row count above 128
    prev_tile = lib.gptq_set_gemm8_tile(0)
    try:
        assert lib.gptq_set_gemm8_tile(100) == -6 and lib.gptq_set_gemm8_tile(0) == 0
        got = {}
        for tile in (192, 256, 0):
            lib.gptq_set_gemm8_tile(tile)
            got[tile] = (hip_forward(x, L, bias=bias), quant.fused_mlp.fused_gate_up(dev(x), gate, up, bits, gs if gs != -1 else K).cpu().numpy())
        for j in (0, 1):
            assert np.array_equal(got[192][j], got[256][j]) and np.array_equal(got[0][j], got[256][j])
        rows = np.unique(np.concatenate([np.arange(0, M, max(M // 24, 1)), [M - 1, 47, 48, 95, 96, 190]]))
        assert rel_err(got[192][0][rows], oracle_forward(x[rows], L, bias=bias)) < TOL
        ref = oracle.fused_mlp(x[rows], (L['qweight'], L['scales'], L['qzeros'], L['g_idx']), (U['qweight'], U['scales'], U['qzeros'], U['g_idx']), bits)
        assert rel_err(got[192][1][rows], ref) < TOL
    finally:
        lib.gptq_set_gemm8_tile(prev_tile)
        lib.gptq_set_stripe_gemm_max_rows(prev_rows)


def test_prefill_falls_back_to_the_own_kernels_without_the_library(monkeypatch):
    """GPTQ_E_LIBRARY (hipBLASLt not loadable) from the prefill entries: the library-free kernels of the C ABI answer -- forward,
    fused MLP (inside gptq_layer_forward) and backward (one Python warning), same results."""
    lib = _native.lib()
    monkeypatch.setattr(QL, '_library_warned', False)
    K, N, M = 480, 288, 300          # K % 128 != 0: the one kind of shape the default route still hands to the library (round 4)
    L = make_random_layer(4, 32, K, N, seed=9)
    U = make_random_layer(4, 32, K, N, seed=10)
    rng = np.random.default_rng(9)
    x = rng.standard_normal((M, K)).astype(np.float16)
    assert lib.gptq_prefill_route_for(M, K, N, 1, 0) == 0
    prev = lib.gptq_set_library_enabled(0)          # test hook: every hipBLASLt call answers GPTQ_E_LIBRARY
    try:
        check_forward(x, L)                         # gptq_layer_forward falls through to the C ABI's own kernels (one line on stderr)
        gate = tuple(dev(L[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
        up = tuple(dev(U[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
        c = quant.fused_mlp.fused_gate_up(dev(x), gate, up, 4, 32).cpu().numpy()
        ref = oracle.fused_mlp(x, (L['qweight'], L['scales'], L['qzeros'], L['g_idx']), (U['qweight'], U['scales'], U['qzeros'], U['g_idx']), 4)
        assert rel_err(c, ref) < TOL                # (library-free route: the round-1 tile GEMM in PAIR mode, SiLU on the fp32 sums as well)
        dy = rng.standard_normal((M, N)).astype(np.float16)
        with pytest.warns(UserWarning, match='falling back'):
            dx = QL.transpose_matmul248(dev(dy), dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), dev(L['g_idx']), 4, 15).cpu().numpy()
        assert rel_err(dx, oracle.transpose_matmul248(dy, L['qweight'], L['scales'], L['qzeros'], L['g_idx'], 4)) < TOL
    finally:
        lib.gptq_set_library_enabled(prev)


def test_prefill_c_abi_entries_strided_and_errors():
    """gptq_prefill_matmul_f16 directly: strided x and y (leading dimensions), bias in the library epilogue, plan cache hit on the
    second call, workspace too small -> GPTQ_E_WORKSPACE, empty batch -> ok."""
    import torch
    lib = _native.lib()
    K, N, M = 512, 288, 300
    L = make_random_layer(4, 128, K, N, seed=5)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((M, K)).astype(np.float16)
    bias = rng.standard_normal(N).astype(np.float16)
    xb = torch.zeros((M, K + 64), dtype=torch.float16, device='cuda:0')
    xb[:, :K] = dev(x)
    yb = torch.full((M, N + 32), 3.0, dtype=torch.float16, device='cuda:0')
    qw, sc, qz, db = dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), dev(bias)
    need = lib.gptq_prefill_workspace_bytes(M, K, N, 1)
    assert need >= K * N * 2 and lib.gptq_prefill_workspace_bytes(M, K, N, 3) == 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda:0')
    s = torch.cuda.current_stream().cuda_stream
    ref = oracle_forward(x, L, bias=bias)
    for _ in range(2):
        rc = lib.gptq_prefill_matmul_f16(xb.data_ptr(), K + 64, qw.data_ptr(), sc.data_ptr(), qz.data_ptr(), None, db.data_ptr(), yb.data_ptr(), N + 32,
                                         M, K, N, 4, 128, ws.data_ptr(), need, s)
        assert rc == 0, _native.lib().gptq_strerror(rc)
        torch.cuda.synchronize()
        assert rel_err(yb[:, :N].cpu().numpy(), ref) < TOL
        assert bool((yb[:, N:] == 3.0).all())
    assert lib.gptq_prefill_matmul_f16(xb.data_ptr(), K + 64, qw.data_ptr(), sc.data_ptr(), qz.data_ptr(), None, None, yb.data_ptr(), N + 32,
                                       M, K, N, 4, 128, ws.data_ptr(), need - 1, s) == -5
    assert lib.gptq_prefill_matmul_f16(xb.data_ptr(), K + 64, qw.data_ptr(), sc.data_ptr(), qz.data_ptr(), None, None, yb.data_ptr(), N + 32,
                                       0, K, N, 4, 128, None, 0, s) == 0


@pytest.mark.parametrize('split_k', [2, 4])
def test_skinny_split_k(split_k):
    L = make_random_layer(4, 128, 2048, 256, seed=11)
    x = np.random.default_rng(5).standard_normal((24, 2048)).astype(np.float16)
    lib = _native.lib()
    lib.gptq_set_split_k(split_k)
    try:
        check_forward(x, L, family='skinny')
        check_forward(x, L, family='skinny')
    finally:
        lib.gptq_set_split_k(-1)


@pytest.mark.parametrize('M', [65, 130, 257])
def test_large_m(M):
    L = make_random_layer(4, 128, 512, 256, seed=M)
    x = np.random.default_rng(M).standard_normal((M, 512)).astype(np.float16)
    check_forward(x, L, family='abi')


@pytest.mark.parametrize('kernel', [3, 2])
@pytest.mark.parametrize('bits,gs', [(4, 128), (4, 32), (4, -1), (4, 64), (8, 128), (8, 64)])
@pytest.mark.parametrize('M,K,N', [(300, 256, 288), (513, 1024, 512), (1024, 4096, 256), (65, 192, 32)])
def test_prefill_mfma_gemm(bits, gs, M, K, N, kernel):
    """the 256x256x64 MFMA tile kernel (M > 64): ragged M / N, several K slabs and group changes,
    bias; it dequantises with the reference's fp16 sequence so it sits very close to the
    faithful oracle."""
    if gs != -1 and K % gs:
        pytest.skip('K not a multiple of the group')
    L = make_random_layer(bits, gs, K, N, seed=M + K + N + bits)
    rng = np.random.default_rng(M)
    x = rng.standard_normal((M, K)).astype(np.float16)
    bias = rng.standard_normal(N).astype(np.float16)
    lib = _native.lib()
    prev = lib.gptq_set_gemm_kernel(kernel)
    try:
        check_forward(x, L, bias=bias, family='abi')
    finally:
        lib.gptq_set_gemm_kernel(prev)


def test_prefill_gemm_rows_independent():
    """size-independent property at a prefill-like size: every output row equals the M = 1 path's
    answer for that row (GEMM tile kernel vs rowwave GEMV on the same packed weights)."""
    K, N, M = 4096, 4096, 2048
    L = make_random_layer(4, 128, K, N, seed=99)
    x = np.random.default_rng(7).standard_normal((M, K)).astype(np.float16)
    y = hip_forward(x, L, family='abi')
    for m in (0, 255, 256, 1000, 2047):
        ym = hip_forward(x[m:m + 1], L)
        assert rel_err(y[m:m + 1], ym) < TOL


@pytest.mark.parametrize('M,K,N,bits,gs', [(4096, 4096, 4096, 4, 128), (8192, 1024, 4096, 4, 128), (4096, 4096, 1024, 8, 128)])
def test_prefill_gemm_vs_oracle_at_prefill_sizes(M, K, N, bits, gs):
    """the MFMA tile GEMM at M >= 4096 and N = 4096 directly against the CPU oracle (reference arithmetic,
    quant_linear.py:128-130) on 48 sampled rows spread over every 256-row tile band -- not only against our own M = 1 kernel."""
    L = make_random_layer(bits, gs, K, N, seed=M + K)
    rng = np.random.default_rng(11)
    x = rng.standard_normal((M, K)).astype(np.float16)
    y = hip_forward(x, L, family='abi')
    rows = np.unique(np.concatenate([np.arange(0, M, M // 32), rng.integers(0, M, 16), [M - 1, 255, 256]]))
    ref = oracle_forward(x[rows], L)
    assert rel_err(y[rows], ref) < TOL, rel_err(y[rows], ref)


@pytest.mark.parametrize('bits', [2, 3, 4, 8])
@pytest.mark.parametrize('M', [1, 3, 9])
def test_act_order_and_3bit(bits, M):
    """non-trivial g_idx (act-order) for every width; 3-bit is the layout EXTENSION (no reference)."""
    L = make_random_layer(bits, 128, 512, 256 if bits != 3 else 96 * 2 + 64, act_order=True, seed=bits)
    x = np.random.default_rng(M + 20).standard_normal((M, 512)).astype(np.float16)
    check_forward(x, L)


@pytest.mark.parametrize('bits', [4, 8, 3])
@pytest.mark.parametrize('world,M', [(8, 1), (4, 3), (2, 1)])
def test_act_order_row_shards_fp32_partials_one_rounding(bits, world, M):
    """Round 6: a tensor-parallel rank's ROW shard of an act-order layer -- rows k0 .. k1 of the checkpoint, whose g_idx points
    into all groups of the layer -- leaves as an fp32 partial (gptq_matmul248_partial_f32), like every other shard: the ranks' partials are summed
    in fp32 and rounded ONCE (north_star).  Simulated for `world` ranks on one GPU: (a) every partial is the float64 sum of its shard (weights
    dequantised as the reference does) to fp32 accuracy; (b) fp16(sum of the partials in rank order) is the correctly rounded result up to that
    fp32 noise -- equal to the rounded float64 sum or its neighbour, and within half an ulp + the noise; (c) the round-5 way (an fp16 output per
    rank, widened and summed) is measurably worse on the same data."""
    K, N, gs = 2048, 512, 128
    L = make_random_layer(bits, gs, K, N, act_order=True, seed=60 + bits)
    rng = np.random.default_rng(world + M)
    x = rng.standard_normal((M, K)).astype(np.float16)
    lib = _native.lib()
    s = _native.stream_ptr(torch.device(DEV))
    ws = _native.workspace(torch.device(DEV))
    W = oracle.np_dequant(L['qweight'], L['qzeros'], L['scales'], L['g_idx'], bits, faithful=True).astype(np.float64)      # [K, N], the reference's fp16 weight
    sc, qz = dev(L['scales']), dev(L['qzeros'])
    G = L['scales'].shape[0]
    Ks = K // world
    parts, parts16, exact, noise = [], [], np.zeros((M, N)), np.zeros((M, N))
    for r in range(world):
        k0, k1 = r * Ks, (r + 1) * Ks
        qw = dev(L['qweight'][k0 * bits // 32:k1 * bits // 32])
        gi = dev(L['g_idx'][k0:k1])
        xs = dev(x[:, k0:k1])
        y32 = torch.full((M, N), float('nan'), dtype=torch.float32, device=DEV)
        rc = lib.gptq_matmul248_partial_f32(xs.data_ptr(), xs.stride(0), qw.data_ptr(), sc.data_ptr(), qz.data_ptr(), gi.data_ptr(), y32.data_ptr(), N, M, Ks, N,
                                            bits, G, s)
        assert rc == 0, rc
        e = x[:, k0:k1].astype(np.float64) @ W[k0:k1]
        mag = np.abs(x[:, k0:k1].astype(np.float64)) @ np.abs(W[k0:k1])
        got = y32.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all()
        assert (np.abs(got - e) <= mag * 2.0**-20).all(), np.abs(got - e).max()            # (a)
        parts.append(y32)
        exact += e
        noise += mag * 2.0**-20
        # round 5's launch: the generic kernel with an fp16 output (told a group size that makes its table hold every group of the layer)
        y16 = torch.empty((M, N), dtype=torch.float16, device=DEV)
        rc = lib.gptq_matmul248_f16(xs.data_ptr(), xs.stride(0), qw.data_ptr(), sc.data_ptr(), qz.data_ptr(), gi.data_ptr(), None, y16.data_ptr(), N, M, Ks, N, bits,
                                    max(1, Ks // G), ws.data_ptr(), ws.numel(), s)
        assert rc == 0, rc
        parts16.append(y16.float())
    total = parts[0].clone()
    total16 = parts16[0].clone()
    for r in range(1, world):
        total += parts[r]                      # rank order, fp32: what the one-shot exchange does (csrc/p2p.hip)
        total16 += parts16[r]
    y = total.half().cpu().numpy()
    y_old = total16.half().cpu().numpy()
    best = exact.astype(np.float16)             # the correctly rounded result
    ulp = np.spacing(np.abs(best).astype(np.float16)).astype(np.float64)
    err, err_old = np.abs(y.astype(np.float64) - exact), np.abs(y_old.astype(np.float64) - exact)
    noise += np.abs(exact) * 2.0**-21                    # (+ the fp32 additions of the exchange)
    assert (err <= 0.5 * ulp + noise).all()                                                    # (b): one rounding
    assert (y == best).mean() > 0.99
    if world > 2:
        assert err_old.max() > err.max() and (err_old > 0.5 * ulp + noise).any()      # (c): one rounding per rank shows
    # error paths: a missing g_idx / table, a K that is no multiple of 32
    assert lib.gptq_matmul248_partial_f32(dev(x).data_ptr(), K, qw.data_ptr(), sc.data_ptr(), qz.data_ptr(), None, total.data_ptr(), N, M, Ks, N, bits, G, s) < 0
    assert lib.gptq_matmul248_partial_f32(dev(x).data_ptr(), K, qw.data_ptr(), sc.data_ptr(), qz.data_ptr(), gi.data_ptr(), total.data_ptr(), N, M, Ks - 8, N, bits, G, s) < 0


@pytest.mark.parametrize('bits,gs', [(4, 128), (4, 32), (8, 64), (2, 128)])
@pytest.mark.parametrize('M', [1, 2, 70])
def test_act_order_sorted_fast_path(bits, gs, M):
    """act-order layers run through their group-sorted copy (one-off repack + x[perm]); the result
    must agree with the oracle AND with the generic g_idx-table kernel on the checkpoint layout."""
    K, N = 1024, 512
    L = make_random_layer(bits, gs, K, N, act_order=True, seed=bits + gs + M)
    x = np.random.default_rng(M + 5).standard_normal((M, K)).astype(np.float16)
    qw, gi = dev(L['qweight']), dev(L['g_idx'])
    srt = QL.act_order_sorted(qw, gi, K, gs, bits)
    assert srt is not None and srt[0].shape == qw.shape and srt[1].shape == (K, )
    # the sorted copy really is a trivial-g_idx layer of x[perm]
    perm = srt[1].cpu().numpy()
    assert np.array_equal(np.sort(perm), np.arange(K)) and np.array_equal(L['g_idx'][perm], np.arange(K) // gs)
    ref = oracle.matmul248(x[:, perm], srt[0].cpu().numpy(), L['scales'], L['qzeros'], (np.arange(K) // gs).astype(np.int32), bits)
    full = oracle_forward(x, L)
    assert rel_err(ref, full) < TOL
    fam = 'abi' if M > QL.STREAM_MAX_M else None      # keep the C-ABI kernels under test for every M
    y, _ = check_forward(x, L, family=fam)
    QL.ACT_ORDER_SORT = False
    try:
        y_generic = hip_forward(x, L, family=fam)
    finally:
        QL.ACT_ORDER_SORT = True
    assert rel_err(y, y_generic) < TOL


@pytest.mark.parametrize('bits,gs,K,N', [(4, 128, 4096, 512), (4, 32, 1024, 160), (8, 64, 1024, 96), (2, 128, 1024, 64), (4, 128, 11008, 256),
                                         (3, 128, 4096, 512), (3, 32, 1152, 160)])
@pytest.mark.parametrize('M', [1, 2, 4, 7, 16, 50, 100])
def test_act_order_batches_through_stripe_kernels(bits, gs, K, N, M):
    """batches of an act-order layer: one gather x[:, perm], then the stripe16 decode / MFMA-tile kernels on the image of the
    group-sorted rows -- against the oracle on the ORIGINAL checkpoint buffers, and run twice"""
    L = make_random_layer(bits, gs, K, N, act_order=True, seed=bits + gs + M)
    x = np.random.default_rng(M + 9).standard_normal((M, K)).astype(np.float16)
    b = np.random.default_rng(4).standard_normal(N).astype(np.float16)
    qw = dev(L['qweight'])
    y = QL.matmul248(dev(x), qw, dev(L['scales']), dev(L['qzeros']), dev(L['g_idx']), bits, 2**bits - 1, bias=dev(b)).cpu().numpy()
    pl = quant.layer._LAYERS.get(qw)
    assert pl is not None and pl[1].kind == 1 and pl[1].stripe is not None and pl[1].perm16 is not None      # group-sorted image + permutation served the call
    assert rel_err(y, exact_forward(x, L, b)) < TOL
    y2 = QL.matmul248(dev(x), qw, dev(L['scales']), dev(L['qzeros']), dev(L['g_idx']), bits, 2**bits - 1, bias=dev(b)).cpu().numpy()
    assert np.array_equal(y.view(np.uint16), y2.view(np.uint16))


def test_act_order_irregular_groups_stay_generic():
    """a g_idx whose groups do not all have `groupsize` members cannot be sorted into the trivial
    layout: the generic kernel serves it."""
    K, N = 512, 256
    L = make_random_layer(4, 128, K, N, act_order=True, seed=3)
    L['g_idx'] = L['g_idx'].copy()
    L['g_idx'][:5] = 0
    assert QL.act_order_sorted(dev(L['qweight']), dev(L['g_idx']), K, 128, 4) is None
    x = np.random.default_rng(1).standard_normal((1, K)).astype(np.float16)
    check_forward(x, L)


@pytest.mark.parametrize('gs', [-1, 32, 64, 128])
@pytest.mark.parametrize('K,N,M', [(4096, 512, 1), (1056, 288, 3), (96, 32, 1), (11008, 256, 1)])
def test_3bit_rowwave(gs, K, N, M):
    """the 3-bit rowwave GEMV (EXTENSION, no reference: checked against the oracle's own 3-bit
    restatement and the float64 exact product); incl. one group over all of K and ragged shapes."""
    if gs != -1 and K % gs:
        pytest.skip('K not a multiple of the group')
    L = make_random_layer(3, gs, K, N, seed=K + N + gs)
    rng = np.random.default_rng(K)
    x = rng.standard_normal((M, K)).astype(np.float16)
    bias = rng.standard_normal(N).astype(np.float16)
    y, ref = check_forward(x, L, bias=bias)
    ye = oracle.matmul248_exact(x, L['qweight'], L['scales'], L['qzeros'], L['g_idx'], 3) + bias.astype(np.float64)
    assert rel_err(y, ye) < TOL


@pytest.mark.parametrize('gs', [-1, 128])
def test_3bit_no_group(gs):
    L = make_random_layer(3, gs, 1024, 256, seed=33)
    x = np.random.default_rng(2).standard_normal((1, 1024)).astype(np.float16)
    check_forward(x, L)


def test_odd_groupsize_goes_generic():
    L = make_random_layer(4, 48, 96 * 4, 128, seed=5)       # groupsize not a multiple of 32
    x = np.random.default_rng(2).standard_normal((2, 96 * 4)).astype(np.float16)
    check_forward(x, L)


def test_very_wide_layer_runs_without_k_split():
    """N > 32768: the split-K words would not fit their workspace region; the GEMV must stay correct."""
    K, N = 256, 32768 + 256
    L = make_random_layer(4, 128, K, N, seed=5)
    x = np.random.default_rng(2).standard_normal((1, K)).astype(np.float16)
    check_forward(x, L)
    L2 = make_random_layer(4, 128, 1024, 512, seed=6)        # and the next split-K launch still finds zeros
    x2 = np.random.default_rng(3).standard_normal((1, 1024)).astype(np.float16)
    check_forward(np.repeat(x2, 40, 0), L2, family='skinny')
    check_forward(x2, L2)


def test_zero_rows_and_empty():
    L = make_random_layer(4, 128, 256, 128, seed=1)
    y = QL.matmul248(torch.empty(0, 256, dtype=torch.float16, device=DEV), dev(L['qweight']), dev(L['scales']),
                     dev(L['qzeros']), dev(L['g_idx']), 4, 15)
    assert y.shape == (0, 128)
    x = np.zeros((3, 256), dtype=np.float16)
    assert np.all(hip_forward(x, L) == 0)


def test_strided_rows_and_fp32_input():
    L = make_random_layer(4, 128, 256, 128, seed=2)
    rng = np.random.default_rng(0)
    big = rng.standard_normal((4, 512)).astype(np.float16)
    xs = dev(big)[:, :256]                      # row stride 512, last dim contiguous
    y = QL.matmul248(xs, dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), dev(L['g_idx']), 4, 15).cpu().numpy()
    assert rel_err(y, oracle_forward(big[:, :256], L)) < TOL
    y32 = QL.matmul248(xs.float(), dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), dev(L['g_idx']), 4, 15)
    assert y32.dtype == torch.float16


SHAPES_7B = [(4096, 4096), (4096, 11008), (11008, 4096), (4096, 12288)]


@pytest.mark.parametrize('K,N', SHAPES_7B)
def test_llama7b_shapes_vs_oracle(K, N):
    """BASELINE config 2 at full size, M = 1, against the CPU oracle (seconds on the host)."""
    L = make_random_layer(4, 128, K, N, seed=K + N)
    x = np.random.default_rng(1).standard_normal((1, K)).astype(np.float16)
    y, ref = check_forward(x, L)
    ye = oracle.matmul248_exact(x, L['qweight'], L['scales'], L['qzeros'], L['g_idx'], 4)
    assert rel_err(y, ye) < TOL
    # the pre-rounding error budget: HIP is closer to real arithmetic than the fp16-weight reference
    assert rel_err(y, ye) <= rel_err(ref, ye) + 5e-4


# the other LLaMA sizes (13B / 30B / 65B: BASELINE config 5 shapes), decode batch 1 and 3
@pytest.mark.parametrize('M', [1, 3])
@pytest.mark.parametrize('K,N', [(5120, 13824), (13824, 5120), (6656, 17920), (17920, 6656), (8192, 8192), (8192, 22016), (22016, 8192)])
def test_larger_llama_shapes_vs_oracle(K, N, M):
    L = make_random_layer(4, 128, K, N, seed=K + N)
    x = (np.random.default_rng(M).standard_normal((M, K)) * 0.5).astype(np.float16)
    check_forward(x, L)


@pytest.mark.parametrize('split_k', [1, 4, 16])
def test_fused_mlp_split_k(split_k):
    K, N = 1024, 512
    A = make_random_layer(4, 128, K, N, seed=21)
    B = make_random_layer(4, 128, K, N, seed=22)
    x = np.random.default_rng(1).standard_normal((2, K)).astype(np.float16)
    gate = tuple(dev(A[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    up = tuple(dev(B[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    lib = _native.lib()
    lib.gptq_set_split_k(split_k)
    try:
        c = quant.fused_mlp.fused_gate_up(dev(x), gate, up, 4, 128, family='abi').cpu().numpy()
        c2 = quant.fused_mlp.fused_gate_up(dev(x), gate, up, 4, 128, family='abi').cpu().numpy()
    finally:
        lib.gptq_set_split_k(-1)
    ref = oracle.fused_mlp(x, (A['qweight'], A['scales'], A['qzeros'], A['g_idx']),
                           (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), 4)
    assert rel_err(c, ref) < TOL
    assert_not_worse_than_reference(c, ref, oracle.fused_mlp_exact(x, (A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), 4))
    assert np.array_equal(c.view(np.uint16), c2.view(np.uint16))


def test_fused_mlp_prefill_goes_through_the_gemm():
    """M > 64: gate and up through the MFMA tile GEMM + fp32 SiLU*mul, against the fused oracle."""
    K, N, M = 512, 256, 200
    A = make_random_layer(4, 128, K, N, seed=31)
    B = make_random_layer(4, 128, K, N, seed=32)
    x = np.random.default_rng(4).standard_normal((M, K)).astype(np.float16)
    gate = tuple(dev(A[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    up = tuple(dev(B[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    c = quant.fused_mlp.fused_gate_up(dev(x), gate, up, 4, 128).cpu().numpy()
    ref = oracle.fused_mlp(x, (A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), 4)
    assert rel_err(c, ref) < TOL
    assert_not_worse_than_reference(c, ref, oracle.fused_mlp_exact(x, (A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), 4))


def test_llama7b_fused_mlp_full_size():
    K, N = 4096, 11008
    A = make_random_layer(4, 128, K, N, seed=1)
    B = make_random_layer(4, 128, K, N, seed=2)
    x = np.random.default_rng(1).standard_normal((1, K)).astype(np.float16)
    gate = tuple(dev(A[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    up = tuple(dev(B[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    c = quant.fused_mlp.fused_gate_up(dev(x), gate, up, 4, 128).cpu().numpy()
    ref = oracle.fused_mlp(x, (A['qweight'], A['scales'], A['qzeros'], A['g_idx']),
                           (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), 4)
    assert rel_err(c, ref) < TOL
    assert_not_worse_than_reference(c, ref, oracle.fused_mlp_exact(x, (A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), 4))


def test_linearity_property_full_size():
    """f(a*x1 + x2) == a*f(x1) + f(x2) up to fp16 rounding -- size independent."""
    K, N = 4096, 4096
    L = make_random_layer(4, 128, K, N, seed=9)
    rng = np.random.default_rng(4)
    x1 = rng.standard_normal((1, K)).astype(np.float16)
    x2 = rng.standard_normal((1, K)).astype(np.float16)
    xs = (2.0 * x1.astype(np.float32) + x2.astype(np.float32)).astype(np.float16)
    y1, y2, ys = hip_forward(x1, L), hip_forward(x2, L), hip_forward(xs, L)
    lin = 2.0 * y1.astype(np.float64) + y2.astype(np.float64)
    assert np.abs(ys - lin).max() / np.abs(lin).max() < 3e-3


@pytest.mark.parametrize('K,N,world,M', [(8192, 512, 8, 1), (22016, 256, 8, 1), (1024, 512, 8, 2), (4096, 11008, 4, 1)])
def test_row_shards_sum_to_full(K, N, world, M):
    """BASELINE config 5 emulated on one GPU: the fp32 partials of the K-shards (stripe16 kernel, unrounded sums at M == 1;
    uneven group counts for K = 22016: 22,22,22,22,21,21,21,21) sum to the full product, rounded to fp16 ONCE: 1e-3 vs the
    oracle like the unsharded layer."""
    from quant import tensor_parallel as tp
    L = make_random_layer(4, 128, K, N, seed=3)
    layer = quant.QuantLinear(4, 128, K, N, False)
    layer.qweight, layer.qzeros, layer.scales, layer.g_idx = (dev(L['qweight']), dev(L['qzeros']), dev(L['scales']),
                                                               dev(L['g_idx']))
    xh = np.random.default_rng(0).standard_normal((M, K)).astype(np.float16)
    x = dev(xh)
    acc = torch.zeros((M, N), dtype=torch.float32, device=DEV)
    for r in range(world):
        shard, (k0, k1) = tp.shard_rows(layer, r, world)
        shard.bias = None
        part = tp._default_partial(x[:, k0:k1].contiguous(), shard)
        assert part.dtype == torch.float32
        acc += part
    ref = oracle_forward(xh, L)
    assert rel_err(acc.half().cpu().numpy(), ref) < TOL


def test_stripe_partial_f32_gate_up_pair():
    """nsets = 2: the gate and the up sums of a K-shard leave separately ([2][N] fp32, no SiLU)"""
    K, N = 1024, 288
    A, B = make_random_layer(4, 128, K, N, seed=61), make_random_layer(4, 128, K, N, seed=62)
    st, _ = _stripe_image([A, B], 128)
    x = (np.random.default_rng(9).standard_normal((1, K))).astype(np.float16)
    part = torch.empty((2, N), dtype=torch.float32, device=DEV)
    rc = _native.lib().gptq_stripe_matvec_partial_f32(dev(x).data_ptr(), st.data_ptr(), st.numel(), part.data_ptr(), K, N, 4, 128, 2, None,
                                                      _native.stream_ptr(torch.device(DEV)))
    _native.check(rc, 'gptq_stripe_matvec_partial_f32')
    torch.cuda.synchronize()
    for i, L in enumerate((A, B)):
        ref = oracle.matmul248_exact(x, L['qweight'], L['scales'], L['qzeros'], L['g_idx'], 4)
        assert rel_err(part[i:i + 1].cpu().numpy(), ref) < 2e-4         # fp32 result vs the float64 oracle: no fp16 rounding left


def test_gpu_pack_bit_exact():
    """gptq_pack_f32 == oracle.pack (== reference pack, see test_oracle_golden) bit for bit."""
    for name in golden_names('pack_'):
        f = load_golden(name)
        bits, gs = int(f['bits']), int(f['groupsize'])
        N, K = f['weight_q'].shape
        lin = torch.nn.Linear(K, N, bias=False)
        lin.weight.data = torch.from_numpy(f['weight_q'])
        lin = lin.to(DEV)
        ql = quant.QuantLinear(bits, gs, K, N, False)
        ql.pack(lin, torch.from_numpy(f['scales_in']), torch.from_numpy(f['zeros_in']), torch.from_numpy(f['g_idx']))
        assert np.array_equal(ql.qweight.cpu().numpy(), f['qweight']), name
        assert np.array_equal(ql.qzeros.cpu().numpy(), f['qzeros']), name
        assert np.array_equal(ql.scales.cpu().numpy().view(np.uint16), f['scales'].view(np.uint16)), name


def test_hipgraph_capture_and_replay():
    L = make_random_layer(4, 128, 1024, 512, seed=4)
    args = (dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), dev(L['g_idx']), 4, 15)
    x = dev(np.random.default_rng(0).standard_normal((1, 1024)).astype(np.float16))
    y_eager = QL.matmul248(x, *args).clone()      # also warms the g_idx cache / workspace
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        QL.matmul248(x, *args)
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        y_cap = QL.matmul248(x, *args)
    x.copy_(x * 2)
    g.replay()
    torch.cuda.synchronize()
    assert rel_err(y_cap.cpu().numpy(), (2 * y_eager.float()).cpu().numpy()) < TOL


def test_error_behaviour():
    with pytest.raises(NotImplementedError):
        quant.QuantLinear(5, 128, 256, 128, False)
    L = make_random_layer(4, 128, 256, 128, seed=1)
    with pytest.raises(RuntimeError):
        QL.matmul248(torch.zeros(1, 256, dtype=torch.float16), dev(L['qweight']), dev(L['scales']), dev(L['qzeros']),
                     dev(L['g_idx']), 4, 15)
    with pytest.raises(RuntimeError):
        quant.triton_norm.rms_norm(torch.zeros(1, 40000, dtype=torch.float16, device=DEV),
                                   torch.ones(40000, dtype=torch.float16, device=DEV), 1e-6)


def test_autograd_backward_matches_oracle():
    L = make_random_layer(4, 128, 256, 128, seed=8)
    layer = quant.QuantLinear(4, 128, 256, 128, False)
    layer.qweight, layer.qzeros, layer.scales, layer.g_idx = (dev(L['qweight']), dev(L['qzeros']), dev(L['scales']),
                                                               dev(L['g_idx']))
    x = dev(np.random.default_rng(0).standard_normal((3, 256)).astype(np.float16)).requires_grad_(True)
    y = layer(x)
    dy = np.random.default_rng(1).standard_normal((3, 128)).astype(np.float16)
    y.backward(dev(dy))
    ref = oracle.transpose_matmul248(dy, L['qweight'], L['scales'], L['qzeros'], L['g_idx'], 4)
    assert rel_err(x.grad.cpu().numpy(), ref) < TOL


@pytest.mark.parametrize('family', [None, 'abi'])
@pytest.mark.parametrize('bits,gs,act,M,K,N', [(4, 128, False, 300, 512, 288), (4, 128, True, 64, 1024, 512), (3, -1, False, 16, 256, 320),
                                               (2, 64, False, 16, 512, 256), (8, 32, False, 2048, 256, 1024)])
def test_backward_both_routes_vs_oracle(family, bits, gs, act, M, K, N):
    """dx = dy . deq(W)^T (reference quant_linear.py:191-258, :272-279): from 16 rows on through the prefill route (our dequantise
    kernel + hipBLASLt with the transposition flag, gptq_prefill_transpose_matmul248_f16) and, with family='abi', through the
    LDS-tiled kernel of transpose.hip -- every width, act-order included."""
    L = make_random_layer(bits, gs, K, N, act_order=act, seed=M + bits)
    dy = np.random.default_rng(M).standard_normal((M, N)).astype(np.float16)
    dx = QL.transpose_matmul248(dev(dy), dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), dev(L['g_idx']), bits, 2**bits - 1,
                                family=family).cpu().numpy()
    ref = oracle.transpose_matmul248(dy, L['qweight'], L['scales'], L['qzeros'], L['g_idx'], bits)
    assert dx.shape == (M, K) and rel_err(dx, ref) < TOL, rel_err(dx, ref)


def _fuzz_cases(n=96, seed=2024):
    rng = np.random.default_rng(seed)
    cases = []
    while len(cases) < n:
        bits = int(rng.choice([2, 3, 4, 8]))
        gs = int(rng.choice([-1, 32, 64, 128]))
        K = 32 * int(rng.integers(1, 65))
        if gs != -1 and K % gs:
            continue
        N = 32 * int(rng.integers(1, 33))
        M = int(rng.choice([1, 1, 1, 2, 3, 5, 16, 17, 40, 70, 130, 300]))
        act = bool(rng.integers(0, 4) == 0) and gs != -1
        fam = [None, 'abi'][int(rng.integers(0, 2))]
        cases.append((bits, gs, K, N, M, act, bool(rng.integers(0, 2)), fam))
    return cases


@pytest.mark.parametrize('case', _fuzz_cases(), ids=lambda c: 'w%dg%d_K%d_N%d_M%d%s%s_%s' % (c[0], c[1], c[2], c[3], c[4], '_act' if c[5] else '',
                                                                                      '_bias' if c[6] else '', c[7] or 'py'))
def test_fuzz_shapes_vs_oracle(case):
    """seeded random sweep over bits / group / act-order / ragged shapes / M regimes through both the
    Python dispatch and the bare C-ABI dispatch: every kernel family against the oracle."""
    bits, gs, K, N, M, act, with_bias, fam = case
    L = make_random_layer(bits, gs, K, N, act_order=act, seed=K + N + M + bits)
    rng = np.random.default_rng(K * 7 + N)
    x = rng.standard_normal((M, K)).astype(np.float16)
    bias = rng.standard_normal(N).astype(np.float16) if with_bias else None
    check_forward(x, L, bias=bias, family=fam)


def _fuzz_mlp_cases(n=32, seed=77):
    rng = np.random.default_rng(seed)
    cases = []
    while len(cases) < n:
        bits = int(rng.choice([2, 4, 4, 8, 3]))
        gs = int(rng.choice([-1, 32, 128]))
        K = 32 * int(rng.integers(1, 40))
        if gs != -1 and K % gs:
            continue
        cases.append((bits, gs, K, 32 * int(rng.integers(1, 24)), int(rng.choice([1, 1, 2, 4, 9, 33, 70, 200])), bool(rng.integers(0, 5) == 0) and gs != -1))
    return cases


@pytest.mark.parametrize('case', _fuzz_mlp_cases(), ids=lambda c: 'w%dg%d_K%d_N%d_M%d%s' % (c[0], c[1], c[2], c[3], c[4], '_act' if c[5] else ''))
def test_fuzz_fused_mlp_vs_oracle(case):
    """silu(x.Wg) * (x.Wu) through every regime of the fused path (rowwave pair-atomic, MFMA stream kernel,
    generic kernel for 3-bit / act-order, two GEMMs for prefill) against the oracle's fused restatement."""
    bits, gs, K, N, M, act = case
    A = make_random_layer(bits, gs, K, N, act_order=act, seed=K + N)
    B = make_random_layer(bits, gs, K, N, act_order=act, seed=K + N + 1)
    if act:
        B['g_idx'] = A['g_idx'].copy()          # gate and up see the same input: same act-order permutation
    x = (np.random.default_rng(M + K).standard_normal((M, K)) * 0.5).astype(np.float16)
    gate = tuple(dev(A[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    up = tuple(dev(B[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    c = quant.fused_mlp.fused_gate_up(dev(x), gate, up, bits, K if gs == -1 else gs).cpu().numpy()
    ref = oracle.fused_mlp(x, (A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), bits)
    assert np.isfinite(c.astype(np.float32)).all()
    assert rel_err(c, ref) < TOL
    assert_not_worse_than_reference(c, ref, oracle.fused_mlp_exact(x, (A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), bits))


# ---------------------------------------------------------------------------------------
# stripe16 decode path (csrc/stripe.hip): repack bit-exact vs the numpy restatement; matvec vs the oracle on the
# ORIGINAL checkpoint buffers (the layout must be invisible in the results)
# ---------------------------------------------------------------------------------------
def _stripe_image(Ls, gs, bits=4):
    K = Ls[0]['qweight'].shape[0] * 32 // bits
    t = [(dev(L['qweight']), dev(L['scales']), dev(L['qzeros'])) for L in Ls]
    st = QL.stripe_copy(t[0][0], t[0][1], t[0][2], bits, K if gs == -1 else gs, up=t[1] if len(t) == 2 else None)
    torch.cuda.synchronize()
    return st, t


@pytest.mark.parametrize('bits,K,N,gs,NS', [(4, 4096, 4096, 128, 1), (4, 1024, 288, 64, 2), (4, 384, 64, 32, 1), (4, 512, 64, -1, 2),
                                            (4, 2176, 32, 128, 1), (4, 4096, 11008, 128, 2), (8, 4096, 512, 128, 1), (8, 1088, 96, 64, 2),
                                            (8, 192, 32, 16, 1), (2, 4096, 512, 128, 1), (2, 1280, 64, 64, 2), (2, 512, 32, -1, 1),
                                            (3, 4096, 512, -1, 1), (3, 1152, 96, 128, 2), (3, 384, 32, 32, 1)])
def test_stripe_repack_bit_exact(bits, K, N, gs, NS):
    Ls = [make_random_layer(bits, gs, K, N, seed=K + N + i) for i in range(NS)]
    st, _ = _stripe_image(Ls, gs, bits)
    assert st is not None
    ref = oracle.stripe16_repack([(L['qweight'], L['scales'], L['qzeros']) for L in Ls], gs, bits)
    assert np.array_equal(st.cpu().numpy(), ref)


@pytest.mark.parametrize('M', [1, 3])
@pytest.mark.parametrize('bits,K,N,gs', [(8, 4096, 4096, 128), (8, 11008, 256, 128), (8, 64, 32, 64), (8, 1088, 96, 16), (8, 2240, 64, 32),
                                         (8, 22016, 32, 128), (8, 512, 64, -1), (2, 4096, 4096, 128), (2, 11008, 256, 128), (2, 256, 32, 64),
                                         (2, 2304, 96, 256), (2, 24576, 32, 128), (2, 1024, 64, -1),
                                         (3, 4096, 4096, -1), (3, 4096, 11008, -1), (3, 11008, 256, -1), (3, 4096, 512, 128), (3, 1152, 96, 32), (3, 2176, 64, 64),
                                         (3, 24576, 32, 128), (3, 128, 32, -1)])
def test_stripe_2bit_and_8bit_vs_oracle(bits, K, N, gs, M):
    """the reference's other widths (quant_linear.py:308) on the stripe16 kernel: every unpack position of a word, ragged
    row-block counts, group sizes from one lane block to all of K; M = 3 rides along for free"""
    L = make_random_layer(bits, gs, K, N, seed=bits * K + N)
    x = np.random.default_rng(K + M).standard_normal((M, K)).astype(np.float16)
    fam = 'stripe' if (M == 1 or K <= 16384) else None      # four rows of a longer K do not fit in LDS: the dispatch falls back
    y1, ref = check_forward(x, L, family=fam)
    y2 = hip_forward(x, L, family=fam)
    assert np.array_equal(y1.view(np.uint16), y2.view(np.uint16))
    ye = oracle.matmul248_exact(x, L['qweight'], L['scales'], L['qzeros'], L['g_idx'], bits)
    assert rel_err(y1, ye) < TOL
    assert rel_err(y1, hip_forward(x, L, family='gemv')) < TOL            # and against round 1's rowwave kernel


@pytest.mark.parametrize('M', [2, 3, 4])
@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('K,N,gs', [(4096, 4096, 128), (11008, 256, 128), (1024, 288, 32), (2176, 96, 64), (512, 64, -1)])
def test_stripe_small_batch_rows(K, N, gs, M, bias):
    """2 <= M <= 4: lane l supplies row l % 4 of x to the MFMA, result row i is x row i -- every row against the oracle,
    strided x, each row equal (bit for bit) to what the M = 1 launch returns for it"""
    L = make_random_layer(4, gs, K, N, seed=K + N + M)
    rng = np.random.default_rng(M)
    xs = rng.standard_normal((M, K + 64)).astype(np.float16)
    x = xs[:, :K]                                                           # row stride K + 64
    b = rng.standard_normal(N).astype(np.float16) if bias else None
    y = hip_forward(np.ascontiguousarray(x), L, b, family='stripe')
    ref = oracle_forward(np.ascontiguousarray(x), L, b)
    assert rel_err(y, exact_forward(np.ascontiguousarray(x), L, b) if bias else ref) < TOL
    xt = dev(xs)[:, :K]
    ys = QL.matmul248(xt, dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), dev(L['g_idx']), 4, 15, bias=None if b is None else dev(b),
                      family='stripe').cpu().numpy()
    assert np.array_equal(ys.view(np.uint16), y.view(np.uint16))
    for m in range(M):
        y1 = hip_forward(np.ascontiguousarray(x[m:m + 1]), L, b, family='stripe')
        assert np.array_equal(y1.view(np.uint16), y[m:m + 1].view(np.uint16))


@pytest.mark.parametrize('M', [5, 8, 9, 13, 16])
@pytest.mark.parametrize('bits,K,N,gs', [(4, 4096, 4096, 128), (4, 4096, 11008, 128), (4, 2176, 96, 64), (8, 2048, 288, 128), (2, 4096, 64, 128), (3, 4096, 96, -1)])
def test_stripe_row_groups_m5_to_16(bits, K, N, gs, M):
    """5 <= M <= 16 in the decode launch: every row against the oracle.  Rounds 2-5 ran two / four 4x4x4 row groups on the same unpacked words, whose
    rows were bit-identical to the M = 1 launch; since round 6 these batches go through v_mfma_f32_16x16x16_f16 wherever the group spans a row
    block (the matrix core sums the four k quads of a row block, the x sums are per row block): another summation order than the one-row
    launch, so a row equals its M = 1 result to the op-level bar, not bit for bit -- what still holds bit for bit is that a row's result does not
    depend on WHERE it sits in the batch, nor on the other rows."""
    L = make_random_layer(bits, gs, K, N, seed=K + N + M)
    x = np.random.default_rng(M).standard_normal((M, K)).astype(np.float16)
    y, ref = check_forward(x, L, family='stripe')
    for m in (0, M // 2, M - 1):
        y1 = hip_forward(x[m:m + 1], L, family='stripe')
        assert rel_err(y1, y[m:m + 1]) < TOL
    perm = np.random.default_rng(2).permutation(M)
    yp = hip_forward(np.ascontiguousarray(x[perm]), L, family='stripe')
    assert np.array_equal(yp.view(np.uint16), y[perm].view(np.uint16))
    x2 = x.copy()
    x2[1:] = np.random.default_rng(3).standard_normal((M - 1, K)).astype(np.float16)      # other neighbours, the same row 0
    y2 = hip_forward(x2, L, family='stripe')
    assert np.array_equal(y2[:1].view(np.uint16), y[:1].view(np.uint16))


@pytest.mark.parametrize('M', [5, 16, 17, 33, 48, 64, 65, 100, 128])
@pytest.mark.parametrize('bits,K,N,gs', [(4, 4096, 4096, 128), (4, 4096, 11008, 128), (4, 11008, 4096, 128), (4, 1152, 288, 128), (4, 2048, 96, -1),
                                         (4, 3072, 64, 256), (8, 2048, 288, 64), (8, 4096, 4096, 128), (8, 1088, 96, -1),
                                         # prescale kernels (group smaller than a row block) and the other widths
                                         (4, 2048, 96, 32), (4, 4096, 512, 64), (8, 1088, 96, 16), (8, 2048, 160, 32), (2, 4096, 512, 128), (2, 1024, 96, -1),
                                         (2, 2304, 64, 64), (3, 4096, 512, -1), (3, 1152, 96, 32), (3, 4096, 11008, 128)])
def test_stripe_mm_vs_oracle(bits, K, N, gs, M):
    """5 <= M <= 64 on the stripe16 image through 16-row MFMA tiles (gptq_stripe_matmul_f16): one launch (x streamed through LDS)
    or K slices + the reduce kernel, ragged row-block counts, column groups that are not full (N % 128), one group; against the
    oracle, run twice (bit-reproducible), and every row independent of its position in the batch"""
    L = make_random_layer(bits, gs, K, N, seed=K + N + M)
    x = np.random.default_rng(M).standard_normal((M, K)).astype(np.float16)
    y, ref = check_forward(x, L, family='stripe_mm')
    y2 = hip_forward(x, L, family='stripe_mm')
    assert np.array_equal(y.view(np.uint16), y2.view(np.uint16))
    perm = np.random.default_rng(1).permutation(M)
    yp = hip_forward(np.ascontiguousarray(x[perm]), L, family='stripe_mm')
    if M <= 64:     # one pass, one schedule: a row's result does not depend on where it sits in the batch
        assert np.array_equal(yp.view(np.uint16), y[perm].view(np.uint16))
    else:           # passes of 64 rows may take different schedules (one launch vs K slices): same value up to fp32 summation order
        assert rel_err(yp, y[perm]) < TOL


@pytest.mark.parametrize('M', [17, 40, 64, 77, 80, 96, 112, 113, 128])
@pytest.mark.parametrize('K,N,gs', [(4096, 11008, 128), (1024, 6176, 128), (2048, 8192, 256), (1152, 12288, -1), (11008, 4096, 128), (6272, 3584, 128)])
def test_stripe_mm_loader_consumer_route(K, N, gs, M):
    """17 .. 128 rows on shapes whose stripes need two or three rounds of workgroups and K <= 8192 -- the home ground of the loader / consumer kernel
    (csrc/stripe_mm.inc stripe_mmr_kernel, round 6: x through an LDS ring of (row block, 64-row pass) chunks, two passes per row block from 65 rows on):
    a ragged stripe count (688 = 229 x 3 + 1: the last workgroup's clamped stripes), ragged batches (rows >= M are clamped loads and
    skipped stores), groups of two row blocks and one group, a row-block count that is not a multiple of the six consumer waves / two loader waves, a
    bias, and x as a strided view; against the oracle, bit-reproducible, every row bit-independent of its position (ONE launch, one schedule).
    The last two shapes (one round of stripes, long K: LLaMA-7B's down_proj; 224 stripes x 49 row blocks) take its K-SLICED form -- four stripes x four
    slices per round of workgroups (a ragged last slice: 86 = 3 x 22 + 20, 49 = 3 x 13 + 10), fp32 rows per slice, the combine launch adds them in slice order"""
    L = make_random_layer(4, gs, K, N, seed=K + N + M)
    rng = np.random.default_rng(M)
    x = rng.standard_normal((M, K)).astype(np.float16)
    y, ref = check_forward(x, L, family='stripe_mm')
    assert np.array_equal(hip_forward(x, L, family='stripe_mm').view(np.uint16), y.view(np.uint16))
    perm = rng.permutation(M)
    yp = hip_forward(np.ascontiguousarray(x[perm]), L, family='stripe_mm')
    assert np.array_equal(yp.view(np.uint16), y[perm].view(np.uint16))
    ya = hip_forward(x, L)                                                   # the layer ABI's own dispatch: the same launch
    assert np.array_equal(ya.view(np.uint16), y.view(np.uint16))
    assert _native.lib().gptq_layer_route_for_shape(M, K, N, 4, K if gs == -1 else gs, 1, 0, 1) == 2         # GPTQ_ROUTE_STRIPE_TILES
    bias = rng.standard_normal(N).astype(np.float16)
    xs = np.zeros((M, K + 72), dtype=np.float16)
    xs[:, :K] = x
    xs[:, K:] = np.float16(np.nan)          # (nothing beyond a row's K columns may be read into a sum)
    args = (dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), dev(L['g_idx']), 4, 15)
    yb = QL.matmul248(dev(xs)[:, :K], *args, bias=dev(bias)).cpu().numpy()
    assert rel_err(yb, exact_forward(x, L, bias)) < TOL
    yb2 = QL.matmul248(dev(x), *args, bias=dev(bias)).cpu().numpy()
    assert np.array_equal(yb.view(np.uint16), yb2.view(np.uint16))


@pytest.mark.parametrize('M', [129, 200, 256, 384, 1000])
@pytest.mark.parametrize('bits,K,N,gs', [(4, 4096, 4096, 128), (4, 4096, 11008, 128), (4, 11008, 4096, 128), (4, 1152, 288, 128), (4, 2048, 96, -1),
                                         (4, 3072, 64, 256), (8, 2048, 288, 64), (8, 1088, 96, -1), (3, 4096, 512, -1), (3, 1152, 160, 128)])
def test_stripe_gemm_vs_oracle(bits, K, N, gs, M):
    """batches above 128 rows on the stripe16 image: the 2-D tiled fused-dequantise GEMM (csrc/stripe_mm.inc stripe_gemm_kernel, reached
    through gptq_stripe_matmul_f16 and through gptq_layer_forward up to gptq_set_stripe_gemm_max_rows): ragged last row tile (M % 128),
    column groups that are not full (N % 128), K that is not a multiple of the four-chunk round, one group, 3 / 8 bits; against the
    oracle at 1e-3, bit-reproducible, rows independent of their position"""
    if K * M > 3e6 and N > 4096:
        M = min(M, 384)                  # keep the oracle's share of the run time bounded on the widest layer
    L = make_random_layer(bits, gs, K, N, seed=K + N + M)
    x = np.random.default_rng(M).standard_normal((M, K)).astype(np.float16)
    y, ref = check_forward(x, L, family='stripe_mm')
    y2 = hip_forward(x, L, family='stripe_mm')
    assert np.array_equal(y.view(np.uint16), y2.view(np.uint16))
    perm = np.random.default_rng(1).permutation(M)
    yp = hip_forward(np.ascontiguousarray(x[perm]), L, family='stripe_mm')
    assert np.array_equal(yp.view(np.uint16), y[perm].view(np.uint16))      # one schedule for every row tile
    ya = hip_forward(x, L)                                                   # the layer ABI takes the same kernel (M <= 1024)
    assert np.array_equal(ya.view(np.uint16), y.view(np.uint16))
    lib = _native.lib()
    assert lib.gptq_layer_route_for_shape(M, K, N, bits, K if gs == -1 else gs, 1, 0, 1) == 3     # ... and the host-side table says so (GPTQ_ROUTE_STRIPE_GEMM)
    prev = lib.gptq_set_stripe_gemm_max_rows(0)                              # ... and the dense route when it is switched off
    try:
        yd = hip_forward(x, L)
    finally:
        lib.gptq_set_stripe_gemm_max_rows(prev)
    assert rel_err(yd, ref) < TOL


@pytest.mark.parametrize('M', [130, 300])
@pytest.mark.parametrize('bits,K,N,gs', [(4, 4096, 11008, 128), (8, 1024, 288, 64), (4, 1280, 96, 128)])
def test_stripe_gemm_fused_mlp_and_bias(bits, K, N, gs, M):
    """the pair instance (gate | up of one stripe per wave, SiLU on the fp32 sums) and the bias epilogue of the single-set instance"""
    A, B = make_random_layer(bits, gs, K, N, seed=81), make_random_layer(bits, gs, K, N, seed=82)
    x = (np.random.default_rng(M).standard_normal((M, K)) * 0.5).astype(np.float16)
    gate = tuple(dev(A[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    up = tuple(dev(B[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    c = quant.fused_mlp.fused_gate_up(dev(x), gate, up, bits, gs, family='stripe_mm').cpu().numpy()
    sets = ((A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx']))
    ref = oracle.fused_mlp(x, sets[0], sets[1], bits)
    assert rel_err(c, ref) < TOL
    assert_not_worse_than_reference(c, ref, oracle.fused_mlp_exact(x, sets[0], sets[1], bits))
    c2 = quant.fused_mlp.fused_gate_up(dev(x), gate, up, bits, gs).cpu().numpy()     # the default dispatch takes the same kernel ...
    if M > 16:
        assert np.array_equal(c.view(np.uint16), c2.view(np.uint16))
    else:       # ... except for 9 .. 16 rows of a pair (round 6): the decode launch with sixteen A rows where it serves the shape -- the same bars
        assert rel_err(c2, ref) < TOL
        assert_not_worse_than_reference(c2, ref, oracle.fused_mlp_exact(x, (A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), bits))
    bias = (np.random.default_rng(3).standard_normal(N) * 0.1).astype(np.float16)
    yb, _ = check_forward(x, A, bias=bias)
    yf, _ = check_forward(x, A, bias=bias, family='stripe_mm')
    assert np.array_equal(yb.view(np.uint16), yf.view(np.uint16))


@pytest.mark.parametrize('M', [6, 33, 70])
def test_stripe_mm_strided_rows(M):
    """x as a column slice of a wider buffer (row stride K + 64, the way a fused qkv / hidden-state view arrives): same bits as
    the contiguous copy, on every schedule the dispatch picks for these M (row groups / one launch / K slices / two passes)"""
    K, N = 2048, 384
    L = make_random_layer(4, 128, K, N, seed=M)
    xs = np.random.default_rng(M).standard_normal((M, K + 64)).astype(np.float16)
    b = np.random.default_rng(2).standard_normal(N).astype(np.float16)
    args = (dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), dev(L['g_idx']), 4, 15)
    y_view = QL.matmul248(dev(xs)[:, :K], *args, bias=dev(b)).cpu().numpy()
    y_copy = QL.matmul248(dev(np.ascontiguousarray(xs[:, :K])), *args, bias=dev(b)).cpu().numpy()
    assert np.array_equal(y_view.view(np.uint16), y_copy.view(np.uint16))
    assert rel_err(y_view, exact_forward(np.ascontiguousarray(xs[:, :K]), L, b)) < TOL


@pytest.mark.parametrize('slices', [0, 4, 7, 16])
@pytest.mark.parametrize('M', [16, 64])
def test_stripe_mm_forced_variants(M, slices):
    """both schedules on the same problem: one launch (0) and S K slices; with a bias (two fp16 roundings: bar held against the float64 result)"""
    L = make_random_layer(4, 128, 4096 + 128, 512, seed=M)
    x = np.random.default_rng(M).standard_normal((M, 4096 + 128)).astype(np.float16)
    b = np.random.default_rng(3).standard_normal(512).astype(np.float16)
    lib = quant._native.lib()
    prev = lib.gptq_set_split_k(slices)
    try:
        y = hip_forward(x, L, b, family='stripe_mm')
    finally:
        lib.gptq_set_split_k(prev)
    assert rel_err(y, exact_forward(x, L, b)) < TOL


@pytest.mark.parametrize('bits,K,N,gs', [(4, 4096, 11008, 128), (8, 1024, 288, 64), (4, 11008 // 2, 256, 128), (2, 1024, 96, 128), (3, 1152, 96, 128),
                                         (4, 1024, 160, 32)])
@pytest.mark.parametrize('M', [9, 16, 40, 64, 100])
def test_stripe_mm_fused_mlp(bits, K, N, gs, M):
    A, B = make_random_layer(bits, gs, K, N, seed=81), make_random_layer(bits, gs, K, N, seed=82)
    x = (np.random.default_rng(M).standard_normal((M, K)) * 0.5).astype(np.float16)
    gate = tuple(dev(A[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    up = tuple(dev(B[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    c = quant.fused_mlp.fused_gate_up(dev(x), gate, up, bits, gs, family='stripe_mm').cpu().numpy()
    ref = oracle.fused_mlp(x, (A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), bits)
    assert rel_err(c, ref) < TOL
    assert_not_worse_than_reference(c, ref, oracle.fused_mlp_exact(x, (A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), bits))
    c2 = quant.fused_mlp.fused_gate_up(dev(x), gate, up, bits, gs).cpu().numpy()     # the default dispatch takes the same kernel ...
    if M > 16:
        assert np.array_equal(c.view(np.uint16), c2.view(np.uint16))
    else:       # ... except for 9 .. 16 rows of a pair (round 6): the decode launch with sixteen A rows where it serves the shape -- the same bars
        assert rel_err(c2, ref) < TOL
        assert_not_worse_than_reference(c2, ref, oracle.fused_mlp_exact(x, (A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), bits))


@pytest.mark.parametrize('M', [17, 48, 64, 77, 96, 112, 113, 128])
@pytest.mark.parametrize('K,N,gs', [(4096, 11008, 128), (1024, 6176, 128), (1152, 8192, -1)])
def test_stripe_mm_loader_consumer_pair(K, N, gs, M):
    """the gate | up pair at 17 .. 128 rows on shapes with two or three rounds of column stripes: the loader / consumer kernel with the consumers
    split by SET (csrc/stripe_mm.inc stripe_mmr_kernel<.., NS = 2, SS = 1>, round 6) -- three k lanes per set, a chunk of x released when the
    consumers of both sets are done with it, SiLU(gate) * up on the fp32 sums; 113 .. 128 rows of three-stripe shapes run as two launches
    of the four-tile instance, rows 0 .. 63 and 64 .. M - 1 (an eight-tile instance of three stripes would spill).  Against the oracle and the float64 result, bit-reproducible, rows bit-independent
    of their position, x as a strided view with NaN padding, the default dispatch takes the same launch"""
    A, B = make_random_layer(4, gs, K, N, seed=K + M), make_random_layer(4, gs, K, N, seed=K + M + 1)
    rng = np.random.default_rng(M)
    gsz = K if gs == -1 else gs
    x = (rng.standard_normal((M, K)) * 0.5).astype(np.float16)
    gate = tuple(dev(A[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    up = tuple(dev(B[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    sets = ((A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx']))
    c = quant.fused_mlp.fused_gate_up(dev(x), gate, up, 4, gsz, family='stripe_mm').cpu().numpy()
    ref = oracle.fused_mlp(x, sets[0], sets[1], 4)
    assert rel_err(c, ref) < TOL
    assert_not_worse_than_reference(c, ref, oracle.fused_mlp_exact(x, sets[0], sets[1], 4))
    c2 = quant.fused_mlp.fused_gate_up(dev(x), gate, up, 4, gsz).cpu().numpy()
    assert np.array_equal(c.view(np.uint16), c2.view(np.uint16))
    perm = rng.permutation(M)
    cp = quant.fused_mlp.fused_gate_up(dev(np.ascontiguousarray(x[perm])), gate, up, 4, gsz, family='stripe_mm').cpu().numpy()
    assert np.array_equal(cp.view(np.uint16), c[perm].view(np.uint16))
    xs = np.full((M, K + 72), np.nan, dtype=np.float16)
    xs[:, :K] = x
    cs = quant.fused_mlp.fused_gate_up(dev(xs)[:, :K], gate, up, 4, gsz).cpu().numpy()
    assert np.array_equal(cs.view(np.uint16), c.view(np.uint16))


def test_stripe_long_k_small_batch():
    """M rows of x must fit in LDS.  Round 5: 5 .. 8 rows on K = 11008 (LLaMA-7B down_proj) run in the decode kernel with x staged in two K
    halves (stripe_gemv2p_kernel) -- with a bias and with a per-row residual; 16 rows on that K, or 8 rows on K = 22016, are still refused by
    the stripe kernel (GPTQ_E_VARIANT) and the default dispatch takes the 16-row MFMA tiles -- same result"""
    L = make_random_layer(4, 128, 11008, 256, seed=8)
    rng = np.random.default_rng(8)
    for M in (5, 7, 8):
        x = rng.standard_normal((M, 11008)).astype(np.float16)
        y = hip_forward(x, L, family='stripe')
        assert rel_err(y, oracle_forward(x, L)) < TOL, M
        bias = rng.standard_normal(256).astype(np.float16)
        yb = hip_forward(x, L, bias=bias, family='stripe')
        assert rel_err(yb, exact_forward(x, L, bias)) < TOL, M
        check_forward(x, L)                                   # the default dispatch takes the same kernel
    # ragged tail: K = 11008 + 128 (87 row blocks: the last wave-round is partial in the second phase), one group per 64 k
    L2 = make_random_layer(4, 64, 11136, 96, seed=9)
    x = rng.standard_normal((6, 11136)).astype(np.float16)
    assert rel_err(hip_forward(x, L2, family='stripe'), oracle_forward(x, L2)) < TOL
    x = rng.standard_normal((16, 11008)).astype(np.float16)
    with pytest.raises(RuntimeError):
        hip_forward(x, L, family='stripe')
    check_forward(x, L)
    L3 = make_random_layer(4, 128, 22016, 64, seed=10)
    x = rng.standard_normal((8, 22016)).astype(np.float16)
    with pytest.raises(RuntimeError):
        hip_forward(x, L3, family='stripe')
    check_forward(x, L3)


@pytest.mark.parametrize('bits,K,N,gs', [(4, 4096, 11008, 128), (8, 1024, 288, 64), (2, 1024, 96, 128), (3, 4096, 11008, 4096), (3, 1152, 96, 128)])
@pytest.mark.parametrize('M', [2, 4, 7, 8])
def test_stripe_fused_mlp_small_batch(bits, K, N, gs, M):
    A, B = make_random_layer(bits, gs, K, N, seed=71), make_random_layer(bits, gs, K, N, seed=72)
    x = (np.random.default_rng(M).standard_normal((M, K)) * 0.5).astype(np.float16)
    gate = tuple(dev(A[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    up = tuple(dev(B[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    c = quant.fused_mlp.fused_gate_up(dev(x), gate, up, bits, gs).cpu().numpy()
    assert quant.layer._LAYERS.get(gate[0]) is not None and quant.layer._LAYERS.get(gate[0])[1].stripe is not None
    ref = oracle.fused_mlp(x, (A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), bits)
    assert rel_err(c, ref) < TOL
    assert_not_worse_than_reference(c, ref, oracle.fused_mlp_exact(x, (A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), bits))


@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('K,N,gs', [(4096, 4096, 128), (4096, 12288, 128), (11008, 4096, 128), (128, 32, 128), (1024, 288, 32), (2176, 96, 64),
                                    (3072, 64, 256), (512, 64, -1), (8192, 256, 128), (22016, 64, 128), (24576, 32, 128), (5120, 160, 128)])
def test_stripe_matvec_vs_oracle(K, N, gs, bias):
    """every row-block count per wave (1 .. 24, ragged tails), group sizes 32 .. K, bias epilogue; twice: bit-identical"""
    L = make_random_layer(4, gs, K, N, seed=K + N)
    x = np.random.default_rng(K).standard_normal((1, K)).astype(np.float16)
    b = np.random.default_rng(N).standard_normal(N).astype(np.float16) if bias else None
    y1 = hip_forward(x, L, b, family='stripe')
    ref = oracle_forward(x, L, b)
    # with a bias the result is rounded to fp16 twice (fp16(fp16(acc) + bias), reference quant_linear.py:376): a 1-ulp difference of
    # the first rounding against the faithful oracle can survive as 1-2 ulp of a LARGER sum -> the bar is held against the float64 result there
    assert rel_err(y1, exact_forward(x, L, b) if bias else ref) < TOL, rel_err(y1, ref)
    y2 = hip_forward(x, L, b, family='stripe')
    assert np.array_equal(y1.view(np.uint16), y2.view(np.uint16))
    ye = oracle.matmul248_exact(x, L['qweight'], L['scales'], L['qzeros'], L['g_idx'], 4)
    if b is None:
        assert rel_err(y1, ye) < TOL


def test_stripe_is_the_default_decode_path_and_rowwave_still_agrees():
    L = make_random_layer(4, 128, 4096, 4096, seed=5)
    x = np.random.default_rng(5).standard_normal((1, 4096)).astype(np.float16)
    ys = hip_forward(x, L)                       # default dispatch at M == 1
    yf = hip_forward(x, L, family='stripe')
    yr = hip_forward(x, L, family='gemv')        # rowwave (split-K) on the checkpoint layout
    assert np.array_equal(ys.view(np.uint16), yf.view(np.uint16))
    assert rel_err(ys, yr) < TOL
    with pytest.raises(RuntimeError):            # shapes the stripe kernel does not serve are refused when forced
        hip_forward(x[:, :1056], make_random_layer(4, 32, 1056, 64, seed=1), family='stripe')          # K % 128
    with pytest.raises(RuntimeError):
        hip_forward(np.tile(x, (17, 1)), L, family='stripe')                                             # M > 16


@pytest.mark.parametrize('K,N,gs', [(4096, 11008, 128), (1024, 2816, 64), (512, 96, 32), (2176, 32, -1)])
def test_stripe_fused_mlp_vs_oracle(K, N, gs):
    A, B = make_random_layer(4, gs, K, N, seed=31), make_random_layer(4, gs, K, N, seed=32)
    x = (np.random.default_rng(2).standard_normal((1, K)) * 0.5).astype(np.float16)
    g = K if gs == -1 else gs
    gate = tuple(dev(A[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    up = tuple(dev(B[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    c = quant.fused_mlp.fused_gate_up(dev(x), gate, up, 4, g).cpu().numpy()
    c2 = quant.fused_mlp.fused_gate_up(dev(x), gate, up, 4, g).cpu().numpy()
    assert quant.layer._LAYERS.get(gate[0]) is not None and quant.layer._LAYERS.get(gate[0])[1].stripe is not None   # the pair image was built and is kept
    ref = oracle.fused_mlp(x, (A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), 4)
    assert rel_err(c, ref) < TOL
    assert_not_worse_than_reference(c, ref, oracle.fused_mlp_exact(x, (A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), 4))
    assert np.array_equal(c.view(np.uint16), c2.view(np.uint16))


@pytest.mark.parametrize('K,N,gs,NS', [(4096, 12288, 128, 1), (1024, 288, 64, 1), (4096, 11008, 128, 2), (2176, 64, 32, 2)])
def test_stripe_fused_rmsnorm(K, N, gs, NS):
    """[RMSNorm -> QuantLinear] and [RMSNorm -> gate/up + SiLU] in one launch vs oracle.rmsnorm + oracle matvec"""
    Ls = [make_random_layer(4, gs, K, N, seed=41 + i) for i in range(NS)]
    rng = np.random.default_rng(K)
    x = rng.standard_normal((1, K)).astype(np.float16)
    nw = (1 + 0.1 * rng.standard_normal(K)).astype(np.float16)
    eps = 1e-6
    st, _ = _stripe_image(Ls, gs)
    out = torch.empty((1, N), dtype=torch.float16, device=DEV)
    QL.stripe_matvec(dev(x), st, out, K, N, 4, K if gs == -1 else gs, nsets=NS, norm_weight=dev(nw), eps=eps)
    torch.cuda.synchronize()
    xn = oracle.rmsnorm(x, nw, eps)
    if NS == 1:
        ref = oracle.matmul248(xn, Ls[0]['qweight'], Ls[0]['scales'], Ls[0]['qzeros'], Ls[0]['g_idx'], 4)
    else:
        ref = oracle.fused_mlp(xn, *[(L['qweight'], L['scales'], L['qzeros'], L['g_idx']) for L in Ls], 4)
    assert rel_err(out.cpu().numpy(), ref) < TOL


@pytest.mark.parametrize('bits,K,N,gs', [(4, 4096, 4096, 128), (4, 1024, 288, 32), (4, 2176, 64, 64), (3, 4096, 4096, 128), (3, 256, 768, 128), (3, 1152, 288, 32),
                                         (8, 1024, 96, 64)])
@pytest.mark.parametrize('norm', [False, True])
@pytest.mark.parametrize('pair', [False, True])
def test_stripe_act_order(bits, K, N, gs, norm, pair):
    """act-order layer (or gate/up pair sharing one permutation): the image holds the rows sorted by group (gathered from the checkpoint layout
    while it is written); x -- optionally RMS-normalised first -- is gathered through the permutation inside the decode kernel.  Against the
    oracle on the ORIGINAL g_idx.  3-bit since round 4."""
    Ls = [make_random_layer(bits, gs, K, N, act_order=True, seed=K + i) for i in range(2 if pair else 1)]
    for L in Ls[1:]:
        L['g_idx'] = Ls[0]['g_idx']
    rng = np.random.default_rng(N)
    x = rng.standard_normal((1, K)).astype(np.float16)
    nw = (1 + 0.1 * rng.standard_normal(K)).astype(np.float16)
    sets = tuple(tuple(dev(L[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx')) for L in Ls)
    pl = quant.layer.prepared(sets, None, bits, gs, K, N)
    assert pl.kind == 1 and pl.stripe is not None and pl.perm16 is not None
    out = torch.empty((1, N), dtype=torch.float16, device=DEV)
    QL.stripe_matvec(dev(x), pl.stripe, out, K, N, bits, gs, nsets=len(Ls), norm_weight=dev(nw) if norm else None, eps=1e-6, perm=pl.perm16)
    torch.cuda.synchronize()
    xin = oracle.rmsnorm(x, nw, 1e-6) if norm else x
    ts = [(L['qweight'], L['scales'], L['qzeros'], L['g_idx']) for L in Ls]
    ref = oracle.fused_mlp(xin, ts[0], ts[1], bits) if pair else oracle.matmul248(xin, *ts[0], bits)
    assert rel_err(out.cpu().numpy(), ref) < TOL


def test_stripe_copy_follows_buffer_updates():
    """the cached image is keyed by the version counters of the checkpoint buffers: an in-place update (load_state_dict)
    rebuilds it"""
    L1, L2 = make_random_layer(4, 128, 512, 64, seed=1), make_random_layer(4, 128, 512, 64, seed=2)
    m = quant.QuantLinear(4, 128, 512, 64, False).to(DEV)
    x = np.random.default_rng(0).standard_normal((1, 512)).astype(np.float16)
    for L in (L1, L2):
        m.load_state_dict({k: torch.from_numpy(L[k]) for k in ('qweight', 'qzeros', 'scales', 'g_idx')})
        y = m(dev(x)).cpu().numpy()
        assert rel_err(y, oracle_forward(x, L)) < TOL


def test_split_k_64_with_positive_sums():
    """with 128 slices the 2^49 biases of the former fixed-point combine carried into the arrival count.  The cap is 64
    now; all-positive partial sums at the cap (and a request above it) must still find their owner."""
    K, N = 16384, 256
    L = make_random_layer(4, 128, K, N, seed=3)
    L['qzeros'][:] = 0                                                  # zero point 1: every (q - z) >= -1
    x = np.abs(np.random.default_rng(4).standard_normal((1, K))).astype(np.float16)
    lib = _native.lib()
    for sk in (64, 128):
        lib.gptq_set_split_k(sk)
        try:
            y1, _ = check_forward(x, L, family='gemv')
            y2, _ = check_forward(x, L, family='gemv')
            assert np.array_equal(y1.view(np.uint16), y2.view(np.uint16))
        finally:
            lib.gptq_set_split_k(-1)


def test_fused_mlp_rowwave_large_partials_are_not_clamped():
    """the gate/up split-K combine used to clamp every per-slice partial to +-512.  Scales 50x the usual
    range put the partial sums far beyond that; the result must still match the oracle (rowwave path forced by bits = 8)."""
    K, N = 2048, 512
    A, B = make_random_layer(8, 128, K, N, seed=51), make_random_layer(8, 128, K, N, seed=52)
    A['scales'] = (A['scales'].astype(np.float32) * 16).astype(np.float16)     # gate partials of a K slice: sigma ~ 220, total ~ 630
    B['scales'] = (B['scales'].astype(np.float32) * 0.1).astype(np.float16)    # keeps silu(gate) * up inside fp16
    x = (np.random.default_rng(6).standard_normal((1, K)) * 2).astype(np.float16)
    gate = tuple(dev(A[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    up = tuple(dev(B[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    lib = _native.lib()
    lib.gptq_set_split_k(8)
    try:
        c = quant.fused_mlp.fused_gate_up(dev(x), gate, up, 8, 128, family='abi').cpu().numpy()
    finally:
        lib.gptq_set_split_k(-1)
    ga = oracle.matmul248_exact(x, A['qweight'], A['scales'], A['qzeros'], A['g_idx'], 8)
    assert np.abs(ga).max() > 1500                                       # sums (and many slice partials) beyond the old +-512 range
    ref = oracle.fused_mlp(x, (A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), 8)
    ok = np.isfinite(ref.astype(np.float32))
    assert rel_err(np.where(ok, c, 0), np.where(ok, ref, 0)) < TOL


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [-1, 100, 101])
@pytest.mark.parametrize('M', [2, 3, 4, 5, 8])
@pytest.mark.parametrize('gs,K,N', [(128, 4096, 4096), (128, 1024, 2816), (64, 512, 288), (-1, 256, 1024), (32, 256, 512)])
def test_small_batch_rowwave(gs, K, N, M, variant):
    """2 <= M <= 4 (8 with the forced two-block MFMA variant) at 4 bits: all rows in ONE rowwave launch -- default choice,
    dot2 kernel (100), MFMA 4x4x4 kernel (101) -- plain and fused gate/up, bias, strided x rows; split-K words are [M][N] and must be back to zero."""
    if variant != 101 and M > 4:
        pytest.skip('M > 4 is served by the stream kernel unless the two-block MFMA variant is forced')
    prev = _native.lib().gptq_set_gemv_variant(variant)
    try:
        _small_batch_body(gs, K, N, M, plain_family=(variant == -1))
    finally:
        _native.lib().gptq_set_gemv_variant(prev)


def _small_batch_body(gs, K, N, M, plain_family):
    import torch
    L = make_random_layer(4, gs, K, N, seed=M + K)
    U = make_random_layer(4, gs, K, N, seed=M + K + 1)
    rng = np.random.default_rng(M * K + N)
    x = (rng.standard_normal((M, K)) * 0.5).astype(np.float16)
    bias = rng.standard_normal(N).astype(np.float16)
    yb = hip_forward(x, L, bias=bias, family='abi')                         # the C-ABI dispatch (rowwave / stream kernels): the Python
    assert rel_err(yb, exact_forward(x, L, bias)) < TOL                     # default would take the stripe16 image; bias = two roundings: float64 bar
    if plain_family:
        check_forward(x, L, family='gemv')
    # strided rows
    wide = torch.zeros((M, K + 64), dtype=torch.float16, device='cuda:0')
    wide[:, :K] = torch.from_numpy(x).cuda()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')
    y = QL.matmul248(wide[:, :K], dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), dev(L['g_idx']), 4, 15, family='abi')
    assert rel_err(y.cpu().numpy(), oracle_forward(x, L)) < TOL
    gate = tuple(dev(L[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    up = tuple(dev(U[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    c = quant.fused_mlp.fused_gate_up(dev(x), gate, up, 4, gs if gs != -1 else K, family='abi')
    ref = oracle.fused_mlp(x, (L['qweight'], L['scales'], L['qzeros'], L['g_idx']), (U['qweight'], U['scales'], U['qzeros'], U['g_idx']), 4)
    assert rel_err(c.cpu().numpy(), ref) < TOL
    ws = _native.workspace(torch.device('cuda:0'))
    torch.cuda.synchronize()
    assert int(ws[:4 * 12288 * 8].view(torch.int64).ne(0).sum()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize('bits,gs,M,K,N', [(4, 128, 700, 1024, 768), (8, 64, 300, 512, 288), (4, 64, 3300, 256, 4096)])
def test_fused_mlp_prefill_in_place_epilogue(bits, gs, M, K, N):
    """M > 64 through gptq_fused_mlp_f16: two MFMA-tile GEMMs, the second writes silu(gate) * up over gate in its
    epilogue (ragged M / N tiles; the last case also goes that way from Python: enough tiles to fill the GPU)."""
    import torch
    A = make_random_layer(bits, gs, K, N, seed=M)
    B = make_random_layer(bits, gs, K, N, seed=M + 1)
    x = (np.random.default_rng(M).standard_normal((M, K)) * 0.5).astype(np.float16)
    ref = oracle.fused_mlp(x, (A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), bits)
    dx = dev(x)
    a = [dev(A[k]) for k in ('qweight', 'scales', 'qzeros')]
    b = [dev(B[k]) for k in ('qweight', 'scales', 'qzeros')]
    c = torch.full((M, N), float('nan'), dtype=torch.float16, device='cuda:0')
    ws = _native.workspace(torch.device('cuda:0'))
    rc = _native.lib().gptq_fused_mlp_f16(dx.data_ptr(), K, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), None, b[0].data_ptr(), b[1].data_ptr(),
                                          b[2].data_ptr(), None, c.data_ptr(), N, M, K, N, bits, gs, ws.data_ptr(), ws.numel(),
                                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert rel_err(c.cpu().numpy(), ref) < TOL       # PAIR mode of the tile GEMM: SiLU on the fp32 sums (round 3; was two launches with a rounded gate)
    gate = tuple(dev(A[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    up = tuple(dev(B[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    c2 = quant.fused_mlp.fused_gate_up(dx, gate, up, bits, gs)
    assert rel_err(c2.cpu().numpy(), ref) < TOL


@pytest.mark.gpu
@pytest.mark.parametrize('gs,K,N', [(128, 4096, 11008), (64, 1024, 2816), (32, 512, 288)])
def test_act_order_fused_mlp_sorted(gs, K, N):
    """act-order gate/up at decode: one shared permutation (same input => same Hessian diagonal), two group-sorted
    weight copies, the trivial-g_idx fused kernel; against the fused oracle on the checkpoint layout.  A pair with
    DIFFERENT permutations must still be right (generic kernel)."""
    from util import act_order_g_idx
    rng = np.random.default_rng(K + N)
    A = make_random_layer(4, gs, K, N, act_order=True, seed=5)
    B = make_random_layer(4, gs, K, N, act_order=True, seed=6)
    B_same = dict(B)
    B_same['g_idx'] = A['g_idx'].copy()                       # what a real checkpoint has
    x = (rng.standard_normal((1, K)) * 0.5).astype(np.float16)
    for up_layer in (B_same, B):
        gate = tuple(dev(A[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
        up = tuple(dev(up_layer[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
        c = quant.fused_mlp.fused_gate_up(dev(x), gate, up, 4, gs)
        ref = oracle.fused_mlp(x, (A['qweight'], A['scales'], A['qzeros'], A['g_idx']),
                               (up_layer['qweight'], up_layer['scales'], up_layer['qzeros'], up_layer['g_idx']), 4)
        assert rel_err(c.cpu().numpy(), ref) < TOL


@pytest.mark.gpu
@pytest.mark.parametrize('gs,K,N', [(-1, 4096, 11008), (128, 1024, 2816), (64, 256, 288)])
def test_3bit_fused_mlp_rowwave(gs, K, N):
    """3-bit gate/up + SiLU at decode through the 3-bit rowwave kernel (both weight sets in one launch), BASELINE
    config 4 (3-bit no-group) for the MLP; M = 1 and 2."""
    A = make_random_layer(3, gs, K, N, seed=K)
    B = make_random_layer(3, gs, K, N, seed=K + 1)
    gate = tuple(dev(A[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    up = tuple(dev(B[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx'))
    for M in (1, 2):
        x = (np.random.default_rng(M + K).standard_normal((M, K)) * 0.5).astype(np.float16)
        c = quant.fused_mlp.fused_gate_up(dev(x), gate, up, 3, K if gs == -1 else gs)
        ref = oracle.fused_mlp(x, (A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), 3)
        assert rel_err(c.cpu().numpy(), ref) < TOL


# ---------------------------------------------------------------------------------------
# BASELINE config 5 with REAL kernels and a REAL collective on the one GPU of the test box: two processes share cuda:0
# and all-reduce their fp32 partials through gloo (RCCL refuses two ranks on one device; on an 8-GPU node the same
# module runs on "nccl" = RCCL over xGMI)
# ---------------------------------------------------------------------------------------
def _tp_gpu_worker(rank, world, port, ret):
    import os
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from quant import tensor_parallel as tp
        torch.cuda.set_device(0)
        ok = True
        for K, N, M, act in [(8192, 512, 1, False), (2816 * 2, 256, 1, False), (1024 + 128, 256, 3, False), (2048, 288, 1, True)]:
            L = make_random_layer(4, 128, K, N, act_order=act, seed=K + N)
            bias = np.random.default_rng(1).standard_normal(N).astype(np.float16)
            layer = quant.QuantLinear(4, 128, K, N, True)
            layer.qweight, layer.qzeros, layer.scales, layer.g_idx, layer.bias = (dev(L['qweight']), dev(L['qzeros']), dev(L['scales']),
                                                                                  dev(L['g_idx']), dev(bias))
            xh = np.random.default_rng(2).standard_normal((M, K)).astype(np.float16)
            row = tp.RowShardedQuantLinear(layer)
            y = row(dev(xh)).cpu().numpy()
            ref = oracle.matmul248(xh, L['qweight'], L['scales'], L['qzeros'], L['g_idx'], 4, bias=bias)
            ex = oracle.matmul248_exact(xh, L['qweight'], L['scales'], L['qzeros'], L['g_idx'], 4)
            ok = ok and rel_err(y, ex + bias.astype(np.float64)) < TOL              # bias: two fp16 roundings -> float64 bar, see exact_forward
            y0 = row.forward(dev(xh)) - dev(bias)
            ok = ok and rel_err(y0.cpu().numpy(), ex) < 2 * TOL                       # (y - bias: a THIRD rounding, not an op of the product)
        t = torch.tensor([1 if ok else 0])
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        if rank == 0:
            ret.put(int(t.item()))
    finally:
        dist.destroy_process_group()


def test_row_sharded_linear_two_processes_one_gpu():
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    ret = ctx.Queue()
    procs = [ctx.Process(target=_tp_gpu_worker, args=(r, 2, port, ret)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    assert ret.get(timeout=5) == 1


# ---------------------------------------------------------------------------------------
# one-shot all-reduce over HIP IPC peer mappings (csrc/p2p.hip): two processes on cuda:0 map each other's exchange buffer
# and reduce through it -- the same code path as two GPUs over xGMI (system-scope stores / flags), minus the link
# ---------------------------------------------------------------------------------------
def _p2p_worker(rank, world, port, ret):
    import os
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from quant import tensor_parallel as tp
        from quant.p2p import P2PAllReduce
        torch.cuda.set_device(0)
        ar = P2PAllReduce(2 * 22016)
        ok = True
        # raw all-reduce: exact fp32 sums in rank order, odd sizes, many calls back to back (slot parity), bias, fp32 output
        for it, n in enumerate([4096, 16384, 4, 2052, 11008, 8192, 8192, 8192]):
            parts = [np.random.default_rng(100 * it + r).standard_normal(n).astype(np.float32) for r in range(world)]
            want = parts[0].copy()
            for r in range(1, world):
                want = want + parts[r]
            bias = np.random.default_rng(it).standard_normal(n).astype(np.float16) if it % 2 else None
            y = ar.allreduce(dev(parts[rank]), bias=None if bias is None else dev(bias)).cpu().numpy()
            w16 = want.astype(np.float16)
            if bias is not None:
                w16 = (w16.astype(np.float32) + bias.astype(np.float32)).astype(np.float16)
            ok = ok and np.array_equal(y, w16)
            y32 = ar.allreduce(dev(parts[rank]), out=torch.empty(n, dtype=torch.float32, device='cuda')).cpu().numpy()
            ok = ok and np.array_equal(y32, want)
        # gate | up partials -> silu(sum gate) * sum up, rounded once (fused_mlp.py:160-166 after the reduce)
        for n in (11008, 22016, 64):
            parts = [np.random.default_rng(7 * n + r).standard_normal((2, n)).astype(np.float32) for r in range(world)]
            tot = parts[0].copy()
            for r in range(1, world):
                tot = tot + parts[r]
            y = ar.allreduce_silu_mul(dev(parts[rank])).cpu().numpy()
            want = (tot[0].astype(np.float64) / (1 + np.exp(-tot[0].astype(np.float64))) * tot[1]).astype(np.float32)
            ok = ok and y.shape == (1, n) and rel_err(y, want[None]) < TOL
        # a burst without host synchronisation in between (a rank may run one call ahead of its peer)
        outs = []
        for it in range(32):
            outs.append(ar.allreduce(torch.full((4096,), float(it + rank), dtype=torch.float32, device='cuda')))
        torch.cuda.synchronize()
        for it, o in enumerate(outs):
            ok = ok and bool((o == float(world * it + world * (world - 1) // 2)).all())     # sum over ranks of (it + rank)
        # the module: K-sharded QuantLinear, one launch for partial + one for the exchange
        for K, N, act in [(8192, 512, False), (2048, 288, True)]:
            L = make_random_layer(4, 128, K, N, act_order=act, seed=K + N)
            bias = np.random.default_rng(1).standard_normal(N).astype(np.float16)
            layer = quant.QuantLinear(4, 128, K, N, True)
            layer.qweight, layer.qzeros, layer.scales, layer.g_idx, layer.bias = (dev(L['qweight']), dev(L['qzeros']), dev(L['scales']),
                                                                                  dev(L['g_idx']), dev(bias))
            xh = np.random.default_rng(2).standard_normal((1, K)).astype(np.float16)
            row = tp.RowShardedQuantLinear(layer, p2p=ar)
            y = row(dev(xh)).cpu().numpy()
            y_rccl = tp.RowShardedQuantLinear(layer)(dev(xh)).cpu().numpy()       # gloo all-reduce of the same partials
            ref = oracle.matmul248(xh, L['qweight'], L['scales'], L['qzeros'], L['g_idx'], 4, bias=bias)
            # two ranks: any order gives the same fp32 sum; four: gloo's reduction order is its own, the exchange sums in rank order
            ex = oracle.matmul248_exact(xh, L['qweight'], L['scales'], L['qzeros'], L['g_idx'], 4) + bias.astype(np.float64)   # bias: two roundings -> float64 bar
            ok = ok and rel_err(y, ex) < TOL and (np.array_equal(y, y_rccl) if world == 2 else rel_err(y, y_rccl) < TOL)
        # hipGraph replay: the epoch is device state, so a captured exchange can be replayed
        part = torch.zeros(4096, dtype=torch.float32, device='cuda')
        out = torch.empty(4096, dtype=torch.float16, device='cuda')
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ar.allreduce(part, out=out)
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                ar.allreduce(part, out=out)
        torch.cuda.synchronize()
        for it in range(5):
            part.fill_(float(it * (rank + 1)))
            g.replay()
            torch.cuda.synchronize()
            ok = ok and bool((out == float(it * world * (world + 1) // 2)).all())           # sum over ranks of it * (rank + 1)
        ok = ok and ar.status() == 0
        t = torch.tensor([1 if ok else 0])
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        ar.close()
        if rank == 0:
            ret.put(int(t.item()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 4, 8])      # 8: the world the driver's scaling tier ends at
def test_p2p_allreduce_two_processes_one_gpu(world):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    ret = ctx.Queue()
    procs = [ctx.Process(target=_p2p_worker, args=(r, world, port, ret)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        if p.exitcode is None:
            p.kill()
        assert p.exitcode == 0
    assert ret.get(timeout=5) == 1


@pytest.mark.parametrize('bits,gs,K,N,act,pair', [(4, 128, 4096, 4096, False, False), (4, 128, 1024, 512, True, False), (4, 128, 4096, 11008, False, True),
                                                 (4, 128, 1024, 288, True, True), (8, 64, 1024, 96, False, False), (3, -1, 512, 320, False, False),
                                                 (2, 128, 1024, 64, True, False), (4, 32, 416, 288, False, False), (3, 128, 1024, 288, True, False),
                                                 (3, 64, 512, 320, True, True)])
def test_prepared_layer_abi_direct(bits, gs, K, N, act, pair):
    """the product's ONE call site used the way a non-Python consumer uses it: gptq_layer_inspect ->
    gptq_layer_image_bytes -> gptq_layer_prepare -> gptq_layer_forward for M = 1 .. 300 with nothing but raw pointers; act-order layers
    (group-sorted image + permutation inside the handle), the gate/up pair, shapes without an image; against the oracle on the original
    buffers.  Then memory mode: release_checkpoint, free the buffers, same answers; unpack_checkpoint reproduces them bit for bit."""
    import ctypes
    lib = _native.lib()
    A = make_random_layer(bits, gs, K, N, act_order=act, seed=K + N)
    B = make_random_layer(bits, gs, K, N, act_order=act, seed=K + N + 1)
    if act:
        B['g_idx'] = A['g_idx']
    gsz = K if gs == -1 else gs
    a = [dev(A[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx')]
    b = [dev(B[k]) for k in ('qweight', 'scales', 'qzeros', 'g_idx')] if pair else [None] * 4
    bias = None if pair else np.random.default_rng(5).standard_normal(N).astype(np.float16)
    dbias = None if bias is None else dev(bias)
    s = torch.cuda.current_stream().cuda_stream
    kind = lib.gptq_layer_inspect(a[3].data_ptr(), K, gsz, s)
    assert kind == (1 if act else 0)
    nbytes = lib.gptq_layer_image_bytes(K, N, bits, gsz, 2 if pair else 1, kind)
    image = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV)
    h = ctypes.c_void_p()
    p = _native.ptr
    rc = lib.gptq_layer_prepare(ctypes.byref(h), a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), p(dbias), p(b[0]), p(b[1]), p(b[2]), p(b[3]),
                                K, N, bits, gsz, image.data_ptr() if nbytes else None, nbytes, s)
    assert rc == 0 and lib.gptq_layer_kind(h) == kind
    ws = torch.zeros(lib.gptq_layer_workspace_bytes(), dtype=torch.uint8, device=DEV)
    rng = np.random.default_rng(K)

    def run(M):
        x = (rng.standard_normal((M, K)) * 0.5).astype(np.float16)
        dx, y = dev(x), torch.full((M, N), float('nan'), dtype=torch.float16, device=DEV)
        need = lib.gptq_layer_scratch_bytes(h, M)
        scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=DEV)
        rc = lib.gptq_layer_forward(h, dx.data_ptr(), K, y.data_ptr(), N, M, ws.data_ptr(), ws.numel(), scratch.data_ptr() if need else None, need, s)
        assert rc == 0, (M, rc)
        torch.cuda.synchronize()
        return x, y.cpu().numpy()

    def check(M):
        x, y = run(M)
        ta = (A['qweight'], A['scales'], A['qzeros'], A['g_idx'])
        if pair:
            ref = oracle.fused_mlp(x, ta, (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), bits)
            assert rel_err(y, ref) < TOL, (M, rel_err(y, ref))
        else:
            assert rel_err(y, exact_forward(x, A, bias)) < TOL, M          # bias: two roundings -> float64 bar
        return y
    ys = {M: check(M) for M in (1, 3, 8, 17, 64, 100, 300)}
    if nbytes:       # trivial AND (round 4) regular act-order layers -- the image of the group-sorted rows + both permutations --, 3-bit included: a bijection
        assert lib.gptq_layer_release_checkpoint(h) == 0
        keep = [t.clone() for t in a[:3]]
        for t in a[:3] + (b[:3] if pair else []):
            t.fill_(0)                                                       # the "freed" buffers must never be read again
        rng = np.random.default_rng(K)
        for M in (1, 3, 8, 17, 64, 100, 300):
            _, y = run(M)
            assert np.array_equal(y.view(np.uint16), ys[M].view(np.uint16)), M
        qw, sc, qz = torch.empty_like(keep[0]), torch.empty_like(keep[1]), torch.empty_like(keep[2])
        assert lib.gptq_layer_unpack_checkpoint(h, 0, qw.data_ptr(), sc.data_ptr(), qz.data_ptr(), s) == 0
        torch.cuda.synchronize()
        assert torch.equal(qw, keep[0]) and torch.equal(sc, keep[1]) and torch.equal(qz, keep[2])
        if pair:
            keep_b = [dev(B[k]) for k in ('qweight', 'scales', 'qzeros')]
            assert lib.gptq_layer_unpack_checkpoint(h, 1, qw.data_ptr(), sc.data_ptr(), qz.data_ptr(), s) == 0
            torch.cuda.synchronize()
            assert torch.equal(qw, keep_b[0]) and torch.equal(sc, keep_b[1]) and torch.equal(qz, keep_b[2])
    else:
        assert lib.gptq_layer_release_checkpoint(h) == -6 or not nbytes
    lib.gptq_layer_destroy(h)


# ---------------------------------------------------------------------------------------
# BASELINE config 4 and config 3 AT THE SIZES bench.py TIMES (VERDICT r3 missing #3 / next #5): 3-bit without groups and 4-bit act-order on
# every LLaMA-7B shape at M = 1; M = 32 x 2048 = 65 536 rows on 4096 x 4096 against the oracle on sampled rows.
# ---------------------------------------------------------------------------------------
LLAMA7B_SHAPES = [(4096, 4096), (4096, 11008), (11008, 4096), (4096, 12288)]


@pytest.mark.parametrize('K,N', LLAMA7B_SHAPES)
@pytest.mark.parametrize('variant', ['w3_nogroup', 'w4_g128_act_order', 'w3_g128_act_order'])
def test_config4_full_size_batch1(K, N, variant):
    """3-bit is the layout EXTENSION (the reference raises NotImplementedError, quant_linear.py:308-309: parity unpinned by construction,
    checked against the oracle's own 3-bit restatement AND the float64 product); act-order g_idx as gptq.py:210-216 produces it."""
    bits, gs, act = {'w3_nogroup': (3, -1, False), 'w4_g128_act_order': (4, 128, True), 'w3_g128_act_order': (3, 128, True)}[variant]
    L = make_random_layer(bits, gs, K, N, act_order=act, seed=K + N + bits)
    x = np.random.default_rng(K + bits).standard_normal((1, K)).astype(np.float16)
    y, ref = check_forward(x, L)
    ye = oracle.matmul248_exact(x, L['qweight'], L['scales'], L['qzeros'], L['g_idx'], bits)
    assert rel_err(y, ye) < TOL, rel_err(y, ye)
    assert_not_worse_than_reference(y, ref, ye, name='%s %dx%d' % (variant, K, N))
    y2 = hip_forward(x, L)
    assert np.array_equal(y.view(np.uint16), y2.view(np.uint16))       # no atomics on these routes: bit-reproducible


@pytest.mark.parametrize('K,N', [(4096, 4096), (4096, 11008), (11008, 4096)])
def test_prefill_config3_65536_rows_vs_oracle_on_sampled_rows(K, N):
    """BASELINE config 3 as benchmarked: batch 32 x seq 2048 = 65 536 rows, 4-bit g128, through the product's call site
    (gptq_layer_forward -> the prefill tile GEMM); 100+ rows spread over every 1024-row band + the tile edges against the CPU oracle.
    Round 6: the MLP shapes of LLaMA-7B next to 4096 x 4096 (a ragged last column tile at N = 11008, the long K of down_proj)."""
    M = 65536
    L = make_random_layer(4, 128, K, N, seed=65536 + N)
    g = torch.Generator(device=DEV)
    g.manual_seed(65536)
    x = torch.randn((M, K), device=DEV, generator=g, dtype=torch.float16)
    y = QL.matmul248(x, dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), dev(L['g_idx']), 4, 15)
    torch.cuda.synchronize()
    assert y.shape == (M, N)
    rng = np.random.default_rng(3)
    rows = np.unique(np.concatenate([np.arange(0, M, 1024), rng.integers(0, M, 40), [255, 256, 257, 32767, 32768, M - 257, M - 256, M - 1]]))
    idx = torch.from_numpy(rows).to(DEV)
    ref = oracle_forward(x[idx].cpu().numpy(), L)
    got = y[idx].cpu().numpy()
    assert np.isfinite(got.astype(np.float32)).all()
    assert rel_err(got, ref) < TOL, rel_err(got, ref)
    # size-independent property at the full size: every sampled row equals the M = 1 decode kernel's answer for that row
    for m in rows[::16]:
        ym = QL.matmul248(x[int(m):int(m) + 1], dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), dev(L['g_idx']), 4, 15).cpu().numpy()
        assert rel_err(y[int(m):int(m) + 1].cpu().numpy(), ym) < TOL


@pytest.mark.parametrize('M', [1, 2, 3, 4])
@pytest.mark.parametrize('K,N', [(8192, 4096), (22016, 1024)])
def test_row_shards_of_eight_ranks_sum_within_the_bar(M, K, N):
    """BASELINE config 5 numerics at world 8 on one GPU: the eight K-shards of a LLaMA-65B-shaped layer (22016 = 172 groups -> 22,22,22,22,
    21,21,21,21) computed one after the other through the module path's partial function, summed in fp32, rounded once -- against the
    unsharded oracle at the op-level bar.  Batches of 2..4 rows leave in fp32 too (gptq_stripe_matmul_partial_f32), so the sharded sum
    keeps the unsharded layer's single rounding."""
    from quant import tensor_parallel as tp
    L = make_random_layer(4, 128, K, N, seed=K + M)
    x = np.random.default_rng(M).standard_normal((M, K)).astype(np.float16)
    layer = quant.QuantLinear(4, 128, K, N, False)
    layer.qweight, layer.scales, layer.qzeros, layer.g_idx = dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), dev(L['g_idx'])
    xd = dev(x)
    total = torch.zeros((M, N), dtype=torch.float32, device=DEV)
    for rank in range(8):
        shard, (k0, k1) = tp.shard_rows(layer, rank, 8, trivial_g_idx=True)
        shard.bias = None
        part = tp._default_partial(xd[:, k0:k1], shard)
        assert part.dtype == torch.float32 and part.shape == (M, N)
        total += part
    y = total.half().cpu().numpy()
    ref = oracle_forward(x, L)
    assert rel_err(y, ref) < TOL, rel_err(y, ref)
    full = hip_forward(x, L)
    assert rel_err(y, full) < TOL


@pytest.mark.parametrize('nsets', [1, 2])
@pytest.mark.parametrize('M', [2, 4])
def test_stripe_matmul_partial_f32_matches_the_fp16_kernel_before_rounding(M, nsets):
    """gptq_stripe_matmul_partial_f32: fp32 sums [M][nsets][N] of up to four rows; rounding them (and applying SiLU * up for a pair)
    reproduces gptq_stripe_matvec_f16 bit for bit."""
    K, N = 4096, 512
    A = make_random_layer(4, 128, K, N, seed=5)
    B = make_random_layer(4, 128, K, N, seed=6)
    x = dev(np.random.default_rng(M).standard_normal((M, K)).astype(np.float16))
    st = QL.stripe_copy(dev(A['qweight']), dev(A['scales']), dev(A['qzeros']), 4, 128,
                        up=(dev(B['qweight']), dev(B['scales']), dev(B['qzeros'])) if nsets == 2 else None)
    lib = _native.lib()
    part = torch.empty((M, nsets, N), dtype=torch.float32, device=DEV)
    y = torch.empty((M, N), dtype=torch.float16, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    _native.check(lib.gptq_stripe_matmul_partial_f32(x.data_ptr(), K, st.data_ptr(), st.numel(), part.data_ptr(), M, K, N, 4, 128, nsets, s), 'partial')
    _native.check(lib.gptq_stripe_matvec_f16(x.data_ptr(), K, st.data_ptr(), st.numel(), None, y.data_ptr(), N, M, K, N, 4, 128, nsets, None, 0.0, None, s), 'f16')
    torch.cuda.synchronize()
    if nsets == 1:
        want = part[:, 0].half()
    else:
        want = (torch.nn.functional.silu(part[:, 0]) * part[:, 1]).half()
        assert rel_err(want.cpu().numpy(), y.cpu().numpy()) < TOL       # (__expf vs torch's exp: not bit-identical)
        return
    assert torch.equal(want, y)
    assert lib.gptq_stripe_matmul_partial_f32(x.data_ptr(), K, st.data_ptr(), st.numel(), part.data_ptr(), 5, K, N, 4, 128, nsets, s) == -6


# ---------------------------------------------------------------------------------------
# the LM head of a decode step: dense fp16 matvec (csrc/dense_gemv.hip) against a float64 product of the same fp16 operands
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,K', [(32000, 4096), (32001, 4096), (1000, 11008), (50, 256), (3, 8)])
@pytest.mark.parametrize('norm', [False, True])
def test_dense_matvec_lm_head(N, K, norm):
    rng = np.random.default_rng(N + K)
    W = (rng.standard_normal((N, K)) * 0.02).astype(np.float16)
    x = rng.standard_normal((1, K)).astype(np.float16)
    nw = (1 + 0.1 * rng.standard_normal(K)).astype(np.float16)
    bias = rng.standard_normal(N).astype(np.float16) if N == 50 else None
    lib = _native.lib()
    Wd, xd, nd = dev(W), dev(x), dev(nw)
    y = torch.empty((1, N), dtype=torch.float16, device=DEV)
    rc = lib.gptq_dense_matvec_f16(xd.data_ptr(), Wd.data_ptr(), K, _native.ptr(None if bias is None else dev(bias)), y.data_ptr(), N, K,
                                   nd.data_ptr() if norm else None, 1e-6, torch.cuda.current_stream().cuda_stream)
    _native.check(rc, 'gptq_dense_matvec_f16')
    torch.cuda.synchronize()
    xe = oracle.rmsnorm(x, nw, 1e-6) if norm else x          # the reference norm's own fp16-rounded output (triton_norm.py:22-39)
    exact = xe.astype(np.float64) @ W.astype(np.float64).T
    if bias is not None:
        exact = exact.astype(np.float16).astype(np.float64) + bias.astype(np.float64)
    assert rel_err(y.cpu().numpy(), exact) < TOL, rel_err(y.cpu().numpy(), exact)
    y2 = torch.empty_like(y)
    lib.gptq_dense_matvec_f16(xd.data_ptr(), Wd.data_ptr(), K, _native.ptr(None if bias is None else dev(bias)), y2.data_ptr(), N, K,
                              nd.data_ptr() if norm else None, 1e-6, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(y, y2)                                # no atomics: bit-reproducible


def test_dense_matvec_rejects_bad_arguments():
    lib = _native.lib()
    a = torch.zeros(64, dtype=torch.float16, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    assert lib.gptq_dense_matvec_f16(None, a.data_ptr(), 8, None, a.data_ptr(), 4, 8, None, 0.0, s) == -4        # GPTQ_E_NULL
    assert lib.gptq_dense_matvec_f16(a.data_ptr(), a.data_ptr(), 8, None, a.data_ptr(), 4, 12, None, 0.0, s) != 0  # K % 8
    assert lib.gptq_dense_matvec_f16(a.data_ptr(), a.data_ptr(), 4, None, a.data_ptr(), 4, 8, None, 0.0, s) != 0   # ldw < K


# ---------------------------------------------------------------------------------------
# round 4: several stripes per workgroup on the same staged x (stripe_mm3_kernel C = 2 / 3: 5 .. 32 rows on shapes with 2-3 rounds of stripes)
# and K slices of the 128-row fused tile GEMM (65 .. 128 rows on multi-round / long-K shapes) -- against the oracle on sampled rows
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('bits', [3, 4, 8])
@pytest.mark.parametrize('K,N', [(4096, 12288), (4096, 11008), (4096, 8192), (11008, 4096), (4096, 8224)])
@pytest.mark.parametrize('M', [5, 16, 17, 32, 33, 48, 49, 64, 65, 96, 100, 128])
def test_small_batches_on_multi_round_shapes(bits, K, N, M):
    """every schedule of gptq_stripe_matmul_f16 that round 4 added or re-routed: C adjacent stripes per workgroup (N = 8192: 2, 11008 / 12288: 3;
    8224 = 514 stripes = 171 x 3 + 1: a ragged last workgroup), the four-wave instances at 33 .. 64 rows (.. 96 on N = 8192), the sliced tile GEMM from 65
    rows on elsewhere; bias in the epilogue; bit-reproducible"""
    if bits == 8 and K == 11008:
        pytest.skip('8-bit row block = 64 k: covered by the 4096-k shapes')
    L = make_random_layer(bits, 128, K, N, seed=bits * 1000 + N + M)
    rng = np.random.default_rng(M + K)
    x = rng.standard_normal((M, K)).astype(np.float16)
    b = rng.standard_normal(N).astype(np.float16)
    xd, out = dev(x), torch.empty((M, N), dtype=torch.float16, device=DEV)
    st = QL.stripe_copy(dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), bits, 128)
    assert st is not None
    assert QL.stripe_matmul(xd, st, out, K, N, bits, 128, bias=dev(b))
    torch.cuda.synchronize()
    y = out.cpu().numpy()
    rows = np.unique(np.concatenate([[0, M - 1, M // 2], rng.integers(0, M, 5)]))
    ref = exact_forward(x[rows], L, b)
    assert np.isfinite(y.astype(np.float32)).all()
    assert rel_err(y[rows], ref) < TOL, rel_err(y[rows], ref)
    out2 = torch.empty_like(out)
    assert QL.stripe_matmul(xd, st, out2, K, N, bits, 128, bias=dev(b))
    torch.cuda.synchronize()
    assert torch.equal(out, out2)                              # partial tiles are summed in slice order: no atomics anywhere
    # every row agrees with the M = 1 decode kernel on the same image (size-independent property; catches a wrong row / column map at once)
    one = torch.empty((1, N), dtype=torch.float16, device=DEV)
    for m in (0, M - 1):
        assert QL.stripe_matvec(xd[m:m + 1], st, one, K, N, bits, 128, bias=dev(b))
        # two independently rounded fp16 results (bias: two roundings each): ONE fp16 spacing at the top of the range is already 1e-3 of max|y|
        assert rel_err(y[m:m + 1], one.cpu().numpy()) < 2 * TOL


@pytest.mark.parametrize('bits,gs,K,N,pair', [(4, 128, 4096, 4096, False), (4, 128, 1024, 2816, True), (8, 64, 1024, 288, False), (3, 128, 1152, 320, False),
                                             (2, 128, 1024, 96, False)])
def test_released_layer_prefill_straight_from_the_image(bits, gs, K, N, pair):
    """round 5: memory mode at prompt sizes.  A released layer used to rebuild the checkpoint layout per call and dequantise
    THAT; now its W^T comes out of the stripe16 image in one pass (stripe_dequant_t_kernel) -- the SAME fp16 weight, so the product of the
    tile GEMM is bit-identical to the two-copy route's, for every width, the gate/up pair included; the scratch request shrinks by the
    rebuilt buffers; against the oracle as well."""
    lib = _native.lib()
    A = make_random_layer(bits, gs, K, N, seed=K + N + bits)
    B = make_random_layer(bits, gs, K, N, seed=K + N + bits + 1)
    sets = tuple((dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), dev(L['g_idx'])) for L in ((A, B) if pair else (A,)))
    from quant.layer import PreparedLayer
    pl = PreparedLayer(sets, None, bits, gs, K, N)
    M = 2600                                          # above the fused tile GEMM on the image (2048 rows): the dense route
    x = dev((np.random.default_rng(5).standard_normal((M, K)) * 0.5).astype(np.float16))
    y0 = torch.empty((M, N), dtype=torch.float16, device=DEV)
    pl.forward(x, y0)
    need0 = lib.gptq_layer_scratch_bytes(pl.handle, M)
    assert pl.release()
    need1 = lib.gptq_layer_scratch_bytes(pl.handle, M)
    if K % 128 == 0:
        assert need1 == need0                         # nothing is rebuilt: the dense workspace alone
    assert lib.gptq_layer_fallback_scratch_bytes(pl.handle, M) > need1
    for t in sets:
        for u in t[:3]:
            u.fill_(0)                                # the "freed" buffers must never be read again
    y1 = torch.full((M, N), float('nan'), dtype=torch.float16, device=DEV)
    pl.forward(x, y1)
    torch.cuda.synchronize()
    assert torch.equal(y0, y1)
    xs = x[:64].cpu().numpy()
    ta = (A['qweight'], A['scales'], A['qzeros'], A['g_idx'])
    ref = oracle.fused_mlp(xs, ta, (B['qweight'], B['scales'], B['qzeros'], B['g_idx']), bits) if pair else oracle.matmul248(xs, *ta, bits)
    assert rel_err(y1[:64].cpu().numpy(), ref) < (2 * TOL if pair else TOL)


@pytest.mark.parametrize('pair', [False, True])
def test_long_prompts_on_wide_layers_take_the_dense_route(pair):
    """Round 5: gptq_layer_forward keeps a batch of 129 .. 2048 rows on the fused image GEMM only while its 128 x 128 tiles fit the chip at once
    (at most 512) or the batch is too short to pay for a dequantise pass (640 rows; the gate | up pair: 1152) -- above, dequantise + the tile
    GEMM of gemm8.hip (capi.hip image_gemm_wanted; measured in profiles/r5e_gemm8_tile/).  The host-side table says so, both routes meet the
    oracle, a released layer takes its W^T straight from the image (same bits), and a caller who brings NO scratch stays on the image."""
    lib = _native.lib()
    bits, gs, K, N = 4, 128, 512, 8192
    M = 1300 if pair else 1100                            # 11 / 9 row tiles x 128 (pair) / 64 column groups: more than 512 tiles
    A = make_random_layer(bits, gs, K, N, seed=31)
    B = make_random_layer(bits, gs, K, N, seed=32)
    sets = tuple((dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), dev(L['g_idx'])) for L in ((A, B) if pair else (A,)))
    from quant.layer import PreparedLayer
    pl = PreparedLayer(sets, None, bits, gs, K, N)
    assert lib.gptq_layer_route_for(pl.handle, M) == 4 and lib.gptq_layer_route_for(pl.handle, 600) == 3        # DENSE_TILE_GEMM / STRIPE_GEMM
    assert lib.gptq_layer_scratch_bytes(pl.handle, M) >= K * N * 2 * len(sets) and lib.gptq_layer_scratch_bytes(pl.handle, 600) == 0
    x = dev((np.random.default_rng(6).standard_normal((M, K)) * 0.5).astype(np.float16))
    y_dense = torch.full((M, N), float('nan'), dtype=torch.float16, device=DEV)
    pl.forward(x, y_dense)
    # no scratch: the same call stays on the image (exact q - z and fp32 group scales: other roundings, same tolerance)
    s = _native.stream_ptr(torch.device(DEV))
    ws = _native.layer_workspace(torch.device(DEV), s)
    y_image = torch.full((M, N), float('nan'), dtype=torch.float16, device=DEV)
    _native.check(lib.gptq_layer_forward(pl.handle, x.data_ptr(), x.stride(0), y_image.data_ptr(), y_image.stride(0), M, ws.data_ptr(), ws.numel(), None, 0, s),
                  'gptq_layer_forward')
    torch.cuda.synchronize()
    rows = np.unique(np.concatenate([np.arange(0, M, 97), [127, 128, M - 1]]))
    ta, tb = (A['qweight'], A['scales'], A['qzeros'], A['g_idx']), (B['qweight'], B['scales'], B['qzeros'], B['g_idx'])
    xs = x.cpu().numpy()[rows]
    ref = oracle.fused_mlp(xs, ta, tb, bits) if pair else oracle.matmul248(xs, *ta, bits)
    for y in (y_dense, y_image):
        assert rel_err(y.cpu().numpy()[rows], ref) < (2 * TOL if pair else TOL)
    assert not torch.equal(y_dense, y_image)              # (two different kernels did run)
    assert pl.release()
    y_rel = torch.full((M, N), float('nan'), dtype=torch.float16, device=DEV)
    pl.forward(x, y_rel)
    torch.cuda.synchronize()
    assert torch.equal(y_rel, y_dense)


def test_released_layer_retries_with_the_fallback_scratch():
    """gptq_layer_scratch_bytes answers for the route the table picks; when that kernel declines at launch -- here the fused tile
    GEMM on the image refuses an x whose rows are 2^23 halves apart (its buffer descriptor ends at 2 GB) -- a released layer's fall-back
    needs the rebuilt checkpoint layout + the dense workspace.  PreparedLayer.forward retries once with gptq_layer_fallback_scratch_bytes
    instead of raising GPTQ_E_WORKSPACE."""
    K, N, bits, gs = 1024, 512, 4, 128
    L = make_random_layer(bits, gs, K, N, seed=77)
    from quant.layer import PreparedLayer
    pl = PreparedLayer(((dev(L['qweight']), dev(L['scales']), dev(L['qzeros']), dev(L['g_idx'])),), None, bits, gs, K, N)
    assert pl.release()
    M, ld = 200, 1 << 23
    big = torch.zeros(M * ld, dtype=torch.float16, device=DEV)
    xv = torch.as_strided(big, (M, K), (ld, 1))
    xs = (np.random.default_rng(9).standard_normal((M, K)) * 0.5).astype(np.float16)
    xv.copy_(dev(xs))
    y = torch.empty((M, N), dtype=torch.float16, device=DEV)
    pl.forward(xv, y)
    torch.cuda.synchronize()
    assert rel_err(y.cpu().numpy(), oracle_forward(xs, L)) < TOL
