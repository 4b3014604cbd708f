"""The launch plan of the checkpoint-layout kernels, pinned on the CPU (no GPU needed).

gptq_gemv_plan_for_shape (include/gptq_mi355x.h) walks the dispatch code of gptq_matmul248_f16 / gptq_fused_mlp_f16 / gptq_gemv_f16 /
gptq_skinny_f16 and the direct rowwave entries up to the first dispatch call and reports that call's kernel family and plan: rows of the
pass, U / nl / stage units, K slices, waves, x in LDS, log2(units per group), tiles, chunks per slice.  A changed split moves a result by
less than any test tolerance, so no GPU test would see it; this table does.

How tests/golden/gemv_plans.json was made: the commit before the query existed was built with one line added at the top of the six
dispatch functions (gemv_fast_dispatch, gemv_rowwave_mr_dispatch, gemv_rowwave_mfma_dispatch, gemv_generic_dispatch, skinny_dispatch,
gemm_dispatch) that records the kernel's template arguments and the plan fields of GemvParams of the FIRST call, and the C ABI entries
were called on a machine without a GPU with pointers into a host buffer: such a call gets through validation and planning and fails
at its first launch.  The recorded first call -- or the GPTQ_E_* code returned before any -- is the fixture; the fields a family does
not set (they are uninitialised in GemvParams there) are stored as 0.  The grid was 254 441 calls: bits 2/3/4/8, M 0..257, seven
(K, N) up to N = 131 104, groupsize 32/128/K/96, single set and pair, with and without g_idx, the norm and x-permutation entries, four
workspace sizes, every forced variant and split below; it is thinned here to one case per distinct planner outcome per entry, flag set,
bit width, forced value and workspace class, plus every M, every shape x groupsize and every K split that occurs (1 550 cases).  The
same recording on the library that has the query agreed with the query on all 254 441 calls."""
import ctypes
import json
import os

import pytest

from quant import _native

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gemv_plans.json')
FIELDS = 8                                           # GPTQ_PLAN_FIELDS
PART_OFFSET = 65536 * 8 + 4096                       # SPLITK_PART_OFFSET (csrc/gptq_internal.h)


@pytest.fixture(scope='module')
def table():
    doc = json.load(open(GOLDEN))
    assert doc['columns'][:12] == ['entry', 'M', 'K', 'N', 'bits', 'groupsize', 'nsets', 'flags', 'workspace_bytes', 'gemv_variant', 'split_k', 'result']
    return [tuple(c) for c in doc['cases']]


def _query(lib, case):
    entry, M, K, N, bits, gs, nsets, flags, ws, fv, fs = case[:11]
    lib.gptq_set_gemv_variant(fv)
    lib.gptq_set_split_k(fs)
    plan = (ctypes.c_int * FIELDS)(*([-77] * FIELDS))
    rc = lib.gptq_gemv_plan_for_shape(entry, M, K, N, bits, gs, nsets, flags, ws, plan)
    return (rc,) + tuple(plan)


def test_gemv_plan_equals_the_recorded_first_dispatch(table):
    lib = _native.lib()
    bad = []
    try:
        for case in table:
            got = _query(lib, case)
            if got != case[11:]:
                bad.append((case[:11], case[11:], got))
    finally:
        lib.gptq_set_gemv_variant(-1)
        lib.gptq_set_split_k(-1)
    assert not bad, '%d of %d plans differ from the record; first (inputs, recorded, query): %r' % (len(bad), len(table), bad[:5])


def test_gemv_plan_fixture_reaches_every_branch(table):
    """the thinned grid still holds what the planners branch on"""
    col = lambda i: {c[i] for c in table}
    ws_bytes = _native.lib().gptq_query(3)
    assert col(4) == {2, 3, 4, 5, 7, 8} and col(0) == {0, 1, 2, 3} and col(6) == {1, 2} and col(7) == {0, 1, 2, 3, 4, 6}
    assert col(1) >= {0, 1, 2, 3, 4, 5, 8, 9, 16, 32, 33, 64, 65, 128, 256, 257}
    assert {(c[2], c[3]) for c in table} >= {(64, 64), (256, 256), (512, 256), (4096, 4096), (4096, 12288), (11008, 4096), (256, 131104)}
    assert col(5) >= {32, 96, 128, 4096, 11008}
    assert col(8) == {0, PART_OFFSET + 1, PART_OFFSET + 65536, ws_bytes}
    assert col(9) >= {-1, 0, 1, 2, 3, 100, 101} and col(10) == {-1, 1, 4, 64}
    assert col(11) == {-6, -5, -2, -1, 0, 1, 2, 3, 4, 5, 6}                      # every kernel family, every code the planners return
    stream = [c for c in table if c[11] == 5]
    assert {c[13] for c in stream} == {1, 2, 4} and {c[15] for c in stream} == {2, 4, 8} and {c[16] for c in stream} == {0, 1}
    assert {c[13] for c in table if c[11] == 1} == {1, 2, 4, 8} and {c[13] for c in table if c[11] == 4} == {4, 16}
    assert {c[14] for c in table if c[11] in (1, 2, 3)} >= {1, 2, 4, 64}           # no split, shrunk to the workspace, forced, the cap


def test_gemv_plan_query_validation():
    lib = _native.lib()
    plan = (ctypes.c_int * FIELDS)()
    ws = lib.gptq_query(3)
    assert lib.gptq_gemv_plan_for_shape(0, 1, 4096, 4096, 4, 128, 1, 0, ws, None) == -4          # GPTQ_E_NULL
    assert lib.gptq_gemv_plan_for_shape(4, 1, 4096, 4096, 4, 128, 1, 0, ws, plan) == -6          # unknown entry
    assert lib.gptq_gemv_plan_for_shape(0, 1, 4096, 4096, 4, 128, 1, 8, ws, plan) == -6          # unknown flag
    assert lib.gptq_gemv_plan_for_shape(0, 1, 4096, 4096, 4, 128, 1, 2, ws, plan) == -6          # the norm belongs to the direct rowwave entries
    assert lib.gptq_gemv_plan_for_shape(0, 1, 4096, 4096, 4, 128, 3, 0, ws, plan) == -2          # nsets
    assert lib.gptq_gemv_plan_for_shape(3, 2, 4096, 4096, 4, 128, 1, 2, ws, plan) == -2          # the norm entries have one row
    # the decode product of a LLaMA-7B layer, spelled out: rowwave, one row, U = 8, 16 K slices, 16 packed rows per group
    assert lib.gptq_gemv_plan_for_shape(0, 1, 4096, 4096, 4, 128, 1, 0, ws, plan) == 1 and list(plan) == [1, 8, 16, 0, 0, 4, 0, 0]
