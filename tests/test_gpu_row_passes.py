"""GPU test of the pass the token-choice kernels share (csrc/sample_common.h row_top: the row's largest key, its first index, the first NaN /
+inf) through its three consumers -- gptq_sample_rows_f16, gptq_beam_select_f16, gptq_logprobs_rows_f16 -- on ONE 2-byte-aligned row of 41
elements at an odd element offset: the smallest row whose walk has a head (ids 0 .. 6), 16-byte vectors (7 .. 38) and a tail (39, 40).  The
expectation is plain numpy."""
import numpy as np
import pytest
import torch

import beam_ref as B
from quant import _native

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
V = 41
NAN, INF = float('nan'), float('inf')
REC_WORDS = 4 + 4 * 16                    # a row's record of the beam state block: {max, log sum, bad, -, 2 x 16 x (id, bits)}

#        name                 (index, value) edits of the finite base row
CASES = [('finite', []),
         ('nan-head', [(3, NAN)]), ('inf-head', [(6, INF)]),
         ('nan-body', [(20, NAN)]), ('inf-body', [(7, INF)]),
         ('nan-tail', [(40, NAN)]), ('inf-tail', [(39, INF)]),
         ('two-bad-body-before-tail', [(39, NAN), (9, INF)]),          # the first one wins, whichever kind and whichever thread holds it
         ('two-bad-head-before-body', [(33, INF), (4, NAN)]),
         ('two-bad-one-vector', [(14, INF), (12, NAN)]),
         ('minus-inf-only', [(i, -INF) for i in range(V)]),
         ('equal-maxima-head-body', [(5, 9.0), (22, 9.0)]),            # the lower id wins
         ('equal-maxima-body-tail', [(40, 9.0), (30, 9.0)])]


def _row(edits):
    row = (np.random.default_rng(41).standard_normal(V) * 2).astype(np.float16)
    for i, v in edits:
        row[i] = v
    return row


def _odd(rows):
    """the rows in a buffer whose rows are 2-byte aligned only: element offset 1, an odd leading dimension, NaN around them"""
    n = len(rows)
    ld = V + 2
    buf = torch.full((n * ld + 1,), NAN, dtype=torch.float16, device=DEV)
    view = buf[1:].view(n, ld)[:, :V]
    view.copy_(torch.from_numpy(np.stack(rows)))
    assert view.data_ptr() % 16 == 2 and view.stride(0) % 2 == 1
    return view


def _expect(row):
    """(the first NaN / +inf or None, the first maximum, whether the row has no distribution)"""
    nonfinite = np.isnan(row) | (row == np.float16(INF))
    bad = int(np.argmax(nonfinite)) if nonfinite.any() else None
    r64 = np.where(np.isnan(row), -INF, row.astype(np.float64))
    return bad, int(np.argmax(r64)), bad is not None or bool((r64 == -INF).all())


@pytest.mark.parametrize('name,edits', CASES, ids=[c[0] for c in CASES])
def test_pass_one_through_its_three_consumers(name, edits):
    lib, s = _native.lib(), _native.stream_ptr(torch.device(DEV))
    row = _row(edits)
    plain = _row([])
    bad, argmax, dead = _expect(row)
    view = _odd([row, row, plain])

    # sampling: the first non-finite index, else the first maximum under a greedy setting; a sampled setting gives the same on a row without mass
    out = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    u, T = torch.tensor([0.5, 0.5], device=DEV), torch.tensor([0.0, 1.0], device=DEV)
    k, p = torch.zeros(2, dtype=torch.int32, device=DEV), torch.ones(2, device=DEV)
    rc = lib.gptq_sample_rows_f16(view.data_ptr(), view.stride(0), 2, V, u.data_ptr(), T.data_ptr(), k.data_ptr(), p.data_ptr(), out.data_ptr(), s)
    assert rc == 0, rc
    ids = out.tolist()
    want = bad if bad is not None else argmax
    assert ids[0] == want, (ids, want)
    if dead:
        assert ids[1] == want, (ids, want)
    else:
        assert 0 <= ids[1] < V and np.isfinite(row[ids[1]])

    # beam select, rows 1 and 2 of the view: the row's record is marked bad exactly when it has no distribution, the plain row's never
    st = B.State(2, 50, t_cap=64)
    st.t, st.score = 3, np.array([-0.5, -0.75])
    w = torch.from_numpy(B.pack(st)).to(DEV)
    rc = lib.gptq_beam_select_f16(view[1:].data_ptr(), view.stride(0), 2, V, w.data_ptr(), s)
    assert rc == 0, rc
    words = w.cpu().numpy()
    assert [int(words[B.W_REC + b * REC_WORDS + 2]) for b in range(2)] == [int(dead), 0]
    assert (int(words[B.W_STATUS]) & 1) == int(dead)
    got = B.unpack(words)
    assert all(0 <= c[2] < V for c in got['cand'])
    if not dead:                                               # the row's first candidate is its first maximum
        assert [c[2] for c in got['cand'] if c[1] == 0][0] == argmax

    # log-probabilities: NaN and rank -1 exactly when the row has no distribution; else the rank numpy counts
    chosen_ids = [argmax, V - 1, 0]
    cid = torch.tensor(chosen_ids, dtype=torch.int64, device=DEV)
    chosen, rank = torch.empty(3, dtype=torch.float32, device=DEV), torch.empty(3, dtype=torch.int32, device=DEV)
    top_ids, top_lp = torch.empty((3, 2), dtype=torch.int32, device=DEV), torch.empty((3, 2), dtype=torch.float32, device=DEV)
    rc = lib.gptq_logprobs_rows_f16(view.data_ptr(), view.stride(0), 3, V, cid.data_ptr(), 2, None, 1, chosen.data_ptr(), rank.data_ptr(),
                                    top_ids.data_ptr(), top_lp.data_ptr(), s)
    assert rc == 0, rc
    chosen, rank, top_ids, top_lp = chosen.cpu().numpy(), rank.cpu().numpy(), top_ids.cpu().numpy(), top_lp.cpu().numpy()
    for r, (x, c) in enumerate(zip((row, row, plain), chosen_ids)):
        if r < 2 and dead:
            assert np.isnan(chosen[r]) and rank[r] == -1 and np.isnan(top_lp[r]).all() and top_ids[r].tolist() == [0, 1], r
        else:
            x64 = x.astype(np.float64)
            assert not np.isnan(chosen[r]) and not np.isnan(top_lp[r]).any(), r
            assert rank[r] == int((x64 > x64[c]).sum() + (x64[:c] == x64[c]).sum()), r
            assert top_ids[r, 0] == int(np.argmax(x64)), r
