"""GPU test of gptq_beam_src_update_u8 (csrc/beam.hip): the ancestry table's rows gathered by the step's parents, in place, and the count of the
leading columns all rows share -- against src[parent] in numpy, with guard bytes around the table."""
import numpy as np
import pytest
import torch

from quant import _native

pytestmark = pytest.mark.gpu
DEV, T_MAX, GUARD = 'cuda:0', 1930, 64
PARENTS = dict(identity=lambda n: np.arange(n), swap=lambda n: np.r_[n - 1, np.arange(1, n - 1), 0],
               cycle=lambda n: np.r_[1, n - 1, np.arange(2, n - 1), 0] if n >= 3 else np.r_[1, 0],          # a 3-cycle, every other row in place
               one=lambda n: np.full(n, n - 1), random=lambda n: np.random.default_rng(n).integers(n, size=n))


@pytest.mark.parametrize('length', [0, 1, 33, T_MAX])
@pytest.mark.parametrize('kind', list(PARENTS))
@pytest.mark.parametrize('n', [2, 16])
def test_src_update(n, kind, length):
    src = np.random.default_rng(1000 * n + length).integers(n, size=(n, T_MAX)).astype(np.uint8)
    src[:, :length // 2] = src[0, :length // 2]                            # a shared trunk: half of the columns in play (then random ones)
    parent = PARENTS[kind](n).astype(np.int32)
    want = src.copy()
    want[:, :length] = src[parent][:, :length]
    same = (want[:, :length] == want[0, :length]).all(axis=0)
    common = length if same.all() else int(np.argmin(same))                # the LEADING uniform columns
    frame = np.full(GUARD, 0x5A, np.uint8)
    sd = torch.from_numpy(np.concatenate([frame, src.reshape(-1), frame])).to(DEV)
    pd, ld = torch.from_numpy(parent).to(DEV), torch.tensor([length], dtype=torch.int64, device=DEV)
    cd = torch.tensor([-7, 0x5A5A5A5A], dtype=torch.int32, device=DEV)
    rc = _native.lib().gptq_beam_src_update_u8(sd[GUARD:].data_ptr(), n, T_MAX, pd.data_ptr(), ld.data_ptr(), cd.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream)
    _native.check(rc, 'gptq_beam_src_update_u8')
    torch.cuda.synchronize()
    assert np.array_equal(sd.cpu().numpy(), np.concatenate([frame, want.reshape(-1), frame])), 'rows, columns at and past len, or guard bytes'
    assert cd.tolist() == [common, 0x5A5A5A5A] and pd.tolist() == parent.tolist() and ld.tolist() == [length]
    assert common >= length // 2 and (kind != 'one' or common == length)   # (the case has a trunk; all-to-one makes every column one)
