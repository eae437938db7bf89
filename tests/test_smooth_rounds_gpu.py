"""GPU: the block inverses of `mdq_smooth_fast` at the block counts where the rounds of their construction change.

Eleven waves of the workgroup build one block inverse each per round (eleven packed triangles fit the position buffers).
Structured rectangles of 32 x nb interior vertices for nb = 11 (one round), 12 and 13 (a second round of one and two), 22
(two full rounds), 23, 24 and 25 (a third round): 3 sweeps against the careful walk `mdq_smooth`, within 1e-13.  (Building
with all twelve waves - 24 blocks in two rounds - was measured and taken out again: HISTORY, "Gathers at the block's width".)"""
import numpy as np
import pytest

import smooth_gather_cases as sgc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results(lib_built):
    batch = [sgc.rectangle(nb, 32, 90 + nb) for nb in sgc.ROUNDS_BLOCKS]
    fast, st, nv = sgc.smooth(batch, 3, True)
    walk, _, _ = sgc.smooth(batch, 3, False)
    again, st2, _ = sgc.smooth(batch, 3, True)
    assert np.array_equal(fast, again) and np.array_equal(st, st2)
    return batch, fast, walk, st, nv


@pytest.mark.parametrize("k", range(len(sgc.ROUNDS_BLOCKS)))
def test_block_inverses_by_all_waves(results, k):
    batch, fast, walk, st, nv = results
    nb = sgc.ROUNDS_BLOCKS[k]
    assert nv[k] == (nb + 2) * 34 and nv[k] < 1024
    assert len(sgc.row_slots(batch[k][1], int(nv[k]))) == 32 * nb
    err = np.abs(fast[k, :nv[k]] - walk[k, :nv[k]]).max()
    moved = np.abs(fast[k, :nv[k]] - batch[k][0]).max()
    print(f"{nb} blocks, 3 sweeps: against the walk {err:.2e} (moved {moved:.2e}), stats {st[k]}")
    assert err < 1e-13, (nb, err)
    assert moved > 1e-4, nb
    assert st[k, 0] == 0, (nb, st[k])                       # in the blocked solve, nothing handed back
