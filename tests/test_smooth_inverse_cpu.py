"""CPU: the fp64 restatement of the block-inverse recurrence that tests/test_smooth_inverse_gpu.py holds the device to, and
the share of rows without in-block lower neighbours on the lab meshes - the premise of walking only the other rows.

The restatement (`smooth_inverse_cases.reference_inverses`) is checked against the definition: M_B = (I - D^-1 L_BB)^-1 D^-1
by a dense solve, per block of 32 interior ranks.  The shares are counted by the rule of the set-up (a lower neighbour is
an interior neighbour with a smaller vertex index whose rank lies in the same block) on ys930 and ah93w145 as loaded and
on ys930 after 20 and 42 scripted removals (tests/pressure_width_cases.py)."""
import numpy as np
import pytest

import smooth_gather_cases as sgc
import smooth_inverse_cases as sic
from pressure_width_cases import case_mesh

# mesh -> (interior rows, rows with 0, 1, 2, 3 in-block lower neighbours)
LOWER = {
    "ys930": (694, [422, 111, 157, 4]),
    "ys930-hub20": (674, [402, 125, 144, 3]),
    "ys930-hub42": (652, [401, 116, 133, 2]),
    "ah93w145": (634, [374, 118, 138, 4]),
}


def _dense(cells, nv):
    rows = sic.block_rows(cells, nv)
    nblk = (len(rows) + sic.BS - 1) // sic.BS
    rows += [(1, [])] * (nblk * sic.BS - len(rows))
    out = np.zeros((nblk, sic.BS, sic.BS))
    for b in range(nblk):
        k = np.array([rows[b * sic.BS + i][0] for i in range(sic.BS)], np.float64)
        L = np.zeros((sic.BS, sic.BS))
        for i in range(sic.BS):
            L[i, rows[b * sic.BS + i][1]] = 1.0
        out[b] = np.linalg.inv(np.eye(sic.BS) - L / k[:, None]) / k[None, :]
    return out


@pytest.mark.parametrize("name", [n for n, _, _ in sic.small_cases()])
def test_restatement_is_the_block_inverse(name):
    c, t = {n: (c, t) for n, c, t in sic.small_cases()}[name]
    ref, dense = sic.reference_inverses(t, len(c)), _dense(t, len(c))
    assert ref.shape == dense.shape
    assert (np.triu(ref, 1) == 0.0).all() and (ref >= 0.0).all()
    np.testing.assert_allclose(ref, dense, rtol=1e-13, atol=1e-15)


def test_workspace_layout_round_trip():
    rng = np.random.default_rng(3)
    M = rng.uniform(size=(3, sic.BS, sic.BS))
    flat = M.reshape(3, sic.BS, 2, 8, 2).transpose(0, 2, 3, 1, 4).ravel()      # [block][half][t][row][2]
    assert np.array_equal(sic.unpack_workspace(flat, 3), M)
    assert flat[((1 * 2 + 1) * 8 + 3) * 64 + 5 * 2 + 1] == M[1, 5, 16 + 2 * 3 + 1]


@pytest.mark.parametrize("name", list(LOWER))
def test_most_rows_have_no_in_block_lower_neighbour(lib_built, meshes, name):
    c, t, _ = case_mesh(meshes, name)
    low = sic.lower_counts(np.sort(t, axis=1).astype(np.int32), len(c))
    rows, hist = LOWER[name]
    print(f"{name}: {rows} interior rows, in-block lower neighbours {np.bincount(low).tolist()}, mean {low.mean():.2f}")
    assert len(low) == rows and np.bincount(low).tolist() == hist
    assert hist[0] > 0.55 * rows and low.max() <= sic.MAXLOW


def test_restatement_on_ys930(meshes):
    c, t = meshes["ys930"]
    t = np.sort(np.asarray(t), axis=1).astype(np.int32)
    np.testing.assert_allclose(sic.reference_inverses(t, len(c)), _dense(t, len(c)), rtol=1e-13, atol=1e-15)
    assert int(sgc.interior_mask(t, len(c)).sum()) == 694
