"""GPU: the sweeps of `mdq_smooth_fast` at the block counts where their start and their end can go wrong.

Every sweep of the blocked solve starts from the copy of the block inverses 0 and 1 that the set-up leaves in LDS and streams
the others from the workspace through three register buffers, three block steps per loop trip.  Structured triangulated
rectangles with 1, 32, 33, 64, 65, 96 and 97 interior vertices give 1, 1, 2, 2, 3, 3 and 4 blocks of 32 rows: a mesh without a
block 1, full and one-row last blocks, every exit of the unrolled loop.  1, 2, 3 and 50 sweeps against `mdq_smooth` (the
per-vertex walk), and one ys930 mesh with displaced vertices, whose repair rounds sit between the pipelined sweeps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INTERIOR = {1: (1, 1), 32: (4, 8), 33: (3, 11), 64: (8, 8), 65: (5, 13), 96: (8, 12), 97: (1, 97)}   # count: rows x columns
SWEEPS = (1, 2, 3, 50)


def _rectangle(ny, nx, seed):
    """(ny + 2) x (nx + 2) vertices in row-major order, every quad cut along the same diagonal, spacing 0.05; the interior
    vertices jittered by up to 0.15 of the spacing (full steps to the centroid: far inside half the smallest altitude)."""
    rng = np.random.default_rng(seed)
    h = 0.05
    jj, ii = np.meshgrid(np.arange(ny + 2), np.arange(nx + 2), indexing="ij")
    coords = h * np.stack([ii.ravel(), jj.ravel()], 1).astype(np.float64)
    inner = ((ii > 0) & (ii < nx + 1) & (jj > 0) & (jj < ny + 1)).ravel()
    coords[inner] += rng.uniform(-0.15 * h, 0.15 * h, (int(inner.sum()), 2))
    vid = lambda j, i: j * (nx + 2) + i   # noqa: E731
    cells = []
    for j in range(ny + 1):
        for i in range(nx + 1):
            cells += [[vid(j, i), vid(j, i + 1), vid(j + 1, i + 1)], [vid(j, i), vid(j + 1, i + 1), vid(j + 1, i)]]
    assert int(inner.sum()) == ny * nx
    return coords, np.sort(np.array(cells, np.int32), axis=1)


def _smooth(batch, iters, fast):
    import torch
    from meshdqn_amd.mesh_ops import smooth_batch_gpu, smooth_fast_stats
    B = len(batch)
    NV, NT = max(len(c) for c, _ in batch), max(len(t) for _, t in batch)
    coords, cells = np.zeros((B, NV, 2)), np.zeros((B, NT, 3), np.int32)
    nv, nt = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b, (c, t) in enumerate(batch):
        coords[b, :len(c)], cells[b, :len(t)], nv[b], nt[b] = c, t, len(c), len(t)
    dev = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    tc = dev(coords.copy())
    smooth_batch_gpu(tc, dev(cells), dev(nv), dev(nt), dev(np.asarray(iters, np.int32)), fast=fast)
    torch.cuda.synchronize()
    return tc.cpu().numpy(), (smooth_fast_stats(tc.device, B, NV) if fast else None), nv


@pytest.fixture(scope="module")
def rectangles():
    return [_rectangle(ny, nx, 40 + n) for n, (ny, nx) in INTERIOR.items()]


@pytest.mark.parametrize("sweeps", SWEEPS)
def test_block_counts_one_to_four(lib_built, rectangles, sweeps):
    iters = [sweeps] * len(rectangles)
    walk, _, nv = _smooth(rectangles, iters, False)
    fast, st, _ = _smooth(rectangles, iters, True)
    again, st2, _ = _smooth(rectangles, iters, True)
    for b, n in enumerate(INTERIOR):
        err = np.abs(fast[b, :nv[b]] - walk[b, :nv[b]]).max()
        moved = np.abs(fast[b, :nv[b]] - rectangles[b][0]).max()
        print(f"{n} interior vertices ({(n + 31) // 32} blocks), {sweeps} sweeps: against the walk {err:.2e} (moved {moved:.2e}), stats {st[b]}")
        assert err < 1e-13, (n, sweeps, err)
        assert moved > 1e-4, (n, sweeps)               # (the sweeps did something)
        assert st[b, 0] == 0, (n, st)                   # in the blocked solve, nothing handed back
    assert np.array_equal(fast, again) and np.array_equal(st, st2)


def test_repair_rounds_between_the_sweeps(lib_built, meshes):
    """ys930 after three removals (the last one unsmoothed) with six interior vertices moved 97 % of the way to a
    neighbour, as in `test_fast_smoothing_rolls_back_sweeps_with_limited_steps`: checked sweeps with repair rounds and
    pipelined sweeps alternate.  Bound 1e-12, as there; bitwise reproducible."""
    from meshdqn_amd.topology import MeshTopology
    from test_env_gpu import _coarsened
    rng = np.random.default_rng(3)
    c, t = _coarsened(meshes, "ys930", 3, 7)
    interior = np.flatnonzero(~MeshTopology(c, t).on_boundary)
    for v in rng.choice(interior, 6, replace=False):
        cellsv = t[(t == v).any(axis=1)]
        w = int([u for u in cellsv[0] if u != v][0])
        c[v] = c[v] + 0.97 * (c[w] - c[v])
    walk, _, nv = _smooth([(c, t)], [50], False)
    fast, st, _ = _smooth([(c, t)], [50], True)
    again, st2, _ = _smooth([(c, t)], [50], True)
    err = np.abs(fast[0, :nv[0]] - walk[0, :nv[0]]).max()
    print(f"against the walk {err:.2e}; handed back / repaired sweeps / repair rounds / sent back: {st[0]}")
    assert err < 1e-12, err
    assert st[0, 0] == 0 and st[0, 1] >= 4, st         # repaired in the kernel, over several sweeps
    assert np.array_equal(fast, again) and np.array_equal(st, st2)
