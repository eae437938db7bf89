"""The meshes of the smoothing-width tests, the width rule of the blocked solve on the host, and the child process that runs
every case once (`python tests/smooth_gather_cases.py OUT.npz`).

A block step of `smooth_linear_kernel` gathers, per row, the neighbours that are not lower-numbered members of the row's own
block of 32 interior ranks.  A block whose rows all have at most 8 such slots reads four per lane half, any other block all
seven; `MDQ_SMOOTH_GATHER=7` makes every block read seven (the parent's arithmetic).  The switch is read once per process,
so the two sides of a comparison come from two child processes, each of which runs ALL the cases and leaves them in one file.

Meshes: structured triangulated rectangles (interior degree 6: narrow blocks only), the strip of 1 x 97 interior vertices
with one vertex re-fanned into a hub of 8 + a + b cells (below), and ys930 after scripted removals with one vertex displaced."""
import os
import sys

import numpy as np

H = 0.05                                                    # grid spacing
RECT = {1: (1, 1), 31: (1, 31), 32: (4, 8), 33: (3, 11), 64: (8, 8), 65: (5, 13), 97: (1, 97)}   # interior count: rows x columns
RECT_SWEEPS = (1, 2, 3, 50)
# name -> (rank of the hub in the strip, a, b): the hub has 8 + a + b cells, and as many gather slots less one if its left
# neighbour (rank - 1) is in its block
HUBS = {
    "hub12-block0": (10, 2, 2),       # 11 slots
    "hub12-block1": (40, 2, 2),
    "hub12-last": (96, 0, 4),         # the only row of block 3; its left neighbour is in block 2: 12 slots
    "hub12-rank31": (31, 2, 2),       # the two sides of a block boundary: 11 slots in block 0 ...
    "hub12-rank32": (32, 2, 2),       # ... and 12 in block 1
    "hub-8slots": (40, 1, 0),         # 9 cells, 8 slots: the widest narrow row
    "hub-9slots": (40, 1, 1),         # 10 cells, 9 slots: the narrowest wide row
}
HUB_WIDE = {"hub12-block0": [0], "hub12-block1": [1], "hub12-last": [3], "hub12-rank31": [0], "hub12-rank32": [1],
            "hub-8slots": [], "hub-9slots": [1]}
HUB_SLOTS = {"hub12-block0": 11, "hub12-block1": 11, "hub12-last": 12, "hub12-rank31": 11, "hub12-rank32": 12,
             "hub-8slots": 8, "hub-9slots": 9}
HUB_SWEEPS = (3, 50)
YS_REMOVALS = (0, 20, 42)
ROUNDS_BLOCKS = (11, 12, 13, 22, 23, 24, 25)


def _grid(ny, nx):
    jj, ii = np.meshgrid(np.arange(ny + 2), np.arange(nx + 2), indexing="ij")
    coords = H * np.stack([ii.ravel(), jj.ravel()], 1).astype(np.float64)
    inner = ((ii > 0) & (ii < nx + 1) & (jj > 0) & (jj < ny + 1)).ravel()
    vid = lambda j, i: j * (nx + 2) + i   # noqa: E731
    cells = []
    for j in range(ny + 1):
        for i in range(nx + 1):
            cells += [[vid(j, i), vid(j, i + 1), vid(j + 1, i + 1)], [vid(j, i), vid(j + 1, i + 1), vid(j + 1, i)]]
    return coords, inner, np.array(cells, np.int64)


def rectangle(ny, nx, seed):
    """(ny + 2) x (nx + 2) vertices in row-major order, every quad cut along the same diagonal; the interior vertices
    jittered by up to 0.15 of the spacing (full steps to the centroid: far inside half the smallest altitude)."""
    coords, inner, cells = _grid(ny, nx)
    coords[inner] += np.random.default_rng(seed).uniform(-0.15 * H, 0.15 * H, (int(inner.sum()), 2))
    return coords, np.sort(cells.astype(np.int32), axis=1)


def _area2(p, t):
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    return (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])


def check_triangulation(coords, cells, area):
    """Counter-clockwise cells, every edge in one or two of them, and the areas add up: a valid triangulation of the domain."""
    a2 = _area2(coords, cells)
    assert (a2 > 0).all(), "inverted or degenerate cell"
    assert abs(0.5 * a2.sum() - area) < 1e-12 * max(area, 1.0), "the cells do not tile the domain"
    e = np.sort(np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [2, 0]]]), axis=1)
    _, cnt = np.unique(e, axis=0, return_counts=True)
    assert cnt.max() <= 2


def neighbours(cells, nv):
    nb = [set() for _ in range(nv)]
    for a, b, c in np.asarray(cells).tolist():
        nb[a] |= {b, c}
        nb[b] |= {a, c}
        nb[c] |= {a, b}
    return nb


def interior_mask(cells, nv):
    """The set-up's interior test: a vertex all of whose neighbours appear in exactly two of its cells."""
    e = np.sort(np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [0, 2]]]), axis=1)
    ue, cnt = np.unique(e, axis=0, return_counts=True)
    boundary = np.zeros(nv, bool)
    boundary[ue[cnt != 2].ravel()] = True
    used = np.zeros(nv, bool)
    used[np.asarray(cells).ravel()] = True
    return used & ~boundary


def row_slots(cells, nv):
    """Gather slots per interior rank, as the set-up of `smooth_linear_kernel` counts them: the neighbours of the rank's
    vertex that are not lower-numbered interior vertices of the same block of 32 ranks."""
    inner = interior_mask(cells, nv)
    rank = np.full(nv, -1)
    rank[inner] = np.arange(int(inner.sum()))
    nb = neighbours(cells, nv)
    ns = np.zeros(int(inner.sum()), np.int64)
    for v in np.flatnonzero(inner):
        r = rank[v]
        ns[r] = sum(1 for w in nb[v] if not (rank[w] >= 0 and w < v and rank[w] // 32 == r // 32))
    return ns


def wide_blocks(cells, nv):
    """The blocks that take the wide block step: some row has more than 8 gather slots."""
    ns = row_slots(cells, nv)
    return sorted({int(r) // 32 for r in np.flatnonzero(ns > 8)})


def strip_hub(rank, a, b, seed):
    """The strip of 1 x 97 interior vertices (3 x 99 vertices; interior rank r = column r + 1 of the middle row) with the
    interior vertex `rank` re-fanned into a hub of 8 + a + b cells: its ring is its two row neighbours, the top-row vertices
    of the columns i - 1 ... i + 1 + a and the bottom-row vertices of the columns i - 1 - b ... i + 1 (i = its column).  The
    row neighbours beyond it are fanned from the last top / bottom vertex of the ring, the rest of the strip stays.  The
    interior vertices sit at the Laplacian equilibrium of this topology (a valid mesh: convex boundary), jittered by up to
    0.02 of the spacing - every update of the first sweeps is a clear full step, so the block steps' results are the output
    (after about 11 sweeps the strip has converged to round-off and the updates fall under DOLFIN_EPS: repaired sweeps)."""
    nx, i = 97, rank + 1
    assert 1 <= i <= nx and i + 1 + a <= nx + 1 and i - 1 - b >= 0
    coords, inner, cells = _grid(1, nx)
    vid = lambda j, k: j * (nx + 2) + k   # noqa: E731
    v = vid(1, i)
    ring = ([vid(1, i + 1)] + [vid(2, k) for k in range(i + 1 + a, i - 2, -1)] + [vid(1, i - 1)] +
            [vid(0, k) for k in range(i - 1 - b, i + 2)])
    new = [[v, ring[m], ring[(m + 1) % len(ring)]] for m in range(len(ring))]
    new += [[vid(1, k), vid(1, k + 1), vid(2, i + 1 + a)] for k in range(i + 1, i + 1 + a)]
    new += [[vid(1, k), vid(1, k - 1), vid(0, i - 1 - b)] for k in range(i - 1, i - 1 - b, -1)]
    new = np.array(new, np.int64)
    assert len(ring) == 8 + a + b and (_area2(coords, new) > 0).all()
    # the cells of the strip that the new ones replace: those whose centroid lies in one of them
    cen = coords[cells].mean(axis=1)
    covered = np.zeros(len(cells), bool)
    for t in new:
        p = coords[t]
        d0 = (p[1, 0] - p[0, 0]) * (cen[:, 1] - p[0, 1]) - (p[1, 1] - p[0, 1]) * (cen[:, 0] - p[0, 0])
        d1 = (p[2, 0] - p[1, 0]) * (cen[:, 1] - p[1, 1]) - (p[2, 1] - p[1, 1]) * (cen[:, 0] - p[1, 0])
        d2 = (p[0, 0] - p[2, 0]) * (cen[:, 1] - p[2, 1]) - (p[0, 1] - p[2, 1]) * (cen[:, 0] - p[2, 0])
        covered |= (d0 > 0) & (d1 > 0) & (d2 > 0)
    cells = np.concatenate([cells[~covered], new])
    assert len(cells) == 2 * 2 * (nx + 1)
    check_triangulation(coords, cells, 2 * (nx + 1) * H * H)
    # Laplacian equilibrium of the interior vertices
    nv = len(coords)
    nb = neighbours(cells, nv)
    idx = np.flatnonzero(inner)
    pos = {int(u): n for n, u in enumerate(idx)}
    A, rhs = np.zeros((len(idx), len(idx))), np.zeros((len(idx), 2))
    for n, u in enumerate(idx):
        A[n, n] = len(nb[u])
        for w in nb[u]:
            if w in pos:
                A[n, pos[w]] -= 1.0
            else:
                rhs[n] += coords[w]
    coords[idx] = np.linalg.solve(A, rhs)
    coords[idx] += np.random.default_rng(seed).uniform(-0.02 * H, 0.02 * H, (len(idx), 2))
    check_triangulation(coords, cells, 2 * (nx + 1) * H * H)
    assert np.array_equal(interior_mask(cells, nv), inner) and len(nb[v]) == 8 + a + b
    return coords, np.sort(cells.astype(np.int32), axis=1)


def ys930_displaced(meshes, removals):
    """ys930 after `removals` scripted removals (tests/pressure_width_cases.py), one interior vertex moved 97 % of the way
    to a neighbour: its first sweeps take limited steps, so repair rounds run between the block steps."""
    from pressure_width_cases import case_mesh
    c, t, _ = case_mesh(meshes, {0: "ys930", 20: "ys930-hub20", 42: "ys930-hub42"}[removals])
    c, t = c.copy(), np.sort(t, axis=1).astype(np.int32)
    rng = np.random.default_rng(1370)
    v = int(rng.choice(np.flatnonzero(interior_mask(t, len(c)))))
    w = int([u for u in t[(t == v).any(axis=1)][0] if u != v][0])
    c[v] = c[v] + 0.97 * (c[w] - c[v])
    return c, t


def golden_meshes():
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = {}
    for name in ("ys930", "ah93w145"):
        z = np.load(os.path.join(g, f"{name}.npz"))
        out[name] = (z["coords"], z["cells"])
    return out


def groups():
    """name -> (list of (case, coords, cells), sweeps to run): the cases of a group run as one batch."""
    return {
        "rect": ([(str(n), *rectangle(ny, nx, 40 + n)) for n, (ny, nx) in RECT.items()], RECT_SWEEPS),
        "hub": ([(name, *strip_hub(r, a, b, 7 + r)) for name, (r, a, b) in HUBS.items()], HUB_SWEEPS),
        "ys930": ([(str(k), *ys930_displaced(golden_meshes(), k)) for k in YS_REMOVALS], (50,)),
    }


def smooth(batch, sweeps, fast, env=False):
    """`sweeps` sweeps of every mesh of `batch` in one launch -> (coords (B, NV, 2), diagnostics (B, 4) or None, nv):
    `mdq_smooth_fast` (or, `env`: `mdq_smooth_fast_env` with a successful removal everywhere), or the walk `mdq_smooth`."""
    import torch
    from meshdqn_amd.mesh_ops import smooth_batch_gpu, smooth_env_gpu, smooth_fast_stats
    B = len(batch)
    NV, NT = max(len(c) for c, _ in batch), max(len(t) for _, t in batch)
    coords, cells = np.zeros((B, NV, 2)), np.zeros((B, NT, 3), np.int32)
    nv, nt = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b, (c, t) in enumerate(batch):
        coords[b, :len(c)], cells[b, :len(t)], nv[b], nt[b] = c, t, len(c), len(t)
    dev = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    tc = dev(coords.copy())
    if env:
        smooth_env_gpu(tc, dev(cells), dev(nv), dev(nt), dev(np.zeros(B, np.int32)), dev(np.zeros(B, np.int32)), sweeps)
    else:
        smooth_batch_gpu(tc, dev(cells), dev(nv), dev(nt), dev(np.full(B, sweeps, np.int32)), fast=fast)
    torch.cuda.synchronize()
    return tc.cpu().numpy(), (smooth_fast_stats(tc.device, B, NV) if fast else None), nv


def run_all(out_path):
    """Every case with this process's setting of the switch: `<group>/<sweeps>/fast`, `/stats`, `/env` (the env-step entry
    point, largest sweep count only) and - the careful walk - `/walk`."""
    out = {}
    for g, (cases, sweeps) in groups().items():
        batch = [(c, t) for _, c, t in cases]
        for s in sweeps:
            out[f"{g}/{s}/fast"], out[f"{g}/{s}/stats"], out[f"{g}/nv"] = smooth(batch, s, True)
            out[f"{g}/{s}/walk"] = smooth(batch, s, False)[0]
        out[f"{g}/{sweeps[-1]}/env"], out[f"{g}/{sweeps[-1]}/envstats"], _ = smooth(batch, sweeps[-1], True, env=True)
        out[f"{g}/start"] = np.stack([np.pad(c, ((0, out[f"{g}/{sweeps[-1]}/fast"].shape[1] - len(c)), (0, 0))) for c, _ in batch])
    np.savez(out_path, **out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    run_all(sys.argv[1])
