"""The meshes of the block-inverse tests, the recurrence of the set-up on the host, and the child process that runs every case
once (`python tests/smooth_inverse_cases.py OUT.npz`).

The set-up of `smooth_linear_kernel` cuts the interior ranks into blocks of 32 and builds, per block,
    T = (I - D^-1 L)^-1,  row i:  T[i] = e_i + (1 / k_i) sum of T[w] over the in-block lower neighbours w of row i,
    M = T D^-1            (lower triangular; k = number of neighbours, L = adjacency towards lower-numbered vertices whose rank is
                           in the same block),
and leaves M in the launch's workspace as [block][half][t][row][2]: column 16 half + 2 t + e of row `row`.  A row without
in-block lower neighbours is e_i; by default only the other rows go through the serial row loop, and
`MDQ_SMOOTH_SETUP_PARENT=3` (read once per process) selects the loop over all 32 rows and the neighbour lists by look-up:
the parent's code.  Both sides of the comparison come from child processes that run ALL the cases.

Meshes: the rectangles of tests/smooth_gather_cases.py with 1, 31, 32, 33 and 65 interior vertices; a strip of quads with
a centre vertex each (40 interior vertices none of which has an interior neighbour: empty masks); the strip of 1 x 97
interior vertices numbered along itself (every row but a block's first has its left neighbour: full masks); a wheel whose hub
has 8 interior neighbours, all numbered below it (MAXLOW); ys930 after 0 and 42 scripted removals."""
import os
import sys

import numpy as np

import smooth_gather_cases as sgc

BS, MBLK, MAXLOW = 32, 1024, 8
RECT = (1, 31, 32, 33, 65)
SMALL_SWEEPS = (1, 3)
YS_REMOVALS = (0, 42)
YS_SWEEPS = 3
H = sgc.H


def centred_quads(n, seed):
    """A strip of n unit quads, each cut into four cells by a centre vertex: the centres are the interior vertices and all
    their neighbours lie on the boundary."""
    bottom = [[i * H, 0.0] for i in range(n + 1)]
    top = [[i * H, H] for i in range(n + 1)]
    cen = np.array([[(i + 0.5) * H, 0.5 * H] for i in range(n)])
    cen += np.random.default_rng(seed).uniform(-0.15 * H, 0.15 * H, cen.shape)
    coords = np.array(bottom + top + cen.tolist())
    cells = []
    for i in range(n):
        b0, b1, t0, t1, c = i, i + 1, n + 1 + i, n + 2 + i, 2 * (n + 1) + i
        cells += [[b0, b1, c], [b1, t1, c], [t1, t0, c], [t0, b0, c]]
    cells = np.array(cells, np.int64)
    sgc.check_triangulation(coords, cells, n * H * H)
    return coords, np.sort(cells.astype(np.int32), axis=1)


def wheel(seed):
    """Two concentric octagons around a hub, the outer one (the boundary) numbered first, the hub last: the hub's eight
    neighbours are interior, lower-numbered and in its block."""
    ang = 2.0 * np.pi * np.arange(8) / 8.0
    outer = 2.0 * H * np.stack([np.cos(ang + np.pi / 8.0), np.sin(ang + np.pi / 8.0)], 1)      # 0..7: outer m between inner m and m + 1
    inner = H * np.stack([np.cos(ang), np.sin(ang)], 1)                                        # 8..15
    coords = np.concatenate([outer, inner, np.zeros((1, 2))])
    coords[8:] += np.random.default_rng(seed).uniform(-0.05 * H, 0.05 * H, (9, 2))
    cells = []
    for m in range(8):
        n = (m + 1) % 8
        cells += [[16, 8 + m, 8 + n], [8 + m, m, 8 + n], [8 + m, (m - 1) % 8, m]]
    cells = np.array(cells, np.int64)
    sgc.check_triangulation(coords, cells, 0.5 * sgc._area2(coords, cells).sum())
    return coords, np.sort(cells.astype(np.int32), axis=1)


def small_cases():
    out = [(f"rect{n}", *sgc.rectangle(*sgc.RECT[n], 40 + n)) for n in RECT]
    out.append(("quads40", *centred_quads(40, 5)))
    out.append(("strip97", *sgc.rectangle(*sgc.RECT[97], 137)))
    out.append(("wheel8", *wheel(11)))
    return out


def ys_cases():
    g = sgc.golden_meshes()
    return [(f"ys930-{k}", *sgc.ys930_displaced(g, k)) for k in YS_REMOVALS]


def block_rows(cells, nv):
    """Per interior rank, by the rule of the set-up: (number of neighbours, in-block lower neighbours as local row indices)."""
    inner = sgc.interior_mask(cells, nv)
    rank = np.full(nv, -1)
    rank[inner] = np.arange(int(inner.sum()))
    nb = sgc.neighbours(cells, nv)
    rows = []
    for v in np.flatnonzero(inner):
        r = rank[v]
        rows.append((len(nb[v]), sorted(int(rank[w]) % BS for w in nb[v] if rank[w] >= 0 and w < v and rank[w] // BS == r // BS)))
    return rows


def lower_counts(cells, nv):
    """In-block lower neighbours per interior rank."""
    return np.array([len(low) for _, low in block_rows(cells, nv)], np.int64)


def reference_inverses(cells, nv):
    """M of every block in fp64, (blocks, 32, 32): the recurrence as stated above, rows behind the last rank as the set-up
    pads them (one neighbour, no lower ones: the identity)."""
    rows = block_rows(cells, nv)
    nblk = (len(rows) + BS - 1) // BS
    rows += [(1, [])] * (nblk * BS - len(rows))
    M = np.zeros((nblk, BS, BS))
    for b in range(nblk):
        T = np.zeros((BS, BS))
        inv_k = np.array([1.0 / rows[b * BS + i][0] for i in range(BS)])
        for i in range(BS):
            acc = np.zeros(BS)
            for w in rows[b * BS + i][1]:
                acc += T[w]
            T[i] = acc * inv_k[i]
            T[i, i] += 1.0
        M[b] = T * inv_k[None, :]
    return M


def unpack_workspace(flat, nblk):
    """[block][half][t][row][2] -> (blocks, 32 rows, 32 columns)."""
    a = np.asarray(flat[:nblk * MBLK]).reshape(nblk, 2, 8, BS, 2)
    return a.transpose(0, 3, 1, 2, 4).reshape(nblk, BS, BS)


def _launch(batch, sweeps, env):
    """One launch of the batch -> (coords, diagnostics, per mesh the written part of the block-inverse workspace)."""
    import torch
    from meshdqn_amd import mesh_ops
    B, NV = len(batch), max(len(c) for c, _ in batch)
    mesh_ops._SMOOTH_WS.clear()                   # (a fresh workspace per launch: nothing of an earlier launch to be read back)
    coords, stats, _ = sgc.smooth(batch, sweeps, True, env=env)
    (ws,) = mesh_ops._SMOOTH_WS.values()
    torch.cuda.synchronize()
    mstride = ((NV + BS - 1) // BS + 2) * MBLK
    raw = ws[:B * mstride * 8].view(torch.float64).cpu().numpy().reshape(B, mstride)
    inv = []
    for b, (c, t) in enumerate(batch):
        n_int = int(sgc.interior_mask(t, len(c)).sum())
        inv.append(raw[b, :(n_int + BS - 1) // BS * MBLK].copy())
    return coords, stats, inv


def run_all(out_path):
    out = {}
    for g, cases, sweeps in (("small", small_cases(), SMALL_SWEEPS), ("ys930", ys_cases(), (YS_SWEEPS,))):
        batch = [(c, t) for _, c, t in cases]
        for s in sweeps:
            for tag, env in (("fast", False), ("env", True)):
                coords, stats, inv = _launch(batch, s, env)
                out[f"{g}/{s}/{tag}/coords"], out[f"{g}/{s}/{tag}/stats"] = coords, stats
                for (name, _, _), m in zip(cases, inv):
                    out[f"{g}/{s}/{tag}/inv/{name}"] = m
    np.savez(out_path, **out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    run_all(sys.argv[1])
