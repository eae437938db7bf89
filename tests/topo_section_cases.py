"""The meshes of the topology-section test and the child process that runs the device engines on them
(`python tests/topo_section_cases.py OUT.npz`).

`topology_kernel<1>` keeps the hash position of a slot from its insert and runs its compactions at the width of their domain
with the flags in registers.  `MDQ_TOPO_INDEX_PARENT=15` (read once per process) selects the general code for both (and for
the two older switches): the parent's code.  Both sides of the comparison come from child processes
that run ALL the batches through
  `main`  - the env step's main engine (`ipcs=False`), which also hands its mesh and numbering over (`set_handover`),
  `full`  - one engine with the state outputs and the IPCS index data (`ipcs=True`),
  `hash`  - the flow stream's engine (`ipcs=True, flow_only=True`) on its own hash numbering,
  `given` - the same engine fed through the hand-over arrays of `main` (`take_edges_from`).

Meshes: structured channels on [-0.5, 3] x [-0.5, 0.5] with a rectangular hole, tuned by splitting wall edges and cells so
that the vertex, cell and edge counts land on both sides of the sizes at which the kernel changes its pass counts (CASES
below); one channel with a pinched boundary vertex; the hand-built channel of flow_index_cases.py; ys930 as loaded and
after 42 scripted removals, ah93w145.  One polygon for every batch: a rectangle of 12 points (what the distances are taken
to need not be the hole the mesh has)."""
import os
import sys

import numpy as np

import flow_index_cases as fic

ALL_BITS = "15"
# name -> (nx, ny, hole (i0, i1, j0, j1) in grid cells, split wall edges, split cells, pinch) and what it is there for.
# Counts (nv, nt, ne) are asserted by test_topo_sections_cpu.py.
CASES = {
    # SELL slices: 63 / 64 / 65 vertices = one slice short by one, full, and a second slice of one row
    "nv63": ((9, 7, (3, 6, 2, 4), 0, 2, None), dict(nv=63)),
    "nv64": ((9, 7, (3, 6, 2, 4), 0, 3, None), dict(nv=64)),
    "nv65": ((9, 7, (3, 6, 2, 4), 0, 4, None), dict(nv=65)),
    # two fans of cells and four boundary edges meet in one vertex (more incident edges than cells + 1)
    "pinch": ((10, 7, (2, 4, 2, 4), 0, 0, (6, 2)), dict()),
    # 3 nt on both sides of 1 024 slots (nt 341 / 342), ne on both sides of 1 024
    "nt341": ((21, 10, (5, 9, 3, 6), 1, 2, None), dict(nv=207, nt=341, ne=548)),
    "nt342": ((21, 10, (5, 9, 3, 6), 0, 3, None), dict(nv=207, nt=342, ne=549)),
    "ne1024": ((32, 12, (8, 14, 4, 8), 3, 5, None), dict(nv=377, nt=647, ne=1024)),
    "ne1025": ((30, 13, (7, 13, 4, 8), 1, 0, None), dict(nv=376, nt=649, ne=1025)),
    # 3 nt on both sides of 2 048 slots (nt 682 / 683)
    "nt682": ((31, 13, (7, 13, 4, 8), 0, 5, None), dict(nv=393, nt=682, ne=1075)),
    "nt683": ((31, 13, (7, 13, 4, 8), 1, 5, None), dict(nv=394, nt=683, ne=1077)),
    # ne on both sides of 2 048 (edges per thread: two / three), nt on both sides of 1 024 (cells per thread: one / two)
    "ne2048": ((40, 19, (10, 18, 6, 12), 0, 5, None), dict(nv=730, nt=1318, ne=2048)),
    "ne2049": ((40, 19, (10, 18, 6, 12), 2, 4, None), dict(nv=731, nt=1318, ne=2049)),
    "nt1024": ((35, 17, (8, 15, 5, 10), 0, 3, None), dict(nv=574, nt=1024, ne=1598)),
    "nt1025": ((35, 17, (8, 15, 5, 10), 1, 3, None), dict(nv=575, nt=1025, ne=1600)),
    # the vertex capacity of the instance = the workgroup's width: 1 023 and 1 024 vertices (1 025 belong to the K = 4 instance,
    # which keeps the general paths)
    "nv1023": ((51, 21, (12, 22, 7, 14), 1, 5, None), dict(nv=1023, nt=1871, ne=2894)),
    "nv1024": ((51, 21, (12, 22, 7, 14), 2, 5, None), dict(nv=1024, nt=1872, ne=2896)),
}
POLYGON = np.array([(0.2, -0.2), (0.45, -0.2), (0.7, -0.2), (0.9, -0.2), (0.9, -0.05), (0.9, 0.1), (0.9, 0.2), (0.7, 0.2),
                    (0.45, 0.2), (0.2, 0.2), (0.2, 0.1), (0.2, -0.05)], np.float64)
# (meshes of similar size share a batch: the capacities are the batch's largest; the hand-built mesh last in the lab batch)
BATCHES = {"small": ("nv63", "nv64", "nv65", "pinch", "hand"),
           "mid": ("nt341", "nt342", "ne1024", "ne1025", "nt682", "nt683"),
           "large": ("ne2048", "ne2049", "nt1024", "nt1025", "nv1023", "nv1024"),
           "lab": ("ys930", "ys930-hub42", "ah93w145", "hand")}
NAF_CAP, NSEL, EMAX = 256, 180, 6144


def channel(nx, ny, hole, wall_splits=0, cell_splits=0, pinch=None):
    """(coords, cells) of an nx x ny vertex grid on the channel, every quad cut along its (0, 0)-(1, 1) diagonal, without the
    quads i0 <= i < i1, j0 <= j < j1 (and the vertices strictly inside that block).  `wall_splits`: the first that many edges
    of the bottom wall get a vertex at their midpoint (one vertex, one cell, two edges more each); `cell_splits`: that many
    upper triangles, spread over the grid, get a vertex at their centroid (one vertex, two cells, three edges more each).
    `pinch = (i, j)`: the quads (i, j) and (i + 1, j + 1) are taken out as well - two holes whose boundaries meet in vertex
    (i + 1, j + 1), where four boundary edges and two fans of cells meet."""
    i0, i1, j0, j1 = hole
    assert 1 <= i0 < i1 <= nx - 2 and 1 <= j0 < j1 <= ny - 2
    xs, ys = np.linspace(-0.5, 3.0, nx), np.linspace(-0.5, 0.5, ny)
    gone = lambda i, j: (i0 <= i < i1 and j0 <= j < j1) or (pinch is not None and (i, j) in (pinch, (pinch[0] + 1, pinch[1] + 1)))  # noqa: E731
    vid, coords = {}, []
    for j in range(ny):
        for i in range(nx):
            if not (i0 < i < i1 and j0 < j < j1):
                vid[i, j] = len(coords)
                coords.append((xs[i], ys[j]))
    lower, upper = [], []
    for j in range(ny - 1):
        for i in range(nx - 1):
            if gone(i, j):
                continue
            a, b, c, d = vid[i, j], vid[i + 1, j], vid[i + 1, j + 1], vid[i, j + 1]
            lower.append([a, b, c])
            upper.append([a, c, d])
    assert wall_splits <= nx - 1 and cell_splits <= len(upper)
    extra = []
    for q in range(wall_splits):              # (the first quads of the bottom row: never part of the hole)
        a, b, c = lower[q]
        m = len(coords)
        coords.append((0.5 * (coords[a][0] + coords[b][0]), -0.5))
        lower[q] = [a, m, c]
        extra.append([m, b, c])
    step = max(1, len(upper) // max(1, cell_splits))
    for q in range(cell_splits):
        a, c, d = upper[q * step]
        m = len(coords)
        coords.append(tuple(np.mean([coords[a], coords[c], coords[d]], axis=0)))
        upper[q * step] = [a, c, m]
        extra += [[c, d, m], [a, d, m]]
    cells = np.sort(np.array(lower + upper + extra, np.int32), axis=1)
    return np.array(coords, np.float64), cells


def counts(cells):
    return int(cells.max()) + 1, len(cells), fic.edge_count(cells)


def mesh(meshes, name):
    if name in CASES:
        return channel(*CASES[name][0])
    return fic.mesh(meshes, name)


def batch(meshes, key):
    """(list of (coords, cells), constructor arguments of the engines) of a batch."""
    ms = [mesh(meshes, n) for n in BATCHES[key]]
    NV, NT, NE = max(len(c) for c, _ in ms), max(len(t) for _, t in ms), max(fic.edge_count(t) for _, t in ms)
    return ms, (len(ms), NV, NT, NE, NAF_CAP, NSEL, EMAX, POLYGON)


T_FLOW = ("ne", "cell_dofs", "points", "naf", "af_facets")          # what a flow_only engine writes of `t`
HANDOVER = ("coords", "cells", "nv", "nt", "cell_dofs", "ne")


def run_all(out_path):
    import torch
    from meshdqn_amd.mesh_ops import DeviceTopologyBatch
    meshes, out = fic.golden_meshes(), {}
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    for key in BATCHES:
        ms, args = batch(meshes, key)
        main = DeviceTopologyBatch(*args, device="cuda")
        full = DeviceTopologyBatch(*args, device="cuda", ipcs=True)
        first = DeviceTopologyBatch(*args, device="cuda", ipcs=True, flow_only=True)
        second = DeviceTopologyBatch(*args, device="cuda", ipcs=True, flow_only=True)
        for eng in (main, full, first):
            fic.fill(eng, ms, up)
        # `second` gets its mesh and its edge numbering from `main`'s launch, as the env step's flow stream does
        hand = dict(coords=second.coords, cells=second.cells, nv=second.nv, nt=second.nt,
                    cell_dofs=torch.zeros_like(main.t["cell_dofs"]), ne=torch.zeros_like(main.t["ne"]))
        main.set_handover(**hand)
        second.take_edges_from(hand["cell_dofs"], hand["ne"])
        for eng in (main, full, first, second):
            eng.run()
        torch.cuda.synchronize()
        for tag, eng in (("main", main), ("full", full), ("hash", first), ("given", second)):
            for k, v in eng.t.items():
                out[f"{key}/{tag}/t/{k}"] = v.cpu().numpy()
            for k, v in (eng.ti or {}).items():
                out[f"{key}/{tag}/ti/{k}"] = v.cpu().numpy()
        for k, v in hand.items():
            out[f"{key}/handover/{k}"] = v.cpu().numpy()
    np.savez(out_path, **out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    run_all(sys.argv[1])
