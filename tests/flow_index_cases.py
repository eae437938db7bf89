"""The meshes of the flow-index-list test and the child process that runs the device engine on them
(`python tests/flow_index_cases.py OUT.npz`).

The IPCS index section of `topology_kernel` builds the dof <- slot gather lists (g2 / g1) and the SELL pattern of the P1
Laplacian (sl1).  By default the rows of the edge dofs are written straight from the edge tables and short lists are ranked in
registers; `MDQ_TOPO_INDEX_PARENT=3` (read once per process) selects the general count / fill / sort path and the ranking loops
for everything: the parent's code.  Both sides of the comparison come from child processes that run ALL the cases, each
through both edge numberings of the flow stream's engine: its own hash table, and the numbering handed over by another
engine's run (`take_edges_from`).

Meshes: a hand-built channel [-0.5, 3] x [-0.5, 0.5] of 44 vertices with a pentagonal hole (below), ys930 as loaded and after 20
and 42 scripted removals (tests/pressure_width_cases.py), ah93w145.  Two batches of three, the hand-built mesh in the last
slot of both."""
import os
import sys

import numpy as np

# 44 vertices: 0-18 the channel's boundary (7 along the bottom, 7 along the top, 3 on the inlet, 2 on the outlet), 19-23 the
# hole, 24 a hub inside the ring 25-34, 35-43 scattered.  Vertex lists (cells per vertex) of every length from 1 (the corners
# 0 and 7, cut off by one cell) to 8, and the hub's 10; boundary edges on the walls, the inlet, the outlet and the hole.
HAND_COORDS = [
    (-0.5, -0.5), (-0.3, -0.5), (0.2, -0.5), (0.9, -0.5),
    (1.6, -0.5), (2.3, -0.5), (3.0, -0.5), (-0.5, 0.5),
    (-0.3, 0.5), (0.2, 0.5), (0.9, 0.5), (1.6, 0.5),
    (2.3, 0.5), (3.0, 0.5), (-0.5, -0.3), (-0.5, 0.0),
    (-0.5, 0.3), (3.0, -0.2), (3.0, 0.2), (0.3859802840213045, 0.02659681859952056),
    (0.30127429130197364, 0.08999097833492929), (0.21480727131488353, 0.029020664692321185), (0.24607370677627619, -0.0720552211789608), (0.351864446585562, -0.07355324044781023),
    (1.75, 0.0), (2.018651124625067, 0.026955022494643602), (1.9514995606820578, 0.17971624034832728), (1.8073820132766745, 0.2638319627192952),
    (1.6413464871424992, 0.2471728426500875), (1.5168129099228156, 0.13610209778447596), (1.481348875374933, -0.026955022494643592), (1.5485004393179422, -0.17971624034832728),
    (1.6926179867233255, -0.26383196271929515), (1.8586535128575008, -0.24717284265008754), (1.9831870900771844, -0.1361020977844761), (-0.22, -0.24),
    (-0.2, 0.2), (0.7, 0.15), (0.75, -0.2), (1.1, 0.0),
    (2.5, 0.1), (2.6, -0.25), (0.3, 0.3), (0.3, -0.3),
]
HAND_CELLS = [
    (3, 38, 39), (10, 37, 39), (37, 38, 39), (2, 3, 43), (3, 38, 43), (13, 18, 40), (3, 4, 31), (3, 31, 39),
    (12, 13, 40), (15, 16, 36), (8, 9, 36), (7, 8, 16), (8, 16, 36), (0, 1, 14), (19, 37, 38), (17, 18, 40),
    (25, 34, 40), (10, 11, 29), (10, 29, 39), (25, 26, 40), (12, 26, 40), (14, 15, 35), (15, 35, 36), (1, 14, 35),
    (21, 35, 36), (1, 2, 35), (2, 35, 43), (21, 22, 35), (22, 35, 43), (23, 38, 43), (19, 23, 38), (22, 23, 43),
    (19, 37, 42), (9, 10, 42), (10, 37, 42), (21, 36, 42), (9, 36, 42), (5, 6, 41), (6, 17, 41), (17, 40, 41),
    (34, 40, 41), (5, 34, 41), (4, 5, 33), (5, 33, 34), (30, 31, 39), (29, 30, 39), (11, 12, 27), (12, 26, 27),
    (20, 21, 42), (19, 20, 42), (4, 31, 32), (4, 32, 33), (11, 28, 29), (11, 27, 28), (24, 25, 26), (24, 25, 34),
    (24, 31, 32), (24, 30, 31), (24, 33, 34), (24, 29, 30), (24, 26, 27), (24, 32, 33), (24, 27, 28), (24, 28, 29),
]
HAND_HOLE = (19, 20, 21, 22, 23)
BATCHES = {"a": ("ys930", "ys930-hub20", "hand"), "b": ("ys930-hub42", "ah93w145", "hand")}
KEYS_T = ("ne", "cell_dofs")
KEYS_TI = ("g2_ptr", "g2_src", "g1_ptr", "g1_src", "sl1_off", "sl1_col")
NAF_CAP, NSEL, EMAX = 256, 180, 1536


def hand_mesh():
    return np.array(HAND_COORDS, np.float64), np.array(HAND_CELLS, np.int32)


def golden_meshes():
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = {}
    for name in ("ys930", "ah93w145"):
        z = np.load(os.path.join(g, f"{name}.npz"))
        out[name] = (z["coords"], z["cells"])
    return out


def mesh(meshes, name):
    if name == "hand":
        return hand_mesh()
    from pressure_width_cases import case_mesh
    c, t, _ = case_mesh(meshes, name)
    return np.asarray(c, np.float64), np.sort(t, axis=1).astype(np.int32)


def edge_count(cells):
    e = np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [0, 2]]])
    return len(np.unique(np.sort(e, axis=1), axis=0))


def batch(meshes, key):
    """(list of (coords, cells), constructor arguments of the engines) of a batch."""
    ms = [mesh(meshes, n) for n in BATCHES[key]]
    NV, NT, NE = max(len(c) for c, _ in ms), max(len(t) for _, t in ms), max(edge_count(t) for _, t in ms)
    polygon = np.array(HAND_COORDS, np.float64)[list(HAND_HOLE)]
    return ms, (len(ms), NV, NT, NE, NAF_CAP, NSEL, EMAX, polygon)


def fill(eng, ms, to=lambda a: a):
    for b, (c, t) in enumerate(ms):
        eng.coords[b, :len(c)] = to(c)
        eng.cells[b, :len(t)] = to(t)
        eng.nv[b], eng.nt[b] = len(c), len(t)


def run_all(out_path):
    """Every batch through the flow stream's engine (`flow_only`) with its own edge numbering (`hash/...`) and with the
    numbering of a first run handed over (`given/...`)."""
    import torch
    from meshdqn_amd.mesh_ops import DeviceTopologyBatch
    meshes, out = golden_meshes(), {}
    for key in BATCHES:
        ms, args = batch(meshes, key)
        first = DeviceTopologyBatch(*args, device="cuda", ipcs=True, flow_only=True)
        fill(first, ms, lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
        first.run()
        second = DeviceTopologyBatch(*args, device="cuda", ipcs=True, flow_only=True)
        fill(second, ms, lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
        second.take_edges_from(first.t["cell_dofs"].clone(), first.t["ne"].clone())
        second.run()
        torch.cuda.synchronize()
        for tag, eng in (("hash", first), ("given", second)):
            for k in KEYS_T:
                out[f"{key}/{tag}/{k}"] = eng.t[k].cpu().numpy()
            for k in KEYS_TI:
                out[f"{key}/{tag}/{k}"] = eng.ti[k].cpu().numpy()
    np.savez(out_path, **out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    run_all(sys.argv[1])
