"""The size ladder of the IPCS tests: synthetic channel meshes whose sizes sit on the kernels' size switches
(tests/golden/ipcs_ladder.npz, written by tests/golden/make_ipcs_ladder.py), their names, the batches the GPU tests run and
the child process of the 512-wide velocity kernel (`python tests/ipcs_ladder_cases.py OUT.npz`).

`MDQ_AT_WG=512` selects `at_velocity_kernel<512, 7, 2>` in place of the default `<768, 5, 1>`; the library reads the variable
once per process, so the parent starts a fresh child with it set, the child runs every case of WIDTH_BATCHES through mode 3 and
writes what it got, and the parent compares with the oracle."""
import os
import sys

import numpy as np

from flow_index_cases import hand_mesh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name -> (the size the mesh was built for, its value); "hand" is the hand-built mesh of tests/flow_index_cases.py
TARGETS = {
    "hand": ("n2", 152), "nv64": ("nv", 64), "nv65": ("nv", 65),
    "nt512": ("nt", 512), "nt513": ("nt", 513), "nt768": ("nt", 768), "nt769": ("nt", 769), "nt1024": ("nt", 1024),
    "nt1025": ("nt", 1025), "nt1536": ("nt", 1536), "nt1537": ("nt", 1537),
    "outflow_heavy": ("n2", 1135), "outflow_collide": ("n2", 1135),
    "n2_3402": ("n2", 3402), "n2_3404": ("n2", 3404), "n2_3584": ("n2", 3584), "n2_3586": ("n2", 3586),
    "n2_4096": ("n2", 4096), "n2_4098": ("n2", 4098), "n2_5104": ("n2", 5104), "n2_5106": ("n2", 5106),
}
CASES = tuple(TARGETS)
# every case of at most 2 400 rows in ONE batch, the tiny meshes beside the largest (capacity NV = 578 < 1 024: the padded NVp)
SMALL = ("nt1025", "hand", "nv64", "nt1024", "nv65", "nt512", "nt513", "outflow_heavy", "outflow_collide", "nt768", "nt769")
MID = ("nt1536", "nt1537")                     # two / three rounds of the 768-wide velocity kernel, two tiles of 1 024
EDGES = ("n2_3402", "n2_3404", "n2_3584", "n2_3586", "n2_4096", "n2_4098", "n2_5104", "n2_5106")
WIDTH_BATCHES = {"small": SMALL, "n2_3402": ("n2_3402",)}
STEPS = 3


def load_ladder():
    """name -> (coords float64 (nv, 2), cells int32 (nt, 3))."""
    z = np.load(os.path.join(GOLDEN, "ipcs_ladder.npz"))
    out = {"hand": hand_mesh()}
    for name in CASES:
        if name != "hand":
            out[name] = (z[f"{name}/coords"], z[f"{name}/cells"])
    return out


def sizes(coords, cells):
    e = np.sort(np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [0, 2]]]), axis=1)
    ne = len(np.unique(e, axis=0))
    return dict(nv=len(coords), nt=len(cells), ne=ne, n2=len(coords) + ne)


def smoothed(coords, cells):
    """The coordinates both sides step on: the oracle's own `smooth(50)` of the mesh (one source, no second smoother)."""
    from oracle.mesh import OracleMesh
    m = OracleMesh(coords, cells)
    m.smooth(50)
    return np.ascontiguousarray(m.coords, dtype=np.float64)


def make_batch(meshes, names, **kw):
    from meshdqn_amd.ipcs_batch import IpcsBatch
    from meshdqn_amd.topology import MeshTopology
    topos = [MeshTopology(*meshes[n]) for n in names]
    return IpcsBatch(topos, [smoothed(*meshes[n]) for n in names], device="cuda", rtol=1e-12, **kw)


def run_steps(batch, steps=STEPS):
    """`steps` single steps from rest -> dict of host arrays: u (steps, B, N2, 2), p (steps, B, NV), drag / lift (steps, B),
    iters (B, 3), status (B,)."""
    import torch
    u, p, dr, li = [], [], [], []
    for _ in range(steps):
        d, l = batch.evolve(1)
        torch.cuda.synchronize()
        u.append(batch.u_n.cpu().numpy().copy())
        p.append(batch.p_n.cpu().numpy().copy())
        dr.append(d[:, 0].cpu().numpy().copy())
        li.append(l[:, 0].cpu().numpy().copy())
    return dict(u=np.stack(u), p=np.stack(p), drag=np.stack(dr), lift=np.stack(li), iters=batch.iters.cpu().numpy(),
                status=batch.status.cpu().numpy())


def run_widths(out_path):
    """The child of the width test: mode 3 on every batch of WIDTH_BATCHES, CG pressure."""
    meshes, out = load_ladder(), {}
    for key, names in WIDTH_BATCHES.items():
        res = run_steps(make_batch(meshes, names, mode=3, pressure_direct=False))
        for k, a in res.items():
            out[f"{key}/{k}"] = a
    np.savez(out_path, **out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    run_widths(sys.argv[1])
