"""GPU: `mdq_ipcs_evolve_fresh` - "a new mesh in the same descriptor" without the reset launch - against
`mdq_ipcs_reset_history` + `mdq_ipcs_evolve` from the same DIRTY workspace.

The workspace is dirtied by 6 steps on [ys930, ah93w145] (a full tentative-velocity history, a full correction ring, a lagged
|b| of the fused correction start); the descriptor then gets two other meshes (each airfoil after one vertex removal on the host
engine) and fields at rest.  Both paths must leave the same iteration and history counters and meet, on the new meshes, the
bound of `test_ipcs_gpu.py::test_first_steps_match_oracle` (1e-8, relative to the oracle's maximum) against the sparse-LU
oracle from rest - a path that read any of the stale history would start its solves from vectors of another mesh.  Mode 3
sums with LDS atomics (no bitwise comparison between two runs); mode 2, where the entry point launches the reset kernel
itself, must be bitwise equal."""
import ctypes as C

import numpy as np
import pytest

from oracle_util import interleaved_to_oracle_vel

pytestmark = pytest.mark.gpu

NAMES = ["ys930", "ah93w145"]
DIRTY_STEPS, STEPS = 6, 2
BOUND = 1e-8        # test_first_steps_match_oracle


@pytest.fixture(scope="module")
def removed(meshes, lib_built):
    """The two airfoils after one scripted removal each (host engine: removal + Delaunay restoration + smooth(50)), and
    the oracle's u, p, drag, lift after every one of STEPS steps from rest on them."""
    from meshdqn_amd.mesh_ops import remesh_batch
    from oracle.ipcs import OracleFlowSolver
    from oracle.mesh import OracleMesh
    out = []
    for k, n in enumerate(NAMES):
        coords, cells = meshes[n]
        rem = np.flatnonzero(OracleMesh(coords, cells).removable())
        idx = int(rem[(7 + 31 * k) % rem.size])
        c = np.ascontiguousarray(coords[None], np.float64).copy()
        t = np.ascontiguousarray(cells[None], np.int32).copy()
        nv, nt = np.array([coords.shape[0]], np.int32), np.array([cells.shape[0]], np.int32)
        assert (remesh_batch(c, t, nv, nt, np.array([idx], np.int32)) == 0).all()
        assert nv[0] == coords.shape[0] - 1
        c, t = c[0, :nv[0]].copy(), t[0, :nt[0]].copy()
        o = OracleFlowSolver(c, t, smooth=False)
        out.append(dict(coords=c, cells=t, n2=o.th.np2, nv=o.th.nv, steps=[o.evolve() for _ in range(STEPS)]))
    return out


def _counters(work, cap, B):
    """(B, 7) history words of every environment's slab: histc | ccnt[0..3] (mode 3) | hcnt[0..1] (the other modes)."""
    from meshdqn_amd import _lib
    NV, NT, NE = cap["NV"], cap["NT"], cap["NE"]
    N2 = NV + NE
    per = int(_lib.load().mdq_ipcs_workspace_doubles(1, NV, NT, NE))
    hist = (12 * NT + 12 * N2 + NV + 25) & ~1
    w = work.cpu().numpy().reshape(B, per)
    cols = [12 * NT + 6 * N2] + [hist + 6 * N2 + i for i in range(4)] + [hist + 10 * N2, hist + 10 * N2 + 1]
    return w[:, cols]


def _setup(meshes, removed, mode):
    import torch
    from meshdqn_amd.ipcs_batch import IpcsBatch, smooth_coords
    from meshdqn_amd.topology import MeshTopology
    kw = dict(device="cuda", rtol=1e-12, mode=mode, pressure_direct=False)
    old = [MeshTopology(*meshes[n]) for n in NAMES]
    new = [MeshTopology(r["coords"], r["cells"]) for r in removed]
    fresh = IpcsBatch(new, [r["coords"] for r in removed], **kw)
    dirty = IpcsBatch(old, [smooth_coords(t, 50) for t in old], **kw)
    cap = {k: max(fresh.cap[k], dirty.cap[k]) for k in dirty.cap}
    if cap != dirty.cap:
        dirty = IpcsBatch(old, [smooth_coords(t, 50) for t in old], capacities=cap, **kw)
    if cap != fresh.cap:
        fresh = IpcsBatch(new, [r["coords"] for r in removed], capacities=cap, **kw)
    dirty.evolve(DIRTY_STEPS)
    fresh.assemble()            # the operators of the new meshes
    torch.cuda.synchronize()
    return dirty, fresh, cap


def _descriptor(dirty, fresh):
    """A descriptor on the new meshes whose workspace is a copy of the dirty one; fields at rest, iteration words set."""
    import torch
    from meshdqn_amd import _lib
    d = _lib.IpcsDesc()
    C.memmove(C.byref(d), C.byref(fresh.desc), C.sizeof(d))
    own = dict(work=dirty.t["work"].clone(), u_n=torch.zeros_like(fresh.t["u_n"]), p_n=torch.zeros_like(fresh.t["p_n"]),
               status=torch.zeros_like(fresh.status), iters=torch.full_like(fresh.iters, 777),
               drag=torch.zeros((fresh.B, STEPS), dtype=torch.float64, device="cuda"))
    own["lift"] = torch.zeros_like(own["drag"])
    for k in ("work", "u_n", "p_n", "status"):
        setattr(d, k, own[k].data_ptr())
    return d, own


def _run(lib, d, own, fresh_entry, iters=True):
    import torch
    from meshdqn_amd import _lib
    it = own["iters"].data_ptr() if iters else None
    if fresh_entry:
        _lib.check(lib.mdq_ipcs_evolve_fresh(C.byref(d), STEPS, own["drag"].data_ptr(), own["lift"].data_ptr(), it, None,
                                             _lib.stream_ptr()), "mdq_ipcs_evolve_fresh")
    else:
        _lib.check(lib.mdq_ipcs_reset_history(C.byref(d), it, _lib.stream_ptr()), "mdq_ipcs_reset_history")
        _lib.check(lib.mdq_ipcs_evolve(C.byref(d), STEPS, own["drag"].data_ptr(), own["lift"].data_ptr(), it,
                                       _lib.stream_ptr()), "mdq_ipcs_evolve")
    torch.cuda.synchronize()
    assert (own["status"].cpu().numpy() == 0).all()
    return {k: v.cpu().numpy() for k, v in own.items() if k != "work"}


def _against_oracle(res, removed, what):
    for b, r in enumerate(removed):
        uo, po, _, _ = r["steps"][-1]
        eu = np.abs(interleaved_to_oracle_vel(res["u_n"][b][:r["n2"]]) - uo).max() / np.abs(uo).max()
        ep = np.abs(res["p_n"][b][:r["nv"]] - po).max() / np.abs(po).max()
        ed = max(abs(res["drag"][b, s] - r["steps"][s][2]) / abs(r["steps"][s][2]) for s in range(STEPS))
        el = max(abs(res["lift"][b, s] - r["steps"][s][3]) / abs(r["steps"][s][3]) for s in range(STEPS))
        print(f"{what} env {b}: rel err vs oracle u {eu:.2e} p {ep:.2e} drag {ed:.2e} lift {el:.2e}")
        assert max(eu, ep, ed, el) < BOUND, (what, b, eu, ep, ed, el)


def test_fresh_history_mode3(meshes, removed, lib_built):
    from meshdqn_amd import _lib
    lib = _lib.load()
    dirty, fresh, cap = _setup(meshes, removed, 3)
    B = fresh.B
    c0 = _counters(dirty.t["work"], cap, B)
    assert (c0[:, 0] == 5).all() and (c0[:, 1] == 3).all() and (c0[:, 3] > 0).all() and (c0[:, 4] == DIRTY_STEPS).all()
    dA, ownA = _descriptor(dirty, fresh)
    dB, ownB = _descriptor(dirty, fresh)
    dN, ownN = _descriptor(dirty, fresh)
    a = _run(lib, dA, ownA, True)
    b = _run(lib, dB, ownB, False)
    n = _run(lib, dN, ownN, True, iters=False)          # iters = NULL
    cA, cB, cN = (_counters(o["work"], cap, B) for o in (ownA, ownB, ownN))
    print("iters fresh", a["iters"].tolist(), "reset + evolve", b["iters"].tolist())
    print("counters fresh", cA.tolist(), "reset + evolve", cB.tolist())
    # iteration counters: assigned by the first step, equal to the reset path's; untouched without an `iters` array
    assert np.array_equal(a["iters"], b["iters"]) and (a["iters"] > 0).all() and (a["iters"] < 777).all()
    assert (n["iters"] == 777).all()
    # history counters after the call: STEPS tentative velocities / corrections stored, ring position and step count STEPS,
    # the other modes' counters zero - and the lagged |b|^2 of the last exact correction start to round-off
    for c in (cA, cB, cN):
        assert np.array_equal(c[:, [0, 1, 2, 4, 5, 6]], np.tile([STEPS, STEPS, STEPS % 3, STEPS, 0, 0], (B, 1)))
    for c in (cA, cN):
        assert np.array_equal(c[:, [0, 1, 2, 4, 5, 6]], cB[:, [0, 1, 2, 4, 5, 6]])
        assert (np.abs(c[:, 3] - cB[:, 3]) <= 1e-9 * np.abs(cB[:, 3])).all() and (cB[:, 3] > 0).all()
    _against_oracle(a, removed, "fresh")
    _against_oracle(b, removed, "reset + evolve")
    _against_oracle(n, removed, "fresh, iters = NULL")


def test_fresh_history_mode2_is_bitwise_the_reset_path(meshes, removed, lib_built):
    from meshdqn_amd import _lib
    lib = _lib.load()
    dirty, fresh, cap = _setup(meshes, removed, 2)
    B = fresh.B
    c0 = _counters(dirty.t["work"], cap, B)
    assert (c0[:, 5] == 5).all()                        # hcnt: a full history of the one-kernel modes
    dA, ownA = _descriptor(dirty, fresh)
    dB, ownB = _descriptor(dirty, fresh)
    a = _run(lib, dA, ownA, True)
    b = _run(lib, dB, ownB, False)
    for k in ("iters", "u_n", "p_n", "drag", "lift"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    assert (a["iters"] > 0).all() and (a["iters"] < 777).all()
    cA, cB = _counters(ownA["work"], cap, B), _counters(ownB["work"], cap, B)
    assert np.array_equal(cA.view(np.uint64), cB.view(np.uint64)) and (cA[:, 5] == STEPS).all()
    _against_oracle(a, removed, "mode 2 fresh")
