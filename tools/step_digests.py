"""sha256 of u_n, p_n, drag, lift and iters after ONE launch of a few IPCS steps, one line per case - for whichever build of
the library MDQ_LIB_PATH names (default: the tree's).  The evolve kernels are run-to-run bitwise reproducible in the
operator modes listed here, so a change that must not alter a result bit (a refactor of the time step) is checked by

    MDQ_LIB_PATH=<parent build> python tools/step_digests.py > a.txt;  python tools/step_digests.py > b.txt;  diff a.txt b.txt

(run the parent build twice first: a case whose digests differ between those two runs says nothing).  Every batch carries an
env_phys table of two flow settings and per-environment inflow schedules, so the per-environment constants and the inflow
factor are part of what is hashed.  Mode 3 is left out: its LDS atomics are reproducible to round-off only."""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from meshdqn_amd import _lib
from meshdqn_amd.ipcs_batch import IpcsBatch, smooth_coords
from meshdqn_amd.mesh_ops import red_refine
from meshdqn_amd.topology import MeshTopology

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
SCHED = [dict(amplitude=1.0, pulsation=0.5, frequency=125.0), dict(amplitude=0.8, pulsation=0.3, frequency=50.0, phase=1.0)]
PHYS = [(1e-3, 2.0, 5e-4), (1e-3, 1.0, 1e-3)]      # mu, rho, dt


def mesh(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    t = MeshTopology(z["coords"], z["cells"])
    return t, smooth_coords(t, 50), z["cells"]


def digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()[:16]


def case(label, topos, xs, nsteps, **kw):
    B = len(topos)
    phys = [PHYS[b % 2] for b in range(B)]
    try:
        batch = IpcsBatch(topos, xs, mu=[p[0] for p in phys], rho=[p[1] for p in phys], dt=[p[2] for p in phys], rtol=1e-12,
                          inflow=[SCHED[b % 2] for b in range(B)], **kw)
        drag, lift = batch.evolve(nsteps)
        torch.cuda.synchronize()
    except (_lib.MeshDQNHipError, ValueError) as e:       # (a mode that does not take this batch: the same line from both builds)
        print(f"{label}: {type(e).__name__}: {str(e)[:100]}", flush=True)
        return
    print(f"{label}: mode {batch.desc.mode} u {digest(batch.u_n)} p {digest(batch.p_n)} drag {digest(drag)} lift {digest(lift)} "
          f"iters {digest(batch.iters)} {batch.iters.cpu().numpy().ravel().tolist()}", flush=True)


def main():
    print("library", os.path.basename(_lib.LIB_PATH), flush=True)
    t0, x0, cells0 = mesh("ys930")
    t1, x1, _ = mesh("ah93w145")
    rc, rcells = red_refine(x0, cells0)
    tr = MeshTopology(rc, rcells)
    for direct in ("device", False):
        for mode in (0, 1, 4, 5, 7):       # small meshes: packed tile words
            case(f"small  mode {mode:2d} direct {direct}", [t0, t1], [x0, x1], 3, mode=mode, pressure_direct=direct)
        for mode in (0, 4, 5, 7, -1):      # refined meshes: plain tile maps, row lists
            case(f"refined mode {mode:2d} direct {direct}", [tr, tr, t0], [rc, rc, x0], 3, mode=mode, pressure_direct=direct)
    rc2, rcells2 = red_refine(rc, rcells)       # pressure vectors in the workspace slab
    t2 = MeshTopology(rc2, rcells2)
    for mode in (-1, 0):
        case(f"twice refined mode {mode:2d}", [t2], [rc2], 2, mode=mode)
    case("mode 2", [t0], [x0], 3, mode=2, pressure_direct=False)


if __name__ == "__main__":
    main()
