"""What the mesh-quality guard costs when it is on: env-steps/s of the device-resident rollout (`rollout_device`, greedy / random
actions as in tools/time_mixed.py) of 128 ys930 environments with `min_angle` set against the same build without the keys,
S1 (flow 0) or S3 (flow 1), the two batches measured in turns (median of the repeats), and the HIP-event time of
`mesh_quality_kernel` alone on 128 ys930 meshes and on 128 red-refined ones (3 322 vertices / 6 280 cells).  The ground truth
comes from the committed oracle episode's snapshots (tests/golden/oracle_stock_ys930.npz), so no 5000-step solve is run.
   python tools/time_quality.py [flow] [steps] [repeats]"""
import os
import sys
import tempfile
import time

for _k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_k, "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(1)
from meshdqn_amd.airfoilgcnn import NodeRemovalNet  # noqa: E402
from meshdqn_amd.env import Env2DAirfoil  # noqa: E402
from meshdqn_amd.gcn_fused import FusedGcn  # noqa: E402
from meshdqn_amd.mesh_ops import mesh_quality_gpu  # noqa: E402
from meshdqn_amd.vec_env import VecEnv2DAirfoil  # noqa: E402

FLOW = int(sys.argv[1]) if len(sys.argv) > 1 else 0
K = int(sys.argv[2]) if len(sys.argv) > 2 else 50
REP = int(sys.argv[3]) if len(sys.argv) > 3 else 5
G = os.path.join(ROOT, "tests", "golden")


def snapshot_cfg(mesh, tmp, **agent):
    z = np.load(os.path.join(G, f"oracle_stock_{mesh}.npz"))
    snap = os.path.join(tmp, mesh, "snapshots")
    os.makedirs(snap, exist_ok=True)
    u, p = z["u"], z["p"]
    n2 = u.shape[1] // 2
    np.save(os.path.join(snap, "save_velocities.npy"), np.stack([u[:, :n2], u[:, n2:]], axis=2).reshape(len(u), -1))
    np.save(os.path.join(snap, "save_pressures.npy"), p)
    return dict(flow_config=dict(flow_params=dict(mu=1e-3, rho=1.0, inflow="constant"),
                                 geometry_params=dict(mesh=os.path.join(G, f"{mesh}.npz")),
                                 solver_params=dict(dt=0.001, solver_type="lu", smooth=True)),
                agent_params=dict(solver_steps=5000, episodes=10, timesteps=10000, threshold=0.001, N_closest=180,
                                  gt_drag=z["gt_drag"].copy(), gt_lift=z["gt_lift"].copy(), gt_time=np.array([5.0]), u=-1, p=-1,
                                  time_reward=0.005, save_steps=1000, goal_vertices=0.95, plot_dir=os.path.join(tmp, mesh), **agent))


def kernel_time(name, coords, cells, B=128, reps=200):
    """Median HIP-event time of one `mdq_mesh_quality` launch on B copies of a mesh, in microseconds."""
    c = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(coords, (B,) + coords.shape))).cuda()
    t = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(cells.astype(np.int32), (B,) + cells.shape))).cuda()
    nv = torch.full((B,), coords.shape[0], dtype=torch.int32, device="cuda")
    nt = torch.full((B,), cells.shape[0], dtype=torch.int32, device="cuda")
    out = mesh_quality_gpu(c, t, nv, nt)
    for _ in range(20):
        mesh_quality_gpu(c, t, nv, nt, out=out)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        mesh_quality_gpu(c, t, nv, nt, out=out)
        e1.record()
    torch.cuda.synchronize()
    us = sorted(1e3 * e0.elapsed_time(e1) for e0, e1 in ev)
    print(f"mesh_quality_kernel, {B} x {name} ({coords.shape[0]} vertices, {cells.shape[0]} cells): median {us[reps // 2]:.2f} us, "
          f"min {us[0]:.2f} us, q_min {float(out[0][0, 0]):.4f}")


tmp = tempfile.mkdtemp()
cfg_off = snapshot_cfg("ys930", tmp)
cfg_on = snapshot_cfg("ys930", tmp, min_angle=5.0)      # (on, and far below the angles of an episode: the batches stay alike)
base = Env2DAirfoil(cfg_off)
kw = dict(flow_steps=FLOW, flow_overlap=bool(FLOW))
envs = {"without the keys": VecEnv2DAirfoil(cfg_off, 128, base_env=base, **kw),
        "min_angle set": VecEnv2DAirfoil(cfg_on, 128, base_env=base, **kw)}
net = NodeRemovalNet(181, conv_width=128, topk=0.1)
net.set_num_nodes(17)
fused = FusedGcn(net.cuda())


def run(venv, k, seed):
    rng = np.random.default_rng(seed)       # (the same draws for both batches)
    ex = rng.random((k, venv.B)) < 0.5
    ra = rng.integers(0, 181, (k, venv.B))
    return venv.rollout_device(fused, k, ex, ra)


for venv in envs.values():
    venv.get_state()
    run(venv, 30, 0)
rates = {n: [] for n in envs}
for r in range(REP):
    for name, venv in envs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(venv, K, 1 + r)
        torch.cuda.synchronize()
        rates[name].append(venv.B * K / (time.perf_counter() - t0))
med = {n: float(np.median(v)) for n, v in rates.items()}
for n, v in med.items():
    print(f"flow={FLOW} {n}: median {v:.0f} env-steps/s ({1e3 * 128 / v:.3f} ms per batched step; "
          f"min {min(rates[n]):.0f} max {max(rates[n]):.0f})")
print(f"flow={FLOW} min_angle set / without the keys: {med['min_angle set'] / med['without the keys']:.3f}")
z = np.load(os.path.join(G, "ys930.npz"))
kernel_time("ys930", z["coords"], z["cells"])
z = np.load(os.path.join(G, "oracle_stock_ys930_refined.npz"))
kernel_time("ys930 red-refined", z["coords"], z["cells"])
