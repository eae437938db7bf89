"""A batch that mixes two airfoils against the homogeneous batches: env-steps/s of the device-resident rollout
(`rollout_device`, greedy / random actions as in tools/time_rollout.py) of 128 ys930, 128 ah93w145 and 64 + 64 mixed
environments, S1 (flow 0) or S3 (flow 1), the three batches measured in turns (median of the repeats).  The ground truth
comes from the committed oracle episodes' snapshots (tests/golden/oracle_stock_*.npz), so no 5000-step solve is run.
   python tools/time_mixed.py [flow] [steps] [repeats]"""
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
from meshdqn_amd.vec_env import VecEnv2DAirfoil  # noqa: E402

FLOW = int(sys.argv[1]) if len(sys.argv) > 1 else 0
K = int(sys.argv[2]) if len(sys.argv) > 2 else 50
REP = int(sys.argv[3]) if len(sys.argv) > 3 else 5
G = os.path.join(ROOT, "tests", "golden")


def snapshot_cfg(mesh, tmp):
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
                                  time_reward=0.005, save_steps=1000, goal_vertices=0.95, plot_dir=os.path.join(tmp, mesh)))


tmp = tempfile.mkdtemp()
cfgs = [snapshot_cfg(m, tmp) for m in ("ys930", "ah93w145")]
bases = [Env2DAirfoil(c) for c in cfgs]
kw = dict(flow_steps=FLOW, flow_overlap=bool(FLOW))
envs = {"ys930 x128": VecEnv2DAirfoil(cfgs[0], 128, base_env=bases[0], **kw),
        "ah93w145 x128": VecEnv2DAirfoil(cfgs[1], 128, base_env=bases[1], **kw),
        "mixed 64+64": VecEnv2DAirfoil(cfgs, 128, base_env=bases, **kw)}
net = NodeRemovalNet(181, conv_width=128, topk=0.1)
net.set_num_nodes(17)
fused = FusedGcn(net.cuda())
rng = np.random.default_rng(1370)


def run(venv, k):
    ex = rng.random((k, venv.B)) < 0.5
    ra = rng.integers(0, 181, (k, venv.B))
    return venv.rollout_device(fused, k, ex, ra)


for venv in envs.values():
    venv.get_state()
    run(venv, 30)
rates = {n: [] for n in envs}
for r in range(REP):
    for name, venv in envs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(venv, K)
        torch.cuda.synchronize()
        rates[name].append(venv.B * K / (time.perf_counter() - t0))
med = {n: float(np.median(v)) for n, v in rates.items()}
for n, v in med.items():
    print(f"flow={FLOW} {n}: median {v:.0f} env-steps/s ({1e3 * 128 / v:.3f} ms per batched step; "
          f"min {min(rates[n]):.0f} max {max(rates[n]):.0f})")
mean_h = 0.5 * (med["ys930 x128"] + med["ah93w145 x128"])
print(f"flow={FLOW} mixed / mean of the homogeneous rates: {med['mixed 64+64'] / mean_h:.3f}")
