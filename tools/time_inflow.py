"""Inflow schedules, two measurements.

1. The time-dependent ground truth: 1000 IPCS steps of ONE ys930 `FlowSolver` (default, reproducible operator mode) under
   schedule d = (0.8, 0.3, 50 Hz, 1.0) three ways - through the schedule dict (`mdq_ipcs_evolve_inflow`: one launch per
   `save_steps` steps, the factors applied inside the kernels), through the callable path given the same inflow (one H2D
   copy + set-up launch + evolve launch + read-back per step: the only way before schedules existed), and under the constant
   inflow.  HIP events and wall clock around the whole run, after one warm-up run of each.
2. The S3 rate (`rollout_device`, flow_steps=1, overlap) of 64 + 64 ys930 environments under schedule a and schedule d
   (`mixed_inflow=True`) against the mean of the two homogeneous 128-environment rates, measured in turns (median of the
   repeats), as tools/time_mixed_flow.py does for mu.
   python tools/time_inflow.py [steps] [repeats]"""
import math
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
from meshdqn_amd.flow_solver import FlowSolver  # noqa: E402
from meshdqn_amd.gcn_fused import FusedGcn  # noqa: E402
from meshdqn_amd.vec_env import VecEnv2DAirfoil  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 50
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 5
G = os.path.join(ROOT, "tests", "golden")
A_, D_ = dict(amplitude=1.0), dict(amplitude=0.8, pulsation=0.3, frequency=50.0, phase=1.0)
STEPS, SAVE = 1000, 200


def a_d(t):
    return D_["amplitude"] * (1.0 + D_["pulsation"] * math.sin(2.0 * math.pi * D_["frequency"] * t + D_["phase"]))


def solver(inflow):
    return FlowSolver(flow_params=dict(mu=1e-3, rho=1.0, inflow=inflow), geometry_params=dict(mesh=os.path.join(G, "ys930.npz")),
                      solver_params=dict(dt=1e-3, smooth=True))


def timed_run(inflow):
    fs = solver(inflow)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(STEPS // SAVE):
        fs.evolve(SAVE)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0), fs.accumulated_drag[-1]


ways = {"schedule dict": D_, "callable": lambda x, y, t: -4.0 * 1.5 * (y + 0.5) * (y - 0.5) * a_d(t), "constant": "constant"}
for name, inflow in ways.items():
    timed_run(inflow)                      # warm-up
    ev, wall, drag = timed_run(inflow)
    print(f"ground truth, {STEPS} steps, {name}: HIP events {ev:.1f} ms, wall {wall:.1f} ms ({1e3 * wall / STEPS:.1f} us per step), "
          f"last drag {drag:.9f}", flush=True)


def cfg(key, inflow, tmp):
    return dict(flow_config=dict(flow_params=dict(mu=1e-3, rho=1.0, inflow=inflow),
                                 geometry_params=dict(mesh=os.path.join(G, "ys930.npz")),
                                 solver_params=dict(dt=1e-3, solver_type="lu", smooth=True)),
                agent_params=dict(solver_steps=STEPS, episodes=10, timesteps=10000, threshold=0.001, N_closest=180,
                                  gt_drag=-1, gt_time=-1, u=-1, p=-1, time_reward=0.005, save_steps=SAVE, goal_vertices=0.95,
                                  plot_dir=os.path.join(tmp, key)))


tmp = tempfile.mkdtemp()
cfgs = [cfg("a", A_, tmp), cfg("d", D_, tmp)]
bases = [Env2DAirfoil(c) for c in cfgs]
print(f"ground truths: drag a {np.asarray(bases[0].gt_drag)[-1]:.5f}, d {np.asarray(bases[1].gt_drag)[-1]:.5f}")
net = NodeRemovalNet(181, conv_width=128, topk=0.1)
net.set_num_nodes(2 + 3 * (STEPS // SAVE))
fused = FusedGcn(net.cuda())
rng = np.random.default_rng(1370)


def run(venv, k):
    ex = rng.random((k, venv.B)) < 0.5
    ra = rng.integers(0, 181, (k, venv.B))
    return venv.rollout_device(fused, k, ex, ra)


kw = dict(flow_steps=1, flow_overlap=True)
envs = {"a x128": VecEnv2DAirfoil(cfgs[0], 128, base_env=bases[0], **kw),
        "d x128": VecEnv2DAirfoil(cfgs[1], 128, base_env=bases[1], **kw),
        "mixed 64+64": VecEnv2DAirfoil(cfgs, 128, base_env=bases, mixed_inflow=True, **kw)}
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
    print(f"S3 {n}: median {v:.0f} env-steps/s ({1e3 * 128 / v:.3f} ms per batched step; min {min(rates[n]):.0f} max {max(rates[n]):.0f})")
print(f"S3 mixed / mean of the homogeneous rates: {med['mixed 64+64'] / (0.5 * (med['a x128'] + med['d x128'])):.3f}", flush=True)
