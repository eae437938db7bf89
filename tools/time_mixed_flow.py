"""A batch that mixes two flow conditions on ONE mesh against the homogeneous batches: env-steps/s of the device-resident
rollout (`rollout_device`, greedy / random actions as in tools/time_mixed.py) of 128 ys930 environments at setting a
(mu 1e-3, rho 1, dt 1e-3), 128 at setting b (mu 2e-3) and 64 + 64 mixed (`mixed_flow=True`: per-environment constants through
`mdq_ipcs_desc.env_phys`), S1 (flow 0) and S3 (flow 1) in one process, the three batches measured in turns (median of the
repeats).  Each setting's ground truth is computed on the device when its base environment is built (5000 IPCS steps).
Then, to say WHICH kernels pay if the ratio is low: HIP-event times of the two entry points whose kernels read the table,
alone on the stream - the flow leg's mode 3 kernel by kernel (`at_velocity / at_pressure / at_correction_kernel`:
`IpcsBatch.evolve_timed`, 20 steps from a developed flow; the iteration counts are printed, since mu moves them) and
`mdq_probe_forces` (`probe_kernel`) -
for 128 ys930 meshes at a, at b, 64 + 64 with the table, and at a with a table whose rows all repeat a (the cost of the load
alone: same work, same iteration counts).
   python tools/time_mixed_flow.py [steps] [repeats]"""
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
from meshdqn_amd.ipcs_batch import IpcsBatch, smooth_coords  # noqa: E402
from meshdqn_amd.mesh_ops import LightMeshBatch  # noqa: E402
from meshdqn_amd.topology import MeshTopology  # noqa: E402
from meshdqn_amd.vec_env import VecEnv2DAirfoil  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 50
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 5
G = os.path.join(ROOT, "tests", "golden")
FLOWS = {"a": (1e-3, 1.0, 1e-3), "b": (2e-3, 1.0, 1e-3)}


def cfg(key, tmp):
    mu, rho, dt = FLOWS[key]
    return dict(flow_config=dict(flow_params=dict(mu=mu, rho=rho, inflow="constant"),
                                 geometry_params=dict(mesh=os.path.join(G, "ys930.npz")),
                                 solver_params=dict(dt=dt, solver_type="lu", smooth=True)),
                agent_params=dict(solver_steps=5000, episodes=10, timesteps=10000, threshold=0.001, N_closest=180,
                                  gt_drag=-1, gt_time=-1, u=-1, p=-1, time_reward=0.005, save_steps=1000, goal_vertices=0.95,
                                  plot_dir=os.path.join(tmp, key)))


tmp = tempfile.mkdtemp()
cfgs = [cfg(k, tmp) for k in FLOWS]
t0 = time.perf_counter()
bases = [Env2DAirfoil(c) for c in cfgs]
print(f"ground truths ({time.perf_counter() - t0:.1f} s): drag a {np.asarray(bases[0].gt_drag)[-1]:.5f}, b {np.asarray(bases[1].gt_drag)[-1]:.5f}")
net = NodeRemovalNet(181, conv_width=128, topk=0.1)
net.set_num_nodes(17)
fused = FusedGcn(net.cuda())
rng = np.random.default_rng(1370)


def run(venv, k):
    ex = rng.random((k, venv.B)) < 0.5
    ra = rng.integers(0, 181, (k, venv.B))
    return venv.rollout_device(fused, k, ex, ra)


for FLOW in (0, 1):
    kw = dict(flow_steps=FLOW, flow_overlap=bool(FLOW))
    envs = {"a x128": VecEnv2DAirfoil(cfgs[0], 128, base_env=bases[0], **kw),
            "b x128": VecEnv2DAirfoil(cfgs[1], 128, base_env=bases[1], **kw),
            "mixed 64+64": VecEnv2DAirfoil(cfgs, 128, base_env=bases, mixed_flow=True, **kw)}
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
    mean_h = 0.5 * (med["a x128"] + med["b x128"])
    print(f"flow={FLOW} mixed / mean of the homogeneous rates: {med['mixed 64+64'] / mean_h:.3f}", flush=True)
    del envs


# ---- the entry points that read the table, by HIP events
def event_ms(fn, n=20):
    """median over n of the HIP-event time of one call of fn alone on the stream (ms)."""
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out))


z = np.load(os.path.join(G, "ys930.npz"))
topo = MeshTopology(z["coords"], z["cells"])
x0 = smooth_coords(topo, 50)
(mua, rhoa, dta), (mub, rhob, dtb) = FLOWS["a"], FLOWS["b"]
half = [mua] * 64 + [mub] * 64
settings = {"a x128": dict(mu=mua, rho=rhoa, dt=dta), "b x128": dict(mu=mub, rho=rhob, dt=dtb),
            "mixed 64+64": dict(mu=half, rho=[rhoa] * 64 + [rhob] * 64, dt=[dta] * 64 + [dtb] * 64),
            "a x128, table of equal rows": dict(mu=[mua] * 128, rho=[rhoa] * 128, dt=[dta] * 128)}
ev = {}
for name, kw in settings.items():
    batch = IpcsBatch([topo] * 128, [x0] * 128, rtol=1e-12, mode=3, **kw)
    batch.evolve(200)                      # a developed flow, warm kernels
    kms = np.median([np.asarray(batch.evolve_timed(20)[2]) / 20 for _ in range(5)], axis=0)      # ms per step and kernel
    it = batch.iters.cpu().numpy()
    light = LightMeshBatch([topo] * 128, [x0] * 128, kw["mu"])
    u = batch.u_n[:, None, :topo.np2].contiguous()
    p = batch.p_n[:, None, :topo.nv].contiguous()
    light.probe_forces(u, p)
    ev[name] = list(kms) + [event_ms(lambda: light.probe_forces(u, p))]
    print(f"events {name}: per step velocity {1e3 * kms[0]:.1f} us, pressure {1e3 * kms[1]:.1f} us, correction {1e3 * kms[2]:.1f} us "
          f"(iterations u / p / m {it[:, 0].mean():.1f} / {it[:, 1].mean():.1f} / {it[:, 2].mean():.1f}); "
          f"probe_kernel {1e3 * ev[name][3]:.1f} us")
    del batch, light
for i, what in enumerate(("at_velocity_kernel", "at_pressure_kernel", "at_correction_kernel", "probe_kernel")):
    print(f"events {what}: mixed / mean(a, b) {ev['mixed 64+64'][i] / (0.5 * (ev['a x128'][i] + ev['b x128'][i])):.3f}; "
          f"table of equal rows / no table {ev['a x128, table of equal rows'][i] / ev['a x128'][i]:.3f}", flush=True)
