"""Inflow profiles: 1000 IPCS steps of ONE ys930 `FlowSolver` in operator mode 2 (the reproducible default) and in mode 3, three ways:

  profile    under the non-separable test profile through `mdq_ipcs_evolve_profile` (`FlowSolver.evolve(save_steps)`: the values
             of a call evaluated on the host up front, one upload, one small kernel in front of every step, one read-back);
  per step   the same inflow through the per-step loop the flow solver used before, driven directly: `batch.update_inflow`
             (host evaluation, H2D copy of bcu_gx, the whole set-up kernel) + `batch.evolve(1)` + read-back, every step;
  constant   under the constant inflow (`FlowSolver.evolve(save_steps)`: the yardstick of the same build).

HIP events and wall clock around the whole run, after one warm-up run of each way.
   python tools/time_inflow_profile.py [steps] [save_steps]

S3 case: the batched environment step with its flow leg (`VecEnv2DAirfoil.rollout_device`, flow_steps = 1, overlap mode, B
ys930 environments) under the constant inflow, under a schedule (one factor per environment and step inside the kernels) and
under a callable (the leg maps the inlet onto every new mesh - `mdq_ipcs_build_inlet_map` - and rewrites the lifts in front of
its step: two launches more per leg).  The cases alternate in one process; every window is `steps` batched steps between two
device synchronisations, after a warm-up rollout of each environment.
   python tools/time_inflow_profile.py s3 [B] [steps] [repeats] [cases, e.g. constant,schedule]"""
import os
import sys
import time

for _k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_k, "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(1)
from meshdqn_amd.flow_solver import FlowSolver  # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1] != "s3" else 1000
SAVE = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] != "s3" else 200
G = os.path.join(ROOT, "tests", "golden")
DT = 1e-3


def profile(x, y, t):
    """The tests' profile with its ramp held at 1 from t = 5 ms on (1000 steps reach t = 1: the plain ramp would drive the inflow
    to 100 times the constant one)."""
    return 6.0 * (0.5 + y) * (0.5 - y) * (1.0 + 0.6 * y * np.sin(2.0 * np.pi * 125.0 * t)) * min(0.5 + 100.0 * t, 1.0)


def solver(inflow, reproducible):
    return FlowSolver(flow_params=dict(mu=1e-3, rho=1.0, inflow=inflow), geometry_params=dict(mesh=os.path.join(G, "ys930.npz")),
                      solver_params=dict(dt=DT, smooth=True, reproducible=reproducible))


def run_calls(fs):
    for _ in range(STEPS // SAVE):
        fs.evolve(SAVE)
    return fs.accumulated_drag[-1]


def run_per_step(fs):
    """The per-step loop of the flow solver before profiles ran on the device, on a solver built under the constant inflow."""
    t, drag = 0.0, None
    for _ in range(STEPS):
        t += DT
        fs.batch.update_inflow(profile, t)
        d, _ = fs.batch.evolve(1)
        drag = d[0, 0].item()
    return drag


def timed(make, run):
    fs = make()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    drag = run(fs)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0), drag


def s3_main(argv):
    from meshdqn_amd.airfoilgcnn import NodeRemovalNet
    from meshdqn_amd.env import Env2DAirfoil
    from meshdqn_amd.gcn_fused import FusedGcn
    from meshdqn_amd.vec_env import VecEnv2DAirfoil
    nenv = int(argv[0]) if len(argv) > 0 else 128
    steps = int(argv[1]) if len(argv) > 1 else 40
    repeats = int(argv[2]) if len(argv) > 2 else 3
    names = argv[3].split(",") if len(argv) > 3 else ["constant", "schedule", "callable"]
    inflows = dict(constant="constant", schedule=dict(amplitude=1.0, pulsation=0.5, frequency=125.0), callable=profile)
    dev = torch.device("cuda")
    torch.manual_seed(0)
    net = NodeRemovalNet(181, conv_width=128, topk=0.1)
    net.set_num_nodes(17)
    net = net.to(dev)
    rng = np.random.default_rng(1370)
    envs = {}
    for name in names:
        cfg = dict(flow_config=dict(flow_params=dict(mu=1e-3, rho=1.0, inflow=inflows[name]),
                                    geometry_params=dict(mesh=os.path.join(G, "ys930.npz")),
                                    solver_params=dict(dt=DT, solver_type="lu", smooth=True)),
                   agent_params=dict(solver_steps=20, episodes=10, timesteps=10000, threshold=0.001, N_closest=180, gt_drag=-1,
                                     gt_time=-1, u=-1, p=-1, time_reward=0.005, save_steps=4, goal_vertices=0.95, plot_dir=""))
        venv = VecEnv2DAirfoil(cfg, nenv, compute_device=dev, base_env=Env2DAirfoil(cfg, compute_device=dev), flow_steps=1,
                               flow_rtol=1e-10, flow_overlap=True)
        fused = FusedGcn(net)
        venv.calibrate_streams(fused)
        envs[name] = (venv, fused)

    def window(name, k):
        venv, fused = envs[name]
        ex, ra = rng.random((k, nenv)) < 0.5, rng.integers(0, 181, (k, nenv))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        venv.rollout_device(fused, k, ex, ra)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for name in names:
        window(name, 8)                       # warm-up
    rates = {name: [] for name in names}
    for _ in range(repeats):
        for name in names:                    # alternating: drift of the machine hits every case alike
            rates[name].append(nenv * steps / window(name, steps))
    for name in names:
        r = rates[name]
        venv = envs[name][0]
        kind = "profile table" if getattr(venv.flow, "inflow_profile", None) is not None else ("factors" if venv.flow.inflow_scale is not None else "none")
        print(f"S3 B = {nenv}, {steps} batched steps per window, {name} (leg's inflow table: {kind}): env steps/s "
              f"{' '.join(f'{x:.0f}' for x in r)} | median {np.median(r):.0f}, min {min(r):.0f}, max {max(r):.0f}", flush=True)


if sys.argv[1:2] == ["s3"]:
    s3_main(sys.argv[2:])
    sys.exit(0)

for mode, reproducible in ((2, True), (3, False)):
    ways = {"profile": (lambda: solver(profile, reproducible), run_calls),
            "per step": (lambda: solver("constant", reproducible), run_per_step),
            "constant": (lambda: solver("constant", reproducible), run_calls)}
    for name, (make, run) in ways.items():
        timed(make, run)                      # warm-up
        ev, wall, drag = timed(make, run)
        print(f"mode {mode}, {STEPS} steps in calls of {SAVE if name != 'per step' else 1}, {name}: HIP events {ev:.1f} ms, wall {wall:.1f} ms "
              f"({1e3 * wall / STEPS:.1f} us per step), last drag {drag:.9f}", flush=True)
