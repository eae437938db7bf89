import os, sys, time
for _k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_k, "1")
sys.path.insert(0, "/root/repo")
import numpy as np, torch
torch.set_num_threads(1)
from meshdqn_amd.env import Env2DAirfoil
from meshdqn_amd.vec_env import VecEnv2DAirfoil
from meshdqn_amd.airfoilgcnn import NodeRemovalNet
from meshdqn_amd.gcn_fused import FusedGcn
G = "/root/repo/tests/golden"
cfg = dict(flow_config=dict(flow_params=dict(mu=1e-3, rho=1.0, inflow="constant"), geometry_params=dict(mesh=os.path.join(G, "ys930.npz")),
                            solver_params=dict(dt=0.001, solver_type="lu", smooth=True)),
           agent_params=dict(solver_steps=500, episodes=10, timesteps=10000, threshold=0.001, N_closest=180, gt_drag=-1, gt_time=-1, u=-1, p=-1,
                             time_reward=0.005, save_steps=100, goal_vertices=0.95, plot_dir=""))
base = Env2DAirfoil(cfg)
net = NodeRemovalNet(181, conv_width=128, topk=0.1); net.set_num_nodes(17); net = net.cuda()
rng = np.random.default_rng(1370)
B, K = 128, 40
for name, kw in (("flow_steps=1 cg", dict(flow_steps=1)), ("flow_steps=2 cg", dict(flow_steps=2)), ("flow_steps=3 cg", dict(flow_steps=3)),
                 ("flow_steps=1 direct", dict(flow_steps=1, flow_pressure="direct")),
                 ("inline flow_steps=0", dict(flow_steps=0, flow_overlap=False)),
                 ("inline flow_steps=1 cg", dict(flow_steps=1, flow_overlap=False)),
                 ("inline flow_steps=1 direct", dict(flow_steps=1, flow_pressure="direct", flow_overlap=False))):
    kw = dict(dict(flow_overlap=True), **kw)
    env = VecEnv2DAirfoil(cfg, B, base_env=base, **kw)
    fg = FusedGcn(net)
    def run(k):
        t0 = time.perf_counter()
        env.rollout_device(fg, k, rng.random((k, B)) < 0.5, rng.integers(0, 181, (k, B)))
        torch.cuda.synchronize(); return (time.perf_counter() - t0) / k * 1e3
    run(10)
    best = min(run(K) for _ in range(3))
    leg = float("nan")                  # (only an overlapped leg is timed on its own stream)
    if env.flow is not None:
        env.flow.events = []
        run(20)
        if env.flow.events:
            leg = np.median([a.elapsed_time(b) for a, b in env.flow.events])
        env.flow.events = None
    print(f"{name:28s}: {best:.3f} ms per batched step; flow leg on its stream {leg:.3f} ms", flush=True)
    env.flow_wait(); del env
