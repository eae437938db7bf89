"""Time train_loop_device (S3 env step + replay + optimiser chain) with the optimiser chain on the flow stream / on a stream
of its own (dev tool).   python tools/time_train_device.py [B] [steps] [--prioritized] [--n-step N] [--target-net KIND] [--q-head HEAD] [--noisy-net]
--prioritized: every placement is timed with uniform replay and, beside it, with prioritized replay (three more launches per
optimiser step on the optimiser stream).  --n-step N: the trainer composes N-step returns inside its sampling launch.
--target-net KIND (max | double): the trainer keeps policy_net_2 as a target network (one more forward and the select launch
per optimiser step for double, the target update every 50 steps).  MDQ_TARGET_PERIOD / MDQ_TARGET_TAU: its other options.
--q-head HEAD (softmax | linear | dueling): the head of both Q-networks (default softmax).
--noisy-net: noisy networks (sigma0 0.5) instead of epsilon-greedy: the acting pack and both train packs of every step carry
noise, one mdq_noisy_grad per optimiser step."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import numpy as np, torch
from meshdqn_amd.env import Env2DAirfoil
from meshdqn_amd.trainer import DistContext, DQNTrainer, train_loop_device
from meshdqn_amd.vec_env import VecEnv2DAirfoil
G_ = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
cfg = dict(flow_config=dict(flow_params=dict(mu=1e-3, rho=1.0, inflow="constant"), geometry_params=dict(mesh=os.path.join(G_, "ys930.npz")),
                            solver_params=dict(dt=0.001, solver_type="lu", smooth=True)),
           agent_params=dict(solver_steps=500, episodes=10, timesteps=10000, threshold=0.001, N_closest=180, gt_drag=-1, gt_time=-1, u=-1, p=-1,
                             time_reward=0.005, save_steps=100, goal_vertices=0.95, plot_dir=""))
argv = sys.argv[1:]
n_step = 1
if "--n-step" in argv:
    k = argv.index("--n-step")
    n_step = int(argv[k + 1])
    del argv[k:k + 2]
target_net = None
if "--target-net" in argv:
    k = argv.index("--target-net")
    target_net = dict(kind=argv[k + 1], period=int(os.environ.get("MDQ_TARGET_PERIOD", "50")), tau=float(os.environ.get("MDQ_TARGET_TAU", "1.0")))
    del argv[k:k + 2]
q_head = "softmax"
if "--q-head" in argv:
    k = argv.index("--q-head")
    q_head = argv[k + 1]
    del argv[k:k + 2]
noisy = dict(sigma0=0.5) if "--noisy-net" in argv else None
pos = [a for a in argv if not a.startswith("--")]
B = int(pos[0]) if len(pos) > 0 else 128
n = int(pos[1]) if len(pos) > 1 else 40
base = Env2DAirfoil(cfg)
for mode, prio in [(m, p) for m in ("flow", "own", "flow", "own") for p in ((None, {}) if "--prioritized" in sys.argv else (None,))]:
    trainer = DQNTrainer(n_actions=180, num_inputs=17, ctx=DistContext(), prioritized=prio, n_step=n_step, target_net=target_net, head=q_head, noisy=noisy)
    venv = VecEnv2DAirfoil(cfg, B, base_env=base, flow_steps=1, flow_overlap=True)
    train_loop_device(trainer, venv, 6, optimiser_stream=mode)
    torch.cuda.synchronize(); t0 = time.time()
    train_loop_device(trainer, venv, n, optimiser_stream=mode)
    torch.cuda.synchronize(); dt = time.time() - t0
    print(f"optimiser_stream={mode} prioritized={'off' if prio is None else 'on'} n_step={n_step} target_net={'off' if target_net is None else target_net['kind']} q_head={q_head} noisy={'off' if noisy is None else 'on'}: {dt / n * 1e3:.3f} ms per batched step -> {B * n / dt:.0f} env-steps/s; calibration flow "
          f"{[round(v, 2) for v in getattr(venv, 'calibration_ms', [])]} opt {[round(v, 2) for v in trainer.opt_calibration_ms]}", flush=True)
    venv.flow_wait()
    del venv, trainer
