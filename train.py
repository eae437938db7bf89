#!/usr/bin/env python3
"""Multi-GPU counterpart of `python3 airfoil_dqn.py` (reference airfoil_dqn.py:343-514):

    python train.py --config configs/ray_ys930.yaml                                   # 1 GPU
    python train.py --gpus 8 --config configs/ray_ys930.yaml                          # 8 GPUs (RCCL): starts its ranks itself
    torchrun --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 train.py --config ...   # the same under torchrun

One process per GPU; every rank steps `--envs` environments (VecEnv2DAirfoil), all ranks apply the same
all-reduced gradient, replay transitions are optionally all-gathered.  The yaml is the reference's own format
(`flow_config`, `agent_params`, `optimizer`, `epsilon`); `geometry_params.mesh` may point at an .xdmf or .npz file."""
import argparse
import os as _os

# single-threaded BLAS / OpenMP pools BEFORE numpy / scipy / torch are imported: the hosts expose hundreds of logical CPUs
# under a small CPU quota, and idle pool threads that keep spinning starve the threads that launch kernels
for _k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    _os.environ.setdefault(_k, "1")
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # concurrent streams on separate hardware queues (meshdqn_amd/__init__.py)
import os

import numpy as np
import yaml


def prioritized_options(flag: bool, cfg: dict):
    """The `prioritized` argument of `DQNTrainer` from --prioritized-replay and the optional yaml block
    `replay: {prioritized: true, alpha: 0.6, beta0: 0.4, beta_steps: 100000, eps: 1.0e-6}` (not a reference section: its
    replay is uniform).  None: uniform replay; the flag alone: the defaults; the block's numbers hold with either switch."""
    block = dict(cfg.get("replay") or {})
    block.pop("n_step", None)               # (the block's other option: `n_step_option`)
    on = bool(block.pop("prioritized", False)) or bool(flag)
    unknown = sorted(set(block) - {"alpha", "beta0", "beta_steps", "eps"})
    if unknown:
        raise SystemExit(f"replay: unknown key(s) {unknown} (known: prioritized, alpha, beta0, beta_steps, eps, n_step)")
    return {k: float(v) for k, v in block.items()} if on else None


def n_step_option(flag, cfg: dict) -> int:
    """The `n_step` argument of `DQNTrainer` from --n-step and the optional yaml key `replay: {n_step: N}` (not a reference
    key: its targets are 1-step).  The flag wins when both are given; neither: 1."""
    if flag is not None:
        return int(flag)
    n = (cfg.get("replay") or {}).get("n_step", 1)
    if isinstance(n, bool) or not isinstance(n, int):
        raise SystemExit(f"replay: n_step must be an integer, not {n!r}")
    return n


def target_options(args, cfg: dict):
    """The `target_net` argument of `DQNTrainer` from --target-net / --target-tau / --target-period and the optional
    top-level yaml block `target_net: {kind: double, tau: 1.0, period: 50}` (not a reference section: its two networks swap
    roles and never exchange weights).  None: the reference's toggle.  The block alone switches the option on; every flag
    wins over the block's key; --target-tau / --target-period without a kind from either side: an error."""
    block = cfg.get("target_net")
    if block is not None and not isinstance(block, dict):
        raise SystemExit(f"target_net: a block with any of kind, tau, period, not {block!r}")
    opt = dict(block or {})
    unknown = sorted(set(opt) - {"kind", "tau", "period"}, key=repr)
    if unknown:
        raise SystemExit(f"target_net: unknown key(s) {unknown} (known: kind, tau, period)")
    for key, flag in (("kind", args.target_net), ("tau", args.target_tau), ("period", args.target_period)):
        if flag is not None:
            opt[key] = flag
    if block is None and args.target_net is None:
        if opt:
            raise SystemExit("--target-tau / --target-period need --target-net {max,double} or a yaml block target_net:")
        return None
    return opt


Q_HEADS = ("softmax", "linear", "dueling")


def q_head_option(flag, cfg: dict) -> str:
    """The `head` argument of `DQNTrainer` from --q-head and the optional top-level yaml key `q_head: dueling` (not a
    reference key: its network's outputs are softmax probabilities).  The flag wins when both are given; neither: softmax."""
    head = flag if flag is not None else cfg.get("q_head", "softmax")
    if not isinstance(head, str) or head not in Q_HEADS:
        raise SystemExit(f"q_head: {head!r} is none of " + ", ".join(Q_HEADS))
    return head


def noisy_options(flag, cfg: dict):
    """The `noisy` argument of `DQNTrainer` from --noisy-net [SIGMA0] and the optional top-level yaml block
    `noisy_net: {sigma0: 0.5}` (not a reference section: its exploration is epsilon-greedy).  None: epsilon-greedy.  The
    block alone switches the option on; the flag's number wins over the block's; the noise seed is the trainer's."""
    block = cfg.get("noisy_net")
    if block is not None and not isinstance(block, dict):
        raise SystemExit(f"noisy_net: a block with sigma0, not {block!r}")
    if block is None and flag is None:
        return None
    opt = dict(block or {})
    unknown = sorted(set(opt) - {"sigma0"}, key=repr)
    if unknown:
        raise SystemExit(f"noisy_net: unknown key(s) {unknown} (known: sigma0)")
    if flag is not None and flag is not True:
        opt["sigma0"] = float(flag)
    return opt


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True, action="append",
                    help="yaml config; repeat it to train ONE policy on several airfoils (their configs may differ only in the "
                         "mesh, gt_*, u / p and plot_dir; global env id g steps airfoil g mod A)")
    ap.add_argument("--mixed-flow", action="store_true",
                    help="with several --config: they may also differ in flow_params.mu / .rho and solver_params.dt (ONE policy "
                         "over several Reynolds numbers, also on one and the same mesh); without it such a difference is an error")
    ap.add_argument("--mixed-inflow", action="store_true",
                    help="with several --config: they may also differ in flow_params.inflow, the inflow schedule "
                         "(inflow: {amplitude: 0.5, pulsation: 0.2, frequency: 2.0}; ONE policy over several inflows, also on "
                         "one and the same mesh); without it such a difference is an error")
    ap.add_argument("--gpus", type=int, default=0,
                    help="N > 1 without a launcher (WORLD_SIZE unset): this process becomes the parent of N rank processes "
                         "(meshdqn_amd/launcher.py: 127.0.0.1 rendezvous, every rank watched, a dying rank ends the job)")
    ap.add_argument("--digest", action="store_true",
                    help="debugging / tests: one batched step per chunk, and after EVERY batched step every rank appends "
                         "sha256 digests of both Q-networks, the optimiser moments and its replay ring to "
                         "<save-dir>/digest_rank<r>.jsonl (replicas that diverge show up as differing lines)")
    ap.add_argument("--envs", type=int, default=128, help="environments per GPU")
    ap.add_argument("--steps", type=int, default=1000, help="batched rollout steps")
    ap.add_argument("--flow-steps", type=int, default=0, help="IPCS steps on the coarsened mesh per env step (S3)")
    ap.add_argument("--share-replay", action="store_true")
    ap.add_argument("--save-dir", default="training_results/run")
    ap.add_argument("--restart", action="store_true",
                    help="continue the run found in --save-dir: both Q-networks, optimiser / scheduler state, epsilon "
                         "counters and the logs (files of restart n carry n 'restart_' / 'RESTART_' prefixes, like the "
                         "reference's RESTART_NUM chain, airfoil_dqn.py:359-366)")
    ap.add_argument("--save-every", type=int, default=50, help="batched steps between checkpoints / log writes (0 = only at the end)")
    ap.add_argument("--host-loop", action="store_true",
                    help="host-driven loop (train_loop_vec: autograd replayed as a HIP graph, one read-back per step) instead "
                         "of the device-resident one (train_loop_device: replay, sampling, forward + backward and Adam as kernels)")
    ap.add_argument("--prioritized-replay", action="store_true",
                    help="proportional prioritized experience replay in the device-resident loop (draw, importance weights and "
                         "priority update as kernels of the optimiser chain); its numbers come from the optional yaml block "
                         "replay: {prioritized: true, alpha: 0.6, beta0: 0.4, beta_steps: 100000, eps: 1.0e-6}")
    ap.add_argument("--n-step", type=int, default=None, metavar="N",
                    help="n-step returns in the device-resident loop, 1 .. 64 (the n-step transition of every drawn record is "
                         "composed from the record ring inside the sampling launch); also the yaml key replay: {n_step: N}; "
                         "default 1")
    ap.add_argument("--target-net", choices=("max", "double"), default=None,
                    help="a target network in the device-resident loop: policy_net_1 is trained on every step, policy_net_2 is "
                         "its copy, refreshed every --target-period gradient steps; double: Double-DQN targets "
                         "Q_target(s', argmax_a Q_online(s', a)), max: max_a Q_target(s', a); also the yaml block "
                         "target_net: {kind: double, tau: 1.0, period: 50}; default: the reference's toggle")
    ap.add_argument("--target-tau", type=float, default=None, metavar="T",
                    help="Polyak factor of the target refresh in (0, 1], target += T (online - target); default 1: a copy")
    ap.add_argument("--target-period", type=int, default=None, metavar="P",
                    help="gradient steps between two refreshes of the target network; default: agent_params.target_update")
    ap.add_argument("--q-head", choices=Q_HEADS, default=None,
                    help="what both Q-networks put out, in every loop: softmax (default, the reference's probabilities), linear "
                         "(the raw lin3 outputs) or dueling (v + A - mean A with a value stream lin_v, Wang et al. 2016); also "
                         "the top-level yaml key q_head:; checkpoints of different heads do not load into each other")
    ap.add_argument("--noisy-net", nargs="?", type=float, const=True, default=None, metavar="SIGMA0",
                    help="noisy networks in the device-resident loop instead of epsilon-greedy: factorised Gaussian noise of "
                         "initial scale SIGMA0 / sqrt(inputs) (default 0.5) on the dense head of both Q-networks, drawn on the "
                         "device while the parameters are packed, one draw per batched step; also the yaml block "
                         "noisy_net: {sigma0: 0.5}; checkpoints with and without it do not load into each other")
    ap.add_argument("--lift-weight", type=float, default=None, metavar="W",
                    help="weight of the lift in the reward, (drag_reward + W lift_reward) / (1 + W): the yaml key "
                         "agent_params.lift_weight (not a reference key: its reward reads the drag only); alone, the lift also "
                         "stops an episode at the drag's `threshold`")
    ap.add_argument("--lift-threshold", type=float, default=None, metavar="T",
                    help="relative lift error that ends an episode (agent_params.lift_threshold); alone, a pure stop criterion "
                         "(W = 0)")
    ap.add_argument("--quality-weight", type=float, default=None, metavar="WQ",
                    help="weight of the mesh quality in the reward, (drag_reward [+ W lift_reward] + WQ quality_reward) / "
                         "(1 [+ W] + WQ) with quality_reward = 2 min(q_min / q_min of the initial mesh, 1) - 1: the yaml key "
                         "agent_params.quality_weight (not a reference key: its reward never looks at the cells)")
    ap.add_argument("--min-quality", type=float, default=None, metavar="Q",
                    help="smallest shape quality q in [0, 1) below which an episode ends (agent_params.min_quality; 0: no stop)")
    ap.add_argument("--min-angle", type=float, default=None, metavar="DEG",
                    help="smallest cell angle in degrees, in [0, 60), below which an episode ends (agent_params.min_angle; 0: no "
                         "stop); any of the three switches the per-step quality launch on")
    return ap


def quality_options(args, cfgs):
    """--quality-weight / --min-quality / --min-angle written into agent_params of every config (the flags win over the
    yaml keys) before the environments are built; meshdqn_amd/reward.py reads and validates them."""
    for c in cfgs:
        for key in ("quality_weight", "min_quality", "min_angle"):
            v = getattr(args, key)
            if v is not None:
                c["agent_params"][key] = float(v)


def lift_options(args, cfgs):
    """--lift-weight / --lift-threshold written into agent_params of every config (the flags win over the yaml keys) before
    the environments are built; meshdqn_amd/reward.py reads and validates them."""
    for c in cfgs:
        if args.lift_weight is not None:
            c["agent_params"]["lift_weight"] = float(args.lift_weight)
        if args.lift_threshold is not None:
            c["agent_params"]["lift_threshold"] = float(args.lift_threshold)


def main():
    args = parser().parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        import importlib.util
        import sys
        spec = importlib.util.spec_from_file_location("mdq_launcher", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                                    "meshdqn_amd", "launcher.py"))
        launcher = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(launcher)              # (by file path: the parent never imports the package / torch)
        have = launcher.visible_gpus()
        if have is not None and have < args.gpus and not os.environ.get("MDQ_SHARE_GPU"):
            raise SystemExit(f"--gpus {args.gpus} needs {args.gpus} GPUs on this node, the driver exposes {have} "
                             "(MDQ_SHARE_GPU=1 MDQ_DIST_BACKEND=gloo lets several ranks share a GPU, for debugging only)")
        rc, out0 = launcher.start_ranks(os.path.abspath(__file__), sys.argv[1:], args.gpus, tag="train")
        sys.stdout.write("".join(out0))
        raise SystemExit(rc)
    if args.gpus > 1 and int(os.environ["WORLD_SIZE"]) != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} and the launcher's WORLD_SIZE={os.environ['WORLD_SIZE']} disagree")
    from meshdqn_amd.env import Env2DAirfoil
    from meshdqn_amd.trainer import DistContext, DQNTrainer, TrainingLog, train_loop_device, train_loop_vec
    from meshdqn_amd.vec_env import VecEnv2DAirfoil, airfoil_assignment, check_airfoil_configs
    import torch
    torch.set_num_threads(1)   # (many-core hosts under a CPU quota: the CPU-side tensor ops are tiny, no intra-op pool)
    cfgs = [yaml.safe_load(open(path)) for path in args.config]
    lift_options(args, cfgs)
    quality_options(args, cfgs)
    check_airfoil_configs(cfgs, mixed_flow=args.mixed_flow, mixed_inflow=args.mixed_inflow)     # (before any device work: a typo in a yaml ends the run here)
    cfg = cfgs[0]
    ctx = DistContext()
    opt = cfg.get("optimizer", {})          # reference yaml sections: optimizer / epsilon (configs/ray_ys930.yaml)
    eps = cfg.get("epsilon", {})
    ap_ = cfg["agent_params"]
    trainer = DQNTrainer(n_actions=int(ap_["N_closest"]), num_inputs=2 + 3 * (int(ap_["solver_steps"]) // int(ap_["save_steps"])),
                         ctx=ctx, lr=float(opt.get("lr", 1e-5)), weight_decay=float(opt.get("weight_decay", 1e-6)),
                         batch_size=int(opt.get("batch_size", 32)), gamma=float(eps.get("gamma", 1.0)),
                         target_update=int(ap_.get("target_update", 50)),
                         prioritized=prioritized_options(args.prioritized_replay, cfg), n_step=n_step_option(args.n_step, cfg),
                         target_net=target_options(args, cfg), head=q_head_option(args.q_head, cfg),
                         noisy=noisy_options(args.noisy_net, cfg))
    # restart chain: restart n reads the checkpoint with n - 1 "restart_" prefixes and writes with n (every rank loads the
    # same files, so the replicas stay identical)
    restart_num, steps_done0 = 0, None
    if args.restart:
        restart_num = sum(f.endswith("policy_net_1.pt") for f in os.listdir(args.save_dir))
        if restart_num == 0:
            raise SystemExit(f"--restart: no policy_net_1.pt checkpoint in {args.save_dir}")
        extra = trainer.load(args.save_dir, "restart_" * (restart_num - 1))
        steps_done0 = extra.get("steps_done")
        if steps_done0 is not None and len(steps_done0) != args.envs:      # other batch size: restart the counters at the mean
            steps_done0 = np.full(args.envs, int(np.mean(steps_done0)), np.int64)
    prefix = "restart_" * restart_num
    if len(cfgs) == 1:
        base = Env2DAirfoil(cfg, compute_device=ctx.device)      # ground truth + snapshots (the reference's first reset())
        venv = VecEnv2DAirfoil(cfg, args.envs, compute_device=ctx.device, base_env=base, flow_steps=args.flow_steps,
                               flow_overlap=args.flow_steps > 0)
    else:
        # one policy over several airfoils: global env id g = rank * envs + b steps airfoil g mod A (every rank's block of
        # ids sees every airfoil); one base environment (ground truth + snapshots) per airfoil
        bases = [Env2DAirfoil(c, compute_device=ctx.device) for c in cfgs]
        venv = VecEnv2DAirfoil(cfgs, args.envs, compute_device=ctx.device, base_env=bases, flow_steps=args.flow_steps,
                               flow_overlap=args.flow_steps > 0,
                               airfoil_of_env=airfoil_assignment(args.envs, len(cfgs), ctx.rank * args.envs),
                               mixed_flow=args.mixed_flow, mixed_inflow=args.mixed_inflow)
    log = TrainingLog(args.save_dir, restart=args.restart, restart_num=restart_num) if ctx.rank == 0 else None

    def checkpoint(step, steps_done):
        if ctx.rank == 0:                                        # (the reference writes after every episode)
            trainer.save(args.save_dir, prefix, extra=dict(steps_done=np.asarray(steps_done).copy(), batched_steps=step))
            log.write()                                          # reward / rewards / losses / actions / eps .npy

    device_loop = ctx.device.type == "cuda" and venv.gpu_remesh and not args.host_loop
    if trainer.prioritized is not None and not device_loop:
        raise SystemExit("prioritized replay needs the device-resident loop (a GPU, the device mesh engine, no --host-loop)")
    if trainer.n_step > 1 and not device_loop:
        raise SystemExit("n-step returns need the device-resident loop (a GPU, the device mesh engine, no --host-loop)")
    if trainer.target_net is not None and not device_loop:
        raise SystemExit("a target network needs the device-resident loop (a GPU, the device mesh engine, no --host-loop)")
    if trainer.noisy is not None and not device_loop:
        raise SystemExit("noisy networks need the device-resident loop (a GPU, the device mesh engine, no --host-loop)")
    loop = train_loop_device if device_loop else train_loop_vec
    kw, every, on_every = {}, args.save_every, checkpoint
    if args.digest:
        import hashlib
        import json
        os.makedirs(args.save_dir, exist_ok=True)
        dpath = os.path.join(args.save_dir, f"{prefix}digest_rank{ctx.rank}.jsonl")
        open(dpath, "w").close()

        def sha(tensors):
            h = hashlib.sha256()
            for t in tensors:
                h.update(t.detach().contiguous().cpu().numpy().tobytes())
            return h.hexdigest()

        def ring_rows(step):
            # FINISHED records of this job (the rows every rank must agree on): a step's records get their next state - and,
            # with the shared replay, travel to the other ranks - one step later (at once for the last step of the job)
            wrec = args.envs * (ctx.world if (args.share_replay and ctx.multi) else 1)
            return min((step if step >= args.steps else step - 1) * wrec, trainer.device_memory.capacity)

        def on_every(step, steps_done):          # noqa: F811 - every batched step: digests, then the periodic checkpoint
            torch.cuda.synchronize() if ctx.device.type == "cuda" else None
            rep = trainer.device_memory
            opt_state = [v for o in trainer.opts for st in o.state.values() for k, v in sorted(st.items()) if torch.is_tensor(v)]
            rec = dict(step=int(step), net1=sha(trainer.policy_net_1.parameters()), net2=sha(trainer.policy_net_2.parameters()),
                       optimiser=sha(opt_state), optimiser_steps=len(trainer.losses),
                       ring=None if rep is None else sha([rep.R[:ring_rows(step)]]), steps_done=[int(v) for v in steps_done])
            with open(dpath, "a") as f:
                f.write(json.dumps(rec) + "\n")
            if args.save_every and step % args.save_every == 0:
                checkpoint(step, steps_done)
        every = 1
        if device_loop:
            kw["chunk"] = 1
    out = loop(trainer, venv, args.steps, log=log, eps_decay=float(eps.get("decay", 10000)),
               eps_start=float(eps.get("start", 1.0)), eps_end=float(eps.get("end", 0.01)),
               share_replay=args.share_replay, steps_done0=steps_done0, every=every, on_every=on_every, **kw)
    if ctx.rank == 0:
        os.makedirs(args.save_dir, exist_ok=True)
        checkpoint(args.steps, out["steps_done"])
        np.save(os.path.join(args.save_dir, prefix + "step_rewards.npy"), out["rewards"])
        yaml.safe_dump(cfg, open(os.path.join(args.save_dir, "config.yaml"), "w"))
        for a, c in enumerate(cfgs[1:], 1):      # (several airfoils: config.yaml is airfoil 0's, config_<a>.yaml the others')
            yaml.safe_dump(c, open(os.path.join(args.save_dir, f"config_{a}.yaml"), "w"))
        print(f"ranks {ctx.world}: {args.steps} batched steps x {args.envs} envs/rank, mean reward {out['rewards'].mean():.4f}")
        if "reasons" in out and out["reasons"].size:     # (device loop) what ended the episodes of this rank, by reason bit
            names = {1: "drag", 2: "lift", 4: "vertex goal", 8: "failed step", 16: "step limit", 32: "mesh quality"}
            ends = ", ".join(f"{n} {int((out['reasons'] & b != 0).sum())}" for b, n in names.items())
            print(f"episode ends: {int((out['reasons'] != 0).sum())} ({ends})")
        if ctx.backend:
            print(f"process group: backend {ctx.backend}, {ctx.world} rank(s)")
    ctx.close()


if __name__ == "__main__":
    main()
