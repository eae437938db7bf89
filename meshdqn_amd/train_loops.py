"""The learning loops of the DQN trainer and their on-disk log.  The loops decide WHEN things happen; the replay stores
(replay.py) decide where records go and which are sampleable, `DQNTrainer` (trainer.py) owns the learning step."""
from __future__ import annotations

import math
import os
import random
from typing import TYPE_CHECKING, Optional

import numpy as np
import torch

from ._lib import MeshDQNHipError
from .dist_context import allgather_records, allgather_records_into, allgather_transitions
from .gcn_fused import FusedGcn
from .replay import DeviceReplay, SharedDeviceReplay, Transition, pack_transitions_device, state_refs
from .streams import concurrent_stream, role_streams, same_stream

if TYPE_CHECKING:
    from .trainer import DQNTrainer


def epsilon_threshold(steps_done, start=1.0, end=0.01, decay=10000):
    """airfoil_dqn.py:455."""
    return end + (start - end) * math.exp(-steps_done / decay)


class TrainingLog:
    """The reference's on-disk training log (DataHandler, airfoil_dqn.py:79-133): `reward.npy` (sum per episode),
    `rewards.npy` / `actions.npy` (per-episode lists), `losses.npy`, `eps.npy`, written under `save_dir + prefix`;
    `restart=True` continues from existing files and switches to the `RESTART_` prefix like the reference."""
    FILES = dict(rewards="reward.npy", ep_rewards="rewards.npy", losses="losses.npy", actions="actions.npy", epss="eps.npy",
                 airfoils="airfoil.npy")

    def __init__(self, save_dir: str, prefix: str = "", restart: bool = False, restart_num: int = 1):
        self.base = os.path.join(save_dir, prefix)
        self.rewards, self.ep_rewards, self.losses, self.actions, self.epss = [], [], [], [], []
        # a batch over several airfoils (VecEnv2DAirfoil with a list of configs): the airfoil of every finished episode,
        # `airfoil.npy` beside `reward.npy` (not written by single-airfoil runs)
        self.airfoils = []
        if restart:
            # the n-th restart reads the files of restart n - 1 and writes with one more prefix (airfoil_dqn.py:87-110)
            self.base += "RESTART_" * (max(int(restart_num), 1) - 1)
            for attr, fn in self.FILES.items():
                try:
                    setattr(self, attr, list(np.load(self.base + fn, allow_pickle=True)))
                except OSError:
                    pass
            self.base += "RESTART_"

    def add_eps(self, eps):
        self.epss.append(float(eps))

    def add_loss(self, loss):
        self.losses.append(float(loss))

    def add_episode(self, ep_rewards, ep_actions, airfoil=None):
        self.rewards.append(float(sum(ep_rewards)))
        self.ep_rewards.append(list(ep_rewards))
        self.actions.append(list(ep_actions))
        if airfoil is not None:
            self.airfoils.append(int(airfoil))

    def write(self):
        os.makedirs(os.path.dirname(self.base) or ".", exist_ok=True)
        np.save(self.base + "reward.npy", np.array(self.rewards))
        np.save(self.base + "rewards.npy", np.array(self.ep_rewards, dtype=object), allow_pickle=True)
        np.save(self.base + "losses.npy", np.array(self.losses))
        np.save(self.base + "actions.npy", np.array(self.actions, dtype=object), allow_pickle=True)
        np.save(self.base + "eps.npy", np.array(self.epss))
        if self.airfoils:
            np.save(self.base + "airfoil.npy", np.array(self.airfoils, dtype=np.int64))


def _refuse_prioritized(trainer, loop: str):
    """Prioritized replay draws with priorities that change with every optimiser step: only the device loop, whose draw is a
    kernel of the optimiser chain, offers it."""
    if trainer.prioritized is not None:
        raise ValueError(f"{loop} samples its replay uniformly on the host: a trainer with prioritized replay "
                         "(DQNTrainer(prioritized=...)) needs train_loop_device")


def _refuse_n_step(trainer, loop: str):
    """N-step targets are composed from the device ring, whose groups keep the environments' lane order (record j + W is the
    successor of record j); the host replay stores keep no such order."""
    if trainer.n_step > 1:
        raise ValueError(f"{loop} samples a host replay store that keeps no lane order: a trainer with n-step returns "
                         "(DQNTrainer(n_step=...)) needs train_loop_device")


def _refuse_target_net(trainer, what: str):
    """The target network's selection and refresh are launches of the device loop's optimiser chain; the host paths restate
    the reference's toggle, in which policy_net_2 is a second learner and not a copy."""
    if trainer.target_net is not None:
        raise ValueError(f"{what} restates the reference's toggle between two learners: a trainer with a target network "
                         "(DQNTrainer(target_net=...)) needs train_loop_device")


def _refuse_noisy(trainer, what: str):
    """Noisy networks get their noise from the pack launch of a device copy; the host paths run the torch modules, which
    would be the mean networks without any exploration."""
    if trainer.noisy is not None:
        raise ValueError(f"{what} runs the torch modules, which carry no noise: a trainer with noisy networks "
                         "(DQNTrainer(noisy=...)) needs train_loop_device")


def _draw_epsilon(steps_done, n_actions: int, eps_start, eps_end, eps_decay):
    """Host random numbers of one batched step (both batched loops): epsilon per env, who explores, the random actions."""
    eps = eps_end + (eps_start - eps_end) * np.exp(-1.0 * steps_done / eps_decay)
    steps_done += 1
    explore = np.random.random(len(steps_done)) <= eps
    return eps, explore, np.random.randint(0, n_actions + 1, len(steps_done))


class _EpisodeLog:
    """The running episode of every environment of a batched loop, handed to the `TrainingLog` (if any) when it ends."""

    def __init__(self, log: Optional["TrainingLog"], venv):
        self.log, self.venv = log, venv
        self.ep_r, self.ep_a = [[] for _ in range(venv.B)], [[] for _ in range(venv.B)]

    def add_step(self, eps_mean: float, actions, rew, done):
        if self.log is None:
            return
        self.log.add_eps(eps_mean)
        for b in range(self.venv.B):
            self.ep_r[b].append(float(rew[b]))
            self.ep_a[b].append(int(actions[b]))
            if done[b]:
                self.log.add_episode(self.ep_r[b], self.ep_a[b], int(self.venv.airfoil[b]) if self.venv.A > 1 else None)
                self.ep_r[b], self.ep_a[b] = [], []


def train_loop_per_worker(trainer: DQNTrainer, env_factory, num_episodes: int, max_steps: Optional[int] = None,
                          eps_decay=10000, eps_start=1.0, eps_end=0.01, share_replay=False, e_max=None):
    """Rollout loop of one rank (airfoil_dqn.py:428-503): epsilon-greedy over N_closest+1 actions, push the
    transition, optimise, rebuild the env every episode.  Returns per-episode reward lists.

    With more than one rank every step issues collectives (the gradient all-reduce of `optimize`, the transition
    all-gather), so all ranks must take the SAME number of steps: episode lengths differ between ranks (per-rank
    seeds), hence the loop must be bounded by `max_steps` (episodes are then cut at that common step count)."""
    _refuse_prioritized(trainer, "train_loop_per_worker")
    _refuse_n_step(trainer, "train_loop_per_worker")
    _refuse_target_net(trainer, "train_loop_per_worker")
    _refuse_noisy(trainer, "train_loop_per_worker")
    ctx = trainer.ctx
    if ctx.world > 1 and max_steps is None:
        raise ValueError("train_loop_per_worker with more than one rank needs max_steps (a step count common to all "
                         "ranks): ranks that finish their episodes early would leave the others blocked in a collective")
    if ctx.world > 1:
        num_episodes = max(num_episodes, max_steps)   # the step count, not the episode count, ends the loop
    e_max = trainer.e_max if e_max is None else int(e_max)
    n_actions = trainer.n_actions
    steps_done = 0
    env = env_factory()
    history = []
    total = 0
    for episode in range(num_episodes):
        if episode != 0:
            env = env_factory()
        state = env.get_state()
        ep_rewards, ep_actions = [], []
        while True:
            sample = np.random.random()
            eps = epsilon_threshold(steps_done, eps_start, eps_end, eps_decay)
            steps_done += 1
            if sample > eps:
                action = trainer.select_action(state)
            else:
                action = random.sample(range(n_actions + 1), 1)[0]
            next_state, reward, done, _ = env.step(action)
            ep_rewards.append(reward)
            ep_actions.append(action)
            tr = Transition(state, torch.tensor([[action]], dtype=torch.long), None if done else next_state,
                            torch.tensor([reward], dtype=torch.float32))
            if share_replay and ctx.multi:
                for t in allgather_transitions(ctx, [tr], state.x.shape[0], state.x.shape[1], e_max):
                    trainer.memory.push(*t)
            else:
                trainer.memory.push(*tr)
            state = next_state
            trainer.optimize()
            total += 1
            if done or (max_steps is not None and total >= max_steps):
                break
        history.append((ep_rewards, ep_actions))
        if max_steps is not None and total >= max_steps:
            break
    return history


def train_loop_vec(trainer: DQNTrainer, venv, num_steps: int, optim_per_step: int = 1, eps_decay=10000, eps_start=1.0,
                   eps_end=0.01, share_replay=False, e_max=1536, log: Optional["TrainingLog"] = None,
                   device_replay: bool = True, overlap_optimise: bool = True, steps_done0=None, every: int = 0,
                   on_every=None):
    """Batched counterpart of `train_loop_per_worker` for one rank: B environments of a `VecEnv2DAirfoil` stepped
    together (configs[3] of BASELINE.json: 128 envs per GPU, 1024 over 8 ranks).  Per batched step: fused Q-forward
    of policy_net_1 for all B states, epsilon-greedy per environment (per-env step counters, like the reference's
    per-worker `steps_done`), `venv.step`, B transitions into the replay ring (optionally all-gathered over the
    ranks), `optim_per_step` optimiser steps (each with ONE flat gradient all-reduce).  Terminated environments are
    reset in place by the vector env.  `steps_done0` continues the per-environment epsilon counters of an earlier run;
    `on_every(step, steps_done)` is called after every `every`-th batched step (periodic checkpoints / log writes).
    Returns dict(rewards (num_steps,B), dones, losses, steps_done)."""
    _refuse_prioritized(trainer, "train_loop_vec")
    _refuse_n_step(trainer, "train_loop_vec")
    _refuse_target_net(trainer, "train_loop_vec")
    _refuse_noisy(trainer, "train_loop_vec")
    ctx = trainer.ctx
    B, N = venv.B, venv.N
    fused = FusedGcn(trainer.policy_net_1)
    steps_done = np.zeros(B, np.int64) if steps_done0 is None else np.asarray(steps_done0, np.int64).copy()
    st = venv.get_state()
    # GPU-resident replay (states stored once per batched step, minibatches gathered on the device) whenever the
    # environment hands out its padded edge lists; the per-transition list of lazy references otherwise (and when the
    # ranks exchange transitions)
    rep_dev = rep_sh = None
    dev_ok = device_replay and trainer.graphs and trainer.dense and DeviceReplay.eligible(st, trainer.e_max)
    if dev_ok and share_replay and ctx.multi:
        # shared replay: every rank keeps ALL transitions as fixed-size records on its device; per batched step ONE
        # all-gather of the (B, record) tensor packed on the device
        rep_sh = trainer.device_memory
        if not isinstance(rep_sh, SharedDeviceReplay):
            rep_sh = trainer.device_memory = SharedDeviceReplay(trainer.replay_capacity, N, st["x"].shape[2], trainer.e_max,
                                                                ctx.device)

        def snapshot(st_):     # (the padded edge lists are views of buffers the next env step rewrites)
            return dict(x=st_["x"], edge_src_pad=st_["edge_src_pad"].clone(), edge_dst_pad=st_["edge_dst_pad"].clone(),
                        nedges=np.array(st_["nedges"]))
        prev_pack = snapshot(st)
    elif dev_ok:
        rep_dev = trainer.device_memory
        if not isinstance(rep_dev, DeviceReplay) or (rep_dev.B, rep_dev.N, rep_dev.F) != (B, N, st["x"].shape[2]):
            rep_dev = trainer.device_memory = DeviceReplay(trainer.replay_capacity, B, N, st["x"].shape[2], trainer.e_max,
                                                           ctx.device)
        base_prev = rep_dev.store(st)
    # the optimiser step runs on a second stream between the two halves of the environment step: its launches and
    # host work overlap the (latency-bound, half-chip) smoothing kernel; it samples the replay as of the previous step
    # (`venv` is a `VecEnv2DAirfoil` in both batched loops - `VecEnvGroups` has no `get_state` / `step` and drives its
    # groups itself - so every env member is a plain read: no `hasattr` check is left)
    overlap = overlap_optimise and rep_dev is not None and ctx.device.type == "cuda"
    if overlap:
        if trainer._opt_stream is None:
            trainer._opt_stream = concurrent_stream(ctx.device, [venv._flow_stream])
        opt_stream, ev_store = trainer._opt_stream, torch.cuda.Event()
        ev_store.record(torch.cuda.current_stream(ctx.device))
    rewards, dones_hist = [], []
    episodes = _EpisodeLog(log, venv)
    for step_no in range(num_steps):
        with torch.no_grad():
            q = fused.forward_arrays(st["x"], st["node_ptr"], st["esrc"], st["edst"], st["edge_ptr"], N, venv.EMAX,
                                     edge_counts=st["nedges"])
        greedy = q.argmax(1).cpu().numpy()
        eps, explore, rand_act = _draw_epsilon(steps_done, trainer.n_actions, eps_start, eps_end, eps_decay)
        actions = np.where(explore, rand_act, greedy)
        if overlap:
            venv.step_begin(actions)
            opt_stream.wait_event(ev_store)            # (the ring rows written by the last store)
            with torch.cuda.stream(opt_stream):
                for _k in range(optim_per_step):
                    loss = trainer.optimize()
                    if log is not None and loss is not None:
                        log.add_loss(loss)
            st, rew, done, _ = venv.step_end()
            torch.cuda.current_stream(ctx.device).wait_stream(opt_stream)   # the next Q-forward reads the new weights
            base_next = rep_dev.store(st)
            ev_store.record(torch.cuda.current_stream(ctx.device))
        elif rep_dev is not None:
            st, rew, done, _ = venv.step(actions)
            base_next = rep_dev.store(st)
        elif rep_sh is not None:
            st, rew, done, _ = venv.step(actions)
            rec = pack_transitions_device(prev_pack, st, actions, rew, done, trainer.e_max)
            rep_sh.push_records(allgather_records(ctx, rec))
            prev_pack = snapshot(st)
        else:
            prev = state_refs(st)
            st, rew, done, _ = venv.step(actions)
            nxt = state_refs(st)
            a_t = torch.from_numpy(np.asarray(actions, np.int64)).reshape(B, 1, 1).unbind(0)
            r_t = torch.from_numpy(np.asarray(rew, np.float32)).reshape(B, 1).unbind(0)
            trs = [Transition(prev[b], a_t[b], None if done[b] else nxt[b], r_t[b]) for b in range(B)]
            if share_replay and ctx.multi:
                trs = allgather_transitions(ctx, trs, N, st["x"].shape[2], e_max)
            for t in trs:
                trainer.memory.push(*t)
        if rep_dev is not None:
            rep_dev.push(base_prev, base_next, actions, rew, done)
            base_prev = base_next
        for _k in range(0 if overlap else optim_per_step):
            loss = trainer.optimize()
            if log is not None and loss is not None:
                log.add_loss(loss)
        episodes.add_step(float(eps.mean()), actions, rew, done)
        rewards.append(rew.copy())
        dones_hist.append(done.copy())
        if every and on_every is not None and (step_no + 1) % every == 0:
            on_every(step_no + 1, steps_done)
    return dict(rewards=np.array(rewards), dones=np.array(dones_hist), losses=list(trainer.losses), steps_done=steps_done)


def train_loop_device(trainer: DQNTrainer, venv, num_steps: int, optim_per_step: int = 1, eps_decay=10000, eps_start=1.0,
                      eps_end=0.01, share_replay=False, log: Optional["TrainingLog"] = None, steps_done0=None, every: int = 0,
                      on_every=None, chunk: int = 64, optimiser_stream: str = "auto", per_trace: bool = False,
                      nstep_trace: bool = False, target_trace: bool = False):
    """`train_loop_vec` WITHOUT a host round trip inside a batched step (one rank of configs[3]): the environment step is
    `VecEnv2DAirfoil.rollout_step` (Q-forward, epsilon-greedy choice, vertex removal ... reward / reset logic as kernels),
    the B transitions go into the record ring with one launch (`mdq_replay_step`; with `share_replay` the ranks
    all-gather their B records per step), and the optimiser step (`DQNTrainer.optimize_device`: replay sampling,
    hand-written forward + backward, flat gradient all-reduce, Adam as kernels) runs on a side stream beside the
    latency-bound smoothing kernel of the same env step (`optimiser_stream`: the env's flow stream, behind the flow
    leg of the previous step, or a stream of its own).  The host only draws the random numbers (same streams as
    `train_loop_vec`: numpy for epsilon-greedy, `random.sample` for the minibatch) and enqueues; rewards / dones /
    losses are read back once per `chunk` steps.  Same returns as `train_loop_vec`.

    With a prioritized trainer (`DQNTrainer(prioritized=...)`) the minibatches are drawn ON THE DEVICE, because the
    priorities change with every optimiser step: the host uploads one table of uniforms per chunk (`random.random()`, one per
    draw) instead of record numbers, and the optimiser chain of step t becomes `prio_fill` (the group that just got its next
    states: largest priority so far; the group being written: 0), the all-gather, and per optimiser step `prio_draw` ->
    `optimize_device` with the drawn device indices and importance weights -> `prio_update` from the TD errors.  All of it on
    the optimiser stream: the main chain gains no launch and no event.  Over several ranks with `share_replay` the ring
    stays identical on all ranks; the priorities are rank-local (every rank learns from its own minibatch, the gradient is
    all-reduced as before).  `per_trace=True` adds out["per"]: `u`, `idx`, `weight`, `td` (minibatches, batch) and `beta`
    (minibatches,) of every minibatch of the call, in order, read back with the losses at the chunk boundaries.

    With `DQNTrainer(n_step=n)`, n > 1, the sampling launch of every minibatch of step t composes n-step transitions from the
    ring (`mdq_replay_sample_nstep`, head = the group step t writes); the host draw and the prioritized chain do not change -
    a drawn record is never in the head group, and its priority comes from the n-step TD error.  The walk needs no new event
    or stream dependency: the optimiser chain of step t already runs behind the event recorded after `rep.step` of step t,
    which finished group t - 1; the main stream already waits for that chain (`ev_opt`) before the next `rep.step`, the only
    writer of the ring on it; with `share_replay` the all-gather of group t - 1 precedes the minibatches on the optimiser
    stream itself.  So every record a walk can reach (the groups of steps t - G + 1 .. t - 1) is finished and stable while
    the walk reads it.  `nstep_trace=True` (refused for n_step = 1) adds out["nstep"]: `idx`, `reward`, `nonfinal`, `steps`
    (minibatches, batch) and `head` (minibatches,), the first record of the head group, read back like the `per` trace.

    With `DQNTrainer(target_net=...)` policy_net_1 is the one online network and policy_net_2 its target (see
    `optimize_device`): one more forward and the select launch (kind "double") in front of the learning step, and every
    `period` gradient steps the target update behind `mdq_adam_step`, all on the optimiser stream.  No new stream or event:
    the train-role copies of both networks are repacked on that stream, in order with the kernels that write the
    parameters; the acting copy belongs to policy_net_1 and follows it as before.  `target_trace=True` (kind "double" only)
    adds out["target"]: `sel` (int32) and `value` (float32), (minibatches, batch): the action the online network chose in
    every next state and the target network's value of it, read back like the `per` trace.

    With `DQNTrainer(noisy=...)` exploration is the networks' own: where the acting copy follows the parameters (below) it is
    packed with fresh noise instead (`mdq_gcn_pack_noisy` in place of `mdq_gcn_pack`: no launch more), one draw per batched
    step shared by the B environments; `explore` is all false, no epsilon is drawn (the host's numpy stream is not
    touched, the logged epsilon is 0, the step counters still count) and the optimiser chain resamples its own copies
    (`optimize_device`).  At the end the acting copy is told to drop its noise: `select_action` and `deploy` see the mean."""
    ctx = trainer.ctx
    dev = ctx.device
    per = trainer.prioritized
    if per_trace and per is None:
        raise ValueError("per_trace needs a trainer with prioritized replay")
    if target_trace and (trainer.target_net is None or trainer.target_net["kind"] != "double"):
        raise ValueError("target_trace needs a trainer with target_net kind 'double'")
    n_step = trainer.n_step
    if nstep_trace and n_step == 1:
        raise ValueError("nstep_trace needs a trainer with n_step > 1")
    if dev.type != "cuda" or not venv.gpu_remesh or not venv.auto_reset:
        raise MeshDQNHipError("train_loop_device needs a GPU and a vector env with the device mesh engine and auto_reset")
    B, N = venv.B, venv.N
    W = B * ctx.world if (share_replay and ctx.multi) else B     # records per batched step in this rank's ring
    steps_done = np.zeros(B, np.int64) if steps_done0 is None else np.asarray(steps_done0, np.int64).copy()
    fused1 = trainer._fused_of(trainer.policy_net_1)
    main = torch.cuda.current_stream(dev)
    if main == torch.cuda.default_stream(dev):
        # the loop does not run on the legacy default stream (see VecEnv2DAirfoil.rollout_device): a stream of its own
        if trainer._main_stream is None:
            trainer._main_stream = role_streams(dev)["main"]
        trainer._main_stream.wait_stream(main)
        with torch.cuda.stream(trainer._main_stream):
            out = train_loop_device(trainer, venv, num_steps, optim_per_step=optim_per_step, eps_decay=eps_decay,
                                    eps_start=eps_start, eps_end=eps_end, share_replay=share_replay, log=log,
                                    steps_done0=steps_done0, every=every, on_every=on_every, chunk=chunk,
                                    optimiser_stream=optimiser_stream, per_trace=per_trace, nstep_trace=nstep_trace,
                                    target_trace=target_trace)
        main.wait_stream(trainer._main_stream)
        return out
    if venv.flow_overlap and not same_stream(venv._calibrated_for, main):
        venv.calibrate_streams(fused1)       # (a flow stream that really overlaps with this loop's stream; resets the envs)
    # "auto" and "own": a stream of its own.  (With the 1.8 ms smoothing walk the optimiser chain rode on the flow stream behind the flow
    # leg - 1.05 + 0.6 ms still ended before the main chain; since the blocked smoothing solve the main chain is 1.16 ms and
    # that placement costs 1.63 ms per batched step against 1.41 ms with a third stream: tools/time_train_device.py.)
    on_flow = optimiser_stream == "flow" and venv.flow_overlap
    if on_flow:
        # the optimiser chain rides on the (calibrated) flow stream, behind the flow leg of the previous env step: one side
        # stream instead of two
        opt_stream = venv._flow_stream
    else:
        if trainer._opt_stream is None:
            trainer._opt_stream = role_streams(dev)["opt"]
        ocal = trainer._opt_calibrated_for
        if ocal is None or not same_stream(ocal[0], main) or not same_stream(ocal[1], venv._flow_stream):
            trainer.calibrate_opt_stream(venv, fused1)    # (an optimiser stream that really overlaps; resets the envs)
        opt_stream = trainer._opt_stream
    ev_opt = rep = None
    trace = dict(u=[], idx=[], weight=[], td=[], beta=[])
    ntrace = dict(idx=[], reward=[], nonfinal=[], steps=[], head=[])
    ttrace = dict(sel=[], value=[])
    rewards, dones_hist, actions_hist, reasons_hist = [], [], [], []
    episodes = _EpisodeLog(log, venv)
    step_no, prev = 0, None      # prev: (record base, act, rew, done) of the step whose records await their next state
    while step_no < num_steps:
        K = min(int(chunk), num_steps - step_no)
        # random numbers of the chunk, drawn step by step in train_loop_vec's order
        explore, rand_act, eps_mean = np.zeros((K, B), bool), np.zeros((K, B), np.int32), []
        for k in range(K):
            if trainer.noisy is not None:       # no epsilon-greedy: `explore` stays all false
                steps_done += 1
                eps_mean.append(0.0)
                continue
            eps, explore[k], rand_act[k] = _draw_epsilon(steps_done, trainer.n_actions, eps_start, eps_end, eps_decay)
            eps_mean.append(float(eps.mean()))
        ro = venv.rollout_begin(K, explore, rand_act)
        st = ro["state"]
        if rep is None:
            if st["edge_src_pad"].shape[1] != trainer.e_max:
                raise ValueError(f"vector env pads edge lists to {st['edge_src_pad'].shape[1]}, trainer.e_max is {trainer.e_max}")
            rep = trainer.device_memory = SharedDeviceReplay.grouped(trainer.device_memory, trainer.replay_capacity, W, N,
                                                                     st["x"].shape[2], trainer.e_max, dev)
            t0 = rep.steps_pushed                               # the ring continues where an earlier call stopped
            loss_ring = torch.zeros(int(chunk) * max(1, optim_per_step), dtype=torch.float32, device=dev)
            if per is not None:     # what the draw and the learning step hand each other, a row per minibatch of a chunk
                shape = (loss_ring.numel(), trainer.batch_size)
                per_idx = torch.zeros(shape, dtype=torch.int32, device=dev)
                per_w, per_td = torch.zeros(shape, device=dev), torch.zeros(shape, device=dev)
            if nstep_trace:         # what the sampling launch composed, a row per minibatch of a chunk
                shape = (loss_ring.numel(), trainer.batch_size)
                ns_steps = torch.zeros(shape, dtype=torch.int32, device=dev)
                ns_rew, ns_nf = torch.zeros(shape, device=dev), torch.zeros(shape, device=dev)
            if target_trace:        # what the select launch chose, a row per minibatch of a chunk
                shape = (loss_ring.numel(), trainer.batch_size)
                tg_sel, tg_val = torch.zeros(shape, dtype=torch.int32, device=dev), torch.zeros(shape, device=dev)
        # minibatches of the chunk: the number of finished records at every step is known in advance; one upload
        if per is None:
            mbs = [rep.draw(t, trainer.batch_size) for t in range(t0 + step_no, t0 + step_no + K)
                   for _k in range(optim_per_step if rep.finished(t) >= trainer.batch_size else 0)]
            mb_dev = torch.from_numpy(np.stack(mbs)).to(dev) if mbs else None
        else:                       # ... of the uniforms of every draw
            n_mb = sum(optim_per_step for t in range(t0 + step_no, t0 + step_no + K) if rep.finished(t) >= trainer.batch_size)
            u_host = np.array([random.random() for _ in range(n_mb * trainer.batch_size)], np.float64).reshape(n_mb, trainer.batch_size)
            u_dev = torch.from_numpy(u_host).to(dev) if n_mb else None
            betas = []
        heads = []
        n_loss = 0
        for k in range(K):
            t = t0 + step_no + k
            if ev_opt is not None:
                main.wait_event(ev_opt)                        # the weights of the previous optimiser step
            # the ACTING copy follows the parameters here and only here: behind the event of the last optimiser chain and
            # in front of the next one (which waits for `ev` below); rollout_step must not repack (pack=False): by then
            # the host has already bumped the version for an Adam kernel that is still in flight on the other stream
            if trainer.noisy is None:
                fused1._pack()
            else:                               # ... with this step's noise: one draw for the B environments
                trainer.resample("act1")
            base_cur = rep.group_base(t) + (ctx.rank * B if W != B else 0)     # this rank's B records of the step's group
            rep.step(st, base_cur, prev)
            ev = torch.cuda.Event()
            ev.record(main)
            gather = prev is not None and W != B               # shared replay: everybody's finished records of that step
            do_opt = rep.finished(t) >= trainer.batch_size
            if gather or do_opt or per is not None:
                with torch.cuda.stream(opt_stream):
                    opt_stream.wait_event(ev)
                    if per is not None:
                        rep.prio_fill(t, new=prev is not None)     # every step, also before the ring holds a minibatch
                    if gather:
                        # on the optimiser stream, in front of the chain that may sample those records, in place in the ring
                        # (rank r's B records sit at group base + r * B on every rank): off the latency chain of the env step
                        allgather_records_into(ctx, rep.R, prev[0], B, W)
                    for _k in range(optim_per_step if do_opt else 0):
                        nkw = dict(head_step=t, steps_out=ns_steps[n_loss] if nstep_trace else None) if n_step > 1 else {}
                        if target_trace:
                            nkw.update(sel_out=tg_sel[n_loss], value_out=tg_val[n_loss])
                        if per is None:
                            trainer.optimize_device(rep, mb_dev[n_loss], loss_out=loss_ring[n_loss:n_loss + 1], **nkw)
                        else:
                            betas.append(trainer.beta())
                            rep.prio_draw(u_dev[n_loss], betas[-1], per_idx[n_loss], per_w[n_loss])
                            trainer.optimize_device(rep, per_idx[n_loss], loss_out=loss_ring[n_loss:n_loss + 1],
                                                    weight=per_w[n_loss], td_out=per_td[n_loss], **nkw)
                            rep.prio_update(per_idx[n_loss], per_td[n_loss], per["alpha"], per["eps"])
                        if nstep_trace:     # (the minibatch buffers are rewritten by the next sampling launch)
                            ns_rew[n_loss].copy_(trainer._mb_bufs["reward"])
                            ns_nf[n_loss].copy_(trainer._mb_bufs["nonfinal"])
                            heads.append(rep.group_base(t))
                        n_loss += 1
                    ev_opt = torch.cuda.Event()
                    ev_opt.record(opt_stream)
            venv.rollout_step(ro, fused1, pack=False)
            prev = (base_cur, ro["act"][k], ro["rew"][k], ro["done"][k])
            st = ro["state"]
        if step_no + K >= num_steps and prev is not None:       # last chunk: finish the records of the last step too
            rep.step(st, prev=prev)
            if W != B:
                if ev_opt is not None:
                    main.wait_event(ev_opt)
                allgather_records_into(ctx, rep.R, prev[0], B, W)
            if per is not None:     # the last step's records are finished too: their priorities, on the optimiser stream
                ev = torch.cuda.Event()
                ev.record(main)
                with torch.cuda.stream(opt_stream):
                    opt_stream.wait_event(ev)
                    rep.prio_fill(t0 + num_steps, zero=False)
                    ev_opt = torch.cuda.Event()
                    ev_opt.record(opt_stream)
            rep.close(t0 + num_steps)
        out = venv.rollout_end(ro)                              # the one synchronisation of the chunk
        if ev_opt is not None:
            ev_opt.synchronize()                                # (the last optimiser chain writes its loss on the side stream)
        new_losses = loss_ring[:n_loss].cpu().numpy().tolist()
        trainer.losses.extend(new_losses)
        if per_trace:
            trace["u"].append(u_host[:n_loss])
            for key, ring in (("idx", per_idx), ("weight", per_w), ("td", per_td)):
                trace[key].append(ring[:n_loss].cpu().numpy())
            trace["beta"].append(np.asarray(betas[:n_loss], np.float64))
        if nstep_trace:
            ntrace["idx"].append(per_idx[:n_loss].cpu().numpy() if per is not None else
                                 (np.stack(mbs) if mbs else np.zeros((0, trainer.batch_size), np.int32)))
            for key, ring in (("reward", ns_rew), ("nonfinal", ns_nf), ("steps", ns_steps)):
                ntrace[key].append(ring[:n_loss].cpu().numpy())
            ntrace["head"].append(np.asarray(heads, np.int64))
        if target_trace:
            ttrace["sel"].append(tg_sel[:n_loss].cpu().numpy())
            ttrace["value"].append(tg_val[:n_loss].cpu().numpy())
        for k in range(K):
            rew, done = out["rewards"][k], out["dones"][k]
            rewards.append(rew.copy())
            dones_hist.append(done.copy())
            actions_hist.append(out["actions"][k].copy())
            reasons_hist.append(out["reasons"][k].copy())
            episodes.add_step(eps_mean[k], out["actions"][k], rew, done)
        if log is not None:
            for l_ in new_losses:
                log.add_loss(l_)
        step_no += K
        if every and on_every is not None and (step_no // every) > ((step_no - K) // every):
            on_every(step_no, steps_done)
    fused1.denoise()                # (a no-op for a copy that never carried noise)
    out = dict(rewards=np.array(rewards), dones=np.array(dones_hist), losses=list(trainer.losses), steps_done=steps_done,
               actions=np.array(actions_hist), reasons=np.array(reasons_hist))     # (reasons: reward.REASON_* per step)
    if per_trace:
        out["per"] = {key: np.concatenate(v) if v else np.zeros(0) for key, v in trace.items()}
    if nstep_trace:
        out["nstep"] = {key: np.concatenate(v) if v else np.zeros(0) for key, v in ntrace.items()}
    if target_trace:
        out["target"] = {key: np.concatenate(v) if v else np.zeros(0) for key, v in ttrace.items()}
    return out
