"""Data-parallel DQN trainer: the counterpart of the reference's Ray rollout / parameter-server loop
(airfoil_dqn.py:46-67 replay, :151-340 parameter server + gradient worker, :428-503 rollout).

MI355X-first re-design: one process per GPU (torchrun), every rank owns its
environments, a replica of both Q-networks and a replay shard; per optimiser step ONE flat fp32
all-reduce of the 173 493 gradients over RCCL (`torch.distributed`, backend "nccl"; "gloo" on CPU for
the tests) replaces the parameter server, and an optional all-gather of fixed-size transition records
replaces the central replay actor.  No Ray.

Kept from the reference: Transition tuple, ring replay of 10 000, epsilon schedule
0.01 + 0.99 exp(-t/10000) per worker, double DQN with the selected net toggled every `target_update`
gradient applications, Huber loss, gamma, Adam(lr 1e-5, wd 1e-6) + MultiStepLR[5e5,1e6,1.5e6] x0.1,
softmax outputs used as Q-values.  Deliberately NOT kept (bugs of the published script):
the Adam optimiser is persistent per network instead of being re-created on every call, and
`optimizer.step()` runs after the new gradients are set, not before (airfoil_dqn.py:188-199).
"""
from __future__ import annotations

import ctypes as C
import os
import random
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from . import streams as _st
from .airfoilgcnn import NodeRemovalNet, check_head, dense_batch
from .data import Batch
# (besides what this module uses: every name other modules, the tools and the tests import from here)
from .dist_context import DistContext, allgather_records, allgather_records_into, allgather_transitions  # noqa: F401
from .gcn_fused import fused_of
from .replay import (DeviceBatch, DeviceReplay, ReplayMemory, SharedDeviceReplay, StateRef, Transition,  # noqa: F401
                     gather_state_refs, pack_transitions, pack_transitions_device, state_refs, state_to_data_list,
                     unpack_transitions)
from .train_loops import (TrainingLog, _refuse_noisy, _refuse_target_net, epsilon_threshold, train_loop_device,  # noqa: F401
                          train_loop_per_worker, train_loop_vec)


class DQNTrainer:
    def __init__(self, n_actions: int, num_inputs: int, ctx: Optional[DistContext] = None, lr=1e-5, weight_decay=1e-6,
                 batch_size=32, gamma=1.0, target_update=50, replay_capacity=10000, conv_width=128, topk=0.1,
                 seed=1370, dense: bool = True, e_max: int = 1536, prioritized: Optional[dict] = None, n_step: int = 1,
                 target_net: Optional[dict] = None, head: str = "softmax", noisy: Optional[dict] = None):
        self.head = check_head(head)                       # the Q-head of both networks (a constructor option too)
        self.noisy = self._check_noisy(noisy, seed)        # noisy dense heads of both networks (a constructor option too)
        self.prioritized = self._check_prioritized(prioritized, batch_size)
        self.n_step = self._check_n_step(n_step)           # a constructor option like `prioritized`: not checkpointed
        self.target_net = self._check_target_net(target_net, target_update)     # ... and so is this one
        self.ctx = ctx or DistContext()
        self.dense, self.e_max = bool(dense), int(e_max)   # static-shape autograd path for equal-sized graphs
        dev = self.ctx.device
        self.graphs = dev.type == "cuda"                   # replay forward + backward as a HIP graph when possible
        self._graphs, self._graph_error = {}, None
        torch.manual_seed(seed)  # identical initial replicas on every rank (airfoil_dqn.py:28-32)
        nkw = {} if self.noisy is None else dict(noisy=self.noisy["sigma0"])
        self.policy_net_1 = NodeRemovalNet(n_actions + 1, conv_width=conv_width, topk=topk, head=self.head, **nkw).float()
        self.policy_net_2 = NodeRemovalNet(n_actions + 1, conv_width=conv_width, topk=topk, head=self.head, **nkw).float()
        self.policy_net_1.set_num_nodes(num_inputs)
        self.policy_net_2.set_num_nodes(num_inputs)
        self.policy_net_1.to(dev)
        self.policy_net_2.to(dev)
        if self.target_net is not None:
            # both networks were constructed in the default trainer's order (policy_net_1 has its bits from the same seed);
            # the target starts as a copy of the online network.  A later `load()` keeps whatever the checkpoint holds.
            self.policy_net_2.load_state_dict(self.policy_net_1.state_dict())
        self.n_actions, self.batch_size, self.gamma, self.target_update = n_actions, batch_size, gamma, target_update
        # (torch's fused=True Adam measured 4x slower than the foreach implementation on this ROCm build)
        self.opts = [torch.optim.Adam(n.parameters(), lr=lr, weight_decay=weight_decay)
                     for n in (self.policy_net_1, self.policy_net_2)]
        self.scheds = [torch.optim.lr_scheduler.MultiStepLR(o, milestones=[500000, 1000000, 1500000], gamma=0.1)
                       for o in self.opts]
        self.memory = ReplayMemory(replay_capacity)
        self.replay_capacity = replay_capacity
        self.device_memory = None   # DeviceReplay, created by train_loop_vec when the vector env provides padded edges
        self.criterion = torch.nn.HuberLoss()
        self.num_grads = 0
        self.select = True
        self.losses: List[float] = []
        # the device learner's lazily built state: streams of the loops (`train_loop_vec` / `train_loop_device`) and what
        # the optimiser stream was calibrated against, flat Adam moments per network, minibatch buffers of `optimize_device`
        self._opt_stream = self._main_stream = self._opt_calibrated_for = self._adam = self._mb_bufs = None
        self._target_desc = None    # descriptor of `mdq_target_update` (policy_net_2 <- policy_net_1), built on first use
        # noisy networks: the 64-bit draw counter of every packed copy that carries noise (checkpointed with the option on)
        self.noise_draws = {copy: 0 for copy in self.NOISE_COPIES}
        self.opt_calibration_ms: List[float] = []
        random.seed(seed + self.ctx.rank)
        np.random.seed(seed + self.ctx.rank)

    # --- prioritized replay (Schaul et al. 2016, proportional variant; `train_loop_device` only) ----------------
    PRIORITIZED_DEFAULTS = dict(alpha=0.6, beta0=0.4, beta_steps=100000, eps=1e-6)

    @classmethod
    def _check_prioritized(cls, prioritized, batch_size) -> Optional[dict]:
        """None, or the complete option dict: record i is drawn with probability p_i / sum p, p_i = (|td_i| + eps)^alpha;
        its loss term carries the importance weight (N p_i / sum p)^-beta over the largest one of the minibatch."""
        if prioritized is None:
            return None
        opt = dict(cls.PRIORITIZED_DEFAULTS)
        if not isinstance(prioritized, dict):
            raise ValueError("prioritized: None or a dict with any of " + ", ".join(opt))
        unknown = sorted(set(prioritized) - set(opt))
        if unknown:
            raise ValueError(f"prioritized: unknown option(s) {unknown}; known: " + ", ".join(opt))
        opt.update(prioritized)
        opt = dict(alpha=float(opt["alpha"]), beta0=float(opt["beta0"]), beta_steps=float(opt["beta_steps"]), eps=float(opt["eps"]))
        if not 0.0 <= opt["alpha"] <= 1.0:
            raise ValueError(f"prioritized: alpha {opt['alpha']} outside [0, 1]")
        if not 0.0 < opt["beta0"] <= 1.0:
            raise ValueError(f"prioritized: beta0 {opt['beta0']} outside (0, 1]")
        if not opt["beta_steps"] > 0:
            raise ValueError(f"prioritized: beta_steps {opt['beta_steps']} must be positive")
        if not (opt["eps"] > 0 and np.isfinite(opt["eps"])):
            raise ValueError(f"prioritized: eps {opt['eps']} must be positive")
        if int(batch_size) > 1024:
            raise ValueError(f"prioritized: batch_size {batch_size} exceeds the 1024 draws of mdq_replay_prio_draw")
        return opt

    # --- n-step returns (`train_loop_device` only: composed from the record ring inside the sampling launch) ------
    N_STEP_MAX = 64

    @classmethod
    def _check_n_step(cls, n_step) -> int:
        """The number of transitions a target spans: r_0 + g r_1 + ... + g^(m-1) r_(m-1) + g^m max_a Q(s_m, a), m <= n_step
        (fewer where the episode ends or the ring's newest finished group is reached).  1: the 1-step target."""
        if isinstance(n_step, bool) or not isinstance(n_step, (int, np.integer)):
            raise ValueError(f"n_step: an integer in 1 .. {cls.N_STEP_MAX}, not {n_step!r}")
        if not 1 <= int(n_step) <= cls.N_STEP_MAX:
            raise ValueError(f"n_step: {n_step} outside 1 .. {cls.N_STEP_MAX} (the walk of mdq_replay_sample_nstep)")
        return int(n_step)

    # --- target network and Double-DQN targets (`train_loop_device` only: two launches of the optimiser chain) ------
    TARGET_NET_KINDS = ("double", "max")

    @classmethod
    def _check_target_net(cls, target_net, target_update) -> Optional[dict]:
        """None (the reference's toggle: the two networks swap roles every `target_update` steps and never exchange
        weights), or the complete option dict: policy_net_1 is the one online network, trained on every step, and
        policy_net_2 a copy of it that follows every `period` gradient steps, by a copy (tau 1) or Polyak averaging
        (target += tau (online - target)).  kind "double": r + gamma^m Q_target(s', argmax_a Q_online(s', a)) (van Hasselt
        et al. 2016); "max": r + gamma^m max_a Q_target(s', a) (Mnih et al. 2015)."""
        if target_net is None:
            return None
        known = ("kind", "period", "tau")
        if not isinstance(target_net, dict):
            raise ValueError("target_net: None or a dict with any of " + ", ".join(known))
        unknown = sorted(set(target_net) - set(known), key=repr)
        if unknown:
            raise ValueError(f"target_net: unknown option(s) {unknown}; known: " + ", ".join(known))
        kind = target_net.get("kind", "double")
        if not isinstance(kind, str) or kind not in cls.TARGET_NET_KINDS:
            raise ValueError(f"target_net: kind {kind!r} is none of " + ", ".join(cls.TARGET_NET_KINDS))
        period = target_net.get("period", target_update)
        if isinstance(period, bool) or not isinstance(period, (int, np.integer)) or int(period) < 1:
            raise ValueError(f"target_net: period must be an integer >= 1, not {period!r}")
        tau = target_net.get("tau", 1.0)
        if isinstance(tau, bool) or not isinstance(tau, (int, float, np.integer, np.floating)) or \
                not (np.isfinite(tau) and 0.0 < float(tau) <= 1.0):
            raise ValueError(f"target_net: tau must lie in (0, 1], not {tau!r}")
        return dict(kind=kind, period=int(period), tau=float(tau))

    # --- noisy networks (Fortunato et al. 2018; `train_loop_device` only: the noise is added by the pack launch) -----
    NOISE_COPIES = ("act1", "train1", "train2")     # acting copy of net 1, train copies of net 1 and net 2: stream 4 rank + index

    @staticmethod
    def _check_noisy(noisy, seed) -> Optional[dict]:
        """None (epsilon-greedy, the reference's exploration), or the complete option dict: both networks carry factorised
        Gaussian noise of initial scale sigma0 / sqrt(in) on their dense heads (`NodeRemovalNet(noisy=sigma0)`), drawn on the
        device from Philox key (seed, stream of the copy); `seed` defaults to the trainer's."""
        if noisy is None:
            return None
        known = ("sigma0", "seed")
        if not isinstance(noisy, dict):
            raise ValueError("noisy: None or a dict with any of " + ", ".join(known))
        unknown = sorted(set(noisy) - set(known), key=repr)
        if unknown:
            raise ValueError(f"noisy: unknown option(s) {unknown}; known: " + ", ".join(known))
        sigma0 = noisy.get("sigma0", 0.5)
        if isinstance(sigma0, bool) or not isinstance(sigma0, (int, float, np.integer, np.floating)) or \
                not (np.isfinite(sigma0) and float(sigma0) > 0.0):
            raise ValueError(f"noisy: sigma0 must be finite and > 0, not {sigma0!r}")
        nseed = noisy.get("seed", seed)
        if isinstance(nseed, bool) or not isinstance(nseed, (int, np.integer)) or not 0 <= int(nseed) < 2 ** 32:
            raise ValueError(f"noisy: seed must be an integer in 0 .. 2^32 - 1, not {nseed!r}")
        return dict(sigma0=float(sigma0), seed=int(nseed))

    def resample(self, copy: str):
        """New noise for packed copy `copy` (one of NOISE_COPIES) on the current stream: its next draw, from its own stream."""
        k = self.NOISE_COPIES.index(copy)
        net = self.policy_net_2 if copy == "train2" else self.policy_net_1
        fused = self._fused_of(net, "act" if copy == "act1" else "train")
        fused.resample(self.noisy["seed"], 4 * self.ctx.rank + k, self.noise_draws[copy])
        self.noise_draws[copy] += 1
        return fused

    def beta(self, g: Optional[int] = None) -> float:
        """Importance-weight exponent after g gradient applications (`num_grads`, which is checkpointed: a restart
        continues the schedule): linear from beta0 to 1 over beta_steps."""
        o = self.prioritized
        if o is None:
            raise ValueError("beta: the trainer was built without prioritized replay")
        g = self.num_grads if g is None else g
        return min(1.0, o["beta0"] + (1.0 - o["beta0"]) * g / o["beta_steps"])

    # --- acting -------------------------------------------------------------
    @torch.no_grad()
    def select_action(self, state: Data, fused: Optional[bool] = None) -> int:
        """Greedy action of policy_net_1 (airfoil_dqn.py:208-209); fused HIP forward on a GPU."""
        dev = self.ctx.device
        if fused is None:
            fused = dev.type == "cuda"
        st = state.to(dev)
        q = self.policy_net_1.forward_fused(st) if fused else self.policy_net_1(st)
        return int(q.argmax().item())

    # --- learning -----------------------------------------------------------
    def _loss(self, transitions: List[Transition]):
        dev = self.ctx.device
        batch = Transition(*zip(*transitions))
        non_final_mask = torch.tensor([s is not None for s in batch.next_state], dtype=torch.bool, device=dev)
        non_final_next = [s for s in batch.next_state if s is not None]
        action_batch = torch.cat([a.reshape(1, 1) for a in batch.action]).to(dev)
        reward_batch = torch.cat([r.reshape(1) for r in batch.reward]).to(dev).float()
        net_a, net_b = (self.policy_net_1, self.policy_net_2)
        fused = dev.type == "cuda"   # the network evaluated WITHOUT gradient runs through the fused HIP forward
        datas = [s.to(dev) for s in batch.state]
        if self.select:
            if self.dense and all(d.x.shape[0] == datas[0].x.shape[0] for d in datas):
                # static-shape autograd path (no host syncs, fixed kernel sequence)
                out = net_a.forward_dense(*dense_batch(datas, self.e_max, dev))
            else:
                out = net_a(Batch.from_data_list(datas))
        else:
            states = Batch.from_data_list(datas)
            with torch.no_grad():
                out = net_a.forward_fused(states) if fused else net_a(states)
        q_sa = out.gather(1, action_batch).squeeze(1)
        next_vals = torch.zeros(len(transitions), device=dev)
        if non_final_next:
            nb = Batch.from_data_list([s.to(dev) for s in non_final_next])
            if self.select:
                with torch.no_grad():
                    nv = (net_b.forward_fused(nb) if fused else net_b(nb)).max(1)[0].float()
            elif self.dense and all(d.x.shape[0] == non_final_next[0].x.shape[0] for d in non_final_next):
                nv = net_b.forward_dense(*dense_batch([d.to(dev) for d in non_final_next], self.e_max, dev)).max(1)[0].float()
            else:
                nv = net_b(nb).max(1)[0].float()
            next_vals[non_final_mask] = nv
        expected = next_vals * self.gamma + reward_batch
        return self.criterion(q_sa.float(), expected.float())

    def _optimize_graphed(self, transitions: List[Transition]):
        """The autograd half of an optimiser step as ONE replayed HIP graph (static minibatch shape):
          select True : loss(q1(s)[a], r + gamma max q2(s'))   - gradient through policy_net_1 on the states,
                        targets from the fused no-grad forward of policy_net_2;
          select False: the same loss with the gradient through policy_net_2 on the NEXT states (the reference's
                        toggle, airfoil_dqn.py:240-310), q1(s)[a] from the fused no-grad forward; terminal
                        transitions ride along as masked rows (their own state as a placeholder, weight 0).
        Returns the loss value, or None when the minibatch is not eligible (ragged node counts) or capture is
        unsupported (the eager path runs)."""
        dev = self.ctx.device
        sel = self.select
        k = 0 if sel else 1
        net = (self.policy_net_1, self.policy_net_2)[k]
        devb = transitions if isinstance(transitions, DeviceBatch) else None
        batch = None if devb is not None else Transition(*zip(*transitions))
        lazy = devb is not None or (all(isinstance(s_, StateRef) for s_ in batch.state) and
                                    all(s_ is None or isinstance(s_, StateRef) for s_ in batch.next_state))
        if devb is None and lazy:   # replay filled by train_loop_vec: minibatch arrays without per-graph Data objects
            s_refs = list(batch.state)
            n_refs = [(s_ if s_ is not None else batch.state[i]) for i, s_ in enumerate(batch.next_state)]
        elif devb is None:
            states = [s_.to(dev) for s_ in batch.state]
            n0 = states[0].x.shape[0]
            nexts = [(s_.to(dev) if s_ is not None else states[i]) for i, s_ in enumerate(batch.next_state)]
            if any(d.x.shape[0] != n0 for d in states) or any(d.x.shape[0] != n0 for d in nexts):
                return None
        try:
            if devb is not None:
                nonfinal, reward, action = devb.nonfinal, devb.reward, devb.action
            else:
                nonfinal = torch.tensor([0.0 if s_ is None else 1.0 for s_ in batch.next_state], device=dev)
                reward = torch.cat([r.reshape(1) for r in batch.reward]).to(dev).float()
                action = torch.cat([a.reshape(1, 1) for a in batch.action]).to(dev)
            if lazy:
                ga = devb.ga if devb is not None else gather_state_refs(s_refs, self.e_max, dev)
                gb = devb.gb if devb is not None else gather_state_refs(n_refs, self.e_max, dev)
                other = self.policy_net_2 if sel else self.policy_net_1
                go = gb if sel else ga
                with torch.no_grad():
                    qo = self._fused_of(other).forward_arrays(go["x"], go["node_ptr"], go["esrc"], go["edst"], go["edge_ptr"],
                                                          go["n"], self.e_max, edge_counts=go.get("cnt"))
                    aux = (qo.max(1)[0].float() * nonfinal * self.gamma + reward) if sel else \
                        qo.gather(1, action).squeeze(1).float()
                gd = ga if sel else gb
                x, src, dst, mask = gd["x"], gd["src"], gd["dst"], gd["mask"]
            else:
                with torch.no_grad():
                    if sel:   # targets: fused forward of the other network on the next states
                        aux = self.policy_net_2.forward_fused(Batch.from_data_list(nexts)).max(1)[0].float() * nonfinal
                        aux = aux * self.gamma + reward                      # = expected
                    else:     # q1(s)[a]: fused forward of the other network on the states
                        aux = self.policy_net_1.forward_fused(Batch.from_data_list(states)).gather(1, action).squeeze(1).float()
                x, src, dst, mask = dense_batch(states if sel else nexts, self.e_max, dev)
            g = self._graphs.get(k)
            if g is None or g["x"].shape != x.shape:
                st = dict(x=x.clone(), src=src.clone(), dst=dst.clone(), mask=mask.clone(), act=action.clone(),
                          aux=aux.clone(), rew=reward.clone(), nf=nonfinal.clone())

                def fwd_bwd():
                    out = net.forward_dense(st["x"], st["src"], st["dst"], st["mask"])
                    if sel:
                        loss_ = self.criterion(out.gather(1, st["act"]).squeeze(1).float(), st["aux"])
                    else:
                        expected = out.max(1)[0].float() * st["nf"] * self.gamma + st["rew"]
                        loss_ = self.criterion(st["aux"], expected)
                    loss_.backward()
                    return loss_

                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):      # warm-up outside capture (allocator, autograd buffers)
                    for _ in range(3):
                        net.zero_grad(set_to_none=True)
                        fwd_bwd()
                torch.cuda.current_stream(dev).wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                net.zero_grad(set_to_none=True)
                # thread_local: other threads of the process (the RCCL watchdog, env-group workers) may touch the
                # device while this thread captures
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    loss_static = fwd_bwd()
                st.update(graph=graph, loss=loss_static, grads=[p.grad for p in net.parameters()])
                self._graphs[k] = g = st
            else:
                for k_, v_ in (("x", x), ("src", src), ("dst", dst), ("mask", mask), ("act", action), ("aux", aux),
                               ("rew", reward), ("nf", nonfinal)):
                    g[k_].copy_(v_)
            g["graph"].replay()
            flat = None
            if self.ctx.multi:
                flat = torch.cat([(gr if gr is not None else torch.zeros_like(p)).reshape(-1)
                                  for gr, p in zip(g["grads"], net.parameters())])
        except RuntimeError as exc:   # capture not supported for some op on this build: stay on the eager path
            self.graphs = False
            self._graphs = {}
            self._graph_error = repr(exc)
            return None
        if flat is not None:
            self.ctx.allreduce_mean_(flat)
            net.set_flat_gradients(flat)
        else:   # one rank: the graph has written the gradients where the optimiser reads them; parameters outside the
            for p, gr in zip(net.parameters(), g["grads"]):   # graph (conv3 / conv6, unused pools) keep grad None
                p.grad = gr
        return self._apply(k, g["loss"])

    def _apply(self, k: int, loss) -> float:
        """The tail of every host-path optimiser step, gradients of network k in place: returns the loss value."""
        self.opts[k].step()
        self.scheds[k].step()
        self.num_grads += 1
        self.losses.append(float(loss.item()))
        return self.losses[-1]

    def optimize(self, transitions: Optional[List[Transition]] = None):
        """One optimiser step (airfoil_dqn.py:315-340 + :184-200 + :286-310): local loss/backward, ONE flat
        all-reduce of the gradient over all ranks, identical Adam step on every rank."""
        _refuse_target_net(self, "optimize")
        _refuse_noisy(self, "optimize")
        if transitions is None:
            mem = self.device_memory if self.device_memory is not None else self.memory
            if mem.size() < self.batch_size:
                return None
            transitions = mem.sample(self.batch_size)
        if (self.num_grads % self.target_update) == 0:
            self.select = not self.select
        k = 0 if self.select else 1
        net = (self.policy_net_1, self.policy_net_2)[k]
        if self.graphs and self.dense and len(transitions) == self.batch_size:
            done = self._optimize_graphed(transitions)
            if done is not None:
                return done
        if isinstance(transitions, DeviceBatch):      # eager path: per-graph objects
            transitions = transitions.to_transitions()
        net.zero_grad(set_to_none=True)
        loss = self._loss(transitions)
        if loss.requires_grad:
            loss.backward()
            flat = net.flat_gradients()
        else:
            # every sampled transition is terminal while the target network is the trained one (select False):
            # nothing depends on the parameters.  All ranks still join the all-reduce with a zero gradient.
            flat = torch.zeros(sum(p.numel() for p in net.parameters()), device=self.ctx.device)
        self.ctx.allreduce_mean_(flat)
        net.set_flat_gradients(flat)
        return self._apply(k, loss)

    # --- learning on the device: hand-written forward + backward, replay sampling and Adam as kernels --------------
    def _fused_of(self, net, role: str = "act"):
        """The packed device copy of `net`'s parameters + launchers.  Two copies per network: "act" (the Q-forward of
        the env step, repacked on the MAIN stream of a device loop, only behind the event of the last optimiser chain)
        and "train" (the learning step and its no-grad forward, repacked on the OPTIMISER stream, in order with the
        `mdq_adam_step` launches of that stream) - one shared copy was repacked by the acting forward while the Adam
        kernel of the other stream was writing the parameters."""
        return fused_of(net, role)

    def _adam_state(self, k: int, total: int):
        """Flat first / second moment buffers of network k laid out like the flat gradient.  The entries of the torch
        optimiser's `state` ARE views of them (so `state_dict()` checkpoints, `load_state_dict` and an occasional
        `opts[k].step()` on the host path all see the same moments); after a `load_state_dict` the loaded tensors are
        copied in and re-aliased."""
        net, opt = (self.policy_net_1, self.policy_net_2)[k], self.opts[k]
        ad = self._adam = self._adam or [None, None]
        skip = {id(p_) for p_ in net.unused_parameters()}
        prm = [p_ for p_ in net.parameters() if id(p_) not in skip]
        a = ad[k]
        ok = a is not None and a["m"].numel() == total and all(
            p_ in opt.state and opt.state[p_].get("exp_avg") is not None and
            opt.state[p_]["exp_avg"].data_ptr() == a["views"][id(p_)][0].data_ptr() for p_ in prm[:1])
        if ok:
            return a
        dev = self.ctx.device
        a = dict(m=torch.zeros(total, device=dev), v=torch.zeros(total, device=dev), views={}, params=prm)
        off = 0
        for p_ in net.parameters():
            n = p_.numel()
            if id(p_) not in skip:
                mv, vv = a["m"][off:off + n].view_as(p_), a["v"][off:off + n].view_as(p_)
                old = opt.state.get(p_, {})
                step = old.get("step", torch.tensor(0.0))
                if old.get("exp_avg") is not None:
                    mv.copy_(old["exp_avg"])
                    vv.copy_(old["exp_avg_sq"])
                opt.state[p_] = dict(step=step.detach().to("cpu", torch.float32).reshape(()).clone(), exp_avg=mv, exp_avg_sq=vv)
                a["views"][id(p_)] = (mv, vv, off)
            off += n
        d = _lib.AdamDesc()
        if len(prm) > _lib.PACK_MAX:
            raise ValueError("too many trained parameter tensors for mdq_adam_step")
        d.n = len(prm)
        for i, p_ in enumerate(prm):
            d.param[i], d.offset[i], d.len[i] = p_.data_ptr(), a["views"][id(p_)][2], p_.numel()
        d.exp_avg, d.exp_avg_sq = a["m"].data_ptr(), a["v"].data_ptr()
        a["desc"] = d
        ad[k] = a
        return a

    def _adam_step_device(self, k: int, flat: torch.Tensor):
        """`opts[k].step()` + `scheds[k].step()` with ONE kernel launch for the update (mdq_adam_step)."""
        opt = self.opts[k]
        a = self._adam_state(k, flat.numel())
        g = opt.param_groups[0]
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("mdq_adam_step: amsgrad / maximize are not supported")
        for p_ in a["params"]:
            opt.state[p_]["step"] += 1
        step = float(opt.state[a["params"][0]]["step"])
        d = a["desc"]
        if any(d.param[i] != p_.data_ptr() for i, p_ in enumerate(a["params"])):     # (any may be re-seated)
            for i, p_ in enumerate(a["params"]):
                d.param[i] = p_.data_ptr()
        d.grad = flat.data_ptr()
        d.lr, (d.beta1, d.beta2), d.eps, d.weight_decay = float(g["lr"]), g["betas"], float(g["eps"]), float(g["weight_decay"])
        d.bias_correction1, d.bias_correction2 = 1.0 - d.beta1 ** step, 1.0 - d.beta2 ** step
        _lib.check(_lib.load().mdq_adam_step(C.byref(d), _lib.stream_ptr()), "mdq_adam_step")
        # the kernel wrote the parameters behind torch's back (no `_version` bump): tell the fused kernels' packed copy
        net = (self.policy_net_1, self.policy_net_2)[k]
        net._mdq_version = getattr(net, "_mdq_version", 0) + 1
        opt._opt_called = True          # (lr_scheduler's "step() before optimizer.step()" check)
        self.scheds[k].step()

    def calibrate_opt_stream(self, venv, fused_act, tries: int = 6, steps: int = 6):
        """Pick, by measurement, a stream for the optimiser chain that really runs beside the env step (its main stream
        = the current one, and its flow stream): like `VecEnv2DAirfoil.calibrate_streams` - HIP's stream -> hardware queue
        mapping leaves pairs that overlap only partly, and the learning loop then runs at 2.6 instead of 1.95 ms per
        batched step.  Every candidate carries a stand-in chain (fused forward of one network + `mdq_gcn_train_step` of
        the other on a fixed random minibatch, with `target_net` kind "double" also the second forward and the select
        launch: the kernels of `optimize_device`, with `noisy` also the two noisy packs and `mdq_noisy_grad`; no parameter is changed) through a few
        real env steps with the loop's own synchronisation; the fastest stays.  The environments are reset afterwards."""
        dev = self.ctx.device
        main = torch.cuda.current_stream(dev)
        if _st.roles_own_queues(dev):
            roles = _st.role_streams(dev)
            flow_now = venv._flow_stream
            if (self._opt_stream is roles["opt"] and (flow_now is None or flow_now is roles["flow"]) and
                    (main is roles["main"] or main == roles["main"] or _st._overlaps(roles["opt"], main, dev))):
                # CU-mask role streams with every probe passed: a hardware queue each, nothing to choose between
                self._opt_calibrated_for = (main, flow_now)
                self.opt_calibration_ms = []
                return []
        B, N = venv.B, venv.N
        st0 = venv._state_device()
        F_ = st0["x"].shape[2]
        mb, EM = self.batch_size, self.e_max
        g = torch.Generator(device="cpu").manual_seed(7)
        ne = 600
        x = torch.randn((mb, N, F_), generator=g).to(dev)
        esrc = torch.randint(0, N, (mb * ne,), generator=g, dtype=torch.int32).to(dev)
        edst = torch.randint(0, N, (mb * ne,), generator=g, dtype=torch.int32).to(dev)
        node_ptr = torch.arange(mb + 1, dtype=torch.int32, device=dev) * N
        edge_ptr = torch.arange(mb + 1, dtype=torch.int32, device=dev) * ne
        action = torch.zeros(mb, dtype=torch.int64, device=dev)
        reward = torch.zeros(mb, dtype=torch.float32, device=dev)
        nonfinal = torch.ones(mb, dtype=torch.float32, device=dev)
        f1, f2 = self._fused_of(self.policy_net_1, "train"), self._fused_of(self.policy_net_2, "train")
        f1._pack()
        f2._pack()
        noisy, probe = self.noisy is not None, [0]
        double = self.target_net is not None and self.target_net["kind"] == "double"
        q_sel = torch.zeros((mb, self.n_actions + 1), dtype=torch.float32, device=dev) if double else None
        rng = np.random.default_rng(977)

        def timed(cand, k):
            ro = venv.rollout_begin(k, rng.random((k, B)) < 0.5, rng.integers(0, N + 1, (k, B)))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(main)
            for _ in range(k):
                main.wait_stream(cand)
                ev = torch.cuda.Event()
                ev.record(main)
                with torch.cuda.stream(cand):
                    cand.wait_event(ev)
                    if noisy:       # the chain that will run: both noisy packs (another draw forces the launch) and, from
                        probe[0] += 1   # `train_step` of a copy that carries noise, `mdq_noisy_grad`; no counter moves
                        f1.resample(self.noisy["seed"], 1, 2 ** 63 + probe[0])
                        f2.resample(self.noisy["seed"], 2, 2 ** 63 + probe[0])
                    qo = f2.forward_arrays(x, node_ptr, esrc, edst, edge_ptr, N, EM)
                    if double:      # the chain that will run: the online network's forward and the select launch as well
                        q_on = f1.forward_arrays(x, node_ptr, esrc, edst, edge_ptr, N, EM)
                        _lib.check(_lib.load().mdq_double_q_select(mb, q_sel.shape[1], q_on.data_ptr(), qo.data_ptr(),
                                                                   q_sel.data_ptr(), None, _lib.stream_ptr()),
                                   "mdq_double_q_select")
                        qo = q_sel
                    f1.train_step(x, node_ptr, esrc, edst, edge_ptr, N, EM, 0, qo, action, reward, nonfinal, self.gamma)
                venv.rollout_step(ro, fused_act)
            main.wait_stream(cand)
            e1.record(main)
            venv.rollout_end(ro)
            e1.synchronize()
            return e0.elapsed_time(e1) / k
        results = []
        for t in range(max(1, int(tries))):
            cand = self._opt_stream if (t == 0 and self._opt_stream is not None) else torch.cuda.Stream(device=dev)
            timed(cand, 2)
            results.append((timed(cand, int(steps)), cand))
            ms = [r[0] for r in results]
            if len(ms) >= 2 and min(ms) < 0.85 * max(ms) and ms[-1] <= 1.03 * min(ms):
                break
        self._opt_stream = min(results, key=lambda r: r[0])[1]
        self._opt_calibrated_for = (main, venv._flow_stream)
        self.opt_calibration_ms = [r[0] for r in results]
        f1.denoise()
        f2.denoise()
        venv.reset_all()
        return self.opt_calibration_ms

    def optimize_device(self, rep: "SharedDeviceReplay", idx, loss_out: Optional[torch.Tensor] = None,
                        weight: Optional[torch.Tensor] = None, td_out: Optional[torch.Tensor] = None,
                        head_step: Optional[int] = None, steps_out: Optional[torch.Tensor] = None,
                        sel_out: Optional[torch.Tensor] = None, value_out: Optional[torch.Tensor] = None):
        """One optimiser step on a minibatch of the record ring WITHOUT host synchronisation and without autograd:
        `mdq_replay_sample` (records `idx` -> graph arrays), fused forward of the network without gradient,
        `mdq_gcn_train_step` of the other one (forward + double-DQN Huber loss + backward), ONE flat all-reduce over the
        ranks, `mdq_adam_step`.  Everything is enqueued on the current stream; the loss goes to `loss_out` (a (1,)
        device tensor, e.g. a slot of a log ring) and is also returned as a device tensor.  Same `select` toggling as
        `optimize` (airfoil_dqn.py:315-340 + :184-200 + :240-310).  `weight` / `td_out`: (batch,) float32 device tensors
        handed through to the learning step (importance weights in, TD errors out: prioritized replay).

        A trainer with `n_step` > 1 samples with `mdq_replay_sample_nstep` instead: the reward becomes the discounted sum over
        the walk from every drawn record, s' the state the walk ends in, and `nonfinal` carries gamma^(m-1), which the
        unchanged learning step multiplies by gamma.  `head_step` (required then): the batched step t whose group is being
        written, which no walk enters (`rep.group_base(t)`); `steps_out`: (batch,) int32 device tensor for the lengths m.

        A trainer with `target_net` never toggles: policy_net_1 is trained on every step (mode 0) against policy_net_2, the
        target.  The chain becomes: the sampling launch, the fused forward of the target on the next states (q_t), for kind
        "double" the fused forward of the online network on the same graphs (q_o) and `mdq_double_q_select` (q_o, q_t) ->
        a row per graph whose maximum is Q_target(s', argmax_a Q_online(s', a)), the unchanged learning step with that as
        `q_other`, the all-reduce, `mdq_adam_step`, and every `period` gradient steps `mdq_target_update` (target <- online,
        `tau`) on the same stream.  Every rank runs the same update on identical replicas: no collective.  `sel_out` /
        `value_out` (kind "double"): (batch,) int32 / float32 device tensors that receive the chosen action and that value.

        A trainer with `noisy` first resamples the train copies of both networks (`mdq_gcn_pack_noisy` in place of their
        repack): every forward and the learning step of this call see one draw per network - in the Double-DQN chain the
        online network's forward on s' and its learning step share theirs -, `train_step` adds `mdq_noisy_grad` with the
        eps of that draw in front of the all-reduce, and `mdq_adam_step` / `mdq_target_update` take `noisy_sigma` as one more
        parameter tensor."""
        dev = self.ctx.device
        if self.n_step > 1 and head_step is None:
            raise ValueError("optimize_device: a trainer with n_step > 1 needs head_step (the batched step being written)")
        tn = self.target_net
        if (sel_out is not None or value_out is not None) and (tn is None or tn["kind"] != "double"):
            raise ValueError("optimize_device: sel_out / value_out need a trainer with target_net kind 'double'")
        if tn is None and (self.num_grads % self.target_update) == 0:
            self.select = not self.select
        sel = True if tn is not None else self.select
        k = 0 if sel else 1
        net, other = ((self.policy_net_1, self.policy_net_2) if sel else (self.policy_net_2, self.policy_net_1))
        if self.noisy is not None:      # one draw per network per optimiser step, in order with this stream's Adam launches
            self.resample("train1")
            self.resample("train2")
        mb, N, F, EM = len(idx), rep.N, rep.F, rep.e_max
        b = self._mb_bufs
        if b is None or b["key"] != (mb, N, F, EM):
            i32, f32 = torch.int32, torch.float32
            # the output arrays of `mdq_replay_sample`, named like the pointer fields of its descriptor
            b = dict(idx=torch.empty(mb, dtype=i32, device=dev), x_s=torch.empty((mb, N, F), dtype=f32, device=dev),
                     x_n=torch.empty((mb, N, F), dtype=f32, device=dev))
            for nm, n, dt in (("esrc_s", mb * EM, i32), ("edst_s", mb * EM, i32), ("esrc_n", mb * EM, i32),
                              ("edst_n", mb * EM, i32), ("edge_ptr_s", mb + 1, i32), ("edge_ptr_n", mb + 1, i32),
                              ("action", mb, torch.int64), ("reward", mb, f32), ("nonfinal", mb, f32)):
                b[nm] = torch.zeros(n, dtype=dt, device=dev)
            d = _lib.ReplaySampleDesc(n=mb, rec_len=rep.rec_len, nf=N * F, EM=EM, **{nm: t.data_ptr() for nm, t in b.items()})
            b.update(key=(mb, N, F, EM), node_ptr=torch.arange(mb + 1, dtype=i32, device=dev) * N, desc=d)
            self._mb_bufs = b
        if torch.is_tensor(idx):      # already on the device (the loop uploads a whole chunk of minibatches at once)
            if idx.dtype != torch.int32 or idx.device.type != "cuda" or not idx.is_contiguous():
                raise ValueError("optimize_device: device indices must be contiguous int32")
            b["desc"].idx = idx.data_ptr()
        else:
            b["idx"].copy_(torch.as_tensor(np.asarray(idx, dtype=np.int32)))     # (pageable source: a blocking copy)
            b["desc"].idx = b["idx"].data_ptr()
        b["desc"].R = rep.R.data_ptr()
        if self.n_step == 1:
            _lib.check(_lib.load().mdq_replay_sample(C.byref(b["desc"]), _lib.stream_ptr()), "mdq_replay_sample")
        else:
            ns = b["nstep"] = rep.nstep_desc(head_step, self.n_step, self.gamma, steps_out, b.get("nstep"))
            _lib.check(_lib.load().mdq_replay_sample_nstep(C.byref(b["desc"]), C.byref(ns), _lib.stream_ptr()),
                       "mdq_replay_sample_nstep")
        gs = dict(x=b["x_s"], esrc=b["esrc_s"], edst=b["edst_s"], edge_ptr=b["edge_ptr_s"])
        gn = dict(x=b["x_n"], esrc=b["esrc_n"], edst=b["edst_n"], edge_ptr=b["edge_ptr_n"])
        go, gd = (gn, gs) if sel else (gs, gn)
        qo = self._fused_of(other, "train").forward_arrays(go["x"], b["node_ptr"], go["esrc"], go["edst"], go["edge_ptr"], N, EM)
        if tn is not None and tn["kind"] == "double":
            qo = self._double_q_select(net, go, b, qo, N, EM, sel_out, value_out)
        loss, flat = self._fused_of(net, "train").train_step(gd["x"], b["node_ptr"], gd["esrc"], gd["edst"], gd["edge_ptr"], N, EM,
                                                    0 if sel else 1, qo, b["action"], b["reward"], b["nonfinal"], self.gamma,
                                                    loss_out=loss_out, weight=weight, td_out=td_out)
        if self.ctx.multi:
            self.ctx.allreduce_mean_(flat)
        self._adam_step_device(k, flat)
        self.num_grads += 1
        if tn is not None and self.num_grads % tn["period"] == 0:
            self._target_update_device(tn["tau"])
        return loss

    def _double_q_select(self, online, gn, b, q_t, N, EM, sel_out, value_out):
        """The Double-DQN half of `optimize_device`: the online network's train-role forward on the next-state graphs `gn`,
        then `mdq_double_q_select` -> the (batch, out) array whose row b holds q_t[b][argmax_j q_o[b][j]] in every column."""
        q_o = self._fused_of(online, "train").forward_arrays(gn["x"], b["node_ptr"], gn["esrc"], gn["edst"], gn["edge_ptr"], N, EM)
        q_sel = b.get("q_sel")
        if q_sel is None or q_sel.shape != q_t.shape:
            q_sel = b["q_sel"] = torch.zeros_like(q_t)
        mb, out_dim = q_t.shape
        for t, dt in ((sel_out, torch.int32), (value_out, torch.float32)):
            if t is not None and (t.dtype != dt or not t.is_contiguous() or t.device != q_t.device or t.numel() != mb):
                raise ValueError(f"optimize_device: sel_out / value_out must be contiguous int32 / float32 tensors of {mb} "
                                 f"entries on {q_t.device}")
        _lib.check(_lib.load().mdq_double_q_select(mb, out_dim, q_o.data_ptr(), q_t.data_ptr(), q_sel.data_ptr(),
                                                   None if sel_out is None else sel_out.data_ptr(), _lib.stream_ptr()),
                   "mdq_double_q_select")
        if value_out is not None:
            value_out.copy_(q_sel[:, 0])
        return q_sel

    def _target_update_device(self, tau: float):
        """policy_net_2 <- policy_net_1 with ONE launch (`mdq_target_update`) on the current stream - the optimiser stream,
        in order behind the `mdq_adam_step` that wrote the online parameters and in front of the target's next forward."""
        src, dst = list(self.policy_net_1.parameters()), list(self.policy_net_2.parameters())
        d = self._target_desc
        if d is None or any(d.src[i] != p.data_ptr() or d.dst[i] != q.data_ptr() for i, (p, q) in enumerate(zip(src, dst))):
            if len(src) > _lib.PACK_MAX:
                raise ValueError("too many parameter tensors for mdq_target_update")
            d = self._target_desc = _lib.TargetUpdateDesc()
            d.n = len(src)
            for i, (p, q) in enumerate(zip(src, dst)):
                if p.shape != q.shape or p.dtype != torch.float32 or q.dtype != torch.float32 or \
                        not (p.is_contiguous() and q.is_contiguous()):
                    raise ValueError("mdq_target_update needs contiguous float32 parameters of equal shapes")
                d.src[i], d.dst[i], d.len[i] = p.data_ptr(), q.data_ptr(), p.numel()
        d.tau = float(tau)
        _lib.check(_lib.load().mdq_target_update(C.byref(d), _lib.stream_ptr()), "mdq_target_update")
        # the kernel wrote the parameters behind torch's back: the packed copies of the target repack before their next forward
        self.policy_net_2._mdq_version = getattr(self.policy_net_2, "_mdq_version", 0) + 1

    def save(self, save_dir, prefix="", extra: Optional[dict] = None):
        """`ParameterServer.write` (airfoil_dqn.py:214-218): PyG-keyed state dicts `{prefix}policy_net_{1,2}.pt`, plus
        `{prefix}trainer_state.pt` (both Adam states, both schedulers, gradient count, the double-DQN toggle and
        whatever the loop hands over in `extra`, e.g. its epsilon step counters) - what a restart needs beyond the
        reference's two files.  A trainer with `noisy` adds the draw counters of its packed copies."""
        os.makedirs(save_dir, exist_ok=True)
        torch.save(self.policy_net_1.state_dict(), os.path.join(save_dir, f"{prefix}policy_net_1.pt"))
        torch.save(self.policy_net_2.state_dict(), os.path.join(save_dir, f"{prefix}policy_net_2.pt"))
        torch.save(dict(opts=[o.state_dict() for o in self.opts], scheds=[s_.state_dict() for s_ in self.scheds],
                        num_grads=self.num_grads, select=self.select, extra=extra or {},
                        **({} if self.noisy is None else dict(noise_draws=dict(self.noise_draws)))),
                   os.path.join(save_dir, f"{prefix}trainer_state.pt"))

    def load(self, save_dir, prefix="", scheduler_steps: Optional[int] = None) -> dict:
        """RESTART of the reference (airfoil_dqn.py:163-179,230-234): load `{prefix}policy_net_{1,2}.pt` into both
        Q-networks (in place: captured HIP graphs and the fused forward keep working on the same tensors).  When
        `{prefix}trainer_state.pt` exists the optimisers, schedulers, gradient count and toggle continue as well;
        with reference-style checkpoints (two files only) the schedulers are advanced by `scheduler_steps` like the
        reference's hard-coded fast-forward (:177-179).  Returns the `extra` dict of the checkpoint."""
        dev = self.ctx.device
        for net, name in ((self.policy_net_1, "policy_net_1.pt"), (self.policy_net_2, "policy_net_2.pt")):
            net.load_state_dict(torch.load(os.path.join(save_dir, prefix + name), map_location=dev))
        path = os.path.join(save_dir, f"{prefix}trainer_state.pt")
        extra = {}
        if os.path.exists(path):
            # optimiser / scheduler state dicts + numpy arrays of the loops (`extra`): the safe unpickler with numpy's array
            # reconstruction allow-listed - a checkpoint directory is not a code-execution vector
            _ma = (getattr(np, "_core", None) or np.core).multiarray      # (numpy >= 2: numpy._core)
            # (every fixed-size numeric dtype class: `extra` is whatever the loop hands over - an RNG state is uint32 / uint64)
            safe = [np.ndarray, np.dtype] + sorted({type(np.dtype(t)) for t in (
                np.bool_, np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64, np.float16,
                np.float32, np.float64, np.complex64, np.complex128)}, key=lambda c: c.__name__)
            for name in ("_reconstruct", "scalar"):
                fn = getattr(_ma, name, None)
                if fn is not None:
                    safe.append(fn)
            with torch.serialization.safe_globals(safe):
                st = torch.load(path, map_location=dev, weights_only=True)
            for o, sd in zip(self.opts, st["opts"]):
                o.load_state_dict(sd)
            for s_, sd in zip(self.scheds, st["scheds"]):
                s_.load_state_dict(sd)
            self.num_grads, self.select, extra = int(st["num_grads"]), bool(st["select"]), st.get("extra", {})
            if self.noisy is not None:      # the noise continues where the checkpoint stopped (counters of a noisy run only)
                self.noise_draws.update({c: int(v) for c, v in st.get("noise_draws", {}).items() if c in self.noise_draws})
        elif scheduler_steps:
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")       # (scheduler stepped before the optimiser: intended here)
                for s_ in self.scheds:
                    for _ in range(int(scheduler_steps)):
                        s_.step()
        return extra
