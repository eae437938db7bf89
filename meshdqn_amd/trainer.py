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

import math
import os
import random
from collections import namedtuple
from typing import List, Optional

import numpy as np
import torch
import torch.distributed as dist

from .airfoilgcnn import NodeRemovalNet, dense_batch
from .data import Batch, Data

Transition = namedtuple("Transition", ("state", "action", "next_state", "reward"))


class ReplayMemory(object):
    """airfoil_dqn.py:48-67 (without the Ray actor)."""

    def __init__(self, capacity):
        self.capacity = capacity
        self.memory = []
        self.position = 0

    def push(self, *args):
        if len(self.memory) < self.capacity:
            self.memory.append(None)
        self.memory[self.position] = Transition(*args)
        self.position = (self.position + 1) % self.capacity

    def sample(self, batch_size):
        return random.sample(self.memory, batch_size)

    def size(self):
        return len(self.memory)

    __len__ = size


def epsilon_threshold(steps_done, start=1.0, end=0.01, decay=10000):
    """airfoil_dqn.py:455."""
    return end + (start - end) * math.exp(-steps_done / decay)


# ---------------------------------------------------------------------------- distributed helpers

class DistContext:
    """Process-group plumbing: rank / world from the torchrun environment, RCCL on GPUs, gloo on CPU."""

    def __init__(self, backend: Optional[str] = None, device: Optional[torch.device] = None):
        self.rank = int(os.environ.get("RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if device is None:
            if torch.cuda.is_available():
                # MDQ_SHARE_GPU=1 (+ MDQ_DIST_BACKEND=gloo: RCCL refuses two ranks on one device): a debugging aid that lets
                # the multi-rank control flow run on a box with fewer GPUs than ranks; never set by a production launcher
                ndev = torch.cuda.device_count()
                if self.local_rank >= ndev and not os.environ.get("MDQ_SHARE_GPU"):
                    raise RuntimeError(f"rank {self.rank}: local rank {self.local_rank} has no GPU of its own ({ndev} visible)")
                device = torch.device("cuda", self.local_rank % ndev)
            else:
                device = torch.device("cpu")
        self.device = device
        self.owns_group = False
        # `multi`: the collectives run.  MDQ_FORCE_COLLECTIVES=1 turns them on for ONE rank as well - the gradient all-reduce
        # and the record all-gathers then go through the backend (RCCL) with a group of one: what a single-GPU box can
        # exercise of the multi-GPU path (same numbers as without a group; tests/test_trainer_gpu.py)
        self.multi = self.world > 1 or os.environ.get("MDQ_FORCE_COLLECTIVES", "") == "1"
        if self.multi and not dist.is_initialized():
            import datetime
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            backend = backend or os.environ.get("MDQ_DIST_BACKEND") or ("nccl" if device.type == "cuda" else "gloo")
            long_timeout = datetime.timedelta(seconds=float(os.environ.get("MDQ_DIST_TIMEOUT", "1800")))
            kw = dict(timeout=long_timeout)
            store = None
            if self.world == 1 and "TORCHELASTIC_RUN_ID" not in os.environ:
                # a forced group of one rank started by hand (MDQ_FORCE_COLLECTIVES=1 without a launcher): rank 0 of 1 on a free port
                os.environ.setdefault("RANK", "0")
                os.environ.setdefault("WORLD_SIZE", "1")
                if not os.environ.get("MASTER_PORT"):
                    import socket
                    s_ = socket.socket()
                    s_.bind(("127.0.0.1", 0))
                    os.environ["MASTER_PORT"] = str(s_.getsockname()[1])
                    s_.close()
            if "TORCHELASTIC_RUN_ID" not in os.environ and os.environ.get("MASTER_PORT"):
                # started by meshdqn_amd.launcher (not torchrun, whose agent owns the store): rendezvous with a SHORT timeout -
                # a rank that never shows up fails the job in MDQ_RENDEZVOUS_TIMEOUT seconds, not in c10d's 10-30 minutes
                store = dist.TCPStore(os.environ["MASTER_ADDR"], int(os.environ["MASTER_PORT"]), self.world, self.rank == 0,
                                      timeout=datetime.timedelta(seconds=float(os.environ.get("MDQ_RENDEZVOUS_TIMEOUT", "180"))))
                kw.update(store=store, rank=self.rank, world_size=self.world)
            if device.type == "cuda":
                torch.cuda.set_device(device)
            if device.type == "cuda" and backend == "nccl":
                dist.init_process_group(backend, device_id=device, **kw)
            else:
                dist.init_process_group(backend, **kw)
            if store is not None:
                # the SHORT timeout was for the rendezvous only: c10d calls set_timeout on stores it creates itself, not on one it
                # is handed - every later store wait (lazy communicator creation, new_group, gloo's full-mesh connect) would keep
                # the 180 s and fail a job whose ranks drift apart by more than three minutes
                store.set_timeout(long_timeout)
            self.owns_group = True
        self.backend = dist.get_backend() if (self.multi and dist.is_initialized()) else None

    def shard(self, n_total: int):
        """Contiguous block of environment ids owned by this rank (env id -> rank = id // (n/world))."""
        per = n_total // self.world
        extra = n_total % self.world
        lo = self.rank * per + min(self.rank, extra)
        return range(lo, lo + per + (1 if self.rank < extra else 0))

    def allreduce_mean_(self, flat: torch.Tensor) -> torch.Tensor:
        if self.multi:
            dist.all_reduce(flat, op=dist.ReduceOp.SUM)
            flat /= self.world
        return flat

    def max_over_ranks(self, value: float) -> float:
        if not self.multi:
            return value
        t = torch.tensor([value], dtype=torch.float64, device=self.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def barrier(self):
        if self.multi:
            dist.barrier()

    def close(self):
        if self.owns_group and dist.is_initialized():
            dist.destroy_process_group()


# fixed-size transition record for the replay all-gather: x (N,F) f32 twice,
# edge_index padded to E_MAX int32 twice, edge counts, action, reward, done
def pack_transitions(trs: List[Transition], n_nodes: int, n_feat: int, e_max: int) -> torch.Tensor:
    rec = 2 * n_nodes * n_feat + 2 * 2 * e_max + 5
    out = torch.zeros((len(trs), rec), dtype=torch.float32)
    for i, t in enumerate(trs):
        off = 0
        for s in (t.state, t.next_state):
            if s is not None:
                out[i, off:off + n_nodes * n_feat] = s.x.reshape(-1).float().cpu()
            off += n_nodes * n_feat
        for s in (t.state, t.next_state):
            if s is not None:
                e = s.edge_index.shape[1]
                if e > e_max:
                    raise ValueError(f"edge count {e} exceeds e_max {e_max}")
                out[i, off:off + e] = s.edge_index[0].float().cpu()
                out[i, off + e_max:off + e_max + e] = s.edge_index[1].float().cpu()
            off += 2 * e_max
        out[i, off] = t.state.edge_index.shape[1]
        out[i, off + 1] = t.next_state.edge_index.shape[1] if t.next_state is not None else 0
        out[i, off + 2] = float(t.action.item() if torch.is_tensor(t.action) else t.action)
        out[i, off + 3] = float(t.reward.item() if torch.is_tensor(t.reward) else t.reward)
        out[i, off + 4] = 0.0 if t.next_state is not None else 1.0
    return out


def unpack_transitions(rec: torch.Tensor, n_nodes: int, n_feat: int, e_max: int) -> List[Transition]:
    out = []
    nf = n_nodes * n_feat
    for r in rec.cpu():
        off = 2 * nf + 4 * e_max
        e0, e1 = int(r[off].item()), int(r[off + 1].item())
        done = r[off + 4].item() > 0.5

        def graph(k, e):
            x = r[k * nf:(k + 1) * nf].reshape(n_nodes, n_feat).clone()
            base = 2 * nf + k * 2 * e_max
            ei = torch.stack([r[base:base + e], r[base + e_max:base + e_max + e]]).long()
            return Data(x=x, edge_index=ei, edge_attr=[])
        s = graph(0, e0)
        ns = None if done else graph(1, e1)
        out.append(Transition(s, torch.tensor([[int(r[off + 2].item())]]), ns, torch.tensor([r[off + 3].item()])))
    return out


def pack_transitions_device(st_prev: dict, st_next: dict, actions, rewards, dones, e_max: int) -> torch.Tensor:
    """The records of `pack_transitions` for the B transitions of one batched env step, built ON THE DEVICE from the two
    batched state dicts of `VecEnv2DAirfoil.get_state()` (x (B,N,F) f32, padded edge lists (B,e_max) i32 + `nedges`):
    a handful of vectorised torch ops, no per-field host copies.  actions / rewards / dones: (B,) arrays or tensors."""
    x0, x1 = st_prev["x"], st_next["x"]
    dev, B = x0.device, x0.shape[0]

    def dv(a, dt):
        return a.to(dev, dt) if torch.is_tensor(a) else torch.as_tensor(np.asarray(a), dtype=dt, device=dev)

    done = dv(dones, torch.float32).reshape(B, 1)
    cols = torch.arange(e_max, device=dev)[None, :]

    def edges(st):
        if st["edge_src_pad"].shape[1] != e_max:
            raise ValueError(f"padded edge lists have {st['edge_src_pad'].shape[1]} slots, e_max is {e_max}")
        cnt = dv(st["nedges"], torch.int64).reshape(B, 1)
        live = cols < cnt
        return (torch.where(live, st["edge_src_pad"], 0).float(), torch.where(live, st["edge_dst_pad"], 0).float(), cnt.float())
    s0, d0, c0 = edges(st_prev)
    s1, d1, c1 = edges(st_next)
    keep = 1.0 - done                                   # terminal: no next state (zeros, like the host packing)
    return torch.cat([x0.reshape(B, -1).float(), x1.reshape(B, -1).float() * keep, s0, d0, s1 * keep, d1 * keep, c0, c1 * keep,
                      dv(actions, torch.float32).reshape(B, 1), dv(rewards, torch.float32).reshape(B, 1), done], dim=1)


class SharedDeviceReplay:
    """Replay ring of fixed-size transition RECORDS on the device (layout of `pack_transitions`): what the ranks
    exchange when the replay is shared (all-gather of transition records; 1024 envs -> 35 MB per step over
    xGMI).  `push_records` takes the (world * B, record) tensor of an all-gather as it is; `sample` returns the same
    `DeviceBatch` interface as `DeviceReplay` (minibatch arrays gathered by a few torch ops, nothing read back)."""

    def __init__(self, capacity: int, N: int, F: int, e_max: int, device):
        self.capacity, self.N, self.F, self.e_max, self.device = int(capacity), int(N), int(F), int(e_max), device
        self.rec_len = 2 * N * F + 4 * e_max + 5
        self.R = torch.zeros((self.capacity, self.rec_len), dtype=torch.float32, device=device)
        self.position, self.count = 0, 0
        self._cols = torch.arange(e_max, device=device)[None, :]

    def push_records(self, rec: torch.Tensor):
        m = rec.shape[0]
        if rec.shape[1] != self.rec_len:
            raise ValueError(f"record length {rec.shape[1]}, expected {self.rec_len}")
        pos = (self.position + torch.arange(m, device=self.device)) % self.capacity
        self.R.index_copy_(0, pos, rec.to(self.device))
        self.position = int((self.position + m) % self.capacity)
        self.count = min(self.count + m, self.capacity)

    def size(self):
        return self.count

    __len__ = size

    def _graphs(self, rows: torch.Tensor, k: int) -> dict:
        """Minibatch arrays (keys of `DeviceReplay.gather`) of graph k (0: state, 1: next state) of the record rows."""
        N, F, EM, n = self.N, self.F, self.e_max, rows.shape[0]
        nf = N * F
        x = rows[:, k * nf:(k + 1) * nf].reshape(n, N, F)
        base = 2 * nf + k * 2 * EM
        sp, dp = rows[:, base:base + EM].to(torch.int32), rows[:, base + EM:base + 2 * EM].to(torch.int32)
        cnt = rows[:, 2 * nf + 4 * EM + k].to(torch.int64)
        live = self._cols < cnt[:, None]
        edge_ptr = torch.zeros(n + 1, dtype=torch.int64, device=rows.device)
        edge_ptr[1:] = torch.cumsum(cnt, 0)
        # packed edge lists without a host synchronisation: dead slots are scattered into one dump slot behind the end
        posn = torch.where(live, edge_ptr[:-1, None] + self._cols, n * EM)
        esrc = torch.zeros(n * EM + 1, dtype=torch.int32, device=rows.device).scatter_(0, posn.reshape(-1), sp.reshape(-1))
        edst = torch.zeros(n * EM + 1, dtype=torch.int32, device=rows.device).scatter_(0, posn.reshape(-1), dp.reshape(-1))
        return dict(x=x, n=N, cnt=None, esrc=esrc[:-1], edst=edst[:-1], edge_ptr=edge_ptr.to(torch.int32),
                    node_ptr=torch.arange(n + 1, dtype=torch.int32, device=rows.device) * N,
                    src=torch.where(live, sp, 0).long(), dst=torch.where(live, dp, 0).long(), mask=live.float())

    def sample(self, batch_size: int) -> "DeviceBatch":
        idx = torch.from_numpy(np.asarray(random.sample(range(self.count), batch_size), np.int64)).to(self.device)
        rows = self.R.index_select(0, idx)
        nf, E = self.N * self.F, self.e_max
        off = 2 * nf + 4 * E
        done = (rows[:, off + 4] > 0.5)[:, None]
        # terminal transitions: the own state as a masked placeholder for the missing next state (as `DeviceBatch` does)
        nxt = rows.clone()
        nxt[:, nf:2 * nf] = torch.where(done, rows[:, :nf], rows[:, nf:2 * nf])
        nxt[:, 2 * nf + 2 * E:off] = torch.where(done, rows[:, 2 * nf:2 * nf + 2 * E], rows[:, 2 * nf + 2 * E:off])
        nxt[:, off + 1] = torch.where(done[:, 0], rows[:, off], rows[:, off + 1])
        return DeviceBatch.from_arrays(self, self._graphs(rows, 0), self._graphs(nxt, 1), nonfinal=(~done[:, 0]).float(),
                                       reward=rows[:, off + 3].contiguous(), action=rows[:, off + 2].to(torch.int64).reshape(-1, 1))


def allgather_records(ctx: DistContext, rec: torch.Tensor) -> torch.Tensor:
    """One all-gather of the (B, record) tensors of all ranks -> (world * B, record), rank order (RCCL: one call)."""
    if not ctx.multi:
        return rec
    out = torch.empty((ctx.world * rec.shape[0], rec.shape[1]), dtype=rec.dtype, device=rec.device)
    try:
        dist.all_gather_into_tensor(out, rec.contiguous())
    except (RuntimeError, NotImplementedError):      # backends without the flat form (older gloo)
        bufs = [torch.empty_like(rec) for _ in range(ctx.world)]
        dist.all_gather(bufs, rec.contiguous())
        out = torch.cat(bufs)
    return out


def allgather_records_into(ctx: DistContext, R: torch.Tensor, base: int, B: int, W: int):
    """The record all-gather of the device loop, IN PLACE in the record ring `R`: every rank has written its B finished
    records at `base` = group base + rank * B; afterwards the group of W = world * B rows holds everybody's records in
    rank order on every rank.  RCCL: the in-place form of the all-gather (the input is this rank's slice of the output:
    no staging copy, no copy back); other backends (gloo, CPU tests) go through a staging buffer.  Enqueued on the
    CURRENT stream."""
    gp = base // W
    out, inp = R[gp * W:(gp + 1) * W], R[base:base + B]
    if dist.get_backend() == "nccl":
        dist.all_gather_into_tensor(out, inp)
    else:
        out.copy_(allgather_records(ctx, inp.clone()))


def allgather_transitions(ctx: DistContext, trs: List[Transition], n_nodes: int, n_feat: int, e_max: int):
    """All ranks contribute the same number of transitions per call (one per environment step)."""
    rec = pack_transitions(trs, n_nodes, n_feat, e_max).to(ctx.device)
    if not ctx.multi:
        return unpack_transitions(rec, n_nodes, n_feat, e_max)
    bufs = [torch.empty_like(rec) for _ in range(ctx.world)]
    dist.all_gather(bufs, rec)
    return unpack_transitions(torch.cat(bufs), n_nodes, n_feat, e_max)


# ---------------------------------------------------------------------------- trainer

class DQNTrainer:
    def __init__(self, n_actions: int, num_inputs: int, ctx: Optional[DistContext] = None, lr=1e-5, weight_decay=1e-6,
                 batch_size=32, gamma=1.0, target_update=50, replay_capacity=10000, conv_width=128, topk=0.1,
                 seed=1370, dense: bool = True, e_max: int = 1536):
        self.ctx = ctx or DistContext()
        self.dense, self.e_max = bool(dense), int(e_max)   # static-shape autograd path for equal-sized graphs
        dev = self.ctx.device
        self.graphs = dev.type == "cuda"                   # replay forward + backward as a HIP graph when possible
        self._graphs, self._graph_error = {}, None
        torch.manual_seed(seed)  # identical initial replicas on every rank (airfoil_dqn.py:28-32)
        self.policy_net_1 = NodeRemovalNet(n_actions + 1, conv_width=conv_width, topk=topk).float()
        self.policy_net_2 = NodeRemovalNet(n_actions + 1, conv_width=conv_width, topk=topk).float()
        self.policy_net_1.set_num_nodes(num_inputs)
        self.policy_net_2.set_num_nodes(num_inputs)
        self.policy_net_1.to(dev)
        self.policy_net_2.to(dev)
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
        random.seed(seed + self.ctx.rank)
        np.random.seed(seed + self.ctx.rank)

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
        if devb is not None:
            pass
        elif lazy:   # replay filled by train_loop_vec: minibatch arrays without per-graph Data objects
            s_refs = list(batch.state)
            n_refs = [(s_ if s_ is not None else batch.state[i]) for i, s_ in enumerate(batch.next_state)]
        else:
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
                from .gcn_fused import FusedGcn
                ga = devb.ga if devb is not None else gather_state_refs(s_refs, self.e_max, dev)
                gb = devb.gb if devb is not None else gather_state_refs(n_refs, self.e_max, dev)
                other = self.policy_net_2 if sel else self.policy_net_1
                if not hasattr(other, "_fused"):
                    other._fused = FusedGcn(other)
                go = gb if sel else ga
                with torch.no_grad():
                    qo = other._fused.forward_arrays(go["x"], go["node_ptr"], go["esrc"], go["edst"], go["edge_ptr"],
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
        self.opts[k].step()
        self.scheds[k].step()
        self.num_grads += 1
        self.losses.append(float(g["loss"].item()))
        return self.losses[-1]

    def optimize(self, transitions: Optional[List[Transition]] = None):
        """One optimiser step (airfoil_dqn.py:315-340 + :184-200 + :286-310): local loss/backward, ONE flat
        all-reduce of the gradient over all ranks, identical Adam step on every rank."""
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
        if not loss.requires_grad:
            # every sampled transition is terminal while the target network is the trained one (select False):
            # nothing depends on the parameters.  All ranks still join the all-reduce with a zero gradient.
            flat = torch.zeros(sum(p.numel() for p in net.parameters()), device=self.ctx.device)
            self.ctx.allreduce_mean_(flat)
            net.set_flat_gradients(flat)
            self.opts[k].step()
            self.scheds[k].step()
            self.num_grads += 1
            self.losses.append(float(loss.item()))
            return self.losses[-1]
        loss.backward()
        flat = net.flat_gradients()
        self.ctx.allreduce_mean_(flat)
        net.set_flat_gradients(flat)
        self.opts[k].step()
        self.scheds[k].step()
        self.num_grads += 1
        self.losses.append(float(loss.item()))
        return self.losses[-1]

    # --- learning on the device: hand-written forward + backward, replay sampling and Adam as kernels --------------
    def _fused_of(self, net, role: str = "act"):
        """The packed device copy of `net`'s parameters + launchers.  Two copies per network: "act" (the Q-forward of
        the env step, repacked on the MAIN stream of a device loop, only behind the event of the last optimiser chain)
        and "train" (the learning step and its no-grad forward, repacked on the OPTIMISER stream, in order with the
        `mdq_adam_step` launches of that stream) - one shared copy was repacked by the acting forward while the Adam
        kernel of the other stream was writing the parameters."""
        from .gcn_fused import FusedGcn
        attr = "_fused" if role == "act" else "_fused_train"
        if not hasattr(net, attr):
            setattr(net, attr, FusedGcn(net))
        return getattr(net, attr)

    def _adam_state(self, k: int, total: int):
        """Flat first / second moment buffers of network k laid out like the flat gradient.  The entries of the torch
        optimiser's `state` ARE views of them (so `state_dict()` checkpoints, `load_state_dict` and an occasional
        `opts[k].step()` on the host path all see the same moments); after a `load_state_dict` the loaded tensors are
        copied in and re-aliased."""
        net, opt = (self.policy_net_1, self.policy_net_2)[k], self.opts[k]
        ad = getattr(self, "_adam", None)
        if ad is None:
            ad = self._adam = [None, None]
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
        from .gcn_fused import PACK_MAX
        import ctypes as C

        class AdamDesc(C.Structure):
            _fields_ = [("n", C.c_int32), ("_pad", C.c_int32), ("param", C.c_void_p * PACK_MAX),
                        ("offset", C.c_int32 * PACK_MAX), ("len", C.c_int32 * PACK_MAX), ("grad", C.c_void_p),
                        ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("lr", C.c_double), ("beta1", C.c_double),
                        ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
                        ("bias_correction1", C.c_double), ("bias_correction2", C.c_double)]
        d = AdamDesc()
        if len(prm) > PACK_MAX:
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
        import ctypes as C
        from . import _lib
        opt = self.opts[k]
        a = self._adam_state(k, flat.numel())
        g = opt.param_groups[0]
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("mdq_adam_step: amsgrad / maximize are not supported")
        for p_ in a["params"]:
            opt.state[p_]["step"] += 1
        step = float(opt.state[a["params"][0]]["step"])
        d = a["desc"]
        if any(d.param[i] != p_.data_ptr() for i, p_ in enumerate(a["params"][:1])):
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
        the other on a fixed random minibatch: the kernels of `optimize_device`, no parameter is changed) through a few
        real env steps with the loop's own synchronisation; the fastest stays.  The environments are reset afterwards."""
        dev = self.ctx.device
        main = torch.cuda.current_stream(dev)
        from . import streams as _st
        if _st.roles_own_queues(dev):
            roles = _st.role_streams(dev)
            flow_now = getattr(venv, "_flow_stream", None)
            if (getattr(self, "_opt_stream", None) is roles["opt"] and (flow_now is None or flow_now is roles["flow"]) and
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
                    qo = f2.forward_arrays(x, node_ptr, esrc, edst, edge_ptr, N, EM)
                    f1.train_step(x, node_ptr, esrc, edst, edge_ptr, N, EM, 0, qo, action, reward, nonfinal, self.gamma)
                venv.rollout_step(ro, fused_act)
            main.wait_stream(cand)
            e1.record(main)
            venv.rollout_end(ro)
            e1.synchronize()
            return e0.elapsed_time(e1) / k
        results = []
        for t in range(max(1, int(tries))):
            cand = self._opt_stream if (t == 0 and getattr(self, "_opt_stream", None) is not None) else torch.cuda.Stream(device=dev)
            timed(cand, 2)
            results.append((timed(cand, int(steps)), cand))
            ms = [r[0] for r in results]
            if len(ms) >= 2 and min(ms) < 0.85 * max(ms) and ms[-1] <= 1.03 * min(ms):
                break
        self._opt_stream = min(results, key=lambda r: r[0])[1]
        self._opt_calibrated_for = (main, getattr(venv, "_flow_stream", None))
        self.opt_calibration_ms = [r[0] for r in results]
        venv.reset_all()
        return self.opt_calibration_ms

    def optimize_device(self, rep: "SharedDeviceReplay", idx, loss_out: Optional[torch.Tensor] = None):
        """One optimiser step on a minibatch of the record ring WITHOUT host synchronisation and without autograd:
        `mdq_replay_sample` (records `idx` -> graph arrays), fused forward of the network without gradient,
        `mdq_gcn_train_step` of the other one (forward + double-DQN Huber loss + backward), ONE flat all-reduce over the
        ranks, `mdq_adam_step`.  Everything is enqueued on the current stream; the loss goes to `loss_out` (a (1,)
        device tensor, e.g. a slot of a log ring) and is also returned as a device tensor.  Same `select` toggling as
        `optimize` (airfoil_dqn.py:315-340 + :184-200 + :240-310)."""
        import ctypes as C
        from . import _lib
        from .gcn_fused import FusedGcn  # noqa: F401
        dev = self.ctx.device
        if (self.num_grads % self.target_update) == 0:
            self.select = not self.select
        sel = self.select
        k = 0 if sel else 1
        net, other = ((self.policy_net_1, self.policy_net_2) if sel else (self.policy_net_2, self.policy_net_1))
        mb, N, F, EM = len(idx), rep.N, rep.F, rep.e_max
        bufs = getattr(self, "_mb_bufs", None)
        if bufs is None or bufs["key"] != (mb, N, F, EM):
            i32, f32 = torch.int32, torch.float32

            class SampleDesc(C.Structure):
                _fields_ = [("n", C.c_int32), ("rec_len", C.c_int32), ("nf", C.c_int32), ("EM", C.c_int32)] + \
                           [(nm, C.c_void_p) for nm in ("R", "idx", "x_s", "x_n", "esrc_s", "edst_s", "esrc_n", "edst_n",
                                                        "edge_ptr_s", "edge_ptr_n", "action", "reward", "nonfinal")]
            bufs = dict(key=(mb, N, F, EM), idx=torch.empty(mb, dtype=i32, device=dev),
                        x_s=torch.empty((mb, N, F), dtype=f32, device=dev), x_n=torch.empty((mb, N, F), dtype=f32, device=dev),
                        esrc_s=torch.zeros(mb * EM, dtype=i32, device=dev), edst_s=torch.zeros(mb * EM, dtype=i32, device=dev),
                        esrc_n=torch.zeros(mb * EM, dtype=i32, device=dev), edst_n=torch.zeros(mb * EM, dtype=i32, device=dev),
                        edge_ptr_s=torch.zeros(mb + 1, dtype=i32, device=dev), edge_ptr_n=torch.zeros(mb + 1, dtype=i32, device=dev),
                        action=torch.zeros(mb, dtype=torch.int64, device=dev), reward=torch.zeros(mb, dtype=f32, device=dev),
                        nonfinal=torch.zeros(mb, dtype=f32, device=dev),
                        node_ptr=torch.arange(mb + 1, dtype=i32, device=dev) * N)
            d = SampleDesc()
            d.n, d.rec_len, d.nf, d.EM = mb, rep.rec_len, N * F, EM
            for nm in ("idx", "x_s", "x_n", "esrc_s", "edst_s", "esrc_n", "edst_n", "edge_ptr_s", "edge_ptr_n", "action",
                       "reward", "nonfinal"):
                setattr(d, nm, bufs[nm].data_ptr())
            bufs["desc"] = d
            self._mb_bufs = bufs
        b = bufs
        if torch.is_tensor(idx):      # already on the device (the loop uploads a whole chunk of minibatches at once)
            if idx.dtype != torch.int32 or idx.device.type != "cuda" or not idx.is_contiguous():
                raise ValueError("optimize_device: device indices must be contiguous int32")
            b["desc"].idx = idx.data_ptr()
        else:
            b["idx"].copy_(torch.as_tensor(np.asarray(idx, dtype=np.int32)))     # (pageable source: a blocking copy)
            b["desc"].idx = b["idx"].data_ptr()
        b["desc"].R = rep.R.data_ptr()
        _lib.check(_lib.load().mdq_replay_sample(C.byref(b["desc"]), _lib.stream_ptr()), "mdq_replay_sample")
        gs = dict(x=b["x_s"], esrc=b["esrc_s"], edst=b["edst_s"], edge_ptr=b["edge_ptr_s"])
        gn = dict(x=b["x_n"], esrc=b["esrc_n"], edst=b["edst_n"], edge_ptr=b["edge_ptr_n"])
        go, gd = (gn, gs) if sel else (gs, gn)
        qo = self._fused_of(other, "train").forward_arrays(go["x"], b["node_ptr"], go["esrc"], go["edst"], go["edge_ptr"], N, EM)
        loss, flat = self._fused_of(net, "train").train_step(gd["x"], b["node_ptr"], gd["esrc"], gd["edst"], gd["edge_ptr"], N, EM,
                                                    0 if sel else 1, qo, b["action"], b["reward"], b["nonfinal"], self.gamma,
                                                    loss_out=loss_out)
        if self.ctx.multi:
            self.ctx.allreduce_mean_(flat)
        self._adam_step_device(k, flat)
        self.num_grads += 1
        return loss

    def state_dicts(self):
        return self.policy_net_1.state_dict(), self.policy_net_2.state_dict()

    def save(self, save_dir, prefix="", extra: Optional[dict] = None):
        """`ParameterServer.write` (airfoil_dqn.py:214-218): PyG-keyed state dicts `{prefix}policy_net_{1,2}.pt`, plus
        `{prefix}trainer_state.pt` (both Adam states, both schedulers, gradient count, the double-DQN toggle and
        whatever the loop hands over in `extra`, e.g. its epsilon step counters) - what a restart needs beyond the
        reference's two files."""
        os.makedirs(save_dir, exist_ok=True)
        torch.save(self.policy_net_1.state_dict(), os.path.join(save_dir, f"{prefix}policy_net_1.pt"))
        torch.save(self.policy_net_2.state_dict(), os.path.join(save_dir, f"{prefix}policy_net_2.pt"))
        torch.save(dict(opts=[o.state_dict() for o in self.opts], scheds=[s_.state_dict() for s_ in self.scheds],
                        num_grads=self.num_grads, select=self.select, extra=extra or {}),
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
        elif scheduler_steps:
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")       # (scheduler stepped before the optimiser: intended here)
                for s_ in self.scheds:
                    for _ in range(int(scheduler_steps)):
                        s_.step()
        return extra


def train_loop_per_worker(trainer: DQNTrainer, env_factory, num_episodes: int, max_steps: Optional[int] = None,
                          eps_decay=10000, eps_start=1.0, eps_end=0.01, share_replay=False, e_max=None):
    """Rollout loop of one rank (airfoil_dqn.py:428-503): epsilon-greedy over N_closest+1 actions, push the
    transition, optimise, rebuild the env every episode.  Returns per-episode reward lists.

    With more than one rank every step issues collectives (the gradient all-reduce of `optimize`, the transition
    all-gather), so all ranks must take the SAME number of steps: episode lengths differ between ranks (per-rank
    seeds), hence the loop must be bounded by `max_steps` (episodes are then cut at that common step count)."""
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


def _episode_airfoil(venv, b):
    """Airfoil of environment b of a batch over several airfoils (TrainingLog's `airfoil.npy`), None for one airfoil."""
    return int(venv.airfoil[b]) if getattr(venv, "A", 1) > 1 else None


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


class StateRef:
    """One environment's state graph inside a batched state dict of `VecEnv2DAirfoil.get_state()`, materialised as a
    `Data` only when a sampled transition needs it (the replay ring holds 128 of these per batched step; building
    `Data` objects eagerly cost more than the environment step itself)."""
    __slots__ = ("st", "b", "e0", "e1", "_data")

    def __init__(self, st, b, e0, e1):
        self.st, self.b, self.e0, self.e1, self._data = st, b, e0, e1, None

    def data(self) -> Data:
        if self._data is None:
            st = self.st
            self._data = Data(x=st["x"][self.b], edge_index=torch.stack([st["esrc"][self.e0:self.e1].long(),
                                                                          st["edst"][self.e0:self.e1].long()]))
        return self._data

    # the little of the Data interface the trainer / the transition packing use
    @property
    def x(self):
        return self.data().x

    @property
    def edge_index(self):
        return self.data().edge_index

    def to(self, device):
        return self.data().to(device)


def gather_state_refs(refs: List["StateRef"], e_max: int, device):
    """Minibatch arrays straight from lazy state references, without materialising per-graph `Data` objects:
    x (B,n,F) f32; esrc / edst (sumE,) i32 local node ids + edge_ptr (B+1,) i32 + node_ptr for the fused forward;
    src / dst (B,e_max) i64 + mask (B,e_max) f32 for the dense autograd path.  A handful of kernels per minibatch."""
    B = len(refs)
    x = torch.stack([r.st["x"][r.b] for r in refs]).to(device)
    n = x.shape[1]
    cnt = np.array([r.e1 - r.e0 for r in refs], dtype=np.int64)
    if cnt.max(initial=0) > e_max:
        raise ValueError(f"graph with {int(cnt.max())} edges exceeds e_max {e_max}")
    total = int(cnt.sum())
    if total:
        esrc = torch.cat([r.st["esrc"][r.e0:r.e1] for r in refs]).to(device)
        edst = torch.cat([r.st["edst"][r.e0:r.e1] for r in refs]).to(device)
    else:
        esrc = edst = torch.zeros(0, dtype=torch.int32, device=device)
    edge_ptr = np.zeros(B + 1, np.int32)
    np.cumsum(cnt, out=edge_ptr[1:])
    src = torch.zeros((B, e_max), dtype=torch.long, device=device)
    dst = torch.zeros((B, e_max), dtype=torch.long, device=device)
    mask = torch.zeros((B, e_max), dtype=torch.float32, device=device)
    if total:
        rows = np.repeat(np.arange(B, dtype=np.int64), cnt)
        cols = np.arange(total, dtype=np.int64) - np.repeat(edge_ptr[:-1].astype(np.int64), cnt)
        lin = torch.from_numpy(rows * e_max + cols).to(device)
        src.view(-1).scatter_(0, lin, esrc.long())
        dst.view(-1).scatter_(0, lin, edst.long())
        mask.view(-1).scatter_(0, lin, torch.ones(total, dtype=torch.float32, device=device))
    return dict(x=x, n=n, cnt=cnt, esrc=esrc.to(torch.int32), edst=edst.to(torch.int32),
                edge_ptr=torch.from_numpy(edge_ptr).to(device),
                node_ptr=torch.arange(B + 1, dtype=torch.int32, device=device) * n, src=src, dst=dst, mask=mask)


class DeviceBatch:
    """A sampled minibatch of a `DeviceReplay`: everything `_optimize_graphed` needs, already on the device."""

    def __init__(self, replay, s_slots, n_slots, actions, rewards):
        dev = replay.device
        self.replay, self.s_slots, self.n_slots = replay, s_slots, n_slots
        self.n = len(s_slots)
        self.nonfinal = torch.from_numpy((n_slots >= 0).astype(np.float32)).to(dev)
        self.reward = torch.from_numpy(rewards.astype(np.float32)).to(dev)
        self.action = torch.from_numpy(actions.astype(np.int64)).reshape(-1, 1).to(dev)
        self.ga = replay.gather(s_slots)
        self.gb = replay.gather(np.where(n_slots >= 0, n_slots, s_slots))   # terminal: own state as a masked placeholder

    @classmethod
    def from_arrays(cls, replay, ga, gb, nonfinal, reward, action):
        """A minibatch whose arrays are already gathered (`SharedDeviceReplay.sample`)."""
        self = cls.__new__(cls)
        self.replay, self.s_slots, self.n_slots = replay, None, None
        self.n = int(reward.shape[0])
        self.nonfinal, self.reward, self.action, self.ga, self.gb = nonfinal, reward, action, ga, gb
        return self

    def __len__(self):
        return self.n

    def to_transitions(self) -> List[Transition]:
        """The same minibatch as `Transition`s of `Data` graphs (eager fallback, tests)."""
        if self.s_slots is None:       # gathered arrays: rebuild the graphs from them
            out = []
            ep0, ep1 = self.ga["edge_ptr"].cpu().numpy(), self.gb["edge_ptr"].cpu().numpy()
            nf = self.nonfinal.cpu().numpy()
            for i in range(self.n):
                def graph(g, ep):
                    return Data(x=g["x"][i].clone(), edge_index=torch.stack([g["esrc"][ep[i]:ep[i + 1]].long(),
                                                                              g["edst"][ep[i]:ep[i + 1]].long()]))
                out.append(Transition(graph(self.ga, ep0), self.action[i].reshape(1, 1).cpu(),
                                      graph(self.gb, ep1) if nf[i] > 0.5 else None, self.reward[i].reshape(1).cpu()))
            return out
        rp = self.replay
        act, rew = self.action.cpu(), self.reward.cpu()
        return [Transition(rp.data(int(self.s_slots[i])), act[i].reshape(1, 1),
                           rp.data(int(self.n_slots[i])) if self.n_slots[i] >= 0 else None, rew[i].reshape(1))
                for i in range(self.n)]


class DeviceReplay:
    """Replay ring of the batched loop, resident on the GPU (the reference's `ReplayMemory`, airfoil_dqn.py:48-67, for
    B environments stepped together).  Every batched state is stored ONCE - node features (B,N,F) f32 and the padded
    edge lists (B,e_max) i32 of `VecEnv2DAirfoil.get_state()` copied into ring tensors, three copy kernels per
    step - and a transition is four host numbers (state slot, next-state slot or -1, action, reward).  Sampling a
    minibatch is a few gathers instead of a Python loop over per-graph objects.  Holds capacity/B + 2 batched states
    so that the next state of the oldest live transition is still there."""

    def __init__(self, capacity: int, B: int, N: int, F: int, e_max: int, device):
        self.capacity, self.B, self.N, self.F, self.e_max, self.device = int(capacity), B, N, F, e_max, device
        self.K = (self.capacity + B - 1) // B + 2
        S = self.K * B
        self.RX = torch.zeros((S, N, F), dtype=torch.float32, device=device)
        self.RS = torch.zeros((S, e_max), dtype=torch.int32, device=device)
        self.RD = torch.zeros((S, e_max), dtype=torch.int32, device=device)
        self.cnt = np.zeros(S, np.int64)
        self.t_s = np.zeros(self.capacity, np.int64)
        self.t_n = np.zeros(self.capacity, np.int64)
        self.t_a = np.zeros(self.capacity, np.int64)
        self.t_r = np.zeros(self.capacity, np.float32)
        self.position, self.count, self.step = 0, 0, 0
        self._cols = torch.arange(e_max, device=device)[None, :]

    @staticmethod
    def eligible(st: dict, e_max: int) -> bool:
        return "edge_src_pad" in st and st["edge_src_pad"].shape[1] == e_max

    def store(self, st: dict) -> int:
        """Copy a batched state into the ring; returns the slot of its environment 0."""
        base = (self.step % self.K) * self.B
        self.step += 1
        self.RX[base:base + self.B].copy_(st["x"])
        self.RS[base:base + self.B].copy_(st["edge_src_pad"])
        self.RD[base:base + self.B].copy_(st["edge_dst_pad"])
        self.cnt[base:base + self.B] = st["nedges"]
        return base

    def push(self, base_prev: int, base_next: int, actions, rewards, dones):
        """B transitions (state slot base_prev + b -> base_next + b, -1 if terminal)."""
        B = self.B
        pos = (self.position + np.arange(B)) % self.capacity
        self.t_s[pos] = base_prev + np.arange(B)
        self.t_n[pos] = np.where(np.asarray(dones, bool), -1, base_next + np.arange(B))
        self.t_a[pos] = np.asarray(actions, np.int64)
        self.t_r[pos] = np.asarray(rewards, np.float32)
        self.position = int((self.position + B) % self.capacity)
        self.count = min(self.count + B, self.capacity)

    def size(self):
        return self.count

    __len__ = size

    def sample(self, batch_size: int) -> DeviceBatch:
        idx = np.asarray(random.sample(range(self.count), batch_size), np.int64)
        return DeviceBatch(self, self.t_s[idx], self.t_n[idx], self.t_a[idx], self.t_r[idx])

    def gather(self, slots) -> dict:
        """Minibatch arrays of the states in `slots` (same keys as `gather_state_refs`)."""
        dev, e_max, n = self.device, self.e_max, len(slots)
        idx_d = torch.from_numpy(np.asarray(slots, np.int64)).to(dev)
        cnt = self.cnt[slots]
        x = self.RX.index_select(0, idx_d)
        sp, dp = self.RS.index_select(0, idx_d), self.RD.index_select(0, idx_d)
        live = self._cols < torch.from_numpy(cnt).to(dev)[:, None]
        src = torch.where(live, sp, 0).long()          # (slots past the count hold stale entries of earlier steps)
        dst = torch.where(live, dp, 0).long()
        edge_ptr = np.zeros(n + 1, np.int32)
        np.cumsum(cnt, out=edge_ptr[1:])
        flat = np.arange(int(edge_ptr[-1]), dtype=np.int64) + np.repeat(np.arange(n, dtype=np.int64) * e_max - edge_ptr[:-1], cnt)
        flat_d = torch.from_numpy(flat).to(dev)
        return dict(x=x, n=self.N, cnt=cnt, esrc=sp.reshape(-1).index_select(0, flat_d), edst=dp.reshape(-1).index_select(0, flat_d),
                    edge_ptr=torch.from_numpy(edge_ptr).to(dev),
                    node_ptr=torch.arange(n + 1, dtype=torch.int32, device=dev) * self.N, src=src, dst=dst,
                    mask=live.float())

    def data(self, slot: int) -> Data:
        c = int(self.cnt[slot])
        return Data(x=self.RX[slot].clone(), edge_index=torch.stack([self.RS[slot, :c].long(), self.RD[slot, :c].long()]))


def state_to_data_list(st: dict, n_nodes: int) -> List[Data]:
    """Split the batched state dict of `VecEnv2DAirfoil.get_state()` into per-environment `Data` objects
    (x (N,F) f32, edge_index (2,E) i64 with node ids local to the graph)."""
    return [r.data() for r in state_refs(st)]


def state_refs(st: dict) -> List[StateRef]:
    """Per-environment lazy references into a batched state dict (one host read of the edge offsets)."""
    ep = st["edge_ptr"].cpu().numpy()
    return [StateRef(st, b, int(ep[b]), int(ep[b + 1])) for b in range(st["x"].shape[0])]


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
    from .gcn_fused import FusedGcn
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
    overlap = overlap_optimise and rep_dev is not None and hasattr(venv, "step_begin") and ctx.device.type == "cuda"
    if overlap:
        if getattr(trainer, "_opt_stream", None) is None:
            from .streams import concurrent_stream
            trainer._opt_stream = concurrent_stream(ctx.device, [getattr(venv, "_flow_stream", None)])
        opt_stream, ev_store = trainer._opt_stream, torch.cuda.Event()
        ev_store.record(torch.cuda.current_stream(ctx.device))
    rewards, dones_hist = [], []
    ep_r = [[] for _ in range(B)]
    ep_a = [[] for _ in range(B)]
    for step_no in range(num_steps):
        with torch.no_grad():
            q = fused.forward_arrays(st["x"], st["node_ptr"], st["esrc"], st["edst"], st["edge_ptr"], N, venv.EMAX,
                                     edge_counts=st["nedges"])
        greedy = q.argmax(1).cpu().numpy()
        eps = eps_end + (eps_start - eps_end) * np.exp(-1.0 * steps_done / eps_decay)
        steps_done += 1
        explore = np.random.random(B) <= eps
        actions = np.where(explore, np.random.randint(0, trainer.n_actions + 1, B), greedy)
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
            rep_dev.push(base_prev, base_next, actions, rew, done)
            base_prev = base_next
        elif rep_dev is not None:
            st, rew, done, _ = venv.step(actions)
            base_next = rep_dev.store(st)
            rep_dev.push(base_prev, base_next, actions, rew, done)
            base_prev = base_next
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
        for _k in range(0 if overlap else optim_per_step):
            loss = trainer.optimize()
            if log is not None and loss is not None:
                log.add_loss(loss)
        if log is not None:
            log.add_eps(float(eps.mean()))
            for b in range(B):
                ep_r[b].append(float(rew[b]))
                ep_a[b].append(int(actions[b]))
                if done[b]:
                    log.add_episode(ep_r[b], ep_a[b], _episode_airfoil(venv, b))
                    ep_r[b], ep_a[b] = [], []
        rewards.append(rew.copy())
        dones_hist.append(done.copy())
        if every and on_every is not None and (step_no + 1) % every == 0:
            on_every(step_no + 1, steps_done)
    return dict(rewards=np.array(rewards), dones=np.array(dones_hist), losses=list(trainer.losses), steps_done=steps_done)


def train_loop_device(trainer: DQNTrainer, venv, num_steps: int, optim_per_step: int = 1, eps_decay=10000, eps_start=1.0,
                      eps_end=0.01, share_replay=False, log: Optional["TrainingLog"] = None, steps_done0=None, every: int = 0,
                      on_every=None, chunk: int = 64, optimiser_stream: str = "auto"):
    """`train_loop_vec` WITHOUT a host round trip inside a batched step (one rank of configs[3]): the environment step is
    `VecEnv2DAirfoil.rollout_step` (Q-forward, epsilon-greedy choice, vertex removal ... reward / reset logic as kernels),
    the B transitions go into the record ring with one launch (`mdq_replay_step`; with `share_replay` the ranks
    all-gather their B records per step), and the optimiser step (`DQNTrainer.optimize_device`: replay sampling,
    hand-written forward + backward, flat gradient all-reduce, Adam as kernels) runs on a side stream beside the
    latency-bound smoothing kernel of the same env step (`optimiser_stream`: the env's flow stream, behind the flow
    leg of the previous step, or a stream of its own).  The host only draws the random numbers (same streams as
    `train_loop_vec`: numpy for epsilon-greedy, `random.sample` for the minibatch) and enqueues; rewards / dones /
    losses are read back once per `chunk` steps.  Same returns as `train_loop_vec`."""
    from . import _lib
    ctx = trainer.ctx
    dev = ctx.device
    if dev.type != "cuda" or not getattr(venv, "gpu_remesh", False) or not venv.auto_reset:
        raise _lib.MeshDQNHipError("train_loop_device needs a GPU and a vector env with the device mesh engine and auto_reset")
    lib = _lib.load()
    B, N = venv.B, venv.N
    W = B * ctx.world if (share_replay and ctx.multi) else B     # records per batched step in this rank's ring
    steps_done = np.zeros(B, np.int64) if steps_done0 is None else np.asarray(steps_done0, np.int64).copy()
    fused1 = trainer._fused_of(trainer.policy_net_1)
    main = torch.cuda.current_stream(dev)
    if main == torch.cuda.default_stream(dev):
        # the loop does not run on the legacy default stream (see VecEnv2DAirfoil.rollout_device): a stream of its own
        if getattr(trainer, "_main_stream", None) is None:
            from .streams import role_streams
            trainer._main_stream = role_streams(dev)["main"]
        trainer._main_stream.wait_stream(main)
        with torch.cuda.stream(trainer._main_stream):
            out = train_loop_device(trainer, venv, num_steps, optim_per_step=optim_per_step, eps_decay=eps_decay,
                                    eps_start=eps_start, eps_end=eps_end, share_replay=share_replay, log=log,
                                    steps_done0=steps_done0, every=every, on_every=on_every, chunk=chunk,
                                    optimiser_stream=optimiser_stream)
        main.wait_stream(trainer._main_stream)
        return out
    # (torch.cuda.Stream defines `==` between streams only: `None != stream` is False, hence the explicit tests)
    cal = getattr(venv, "_calibrated_for", None)
    if getattr(venv, "flow_overlap", False) and (cal is None or not (cal == main)):
        venv.calibrate_streams(fused1)       # (a flow stream that really overlaps with this loop's stream; resets the envs)
    # "auto": a stream of its own.  (With the 1.8 ms smoothing walk the optimiser chain rode on the flow stream behind the flow
    # leg - 1.05 + 0.6 ms still ended before the main chain; since the blocked smoothing solve the main chain is 1.16 ms and
    # that placement costs 1.63 ms per batched step against 1.41 ms with a third stream: tools/time_train_device.py.)
    if optimiser_stream == "auto":
        optimiser_stream = "own"
    on_flow = optimiser_stream == "flow" and getattr(venv, "flow_overlap", False)
    if on_flow:
        # the optimiser chain rides on the (calibrated) flow stream, behind the flow leg of the previous env step: one side
        # stream instead of two
        opt_stream = venv._flow_stream
    else:
        if getattr(trainer, "_opt_stream", None) is None:
            from .streams import role_streams
            trainer._opt_stream = role_streams(dev)["opt"]
        ocal, flow_now = getattr(trainer, "_opt_calibrated_for", None), getattr(venv, "_flow_stream", None)
        if ocal is None or not (ocal[0] == main) or not ((ocal[1] is None and flow_now is None) or
                                                         (ocal[1] is not None and flow_now is not None and ocal[1] == flow_now)):
            trainer.calibrate_opt_stream(venv, fused1)    # (an optimiser stream that really overlaps; resets the envs)
        opt_stream = trainer._opt_stream
    ev_opt = None
    rep = None
    rewards, dones_hist, losses, actions_hist = [], [], [], []
    ep_r = [[] for _ in range(B)]
    ep_a = [[] for _ in range(B)]
    step_no, prev = 0, None      # prev: (record base, act, rew, done) of the step whose records await their next state
    G = 0
    while step_no < num_steps:
        K = min(int(chunk), num_steps - step_no)
        # random numbers of the chunk, drawn step by step in train_loop_vec's order
        explore, rand_act, eps_mean = np.zeros((K, B), bool), np.zeros((K, B), np.int32), []
        for k in range(K):
            eps = eps_end + (eps_start - eps_end) * np.exp(-1.0 * steps_done / eps_decay)
            steps_done += 1
            explore[k] = np.random.random(B) <= eps
            rand_act[k] = np.random.randint(0, trainer.n_actions + 1, B)
            eps_mean.append(float(eps.mean()))
        ro = venv.rollout_begin(K, explore, rand_act)
        st = ro["state"]
        if rep is None:
            F = st["x"].shape[2]
            if st["edge_src_pad"].shape[1] != trainer.e_max:
                raise ValueError(f"vector env pads edge lists to {st['edge_src_pad'].shape[1]}, trainer.e_max is {trainer.e_max}")
            rep = trainer.device_memory
            cap = max(2, trainer.replay_capacity // W) * W          # whole groups of W records
            if not isinstance(rep, SharedDeviceReplay) or (rep.capacity, rep.N, rep.F) != (cap, N, F):
                rep = trainer.device_memory = SharedDeviceReplay(cap, N, F, trainer.e_max, dev)
            G = rep.capacity // W
            t0 = int(getattr(rep, "steps_pushed", 0))           # the ring continues where an earlier call stopped
            loss_ring = torch.zeros(int(chunk) * max(1, optim_per_step), dtype=torch.float32, device=dev)
        # minibatches of the chunk: the number of finished records at every step is known in advance; one upload
        mbs = []
        for k in range(K):
            t = t0 + step_no + k
            count = min(t, G - 1) * W                          # finished groups (the one being written is not)
            for _k in range(optim_per_step if count >= trainer.batch_size else 0):
                idx = np.asarray(random.sample(range(count), trainer.batch_size), np.int64)
                if t >= G:                                     # wrapped: skip over the group being written
                    idx = np.where(idx < (t % G) * W, idx, idx + W)
                mbs.append(idx.astype(np.int32))
        mb_dev = torch.from_numpy(np.stack(mbs)).to(dev) if mbs else None
        n_loss = 0
        for k in range(K):
            g = (t0 + step_no + k) % G                         # the ring group this step's records go to
            if ev_opt is not None:
                main.wait_event(ev_opt)                        # the weights of the previous optimiser step
            # the ACTING copy follows the parameters here and only here: behind the event of the last optimiser chain and
            # in front of the next one (which waits for `ev` below); rollout_step must not repack (pack=False): by then
            # the host has already bumped the version for an Adam kernel that is still in flight on the other stream
            fused1._pack()
            base_cur = g * W + (ctx.rank * B if W != B else 0)
            _lib.check(lib.mdq_replay_step(rep.R.data_ptr(), rep.rec_len, rep.capacity, B, N * st["x"].shape[2], rep.e_max,
                                           st["x"].data_ptr(), st["edge_src_pad"].data_ptr(), st["edge_dst_pad"].data_ptr(),
                                           st["nedges_dev"].data_ptr(), base_cur, -1 if prev is None else prev[0],
                                           None if prev is None else prev[1].data_ptr(), None if prev is None else prev[2].data_ptr(),
                                           None if prev is None else prev[3].data_ptr(), _lib.stream_ptr()), "mdq_replay_step")
            ev = torch.cuda.Event()
            ev.record(main)
            gather = prev is not None and W != B               # shared replay: everybody's finished records of that step
            do_opt = min(t0 + step_no + k, G - 1) * W >= trainer.batch_size
            if gather or do_opt:
                with torch.cuda.stream(opt_stream):
                    opt_stream.wait_event(ev)
                    if gather:
                        # on the optimiser stream, in front of the chain that may sample those records, in place in the ring
                        # (rank r's B records sit at group base + r * B on every rank): off the latency chain of the env step
                        allgather_records_into(ctx, rep.R, prev[0], B, W)
                    for _k in range(optim_per_step if do_opt else 0):
                        trainer.optimize_device(rep, mb_dev[n_loss], loss_out=loss_ring[n_loss:n_loss + 1])
                        n_loss += 1
                    ev_opt = torch.cuda.Event()
                    ev_opt.record(opt_stream)
            venv.rollout_step(ro, fused1, pack=False)
            prev = (base_cur, ro["act"][k], ro["rew"][k], ro["done"][k])
            st = ro["state"]
        if step_no + K >= num_steps and prev is not None:       # last chunk: finish the records of the last step too
            _lib.check(lib.mdq_replay_step(rep.R.data_ptr(), rep.rec_len, rep.capacity, B, N * st["x"].shape[2], rep.e_max,
                                           st["x"].data_ptr(), st["edge_src_pad"].data_ptr(), st["edge_dst_pad"].data_ptr(),
                                           st["nedges_dev"].data_ptr(), -1, prev[0], prev[1].data_ptr(), prev[2].data_ptr(),
                                           prev[3].data_ptr(), _lib.stream_ptr()), "mdq_replay_step")
            if W != B:
                if ev_opt is not None:
                    main.wait_event(ev_opt)
                allgather_records_into(ctx, rep.R, prev[0], B, W)
            rep.steps_pushed = t0 + num_steps
            rep.count = min(rep.steps_pushed, G) * W
            rep.position = (rep.steps_pushed % G) * W
        out = venv.rollout_end(ro)                              # the one synchronisation of the chunk
        if ev_opt is not None:
            ev_opt.synchronize()                                # (the last optimiser chain writes its loss on the side stream)
        new_losses = loss_ring[:n_loss].cpu().numpy().tolist()
        trainer.losses.extend(new_losses)
        losses.extend(new_losses)
        for k in range(K):
            rew, done = out["rewards"][k], out["dones"][k]
            rewards.append(rew.copy())
            dones_hist.append(done.copy())
            actions_hist.append(out["actions"][k].copy())
            if log is not None:
                log.add_eps(eps_mean[k])
                for b in range(B):
                    ep_r[b].append(float(rew[b]))
                    ep_a[b].append(int(out["actions"][k][b]))
                    if done[b]:
                        log.add_episode(ep_r[b], ep_a[b], _episode_airfoil(venv, b))
                        ep_r[b], ep_a[b] = [], []
        if log is not None:
            for l_ in new_losses:
                log.add_loss(l_)
        step_no += K
        if every and on_every is not None and (step_no // every) > ((step_no - K) // every):
            on_every(step_no, steps_done)
    return dict(rewards=np.array(rewards), dones=np.array(dones_hist), losses=list(trainer.losses), steps_done=steps_done,
                actions=np.array(actions_hist))
