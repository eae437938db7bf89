"""Replay stores of the DQN trainer (airfoil_dqn.py:46-67) and the packing of their transitions: a host list of
`Transition`s, batched states stored once on the GPU, and a device ring of fixed-size records (see the classes)."""
from __future__ import annotations

import ctypes as C
import random
from collections import namedtuple
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from .data import Data

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
    `DeviceBatch` interface as `DeviceReplay` (minibatch arrays gathered by a few torch ops, nothing read back).

    The device loop (`grouped`) writes G groups of W records, one per batched step t (`steps_pushed` so far, over all its
    calls): group t % G is being written during step t - its records get s' one step later -, the others are finished.

    Prioritized replay (`prio_fill` / `prio_draw` / `prio_update`: the three `mdq_replay_prio_*` kernels on the current
    stream): the ring owns `prio` (capacity,) - (|td| + eps)^alpha of every record, 0 for a record that must not be drawn -
    and `pmax` (1,), the largest priority seen so far, started at 1; both are allocated on first use and, like the ring
    itself, are not part of a checkpoint.

    N-step returns (`nstep_desc`): record j + W (mod capacity) is the next transition of the environment of record j - the
    environments reset in place and every record stores `done` -, so `mdq_replay_sample_nstep` composes the n-step
    transition of a drawn record from the finished groups, stopping in front of the one being written."""

    def __init__(self, capacity: int, N: int, F: int, e_max: int, device):
        self.capacity, self.N, self.F, self.e_max, self.device = int(capacity), int(N), int(F), int(e_max), device
        self.rec_len = 2 * N * F + 4 * e_max + 5
        self.R = torch.zeros((self.capacity, self.rec_len), dtype=torch.float32, device=device)
        self.position, self.count = 0, 0
        self.W, self.G, self.steps_pushed = 1, self.capacity, 0
        self._cols = torch.arange(e_max, device=device)[None, :]
        self.prio = self.pmax = self._draw_desc = None

    @classmethod
    def grouped(cls, old, replay_capacity: int, W: int, N: int, F: int, e_max: int, device) -> "SharedDeviceReplay":
        """A ring of whole groups of W records (at least two); `old` is kept when it fits: a later loop call continues it."""
        cap = max(2, replay_capacity // W) * W
        rep = old if isinstance(old, cls) and (old.capacity, old.N, old.F) == (cap, N, F) else cls(cap, N, F, e_max, device)
        rep.W, rep.G = W, cap // W
        return rep

    def group_base(self, t: int) -> int:
        """First record of the group that step t writes."""
        return (t % self.G) * self.W

    def finished(self, t: int) -> int:
        """Number of finished (sampleable) records before step t: every group but the one being written."""
        return min(t, self.G - 1) * self.W

    def draw(self, t: int, batch_size: int) -> np.ndarray:
        """`batch_size` record numbers (int32) for a minibatch of step t, drawn from `random` like `sample`."""
        idx = np.asarray(random.sample(range(self.finished(t)), batch_size), np.int64)
        if t >= self.G:                                        # wrapped: skip over the group being written
            idx = np.where(idx < self.group_base(t), idx, idx + self.W)
        return idx.astype(np.int32)

    def nstep_desc(self, t: int, n_step: int, gamma: float, steps: Optional[torch.Tensor] = None, desc=None):
        """The `mdq_replay_nstep` of a minibatch of step t (a new one, or `desc` refilled): walks over the ring's groups that
        never step into the group step t writes.  `steps`: (n,) int32 device tensor for the composed lengths, or None."""
        if steps is not None and (steps.dtype != torch.int32 or steps.device.type != "cuda" or not steps.is_contiguous()):
            raise ValueError("nstep_desc wants a contiguous int32 device tensor for steps")
        d = desc if desc is not None else _lib.ReplayNstepDesc()
        d.n_step, d.W, d.capacity, d.head, d.gamma = int(n_step), self.W, self.capacity, self.group_base(t), float(gamma)
        d.steps = None if steps is None else steps.data_ptr()
        return d

    def step(self, st: dict, base_cur: int = -1, prev=None):
        """One `mdq_replay_step` launch on the current stream: the batched env state `st` becomes s of the records at `base_cur`
        and s' of those of `prev` = (base, action, reward, done of the step that led to `st`).  -1 / None: that half is skipped."""
        pb, pa, pr, pd = (-1, None, None, None) if prev is None else (prev[0],) + tuple(a.data_ptr() for a in prev[1:])
        _lib.check(_lib.load().mdq_replay_step(
            self.R.data_ptr(), self.rec_len, self.capacity, st["x"].shape[0], self.N * self.F, self.e_max, st["x"].data_ptr(),
            st["edge_src_pad"].data_ptr(), st["edge_dst_pad"].data_ptr(), st["nedges_dev"].data_ptr(), base_cur, pb, pa, pr, pd,
            _lib.stream_ptr()), "mdq_replay_step")

    def close(self, t: int):
        """After the last step of a loop call (t steps pushed in all, the last one's records finished as well)."""
        self.steps_pushed, self.count, self.position = t, min(t, self.G) * self.W, self.group_base(t)

    # --- proportional prioritized replay ----------------------------------------------------------------------
    def _prio(self):
        if self.prio is None:
            self.prio = torch.zeros(self.capacity, dtype=torch.float32, device=self.device)
            self.pmax = torch.ones(1, dtype=torch.float32, device=self.device)
        return self.prio

    def prio_ranges(self, t: int, new: bool = True, zero: bool = True):
        """(base_new, n_new, base_zero, n_zero) of `prio_fill(t)`."""
        n_new = self.W if (new and t > 0) else 0
        return (self.group_base(t - 1) if n_new else 0, n_new, self.group_base(t) if zero else 0, self.W if zero else 0)

    def prio_fill(self, t: int, new: bool = True, zero: bool = True):
        """In front of the minibatches of step t: the group of step t - 1, whose records have just received their next
        states, gets the largest priority so far (`new`; False where that step belongs to an earlier call, which has
        done it), the group step t writes gets 0 (`zero`; False after the last step of a call - `close` -, which writes
        no further group)."""
        bn, nn, bz, nz = self.prio_ranges(t, new, zero)
        _lib.check(_lib.load().mdq_replay_prio_fill(self._prio().data_ptr(), self.capacity, bn, nn, bz, nz, self.pmax.data_ptr(),
                                                    _lib.stream_ptr()), "mdq_replay_prio_fill")

    def prio_draw(self, u: torch.Tensor, beta: float, idx_out: torch.Tensor, w_out: torch.Tensor):
        """One stratified minibatch: `u` (n,) float64 uniforms on the device -> record numbers `idx_out` (n,) int32 and
        importance weights `w_out` (n,) float32 (both device, written in place)."""
        n = u.numel()
        for t_, dt in ((u, torch.float64), (idx_out, torch.int32), (w_out, torch.float32)):
            if t_.dtype != dt or t_.device.type != "cuda" or not t_.is_contiguous() or t_.numel() != n:
                raise ValueError(f"prio_draw wants contiguous device tensors of {n} entries: u float64, idx int32, weight float32")
        d = self._draw_desc = self._draw_desc or _lib.ReplayPrioDrawDesc()
        d.capacity, d.n, d.beta, d.prio = self.capacity, n, float(beta), self._prio().data_ptr()
        d.u, d.idx, d.weight = u.data_ptr(), idx_out.data_ptr(), w_out.data_ptr()
        _lib.check(_lib.load().mdq_replay_prio_draw(C.byref(d), _lib.stream_ptr()), "mdq_replay_prio_draw")

    def prio_update(self, idx: torch.Tensor, td: torch.Tensor, alpha: float, eps: float):
        """New priorities (|td| + eps)^alpha of the records `idx` (n,) int32 from their TD errors `td` (n,) float32."""
        n = idx.numel()
        if (idx.dtype != torch.int32 or td.dtype != torch.float32 or td.numel() != n or not idx.is_contiguous() or
                not td.is_contiguous() or idx.device.type != "cuda" or td.device.type != "cuda"):
            raise ValueError("prio_update wants contiguous device tensors: idx int32, td float32, of one length")
        _lib.check(_lib.load().mdq_replay_prio_update(self._prio().data_ptr(), self.capacity, n, idx.data_ptr(), td.data_ptr(),
                                                      float(alpha), float(eps), self.pmax.data_ptr(), _lib.stream_ptr()),
                   "mdq_replay_prio_update")

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
