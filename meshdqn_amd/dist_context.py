"""Process-group plumbing of the data-parallel trainer and its collectives on replay records."""
from __future__ import annotations

import os
from typing import List, Optional

import torch
import torch.distributed as dist

from .replay import Transition, pack_transitions, unpack_transitions


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
    return unpack_transitions(allgather_records(ctx, rec), n_nodes, n_feat, e_max)
