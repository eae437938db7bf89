"""Fused HIP inference of `NodeRemovalNet` / `AirfoilGCNN` (host side of `mdq_gcn_forward`).

Packs the module's parameters (transposed to [in][out] so that consecutive lanes read consecutive
output channels), builds the per-graph node / edge ranges of a `Batch` and launches the two
kernels of meshdqn_amd/csrc/mdq_gcn.hip (inference) or the learning step of mdq_gcn_train.hip
(`FusedGcn.train_step`: forward + loss + backward without autograd).
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from ._lib import PACK_MAX


class GcnLevel(C.Structure):
    _fields_ = [("type", C.c_int32), ("fin", C.c_int32), ("w_l", C.c_void_p), ("b", C.c_void_p),
                ("w_r", C.c_void_p), ("pool_w", C.c_void_p)]


class GcnNet(C.Structure):
    _fields_ = [("nlevels", C.c_int32), ("C", C.c_int32), ("fin0", C.c_int32), ("out_dim", C.c_int32),
                ("ratio", C.c_double), ("softmax", C.c_int32), ("dueling", C.c_int32),
                ("levels", GcnLevel * 6),
                ("lin1_w", C.c_void_p), ("lin1_b", C.c_void_p), ("lin2_w", C.c_void_p), ("lin2_b", C.c_void_p),
                ("lin3_w", C.c_void_p), ("lin3_b", C.c_void_p), ("lin_v_w", C.c_void_p), ("lin_v_b", C.c_void_p)]


def _levels_of(net):
    """The conv / pool levels the forward runs, and whether a softmax follows lin3 (NodeRemovalNet: its `head` says;
    the "linear" and "dueling" heads have none)."""
    from .airfoilgcnn import AirfoilGCNN, NodeRemovalNet, check_head
    if isinstance(net, NodeRemovalNet):
        # conv3/pool3 and conv6/pool6 are skipped by the reference's forward (airfoilgcnn.py:106-110,124-128)
        return [(net.conv1, net.pool1), (net.conv2, net.pool2), (net.conv4, net.pool4), (net.conv5, net.pool5)], \
            check_head(net.head) == "softmax"
    if isinstance(net, AirfoilGCNN):
        return [(net.conv1, net.pool1), (net.conv2, net.pool2), (net.conv3, net.pool3),
                (net.conv4, net.pool4), (net.conv5, net.pool5), (net.conv6, net.pool6)], False
    raise TypeError(type(net))


class GcnGradLayout(C.Structure):
    _fields_ = [("w_l", C.c_int32 * 6), ("b", C.c_int32 * 6), ("w_r", C.c_int32 * 6), ("pool_w", C.c_int32 * 6),
                ("lin1_w", C.c_int32), ("lin1_b", C.c_int32), ("lin2_w", C.c_int32), ("lin2_b", C.c_int32),
                ("lin3_w", C.c_int32), ("lin3_b", C.c_int32), ("total", C.c_int32), ("lin_v", C.c_int32)]


class GcnTrainDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("NMAX", C.c_int32), ("EMAX", C.c_int32), ("mode", C.c_int32), ("gamma", C.c_double),
                ("x", C.c_void_p), ("node_ptr", C.c_void_p), ("esrc", C.c_void_p), ("edst", C.c_void_p),
                ("edge_ptr", C.c_void_p), ("q_other", C.c_void_p), ("action", C.c_void_p), ("reward", C.c_void_p),
                ("nonfinal", C.c_void_p), ("workspace", C.c_void_p), ("partial", C.c_void_p), ("grad", C.c_void_p),
                ("loss", C.c_void_p), ("out", C.c_void_p), ("layout", GcnGradLayout)]


class GcnPackTable(C.Structure):
    _fields_ = [("n", C.c_int32), ("_pad", C.c_int32), ("src", C.c_void_p * PACK_MAX), ("dst", C.c_void_p * PACK_MAX),
                ("rows", C.c_int32 * PACK_MAX), ("cols", C.c_int32 * PACK_MAX)]


class FusedGcn:
    """Device-side packed copy of a network's parameters + launchers (inference forward, learning step)."""

    def __init__(self, net):
        self.net = net
        self.lib = _lib.load()
        self._version = None
        self._table_key = None
        self._keep = []
        self.desc = None
        self._train_bufs = {}
        # noisy networks: (seed, stream, draw) of the noise the packed copy carries, None: the mean network
        self._noise = None
        self.noisy_desc = self.noisy_layout = self.eps = None

    def resample(self, seed: int, stream: int, draw: int):
        """Pack the parameters WITH noise (`mdq_gcn_pack_noisy`, one launch on the current stream, instead of
        `mdq_gcn_pack`): the dense head of the copy becomes mean + sigma * noise of Philox key (seed, stream), draw `draw`.
        The copy keeps that noise through later repacks (new parameters, same noise) until the next `resample` or
        `denoise`; `self.eps` holds {layer: (eps_in, eps_out)} device vectors the launch wrote, which `train_step` hands to
        `mdq_noisy_grad`."""
        if getattr(self.net, "noisy", None) is None:
            raise ValueError("resample: the network was built without noisy=sigma0")
        seed, stream, draw = int(seed), int(stream), int(draw)
        if not (0 <= seed < 2 ** 32 and 0 <= stream < 2 ** 32 and 0 <= draw < 2 ** 64):
            raise ValueError("resample: seed and stream are 32-bit, draw is a 64-bit unsigned number")
        self._noise = (seed, stream, draw)
        self._pack()

    def denoise(self):
        """The next pack (the next forward of this copy) is the mean network again."""
        self._noise = None

    def _build_noisy(self, table, segs, offs, keep, dev):
        """Descriptor of the noisy pack and layout of the sigma gradients for the table just built (`segs`: parameter id ->
        table segment, `offs`: parameter id -> offset in the flat gradient)."""
        net = self.net
        rows = net.noisy_layout()
        if len(rows) > _lib.NOISY_MAX:
            raise ValueError("too many noisy layers")
        sig = net.noisy_sigma
        if sig.dtype != torch.float32 or not sig.is_contiguous() or sig.device != dev:
            raise ValueError("fused GCN kernels need noisy_sigma as a contiguous float32 parameter beside the others")
        nz, lay = _lib.NoisyDesc(), _lib.NoisyGradLayout()
        nz.n, lay.total = len(rows), self.layout.total
        eps = torch.zeros(sum(o + i for _, o, i, _, _ in rows), dtype=torch.float32, device=dev)
        keep.append(eps)
        self.eps, at = {}, 0
        for l, (name, o, i, off_w, off_b) in enumerate(rows):
            lin = getattr(net, name)
            nz.seg_w[l], nz.seg_b[l] = segs[id(lin.weight)], segs[id(lin.bias)]
            if (table.rows[nz.seg_w[l]], table.cols[nz.seg_w[l]]) != (o, i):
                raise ValueError(f"noisy layer {name}: its weight segment is not a transposed [{o}][{i}] one")
            nz.sigma_w[l], nz.sigma_b[l] = sig.data_ptr() + 4 * off_w, sig.data_ptr() + 4 * off_b
            e_in, e_out = eps[at:at + i], eps[at + i:at + i + o]
            at += i + o
            nz.eps_in[l], nz.eps_out[l] = e_in.data_ptr(), e_out.data_ptr()
            self.eps[name] = (e_in, e_out)
            lay.out[l], getattr(lay, "in")[l] = o, i             # (`in` is a keyword)
            lay.mu_w[l], lay.mu_b[l] = offs[id(lin.weight)], offs[id(lin.bias)]
            lay.sig_w[l], lay.sig_b[l] = offs[id(sig)] + off_w, offs[id(sig)] + off_b
        self.noisy_desc, self.noisy_layout = nz, lay

    def _build_table(self):
        """Packed parameter buffers ([in][out] layout), the kernel descriptor pointing at them, the table of the
        one-launch repack (mdq_gcn_pack) and the offsets of the parameters inside the flat gradient."""
        net = self.net
        levels, softmax = _levels_of(net)
        dueling = getattr(net, "head", None) == "dueling"
        dev = net.lin1.weight.device
        if dev.type != "cuda":
            raise _lib.MeshDQNHipError("fused GCN kernels need the module on a GPU (no CPU fallback)")
        keep, table, segs = [], GcnPackTable(), {}
        offs, pos = {}, 0
        for prm in net.parameters():
            offs[id(prm)] = pos
            pos += prm.numel()
        lay = GcnGradLayout()
        lay.total = pos

        def seg(prm, transpose=False):
            if prm.dtype != torch.float32 or not prm.is_contiguous():
                raise ValueError("fused GCN kernels need contiguous float32 parameters")
            buf = torch.empty(prm.numel(), dtype=torch.float32, device=dev)
            keep.append(buf)
            i = table.n
            if i >= PACK_MAX:
                raise ValueError("too many parameter segments")
            table.src[i], table.dst[i] = prm.data_ptr(), buf.data_ptr()
            if transpose:
                table.rows[i], table.cols[i] = prm.shape[0], prm.shape[1]
            else:
                table.rows[i], table.cols[i] = prm.numel(), 1
            table.n = i + 1
            segs[id(prm)] = i
            return buf.data_ptr()

        d = GcnNet()
        d.nlevels = len(levels)
        d.C = net.lin1.weight.shape[1] // 2
        d.out_dim = net.lin3.weight.shape[0]
        d.ratio = float(levels[0][1].ratio)
        d.softmax = 1 if softmax else 0
        d.dueling = 1 if dueling else 0
        for l in range(6):
            lay.w_l[l] = lay.b[l] = lay.w_r[l] = lay.pool_w[l] = -1
        for l, (conv, pool) in enumerate(levels):
            lv = d.levels[l]
            if hasattr(conv, "lin_l"):
                lv.type = 0
                lv.fin = conv.lin_l.weight.shape[1]
                lv.w_l = seg(conv.lin_l.weight, True)
                lv.b = seg(conv.lin_l.bias)
                lv.w_r = seg(conv.lin_r.weight, True)
                lay.w_l[l], lay.b[l], lay.w_r[l] = offs[id(conv.lin_l.weight)], offs[id(conv.lin_l.bias)], offs[id(conv.lin_r.weight)]
            else:
                lv.type = 1
                lv.fin = conv.lin.weight.shape[1]
                lv.w_l = seg(conv.lin.weight, True)
                lv.b = seg(conv.bias)
                lv.w_r = None
                lay.w_l[l], lay.b[l] = offs[id(conv.lin.weight)], offs[id(conv.bias)]
            lv.pool_w = seg(pool.weight)
            lay.pool_w[l] = offs[id(pool.weight)]
            if l > 0 and lv.fin != d.C:
                raise ValueError("inner levels must have conv_width inputs")
        d.fin0 = d.levels[0].fin
        d.lin1_w, d.lin1_b = seg(net.lin1.weight, True), seg(net.lin1.bias)
        d.lin2_w, d.lin2_b = seg(net.lin2.weight, True), seg(net.lin2.bias)
        d.lin3_w, d.lin3_b = seg(net.lin3.weight, True), seg(net.lin3.bias)
        lay.lin1_w, lay.lin1_b = offs[id(net.lin1.weight)], offs[id(net.lin1.bias)]
        lay.lin2_w, lay.lin2_b = offs[id(net.lin2.weight)], offs[id(net.lin2.bias)]
        lay.lin3_w, lay.lin3_b = offs[id(net.lin3.weight)], offs[id(net.lin3.bias)]
        if dueling:   # the value stream: two plain segments, one offset (the kernel finds the bias at lin_v + 64)
            if tuple(net.lin_v.weight.shape) != (1, 64) or net.lin_v.bias is None:
                raise ValueError("dueling head: lin_v must be Linear(64, 1) with a bias")
            # (a noisy layer's weight segment is a transposed one, rows = out; for this [1][64] weight the same 64 floats)
            d.lin_v_w, d.lin_v_b = seg(net.lin_v.weight, getattr(net, "noisy", None) is not None), seg(net.lin_v.bias)
            lay.lin_v = offs[id(net.lin_v.weight)]
            if offs[id(net.lin_v.bias)] != lay.lin_v + 64:
                raise ValueError("dueling head: lin_v.weight and lin_v.bias must be adjacent in parameters() order")
        if net.lin1.weight.shape[0] != 128 or net.lin2.weight.shape[0] != 64:
            raise ValueError("head must be 2C -> 128 -> 64 -> out (as in the reference)")
        self.desc, self._keep, self._table, self.layout = d, keep, table, lay
        self._train_bufs = {}
        if getattr(net, "noisy", None) is not None:
            self._build_noisy(table, segs, offs, keep, dev)

    def _pack(self, stream=None):
        """Bring the packed copy up to date: ONE launch (mdq_gcn_pack; mdq_gcn_pack_noisy for a copy that carries noise),
        and only after the parameters or the noise state (`resample` / `denoise`) changed."""
        net = self.net
        # (`_mdq_version`: bumped by whoever writes the parameters with a kernel of its own, e.g. mdq_adam_step)
        version = tuple(p._version for p in net.parameters()) + (id(net.conv1), getattr(net, "_mdq_version", 0), self._noise)
        if version == self._version:
            return
        key = tuple(p.data_ptr() for p in net.parameters())
        if key != self._table_key:
            self._build_table()
            self._table_key = key
        if self._noise is None:
            _lib.check(self.lib.mdq_gcn_pack(C.byref(self._table), _lib.stream_ptr(stream)), "mdq_gcn_pack")
        else:
            nz = self.noisy_desc
            nz.seed, nz.stream, nz.draw = self._noise
            _lib.check(self.lib.mdq_gcn_pack_noisy(C.byref(self._table), C.byref(nz), _lib.stream_ptr(stream)),
                       "mdq_gcn_pack_noisy")
        self._version = version

    def train_step(self, x, node_ptr, esrc, edst, edge_ptr, nmax, emax, mode, q_other, action, reward, nonfinal, gamma,
                   loss_out=None, want_out=False, stream=None, weight=None, td_out=None):
        """Forward + double-DQN Huber loss + backward of the module over a minibatch on the hand-written kernels
        (`mdq_gcn_train_step`, no autograd): returns (loss (1,) tensor, flat gradient over ALL parameters in
        `parameters()` order [, head outputs (B, out)]).  The returned tensors are persistent buffers that the next call
        overwrites.  For a copy that carries noise (`resample`) the sigmas' slice is filled by `mdq_noisy_grad`, one more
        launch behind the step; for the mean network it stays zero.  mode 0: this network evaluates the states, `q_other` the next states; mode 1 the other way
        round (the reference's `select` toggle, airfoil_dqn.py:240-310).  `loss_out`: a (1,) float32 device tensor to
        receive the loss instead of the internal one (e.g. a slot of a log ring: no copy, no synchronisation).
        `weight` / `td_out` ((B,) float32 device tensors, either may be None: `mdq_gcn_train_step_weighted`): importance
        weight of every graph's loss term (prioritized replay) / receives every graph's TD error."""
        self._pack(stream)
        d = self.desc
        dev = x.device
        B = node_ptr.numel() - 1
        key = (B, int(nmax), int(emax))
        bufs = self._train_bufs.get(key)
        if bufs is None:
            ws = int(self.lib.mdq_gcn_train_workspace(C.byref(d), int(nmax), max(int(emax), 1)))
            if ws <= 0:
                raise _lib.MeshDQNHipError("mdq_gcn_train_workspace failed")
            bufs = dict(ws=torch.zeros((B, ws), dtype=torch.float32, device=dev),
                        partial=torch.zeros((B, self.layout.total), dtype=torch.float32, device=dev),
                        grad=torch.zeros(self.layout.total, dtype=torch.float32, device=dev),
                        loss=torch.zeros(1, dtype=torch.float32, device=dev),
                        out=torch.zeros((B, d.out_dim), dtype=torch.float32, device=dev))
            self._train_bufs = {key: bufs}
        x = x.reshape(-1, x.shape[-1])
        for t, dt in ((x, torch.float32), (q_other, torch.float32), (reward, torch.float32), (nonfinal, torch.float32),
                      (action, torch.int64), (node_ptr, torch.int32), (edge_ptr, torch.int32), (esrc, torch.int32),
                      (edst, torch.int32)):
            if t.dtype != dt or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"train_step wants contiguous {dt} tensors on {dev}")
        if q_other.shape != (B, d.out_dim) or action.numel() != B or reward.numel() != B or nonfinal.numel() != B:
            raise ValueError("train_step: minibatch arrays of different lengths")
        if x.shape[0] > B * int(nmax):
            raise ValueError(f"{x.shape[0]} nodes in {B} graphs exceed nmax {int(nmax)}")
        for t in (weight, td_out):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or t.numel() != B):
                raise ValueError(f"train_step wants weight / td_out as contiguous float32 tensors of {B} entries on {dev}")
        loss = bufs["loss"] if loss_out is None else loss_out
        t = GcnTrainDesc()
        t.B, t.NMAX, t.EMAX, t.mode, t.gamma = B, int(nmax), max(int(emax), 1), int(mode), float(gamma)
        t.x, t.node_ptr, t.esrc, t.edst, t.edge_ptr = x.data_ptr(), node_ptr.data_ptr(), esrc.data_ptr(), edst.data_ptr(), edge_ptr.data_ptr()
        t.q_other, t.action, t.reward, t.nonfinal = q_other.data_ptr(), action.data_ptr(), reward.data_ptr(), nonfinal.data_ptr()
        t.workspace, t.partial, t.grad, t.loss = bufs["ws"].data_ptr(), bufs["partial"].data_ptr(), bufs["grad"].data_ptr(), loss.data_ptr()
        t.out = bufs["out"].data_ptr() if want_out else None
        t.layout = self.layout
        if weight is None and td_out is None:
            _lib.check(self.lib.mdq_gcn_train_step(C.byref(d), C.byref(t), _lib.stream_ptr(stream)), "mdq_gcn_train_step")
        else:
            _lib.check(self.lib.mdq_gcn_train_step_weighted(
                C.byref(d), C.byref(t), None if weight is None else weight.data_ptr(),
                None if td_out is None else td_out.data_ptr(), _lib.stream_ptr(stream)), "mdq_gcn_train_step_weighted")
        if self._noise is not None:
            # the sigmas' slice (which the learning step leaves at zero) from the means' gradients and the eps of THIS copy's pack
            _lib.check(self.lib.mdq_noisy_grad(C.byref(self.noisy_desc), C.byref(self.noisy_layout), bufs["grad"].data_ptr(),
                                               _lib.stream_ptr(stream)), "mdq_noisy_grad")
        return (loss, bufs["grad"]) + ((bufs["out"],) if want_out else ())

    @torch.no_grad()
    def forward(self, data, return_embedding=False, stream=None):
        """`data`: Data / Batch with x (N,F), edge_index (2,E) global node ids, batch (N,) or None."""
        self._pack(stream)
        d = self.desc
        dev = self.net.lin1.weight.device
        x = data.x.to(dev, torch.float32)
        from .airfoilgcnn import AirfoilGCNN
        if isinstance(self.net, AirfoilGCNN):
            x = x[:, [2, 3]]
        x = x.contiguous()
        n = x.shape[0]
        batch = data.batch if getattr(data, "batch", None) is not None else torch.zeros(n, dtype=torch.long, device=dev)
        batch = batch.to(dev)
        B = int(batch.max().item()) + 1
        counts = torch.bincount(batch, minlength=B)
        node_ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        node_ptr[1:] = torch.cumsum(counts, 0)
        ei = data.edge_index.to(dev).reshape(2, -1)
        eg = batch[ei[0]] if ei.numel() else torch.zeros(0, dtype=torch.long, device=dev)
        order = torch.argsort(eg, stable=True)
        ei, eg = ei[:, order], eg[order]
        ecounts = torch.bincount(eg, minlength=B)
        edge_ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        edge_ptr[1:] = torch.cumsum(ecounts, 0)
        esrc = (ei[0] - node_ptr[eg]).to(torch.int32).contiguous()
        edst = (ei[1] - node_ptr[eg]).to(torch.int32).contiguous()
        NMAX = int(counts.max().item())
        EMAX = max(int(ecounts.max().item()) if ecounts.numel() else 0, 1)
        node_ptr32, edge_ptr32 = node_ptr.to(torch.int32), edge_ptr.to(torch.int32)
        emb = torch.empty((B, 2 * d.C), dtype=torch.float32, device=dev)
        out = torch.empty((B, d.out_dim), dtype=torch.float32, device=dev)
        rc = self.lib.mdq_gcn_forward(C.byref(d), B, NMAX, EMAX, x.data_ptr(), node_ptr32.data_ptr(),
                                      esrc.data_ptr(), edst.data_ptr(), edge_ptr32.data_ptr(), emb.data_ptr(),
                                      out.data_ptr(), _lib.stream_ptr(stream))
        _lib.check(rc, "mdq_gcn_forward")
        return (out, emb) if return_embedding else out


    @torch.no_grad()
    def forward_arrays(self, x, node_ptr, esrc, edst, edge_ptr, nmax, emax, stream=None, edge_counts=None,
                       return_perm=False, return_status=False, pack=True, edge_cnt=None, return_embedding=False):
        """Same launch on pre-built arrays (what `VecEnv2DAirfoil.get_state` returns): x (sumN,F) f32,
        node_ptr / edge_ptr (B+1,) i32, esrc / edst (sumE,) i32 local node ids.  `nmax` / `emax` size the kernel's LDS
        carve-up: `edge_counts` (host array of the per-graph edge counts, where the caller has them) is checked against
        `emax` before the launch, and the kernel itself refuses larger graphs (NaN outputs, `return_status`).
        `return_perm`: also the (B, levels, nmax) TopKPooling `perm` arrays.  `pack=False`: use the packed parameter copy
        as it is (the caller has called `_pack()` at a point ordered against the writers of the parameters).  `edge_cnt`
        ((B,) i32 device tensor): the edge lists are PADDED - esrc / edst are (B, emax) arrays, graph b owns the first
        edge_cnt[b] slots of its row (what `mdq_env_topology` writes) - and `edge_ptr` is ignored.  `return_embedding`: also
        the (B, 2C) graph embeddings the head read, last in the returned tuple."""
        if pack:
            self._pack(stream)
        elif self.desc is None:
            raise _lib.MeshDQNHipError("forward_arrays(pack=False) before the first _pack()")
        d = self.desc
        B = node_ptr.numel() - 1
        if edge_counts is not None and len(edge_counts) and int(max(edge_counts)) > int(emax):
            raise ValueError(f"graph with {int(max(edge_counts))} edges exceeds emax {int(emax)}")
        x = x.reshape(-1, x.shape[-1]).to(torch.float32).contiguous()
        if x.shape[0] > B * int(nmax):
            raise ValueError(f"{x.shape[0]} nodes in {B} graphs exceed nmax {int(nmax)}")
        emb = torch.empty((B, 2 * d.C), dtype=torch.float32, device=x.device)
        out = torch.empty((B, d.out_dim), dtype=torch.float32, device=x.device)
        perm = torch.full((B, d.nlevels, int(nmax)), -1, dtype=torch.int32, device=x.device) if return_perm else None
        status = torch.zeros(B, dtype=torch.int32, device=x.device) if return_status else None
        if edge_cnt is not None:
            if esrc.shape[-1] != int(emax) or esrc.numel() != B * int(emax) or edge_cnt.numel() != B:
                raise ValueError("padded edge lists must be (B, emax) with (B,) counts")
            rc = self.lib.mdq_gcn_forward_padded(C.byref(d), B, int(nmax), int(emax), x.data_ptr(), node_ptr.data_ptr(),
                                                 esrc.data_ptr(), edst.data_ptr(), edge_cnt.data_ptr(), emb.data_ptr(),
                                                 out.data_ptr(), None if perm is None else perm.data_ptr(),
                                                 None if status is None else status.data_ptr(), _lib.stream_ptr(stream))
            _lib.check(rc, "mdq_gcn_forward_padded")
        else:
            rc = self.lib.mdq_gcn_forward_ex(C.byref(d), B, int(nmax), max(int(emax), 1), x.data_ptr(), node_ptr.data_ptr(),
                                             esrc.data_ptr(), edst.data_ptr(), edge_ptr.data_ptr(), emb.data_ptr(),
                                             out.data_ptr(), None if perm is None else perm.data_ptr(),
                                             None if status is None else status.data_ptr(), _lib.stream_ptr(stream))
            _lib.check(rc, "mdq_gcn_forward_ex")
        if return_perm or return_status or return_embedding:
            return (out,) + ((perm,) if return_perm else ()) + ((status,) if return_status else ()) + ((emb,) if return_embedding else ())
        return out


def fused_of(net, role: str = "act") -> FusedGcn:
    """The packed device copy of `net` for `role`, created on first use and kept on the module: "act" (`net._fused`,
    the inference forwards) or "train" (`net._fused_train`, see `DQNTrainer._fused_of`)."""
    attr = "_fused" if role == "act" else "_fused_train"
    if not hasattr(net, attr):
        setattr(net, attr, FusedGcn(net))
    return getattr(net, attr)


def node_removal_forward(net, data):
    return fused_of(net).forward(data)
