"""Batched IPCS solver: B environments (meshes) advanced together on one MI355X.

Host side of `mdq_ipcs_assemble` / `mdq_ipcs_evolve` / `mdq_probe_forces`
(include/meshdqn_hip.h).  Builds the padded index arrays from `MeshTopology`,
owns the device tensors (torch = allocator + stream plumbing only) and hands
raw device pointers to the C ABI.  No CPU fallback.
"""
from __future__ import annotations

import os
import ctypes as C
from typing import Sequence

import numpy as np
import torch

from . import _lib
from .inflow import batch_profiles, batch_specs, inflow_factors, inlet_tables, padded, profile_values, step_times
from .topology import conflict_free_cell_order, morton_cell_order, TAG_AIRFOIL, TAG_OUTFLOW, MeshTopology


def smooth_coords(topo: MeshTopology, iterations: int = 50, coords: np.ndarray | None = None) -> np.ndarray:
    """DOLFIN `Mesh.smooth(iterations)` (`flow_solver.py:65-67,236-237`) via the
    library's host routine; returns the new coordinates (topology unchanged)."""
    lib = _lib.load()
    x = np.array(topo.coords if coords is None else coords, dtype=np.float64, order="C", copy=True)
    nbr_ptr, nbr, vc_ptr, vc = topo.vertex_adjacency()
    cells = np.ascontiguousarray(topo.cells, dtype=np.int32)
    onb = np.ascontiguousarray(topo.on_boundary, dtype=np.uint8)
    nbr_ptr = np.ascontiguousarray(nbr_ptr, np.int64)
    nbr = np.ascontiguousarray(nbr, np.int64)
    vc_ptr = np.ascontiguousarray(vc_ptr, np.int64)
    vc = np.ascontiguousarray(vc, np.int64)
    rc = lib.mdq_smooth_host(x.ctypes.data, topo.nv, cells.ctypes.data, topo.nt, nbr_ptr.ctypes.data,
                             nbr.ctypes.data, vc_ptr.ctypes.data, vc.ctypes.data, onb.ctypes.data, int(iterations))
    _lib.check(rc, "mdq_smooth_host")
    return x


def pd_device_tables(d, B: int, NV: int, device, cap: dict, tables: dict | None = None) -> dict:
    """The pd_* tables `mdq_ipcs_factorize_pressure` fills, for B environments of NV vertices at the capacities `cap`
    (`IpcsBatch.PD_DEVICE_CAP`): allocated unless `tables` are given, their pointers and the six capacities set on the
    descriptor `d`.  Returns the tables."""
    if tables is None:
        i32, f64 = torch.int32, torch.float64
        z = lambda n, dt: torch.zeros((B, n), dtype=dt, device=device)   # noqa: E731
        tables = dict(pd_hdr=z(4, i32), pd_node=z(NV, i32), pd_meta=z(cap["NPART"] * 6, i32), pd_rowblk=z(NV, i32),
                      pd_W=z(cap["NPW"], f64), pd_F=z(cap["NPF"], f64), pd_gidx=z(cap["NPGI"], i32),
                      pd_Sinv=z(cap["NPS"], f64), pd_gk_ptr=z(NV + 1, i32), pd_gk_col=z(cap["NPGK"], i32),
                      pd_gk_val=z(cap["NPGK"], f64))
    for k, a in tables.items():
        setattr(d, k, a.data_ptr())
    d.NPART, d.NPW, d.NPF, d.NPGI, d.NPS, d.NPGK = (cap[k] for k in ("NPART", "NPW", "NPF", "NPGI", "NPS", "NPGK"))
    return tables


def flow_table(mu, rho, dt, B: int) -> np.ndarray | None:
    """The per-environment flow constants of a batch of B environments (`mdq_ipcs_desc.env_phys`): None when mu, rho and
    dt are all scalars (the descriptor's scalars then hold for the whole batch), else a float64 (B, 4) array whose row b
    is mu, rho, dt, 0 of environment b - scalars broadcast, sequences of length B.  The library cannot read a device
    table, so this is where it is validated: a wrong length or a value that is not finite and > 0 raises ValueError
    naming the argument."""
    args = dict(mu=mu, rho=rho, dt=dt)
    table = np.zeros((int(B), 4), np.float64)
    per_env = False
    for k, (name, val) in enumerate(args.items()):
        a = np.asarray(val.detach().cpu().numpy() if isinstance(val, torch.Tensor) else val, dtype=np.float64)
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != B):
            raise ValueError(f"{name} must be a scalar or a sequence of length {B} (one value per environment), got shape {a.shape}")
        if not (np.isfinite(a).all() and (a > 0).all()):
            raise ValueError(f"{name} must be finite and > 0, got {val!r}")
        per_env = per_env or a.ndim == 1
        table[:, k] = a
    return table if per_env else None


# ---- the LDS plan of the IPCS kernels and the entry point's mode conditions, mirrored (csrc/mdq_ipcs_step.hip `lds_plan`,
# csrc/mdq_ipcs_entry.hip `ipcs_evolve_impl`): the ONE place the Python side takes the operator modes' size limits from
LDS_MAX, RED_BYTES = 160 * 1024, 64 * 8     # dynamic LDS of a workgroup; the reduction scratch in front of every layout
WG, MF_ROWS, MF_CH = 512, 7, 1024           # threads of the one-kernel modes, own rows per thread (modes 2 / 3), triangles per tile


def lds_plan(N2: int, NV: int, NSE1: int = 0) -> dict:
    """`lds_plan` of the kernels: padded lengths and the bytes of every layout behind the reduction scratch."""
    N2p = (int(N2) + 1) & ~1
    NVp = (max(int(NV), 1024) + 63) & ~63        # (>= the 1024 threads of the direct pressure kernel)
    NSE1 = int(NSE1)
    return dict(N2p=N2p, NVp=NVp, vel1_bytes=2 * 16 * N2p, vel2_bytes=16 * (N2p + 6 * MF_CH), vel3_bytes=3 * 16 * N2p,
                prs_vec_bytes=5 * 8 * NVp,
                prs_mat_bytes=8 * max(NSE1, WG) + 4 * (NSE1 + (NSE1 & 1)) + 4 * (((int(NV) // 64 + 2) + 1) & ~1))


def operator_mode_limits(N2: int, NV: int = 0, NSE1: int = 0) -> dict:
    """What the entry point decides from the capacities N2 (P2 rows), NV (vertices) and NSE1 (SELL entries of the P1
    Laplacian) alone, for a descriptor that carries every array:
      mode1 / mode2 / mode3   the LDS-resident mode is accepted (vectors in LDS; modes 2 / 3 also N2 <= MF_ROWS * WG = 3 584;
                              three vectors of mode 3 fit up to N2 = 3 402, the stage + tile of mode 2 up to 3 584, the two
                              vectors of mode 1 up to 5 104)
      auto, auto_repro        what modes -1 / -2 choose among them; 0 = beyond them (the element tiles 5 / 7 when the tile maps
                              or slot lists are given, else the assembled operators 0 / 4)
      per_step                that choice launches once per step (modes 2 / 3: what an inflow profile needs)
      pressure_global         the pressure CG vectors do not fit the LDS (modes 0 / 5 only)
      k1_lds                  the P1 Laplacian fits the LDS beside them (Krylov pressure solve)."""
    P = lds_plan(N2, NV, NSE1)
    rows_ok = int(N2) <= MF_ROWS * WG
    m1 = RED_BYTES + P["vel1_bytes"] <= LDS_MAX
    m2 = RED_BYTES + P["vel2_bytes"] <= LDS_MAX and rows_ok
    m3 = RED_BYTES + P["vel3_bytes"] <= LDS_MAX and rows_ok
    repro = 2 if m2 else (1 if m1 else 0)
    auto = 3 if m3 else repro
    pg = RED_BYTES + P["prs_vec_bytes"] > LDS_MAX
    return dict(mode1=m1, mode2=m2, mode3=m3, auto=auto, auto_repro=repro, per_step=auto in (2, 3), pressure_global=pg,
                k1_lds=(not pg) and RED_BYTES + P["prs_vec_bytes"] + P["prs_mat_bytes"] <= LDS_MAX, **P)


MODE3_MAX_N2 = max(n for n in range(MF_ROWS * WG + 1) if operator_mode_limits(n)["mode3"])      # 3 402


class IpcsBatch:
    """Device-resident batch of Taylor-Hood IPCS problems.  `mu`, `rho` and `dt` are scalars (one flow condition for the
    batch) or sequences of length B (one per environment: `self.env_phys`, see `flow_table`).  `inflow`: None (the constant
    parabola), one inflow schedule (inflow.py: a spec or its dict) or a sequence of B of them - `evolve` then scales every
    environment's inlet values by its own factor a_b(t), step by step, inside the kernels.  `inflow_profile`: None, one
    callable profile(x, y, t) -> x-velocity at the inlet dofs (any non-separable profile) or a sequence of B callables / None -
    `evolve` then evaluates every step of a call on the host up front and a small kernel rewrites the inlet values and the
    lifting vectors between the steps (operator modes 2 and 3).  A batch has one kind of time-dependent inflow."""

    def __init__(self, topos: Sequence[MeshTopology], coords: Sequence[np.ndarray] | None = None,
                 mu=1e-3, rho=1.0, dt=1e-3, rtol: float = 1e-10,
                 maxit=(200, 4000, 200), device: str | torch.device = "cuda", capacities: dict | None = None,
                 mode: int = -1, pressure_direct: bool = True, pressure_parts: int = 16,
                 cell_order: str = "auto", pcg_degree: int = 0, inflow=None, inflow_profile=None):
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.MeshDQNHipError("IpcsBatch needs a GPU device (no CPU fallback)")
        self.topos = list(topos)
        B = len(self.topos)
        if B == 0:
            raise ValueError("empty batch")
        table = flow_table(mu, rho, dt, B)      # (validated before any device work)
        self.inflow = batch_specs(inflow, B)    # (likewise) B specs, or None
        self.inflow_profile = batch_profiles(inflow_profile, B)     # (likewise) B callables / None, or None
        if self.inflow is not None and self.inflow_profile is not None:
            raise ValueError("inflow_profile cannot be combined with inflow schedules (inflow=): a batch has one kind of "
                             "time-dependent inflow")
        if cell_order == "auto":
            # every mesh of the batch within the LDS-atomic mode 3 (`operator_mode_limits`: 3 402 velocity dofs): its
            # conflict-free order; beyond it (tiles of 1 024 triangles: mode 2, the element tiles 5 / 7): a spatial order, so that
            # a chunk of 1 024 triangles shares its rows (2 200 touched rows per chunk on the red-refined ys930 instead of 5 100:
            # the chunk's input rows fit the kernels' LDS stage, and a row meets 1.06 chunks instead of 2.4)
            cell_order = "conflictfree" if operator_mode_limits(max(t.np2 for t in self.topos))["mode3"] else "morton"
        if cell_order == "morton":
            cache = {}
            for t in self.topos:
                if id(t) not in cache:
                    cache[id(t)] = t.permuted(morton_cell_order(t.coords, t.cells))
            self.topos = [cache[id(t)] for t in self.topos]
        elif cell_order == "conflictfree":
            # internal cell order: the 64 cells a wave handles in one instruction share no dof, so the LDS atomics of
            # the matrix-free kernels never collide inside an instruction (dof numbering and all vectors unchanged)
            cache = {}
            for t in self.topos:
                if id(t) not in cache:
                    cache[id(t)] = t.permuted(conflict_free_cell_order(t.cells))
            self.topos = [cache[id(t)] for t in self.topos]
        elif cell_order != "mesh":
            raise ValueError("cell_order must be 'auto', 'conflictfree', 'morton' or 'mesh'")
        coords = [t.coords for t in self.topos] if coords is None else list(coords)
        self.B = B
        # the scalars stay what existing callers read (row 0 of a table: what the entry points validate)
        self.mu, self.rho, self.dt = (float(v) for v in (table[0, :3] if table is not None else (mu, rho, dt)))
        self.rtol = float(rtol)
        self.maxit = tuple(int(m) for m in maxit)

        per = [self._host_arrays(t, x) for t, x in zip(self.topos, coords)]
        self._prof_tab = self._prof_dev = self._prof_desc = None     # inflow profiles: host tables, device tables, mdq_inflow_profile
        if self.inflow_profile is not None:
            # the kernel that rewrites the lifts between the steps does not re-apply the outflow correction (- mu/2 B g on the
            # outflow rows): a mesh whose inlet-adjacent rows meet its outflow rows is refused
            self._prof_tab = inlet_tables(self.topos, coords)
            for b, (tab, p) in enumerate(zip(self._prof_tab, per)):
                both = np.intersect1d(tab["rows"], p["bo_rows"])
                if both.size:
                    raise ValueError(f"inflow_profile: environment {b} has {both.size} row(s) that are inlet-adjacent and outflow rows "
                                     f"(e.g. dof {int(both[0])}): the inflow kernel does not re-apply the outflow correction of the lifts")
        cap = dict(NV=max(p["nv"] for p in per), NT=max(p["nt"] for p in per), NE=max(p["ne"] for p in per),
                   NNZ2=max(p["colidx2"].size for p in per), NNZ1=max(p["colidx1"].size for p in per),
                   NAF=max(max(p["af"].shape[0] for p in per), 1),
                   NSE2=max(p["sl2_col"].size for p in per), NSE1=max(p["sl1_col"].size for p in per),
                   NBO=max(max(p["bo_rows"].size for p in per), 1), NBE=max(max(p["bo_col"].size for p in per), 1))
        if capacities:
            for k, val in capacities.items():
                if val < cap[k]:
                    raise ValueError(f"capacity {k}={val} smaller than required {cap[k]}")
                cap[k] = int(val)
        self.cap = cap
        NV, NT, NE, NNZ2, NNZ1, NAF = (cap[k] for k in ("NV", "NT", "NE", "NNZ2", "NNZ1", "NAF"))
        NSE2, NSE1 = cap["NSE2"], cap["NSE1"]
        NBO, NBE = cap["NBO"], cap["NBE"]
        N2 = NV + NE
        self.N2 = N2

        def stack(key, shape, dtype, fill=0):
            out = np.full((B,) + shape, fill, dtype=dtype)
            for b, p in enumerate(per):
                a = p[key]
                out[(b,) + tuple(slice(0, s) for s in a.shape)] = a
            return out

        h = {}
        h["nv"] = np.array([p["nv"] for p in per], np.int32)
        h["nt"] = np.array([p["nt"] for p in per], np.int32)
        h["ne"] = np.array([p["ne"] for p in per], np.int32)
        h["naf"] = np.array([p["af"].shape[0] for p in per], np.int32)
        h["coords"] = stack("coords", (NV, 2), np.float64)
        h["cell_dofs"] = stack("cell_dofs_soa", (6, NT), np.int32)
        h["cell_outflow"] = stack("cell_outflow", (NT,), np.int8, fill=-1)
        h["rowptr2"] = stack("rowptr2", (N2 + 1,), np.int32)
        h["colidx2"] = stack("colidx2", (NNZ2,), np.int32)
        h["asm2_ptr"] = stack("asm2_ptr", (NNZ2 + 1,), np.int32)
        h["asm2_src"] = stack("asm2_src", (36 * NT,), np.int32)
        h["rowptr1"] = stack("rowptr1", (NV + 1,), np.int32)
        h["colidx1"] = stack("colidx1", (NNZ1,), np.int32)
        h["asm1_ptr"] = stack("asm1_ptr", (NNZ1 + 1,), np.int32)
        h["asm1_src"] = stack("asm1_src", (9 * NT,), np.int32)
        h["sl2_off"] = stack("sl2_off", (N2 // 64 + 2,), np.int32)
        h["sl2_col"] = stack("sl2_col", (NSE2,), np.int32)
        h["sl1_off"] = stack("sl1_off", (NV // 64 + 2,), np.int32)
        h["sl1_col"] = stack("sl1_col", (NSE1,), np.int32)
        NCH = (NT + 1023) // 1024
        self._NRL = self._rl_flags = 0      # row lists of the element-tile modes: capacity, first / last-touch bits in the row words
        if N2 > 4096:
            # capacity beyond the packed words (dof ids of 12 bits): the kernels read plain tile positions for EVERY mesh of
            # the batch (mode 5: element tiles with global vectors), also for the ones that would fit the packed form
            for t_, p_ in zip(self.topos, per):
                if t_.np2 <= 4096:
                    p_["mf_scat"], p_["mf_tptr"] = t_.matfree_maps(1024)
            # per chunk the rows its triangles touch (mode 5's row phase: ~2 500 of the refined mesh's 12 924 rows per chunk)
            for p_ in per:
                tp = p_["mf_tptr"]
                cnt = np.diff(tp, axis=1)
                p_["mf_rcnt"] = (cnt > 0).sum(axis=1).astype(np.int32)
            NRL = int(max(p_["mf_rcnt"].max() for p_ in per))
            # bit 31 / 30 of the row word: this chunk is the FIRST / LAST one that touches the row - the row phase starts the
            # row's sum at 0 instead of reading a zero-filled accumulation vector (the last-touch bit is used by an experiment
            # build only, see tile_apply_global); valid when every row of every mesh is touched by some chunk (every dof
            # belongs to a cell)
            flags_ok = os.environ.get("MDQ_NO_RL_FLAGS", "") != "1"      # (A / B switch: plain row words, rl_flags = 0)
            for t_, p_ in zip(self.topos, per):
                flags_ok = flags_ok and bool((np.diff(p_["mf_tptr"], axis=1) > 0)[:, :t_.np2].any(axis=0).all())
            for p_ in per:
                tp = p_["mf_tptr"]
                cnt = np.diff(tp, axis=1)
                touched = cnt > 0
                first = touched & (np.cumsum(touched, axis=0) == 1)
                last = touched & (np.cumsum(touched[::-1], axis=0)[::-1] == 1)
                rl = np.zeros((tp.shape[0], NRL, 2), np.int32)
                for c in range(tp.shape[0]):
                    rows = np.flatnonzero(touched[c])
                    word = rows.astype(np.uint32)
                    if flags_ok:
                        word = word | (first[c, rows].astype(np.uint32) << 31) | (last[c, rows].astype(np.uint32) << 30)
                    rl[c, :rows.size, 0] = word.view(np.int32)
                    rl[c, :rows.size, 1] = tp[c, rows] | (cnt[c, rows] << 16)
                p_["mf_rlist"] = rl
                # packed local maps (round 5): position of every dof of a triangle in its chunk's row list | tile position << 16 -
                # the kernel stages the chunk's input rows in LDS through the row list and gathers from there
                # (MDQ_NO_LPOS=1: the per-triangle gathers from global memory of round 4, A / B switch)
                if NRL <= 0xFFFF and os.environ.get("MDQ_NO_LPOS", "") != "1":
                    cdofs = p_["cell_dofs_soa"]                       # (6, nt)
                    scat = p_["mf_scat"]
                    lpos = np.zeros_like(scat)
                    for c in range(tp.shape[0]):
                        lo_, hi_ = c * 1024, min((c + 1) * 1024, cdofs.shape[1])
                        rows = np.flatnonzero(touched[c])
                        loc = np.searchsorted(rows, cdofs[:, lo_:hi_])
                        assert (rows[loc] == cdofs[:, lo_:hi_]).all() and scat[:, lo_:hi_].max(initial=0) < 0x8000
                        lpos[:, lo_:hi_] = loc | (scat[:, lo_:hi_] << 16)
                    p_["mf_lpos"] = lpos.astype(np.int32)
            self._rl_flags = 1 if flags_ok else 0
            h["mf_rlist"] = stack("mf_rlist", (NCH, NRL, 2), np.int32)
            h["mf_rcnt"] = stack("mf_rcnt", (NCH,), np.int32)
            if all("mf_lpos" in p_ for p_ in per):
                h["mf_lpos"] = stack("mf_lpos", (6, NT), np.int32)
            self._NRL = NRL
        h["mf_scat"] = stack("mf_scat", (6, NT), np.int32)
        h["mf_tptr"] = stack("mf_tptr", (NCH, N2 + 1), np.int32)
        h["nbo"] = np.array([p["bo_rows"].size for p in per], np.int32)
        h["bo_rows"] = stack("bo_rows", (NBO,), np.int32)
        h["bo_ptr"] = stack("bo_ptr", (NBO + 1,), np.int32)
        h["bo_col"] = stack("bo_col", (NBE,), np.int32)
        h["bo_src"] = stack("bo_src", (NBE,), np.int32)
        h["g2_ptr"] = stack("g2_ptr", (N2 + 1,), np.int32)
        h["g2_src"] = stack("g2_src", (6 * NT,), np.int32)
        h["g1_ptr"] = stack("g1_ptr", (NV + 1,), np.int32)
        h["g1_src"] = stack("g1_src", (3 * NT,), np.int32)
        h["bcu_flag"] = stack("bcu_flag", (N2,), np.uint8)
        h["bcu_gx"] = stack("bcu_gx", (N2,), np.float64)
        h["bcp_flag"] = stack("bcp_flag", (NV,), np.uint8)
        h["af_facets"] = stack("af", (NAF, 2), np.int32)
        self.host = h
        self.per = per
        dev = self.device
        self.t = {k: torch.from_numpy(v).to(dev) for k, v in h.items()}

        def z(*shape):
            return torch.zeros(shape, dtype=torch.float64, device=dev)

        t = self.t
        t["geom"] = z(B, 5, NT)
        t["A1"] = z(B, NSE2, 4)
        t["Ms"] = z(B, NSE2)
        t["K1s"] = z(B, NSE1)
        t["lift1"] = z(B, N2, 2)
        t["lift3"] = z(B, N2, 2)
        t["idiag1"] = z(B, N2, 2)
        t["sdiagM"] = z(B, N2)
        t["sdiagK"] = z(B, NV)
        t["bo_val"] = z(B, NBE, 4)
        t["u_n"] = z(B, N2, 2)
        t["p_n"] = z(B, NV)
        nwork = int(self.lib.mdq_ipcs_workspace_doubles(B, NV, NT, NE))
        t["work"] = z(nwork)
        self.iters = torch.zeros((B, 3), dtype=torch.int32, device=dev)
        self.status = torch.zeros(B, dtype=torch.int32, device=dev)       # sticky (mdq_ipcs_desc.status, ABI 7): see `check`
        self.env_phys = None if table is None else torch.from_numpy(table).to(dev)    # (B, 4) mu, rho, dt, 0 per environment
        self.env_phys_host = table      # (the schedules' clocks run on every environment's own dt)
        self._inflow_keep = None
        self.steps_done = 0
        if self._prof_tab is not None:
            n_in, dofs = padded(self._prof_tab, "dofs")
            n_rw, rows = padded(self._prof_tab, "rows")
            assert dofs.max() < N2 and rows.max() < N2
            self._prof_dev = {k: torch.from_numpy(v).to(dev) for k, v in dict(n_inlet=n_in, inlet_dofs=dofs, n_rows=n_rw, rows=rows).items()}
            pd_ = _lib.InflowProfile()
            pd_.NIN, pd_.NIR = dofs.shape[1], rows.shape[1]
            for k, a in self._prof_dev.items():
                setattr(pd_, k, a.data_ptr())
            self._prof_desc = pd_

        d = _lib.IpcsDesc()
        d.B, d.NV, d.NT, d.NE, d.N2, d.NNZ2, d.NNZ1, d.NAF = B, NV, NT, NE, N2, NNZ2, NNZ1, NAF
        d.NSE2, d.NSE1 = NSE2, NSE1
        d.NBO, d.NBE = NBO, NBE
        d.mu, d.rho, d.dt, d.rtol = self.mu, self.rho, self.dt, self.rtol
        d.maxit_u, d.maxit_p, d.maxit_m = self.maxit
        d.mode = int(mode)
        for name, _typ in _lib.IpcsDesc._fields_:
            if name in t:
                setattr(d, name, t[name].data_ptr())
        if os.environ.get("MDQ_NO_TILE_MAPS", "") == "1":     # (A / B: modes 5 / 7 through the dof <- slot lists, as on device-built index data)
            d.mf_tptr = d.mf_scat = d.mf_rlist = d.mf_rcnt = d.mf_lpos = None
        d.work_doubles = nwork
        d.status = self.status.data_ptr()
        d.env_phys = None if self.env_phys is None else self.env_phys.data_ptr()
        d.NRL, d.rl_flags = self._NRL, self._rl_flags
        d.pd_enabled = 0
        # Krylov pressure solve of mode 3: degree of the Chebyshev polynomial preconditioner (0, default: the plain Jacobi-CG
        # kernel).  Measured on ys930 (tools/time_pcg.py): iterations 154 -> 95 / 67 / 52 / 37 / 30 for degree 2 / 3 / 4 / 6 / 8,
        # kernel time unchanged (251-283 us against 253 us): the solve is bound by the LDS gathers of the operator
        # application (~1.6 us each, bank conflicts of the random vertex gather), not by its reductions, and the polynomial
        # trades the one for the other.  pcg_degree < 0: two-level additive preconditioner (8 x 7 geometric aggregates, coarse
        # matrix inverted in LDS): 154 -> 86 iterations, but 465 us per solve in its first version (aggregation + inversion
        # ~0.1 ms, two more barriers and a coarse product per iteration).  Both kept as options (the reference's Krylov option
        # is CG + AMG, flow_solver.py:152-155); the default is the Jacobi-CG.  Meshes beyond mode 3 (pressure vectors in LDS,
        # modes 0 / 4 / 5 / 7): 0 = auto, the two-level preconditioner with an O(n) aggregation from 2048 vertices on
        # (cg_pressure_2l_lds: 325 -> 158 iterations on the refined ys930), > 0 = Jacobi-CG, < 0 = two-level wherever it fits.
        d.pcg_degree = int(pcg_degree)
        self.desc = d
        self.assembled = False
        # True: substructuring factors built on the host (numpy, pressure_direct.py); "device": built by
        # mdq_ipcs_factorize_pressure (one workgroup per environment, no host work); False: Jacobi-CG
        self.pressure_direct = "device" if pressure_direct == "device" else bool(pressure_direct)
        self.pressure_parts = int(pressure_parts)
        self._pd_cache = {}
        self.pds = self.pd_cap = None               # host factors and their capacities (`_factorize_pressure`)
        self._pd_dev = self.pd_status = None        # device-built factors and their status words (`factorize_pressure_device`)
        self._inlet = self._gx_host = None          # inlet dofs + host copy of the Dirichlet values (`update_inflow`)

    # ------------------------------------------------------------------
    @staticmethod
    def _host_arrays(topo: MeshTopology, coords: np.ndarray) -> dict:
        bc = topo.boundary_conditions(coords)
        pat = topo.patterns()
        gat = topo.dof_gathers()
        rowptr2, colidx2, asm2_ptr, asm2_src = pat["p2"]
        rowptr1, colidx1, asm1_ptr, asm1_src = pat["p1"]
        out_f, _ = topo.facets(bc["tags"], TAG_OUTFLOW)
        af, af_edges = topo.facets(bc["tags"], TAG_AIRFOIL)
        sl2_off, sl2_col, pos2 = topo.sell_layout(rowptr2, colidx2)
        sl1_off, sl1_col, pos1 = topo.sell_layout(rowptr1, colidx1)
        cell_outflow = np.full(topo.nt, -1, dtype=np.int8)
        cell_outflow[out_f[:, 0]] = out_f[:, 1]
        # outflow-facet term as a row list: rows = the 3 P2 dofs of every outflow facet, columns = the 6
        # dofs of the adjacent cell (duplicates across neighbouring facets are simply summed by the owner)
        a_l = np.array([1, 0, 0])
        b_l = np.array([2, 2, 1])
        ent = []
        for c, k in out_f:
            for i in (a_l[k], b_l[k], 3 + k):
                for j in range(6):
                    ent.append((int(topo.cell_dofs[c, i]), int(topo.cell_dofs[c, j]), int(c) * 36 + int(i) * 6 + j))
        ent.sort()
        bo_rows = sorted({e[0] for e in ent})
        bo_ptr = np.zeros(len(bo_rows) + 1, np.int32)
        for e in ent:
            bo_ptr[bo_rows.index(e[0]) + 1] += 1
        bo_ptr = np.cumsum(bo_ptr).astype(np.int32)
        bo_col = np.array([e[1] for e in ent], np.int32)
        bo_src = np.array([e[2] for e in ent], np.int32)
        bo_rows = np.array(bo_rows, np.int32)
        if topo.np2 <= 4096:
            mf_scat, mf_tptr = topo.matfree_packed(cell_outflow, 1024)
        else:  # matrix-free mode unavailable for this size (kernel falls back to the SELL operators)
            mf_scat, mf_tptr = topo.matfree_maps(1024)
        return dict(nv=topo.nv, nt=topo.nt, ne=topo.ne, coords=np.asarray(coords, np.float64),
                    cell_dofs_soa=np.ascontiguousarray(topo.cell_dofs.T, dtype=np.int32),
                    cell_outflow=cell_outflow,
                    rowptr2=rowptr2, colidx2=colidx2, asm2_ptr=asm2_ptr, asm2_src=asm2_src,
                    rowptr1=rowptr1, colidx1=colidx1, asm1_ptr=asm1_ptr, asm1_src=asm1_src,
                    sl2_off=sl2_off, sl2_col=sl2_col, sl1_off=sl1_off, sl1_col=sl1_col, pos2=pos2, pos1=pos1,
                    mf_scat=mf_scat, mf_tptr=mf_tptr, bo_rows=bo_rows, bo_ptr=bo_ptr, bo_col=bo_col, bo_src=bo_src,
                    g2_ptr=gat["p2"][0], g2_src=gat["p2"][1], g1_ptr=gat["p1"][0], g1_src=gat["p1"][1],
                    bcu_flag=bc["bcu_flag"], bcu_gx=bc["bcu_gx"], bcp_flag=bc["bcp_flag"],
                    af=af, af_edges=af_edges, tags=bc["tags"])

    # ------------------------------------------------------------------
    @property
    def u_n(self) -> torch.Tensor:
        """(B, N2, 2) velocity dofs [dof][component]."""
        return self.t["u_n"]

    @property
    def p_n(self) -> torch.Tensor:
        return self.t["p_n"]

    def reset_state(self):
        self.t["u_n"].zero_()
        self.t["p_n"].zero_()
        self.t["work"].zero_()  # (also drops the initial-guess history of the velocity solve)
        self.iters.zero_()
        self.steps_done = 0

    def assemble(self, stream=None):
        rc = self.lib.mdq_ipcs_assemble(C.byref(self.desc), _lib.stream_ptr(stream))
        _lib.check(rc, "mdq_ipcs_assemble")
        self.assembled = True
        if self.pressure_direct == "device":
            self.factorize_pressure_device(stream)
        elif self.pressure_direct:
            self._factorize_pressure()

    # capacities of the device-built factors (limits of mdq_ipcs_factorize_pressure: 8 parts, 112 interior nodes per
    # part, 48 separator nodes per part, 112 separator nodes)
    PD_DEVICE_CAP = dict(NPART=8, NPW=8 * 112 * 112, NPF=8 * 112 * 48, NPGI=8 * 48, NPS=112 * 112 + 8 * 48 * 48, NPGK=4096)

    def factorize_pressure_device(self, stream=None):
        """The factorisation of every environment's pressure matrix ON THE DEVICE (`mdq_ipcs_factorize_pressure`: the
        reference re-factorises with MUMPS after every remesh, flow_solver.py:318-328): fills the pd_* arrays the
        solve phase reads and switches the descriptor to the direct solve.  Needs the operators' set-up data (after
        `assemble()` or `mdq_ipcs_setup_matfree`).  `self.pd_status` (device int32 [B]): 0, or < 0 where a mesh exceeds
        the kernel's limits (that environment keeps the Krylov solve)."""
        d = self.desc
        if self.pd_status is None:
            self.pd_status = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self._pd_dev = pd_device_tables(d, self.B, self.cap["NV"], self.device, self.PD_DEVICE_CAP, self._pd_dev)
        self.t.update(self._pd_dev)
        _lib.check(self.lib.mdq_ipcs_factorize_pressure(C.byref(d), self.pd_status.data_ptr(), _lib.stream_ptr(stream)),
                   "mdq_ipcs_factorize_pressure")
        d.pd_enabled = 1
        self.pds = None

    def update_inflow(self, profile, time: float, stream=None):
        """Time dependent inflow (flow_solver.py:70-73,369-371: `inflow.time = gtime` before the three assemblies apply
        the boundary conditions): new Dirichlet values profile(x, y, t) at the inlet dofs of every environment, then the
        vectors that depend on them (the lifting vectors A1[:, bc] g and M[:, bc] g) rebuilt on the device by
        `mdq_ipcs_setup_matfree` (which leaves the operators' other data as they are: same mesh)."""
        if self._inlet is None:
            self._inlet = []
            for t_, p_ in zip(self.topos, self.per):
                d = t_.boundary_conditions(p_["coords"])["inlet_dofs"]
                self._inlet.append((d, t_.dof_coords(p_["coords"])[d]))
            self._gx_host = self.t["bcu_gx"].cpu().numpy().copy()
        for b, (d, xy) in enumerate(self._inlet):
            self._gx_host[b, d] = np.asarray(profile(xy[:, 0], xy[:, 1], float(time)), dtype=np.float64)
        self.t["bcu_gx"].copy_(torch.from_numpy(self._gx_host), non_blocking=True)
        rc = self.lib.mdq_ipcs_setup_matfree(C.byref(self.desc), _lib.stream_ptr(stream))
        _lib.check(rc, "mdq_ipcs_setup_matfree")

    def _factorize_pressure(self):
        """Host factorisation of every environment's (scaled, BC-eliminated) pressure matrix
        (`LUSolver('mumps')` of A2, flow_solver.py:150-159) -> substructuring factors on the device."""
        from .pressure_direct import build_pressure_direct
        torch.cuda.synchronize(self.device)
        K1s = self.t["K1s"].cpu().numpy()
        pds = []
        for b, p in enumerate(self.per):
            nv = p["nv"]
            key = (id(self.topos[b]), p["coords"].tobytes())
            if key not in self._pd_cache:
                rp, ci, pos = p["rowptr1"], p["colidx1"], p["pos1"]
                rows = np.repeat(np.arange(nv), np.diff(rp))
                K = np.zeros((nv, nv))
                K[rows, ci[:rp[-1]]] = K1s[b][pos]
                self._pd_cache[key] = build_pressure_direct(p["coords"], K, self.pressure_parts)
            pds.append(self._pd_cache[key])
        B, NV = self.B, self.cap["NV"]
        cap = dict(NPART=max(q["nparts"] for q in pds), NPW=max(max(q["W"].size for q in pds), 1),
                   NPF=max(max(q["F"].size for q in pds), 1), NPGI=max(max(q["gidx"].size for q in pds), 1),
                   NPS=max(max(q["Sinv"].size for q in pds), 1), NPGK=max(max(q["gk_col"].size for q in pds), 1))
        self.pd_cap = cap

        def stack(key, n, dtype):
            out = np.zeros((B, n), dtype=dtype)
            for b, q in enumerate(pds):
                a = q[key]
                out[b, :a.size] = a
            return out

        h = dict(pd_hdr=np.array([[q["nI"], q["nG"], q["nparts"], 0] for q in pds], np.int32),
                 pd_node=stack("node", NV, np.int32), pd_meta=stack("meta", cap["NPART"] * 6, np.int32),
                 pd_rowblk=stack("rowblk", NV, np.int32), pd_W=stack("W", cap["NPW"], np.float64),
                 pd_F=stack("F", cap["NPF"], np.float64), pd_gidx=stack("gidx", cap["NPGI"], np.int32),
                 pd_Sinv=stack("Sinv", cap["NPS"], np.float64), pd_gk_ptr=stack("gk_ptr", NV + 1, np.int32),
                 pd_gk_col=stack("gk_col", cap["NPGK"], np.int32), pd_gk_val=stack("gk_val", cap["NPGK"], np.float64))
        d = self.desc
        for k, a in h.items():
            self.t[k] = torch.from_numpy(a).to(self.device)
            setattr(d, k, self.t[k].data_ptr())
        d.NPART, d.NPW, d.NPF, d.NPGI, d.NPS, d.NPGK = (cap[k] for k in ("NPART", "NPW", "NPF", "NPGI", "NPS", "NPGK"))
        d.pd_enabled = 1
        self.pds = pds

    def _inflow_table(self, nsteps: int, inflow_scale, stream):
        """The device table [B][nsteps] of `mdq_ipcs_evolve_inflow` for the next `nsteps` steps: the caller's own factors
        (a recorded series; shape and finiteness checked here - the library cannot read a device table) or the batch's
        schedules at steps steps_done + 1 .. steps_done + nsteps on every environment's own dt; None without either."""
        if inflow_scale is None:
            if self.inflow is None:
                return None
            dt = self.env_phys_host[:, 2] if self.env_phys_host is not None else self.dt
            f = torch.from_numpy(inflow_factors(self.inflow, dt, self.steps_done, nsteps))
        else:
            f = inflow_scale.detach() if isinstance(inflow_scale, torch.Tensor) else torch.from_numpy(
                np.ascontiguousarray(inflow_scale, dtype=np.float64))
            if tuple(f.shape) != (self.B, int(nsteps)):
                raise ValueError(f"inflow_scale must have shape ({self.B}, {int(nsteps)}) (one factor per environment and step), "
                                 f"got {tuple(f.shape)}")
            if not bool(torch.isfinite(f).all()):
                raise ValueError("inflow_scale must be finite")
            f = f.to(torch.float64).contiguous()
        if f.is_cuda:
            return f
        # asynchronous upload on the launch stream: page-locked staging, the copy is ordered in front of the kernels
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        with torch.cuda.stream(s):
            return f.pin_memory().to(self.device, non_blocking=True)

    PROFILE_MODES = (2, 3)      # operator modes with one launch sequence per step: what mdq_ipcs_evolve_profile serves

    @classmethod
    def mode_serves_profile(cls, mode: int, n2: int) -> bool:
        """Whether a batch of operator mode `mode` whose largest mesh has `n2` velocity dofs takes an inflow profile: modes
        2 / 3, asked for or what the auto modes -1 / -2 choose (`operator_mode_limits`: mode 3 up to 3 402 dofs, mode 2 up to
        3 584 - the choice of `ipcs_evolve_impl` for a batch that carries the tile pointers, as every IpcsBatch does)."""
        mode = int(mode)
        # (an explicit mode 2 / 3 beyond its own limit is refused by the entry point, with the limit in the message)
        return mode in cls.PROFILE_MODES or ((mode < 0 or mode > 7) and operator_mode_limits(n2)["per_step"])

    def serves_profile(self) -> bool:
        return self.mode_serves_profile(self.desc.mode, self.N2)

    def _profile_table(self, nsteps: int, inflow_times, stream):
        """The device table `values` [B][nsteps][NIN] of `mdq_inflow_profile` for the next `nsteps` steps: every profile
        evaluated on the host (inflow.py: `profile_values`, validated there) at `inflow_times` ((nsteps,) or (B, nsteps)) or,
        by default, at (steps_done + s) * dt_b, s = 1 .. nsteps - the clock of the schedules."""
        if inflow_times is None:
            dt = self.env_phys_host[:, 2] if self.env_phys_host is not None else self.dt
            times = step_times(dt, self.steps_done, nsteps, self.B)
        else:
            times = np.asarray(inflow_times.detach().cpu().numpy() if isinstance(inflow_times, torch.Tensor) else inflow_times,
                               dtype=np.float64)
            if times.shape not in ((int(nsteps),), (self.B, int(nsteps))):
                raise ValueError(f"inflow_times must have shape ({int(nsteps)},) or ({self.B}, {int(nsteps)}), got {times.shape}")
        vals = torch.from_numpy(profile_values(self.inflow_profile, self._prof_tab, times))
        assert tuple(vals.shape) == (self.B, int(nsteps), self._prof_desc.NIN)
        # asynchronous upload on the launch stream: page-locked staging, the copy is ordered in front of the kernels
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        with torch.cuda.stream(s):
            return vals.pin_memory().to(self.device, non_blocking=True)

    def evolve(self, nsteps: int = 1, stream=None, out=None, inflow_scale=None, inflow_times=None):
        """Advance all environments `nsteps` IPCS steps; returns (drag, lift) (B,nsteps) device tensors.  `inflow_scale`:
        explicit (B, nsteps) inflow factors for these steps (tensor or array) in place of the batch's schedules.
        `inflow_times` (a batch with `inflow_profile` only): the times, (nsteps,) or (B, nsteps), at which the profiles are
        evaluated for these steps in place of (steps_done + s) * dt_b."""
        if self.inflow_profile is not None:
            return self._evolve_profile(nsteps, stream, out, inflow_scale, inflow_times)
        if inflow_times is not None:
            raise ValueError("inflow_times needs a batch with inflow_profile")
        ftab = self._inflow_table(nsteps, inflow_scale, stream)       # (validated before anything is launched)
        if not self.assembled:
            self.assemble(stream)
        if out is None:
            drag = torch.empty((self.B, nsteps), dtype=torch.float64, device=self.device)
            lift = torch.empty_like(drag)
        else:
            drag, lift = out
        if ftab is None:
            rc = self.lib.mdq_ipcs_evolve(C.byref(self.desc), int(nsteps), drag.data_ptr(), lift.data_ptr(),
                                          self.iters.data_ptr(), _lib.stream_ptr(stream))
            _lib.check(rc, "mdq_ipcs_evolve")
        else:
            rc = self.lib.mdq_ipcs_evolve_inflow(C.byref(self.desc), int(nsteps), drag.data_ptr(), lift.data_ptr(),
                                                 self.iters.data_ptr(), ftab.data_ptr(), _lib.stream_ptr(stream))
            _lib.check(rc, "mdq_ipcs_evolve_inflow")
            self._inflow_keep = ftab        # (the launch reads it: alive until the next one replaces it)
        self.steps_done += nsteps
        return drag, lift

    def _evolve_profile(self, nsteps, stream, out, inflow_scale, inflow_times):
        """`evolve` of a batch with inflow profiles: one `mdq_ipcs_evolve_profile` call for all `nsteps` steps."""
        if inflow_scale is not None:
            raise ValueError("inflow_scale cannot be combined with inflow_profile: a batch has one kind of time-dependent inflow")
        if int(nsteps) <= 0:
            raise ValueError("nsteps must be positive")
        if not self.serves_profile():       # (the entry point refuses as well - before the assembly is launched, here)
            raise _lib.MeshDQNHipError(f"operator mode {int(self.desc.mode)} runs the steps of a call inside one kernel: an inflow "
                                       f"profile is served by the per-step path (modes 2 / 3, or update_inflow + evolve(1))")
        vals = self._profile_table(nsteps, inflow_times, stream)      # (validated before anything is launched)
        if not self.assembled:
            self.assemble(stream)
        if out is None:
            drag = torch.empty((self.B, nsteps), dtype=torch.float64, device=self.device)
            lift = torch.empty_like(drag)
        else:
            drag, lift = out
        self._prof_desc.values = vals.data_ptr()
        rc = self.lib.mdq_ipcs_evolve_profile(C.byref(self.desc), int(nsteps), drag.data_ptr(), lift.data_ptr(),
                                              self.iters.data_ptr(), C.byref(self._prof_desc), _lib.stream_ptr(stream))
        _lib.check(rc, "mdq_ipcs_evolve_profile")
        self._inflow_keep = vals            # (the launch reads it: alive until the next one replaces it)
        self.steps_done += nsteps
        return drag, lift

    def check(self):
        """Synchronises and raises if any `evolve` since the last call abandoned a step (status words of the descriptor: the
        two-workgroup operator modes 4 / 7 give a step up when a team barrier times out - csrc/mdq_ipcs_team.hip `team_failed`; the
        forces of that step are NaN and u_n / p_n keep the last completed step).  `evolve` itself never synchronises."""
        st = self.status.cpu().numpy()
        if (st != 0).any():
            self.status.zero_()
            raise _lib.MeshDQNHipError(f"IPCS step abandoned in environment(s) {np.flatnonzero(st)[:8].tolist()}: team barrier "
                                       "time-out (another process or stream held CUs of a two-workgroup operator mode)")

    def evolve_timed(self, nsteps: int = 1, stream=None, out=None):
        """`evolve` with HIP events around every kernel (mode 3): returns (drag, lift, ms) where ms[3] are the
        accumulated durations of the velocity / pressure / correction kernels over the nsteps."""
        if self.inflow is not None or self.inflow_profile is not None:     # (mdq_ipcs_evolve_timed takes no table: it would step under the constant parabola)
            raise _lib.MeshDQNHipError("evolve_timed does not apply inflow schedules or profiles (measurement aid of the constant inflow)")
        if not self.assembled:
            self.assemble(stream)
        if out is None:
            drag = torch.empty((self.B, nsteps), dtype=torch.float64, device=self.device)
            lift = torch.empty_like(drag)
        else:
            drag, lift = out
        ms = (C.c_double * 3)()
        rc = self.lib.mdq_ipcs_evolve_timed(C.byref(self.desc), int(nsteps), drag.data_ptr(), lift.data_ptr(),
                                            self.iters.data_ptr(), _lib.stream_ptr(stream), ms)
        _lib.check(rc, "mdq_ipcs_evolve_timed")
        self.steps_done += nsteps
        return drag, lift, [ms[0], ms[1], ms[2]]

    def probe_forces(self, u: torch.Tensor, p: torch.Tensor, stream=None):
        """u (B,F,N2,2), p (B,F,NV) -> drag, lift (B,F)."""
        F = u.shape[1]
        assert u.shape == (self.B, F, self.N2, 2) and p.shape == (self.B, F, self.cap["NV"])
        u = u.contiguous()
        p = p.contiguous()
        drag = torch.empty((self.B, F), dtype=torch.float64, device=self.device)
        lift = torch.empty_like(drag)
        rc = self.lib.mdq_probe_forces(C.byref(self.desc), F, u.data_ptr(), p.data_ptr(), drag.data_ptr(),
                                       lift.data_ptr(), _lib.stream_ptr(stream))
        _lib.check(rc, "mdq_probe_forces")
        return drag, lift

    # ------------------------------------------------------------------
    def algorithmic_bytes_per_step(self, iters_per_step=None) -> float:
        """SURVEY.md 8(d) accounting (assembled-CSR convention): every SpMV streams its CSR matrix
        once (fp64 values, int32 indices), vector passes 8 B per entry per vector.  This is the
        figure of merit the survey defines; the matrix-free modes move far fewer bytes
        (see `implemented_bytes_per_step`)."""
        tot = 0.0
        it = iters_per_step
        for b, p in enumerate(self.per):
            nv, nt, ne = p["nv"], p["nt"], p["ne"]
            n2 = nv + ne
            nnz2, nnz1 = p["colidx2"].size, p["colidx1"].size

            def spmv(nnz, n):
                return 12.0 * nnz + 4.0 * (n + 1) + 16.0 * n
            a1 = spmv(4 * nnz2, 2 * n2)
            mm = spmv(nnz2, n2) * 2
            k1 = spmv(nnz1, nv)
            elem = 268.0 * nt
            iu, ip, im = (it[b] if it is not None else (6.0, 134.0, 3.0))
            tot += (3 * elem + a1 + iu * (2 * a1 + 10 * 8 * 2 * n2) + k1 + ip * (k1 + 6 * 8 * nv)
                    + mm + im * (mm + 6 * 8 * 2 * n2) + 200.0 * p["af"].shape[0])
        return tot

    def implemented_bytes_per_step(self, iters_per_step, mode: int = 3) -> float:
        """Global-memory bytes the IMPLEMENTED algorithm has to move per batch step (no credit for
        L2 hits; LDS / register resident data not counted), modes 2/3 (matrix-free) with the direct
        pressure solver:
          per operator application: element metadata 6 packed words + 5 geometry doubles per triangle
          per BiCGStab iteration (mode 3): x read + write (16 B per dof)
          per step: u_n, p_n read by the element loops and rewritten, u*, right-hand-side scratch of
          step 2, boundary data, direct-solver factors W, F, Sinv, K[G,I]."""
        tot = 0.0
        for b, p in enumerate(self.per):
            nv, nt, ne = p["nv"], p["nt"], p["ne"]
            n2 = nv + ne
            iu, ip, im = iters_per_step[b]
            apply_b = (24.0 + 40.0) * nt
            napply = 2 + 2 * iu + 2 + im  # rhs1, A x0, 2 per BiCGStab it, rhs3, M x0, 1 per CG it
            per_it_vec = 32.0 * n2 * iu
            state = (16.0 * n2 * 6 + 8.0 * nv * 6) + 12.0 * nt * 3 * 2 + 25.0 * n2
            if self.pds is not None and self.desc.pd_enabled:
                q = self.pds[b]
                prs = 8.0 * (q["W"].size + q["F"].size + q["Sinv"].size + q["gk_val"].size) + 4.0 * (
                    q["gk_col"].size + 2 * nv + q["gidx"].size)
            else:
                prs = ip * (12.0 * p["colidx1"].size)
            tot += napply * apply_b + per_it_vec + state + prs
        return tot

    def tile_mode_bytes_per_step(self, iters_per_step) -> float:
        """Global-memory bytes the element-tile modes (5 / 7) have to move per batch step, no cache credit - the ALGORITHMIC
        bytes of `evolve_team_tiles_kernel` / `evolve_kernel<5>` for the roofline of BASELINE configs[4]:
          per operator application and triangle: 6 packed local-map words + 5 geometry doubles + the outflow byte (65 B);
          per application and touched row of a chunk (T = sum of the chunks' row lists): the list entry (8 B) + the staged input row (16 B);
          per application and row: the accumulated result written and read once (32 B);
          per BiCGStab iteration (two applications): 15 vector streams of 16 B per row (p, s, x, r updates and the two
          epilogues' operands); per mass-CG iteration (one application): 8 streams;
          per step: right-hand-side element loops (3 x 65 B per triangle + u_n / p_n gathers 112 B per triangle), state vectors
          (u_n, p_n, u*, the history slots: 10 x 16 B per row), the pressure solve's factors (direct) or its matrix once (Krylov
          with the matrix on the chip)."""
        tot = 0.0
        for b, p in enumerate(self.per):
            nv, nt, ne = p["nv"], p["nt"], p["ne"]
            n2 = nv + ne
            iu, ip, im = iters_per_step[b]
            touched = float(np.asarray(p["mf_rcnt"]).sum()) if "mf_rcnt" in p else float(6 * nt)
            napply = 1 + 2 * iu + 1 + im                     # A x0, 2 per BiCGStab iteration, M x0, 1 per CG iteration
            apply_b = 65.0 * nt + 24.0 * touched + 32.0 * n2
            vec = (15.0 * iu + 8.0 * im) * 16.0 * n2
            rhs = 3 * (65.0 + 112.0) * nt
            state = 10 * 16.0 * n2 + 4 * 8.0 * nv
            if self.pds is not None and self.desc.pd_enabled:
                q = self.pds[b]
                prs = 8.0 * (q["W"].size + q["F"].size + q["Sinv"].size + q["gk_val"].size) + 4.0 * (
                    q["gk_col"].size + 2 * nv + q["gidx"].size)
            else:
                prs = 12.0 * p["colidx1"].size
            tot += napply * apply_b + vec + rhs + state + prs
        return tot

    def velocity_kernel_bytes(self, iters_per_step) -> float:
        """Global-memory bytes of ONE launch of the dominant kernel (at_velocity_kernel, mode 3) for the whole
        batch, no cache credit: per operator application 64 B of triangle metadata (6 packed words + 5 geometry
        doubles), 2 + 2*it applications (rhs1, A x0, two per BiCGStab iteration); x read + written per iteration
        (32 B per dof); per launch and dof: u_n (staged in LDS once), u* and its four predecessors read, five history
        slots written (the shift + the initial guess), idiag, lift, Dirichlet value and flag = 217 B; p_n once."""
        tot = 0.0
        for b, p in enumerate(self.per):
            nv, nt, ne = p["nv"], p["nt"], p["ne"]
            n2 = nv + ne
            iu = iters_per_step[b][0]
            tot += (2 + 2 * iu) * 64.0 * nt + 32.0 * n2 * iu + 217.0 * n2 + 8.0 * nv
        return tot

    def velocity_kernel_flops(self, iters_per_step) -> float:
        tot = 0.0
        for b, p in enumerate(self.per):
            iu = iters_per_step[b][0]
            tot += p["nt"] * ((1 + 2 * iu) * 600.0 + 1800.0) + (p["nv"] + p["ne"]) * iu * 60.0
        return tot

    def flops_per_step(self, iters_per_step) -> float:
        """fp64 operations (FMA = 2) of the matrix-free path per batch step (element operators only)."""
        tot = 0.0
        for b, p in enumerate(self.per):
            nt = p["nt"]
            iu, ip, im = iters_per_step[b]
            f_vel, f_mass, f_rhs1, f_rhs3 = 2 * 300.0, 2 * 60.0, 2 * 900.0, 2 * 80.0
            tot += nt * ((1 + 2 * iu) * f_vel + (1 + im) * f_mass + f_rhs1 + f_rhs3)
        return tot
