"""`VecEnv2DAirfoil` - B `Env2DAirfoil` environments stepped together on one GPU.

Same per-environment semantics as `meshdqn_amd.env.Env2DAirfoil` (= the reference's
Env2DAirfoil.py:318-428 step / reward / state logic), batched:

  host   mdq_remesh_host        vertex removal + Delaunay restoration + smooth(50)     (C++, threads over envs)
  host   mdq_env_topology_host  edges / P2 dofs / airfoil facets / removable / N-closest / state graph
  GPU    mdq_interpolate_snapshots   S snapshots onto every coarsened mesh              (one launch for all envs)
  GPU    mdq_probe_forces            2S force integrals per env                         (one launch)
  GPU    feature gather (torch indexing) and, optionally, the fused Q-network forward (mdq_gcn_forward)

All environments of one airfoil start from the same smoothed original mesh and share its ground truth and snapshots
(computed once by a base `Env2DAirfoil`, i.e. the reference's first `reset()`); terminated environments
are reset in place.  A batch may mix A airfoils (a list of A configs / base envs): environment b then belongs to
airfoil `airfoil[b]` - its mesh, ground truth, snapshots, polygon and resets are that airfoil's - while every kernel
launch still covers the whole batch (capacities = the largest airfoil's).  Triangulations are identical to the reference's as SETS of cells; the cell ORDER
(an artefact of Qhull in the reference) is the engine's own, so `edge_index` columns come in a different
order than in the single-environment class.
"""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from . import reward as _reward
from .env import Env2DAirfoil
from .flow_leg import FlowLeg, check_flow_forces
from .inflow import canonical_inlet, inflow_factors, leg_profile_table, spec_table
from .ipcs_batch import flow_table
from .mesh_ops import (DeviceTopologyBatch, HostTopologyBatch, mesh_quality_gpu, remesh_batch, remesh_batch_gpu, remesh_workspace,
                       smooth_batch_gpu, smooth_env_gpu)


def _host_cores() -> int:
    """Usable host cores: the cgroup CPU quota when one is set (the MI355X boxes expose 256 logical CPUs
    under a 16-core quota), else the affinity mask.  The pool is sized 2x the quota: the mesh tasks are
    uneven and the extra workers hide the tail."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, 2 * int(q) // int(per)))
    except (OSError, ValueError):
        pass
    return n


# keys whose values may differ between the configs of a batch over several airfoils: everything else - flow / solver /
# agent parameters, hence N_closest, S = solver_steps // save_steps, mu, rho, dt - is batch-wide
_PER_AIRFOIL_KEYS = {("flow_config", "geometry_params", "mesh")} | {
    ("agent_params", k) for k in ("gt_drag", "gt_lift", "gt_time", "u", "p", "plot_dir")}
# ... and, in a mixed-FLOW batch (opt-in: a typo in a yaml stays an error), the flow constants
_PER_FLOW_KEYS = {("flow_config", "flow_params", "mu"), ("flow_config", "flow_params", "rho"),
                  ("flow_config", "solver_params", "dt")}
# ... and, in a mixed-INFLOW batch (its own opt-in), the inflow schedule (inflow.py)
_PER_INFLOW_KEYS = {("flow_config", "flow_params", "inflow")}


def _same_value(a, b) -> bool:
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(_same_value(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b or (isinstance(a, (int, float)) and isinstance(b, (int, float)) and a == b)


def _diff_keys(a, b, path=(), allowed=_PER_AIRFOIL_KEYS):
    """Key paths (tuples) where two configs differ, `allowed` per-config keys excluded."""
    if path in allowed:
        return []
    if isinstance(a, dict) and isinstance(b, dict):
        out = []
        for k in list(a) + [k for k in b if k not in a]:
            if k not in a or k not in b:
                if path + (k,) not in allowed:
                    out.append(path + (k,))
            else:
                out += _diff_keys(a[k], b[k], path + (k,), allowed)
        return out
    return [] if _same_value(a, b) else [path]


def check_airfoil_configs(configs, mixed_flow: bool = False, mixed_inflow: bool = False):
    """A batch over several airfoils: the configs may differ only in the mesh path, gt_drag / gt_lift / gt_time, u / p and
    plot_dir - and, with `mixed_flow`, in flow_params.mu / .rho and solver_params.dt, with `mixed_inflow` in
    flow_params.inflow (two configs may then name the same mesh).  Raises ValueError naming the first offending key."""
    allowed = _PER_AIRFOIL_KEYS | (_PER_FLOW_KEYS if mixed_flow else set()) | (_PER_INFLOW_KEYS if mixed_inflow else set())
    for i, c in enumerate(configs[1:], 1):
        bad = _diff_keys(configs[0], c, allowed=allowed)
        if bad:
            raise ValueError(f"configs 0 and {i} of a mixed-airfoil batch differ in `{'.'.join(map(str, bad[0]))}` (only the mesh, "
                             "gt_drag, gt_lift, gt_time, u, p and plot_dir may differ between airfoils"
                             + ("; mu, rho and dt as well in a mixed-flow batch" if mixed_flow else
                                "; mixed_flow=True / --mixed-flow also admits mu, rho and dt")
                             + ("; the inflow schedule as well in a mixed-inflow batch)" if mixed_inflow else
                                "; mixed_inflow=True / --mixed-inflow also admits flow_params.inflow)"))


def airfoil_assignment(num_envs: int, n_airfoils: int, first_env: int = 0) -> np.ndarray:
    """Airfoil of the environments with global ids first_env .. first_env + num_envs - 1: id mod A (a rank that owns the
    contiguous block of ids `DistContext.shard` hands it sees every airfoil as long as it has at least A environments)."""
    return ((int(first_env) + np.arange(int(num_envs))) % int(n_airfoils)).astype(np.int32)


class VecEnv2DAirfoil:
    FLOW_NRL = FlowLeg.NRL

    def __init__(self, config, num_envs: int, compute_device="cuda", nthreads: int = 0, base_env=None,
                 auto_reset: bool = True, emax: int = 1536, flow_steps: int = 0, flow_rtol: float = 1e-10,
                 gpu_smoothing: bool = True, gpu_topology: bool = True, gpu_remesh: bool = True,
                 flow_overlap: bool = False, flow_pressure: str = "cg", flow_pcg_degree: int = 0, airfoil_of_env=None,
                 mixed_flow: bool = False, mixed_inflow: bool = False):
        """`config`: one config dict, or a list of A of them (a batch over A airfoils, see `check_airfoil_configs`);
        `base_env`: an `Env2DAirfoil` or a list of A of them (None: built from the configs); `airfoil_of_env` (B,) ints in
        [0, A): the airfoil of every environment (default b mod A); `mixed_flow`: the configs may also differ in mu, rho
        and dt (one batch over several Reynolds numbers: `self.flow_of_env`), also on one and the same mesh;
        `mixed_inflow`: the configs may also differ in flow_params.inflow, the inflow schedule (inflow.py:
        `self.inflow_of_env`, (B, 4) rows amplitude, pulsation, frequency, phase - set for a single scheduled config as well)
        or a callable profile(x, y, t) (the S3 flow leg then steps under `self.flow.inflow_profile`, the table of inlet values
        of every environment; a single config with a callable needs no flag)."""
        self.lib = _lib.load()
        self.B = int(num_envs)
        configs = list(config) if isinstance(config, (list, tuple)) else [config]
        if not configs:
            raise ValueError("config: an empty list")
        self.mixed_flow = bool(mixed_flow)
        self.mixed_inflow = bool(mixed_inflow)
        check_airfoil_configs(configs, mixed_flow=self.mixed_flow, mixed_inflow=self.mixed_inflow)
        self.A = A = len(configs)
        if base_env is None:
            bases = [Env2DAirfoil(c, compute_device=compute_device) for c in configs]
        else:
            bases = list(base_env) if isinstance(base_env, (list, tuple)) else [base_env]
            if len(bases) != A:
                raise ValueError(f"base_env: {len(bases)} base environments for {A} configs")
        self.bases = bases
        if airfoil_of_env is None:
            airfoil = airfoil_assignment(self.B, A)
        else:
            airfoil = np.asarray(airfoil_of_env)
            if airfoil.shape != (self.B,) or not np.issubdtype(airfoil.dtype, np.integer):
                raise ValueError("airfoil_of_env: one integer per environment")
            if self.B and (airfoil.min() < 0 or airfoil.max() >= A):
                raise ValueError(f"airfoil_of_env: values outside [0, {A})")
        self.airfoil = np.ascontiguousarray(airfoil, dtype=np.int32)
        config = configs[0]
        self.device = torch.device(compute_device)
        # workers of the host engine's persistent pool (one environment per task)
        self.nthreads = int(nthreads) if nthreads > 0 else max(1, min(_host_cores(), self.B))
        self.auto_reset = auto_reset
        self.gpu_smoothing = bool(gpu_smoothing)   # mdq_smooth (dataflow kernel) instead of the host loop
        # mdq_env_topology (device engine, bit-identical to the host engine): the host then only re-triangulates the
        # cavity of a removed vertex; needs the GPU smoothing path (coordinates stay on the device)
        self.gpu_topology = bool(gpu_topology) and self.gpu_smoothing
        # mdq_remesh (cavity re-triangulation + Lawson flips on the device): with it the meshes never leave the GPU;
        # the host arrays `coords / cells / nv / nt` are then read-only mirrors refreshed every step
        self.gpu_remesh = bool(gpu_remesh) and self.gpu_topology
        # S3 ("north-star step"): after every remesh, `flow_steps` IPCS steps on the coarsened mesh warm-started
        # from the interpolated last snapshot (0 = the reference's step, which never re-solves the flow)
        self.flow_steps, self.flow_rtol = int(flow_steps), float(flow_rtol)
        # S3 with the IPCS step of env step k running on a second stream BESIDE the Q-forward of step k and the vertex
        # removal / smoothing of step k + 1 (the state and the reward do not depend on the re-solved flow; the smoothing
        # kernel is one wave per mesh, the IPCS kernels take the other half of the chip): the flow stream works on a
        # private copy of the meshes and the drag / lift of the re-solved flow are reported one step later
        # (`infos["flow_lag"] = 1`).  The streams must sit on different hardware queues: GPU_MAX_HW_QUEUES >= 8 (set by
        # the package at import when the variable is not set)
        self.flow_overlap = bool(flow_overlap) and self.flow_steps > 0 and self.gpu_remesh
        # pressure solve of the S3 flow step on the freshly coarsened mesh: "cg" (Jacobi-CG, ~165 iterations, 0.28 ms on the
        # flow stream) or "direct" = what the reference does at a remesh (re-factorise: mdq_ipcs_factorize_pressure on the
        # device, 0.86 ms per batch, then a direct solve with 0 iterations; an environment whose mesh exceeds the kernel's
        # limits falls back to CG by itself).  Beside the smoothing kernel "direct" costs 1-5 % of the env step, 11 % of the
        # learning loop (its flow leg no longer hides next to the optimiser chain): one solve per mesh does not pay for a
        # factorisation, so "cg" is the default here; FlowSolver / deploy (thousands of steps per mesh) factorise
        if flow_pressure not in ("cg", "direct"):
            raise ValueError("flow_pressure: 'cg' or 'direct'")
        self.flow_pressure = flow_pressure
        self.flow_pcg_degree = int(flow_pcg_degree)     # Chebyshev degree of the pressure CG's preconditioner (0: Jacobi-CG kernel)
        base = bases[0]
        self.base = base
        ap = config["agent_params"]
        self.N = int(ap["N_closest"])
        self.TIME_REWARD = float(ap["time_reward"])
        self.threshold = float(ap["threshold"])
        self.goal_vertices = float(ap["goal_vertices"])
        self.timesteps = int(ap["timesteps"])
        self.NEGATIVE_REWARD = -1.0
        # opt-in (not in the reference): the lift in the reward and in the accuracy stop - batch-wide numbers, like `threshold`
        self.lift = _reward.LiftSpec.from_config(ap)
        # opt-in as well: the mesh quality (one mdq_mesh_quality launch per step) in the reward and as a stop - batch-wide too
        self.quality = _reward.QualitySpec.from_config(ap)
        self.S = len(base.original_u)
        if any(len(bb.original_u) != self.S or np.asarray(bb.gt_drag).shape != (self.S,) for bb in bases):
            raise ValueError("snapshots: every airfoil needs the same S = solver_steps // save_steps snapshots and gt_drag values")
        if not self.mixed_flow and any(bb.flow_solver.mu != base.flow_solver.mu or bb.flow_solver.rho != base.flow_solver.rho or
                                       bb.flow_solver.dt_value != base.flow_solver.dt_value for bb in bases):
            raise ValueError("flow_params / solver_params: mu, rho and dt must agree across the airfoils (mixed_flow=True "
                             "admits one flow condition per config)")
        # mixed-flow batch: mu, rho, dt of every environment's config, and the table both descriptors that carry the
        # constants point at (the probe's light descriptor and the flow leg's: mdq_ipcs_desc.env_phys), uploaded once
        self.flow_of_env = self.env_phys = None
        if self.mixed_flow:
            per_cfg = np.array([[bb.flow_solver.mu, bb.flow_solver.rho, bb.flow_solver.dt_value] for bb in bases], np.float64)
            self.flow_of_env = per_cfg[self.airfoil]                                                   # (B, 3)
            table = flow_table(self.flow_of_env[:, 0], self.flow_of_env[:, 1], self.flow_of_env[:, 2], self.B)
            self.env_phys = torch.from_numpy(table).to(self.device)
        # the descriptors' scalar mu / rho / dt (validated, not read by the kernels, when a table is set): the table's row 0 -
        # environment 0's config, which need not be configs[0] (`airfoil_of_env`, `airfoil_assignment` on a rank > 0)
        self._flow0 = base.flow_solver if self.flow_of_env is None else SimpleNamespace(
            mu=float(self.flow_of_env[0, 0]), rho=float(self.flow_of_env[0, 1]), dt_value=float(self.flow_of_env[0, 2]))
        # inflow schedules (inflow.py): every config's base environment computed its ground truth and snapshots under its own,
        # and the per-airfoil source tables carry them per environment - S1 needs nothing else.  The S3 flow leg always
        # restarts from the last snapshot, at time solver_steps * dt_b: environment b's factors are a_b((solver_steps + s) dt_b),
        # s = 1 .. flow_steps - a static table, built once
        specs = [getattr(bb.flow_solver, "inflow_spec", None) for bb in bases]
        if not self.mixed_inflow and any(s_ != specs[0] for s_ in specs):
            raise ValueError("flow_params: the inflow schedule must agree across the airfoils (mixed_inflow=True admits one "
                             "per config)")
        # ... and callables profile(x, y, t), the non-separable kind: the leg's values at every config's canonical inlet (the
        # inlet points of the original mesh: boundary vertices are never removed or moved) are as static as the factors; the
        # leg maps the points to the dofs of every new mesh on the device.  A batch that mixes the kinds goes through that one
        # table (a schedule config: its factors times the parabola, None: the parabola)
        profs = [getattr(bb.flow_solver, "inflow_profile", None) for bb in bases]
        if not self.mixed_inflow and any(p_ != profs[0] for p_ in profs):
            raise ValueError("flow_params: the inflow profile must agree across the airfoils (mixed_inflow=True admits one "
                             "per config)")
        tab = spec_table(specs)
        self.inflow_of_env = None if tab is None else tab[self.airfoil]                                 # (B, 4)
        self._flow_inflow = self._flow_profile = None
        if any(p_ is not None for p_ in profs) and self.flow_steps > 0:
            inlets = [canonical_inlet(bb._orig_topo, bb._orig_topo.coords) for bb in bases]
            ptab = leg_profile_table(inlets, profs, specs, [bb.flow_solver.dt_value for bb in bases], self.airfoil,
                                     int(base.solver_steps), self.flow_steps)
            self._flow_profile = {k: torch.from_numpy(v).to(self.device) for k, v in ptab.items()}
        elif tab is not None and self.flow_steps > 0:
            dts = (self.flow_of_env[:, 2] if self.flow_of_env is not None else
                   np.array([bb.flow_solver.dt_value for bb in bases], np.float64)[self.airfoil])
            f = inflow_factors([specs[a] for a in self.airfoil], dts, int(base.solver_steps), self.flow_steps)
            self._flow_inflow = torch.from_numpy(f).to(self.device)
        # per airfoil (index a): ground truth, initial mesh, polygon, interpolation source; one airfoil keeps the arrays of
        # the single-airfoil batch (gt_drag (S,), x0 (NV, 2), ...)
        self.gt_drags = np.stack([np.asarray(bb.gt_drag, dtype=np.float64) for bb in bases])            # (A, S)
        self.gt_drag = self.gt_drags[0] if A == 1 else self.gt_drags
        self.gt_lift = (np.asarray(base.gt_lift, dtype=np.float64) if A == 1 else
                        np.stack([np.asarray(bb.gt_lift, dtype=np.float64) for bb in bases]))
        topos = [bb._orig_topo for bb in bases]
        topo0 = topos[0]
        # capacities: the largest airfoil's (the kernel instance K = 1 / 4 / 16 follows from them)
        self.NV, self.NT = max(t.nv for t in topos), max(t.nt for t in topos)
        self.NE = max(t.ne for t in topos)
        self.NP = self.NV + self.NE
        self.EMAX = int(emax)
        self.nv0s = np.array([t.nv for t in topos], np.int32)                                           # (A,)
        self.nt0s = np.array([t.nt for t in topos], np.int32)
        self._x0s = np.zeros((A, self.NV, 2))                   # initial meshes at the batch's row strides (zero padding)
        self._cells0s = np.zeros((A, self.NT, 3), np.int32)
        for a, t in enumerate(topos):
            self._x0s[a, :t.nv] = t.coords
            self._cells0s[a, :t.nt] = t.cells
        self.x0 = topo0.coords.copy() if A == 1 else self._x0s
        self.cells0 = np.ascontiguousarray(topo0.cells, dtype=np.int32) if A == 1 else self._cells0s
        self.polygons = [np.ascontiguousarray(bb.polygon, dtype=np.float64) for bb in bases]
        self.polygon = self.polygons[0] if A == 1 else self.polygons
        self.interps = [bb._interp for bb in bases]
        self.interp = self.interps[0]
        self.mu = base.flow_solver.mu
        B, NV, NT, NP, N = self.B, self.NV, self.NT, self.NP, self.N
        self.NAF = int(max(max((t.facet_tags() == 1).sum(), 1) for t in topos))
        # host state + outputs of the topology engine
        nse1_cap = 0
        for t in topos:
            nbr_ptr = t.vertex_adjacency()[0]
            deg = np.zeros(64 * (NV // 64 + 1), np.int64)
            deg[:t.nv] = np.diff(nbr_ptr) + 1
            nse1 = int(64 * deg.reshape(-1, 64).max(axis=1).sum())        # SELL-64 entries of the P1 Laplacian, initial mesh
            nse1_cap = max(nse1_cap, (int(1.2 * nse1) + 63) // 64 * 64)
        # outflow rows of the facet term: two vertices + one edge dof per outflow facet, shared vertices counted once
        nbo_cap = max(max(64, 2 * (2 * int((t.facet_tags() == 3).sum()) + 1)) for t in topos)
        af = None if A == 1 else self.airfoil
        self.topo = HostTopologyBatch(B, NV, NT, self.NE, self.NAF, N, self.EMAX, self.polygon,
                                      ipcs=self.flow_steps > 0 and not self.gpu_topology, nse1_cap=nse1_cap,
                                      nbo_cap=nbo_cap, airfoil=af)
        self.dtopo = ftopo = None
        if self.gpu_topology:
            self.dtopo = DeviceTopologyBatch(B, NV, NT, self.NE, self.NAF, N, self.EMAX, self.polygon, self.device,
                                             ipcs=self.flow_steps > 0 and not self.flow_overlap, nse1_cap=nse1_cap, nbo_cap=nbo_cap,
                                             airfoil=af)
            if self.flow_overlap:
                # the flow stream's own engine: a private copy of the meshes, the full topology (with the IPCS index data,
                # which only the flow needs: 0.19 ms less on the critical path) and the IPCS step run there
                ftopo = DeviceTopologyBatch(B, NV, NT, self.NE, self.NAF, N, self.EMAX, self.polygon, self.device,
                                            ipcs=True, nse1_cap=nse1_cap, flow_only=True, nbo_cap=nbo_cap, airfoil=af)
        self._packed_host, self._packed_ev, self._pending, self._step_pending = None, torch.cuda.Event(), None, None
        self._restore_args = {}
        self._deferred_mirror = None
        # filled at their first use: the two result sets of the interpolation + its last launch, the rollouts' own main
        # stream, ground truth on the device, descriptor of mdq_env_finish, page-locked buffer of rollout_end
        self._interp_bufs = self._interp_last = self._main_stream = self._gt_drag_dev = self._fin_desc = self._rollout_host = None
        self._interp_i, self._fin_arrive = 0, None
        self.smooth_events = None               # (bench: a list here collects HIP event pairs around every smoothing launch)
        self._calibrated_for, self.calibration_ms = None, []      # (`calibrate_streams`)
        self._node_ptr = torch.arange(B + 1, dtype=torch.int32, device=self.device) * N   # (constant: N rows per graph)
        # the initial meshes on the device (one row per airfoil, at the batch's row strides): source rows of the in-place
        # resets (mdq_restore_rows; several airfoils: mdq_restore_rows_src, the row of environment b's airfoil)
        self._x0_dev = torch.from_numpy(np.ascontiguousarray(self._x0s, dtype=np.float64)).to(self.device)
        self._cells0_dev = torch.from_numpy(np.ascontiguousarray(self._cells0s, dtype=np.int32)).to(self.device)
        self._nv0_dev = torch.from_numpy(self.nv0s.copy()).to(self.device)
        self._nt0_dev = torch.from_numpy(self.nt0s.copy()).to(self.device)
        self._zero_dev = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._airfoil_dev = torch.from_numpy(self.airfoil.copy()).to(self.device)
        self._interp_srcs = None
        if A > 1:       # the interpolation sources of the airfoils: one mdq_interp_src record each, on the device
            recs = (_lib.InterpSrc * A)(*[it.src_record() for it in self.interps])
            raw = np.frombuffer(bytes(recs), dtype=np.uint8).copy()
            self._interp_srcs = torch.from_numpy(raw).to(self.device)
        if self.gpu_remesh:
            self._rstat = torch.zeros(B, dtype=torch.int32, device=self.device)
            self._rstat_host = torch.zeros(B, dtype=torch.int32, pin_memory=True)
            self._mirror_stream = torch.cuda.Stream(device=self.device)
            self._mirror_ev = torch.cuda.Event()
            self._mirror_done = torch.cuda.Event()
        # the S3 flow leg (None without one): descriptor, arrays, the second stream and its double buffering live there
        self.flow = None
        self.flow_t = self.flow_iters = self.flow_status = self.flow_pd_status = None
        self._flow_tile_maps = False
        if self.flow_steps > 0:
            fl = self.flow = FlowLeg(self.device, self.dtopo if self.gpu_topology else self.topo, self._flow0, self.flow_steps,
                                     self.flow_rtol, self.flow_pressure, self.flow_pcg_degree, ftopo, env_phys=self.env_phys,
                                     inflow_scale=self._flow_inflow, inflow_profile=self._flow_profile)
            self.flow_t, self.flow_iters, self.flow_status, self.flow_pd_status = fl.t, fl.iters, fl.status, fl.pd_status
            self._flow_tile_maps = fl.tile_maps
            self.flow_drag = np.zeros((B, self.flow_steps))
            self.flow_lift = np.zeros((B, self.flow_steps))
        self.coords, self.cells, self.nv, self.nt, self.offset = (self.topo.coords, self.topo.cells, self.topo.nv,
                                                                   self.topo.nt, self.topo.offset)
        self.h = self.topo.h   # (device engine: only nsel / n_closest / coord_map / nedges / ne are mirrored here)
        self.steps = np.zeros(B, np.int64)
        # vertex count of the initial mesh, which the time reward and goal_vertices are measured against (per environment
        # in a batch over several airfoils)
        self.initial_num_node = NV if A == 1 else self.nv0s[self.airfoil].astype(np.int64)
        self._gt_drag_env = self.gt_drags[self.airfoil]          # (B, S): the ground truth of every environment's airfoil
        self._gt_lift_env = self._gt_lift_dev = None
        if self.lift.on:
            self.lift.check_gt_lift(self.gt_lift, self.S, names=[bb._mesh_name for bb in bases])
            self._gt_lift_env = np.asarray(self.gt_lift, dtype=np.float64).reshape(A, self.S)[self.airfoil]
        self.new_drags = np.zeros((B, self.S))
        self.new_lifts = np.zeros((B, self.S))
        # mesh quality: q_ref per airfoil from ONE launch on the cached initial meshes; per step the kernel writes
        # `_dev_quality` (B, 2) = (q_min, cot_max) and `_dev_qinfo` (B, 4), mirrored in `mesh_quality` / `quality_cell`
        self.q_ref = self._q_ref_env = self._q_ref_dev = self._dev_quality = self._dev_qinfo = None
        self.mesh_quality, self.quality_cell = np.zeros((B, 2)), np.full(B, -1, np.int32)
        if self.quality.on:
            qual0, _ = mesh_quality_gpu(self._x0_dev, self._cells0_dev, self._nv0_dev, self._nt0_dev)
            self.q_ref = qual0[:, 0].cpu().numpy().copy()                           # (A,)
            self.quality.check_q_ref(self.q_ref, names=[bb._mesh_name for bb in bases])
            self._q_ref_env = self.q_ref[self.airfoil]                              # (B,)
            self._q_ref_dev = qual0[:, 0].contiguous()
            self._dev_quality = torch.empty((B, 2), dtype=torch.float64, device=self.device)
            self._dev_qinfo = torch.empty((B, 4), dtype=torch.int32, device=self.device)
        self.reset_all()

    @property
    def _flow_stream(self):
        """Overlap mode: the stream the flow legs run on (assignable: stream calibration, tools)."""
        return None if self.flow is None else self.flow.stream

    @_flow_stream.setter
    def _flow_stream(self, stream):
        self.flow.stream = stream

    def flow_wait(self):
        """Overlap mode: wait for the IPCS step launched last and return its (drag, lift), or None."""
        return None if self.flow is None else self.flow.results()

    # ------------------------------------------------------------------
    def _reset_env(self, b):
        a = self.airfoil[b]
        self.coords[b] = self._x0s[a]
        self.cells[b] = self._cells0s[a]
        self.nv[b], self.nt[b] = self.nv0s[a], self.nt0s[a]
        self.offset[b] = 0
        self.steps[b] = 0

    def reset_all(self):
        if self.flow is not None:
            self.flow.drop_pending()
        for b in range(self.B):
            self._reset_env(b)
        if self.gpu_topology:
            self._upload_mesh()
        self._refresh()
        if self.A == 1:
            # every environment restarts from the same mesh: cache its derived data (row 0) for in-place resets
            self._init_cache = dict(h={k: a[0].copy() for k, a in self.h.items()}, u=self.u[0].clone(), p=self.p[0].clone(),
                                    drags=self.new_drags[0].copy(), lifts=self.new_lifts[0].copy(),
                                    quality=self.mesh_quality[0].copy(), quality_cell=self.quality_cell[0].copy())
            if self.gpu_topology:
                self._init_cache["dev"] = {k: self.dtopo.t[k][0].clone() for k in self._STATE_KEYS}
        else:
            # every environment of an airfoil restarts from the same mesh: the derived data of one environment per airfoil
            # (rows (A, ...) at the batch's strides; row a = the first environment of airfoil a)
            rows = [int(np.flatnonzero(self.airfoil == a)[0]) if (self.airfoil == a).any() else 0 for a in range(self.A)]
            ri = torch.tensor(rows, dtype=torch.long, device=self.device)
            self._init_cache = dict(h={k: a[rows].copy() for k, a in self.h.items()}, u=self.u[ri].contiguous(),
                                    p=self.p[ri].contiguous(), drags=self.new_drags[rows].copy(), lifts=self.new_lifts[rows].copy(),
                                    quality=self.mesh_quality[rows].copy(), quality_cell=self.quality_cell[rows].copy())
            if self.gpu_topology:
                self._init_cache["dev"] = {k: self.dtopo.t[k][ri].contiguous() for k in self._STATE_KEYS}
        return self.get_state()

    def _cached(self, v, idx):
        """Cached initial rows `v` (one row for one airfoil, (A, ...) for several) for environments idx."""
        return v if self.A == 1 else v[self.airfoil[idx]]

    _STATE_KEYS = ("n_closest", "nsel", "coord_map", "nedges", "edge_src", "edge_dst")   # what get_state reads

    def _upload_mesh(self):
        """Host mesh (page-locked) -> the device engine's input tensors, asynchronously on the current stream."""
        dt, pin = self.dtopo, self.topo.pinned
        dt.coords.copy_(pin["coords"], non_blocking=True)
        dt.cells.copy_(pin["cells"], non_blocking=True)
        dt.nv.copy_(pin["nv"], non_blocking=True)
        dt.nt.copy_(pin["nt"], non_blocking=True)
        dt.offset.copy_(torch.from_numpy(self.offset), non_blocking=False)

    def _restore_initial(self, idx):
        """Reset environments `idx` in place from the cached initial-mesh data (no recomputation)."""
        c = self._init_cache
        idx = np.asarray(idx)
        af = self.airfoil[idx]          # (every environment restarts on its own airfoil)
        self._deferred_mirror = idx     # coords / cells host mirrors: written after the next state has been launched
        self.nv[idx], self.nt[idx] = self.nv0s[af], self.nt0s[af]
        self.offset[idx] = 0
        self.steps[idx] = 0
        # (device engine: only these are mirrored on the host, see _refresh_collect; the others are dead rows)
        keys = ("nsel", "n_closest", "coord_map", "nedges", "ne") if self.gpu_topology else tuple(self.h)
        for k in keys:
            self.h[k][idx] = self._cached(c["h"][k], idx)
        self.new_drags[idx] = self._cached(c["drags"], idx)
        self.new_lifts[idx] = self._cached(c["lifts"], idx)
        self.mesh_quality[idx] = self._cached(c["quality"], idx)
        self.quality_cell[idx] = self._cached(c["quality_cell"], idx)
        # device side: ONE launch restores the rows of every tensor (a dozen index_put launches otherwise).  The
        # argument arrays are built once; only the two per-step buffers (u, p) change their addresses.
        ra = self._restore_arg_arrays()
        ti = torch.from_numpy(idx.astype(np.int32)).to(self.device)
        self._restore_rows(ra, int(ti.numel()), ti)

    def _restore_rows(self, ra, n_idx, ti):
        """mdq_restore_rows over the argument arrays `ra`; several airfoils: mdq_restore_rows_src (each environment from
        the cached row of its own airfoil)."""
        if self.A == 1:
            _lib.check(self.lib.mdq_restore_rows(ra["n"], ra["dst"], ra["src"], ra["nbytes"], n_idx, ti.data_ptr(),
                                                 _lib.stream_ptr()), "mdq_restore_rows")
        else:
            _lib.check(self.lib.mdq_restore_rows_src(ra["n"], ra["dst"], ra["src"], ra["stride"], ra["nbytes"], n_idx,
                                                     ti.data_ptr(), self._airfoil_dev.data_ptr(), _lib.stream_ptr()),
                       "mdq_restore_rows_src")

    def _restore_arg_arrays(self):
        c = self._init_cache
        ra = self._restore_args.get(0)
        if ra is None or ra["coords"] != self._coords_dev.data_ptr():
            pairs = [(self.u, c["u"]), (self.p, c["p"]), (self._coords_dev, self._x0_dev)]
            if self.gpu_topology:
                pairs += [(self.dtopo.t[k], c["dev"][k]) for k in self._STATE_KEYS]
            if self.gpu_remesh:     # the device holds the meshes: reset them there as well
                dt = self.dtopo
                pairs += [(dt.cells, self._cells0_dev), (dt.nv, self._nv0_dev), (dt.nt, self._nt0_dev),
                          (dt.offset, self._zero_dev)]
            n = len(pairs)
            nbytes = [a[0].numel() * a.element_size() for a, _ in pairs]
            # sources: one row per airfoil (stride = the row) or one row for all (the offset: stride 0)
            stride = [nb if b_.numel() * b_.element_size() != nb else 0 for (_, b_), nb in zip(pairs, nbytes)]
            for (a, b_), nb, st in zip(pairs, nbytes, stride):
                assert a.is_contiguous() and b_.is_contiguous() and a.dtype == b_.dtype
                assert b_.numel() * b_.element_size() == (self.A * nb if st else nb)
            ra = self._restore_args[0] = dict(n=n, dst=(C.c_void_p * n)(*[a.data_ptr() for a, _ in pairs]),
                                              src=(C.c_void_p * n)(*[b_.data_ptr() for _, b_ in pairs]),
                                              nbytes=(C.c_int64 * n)(*nbytes), stride=(C.c_int64 * n)(*stride),
                                              coords=self._coords_dev.data_ptr(), keep=pairs)
        ra["dst"][0], ra["dst"][1] = self.u.data_ptr(), self.p.data_ptr()
        return ra

    def _refresh(self):
        """Topology + selection, snapshot interpolation + forces on the GPU, for all envs."""
        self._refresh_launch()
        self._refresh_collect()

    def _refresh_launch(self, readback=True, defer_flow=False, after_topology=None, sparse=0, before_topology=None):
        """Everything of `_refresh` that is enqueued on the stream, up to the asynchronous read-back (`readback=False`:
        the device-resident rollout keeps the results on the device)."""
        dev, h = self.device, self.h
        B, NV, NT, NP = self.B, self.NV, self.NT, self.NP
        if self.gpu_topology:
            dt = self.dtopo
            if before_topology is not None:
                before_topology()
            try:
                dt.run(check=False)                 # status is read back with the other results below
            except Exception:
                dt.set_handover()                   # (a hand-over armed by `before_topology` must not outlive a failed launch:
                raise                               #  a later host-driven step() would overwrite the flow leg's input set)
            if after_topology is not None:
                after_topology()
            t_pts, np1 = dt.t["points"], dt.nv
            npts, npts_extra = np1, dt.t["ne"]          # (P2 points = vertices + edges: added inside the kernel)
        else:
            torch.cuda.current_stream(dev).synchronize()   # pending async uploads read the arrays the engine rewrites
            self.topo.run(self.nthreads)
            up = self.topo.upload
            t_pts = up("points", dev)
            np1 = up("nv", dev)
            npts, npts_extra = np1 + up("ne", dev), None
        it = self.interp
        # two persistent (ping-pong) result sets, zero-filled once: the interpolation writes every valid dof of the current
        # meshes and nothing reads the padding behind them (INVARIANT: rows behind nv / np2 of a set hold stale values of
        # earlier, larger meshes, not zeros) (two 45 MB fills per step were ~30 us of the main chain); the
        # set of the previous step stays intact for whoever still holds it
        if self._interp_bufs is None:
            self._interp_bufs = [(torch.zeros((B, self.S, NP, 2), dtype=torch.float64, device=dev),
                                  torch.zeros((B, self.S, NV), dtype=torch.float64, device=dev)) for _ in range(2)]
        self._interp_i ^= 1
        out_u, out_p = self._interp_bufs[self._interp_i]
        d = _lib.InterpDesc()
        d.B, d.S, d.NP, d.NP1 = B, self.S, NP, NV
        d.src_nv, d.src_nt, d.src_n2 = it.topo.nv, it.topo.nt, it.topo.np2
        d.gnx, d.gny, d.x0, d.y0, d.inv_hx, d.inv_hy = it.grid
        d.npts, d.np1, d.points = npts.data_ptr(), np1.data_ptr(), t_pts.data_ptr()
        d.npts_extra = None if npts_extra is None else npts_extra.data_ptr()
        for k, v in it.t.items():
            setattr(d, k, v.data_ptr())
        if self._interp_srcs is not None:       # several airfoils: every environment from its own airfoil's source
            d.n_src, d.src_of_env, d.srcs = self.A, self._airfoil_dev.data_ptr(), self._interp_srcs.data_ptr()
        d.out_u, d.out_p, d.out_cell = out_u.data_ptr(), out_p.data_ptr(), None
        if sparse and self.gpu_topology:
            # device-resident step: only the entries it reads (vertices, the last snapshot's edge values for the flow leg's warm
            # start, the edges of the airfoil-facet cells for the force integrals) - the edge values of the other snapshots, 60 %
            # of the kernel's work, are read by nothing; the host-driven step() keeps the full fields (self.u is public there)
            d.sparse, d.NT, d.NAF = int(sparse), NT, self.NAF
            d.af_facets, d.naf, d.cell_dofs = dt.t["af_facets"].data_ptr(), dt.t["naf"].data_ptr(), dt.t["cell_dofs"].data_ptr()
        _lib.check(self.lib.mdq_interpolate_snapshots(C.byref(d), _lib.stream_ptr()), "mdq_interpolate_snapshots")
        self._interp_last = (d, int(d.sparse), (out_u, out_p, t_pts, npts, np1, npts_extra))     # (rollout_end completes a sparse field)
        # forces: light mesh descriptor over the batch
        md = _lib.IpcsDesc()
        md.B, md.NV, md.NT, md.NE, md.N2, md.NAF = B, NV, NT, self.NE, NP, self.NAF
        md.mu = self._flow0.mu
        md.env_phys = None if self.env_phys is None else self.env_phys.data_ptr()
        if self.gpu_topology:
            t_coords = dt.coords
            keep = dict(coords=t_coords, cell_dofs=dt.t["cell_dofs"], af_facets=dt.t["af_facets"], nv=np1, nt=dt.nt,
                        ne=dt.t["ne"], naf=dt.t["naf"])
        else:
            t_coords = up("coords", dev)
            keep = dict(coords=t_coords, cell_dofs=up("cell_dofs", dev), af_facets=up("af_facets", dev), nv=np1,
                        nt=up("nt", dev), ne=up("ne", dev), naf=up("naf", dev))
        for k, v in keep.items():
            setattr(md, k, v.data_ptr())
        drag = torch.empty((B, self.S), dtype=torch.float64, device=dev)
        lift = torch.empty_like(drag)
        _lib.check(self.lib.mdq_probe_forces(C.byref(md), self.S, out_u.data_ptr(), out_p.data_ptr(), drag.data_ptr(),
                                             lift.data_ptr(), _lib.stream_ptr()), "mdq_probe_forces")
        self.u, self.p, self._coords_dev = out_u, out_p, t_coords
        self._dev_drag, self._dev_lift = drag, lift
        if self.quality.on:     # ONE launch on the smoothed meshes of this step, either topology engine (off: no launch)
            t_cells = dt.cells if self.gpu_topology else up("cells", dev)
            mesh_quality_gpu(t_coords, t_cells, keep["nv"], keep["nt"], out=(self._dev_quality, self._dev_qinfo))
        fd = fl = None
        if self.flow_overlap:
            if not defer_flow:                  # (deferred: the device-resident step hands over through mdq_env_finish)
                self.flow.start_from_copies(out_u[:, self.S - 1], out_p[:, self.S - 1])
        elif self.flow is not None:
            fd, fl = self.flow.run_inline(keep, out_u[:, self.S - 1], out_p[:, self.S - 1])
            if not self.gpu_topology:
                self.flow_drag, self.flow_lift = fd.cpu().numpy(), fl.cpu().numpy()
        if not readback:
            self._pending = None
            return
        if self.gpu_topology:
            # one read-back for everything the host logic needs: forces + status + the small integer mirrors
            N = self.N
            parts = [drag.reshape(-1).view(torch.int32), lift.reshape(-1).view(torch.int32)]
            nflow = 0
            if fd is not None:      # forces of the re-solved flow ride along (no extra synchronisation)
                parts += [fd.reshape(-1).view(torch.int32), fl.reshape(-1).view(torch.int32)]
                nflow = fd.numel()
            nf = 2 * B * self.S + 2 * nflow
            if self.quality.on:     # (q_min, cot_max) per environment ride behind the forces, their cells behind the integers
                parts.append(self._dev_quality.reshape(-1).view(torch.int32))
                nf += 2 * B
            tail = [self._dev_qinfo[:, 0].contiguous()] if self.quality.on else []
            packed = torch.cat(parts + [dt.status, dt.t["nsel"], dt.t["nedges"], dt.t["ne"], dt.t["coord_map"].reshape(-1),
                                        dt.t["n_closest"].reshape(-1)] + tail)
            if self._packed_host is None or self._packed_host.numel() != packed.numel():
                self._packed_host = torch.empty(packed.numel(), dtype=torch.int32, pin_memory=True)
            self._packed_host.copy_(packed, non_blocking=True)      # page-locked: the copy is queued behind the kernels
            self._packed_ev.record(torch.cuda.current_stream(dev))
            self._pending = (nf, nflow, None if fd is None else tuple(fd.shape))
        else:
            self._pending = (drag, lift)

    def _refresh_collect(self):
        """Wait for the read-back of `_refresh_launch` and update the host mirrors."""
        h, B, N = self.h, self.B, self.N
        if self.gpu_topology:
            nf, nflow, fshape = self._pending
            self._packed_ev.synchronize()
            packed = self._packed_host.numpy()
            fl64 = packed[:2 * nf].view(np.float64)
            ints = packed[2 * nf:]
            if fshape is not None:
                self.flow_drag = fl64[2 * B * self.S:2 * B * self.S + nflow].reshape(fshape).copy()
                self.flow_lift = fl64[2 * B * self.S + nflow:2 * B * self.S + 2 * nflow].reshape(fshape).copy()
            self.new_drags = fl64[:B * self.S].reshape(B, self.S).copy()
            self.new_lifts = fl64[B * self.S:2 * B * self.S].reshape(B, self.S).copy()
            st = ints[:B]
            if (st != 0).any():
                raise _lib.MeshDQNHipError(f"topology kernel failed: env {np.flatnonzero(st)} status {st[st != 0]}")
            h["nsel"][...] = ints[B:2 * B]
            h["nedges"][...] = ints[2 * B:3 * B]
            h["ne"][...] = ints[3 * B:4 * B]
            h["coord_map"][...] = ints[4 * B:4 * B + B * N].reshape(B, N)
            h["n_closest"][...] = ints[4 * B + B * N:4 * B + 2 * B * N].reshape(B, N)
            if self.quality.on:
                self.mesh_quality = fl64[nf - 2 * B:nf].reshape(B, 2).copy()
                self.quality_cell = ints[4 * B + 2 * B * N:5 * B + 2 * B * N].copy()
        else:
            drag, lift = self._pending
            self.new_drags = drag.cpu().numpy().copy()
            self.new_lifts = lift.cpu().numpy().copy()
            if self.quality.on:
                self.mesh_quality = self._dev_quality.cpu().numpy().copy()
                self.quality_cell = self._dev_qinfo[:, 0].cpu().numpy().copy()
        self._pending = None

    # ------------------------------------------------------------------
    def get_state(self):
        """dict of device tensors: x (B,N,2+3S) f32, esrc/edst (sumE,) i32 local ids, edge_ptr (B+1,) i32,
        node_ptr (B+1,) i32 - directly consumable by the fused Q-network forward - plus host copies of
        n_closest / coord_map / nedges."""
        dev, h, B = self.device, self.h, self.B
        x = self._state_features()
        ne = h["nedges"].astype(np.int64)
        edge_ptr = np.zeros(B + 1, np.int32)
        edge_ptr[1:] = np.cumsum(ne)
        if self.gpu_topology:
            # packed edge lists from the padded (B,EMAX) device arrays: one small kernel driven by the offsets (the counts
            # are on the host already, so the output size is known without a device-to-host synchronisation)
            total = int(edge_ptr[-1])
            edge_ptr_d = torch.from_numpy(edge_ptr).to(dev)
            esrc_d = torch.empty(total, dtype=torch.int32, device=dev)
            edst_d = torch.empty(total, dtype=torch.int32, device=dev)
            _lib.check(self.lib.mdq_compact_edges(B, self.EMAX, self.dtopo.t["edge_src"].data_ptr(),
                                                  self.dtopo.t["edge_dst"].data_ptr(), edge_ptr_d.data_ptr(),
                                                  esrc_d.data_ptr(), edst_d.data_ptr(), _lib.stream_ptr()), "mdq_compact_edges")
        else:
            live = np.arange(self.EMAX)[None, :] < ne[:, None]      # (B,EMAX) valid edge slots, row-major = env order
            esrc_d, edst_d = torch.from_numpy(h["edge_src"][live]).to(dev), torch.from_numpy(h["edge_dst"][live]).to(dev)
        pad = {}
        if self.gpu_topology:   # the padded (B,EMAX) edge lists as well (views of the engine's output, valid until
            pad = dict(edge_src_pad=self.dtopo.t["edge_src"], edge_dst_pad=self.dtopo.t["edge_dst"])   # the next step)
        return dict(x=x, esrc=esrc_d, edst=edst_d, **pad,
                    edge_ptr=edge_ptr_d if self.gpu_topology else torch.from_numpy(edge_ptr).to(dev),
                    node_ptr=self._node_ptr,
                    n_closest=h["n_closest"].copy(), coord_map=h["coord_map"].copy(), nedges=h["nedges"].copy(),
                    nsel=h["nsel"].copy())

    # ------------------------------------------------------------------
    def step(self, actions):
        """actions (B,) ints in [0, N]; returns (state, rewards (B,), dones (B,), infos)."""
        self.step_begin(actions)
        return self.step_end()

    def step_begin(self, actions):
        """First half of `step`: everything that is only ENQUEUED (vertex removal, smoothing, topology, interpolation,
        forces, the asynchronous read-back).  The caller may overlap other work (e.g. an optimiser step on another
        stream) with the GPU before `step_end` waits for the results."""
        B, N, h = self.B, self.N, self.h
        actions = np.asarray(actions).astype(np.int64)
        code = np.zeros(B, np.int32)  # 0 ok, 2 broken (Env2DAirfoil.py:342-364)
        shift = actions == N                                   # "do nothing": move the selection window
        pick = (actions >= 0) & (actions < h["nsel"]) & ~shift
        self.offset[shift] += 1
        rem = np.where(pick, h["coord_map"][np.arange(B), np.clip(actions, 0, N - 1)], -1).astype(np.int32)
        code[~shift & ~pick] = 2                               # KeyError in coord_map: "RAN OUT OF VERTICES"
        if self.gpu_remesh:
            dev, dt = self.device, self.dtopo
            rem_d = torch.from_numpy(rem).to(dev)
            dt.offset.copy_(torch.from_numpy(self.offset))
            remesh_batch_gpu(dt.coords, dt.cells, dt.nv, dt.nt, rem_d, self._rstat)
            its = torch.where((rem_d >= 0) & (self._rstat == 0), 50, 0).to(torch.int32)
            smooth_batch_gpu(dt.coords, dt.cells, dt.nv, dt.nt, its)
            # host mirrors of the meshes: device-to-host copies on a side stream, off the critical path of the step
            # (4 MB per 128 meshes; complete before the host logic below reads nv / status)
            pin = self.topo.pinned
            self._mirror_ev.record(torch.cuda.current_stream(dev))
            with torch.cuda.stream(self._mirror_stream):
                self._mirror_stream.wait_event(self._mirror_ev)
                pin["coords"].copy_(dt.coords, non_blocking=True)
                pin["cells"].copy_(dt.cells, non_blocking=True)
                pin["nv"].copy_(dt.nv, non_blocking=True)
                pin["nt"].copy_(dt.nt, non_blocking=True)
                self._rstat_host.copy_(self._rstat, non_blocking=True)
                self._mirror_done.record(self._mirror_stream)
            status = None
        elif self.gpu_smoothing:
            # host: cavity re-triangulation + Delaunay restoration only; GPU: smooth(50) of the changed meshes
            status = remesh_batch(self.coords, self.cells, self.nv, self.nt, rem, 0, self.nthreads)
            dev = self.device
            its = torch.from_numpy(np.where((rem >= 0) & (status == 0), 50, 0).astype(np.int32)).to(dev)
            if self.gpu_topology:
                self._upload_mesh()
                dt = self.dtopo
                smooth_batch_gpu(dt.coords, dt.cells, dt.nv, dt.nt, its)
                # the host engine needs the smoothed coordinates for its next cavity: asynchronous D2H into the
                # page-locked array, complete before this step's results are read back
                self.topo.pinned["coords"].copy_(dt.coords, non_blocking=True)
            else:
                up = self.topo.upload
                tc = up("coords", dev)
                smooth_batch_gpu(tc, up("cells", dev), up("nv", dev), up("nt", dev), its)
                self.topo.pinned["coords"].copy_(tc)    # D2H into the page-locked array (synchronises this stream)
        else:
            status = remesh_batch(self.coords, self.cells, self.nv, self.nt, rem, 50, self.nthreads)
        self._refresh_launch()
        self._step_pending = (code, status)

    def step_end(self):
        """Second half of `step`: wait for the results, rewards / terminal flags / in-place resets, next state."""
        B, N, h = self.B, self.N, self.h
        code, status = self._step_pending
        self._step_pending = None
        # results of the IPCS step launched in the PREVIOUS env step (this step's is still running)
        prev_flow = self.flow.results(previous=True) if self.flow_overlap else None
        self._refresh_collect()
        if status is None:
            self._mirror_done.synchronize()
            status = self._rstat_host.numpy()
        code[status != 0] = 2
        code[h["nsel"] < N] = 2  # out of vertices
        self.steps += 1
        # (B, S) ground truth: every environment's own airfoil; the formula lives in reward.py
        rewards, dones, reasons = _reward.rewards(self.lift, self._gt_drag_env, self.new_drags, self.nv, self.initial_num_node, code,
                                                  self.steps, self.threshold, self.TIME_REWARD, self.goal_vertices, self.timesteps,
                                                  self.NEGATIVE_REWARD, self._gt_lift_env, self.new_lifts, qspec=self.quality,
                                                  quality=self.mesh_quality, q_ref=self._q_ref_env)
        infos = dict(code=code, nv=self.nv.copy(), new_drags=self.new_drags.copy(), new_lifts=self.new_lifts.copy(),
                     reason=reasons)
        if self.quality.on:      # the quality of the step's meshes (before any auto-reset), as the kernel measured it
            infos.update(q_min=self.mesh_quality[:, 0].copy(), min_angle=_reward.min_angle_degrees(self.mesh_quality[:, 1]),
                         quality_cell=self.quality_cell.copy())
        if self.flow_overlap:    # drag / lift of the re-solved flow of the PREVIOUS step's meshes (None at the first step)
            infos.update(flow_lag=1, flow_drag=None if prev_flow is None else prev_flow[0],
                         flow_lift=None if prev_flow is None else prev_flow[1])
        elif self.flow_steps > 0:  # drag / lift of the re-solved flow on the coarsened meshes (before any auto-reset)
            infos.update(flow_lag=0, flow_drag=self.flow_drag.copy(), flow_lift=self.flow_lift.copy())
        if self.auto_reset and dones.any():
            self._restore_initial(np.flatnonzero(dones))
        state = self.get_state()
        if self._deferred_mirror is not None:   # (off the critical path: the GPU is already working on the next state)
            af = self.airfoil[self._deferred_mirror]
            self.coords[self._deferred_mirror] = self._x0s[af]
            self.cells[self._deferred_mirror] = self._cells0s[af]
            self._deferred_mirror = None
        return state, rewards, dones, infos


    # ------------------------------------------------------------------ device-resident rollout
    def _state_features(self):
        """Node features x (B, N, 2 + 3 S) f32 of the current meshes and fields (one launch on the current stream)."""
        dev, B, N, S = self.device, self.B, self.N, self.S
        x = torch.empty((B, N, 2 + 3 * S), dtype=torch.float32, device=dev)
        if self.gpu_topology:
            nc, nsel = self.dtopo.t["n_closest"], self.dtopo.t["nsel"]
        else:
            nc, nsel = self.topo.upload("n_closest", dev), self.topo.upload("nsel", dev)
        _lib.check(self.lib.mdq_state_features(B, N, S, self.NV, self.NP, self._coords_dev.data_ptr(), self.u.data_ptr(),
                                               self.p.data_ptr(), nc.data_ptr(), nsel.data_ptr(), x.data_ptr(),
                                               _lib.stream_ptr()), "mdq_state_features")
        return x

    def _state_device(self, x=None):
        """`get_state` without the host: node features `x` (None: computed here) from device data only; the edge lists stay
        in the padded (B, EMAX) layout the topology engine writes (`mdq_gcn_forward_padded` and `mdq_replay_step` read them
        as they are: no edge offsets, no compaction launches)."""
        dt = self.dtopo
        return dict(x=self._state_features() if x is None else x, node_ptr=self._node_ptr, edge_src_pad=dt.t["edge_src"],
                    edge_dst_pad=dt.t["edge_dst"], nedges_dev=dt.t["nedges"])

    def rollout_device(self, fused, steps: int, explore=None, rand_actions=None, actions=None):
        """`steps` batched env steps WITHOUT a host round trip inside a step: the Q-network forward (`fused`: a
        `FusedGcn`), the epsilon-greedy choice (`explore` (steps,B) bool + `rand_actions` (steps,B) ints, drawn by the
        caller from its own random streams; greedy = first maximum of the Q-row) or given `actions` (steps,B), the
        action decoding, vertex removal, smoothing, topology, interpolation, forces, (S3: the IPCS step), reward /
        terminal logic and the in-place resets are all kernels on the current stream (`mdq_env_act`, `mdq_remesh`,
        `mdq_smooth_fast_env`, `mdq_env_topology`, ..., `mdq_env_result`, `mdq_restore_rows_masked`).
        Same semantics as `steps` calls of `step()` (tested against it).  Returns dict(rewards (steps,B), dones,
        actions, codes, nv, reasons - the bitmask of what ended a step, reward.REASON_*; with the mesh quality on also quality
        (steps,B,2): q_min, cot_max) - read back ONCE at the end, when the
        host mirrors of the environments are refreshed too."""
        cur = torch.cuda.current_stream(self.device)
        if cur == torch.cuda.default_stream(self.device):
            # not on the legacy default stream: with the main chain there, the factorisation kernel of the flow stream
            # was measured to serialise with it (2.5 instead of 1.8 ms per batched step); a stream of the pool is fine
            if self._main_stream is None:
                from .streams import role_streams
                self._main_stream = role_streams(self.device)["main"]
            self._main_stream.wait_stream(cur)
            with torch.cuda.stream(self._main_stream):
                out = self.rollout_device(fused, steps, explore, rand_actions, actions)
            cur.wait_stream(self._main_stream)
            return out
        ro = self.rollout_begin(steps, explore, rand_actions, actions)
        for k in range(int(steps)):
            self.rollout_step(ro, fused)
        return self.rollout_end(ro)

    def calibrate_streams(self, fused, tries: int = 6, steps: int = 8):
        """Pick a flow stream that REALLY runs beside the current (main) stream, by measurement.  HIP maps streams
        round-robin onto hardware queues; besides the pairs that land on one queue (the flow leg then runs behind the
        smoothing kernel: 3.5 ms per batched step instead of 1.85) there are pairs that overlap only partly (2.6 ms;
        two of eight candidates in `tools/time_stream_matrix.py`), and no synthetic probe tried separates those from the
        good ones.  So: a few real env steps with the current flow stream and with up to `tries - 1` fresh ones, the
        fastest stays.  The environments are reset afterwards (`reset_all`); call it on the stream the rollouts will run
        on, once, before they start.  Returns the measured ms per batched step of every candidate."""
        if not (self.flow_overlap and self.gpu_remesh):
            return []
        dev, B = self.device, self.B
        rng = np.random.default_rng(20251)
        cur = torch.cuda.current_stream(dev)

        def timed(k):
            ro = self.rollout_begin(k, rng.random((k, B)) < 0.5, rng.integers(0, self.N + 1, (k, B)))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(cur)
            for _ in range(k):
                self.rollout_step(ro, fused)
            e1.record(cur)
            self.rollout_end(ro)
            e1.synchronize()
            return e0.elapsed_time(e1) / k
        from . import streams as _st
        known = _st.calibrated_flow_stream(dev, cur)
        if known is not None:                       # this process has already chosen a flow stream for this main stream
            self.flow_wait()
            self._flow_stream = known
            self._calibrated_for = cur
            self.calibration_ms = []
            return []
        if (_st.roles_own_queues(dev) and self._flow_stream is _st.role_streams(dev)["flow"] and
                (cur is _st.role_streams(dev)["main"] or cur == _st.role_streams(dev)["main"] or _st._overlaps(self._flow_stream, cur, dev))):
            # CU-mask role streams with every probe passed: a hardware queue each, nothing to choose between.  (The probes of
            # `role_streams` compare the roles with the MAIN role: a caller on another stream - the bench's env groups - is
            # probed here, once, before the shortcut is taken)
            self._calibrated_for = cur
            self.calibration_ms = []
            _st.remember_flow_stream(dev, cur, self._flow_stream, [], "role streams own their hardware queues: no calibration")
            return []
        results = []
        how = "first two candidates agree"
        for t in range(max(1, int(tries))):
            if t > 0:
                self.flow_wait()
                self._flow_stream = _st.new_flow_candidate(dev)
            timed(3)
            results.append((timed(int(steps)), self._flow_stream))
            ms = [r[0] for r in results]
            if len(ms) == 2 and abs(ms[0] - ms[1]) <= 0.03 * min(ms):
                break                               # the role stream and ONE fresh stream agree: both overlap
            if len(ms) >= 2 and min(ms) < 0.85 * max(ms) and ms[-1] <= 1.03 * min(ms):
                how = "both behaviours seen"
                break                               # both behaviours seen and the current candidate is a good one
            if len(ms) > 2:
                how = "full calibration"
        best = min(results, key=lambda r: r[0])
        self.flow_wait()
        self._flow_stream = best[1]
        self._calibrated_for = cur
        self.calibration_ms = [r[0] for r in results]
        _st.remember_flow_stream(dev, cur, best[1], self.calibration_ms, how)
        self.reset_all()
        return self.calibration_ms

    def rollout_begin(self, steps: int, explore=None, rand_actions=None, actions=None):
        """First third of `rollout_device` (the learning loop interleaves its own launches with the steps): uploads the
        per-step action inputs, allocates the per-step outputs; `ro["state"]` is the current batched state on the device
        (x, packed and padded edge lists, `nedges`)."""
        if not self.gpu_remesh:
            raise _lib.MeshDQNHipError("rollout_device needs the device mesh engine (gpu_remesh=True)")
        dev, dt, B, K = self.device, self.dtopo, self.B, int(steps)
        i32 = torch.int32
        if self._pending is not None:
            self._refresh_collect()
        if actions is not None:
            act_all = torch.from_numpy(np.ascontiguousarray(actions, dtype=np.int32).reshape(K, B)).to(dev)
            expl_all = rand_all = None
        else:
            act_all = torch.empty((K, B), dtype=i32, device=dev)
            expl_all = torch.from_numpy(np.ascontiguousarray(explore, dtype=np.uint8).reshape(K, B)).to(dev)
            rand_all = torch.from_numpy(np.ascontiguousarray(rand_actions, dtype=np.int32).reshape(K, B)).to(dev)
        ro = dict(K=K, k=0, given=actions is not None, act=act_all, explore=expl_all, rand=rand_all,
                  rew=torch.empty((K, B), dtype=torch.float64, device=dev), done=torch.empty((K, B), dtype=torch.uint8, device=dev),
                  code=torch.empty((K, B), dtype=i32, device=dev), nv=torch.empty((K, B), dtype=i32, device=dev),
                  rem=torch.empty(B, dtype=i32, device=dev), code_act=torch.empty(B, dtype=i32, device=dev),
                  # step counters: read by every workgroup of mdq_env_finish, written to the other array (si: the current one)
                  d_steps=[torch.from_numpy(self.steps.astype(np.int32)).to(dev), torch.empty(B, dtype=i32, device=dev)], si=0,
                  err=torch.zeros(1, dtype=i32, device=dev), reason=torch.empty((K, B), dtype=i32, device=dev))
        if self.quality.on:     # (q_min, cot_max) of every step: the quality launch of step k writes row k
            ro["quality"] = torch.empty((K, B, 2), dtype=torch.float64, device=dev)
            ro["qinfo"] = torch.empty((K, B, 4), dtype=i32, device=dev)
        if self._gt_drag_dev is None:       # (A, S): row a = airfoil a
            self._gt_drag_dev = torch.from_numpy(np.ascontiguousarray(self.gt_drags, dtype=np.float64)).to(dev)
        if self.lift.on and self._gt_lift_dev is None:
            gl = np.asarray(self.gt_lift, dtype=np.float64).reshape(self.A, self.S)
            self._gt_lift_dev = torch.from_numpy(np.ascontiguousarray(gl)).to(dev)
        dt.offset.copy_(torch.from_numpy(self.offset))
        ro["state"] = self._state_device()
        return ro

    def rollout_step(self, ro, fused, pack: bool = True):
        """One batched env step of a `rollout_begin` context, enqueued on the current stream; afterwards `ro["state"]`
        is the new batched state and `ro["act"][k] / ro["rew"][k] / ro["done"][k]` (device) describe the step (k = ro["k"] - 1).
        `pack=False`: the Q-forward uses the packed parameter copy as it is (a learning loop whose optimiser runs on another
        stream brings it up to date itself, at a point that is ordered against the parameter writes).
        Launches of a step (8 - the smoothing hands back inside its own launch; 14 in round 3): Q-forward (embedding, MLP head),
        `mdq_remesh_act` (action decoding + vertex removal), `mdq_smooth_fast_env`, `mdq_env_topology`,
        `mdq_interpolate_snapshots`, `mdq_probe_forces`, `mdq_env_finish` (reward / terminal logic, hand-over of the meshes
        to the flow stream, in-place resets, node features of the next state).  With the mesh-quality keys set a ninth,
        `mdq_mesh_quality`, sits between `mdq_probe_forces` and `mdq_env_finish`; without them none is added."""
        dt, lib, B, N, S, k = self.dtopo, self.lib, self.B, self.N, self.S, ro["k"]
        if k >= ro["K"]:
            raise IndexError("rollout_step beyond the steps of rollout_begin")
        sp = _lib.stream_ptr
        st, rem = ro["state"], ro["rem"]
        q = None
        if not ro["given"]:
            q = fused.forward_arrays(st["x"], st["node_ptr"], st["edge_src_pad"], st["edge_dst_pad"], None, N, self.EMAX,
                                     pack=pack, edge_cnt=st["nedges_dev"])
        NVc, NTc = dt.coords.shape[1], dt.cells.shape[1]
        _lib.check(lib.mdq_remesh_act(B, NVc, NTc, dt.coords.data_ptr(), dt.cells.data_ptr(), dt.nv.data_ptr(), dt.nt.data_ptr(),
                                      N, None if q is None else q.data_ptr(),
                                      None if ro["explore"] is None else ro["explore"][k].data_ptr(),
                                      None if ro["rand"] is None else ro["rand"][k].data_ptr(), dt.t["nsel"].data_ptr(),
                                      dt.t["coord_map"].data_ptr(), dt.offset.data_ptr(), ro["act"][k].data_ptr(),
                                      rem.data_ptr(), ro["code_act"].data_ptr(), self._rstat.data_ptr(),
                                      *remesh_workspace(self.device, sp(), B, NVc, NTc), sp()), "mdq_remesh_act")
        tm = self.smooth_events     # (bench: HIP events around the launch, on this stream)
        if tm is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        # smooth(50) where a vertex was removed (mdq_env_smooth_iters folded into the smoothing launch)
        smooth_env_gpu(dt.coords, dt.cells, dt.nv, dt.nt, rem, self._rstat, 50)
        if tm is not None:
            e1.record()
            tm.append((e0, e1))
        # overlapped flow leg: the main topology run writes the meshes into the leg's free input set, `mdq_env_finish` the warm
        # start; the leg starts on its stream behind both
        flow = self.flow if self.flow_overlap else None
        sparse = 0 if os.environ.get("MDQ_FULL_INTERP", "") == "1" else (1 if self.flow_steps > 0 else 2)
        if self.quality.on:         # the quality launch inside `_refresh_launch` writes this step's row of the rollout's record
            self._dev_quality, self._dev_qinfo = ro["quality"][k], ro["qinfo"][k]
        self._refresh_launch(readback=False, defer_flow=True, sparse=sparse, before_topology=flow.arm_handover if flow else None,
                             after_topology=flow.mesh_ready if flow else None)
        # ---- the end of the step in one launch
        x = torch.empty((B, N, 2 + 3 * S), dtype=torch.float32, device=self.device)
        d = self._finish_desc(ro, k, x)
        if flow is not None:
            self._finish_handover(d, flow.warm_start_pairs(self.u[:, self.S - 1], self.p[:, self.S - 1]))
        _lib.check(lib.mdq_env_finish(C.byref(d), sp()), "mdq_env_finish")
        if flow is not None:
            flow.start()
        ro["si"] ^= 1
        ro["state"] = self._state_device(x)
        ro["k"] = k + 1

    def _finish_desc(self, ro, k, x):
        """Descriptor of `mdq_env_finish` for step k of a rollout (built once per environment object; the per-step
        pointers are patched in)."""
        dt, B, N, S = self.dtopo, self.B, self.N, self.S
        d = self._fin_desc
        if d is None:
            d = self._fin_desc = _lib.EnvFinishDesc()
            d.B, d.N, d.S, d.NV, d.NP = B, N, S, self.NV, self.NP
            d.nv0, d.timesteps, d.auto_reset = int(self.nv0s[0]), int(self.timesteps), 1 if self.auto_reset else 0
            d.threshold, d.time_reward, d.goal_vertices, d.negative_reward = (float(self.threshold), float(self.TIME_REWARD),
                                                                                float(self.goal_vertices), float(self.NEGATIVE_REWARD))
            d.gt_drag, d.nv, d.rstat = self._gt_drag_dev.data_ptr(), dt.nv.data_ptr(), self._rstat.data_ptr()
            d.topo_status, d.nsel, d.n_closest = dt.status.data_ptr(), dt.t["nsel"].data_ptr(), dt.t["n_closest"].data_ptr()
            self._fin_arrive = torch.zeros(B, dtype=torch.int32, device=self.device)   # (every launch leaves it at zero)
            d.arrive = self._fin_arrive.data_ptr()
            if self.A > 1:          # per-airfoil ground truth, initial vertex counts, cached rows and features
                d.src_of_env, d.nv0_of = self._airfoil_dev.data_ptr(), self._nv0_dev.data_ptr()
            if self.lift.on:        # the lift part of the reward / accuracy stop (off: the tail stays zero, the drag-only step)
                d.gt_lift = self._gt_lift_dev.data_ptr()
                d.lift_weight, d.lift_threshold, d.lift_floor = self.lift.weight, self.lift.threshold, self.lift.floor
            if self.quality.on:     # the quality part (off: the tail stays zero); q_ref [A], the row of the environment's airfoil
                d.quality_ref = self._q_ref_dev.data_ptr()
                d.quality_weight, d.min_quality, d.max_cot = self.quality.weight, self.quality.min_quality, self.quality.max_cot
        c = self._init_cache
        if c.get("x") is None:      # node features of the initial states (what an environment shows right after its reset)
            xi = torch.empty((self.A, N, 2 + 3 * S), dtype=torch.float32, device=self.device)
            _lib.check(self.lib.mdq_state_features(self.A, N, S, self.NV, self.NP, self._x0_dev.data_ptr(), c["u"].data_ptr(),
                                                   c["p"].data_ptr(), c["dev"]["n_closest"].data_ptr(),
                                                   c["dev"]["nsel"].data_ptr(), xi.data_ptr(), _lib.stream_ptr()),
                       "mdq_state_features")
            c["x"] = xi
        d.x_init = c["x"].data_ptr()
        ra = self._restore_arg_arrays()                # (u / p / coords change their addresses from step to step)
        n = ra["n"]
        if n + 2 > _lib.FINISH_MAX_ROWS:
            raise _lib.MeshDQNHipError("mdq_env_finish: too many row arrays")
        d.n_rows = n
        for t in range(n):
            d.dst[t], d.src[t], d.row_bytes[t] = ra["dst"][t], ra["src"][t], ra["nbytes"][t]
            d.src_stride[t] = ra["stride"][t]
            d.handover_dst[t], d.handover_off[t], d.handover_bytes[t] = None, 0, 0
        if not self.auto_reset:                        # nothing is restored: the rows stay as hand-over sources only
            for t in range(n):
                d.src[t] = None
        else:
            # the interpolated snapshots (rows 0 / 1: 0.3 MB per environment) are NOT restored here: every step of a rollout
            # interpolates them again on the current meshes before anything reads them, and the state of a reset environment
            # comes from the cached features (x_init); they stay hand-over sources (the warm start of the flow leg)
            d.src[0] = d.src[1] = None
        d.new_drags = self._dev_drag.data_ptr()
        if self.lift.on:            # (the array the probe launch of this step wrote beside the drags)
            d.new_lifts = self._dev_lift.data_ptr()
        if self.quality.on:         # (what the quality launch of this step wrote)
            d.quality = self._dev_quality.data_ptr()
        d.reason = ro["reason"][k].data_ptr()
        d.code_in, d.code_out = ro["code_act"].data_ptr(), ro["code"][k].data_ptr()
        d.steps_in, d.steps_out = ro["d_steps"][ro["si"]].data_ptr(), ro["d_steps"][ro["si"] ^ 1].data_ptr()
        d.reward, d.done, d.err_flag, d.nv_out = (ro["rew"][k].data_ptr(), ro["done"][k].data_ptr(), ro["err"].data_ptr(),
                                                  ro["nv"][k].data_ptr())
        d.coords, d.u, d.p, d.x = self._coords_dev.data_ptr(), self.u.data_ptr(), self.p.data_ptr(), x.data_ptr()
        return d

    def _finish_handover(self, d, pairs):
        """The hand-over windows of `mdq_env_finish`: every (destination, source) pair of `_flow_handover` is a window of
        one of the row arrays (a whole row, or - the warm start - the last snapshot of the u / p rows) or, for arrays that
        are not reset in place (the edge numbering), a row array of its own without a source."""
        n = d.n_rows
        index = {int(d.dst[t]): t for t in range(n)}
        for dst, src in pairs:
            if dst.dtype != src.dtype or not dst.is_contiguous() or dst.shape != src.shape or not src[0].is_contiguous():
                raise ValueError("flow hand-over: buffers of different shapes")
            base = src._base if src._base is not None else src
            per = src[0].numel() * src.element_size()
            t = index.get(int(base.data_ptr()))
            if t is None:                              # not one of the restored arrays: hand-over only
                if not src.is_contiguous():
                    raise ValueError("flow hand-over: an array that is not reset must be contiguous")
                t = n
                n += 1
                d.dst[t], d.src[t], d.row_bytes[t] = src.data_ptr(), None, per
                off = 0
            else:
                off = src.data_ptr() - base.data_ptr()
                if off < 0 or off + per > d.row_bytes[t] or (not src.is_contiguous() and src.stride(0) * src.element_size() != d.row_bytes[t]):
                    raise ValueError("flow hand-over: the source is not a window of a row array")
            d.handover_dst[t], d.handover_off[t], d.handover_bytes[t] = dst.data_ptr(), off, per
        d.n_rows = n

    def rollout_end(self, ro):
        """The one read-back of a rollout; the host mirrors of the environments follow the device."""
        K = ro["k"]
        last = self._interp_last
        if K and last is not None and last[1]:
            # the steps of a rollout interpolate only what they read (sparse: most edge-midpoint entries of `self.u` are skipped);
            # `self.u` / `self.p` are public - whoever reads them after the rollout (field dumps, deploy, tests, a host-driven
            # step()) finds the COMPLETE fields of the last step's meshes: one full pass here, once per rollout (~45 us)
            d = last[0]
            d.sparse = 0
            _lib.check(self.lib.mdq_interpolate_snapshots(C.byref(d), _lib.stream_ptr()), "mdq_interpolate_snapshots")
            self._interp_last = (d, 0, last[2])
        # ONE read-back: the per-step outputs + every small host mirror as one packed buffer (a dozen device-to-host copies, each
        # a synchronisation of its own, were 0.4-0.5 ms per rollout: round 4's `rollout_end` was 0.7-0.95 ms - 5 % of the
        # driver's 20-step rollouts), the meshes (4 MB per 128 environments) into their page-locked mirrors in front of it
        dev, dt, h = self.device, self.dtopo, self.h
        main = torch.cuda.current_stream(dev)
        pin = self.topo.pinned
        # (on the MAIN stream: the side stream of the host-driven step() - a plain pool stream - cost the S3 rollouts of a process
        #  40 % once it had been used here, 0.73 -> 1.04-1.10 ms per step in bench.py: the stream -> hardware-queue lottery of
        #  HISTORY 5 "Streams"; the copies run behind the last step's kernels either way)
        pin["coords"].copy_(dt.coords, non_blocking=True)
        pin["cells"].copy_(dt.cells, non_blocking=True)
        parts = [("rewards", ro["rew"][:K]), ("dones", ro["done"][:K]), ("actions", ro["act"][:K]), ("codes", ro["code"][:K]),
                 ("nv_steps", ro["nv"][:K]), ("reasons", ro["reason"][:K]), ("err", ro["err"]), ("nv", dt.nv), ("nt", dt.nt),
                 ("offset", dt.offset), ("steps", ro["d_steps"][ro["si"]]), ("drag", self._dev_drag), ("lift", self._dev_lift)]
        parts += [(k, dt.t[k]) for k in ("nsel", "nedges", "ne", "coord_map", "n_closest")]
        if self.quality.on:
            parts += [("quality", ro["quality"][:K]), ("qinfo", ro["qinfo"][:K])]
        if self.flow_steps > 0:
            parts.append(("flow_status", self.flow_status))        # (legs up to the previous step: the last one may still run)
            if self.flow.map_status is not None:
                parts.append(("flow_map_status", self.flow.map_status))
        flat = [t.contiguous().view(torch.uint8).reshape(-1) for _, t in parts]
        pad = [(-f.numel()) % 8 for f in flat]                  # (every part starts 8-byte aligned in the packed buffer)
        packed = torch.cat([x for f, p_ in zip(flat, pad) for x in ((f, f.new_zeros(p_)) if p_ else (f,))])
        host = self._rollout_host
        if host is None or host.numel() < packed.numel():
            host = self._rollout_host = torch.empty(max(packed.numel(), 1 << 16), dtype=torch.uint8, pin_memory=True)
        host[:packed.numel()].copy_(packed, non_blocking=True)
        self._packed_ev.record(main)
        self._packed_ev.synchronize()
        buf, off, got = host.numpy(), 0, {}
        for (name, t), f, p_ in zip(parts, flat, pad):
            np_dt = {torch.float64: np.float64, torch.int32: np.int32, torch.uint8: np.uint8, torch.int64: np.int64}[t.dtype]
            got[name] = buf[off:off + f.numel()].view(np_dt).reshape(tuple(t.shape)).copy()
            off += f.numel() + p_
        out = dict(rewards=got["rewards"], dones=got["dones"].astype(bool), actions=got["actions"], codes=got["codes"],
                   nv=got["nv_steps"], reasons=got["reasons"])
        if self.quality.on:     # (K, B, 2): q_min, cot_max of every step's meshes, before any reset
            out["quality"] = got["quality"]
            if K:
                self.mesh_quality, self.quality_cell = got["quality"][-1].copy(), got["qinfo"][-1][:, 0].copy()
        if int(got["err"][0]) != 0:
            raise _lib.MeshDQNHipError("topology kernel failed inside rollout_device")
        if K:               # a failed flow leg is an ERROR here, not a NaN in what the caller reads later
            check_flow_forces(got["drag"], got["lift"], "rollout_device", got.get("flow_status"), got.get("flow_map_status"))
        self.nv[...], self.nt[...], self.offset[...], self.steps[...] = got["nv"], got["nt"], got["offset"], got["steps"]
        for k in ("nsel", "nedges", "ne", "coord_map", "n_closest"):
            h[k][...] = got[k]
        self.new_drags, self.new_lifts = got["drag"], got["lift"]
        last_done = out["dones"][-1] if K and self.auto_reset else None
        if last_done is not None and last_done.any():      # (restarted environments: the cached initial forces, like step())
            self.new_drags[last_done] = self._cached(self._init_cache["drags"], last_done)
            self.new_lifts[last_done] = self._cached(self._init_cache["lifts"], last_done)
            self.mesh_quality[last_done] = self._cached(self._init_cache["quality"], last_done)
            self.quality_cell[last_done] = self._cached(self._init_cache["quality_cell"], last_done)
            # ... and their interpolated snapshots: `mdq_env_finish` leaves them alone inside a rollout (every step
            # interpolates again before anything reads them); whoever reads the state after the LAST step - get_state(), a
            # host-driven step() - must find the initial fields in the rows of the environments that step reset
            c = self._init_cache
            ti = torch.from_numpy(np.flatnonzero(last_done).astype(np.int32)).to(self.device)
            dst = (C.c_void_p * 2)(self.u.data_ptr(), self.p.data_ptr())
            src = (C.c_void_p * 2)(c["u"].data_ptr(), c["p"].data_ptr())
            nb = (C.c_int64 * 2)(self.u[0].numel() * 8, self.p[0].numel() * 8)
            self._restore_rows(dict(n=2, dst=dst, src=src, nbytes=nb, stride=(C.c_int64 * 2)(nb[0], nb[1])), int(ti.numel()), ti)
        self._deferred_mirror = None
        return out


class VecEnvGroups:
    """`num_envs` environments as G independent `VecEnv2DAirfoil` groups, each driven by its own Python thread on
    its own HIP stream - the counterpart of the reference's asynchronous Ray workers (`num_parallel`,
    airfoil_dqn.py:428-503) inside one process: while one group waits for its GPU kernels (the smoothing kernel is
    latency-bound and occupies only as many CUs as the group has environments) another group runs its host mesh
    engine calls (ctypes and torch release the GIL).  All groups share one base environment (ground truth,
    snapshots, interpolation grid)."""

    def __init__(self, config, num_envs: int, groups: int = 2, compute_device="cuda", base_env: Env2DAirfoil | None = None, **kw):
        self.device = torch.device(compute_device)
        base = base_env or Env2DAirfoil(config, compute_device=compute_device)
        G = max(1, min(int(groups), int(num_envs)))
        sizes = [num_envs // G + (1 if g < num_envs % G else 0) for g in range(G)]
        self.streams = [torch.cuda.Stream(device=self.device) for _ in range(G)]
        self.envs = []
        for g in range(G):
            with torch.cuda.stream(self.streams[g]):
                self.envs.append(VecEnv2DAirfoil(config, sizes[g], compute_device=compute_device, base_env=base, **kw))
        torch.cuda.synchronize(self.device)
        self.B = int(num_envs)

    def rollout(self, act_fn, steps: int, barrier=None):
        """Every group runs `steps` batched steps concurrently: state -> act_fn(group, env, state) -> env.step.
        Returns the list of per-group (rewards, dones) of the last step.  Exceptions of the workers are re-raised."""
        import threading
        out, errs = [None] * len(self.envs), []

        def work(g):
            try:
                env = self.envs[g]
                with torch.cuda.stream(self.streams[g]):
                    st = env.get_state()
                    for _ in range(steps):
                        st, rew, done, info = env.step(act_fn(g, env, st))
                    self.streams[g].synchronize()
                    out[g] = (rew, done)
            except BaseException as exc:  # noqa: BLE001 - surfaced to the caller below
                errs.append(exc)

        threads = [threading.Thread(target=work, args=(g,)) for g in range(len(self.envs))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errs:
            raise errs[0]
        return out

    def rollout_device(self, fused, steps: int, explore, rand_actions):
        """Every group runs `VecEnv2DAirfoil.rollout_device` (no host round trip inside a step) on its own stream:
        fused[g] / explore[g] / rand_actions[g] per group.  Returns the per-group result dicts."""
        import threading
        out, errs = [None] * len(self.envs), []

        def work(g):
            try:
                with torch.cuda.stream(self.streams[g]):
                    out[g] = self.envs[g].rollout_device(fused[g], steps, explore[g], rand_actions[g])
                    self.streams[g].synchronize()
            except BaseException as exc:  # noqa: BLE001 - surfaced to the caller below
                errs.append(exc)

        if len(self.envs) == 1:
            work(0)
        else:
            threads = [threading.Thread(target=work, args=(g,)) for g in range(len(self.envs))]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
        if errs:
            raise errs[0]
        return out
