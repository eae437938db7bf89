"""`FlowSolver` - the reference's surface (flow_solver.py:47-396) on the MI355X IPCS kernels.

Same constructor signature, attributes and methods as the reference class:

    solver = FlowSolver(flow_params, geometry_params, solver_params)
    u_, p_, drag, lift = solver.evolve()
    solver.remesh(mesh); solver.deploy(); solver.mark_boundaries()
    solver.mesh, .removable, .drag_probe, .lift_probe, .num_vertices,
    .accumulated_drag, .accumulated_lift, .gtime, .dt

DOLFIN objects are replaced by light device-backed stand-ins (`Mesh`, `Function`)
that expose the handful of methods the reference's callers use
(`coordinates()`, `cells()`, `vector().get_local()/set_local()`, `copy(deepcopy=True)`).
All arithmetic runs in `libmeshdqn_hip.so` (no CPU fallback).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .inflow import inflow_spec
from .io_xdmf import load_mesh
from .ipcs_batch import IpcsBatch, smooth_coords
from .probes import DragProbe, LiftProbe
from .topology import MeshTopology


class Mesh:
    """Minimal stand-in for `dolfin.Mesh` (vertex coordinates + ordered triangle cells)."""

    def __init__(self, coords, cells=None):
        if isinstance(coords, Mesh):  # copy constructor: Mesh(other)
            self.topology_ = MeshTopology(coords.coordinates().copy(), coords.cells().copy())
        else:
            self.topology_ = MeshTopology(coords, cells)

    def coordinates(self) -> np.ndarray:
        return self.topology_.coords

    def cells(self) -> np.ndarray:
        return self.topology_.cells

    def num_vertices(self) -> int:
        return self.topology_.nv

    def num_cells(self) -> int:
        return self.topology_.nt

    def smooth(self, iterations: int = 50):
        """DOLFIN `Mesh.smooth` (in place)."""
        self.topology_.coords[:] = smooth_coords(self.topology_, iterations)


class _Vector:
    def __init__(self, fn):
        self._fn = fn

    def get_local(self) -> np.ndarray:
        return self._fn.data.detach().cpu().numpy().reshape(-1).copy()

    def set_local(self, values):
        v = torch.as_tensor(np.asarray(values, dtype=np.float64).reshape(self._fn.data.shape))
        self._fn.data.copy_(v.to(self._fn.data.device))


class Function:
    """Stand-in for a `dolfin.Function` on P2^2 (velocity, data (np2,2)) or P1 (pressure, data (nv,))."""

    def __init__(self, topo: MeshTopology, data: torch.Tensor, kind: str):
        self.topo, self.data, self.kind = topo, data, kind
        self.name = kind

    def vector(self) -> _Vector:
        return _Vector(self)

    def copy(self, deepcopy: bool = True) -> "Function":
        return Function(self.topo, self.data.clone() if deepcopy else self.data, self.kind)

    def rename(self, name, label):
        self.name = name

    def set_allow_extrapolation(self, flag: bool):
        pass  # evaluation always extrapolates, bin-locally (see interpolate_kernel in csrc/mdq_mesh.hip)

    def vertex_values(self) -> np.ndarray:
        """Values at the mesh vertices = the vertex dofs (P2 vertex dofs come first)."""
        nv = self.topo.nv
        return self.data[:nv].detach().cpu().numpy().copy()


class FlowSolver(object):
    """IPCS scheme with explicit treatment of nonlinearity (flow_solver.py:47-48)."""

    def __init__(self, flow_params, geometry_params, solver_params, device="cuda"):
        self.mu = float(flow_params["mu"])
        self.rho = float(flow_params["rho"])
        self.viscosity, self.density = self.mu, self.rho
        self.DEPLOY = False
        self.device = torch.device(device)
        # flow_solver.py:70-73: 'constant' = the time independent parabola, anything else = the caller's own profile.  The
        # reference takes a dolfin Expression with a `time` attribute; here: a callable profile(x, y, t) -> x-velocity
        # at the inlet dof coordinates (every boundary condition of the reference has zero y-velocity) - or a schedule dict
        # (inflow.py: a(t) * the constant parabola, applied inside the evolve kernels: K steps per launch like 'constant').
        # A callable runs K steps per call as well where the operator mode launches per step (modes 2 / 3: the batch gets it
        # as `inflow_profile`, evaluated for all K steps up front); in the other modes it is stepped one launch at a time
        inflow = flow_params.get("inflow", "constant")
        self.inflow_profile = inflow if callable(inflow) else None
        self.inflow_spec = None if callable(inflow) else inflow_spec(inflow)    # (TypeError / ValueError before any device work)
        coords, cells = load_mesh(geometry_params["mesh"])
        self.mesh = Mesh(coords, cells)
        self.smooth = solver_params.get("smooth", False)
        if self.smooth:
            self.mesh.smooth(50)
        self.dt_value = float(solver_params["dt"])
        # `solver_type` of the yaml is ignored by the reference (it reads 'la_solve', flow_solver.py:147)
        self.solver_type = solver_params.get("la_solve", "lu")
        assert self.solver_type in ("lu", "la_solve")
        # Krylov tolerance of the velocity / correction solves (and of the pressure solve where no factorisation is in use).
        # The reference's 'lu' solves are exact to round-off; measured over 5000 steps from rest on both lab meshes
        # (tools/traj_determinism.py): at rtol 1e-10 drag / lift sit 1e-8 .. 1.3e-6 from the exact-LU trajectory in EVERY
        # operator mode (the stopping test, not the summation order), at 1e-13 within 7e-10 - so 'lu' defaults to 1e-13
        # (velocity 9.6 -> 14.5, correction 6.9 -> 14 iterations per step), the Krylov option keeps 1e-10
        self.rtol = float(solver_params.get("rtol", 1e-13 if self.solver_type == "lu" else 1e-10))
        # reproducible (default): the bitwise-reproducible operator mode 2 (element results through an LDS tile, summed by
        # the row owners in fixed order) for everything this class is used for - ground truths, run_sim, re-simulations:
        # thousands of steps whose result must not depend on the run or on the batch a mesh is simulated in.  False: mode 3
        # (LDS fp64 atomics, 3x faster, reproducible to the solver tolerance only), what the one-step flow leg of the
        # batched env step uses (vec_env.py)
        self.reproducible = bool(solver_params.get("reproducible", True))
        self.mode = -2 if self.reproducible else -1     # (-2: the fastest reproducible variant that fits the mesh)
        self._setup(reassemble=True)
        self.gtime = 0.0

    # `dt` is a dolfin Constant in the reference; callers use `self.dt(0)`
    def dt(self, _=0):
        return self.dt_value

    # ------------------------------------------------------------------
    def _setup(self, reassemble: bool):
        topo = self.mesh.topology_
        self.removable = list(topo.removable())
        self.bnd_tags = topo.facet_tags()
        n2, nv = topo.np2, topo.nv
        self._light = None
        if reassemble:
            self.batch = IpcsBatch([topo], [topo.coords], mu=self.mu, rho=self.rho, dt=self.dt_value,
                                   rtol=self.rtol, device=self.device, mode=self.mode,
                                   pressure_direct=("device" if self.solver_type == "lu" else False),
                                   inflow=self.inflow_spec,     # (a new batch starts its schedule's clock at 0, as gtime does)
                                   inflow_profile=(self.inflow_profile if IpcsBatch.mode_serves_profile(self.mode, n2) else None))
            self.batch.assemble()
            # solver_type 'lu' = device factorisation of the pressure matrix; a mesh beyond its limits (1024 vertices, 112
            # interior / separator nodes per part) keeps the Jacobi-CG pressure solve (rtol-limited instead of exact): say so
            # once per mesh (remesh is not on the hot path)
            st = getattr(self.batch, "pd_status", None)
            if self.solver_type == "lu" and st is not None and int(st.min().item()) < 0:
                import warnings
                warnings.warn(f"FlowSolver: mesh with {nv} vertices exceeds the limits of the device pressure factorisation "
                              f"(status {int(st.min().item())}); the pressure solve falls back to Jacobi-CG at rtol {self.rtol:g}",
                              RuntimeWarning, stacklevel=2)
            self.u_n = Function(topo, self.batch.u_n[0, :n2], "velocity")
            self.p_n = Function(topo, self.batch.p_n[0, :nv], "pressure")
        else:
            # training mode (DEPLOY False): the reference builds new spaces / zero functions / probes but
            # does NOT re-assemble or re-factorise (flow_solver.py:268 `if(self.DEPLOY)`)
            self.batch = None
            self.u_n = Function(topo, torch.zeros((n2, 2), dtype=torch.float64, device=self.device), "velocity")
            self.p_n = Function(topo, torch.zeros((nv,), dtype=torch.float64, device=self.device), "pressure")
        self.u_, self.p_ = self.u_n, self.p_n
        self.drag_probe = DragProbe(self.viscosity, None, self, tags=[1])
        self.lift_probe = LiftProbe(self.viscosity, None, self, tags=[1])
        self.accumulated_drag, self.accumulated_lift = [], []
        self.num_vertices = nv

    def probe_batch(self):
        """Device mesh data for the force probes on the current mesh."""
        if self.batch is not None:
            return self.batch
        if self._light is None:
            from .mesh_ops import LightMeshBatch
            topo = self.mesh.topology_
            self._light = LightMeshBatch([topo], [topo.coords], self.mu, device=self.device)
        return self._light

    def mark_boundaries(self):
        """Tags of the exterior facets: 0 walls / 1 airfoil / 2 inflow / 3 outflow / 4 other
        (flow_solver.py:194-226).  Returns (edge ids, tags)."""
        topo = self.mesh.topology_
        return topo.boundary_edges, topo.facet_tags()

    def deploy(self):
        self.DEPLOY = True

    _MESH_STATE = ("mesh", "removable", "bnd_tags", "_light", "batch", "u_n", "p_n", "u_", "p_", "drag_probe", "lift_probe",
                   "accumulated_drag", "accumulated_lift", "num_vertices", "gtime")

    def snapshot(self) -> dict:
        """Everything `remesh` replaces (the caller can go back to the old mesh when the new one turns out unusable)."""
        return {k: getattr(self, k) for k in self._MESH_STATE}

    def restore(self, snap: dict):
        for k, v in snap.items():
            setattr(self, k, v)

    def remesh(self, mesh: Mesh):
        """flow_solver.py:233-359: swap the mesh, smooth again, recompute `removable`, new spaces /
        functions / probes; operators are re-assembled (and the clock reset) only in DEPLOY mode."""
        self.mesh = mesh
        if self.smooth:
            self.mesh.smooth(50)
        self._setup(reassemble=self.DEPLOY)
        if self.DEPLOY:
            self.gtime = 0.0

    def evolve(self, nsteps: int = 1):
        """One IPCS time step (flow_solver.py:362-396); returns (u_, p_, drag, lift).
        `nsteps > 1` runs several steps in one kernel launch and returns the last values."""
        if self.batch is None:
            raise RuntimeError("operators are only (re-)assembled in DEPLOY mode after remesh (flow_solver.py:268)")
        if self.inflow_profile is None:     # constant parabola or a schedule (the batch applies its factors): one launch
            drag, lift = self.batch.evolve(nsteps)
            self.gtime += self.dt_value * nsteps
            d = drag[0].tolist()
            l = lift[0].tolist()
        elif self.batch.inflow_profile is not None:
            # time dependent inflow (flow_solver.py:366-371) in the per-step operator modes: the profile evaluated at the
            # instants this clock takes (accumulated step by step, as the loop below does), one call, one read-back
            times = []
            for _ in range(nsteps):
                self.gtime += self.dt_value
                times.append(self.gtime)
            drag, lift = self.batch.evolve(nsteps, inflow_times=np.array(times, np.float64))
            d = drag[0].tolist()
            l = lift[0].tolist()
        else:
            # the modes that loop over the steps inside one kernel: the clock advances, the profile is evaluated at the new
            # time, then the step runs with those boundary values - one launch per step
            d, l = [], []
            for _ in range(nsteps):
                self.gtime += self.dt_value
                self.batch.update_inflow(self.inflow_profile, self.gtime)
                dr, li = self.batch.evolve(1)
                d.append(dr[0, 0].item())
                l.append(li[0, 0].item())
        if d[-1] != d[-1] or l[-1] != l[-1]:       # NaN: the kernels' report of a step they could not take (already synchronised)
            self.batch.check()
            raise _lib.MeshDQNHipError("IPCS step returned non-finite drag / lift (diverged solve)")
        self.accumulated_drag.extend(d)
        self.accumulated_lift.extend(l)
        return self.u_, self.p_, d[-1], l[-1]
