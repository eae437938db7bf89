"""`FlowLeg` - the S3 flow leg of `VecEnv2DAirfoil`: `steps` IPCS steps on every coarsened mesh, warm-started from the
interpolated last snapshot, run in line on the environment's stream or - overlap mode - on a second stream beside the next
env step's mesh kernels.  The class owns the leg's descriptor, arrays, streams and events and decides alone which input
set is free, what the flow stream waits for and which result slot holds which leg; the environment calls its verbs."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from .ipcs_batch import MF_ROWS, MODE3_MAX_N2, WG, IpcsBatch, operator_mode_limits, pd_device_tables
from .mesh_ops import HostTopologyBatch
from .streams import role_streams


class FlowLeg:
    NRL = 4032         # row capacity of a chunk's list in the device-built tile maps (the kernels' LDS stage holds 4064 rows)

    def __init__(self, device, topo, solver, steps: int, rtol: float, pressure: str = "cg", pcg_degree: int = 0, ftopo=None,
                 env_phys=None, inflow_scale=None, inflow_profile=None):
        """`topo`: the environment's topology engine (host or device); `solver`: mu / rho / dt_value of the flow;
        `ftopo`: the flow stream's own `DeviceTopologyBatch` (flow_only, with the IPCS index data) = overlap mode;
        `env_phys`: device float64 (B, 4) rows mu, rho, dt, 0 - the flow constants per environment (validated by the
        caller, `ipcs_batch.flow_table`; `solver` then carries row 0 for the descriptor's scalars, which are only
        validated) - or None; `inflow_scale`: device float64 (B, steps) inflow factors of the leg's steps (built once by the
        caller, `inflow.inflow_factors`: the leg always restarts from the last snapshot, so the table is static) - or None,
        the constant parabola; `inflow_profile`: dict(n_ref int32 (B,), inlet_y float64 (B, NIN), values float64
        (B, steps, NIN)) of device tensors - a non-separable inflow at every environment's canonical inlet
        (`inflow.leg_profile_table`, static for the same reason); the leg maps the inlet points to the dofs of every new mesh
        on the device (`mdq_ipcs_build_inlet_map`) - or None.  Not both."""
        self.lib, self.device, self.steps, self.pressure = _lib.load(), device, int(steps), pressure
        self.topo, self.ftopo = topo, ftopo
        tp = ftopo if ftopo is not None else topo           # the engine whose index data the descriptor reads
        self.host_index = isinstance(tp, HostTopologyBatch)
        self.B = B = tp.B
        dev, NV, NT, NE, NP = device, tp.NV, tp.NT, tp.NE, tp.NP

        def z(*shape):
            return torch.zeros(shape, dtype=torch.float64, device=dev)

        own = dict(geom=z(B, 5, NT), bo_val=z(B, tp.NBE, 4), lift1=z(B, NP, 2), lift3=z(B, NP, 2), idiag1=z(B, NP, 2),
                   sdiagM=z(B, NP), sdiagK=z(B, NV), K1s=z(B, tp.NSE1), u_n=z(B, NP, 2), p_n=z(B, NV))
        nwork = int(self.lib.mdq_ipcs_workspace_doubles(B, NV, NT, NE))
        own["work"] = z(nwork)
        if self.host_index:
            t = {k: torch.from_numpy(a).to(dev) for k, a in tp.hi.items()}
        else:                   # the device engine's outputs ARE the descriptor's index arrays
            t = dict(tp.ti)
        t.update(own)
        d = _lib.IpcsDesc()
        d.B, d.NV, d.NT, d.NE, d.N2, d.NAF = B, NV, NT, NE, NP, tp.NAF
        d.NSE1, d.NBO, d.NBE = tp.NSE1, tp.NBO, tp.NBE
        d.mu, d.rho, d.dt, d.rtol = solver.mu, solver.rho, solver.dt_value, float(rtol)
        d.maxit_u, d.maxit_p, d.maxit_m = 200, 4000, 200
        # mode 3 (LDS-resident vectors) on the lab meshes; a capacity beyond its limits (`operator_mode_limits`: 3 402 rows; the
        # red-refined meshes): auto, which for this descriptor - no assembled operators, no tile pointers - is the element tiles
        # with global vectors (modes 5 / 7, here through the dof <- slot lists of the topology engine or the maps built below)
        self.mode3 = bool(operator_mode_limits(NP, NV, tp.NSE1)["mode3"])
        d.mode, d.pd_enabled = (3 if self.mode3 else -1), 0
        d.pcg_degree = int(pcg_degree)
        for name, _typ in _lib.IpcsDesc._fields_:
            if name in t:
                setattr(d, name, t[name].data_ptr())
        d.work_doubles = nwork
        self.env_phys = env_phys
        if env_phys is not None:
            if env_phys.shape != (B, 4) or env_phys.dtype != torch.float64 or not env_phys.is_contiguous() or env_phys.device.type != "cuda":
                raise ValueError(f"env_phys: a contiguous float64 device tensor of shape ({B}, 4)")
            d.env_phys = env_phys.data_ptr()
        self.inflow_scale = inflow_scale
        if inflow_scale is not None and (inflow_scale.shape != (B, self.steps) or inflow_scale.dtype != torch.float64 or
                                         not inflow_scale.is_contiguous() or inflow_scale.device.type != "cuda"):
            raise ValueError(f"inflow_scale: a contiguous float64 device tensor of shape ({B}, {self.steps})")
        # a non-separable inflow: the static tables of the caller, the map of every leg's mesh (owned here, rebuilt by every
        # leg: NIR = NP cannot overflow, and inflow_lift_kernel loops over n_rows only) and the record the evolve call reads
        self.inflow_profile = inflow_profile
        self.map_status = self._prof = None
        if inflow_profile is not None:
            check_leg_profile(inflow_profile, inflow_scale, B, self.steps, NP)
            NIN = int(inflow_profile["inlet_y"].shape[1])

            def zi(*shape):
                return torch.zeros(shape, dtype=torch.int32, device=dev)

            self.inlet_map = dict(n_inlet=zi(B), inlet_dofs=zi(B, NIN), n_rows=zi(B), rows=zi(B, NP))
            # sticky like `status`: the first failure of an environment's map (codes: MAP_STATUS), read with it
            self.map_status = zi(B)
            pr = self._prof = _lib.InflowProfile()
            pr.NIN, pr.NIR = NIN, NP
            for kk, a in self.inlet_map.items():
                setattr(pr, kk, a.data_ptr())
            pr.values = inflow_profile["values"].data_ptr()
        # meshes beyond the topology engine's small-mesh instance (MF_ROWS * WG = 3 584 rows; auto: the element tiles, modes 5 / 7;
        # a capacity between mode 3's limit and that one runs them through the slot lists): the tile maps of every coarsened mesh are
        # built on the device in front of the IPCS step (mdq_ipcs_build_tile_maps: row lists + packed local maps) - without
        # them the element results of every operator application go through 0.6 MB of global scratch per environment
        # (MDQ_NO_DEVICE_TILE_MAPS=1: that path, A / B switch)
        self.tile_maps = False
        if NP > MF_ROWS * WG and not self.host_index and os.environ.get("MDQ_NO_DEVICE_TILE_MAPS", "") != "1":
            nch = (NT + 1023) // 1024
            nrl = min(self.NRL, NP)
            if (nch + 4) * ((NP + 15) & ~15) + 256 <= 160 * 1024:
                t["mf_rlist"] = torch.zeros((B, nch, nrl, 2), dtype=torch.int32, device=dev)
                t["mf_rcnt"] = torch.zeros((B, nch), dtype=torch.int32, device=dev)
                t["mf_lpos"] = torch.zeros((B, 6, NT), dtype=torch.int32, device=dev)
                for k in ("mf_rlist", "mf_rcnt", "mf_lpos"):
                    setattr(d, k, t[k].data_ptr())
                d.NRL, d.rl_flags = nrl, 1
                d.mf_scat = d.mf_tptr = None
                self.tile_maps = True
        self.t, self.desc = t, d
        self.pd_status = None
        if pressure == "direct":      # outputs of mdq_ipcs_factorize_pressure (capacities: its limits)
            t.update(pd_device_tables(d, B, NV, dev, IpcsBatch.PD_DEVICE_CAP))
            d.pd_enabled = 1
            self.pd_status = torch.zeros(B, dtype=torch.int32, device=dev)
        self.iters = torch.zeros((B, 3), dtype=torch.int32, device=dev)
        # sticky status words of the flow legs (mdq_ipcs_desc.status, ABI 7): a leg that gave up - team barrier time-out of the
        # two-workgroup operator modes - is an ERROR at the next read-back (rollout_end / flow_wait), not a silent NaN
        self.status = torch.zeros(B, dtype=torch.int32, device=dev)
        d.status = self.status.data_ptr()
        self.events = None      # (tools: a list here collects HIP event pairs around every overlapped leg, on the flow stream)
        self._keep = None       # device buffers the descriptor points at
        self._n = 0             # legs started
        self._last = None       # result slot of the leg started last; `_reported`: the one `results(previous=True)` reads next
        self._reported = None
        self._armed = None      # the input set the main topology run of this step fills
        self.stream = self._ready = self._mesh_ready = self._res = self._in = None
        if ftopo is None:
            return
        self.stream = role_streams(dev)["flow"]   # (the process's flow stream: fixed creation order, one probe)
        self._ready, self._mesh_ready = torch.cuda.Event(), torch.cuda.Event()
        # page-locked result buffers (two: the results of step k are read while step k + 1 is in flight) + events; the last
        # IPCS kernel writes drag / lift of the leg straight into them (2 KB over the bus) instead of two device-to-host
        # copies behind it (12 us of the flow chain)
        self._res = [dict(host=torch.zeros((2, B, self.steps), dtype=torch.float64, pin_memory=True),
                          done=torch.cuda.Event()) for _ in range(2)]
        # TWO sets of the flow engine's inputs (private meshes + start fields): the main stream fills set k % 2 for
        # flow k while flow k - 1 still reads the other one.  With one set the hand-over was a serial chain - flow
        # k - 1 ends -> main copies -> flow k starts, two event round trips + the copy per step on the flow's
        # critical path - and the S3 step lasted (flow leg + ~70 us) instead of max(main chain, flow leg).
        self._in = [dict(coords=ftopo.coords, cells=ftopo.cells, nv=ftopo.nv, nt=ftopo.nt, u_n=t["u_n"], p_n=t["p_n"],
                         # the main engine's cell dofs / edge counts of the same meshes: the flow's topology run takes
                         # its edge numbering from them (no second hash pass)
                         cell_dofs=torch.zeros_like(topo.t["cell_dofs"]), ne=torch.zeros_like(topo.t["ne"]))]
        self._in.append({k: torch.zeros_like(a) for k, a in self._in[0].items()})

    # ------------------------------------------------------------------ one leg
    def _launch(self, keep, out, before_evolve=None):
        """Operator set-up on the meshes the descriptor points at, then the IPCS steps; `out` = (drag, lift) tensors the
        kernels write (page-locked host tensors are written over the bus directly)."""
        d = self.desc
        _lib.check(self.lib.mdq_ipcs_setup_matfree(C.byref(d), _lib.stream_ptr()), "mdq_ipcs_setup_matfree")
        if self.tile_maps:
            _lib.check(self.lib.mdq_ipcs_build_tile_maps(C.byref(d), None, _lib.stream_ptr()), "mdq_ipcs_build_tile_maps")
        if self.pressure == "direct":
            _lib.check(self.lib.mdq_ipcs_factorize_pressure(C.byref(d), self.pd_status.data_ptr(), _lib.stream_ptr()),
                       "mdq_ipcs_factorize_pressure")
        pr = self._prof
        if pr is not None:                  # which dof of THIS mesh is which inlet point (reads the mesh + the fresh bcu_gx only)
            ip, m = self.inflow_profile, self.inlet_map
            _lib.check(self.lib.mdq_ipcs_build_inlet_map(C.byref(d), pr.NIN, pr.NIR, ip["n_ref"].data_ptr(), ip["inlet_y"].data_ptr(),
                                                         m["n_inlet"].data_ptr(), m["inlet_dofs"].data_ptr(), m["n_rows"].data_ptr(),
                                                         m["rows"].data_ptr(), self.map_status.data_ptr(), _lib.stream_ptr()),
                       "mdq_ipcs_build_inlet_map")
        if before_evolve is not None:       # (the set-up above reads the mesh only; the warm start is needed from here on)
            before_evolve()
        # a new mesh: no initial-guess history, iteration counters from zero - mode 3 takes both inside the kernels of its
        # first step (no reset launch on the flow chain), the other modes launch the reset kernel themselves
        if pr is not None:
            _lib.check(self.lib.mdq_ipcs_evolve_fresh_profile(C.byref(d), self.steps, out[0].data_ptr(), out[1].data_ptr(),
                                                              self.iters.data_ptr(), C.byref(pr), _lib.stream_ptr()),
                       "mdq_ipcs_evolve_fresh_profile")
            self._keep = keep
            return out
        _lib.check(self.lib.mdq_ipcs_evolve_fresh(C.byref(d), self.steps, out[0].data_ptr(), out[1].data_ptr(),
                                                  self.iters.data_ptr(),
                                                  None if self.inflow_scale is None else self.inflow_scale.data_ptr(),
                                                  _lib.stream_ptr()), "mdq_ipcs_evolve_fresh")
        self._keep = keep
        return out

    def run_inline(self, keep, u0, p0):
        """The leg on the current stream, on the meshes of `keep` (the main engine's arrays), warm-started from u0 / p0;
        returns (drag, lift) device tensors (B, steps)."""
        t, d = self.t, self.desc
        if self.host_index:
            for kk in self.topo.hi:
                t[kk].copy_(self.topo.pinned[kk], non_blocking=True)
        for kk in ("coords", "cell_dofs", "af_facets", "nv", "nt", "ne", "naf"):
            setattr(d, kk, keep[kk].data_ptr())
        t["u_n"].copy_(u0)
        t["p_n"].copy_(p0)
        drag = torch.empty((self.B, self.steps), dtype=torch.float64, device=self.device)
        return self._launch(keep, (drag, torch.empty_like(drag)))

    # ------------------------------------------------------------------ overlap mode: hand-over, start, results
    def _free_input(self):
        """The input set leg k = `_n` will read (filled alternately: leg k - 1 may still be reading the other one)."""
        if self._n >= 2 and self._last is not None:          # leg k - 2 read this input set (long finished)
            torch.cuda.current_stream(self.device).wait_event(self._res[self._n % 2]["done"])
        return self._in[self._n % 2]

    def arm_handover(self):
        """Before the main topology run of a device-resident step: the free input set becomes the second output set of the
        topology kernel (meshes + edge numbering written by that launch itself: no copy launch on the main chain, 6 us + two
        event gaps per step)."""
        fin = self._armed = self._free_input()
        self.topo.set_handover(fin["coords"], fin["cells"], fin["nv"], fin["nt"], fin["cell_dofs"], fin["ne"])

    def mesh_ready(self):
        """Right after that run: the flow stream can derive its own topology and the operator set-up while the main
        stream still interpolates / evaluates the step - handing everything over inside `mdq_env_finish` left the flow stream
        idle for ~60 us of every step (profiles/r04_timeline_s3_step.txt)."""
        self.topo.set_handover()                 # (that launch only: a later host-driven step() must not write there)
        self._mesh_ready.record(torch.cuda.current_stream(self.device))

    def warm_start_pairs(self, u0, p0):
        """The (destination, source) pairs `mdq_env_finish` copies for the armed leg: its warm start (last interpolated
        snapshot), taken BEFORE an in-place reset of a terminated environment rewrites it."""
        return [(self._armed["u_n"], u0), (self._armed["p_n"], p0)]

    def start(self):
        """After `mdq_env_finish` is enqueued on the main stream: the armed leg on the flow stream."""
        self._start(self._armed, mesh_early=True)

    def start_from_copies(self, u0, p0):
        """Host-driven `step()`: meshes, the main engine's edge numbering and the warm start are copied to the free input
        set on the main stream (ONE launch: six torch copies were ~50 us of the main chain), then the leg is started."""
        dt, fin = self.topo, self._free_input()
        pairs = [(fin["coords"], dt.coords), (fin["cells"], dt.cells), (fin["nv"], dt.nv), (fin["nt"], dt.nt), (fin["u_n"], u0),
                 (fin["p_n"], p0), (fin["cell_dofs"], dt.t["cell_dofs"]), (fin["ne"], dt.t["ne"])]
        n = len(pairs)
        vp, i64 = C.c_void_p * n, C.c_int64 * n
        rows, rb, ss, ds = [], [], [], []
        for dst, src in pairs:
            if dst.shape != src.shape or dst.dtype != src.dtype or not dst.is_contiguous():
                raise ValueError("flow hand-over: buffers of different shapes")
            if src.is_contiguous():
                rows.append(1); rb.append(src.numel() * src.element_size()); ss.append(rb[-1]); ds.append(rb[-1])
            else:                                   # a snapshot slice: contiguous per environment
                per = src[0].numel() * src.element_size()
                if not src[0].is_contiguous():
                    raise ValueError("flow hand-over: rows of the source must be contiguous")
                rows.append(src.shape[0]); rb.append(per); ss.append(src.stride(0) * src.element_size()); ds.append(per)
        _lib.check(self.lib.mdq_copy_strided(n, vp(*[d_.data_ptr() for d_, _ in pairs]), vp(*[s_.data_ptr() for _, s_ in pairs]),
                                             i64(*rows), i64(*rb), i64(*ss), i64(*ds), _lib.stream_ptr()), "mdq_copy_strided")
        self._start(fin, mesh_early=False)

    def _start(self, fin, mesh_early):
        """The hand-over is enqueued on the main stream - topology (edges from the main engine), matrix-free set-up and the
        IPCS step(s) follow on the flow stream; results land in page-locked memory.  `mesh_early`: the meshes were handed over
        by the main topology run - topology and set-up wait for THAT, only the IPCS step for the rest."""
        ft, t, d = self.ftopo, self.t, self.desc
        self._ready.record(torch.cuda.current_stream(self.device))
        keep = dict(coords=fin["coords"], cell_dofs=ft.t["cell_dofs"], af_facets=ft.t["af_facets"], nv=fin["nv"], nt=fin["nt"],
                    ne=ft.t["ne"], naf=ft.t["naf"], u_n=fin["u_n"], p_n=fin["p_n"])
        for kk, v in keep.items():
            setattr(d, kk, v.data_ptr())
        for kk in ("coords", "cells", "nv", "nt"):            # the flow's topology engine reads the same set
            setattr(ft.desc, kk, fin[kk].data_ptr())
        ft.take_edges_from(fin["cell_dofs"], fin["ne"])
        t["u_n"], t["p_n"] = fin["u_n"], fin["p_n"]
        res = self._res[self._n % 2]
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(self._mesh_ready if mesh_early else self._ready)
            if self.events is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            if self.tile_maps:
                # the private copy's cells in a spatial order (chunks of 1 024 triangles that share their rows: what the tile maps
                # of the IPCS step need), the main engine's cell dofs of the same cells permuted alike
                _lib.check(self.lib.mdq_flow_sort_cells(self.B, d.NV, d.NT, fin["coords"].data_ptr(), fin["nv"].data_ptr(),
                                                        fin["nt"].data_ptr(), fin["cells"].data_ptr(), fin["cell_dofs"].data_ptr(),
                                                        _lib.stream_ptr()), "mdq_flow_sort_cells")
            ft.run(check=False)                  # (same meshes, same deterministic kernel as the main stream's run)
            self._launch(keep, (res["host"][0], res["host"][1]),
                         (lambda: self.stream.wait_event(self._ready)) if mesh_early else None)
            if self.events is not None:
                e1.record()
                self.events.append((e0, e1))
            res["done"].record(self.stream)
        self._last = self._n % 2
        self._n += 1

    def results(self, previous=False):
        """Waits for the leg started last - or, `previous` (what `step_end` reports, one step late), for the one that was
        the last at the previous such call - and returns copies of its (drag, lift); None when there is no such leg."""
        if previous:
            slot, self._reported = self._reported, self._last
        else:
            slot = self._last
        if slot is None:
            return None
        res = self._res[slot]
        res["done"].synchronize()
        fd, fl = res["host"][0].numpy().copy(), res["host"][1].numpy().copy()
        if not previous:        # (the read-back of `step_end` does not check the status words)
            check_flow_forces(fd, fl, "flow_wait", self.status.cpu().numpy(),
                              None if self.map_status is None else self.map_status.cpu().numpy())
        return fd, fl

    def drop_pending(self):
        """Results of a leg started before a reset belong to meshes that no longer exist: the first step after a reset (or a
        stream calibration) reports no "previous step" forces."""
        if self._last is not None:
            self.results()
            self._last = self._reported = None


def profile_leg_refusal(NP: int):
    """None when a flow leg on meshes of capacity NP rows can take an inflow profile, else the reason: the profile is
    rewritten BETWEEN the steps of a launch sequence, which only the leg's mode 3 has (`operator_mode_limits`: NP <= 3402,
    three velocity vectors in LDS; the leg's descriptor has no tile pointers for mode 2) - larger meshes run modes 5 / 7, which
    loop over the steps inside one kernel."""
    if operator_mode_limits(int(NP))["mode3"]:
        return None
    return (f"inflow_profile: a flow leg on meshes of {int(NP)} P2 rows (> {MODE3_MAX_N2}) runs the element-tile operator modes 5 / 7, which "
            "loop over the steps inside one kernel; a non-separable inflow on such meshes is served by the per-step path "
            "(FlowSolver.evolve / IpcsBatch.update_inflow, one step per call)")


def check_leg_profile(inflow_profile, inflow_scale, B: int, steps: int, NP: int):
    """Argument validation of `FlowLeg(inflow_profile=...)` (needs no device: the tensors are only inspected)."""
    if inflow_scale is not None:
        raise ValueError("inflow_profile and inflow_scale are mutually exclusive (a schedule beside a callable goes through the "
                         "profile's table: inflow.leg_profile_table)")
    why = profile_leg_refusal(NP)
    if why is not None:
        raise ValueError(why)
    if not isinstance(inflow_profile, dict) or set(inflow_profile) != {"n_ref", "inlet_y", "values"}:
        raise ValueError("inflow_profile: a dict with the keys n_ref, inlet_y, values")
    y = inflow_profile["inlet_y"]
    NIN = int(y.shape[1]) if getattr(y, "ndim", 0) == 2 else -1
    want = dict(n_ref=((B,), torch.int32), inlet_y=((B, NIN), torch.float64), values=((B, steps, NIN), torch.float64))
    for k, (shape, dtype) in want.items():
        a = inflow_profile[k]
        if (not isinstance(a, torch.Tensor) or NIN < 1 or tuple(a.shape) != shape or a.dtype != dtype or not a.is_contiguous()
                or a.device.type != "cuda"):
            raise ValueError(f"inflow_profile[{k!r}]: a contiguous {str(dtype).replace('torch.', '')} device tensor of shape "
                             f"{shape if NIN >= 1 else '(B, NIN) / (B, steps, NIN)'}")
    if NIN > 64:
        raise ValueError(f"inflow_profile: {NIN} inlet dofs per environment (the device's inlet map holds 64)")


# map_status of the flow leg's inlet map (mdq_ipcs_build_inlet_map)
MAP_STATUS = {1: "the mesh's inlet has another number of dofs than the canonical inlet",
              2: "an inlet dof's y differs from the canonical inlet's",
              3: "more inlet-adjacent rows than the row list holds",
              4: "an inlet-adjacent free row is also a row of an outflow facet (the inflow kernel does not re-apply its correction)"}


def check_flow_forces(drag, lift, where, status=None, map_status=None):
    """Raises when the inlet map of a leg under an inflow profile failed (`map_status`, codes MAP_STATUS: that environment ran
    under the wrong inflow) or when a flow leg reported a step it could not take: a set status word (mdq_ipcs_desc.status: the two-workgroup
    operator modes 4 / 7 abandon a step when a team barrier times out - the partner workgroup was not resident because another
    process or stream held its CU; csrc/mdq_ipcs_team.hip `team_failed`; u_n / p_n of that environment were not advanced) or
    non-finite drag / lift (the same event seen through the forces, or a solve that diverged)."""
    ms = None if map_status is None else np.asarray(map_status)
    if ms is not None and (ms != 0).any():
        which = np.flatnonzero(ms)
        raise _lib.MeshDQNHipError(
            f"{where}: the inlet map of the flow leg's inflow profile failed in environment(s) {which[:8].tolist()}"
            f"{' ...' if which.size > 8 else ''}: " + "; ".join(f"code {c}: {MAP_STATUS.get(c, 'unknown')}" for c in sorted(set(ms[which].tolist()))))
    bad = ~(np.isfinite(drag) & np.isfinite(lift))
    bad = bad.reshape(bad.shape[0], -1).any(1)
    timed_out = np.zeros_like(bad) if status is None else (np.asarray(status) != 0)
    if bad.any() or timed_out.any():
        which = np.flatnonzero(bad | timed_out)
        raise _lib.MeshDQNHipError(
            f"{where}: the flow leg failed in environment(s) {which[:8].tolist()}{' ...' if which.size > 8 else ''}: "
            + ("team barrier time-out of the two-workgroup IPCS modes (is another process or a CU-masked stream holding CUs? "
               "MDQ_NO_TEAM_TILES=1 keeps one workgroup per environment)" if timed_out.any() else "non-finite drag / lift"))
