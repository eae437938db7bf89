"""GPU: non-separable inflow profiles on the device, K steps per call (`IpcsBatch(inflow_profile=...)`,
`mdq_ipcs_evolve_profile`: one small kernel in front of every step of modes 2 / 3 scatters the step's inlet values into
bcu_gx and recomputes lift1 / lift3 on the inlet-adjacent rows).  The two stock meshes ys930 and ah93w145 as one batch (their
inlets differ in size: the padding is exercised), 1 - 8 steps, against a batch that reruns the whole set-up kernel
(`update_inflow`), against the CPU oracle under the same callables, against split calls, the separable special case, a `None`
row, `env_phys`, the refusing modes, `FlowSolver` and the batched deployment.

Profiles on the channel y in [-0.5, 0.5] (two shape terms with different time factors, not a(t) * parabola):
    A(x, y, t) = 6 (0.5 + y)(0.5 - y) (1 + 0.6 y sin(2 pi 125 t)) (0.5 + 100 t)        environment 0
    B(x, y, t) = 6 (0.5 + y)(0.5 - y) (1 + 0.4 y sin(2 pi 50 t))                        environment 1"""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MU, RHO, DT = 1e-3, 1.0, 1e-3
NAMES = ("ys930", "ah93w145")


def profile_a(x, y, t):
    return 6.0 * (0.5 + y) * (0.5 - y) * (1.0 + 0.6 * y * np.sin(2.0 * np.pi * 125.0 * t)) * (0.5 + 100.0 * t)


def profile_b(x, y, t):
    return 6.0 * (0.5 + y) * (0.5 - y) * (1.0 + 0.4 * y * np.sin(2.0 * np.pi * 50.0 * t))


PROFILES = [profile_a, profile_b]


# ---- helper copied from tests/oracle_util.py
def _oracle_vel(u):
    """device [dof][component] -> the oracle's [ux | uy]."""
    return np.concatenate([u[:, 0], u[:, 1]])


@pytest.fixture(scope="module")
def two(meshes, lib_built):
    """The two stock meshes, smoothed as the flow solver smooths them: topologies, coordinates, raw arrays."""
    from meshdqn_amd.ipcs_batch import smooth_coords
    from meshdqn_amd.topology import MeshTopology
    topos = [MeshTopology(*meshes[k]) for k in NAMES]
    return dict(topos=topos, xs=[smooth_coords(t, 50) for t in topos], raw=[meshes[k] for k in NAMES])


def _oracle_steps(raw, profile, n, **kw):
    from oracle.ipcs import OracleFlowSolver
    o = OracleFlowSolver(raw[0], raw[1], inflow=profile, **kw)
    return [tuple(np.copy(v) for v in o.evolve()) for _ in range(n)]


@pytest.fixture(scope="module")
def oracle4(two):
    """Per environment the oracle's first four steps (u, p, drag, lift) under its profile, computed once."""
    return [_oracle_steps(two["raw"][b], PROFILES[b], 4) for b in range(2)]


def _batch(two, **kw):
    from meshdqn_amd.ipcs_batch import IpcsBatch
    kw.setdefault("mu", MU), kw.setdefault("rho", RHO), kw.setdefault("dt", DT)
    kw.setdefault("rtol", 1e-12), kw.setdefault("pressure_direct", False)
    return IpcsBatch(two["topos"], two["xs"], **kw)


def _collect(batch, dl):
    torch.cuda.synchronize()
    drag = torch.cat([d for d, _ in dl], dim=1).cpu().numpy()
    lift = torch.cat([l for _, l in dl], dim=1).cpu().numpy()
    assert (batch.status.cpu().numpy() == 0).all()
    return drag, lift, batch.u_n.cpu().numpy(), batch.p_n.cpu().numpy()


def _check_oracle(batch, drag, lift, b, ref, where, tol=1e-8):
    t = batch.topos[b]
    uo, po, do, lo = ref
    u, p = batch.u_n[b, :t.np2].cpu().numpy(), batch.p_n[b, :t.nv].cpu().numpy()
    eu = np.abs(_oracle_vel(u) - uo).max() / np.abs(uo).max()
    ep = np.abs(p - po).max() / np.abs(po).max()
    ed, el = abs(drag - do) / abs(do), abs(lift - lo) / abs(lo)
    print(f"{where}: u {eu:.2e} p {ep:.2e} drag {ed:.2e} lift {el:.2e}")
    assert max(eu, ep, ed, el) <= tol, (where, eu, ep, ed, el)


# ------------------------------------------------------------------ 1: what the kernel writes
@pytest.mark.parametrize("mode", [2, 3])
def test_one_step_rewrites_the_inlet_values_and_the_lifts_of_the_listed_rows_only(two, mode):
    """One step in one `evolve` call with profiles against a second batch given the same values through `update_inflow` (which
    reruns the set-up kernel): bcu_gx bit for bit; lift1 / lift3 <= 1e-13 max|lift| (assembled operators; sums
    of a few dozen terms) on every row the step kernels read - the Dirichlet rows of the lifts are read by no kernel (their
    right-hand side is the boundary value) and are in no row list; idiag1, sdiagM, geom and every lift row outside the row list
    and the Dirichlet set keep the bits they had before the call."""
    prof = _batch(two, mode=mode, inflow_profile=PROFILES)
    prof.assemble()
    keys = ("idiag1", "sdiagM", "geom", "lift1", "lift3", "bcu_gx")
    before = {k: prof.t[k].clone() for k in keys}
    prof.evolve(1)
    torch.cuda.synchronize()
    ref = _batch(two, mode=mode)
    ref.assemble()
    n_in = [len(t["dofs"]) for t in prof._prof_tab]
    assert n_in[0] != n_in[1] and len(prof._prof_tab[0]["rows"]) != len(prof._prof_tab[1]["rows"])     # the padding is in use
    ref.update_inflow(lambda x, y, t: PROFILES[0 if len(x) == n_in[0] else 1](x, y, t), 1 * DT)
    torch.cuda.synchronize()
    assert torch.equal(prof.t["bcu_gx"], ref.t["bcu_gx"])
    assert not torch.equal(prof.t["bcu_gx"], before["bcu_gx"])
    for k in ("idiag1", "sdiagM", "geom"):
        assert torch.equal(prof.t[k], before[k]), k
    flag = prof.t["bcu_flag"].cpu().numpy() != 0
    for b, tab in enumerate(prof._prof_tab):
        n2 = prof.topos[b].np2
        listed = np.zeros(prof.N2, bool)
        listed[tab["rows"]] = True
        free = ~flag[b]
        free[n2:] = False
        for k in ("lift1", "lift3"):
            got, want, old = (x[k][b].cpu().numpy() for x in (prof.t, ref.t, before))
            scale = np.abs(want[free]).max()
            err = np.abs(got[free] - want[free]).max() / scale
            print(f"mode {mode} env {b} {k}: {err:.2e} of max|lift| {scale:.3e} over {int(listed.sum())} listed rows")
            assert err <= 1e-13, (mode, b, k, err)
            assert np.array_equal(got[~listed & free], old[~listed & free]), (b, k)      # untouched rows: the bits of before
            assert np.array_equal(got[n2:], old[n2:]), (b, k)                              # and the padding
            assert np.abs(got[listed] - old[listed]).max() > 1e-3 * scale                  # the listed rows did change
        assert not (listed & flag[b]).any()


# ------------------------------------------------------------------ 2: the oracle
@pytest.mark.parametrize("mode", [2, 3])
def test_four_steps_in_one_call_match_the_oracle_under_the_same_callables(two, oracle4, mode):
    """Per-environment profiles, every step against `OracleFlowSolver(coords, cells, inflow=profile_b)`: drag, lift, u, p
    <= 1e-8 relative.  Four steps in ONE call give the forces of every step and the final fields; a second
    batch advanced in four calls of one step gives the fields of every step."""
    whole = _batch(two, mode=mode, inflow_profile=PROFILES)
    d, l = whole.evolve(4)
    torch.cuda.synchronize()
    d, l = d.cpu().numpy(), l.cpu().numpy()
    assert whole.steps_done == 4 and (whole.status.cpu().numpy() == 0).all()
    for b in range(2):
        for s in range(4):
            do, lo = oracle4[b][s][2], oracle4[b][s][3]
            assert abs(d[b, s] - do) <= 1e-8 * abs(do) and abs(l[b, s] - lo) <= 1e-8 * abs(lo), (mode, b, s, d[b, s], do, l[b, s], lo)
        _check_oracle(whole, d[b, 3], l[b, 3], b, oracle4[b][3], (mode, "one call", b))
    single = _batch(two, mode=mode, inflow_profile=PROFILES)
    for s in range(4):
        ds, ls = single.evolve(1)
        torch.cuda.synchronize()
        for b in range(2):
            _check_oracle(single, float(ds[b, 0]), float(ls[b, 0]), b, oracle4[b][s], (mode, "step", s, b))
    assert abs(d[0, 1] - d[1, 1]) > 1e-3 * abs(d[0, 1])                 # two meshes, two profiles: different numbers


# ------------------------------------------------------------------ 3: split launches
@pytest.mark.parametrize("mode", [2, 3])
def test_eight_steps_in_one_call_equal_eight_calls(two, mode):
    """Mode 2 (fixed summation order): drag, lift, u_n, p_n bit for bit.  Mode 3 (LDS atomics): <= 1e-9 relative, the tolerance
    tests/test_ipcs_gpu.py uses for the same comparison."""
    one, many = (_batch(two, mode=mode, inflow_profile=PROFILES) for _ in range(2))
    got = _collect(one, [one.evolve(8)])
    ref = _collect(many, [many.evolve(1) for _ in range(8)])
    assert one.steps_done == many.steps_done == 8 and got[0].shape == (2, 8) and np.isfinite(got[0]).all()
    if mode == 2:
        for g, r in zip(got, ref):
            assert np.array_equal(g, r)
    else:
        for g, r in zip(got[:2], ref[:2]):
            assert np.allclose(g, r, rtol=1e-9, atol=0)
        for g, r in zip(got[2:], ref[2:]):
            assert np.abs(g - r).max() <= 1e-9 * np.abs(r).max()
    # explicit times that equal the default clock give the default's bits
    own = _batch(two, mode=mode, inflow_profile=PROFILES)
    if mode == 2:
        t = np.arange(1, 9) * DT
        for g, r in zip(_collect(own, [own.evolve(8, inflow_times=t)]), got):
            assert np.array_equal(g, r)


# ------------------------------------------------------------------ 4: the separable special case
@pytest.mark.parametrize("mode", [2, 3])
def test_a_separable_profile_equals_the_same_factors_through_inflow_scale(two, mode):
    """profile = a(t) * parabola through `inflow_profile=` against a(t) through `inflow_scale=`: <= 1e-9 relative on drag / lift
    over 4 steps (not bits: the lifts are recomputed rather than scaled)."""
    def a(t):
        return 0.8 * (1.0 + 0.3 * np.sin(2.0 * np.pi * 50.0 * t + 1.0))

    prof = _batch(two, mode=mode, inflow_profile=lambda x, y, t: a(t) * (-4.0 * 1.5 * (y + 0.5) * (y - 0.5)))
    scal = _batch(two, mode=mode)
    F = np.tile(a(np.arange(1, 5) * DT), (2, 1))
    got = _collect(prof, [prof.evolve(4)])
    ref = _collect(scal, [scal.evolve(4, inflow_scale=F)])
    for g, r in zip(got[:2], ref[:2]):
        err = np.abs(g - r) / np.abs(r)
        print(f"mode {mode}: separable profile against inflow_scale {err.max():.2e}")
        assert err.max() <= 1e-9, (mode, err)
    assert abs(got[0][0, 3] - got[0][0, 2]) > 1e-3 * abs(got[0][0, 3])     # the factor moves from step to step


# ------------------------------------------------------------------ 5: None beside a profile
def test_an_environment_without_a_profile_keeps_the_constant_inflow(two):
    mixed = _batch(two, mode=2, inflow_profile=[None, profile_b])
    const = _batch(two, mode=2)
    assert mixed.inflow_profile == [None, profile_b] and const.inflow_profile is None
    got = _collect(mixed, [mixed.evolve(4)])
    ref = _collect(const, [const.evolve(4)])
    for g, r in zip(got[:2], ref[:2]):
        assert np.allclose(g[0], r[0], rtol=1e-9, atol=0), (g[0], r[0])
        assert not np.allclose(g[1], r[1], rtol=1e-3, atol=0)             # environment 1 is under its profile


# ------------------------------------------------------------------ 6: env_phys beside a profile
def test_profiles_beside_per_environment_viscosities(two, oracle4):
    """mu = 1e-3 / 2e-3 in the two-environment batch (the kernel takes a = rho / dt and mu from the environment's view):
    every step of each environment against its own oracle, <= 1e-8."""
    want1 = _oracle_steps(two["raw"][1], profile_b, 4, mu=2e-3)
    batch = _batch(two, mode=2, mu=[1e-3, 2e-3], inflow_profile=PROFILES)
    assert batch.env_phys is not None
    for s in range(4):
        d, l = batch.evolve(1)
        torch.cuda.synchronize()
        _check_oracle(batch, float(d[0, 0]), float(l[0, 0]), 0, oracle4[0][s], ("mu 1e-3", s))
        _check_oracle(batch, float(d[1, 0]), float(l[1, 0]), 1, want1[s], ("mu 2e-3", s))
    assert abs(want1[3][2] - oracle4[1][3][2]) > 1e-3 * abs(want1[3][2])    # the other viscosity is another flow


# ------------------------------------------------------------------ 7: refusals
@pytest.mark.parametrize("mode", [0, 5])
def test_the_modes_that_step_inside_one_kernel_refuse_a_profile_before_any_launch(two, mode):
    from meshdqn_amd import _lib
    batch = _batch(two, mode=mode, inflow_profile=PROFILES)
    with pytest.raises(_lib.MeshDQNHipError, match=f"mode {mode}"):
        batch.evolve(2)
    assert batch.steps_done == 0 and not batch.assembled and batch._inflow_keep is None
    # the entry point itself: an error status, the text names the mode and the per-step path
    vals = torch.zeros((2, 2, batch._prof_desc.NIN), dtype=torch.float64, device="cuda")
    batch._prof_desc.values = vals.data_ptr()
    drag = torch.full((2, 2), 7.0, dtype=torch.float64, device="cuda")
    lift = drag.clone()
    rc = batch.lib.mdq_ipcs_evolve_profile(C.byref(batch.desc), 2, drag.data_ptr(), lift.data_ptr(), batch.iters.data_ptr(),
                                           C.byref(batch._prof_desc), _lib.stream_ptr())
    msg = batch.lib.mdq_last_error().decode()
    assert rc != 0 and f"mode {mode}" in msg and "per-step path" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((drag == 7.0).all()) and not batch.u_n.any()              # nothing ran
    # bad arguments are refused like the other entry points'
    bad = _lib.InflowProfile()
    assert batch.lib.mdq_ipcs_evolve_profile(C.byref(batch.desc), 2, drag.data_ptr(), lift.data_ptr(), None, C.byref(bad),
                                             _lib.stream_ptr()) != 0


def test_a_null_profile_is_mdq_ipcs_evolve(two):
    """`prof = NULL` through the raw entry point gives the bits of `mdq_ipcs_evolve` (mode 2); bad capacities, missing arrays
    and nsteps <= 0 are refused."""
    from meshdqn_amd import _lib
    raw, plain = _batch(two, mode=2), _batch(two, mode=2)
    raw.assemble()
    drag = torch.empty((2, 3), dtype=torch.float64, device="cuda")
    lift = torch.empty_like(drag)
    rc = raw.lib.mdq_ipcs_evolve_profile(C.byref(raw.desc), 3, drag.data_ptr(), lift.data_ptr(), raw.iters.data_ptr(), None,
                                         _lib.stream_ptr())
    assert rc == 0, raw.lib.mdq_last_error()
    ref = _collect(plain, [plain.evolve(3)])
    torch.cuda.synchronize()
    assert np.array_equal(drag.cpu().numpy(), ref[0]) and np.array_equal(lift.cpu().numpy(), ref[1])
    assert np.array_equal(raw.u_n.cpu().numpy(), ref[2]) and np.array_equal(raw.p_n.cpu().numpy(), ref[3])
    assert np.array_equal(raw.iters.cpu().numpy(), plain.iters.cpu().numpy())
    full = _batch(two, mode=2, inflow_profile=PROFILES)
    vals = torch.zeros((2, 3, full._prof_desc.NIN), dtype=torch.float64, device="cuda")
    args = (drag.data_ptr(), lift.data_ptr(), None)
    for field, value in (("NIN", 0), ("NIR", -1), ("rows", None), ("values", None), ("n_inlet", None)):
        p = _lib.InflowProfile()
        C.pointer(p)[0] = full._prof_desc
        p.values = vals.data_ptr()
        setattr(p, field, value)
        assert full.lib.mdq_ipcs_evolve_profile(C.byref(full.desc), 3, *args, C.byref(p), _lib.stream_ptr()) != 0, field
    full._prof_desc.values = vals.data_ptr()
    assert full.lib.mdq_ipcs_evolve_profile(C.byref(full.desc), 0, *args, C.byref(full._prof_desc), _lib.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert not full.u_n.any()


# ------------------------------------------------------------------ 8: FlowSolver
def test_flow_solver_runs_a_callable_in_one_call(two, oracle4, monkeypatch):
    """`FlowSolver(inflow=profile).evolve(4)` in the default (reproducible) mode no longer goes through `update_inflow`: one
    call, the oracle's four steps to <= 1e-8, and the clock of the per-step loop."""
    from meshdqn_amd.flow_solver import FlowSolver
    from meshdqn_amd.ipcs_batch import IpcsBatch

    def no_update(self, *a, **k):
        raise AssertionError("the per-step path was taken")

    monkeypatch.setattr(IpcsBatch, "update_inflow", no_update)
    fs = FlowSolver(flow_params={"mu": MU, "rho": RHO, "inflow": profile_a}, geometry_params={"mesh": os.path.join(GOLDEN, "ys930.npz")},
                    solver_params={"dt": DT, "smooth": True, "rtol": 1e-12})
    assert fs.batch.inflow_profile == [profile_a] and fs.batch.inflow is None and fs.batch.serves_profile()
    u, p, drag, lift = fs.evolve(4)
    assert len(fs.accumulated_drag) == 4 and fs.batch.steps_done == 4
    for s in range(4):
        do, lo = oracle4[0][s][2], oracle4[0][s][3]
        assert abs(fs.accumulated_drag[s] - do) <= 1e-8 * abs(do) and abs(fs.accumulated_lift[s] - lo) <= 1e-8 * abs(lo), s
    uo, po = oracle4[0][3][0], oracle4[0][3][1]
    n2 = fs.mesh.topology_.np2
    assert np.abs(_oracle_vel(u.vector().get_local().reshape(n2, 2)) - uo).max() <= 1e-8 * np.abs(uo).max()
    assert np.abs(p.vector().get_local() - po).max() <= 1e-8 * np.abs(po).max()
    g = 0.0
    for _ in range(4):
        g += DT
    assert fs.gtime == g


# ------------------------------------------------------------------ 9: deployment
def test_batched_resimulation_under_a_callable_equals_the_sequential_one(two):
    """`resimulate_batch` on two coarsened meshes under a callable against the sequential re-simulation of `batched=False`
    (DEPLOY mode: remesh, then `run_sim`): <= 1e-9 relative - and NOT the constant parabola's result, which is what the batch
    silently computed before."""
    from meshdqn_amd.deploy import resimulate_batch, run_sim
    from meshdqn_amd.flow_solver import FlowSolver, Mesh
    from meshdqn_amd.mesh_ops import remove_vertex_delaunay

    def solver(inflow):
        return FlowSolver(flow_params={"mu": MU, "rho": RHO, "inflow": inflow}, geometry_params={"mesh": os.path.join(GOLDEN, "ys930.npz")},
                          solver_params={"dt": DT, "smooth": True, "rtol": 1e-12})

    fs = solver(profile_a)
    fs.deploy()
    env = types.SimpleNamespace(flow_solver=fs, solver_steps=24, save_steps=8)
    meshes, seq_d, seq_l = [], [], []
    for pick in (30, 65):                                          # two removals, one after the other
        topo = fs.mesh.topology_
        c, cells = remove_vertex_delaunay(topo.coords, np.flatnonzero(topo.on_boundary), int(fs.removable[pick]))
        fs.remesh(Mesh(c, cells))
        meshes.append((fs.mesh.coordinates().copy(), fs.mesh.cells().copy()))
        _, _, d, l = run_sim(env)
        seq_d.append(d), seq_l.append(l)
    nv0 = two["raw"][0][0].shape[0]
    assert meshes[0][0].shape[0] == nv0 - 1 and meshes[1][0].shape[0] == nv0 - 2
    D, L = resimulate_batch(env, meshes)
    assert D.shape == (2, 3)
    for got, want in ((D, np.array(seq_d)), (L, np.array(seq_l))):
        err = np.abs(got - want) / np.abs(want)
        print(f"batched against sequential: {err.max():.2e}")
        assert err.max() <= 1e-9, err
    Dc, _ = resimulate_batch(types.SimpleNamespace(flow_solver=solver("constant"), solver_steps=24, save_steps=8), meshes)
    assert (np.abs(D - Dc) > 1e-2 * np.abs(Dc)).all(), (D, Dc)
