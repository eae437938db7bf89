"""GPU: inflow schedules - a per-environment, time-dependent separable inflow a_b(t) * parabola applied inside the evolve
kernels (`mdq_ipcs_evolve_inflow`: one uniform factor per environment and step scales every read of bcu_gx / lift1 / lift3).
Every environment of a batch over several schedules must compute what the CPU oracle computes under
`inflow=lambda x, y, t: a(t) * parabola` and what a batch of its own schedule computes - bit for bit in the fixed-order
operator modes; a table of ones gives the bits of no table; K steps in one launch equal K launches; `FlowSolver`, the
environment step, the S3 flow leg, `train.py --mixed-inflow` and the batched deployment work end to end.

Schedules (A, eps, f [Hz], phi): a = 1, 0, 0, 0; b = 0.5, 0, 0, 0; c = 1, 0.5, 125, 0; d = 0.8, 0.3, 50, 1.  The oracle's drags
on ys930 (mu 1e-3, rho 1, dt 1e-3) over the first three steps: a -75.8479 / -5.8371 / 1.7310, b -37.9240 / -2.9187 / 0.8656,
c -102.6642 / -19.0080 / 12.5953, d -78.2857 / -6.5907 / 2.9559: a table that is ignored, or applied at the wrong time
index, cannot pass."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

SCHED = dict(a=(1.0, 0.0, 0.0, 0.0), b=(0.5, 0.0, 0.0, 0.0), c=(1.0, 0.5, 125.0, 0.0), d=(0.8, 0.3, 50.0, 1.0))
ABCD = [SCHED[k] for k in "abcd"]
ORACLE_DRAGS = dict(a=(-75.8479, -5.8371, 1.7310), b=(-37.9240, -2.9187, 0.8656), c=(-102.6642, -19.0080, 12.5953),
                    d=(-78.2857, -6.5907, 2.9559))
MU, RHO, DT = 1e-3, 1.0, 1e-3
BITWISE_MODES = [0, 1, 2, 4, 5, 7]           # fixed summation order; mode 3 accumulates with LDS fp64 atomics
SOLVER_STEPS, SAVE_STEPS = 50, 10            # S = 5 snapshots, 17 node features: the stock shapes without 5000 steps


def _dict(s):
    return dict(amplitude=s[0], pulsation=s[1], frequency=s[2], phase=s[3])


def _a(s, t):
    """The schedule's factor at time t, as the profile handed to the oracle evaluates it."""
    return s[0] * (1.0 + s[1] * math.sin(2.0 * math.pi * s[2] * t + s[3]))


def _oracle(coords, cells, s, **kw):
    """The CPU oracle under the separable inflow a(t) * its own constant parabola (oracle/ipcs.py takes inflow=callable)."""
    from oracle.ipcs import OracleFlowSolver
    box = {}
    o = OracleFlowSolver(coords, cells, inflow=lambda x, y, t: _a(s, t) * box["o"].th.inflow_profile(np.stack([x, y], axis=1)), **kw)
    box["o"] = o
    return o


# ---- helper copied from tests/oracle_util.py
def _oracle_vel(u):
    """device [dof][component] -> the oracle's [ux | uy]."""
    return np.concatenate([u[:, 0], u[:, 1]])


@pytest.fixture(scope="module")
def ys930(meshes, lib_built):
    from meshdqn_amd.ipcs_batch import smooth_coords
    from meshdqn_amd.topology import MeshTopology
    coords, cells = meshes["ys930"]
    t0 = MeshTopology(coords, cells)
    return dict(coords=coords, cells=cells, t0=t0, x0=smooth_coords(t0, 50))


@pytest.fixture(scope="module")
def oracle_first_steps(ys930):
    """Per schedule: the oracle's first three steps on ys930 (u, p, drag, lift), computed once; the drags are the issue's."""
    from oracle.ipcs import OracleFlowSolver
    out = {}
    for key, s in SCHED.items():
        o = _oracle(ys930["coords"], ys930["cells"], s)
        out[key] = [tuple(np.copy(v) for v in o.evolve()) for _ in range(3)]
        for k in range(3):
            assert abs(float(out[key][k][2]) - ORACLE_DRAGS[key][k]) < 1e-4, (key, k, out[key][k][2])
    drags3 = [float(out[k][2][2]) for k in "abcd"]
    assert all(abs(x - y) > 1e-3 for i, x in enumerate(drags3) for y in drags3[i + 1:])       # pairwise different
    plain = OracleFlowSolver(ys930["coords"], ys930["cells"])                                  # schedule a == no inflow, bit for bit
    for k in range(3):
        for v, w in zip(plain.evolve(), out["a"][k]):
            assert np.array_equal(v, w), k
    return out


def _batch(ys930, n, **kw):
    from meshdqn_amd.ipcs_batch import IpcsBatch
    kw.setdefault("mu", MU), kw.setdefault("rho", RHO), kw.setdefault("dt", DT)
    return IpcsBatch([ys930["t0"]] * n, [ys930["x0"]] * n, **kw)


def _collect(batch, dl):
    torch.cuda.synchronize()
    drag = torch.cat([d for d, _ in dl], dim=1).cpu().numpy()
    lift = torch.cat([l for _, l in dl], dim=1).cpu().numpy()
    assert (batch.status.cpu().numpy() == 0).all()
    return drag, lift, batch.u_n.cpu().numpy(), batch.p_n.cpu().numpy(), batch.iters.cpu().numpy()


def _run(batch, steps, **kw):
    """`steps` single-step launches -> drag, lift (B, steps), u_n, p_n, iters as numpy."""
    return _collect(batch, [batch.evolve(1, **kw) for _ in range(steps)])


def _check_oracle(got, b, n2, nv, ref, where, tol=1e-8):
    uo, po, do, lo = ref
    eu = np.abs(_oracle_vel(got[2][b][:n2]) - uo).max() / np.abs(uo).max()
    ep = np.abs(got[3][b][:nv] - po).max() / np.abs(po).max()
    ed, el = abs(got[0][b, -1] - do) / abs(do), abs(got[1][b, -1] - lo) / abs(lo)
    print(f"{where}: u {eu:.2e} p {ep:.2e} drag {ed:.2e} lift {el:.2e}")
    assert max(eu, ep, ed, el) <= tol, (where, eu, ep, ed, el)


# ------------------------------------------------------------------ 1: every operator mode against the oracle
@pytest.mark.parametrize("mode,direct", [(0, False), (1, False), (2, False), (2, "device"), (3, False), (3, "device"),
                                         (4, False), (5, False), (7, False)])
def test_mixed_inflow_batch_equals_one_schedule_batches_and_the_oracle(ys930, oracle_first_steps, mode, direct):
    """Four environments on ys930 under a / b / c / d, three single-step launches from rest.  Per step against the oracle under
    each schedule: u, p, drag, lift <= 1e-8.  Against four batches of one environment with the same
    schedule: bit for bit in the fixed-order modes; in mode 3 drag, lift, u_n, p_n to 1e-9 (maximum norm) and iteration counts
    within 2 - the mode-3 figures of the mixed-flow test."""
    kw = dict(rtol=1e-12, mode=mode, pressure_direct=direct)
    mixed = _batch(ys930, 4, inflow=[_dict(s) for s in ABCD], **kw)
    assert mixed.inflow == ABCD and mixed.env_phys is None
    ones = [_batch(ys930, 1, inflow=s, **kw) for s in ABCD]
    n2, nv = ys930["t0"].np2, ys930["t0"].nv
    for step in range(3):
        got = _run(mixed, 1)
        refs = [_run(o, 1) for o in ones]
        assert mixed.steps_done == step + 1
        for b, key in enumerate("abcd"):
            ref = refs[b]
            where = (mode, direct, step, key)
            if mode in BITWISE_MODES:
                for g, r in zip(got, ref):
                    assert np.array_equal(g[b], r[0]), where
            else:
                for g, r in zip(got[:2], ref[:2]):                                        # drag, lift
                    assert np.allclose(g[b], r[0], rtol=1e-9, atol=0), where
                for g, r in zip(got[2:4], ref[2:4]):                                      # u_n, p_n: in the maximum norm
                    assert np.abs(g[b] - r[0]).max() <= 1e-9 * np.abs(r[0]).max(), where
                assert np.abs(got[4][b].astype(int) - ref[4][0].astype(int)).max() <= 2, where
            _check_oracle(got, b, n2, nv, oracle_first_steps[key][step], where)
    it = mixed.iters.cpu().numpy()
    assert (it[:, 0] > 0).all() and ((it[:, 1] == 0) if direct else (it[:, 1] > 0)).all()
    assert len(set(got[0][:, 0].tolist())) == 4                                           # the schedules really differ


# ------------------------------------------------------------------ 2: a table of ones
@pytest.mark.parametrize("mode", BITWISE_MODES)
def test_table_of_ones_gives_the_bits_of_no_table(ys930, mode):
    """x * 1.0 is exact and so is a contraction of f - 1.0 * l: schedule a (the entry point WITH a table) gives the bits of
    `mdq_ipcs_evolve` - u_n, p_n, drag, lift and iteration counts over three steps."""
    kw = dict(rtol=1e-12, mode=mode, pressure_direct=False)
    table = _batch(ys930, 2, inflow=[SCHED["a"], dict(amplitude=1.0)], **kw)
    plain = _batch(ys930, 2, **kw)
    assert table.inflow is not None and plain.inflow is None
    got, ref = _run(table, 3), _run(plain, 3)
    assert table._inflow_keep is not None and np.array_equal(table._inflow_keep.cpu().numpy(), np.ones((2, 1)))
    assert plain._inflow_keep is None
    for g, r in zip(got, ref):
        assert np.array_equal(g, r), mode


# ------------------------------------------------------------------ 3: K steps in one launch
@pytest.mark.parametrize("mode", [2, 7, 3])
def test_eight_steps_in_one_launch_equal_eight_launches(ys930, mode):
    """Schedules c and d, B = 2: `evolve(8)` against eight `evolve(1)` on a fresh batch - a wrong time index inside a launch
    or a `steps_done` that is not carried across launches shows here.  Modes 2 and 7 bit for bit, mode 3 to 1e-9."""
    kw = dict(rtol=1e-12, mode=mode, pressure_direct=False, inflow=[SCHED["c"], SCHED["d"]])
    one, many = _batch(ys930, 2, **kw), _batch(ys930, 2, **kw)
    got = _collect(one, [one.evolve(8)])
    ref = _run(many, 8)
    assert one.steps_done == many.steps_done == 8
    assert got[0].shape == (2, 8) and np.isfinite(got[0]).all()
    if mode in BITWISE_MODES:
        for g, r in zip(got, ref):
            assert np.array_equal(g, r), mode
    else:
        for g, r in zip(got[:2], ref[:2]):
            assert np.allclose(g, r, rtol=1e-9, atol=0), mode
        for g, r in zip(got[2:4], ref[2:4]):
            assert np.abs(g - r).max() <= 1e-9 * np.abs(r).max(), mode


# ------------------------------------------------------------------ 4: mixed with env_phys
def test_schedules_beside_per_environment_flow_constants(ys930, oracle_first_steps):
    """B = 2: schedule c at (mu, rho, dt) = (1e-3, 2, 5e-4) beside schedule a at (1e-3, 1, 1e-3), mode 2, three steps against
    the oracle at each setting to 1e-8.  Every environment's clock runs on its own dt (oracle drags of the first
    environment: -180.1288, -124.3695, -79.1955)."""
    o = _oracle(ys930["coords"], ys930["cells"], SCHED["c"], mu=1e-3, rho=2.0, dt=5e-4)
    want0 = [tuple(np.copy(v) for v in o.evolve()) for _ in range(3)]
    for k, d in enumerate((-180.1288, -124.3695, -79.1955)):
        assert abs(float(want0[k][2]) - d) < 1e-4, (k, want0[k][2])
    batch = _batch(ys930, 2, mu=[1e-3, 1e-3], rho=[2.0, 1.0], dt=[5e-4, 1e-3], inflow=[SCHED["c"], SCHED["a"]],
                   rtol=1e-12, mode=2, pressure_direct=False)
    assert batch.env_phys is not None
    n2, nv = ys930["t0"].np2, ys930["t0"].nv
    for step in range(3):
        got = _run(batch, 1)
        _check_oracle(got, 0, n2, nv, want0[step], ("c at d-flow", step))
        _check_oracle(got, 1, n2, nv, oracle_first_steps["a"][step], ("a", step))


# ------------------------------------------------------------------ 5: refined mesh
@pytest.mark.parametrize("mode", [5, 7])
def test_mixed_inflow_on_the_refined_mesh(ys930, mode):
    """ys930 red-refined (3 322 vertices: the non-packed tile paths and - mode 7 - the team barrier) twice beside the lab mesh,
    under a / c / d: two steps, bit for bit against the same batch under one schedule each."""
    from meshdqn_amd.ipcs_batch import IpcsBatch
    from meshdqn_amd.mesh_ops import red_refine
    from meshdqn_amd.topology import MeshTopology
    rc, rcells = red_refine(ys930["x0"], ys930["cells"])
    rt = MeshTopology(rc, rcells)
    assert (rt.nv, rt.nt) == (3322, 6280)
    topos, xs = [rt, rt, ys930["t0"]], [rc, rc, ys930["x0"]]
    kw = dict(mu=MU, rho=RHO, dt=DT, rtol=1e-12, mode=mode, pressure_direct=False)
    scheds = [SCHED[k] for k in "acd"]
    mixed = IpcsBatch(topos, xs, inflow=scheds, **kw)
    got = _run(mixed, 2)
    assert np.isfinite(got[0]).all() and len(set(got[0][:, 1].tolist())) == 3
    for b, s in enumerate(scheds):
        ref = _run(IpcsBatch(topos, xs, inflow=s, **kw), 2)
        for g, r in zip(got, ref):
            assert np.array_equal(g[b], r[b]), (mode, b)


# ------------------------------------------------------------------ 6: explicit factors
def test_explicit_factors_equal_the_schedules_and_are_checked_before_any_launch(ys930):
    from meshdqn_amd.inflow import inflow_factors
    kw = dict(rtol=1e-12, mode=2, pressure_direct=False)
    F = inflow_factors(ABCD, DT, 0, 3)
    sched, own, own_t = _batch(ys930, 4, inflow=ABCD, **kw), _batch(ys930, 4, **kw), _batch(ys930, 4, **kw)
    ref = _collect(sched, [sched.evolve(3)])
    got = _collect(own, [own.evolve(3, inflow_scale=F)])
    got_t = _collect(own_t, [own_t.evolve(3, inflow_scale=torch.from_numpy(F).cuda())])
    for g, gt, r in zip(got, got_t, ref):
        assert np.array_equal(g, r) and np.array_equal(gt, r)
    assert len(set(ref[0][:, 2].tolist())) == 4
    fresh = _batch(ys930, 4, **kw)
    bad = F.copy()
    bad[2, 1] = np.nan
    for wrong in (F[:, :2], F[:3], F.T, F.ravel(), bad, np.where(np.isnan(bad), np.inf, bad)):
        with pytest.raises(ValueError, match="inflow_scale"):
            fresh.evolve(3, inflow_scale=wrong)
    assert fresh.steps_done == 0 and not fresh.assembled and fresh._inflow_keep is None       # nothing was launched
    with pytest.raises(ValueError, match="frequency"):
        _batch(ys930, 2, inflow=[SCHED["a"], dict(frequency=-1.0)])
    with pytest.raises(ValueError, match="length 4"):
        _batch(ys930, 4, inflow=[SCHED["a"], SCHED["b"]])


# ------------------------------------------------------------------ 7: FlowSolver
def test_flow_solver_takes_a_schedule_dict(lib_built):
    """Schedule d through the `FlowSolver` surface, 4 steps against the oracle (drag, lift <= 1e-8 per step, gtime = 0.004);
    the existing callable path given a_d(t) * the constant parabola ends at the same drag (<= 1e-9); `evolve(4)` on a fresh
    solver equals four `evolve()` calls bit for bit (the default operator mode is the reproducible one).  The figures of
    `test_time_dependent_inflow_matches_oracle`."""
    from meshdqn_amd.flow_solver import FlowSolver
    mesh = os.path.join(GOLDEN, "ys930.npz")
    z = np.load(mesh)
    s = SCHED["d"]
    sp = {"dt": 0.001, "smooth": True, "rtol": 1e-12}

    def solver(inflow):
        return FlowSolver(flow_params={"mu": 1e-3, "rho": 1.0, "inflow": inflow}, geometry_params={"mesh": mesh}, solver_params=dict(sp))

    fs = solver(_dict(s))
    assert fs.inflow_spec == s and fs.inflow_profile is None and fs.batch.inflow == [s]
    o = _oracle(z["coords"], z["cells"], s)
    for k in range(4):
        u, p, drag, lift = fs.evolve()
        uo, po, do, lo = o.evolve()
        assert abs(drag - do) < 1e-8 * abs(do) and abs(lift - lo) < 1e-8 * abs(lo), (k, drag, do, lift, lo)
    n2 = o.th.np2
    ug = u.vector().get_local().reshape(n2, 2)
    assert np.abs(_oracle_vel(ug) - uo).max() < 1e-8 * np.abs(uo).max()
    assert abs(fs.gtime - 0.004) < 1e-15 and fs.batch.steps_done == 4
    # the callable path, one launch per step, under the same inflow
    fc = solver(lambda x, y, t: -4.0 * 1.5 * (y + 0.5) * (y - 0.5) * _a(s, t))
    assert fc.inflow_spec is None and fc.batch.inflow is None
    fc.evolve(4)
    assert abs(fc.accumulated_drag[-1] - drag) < 1e-9 * abs(drag)
    # four steps in one launch
    fs2 = solver(_dict(s))
    fs2.evolve(4)
    assert fs2.accumulated_drag == fs.accumulated_drag and fs2.accumulated_lift == fs.accumulated_lift
    assert torch.equal(fs2.batch.u_n, fs.batch.u_n) and torch.equal(fs2.batch.p_n, fs.batch.p_n)
    assert abs(fs2.gtime - 0.004) < 1e-15
    assert solver("constant").inflow_spec is None


# ------------------------------------------------------------------ configs with the oracle's ground truth
def _agent_params():
    ap = dict(json.load(open(os.path.join(GOLDEN, "oracle_stock_ys930.json")))["agent_params"])
    ap.update(solver_steps=SOLVER_STEPS, save_steps=SAVE_STEPS)
    return ap


@pytest.fixture(scope="module")
def inflow_cases(meshes, lib_built, tmp_path_factory):
    """schedule key -> dict(cfg, base, snap) on ys930: the oracle's ground truth under that schedule (50 IPCS steps, every 10th
    kept) computed once and loaded through the reference's snapshot-reload branch (as `flow_cases` of
    tests/test_mixed_flow_gpu.py does), so that the GPU environment and the oracle share one ground truth."""
    from meshdqn_amd.env import Env2DAirfoil
    cache = {}

    def case(key):
        if key in cache:
            return cache[key]
        coords, cells = meshes["ys930"]
        o = _oracle(coords, cells, SCHED[key])
        us, ps, drags, lifts = [], [], [], []
        for i in range(SOLVER_STEPS):
            u, p, drag, lift = o.evolve()
            if (i + 1) % SAVE_STEPS == 0:
                us.append(u.copy()), ps.append(p.copy()), drags.append(drag), lifts.append(lift)
        snap = dict(gt_drag=np.array(drags), gt_lift=np.array(lifts), u=np.array(us), p=np.array(ps))
        tmp = str(tmp_path_factory.mktemp(f"ys930_inflow_{key}"))
        sdir = os.path.join(tmp, "snapshots")
        os.makedirs(sdir)
        n2 = snap["u"].shape[1] // 2
        np.save(os.path.join(sdir, "save_velocities.npy"),
                np.stack([snap["u"][:, :n2], snap["u"][:, n2:]], axis=2).reshape(len(us), -1))
        np.save(os.path.join(sdir, "save_pressures.npy"), snap["p"])
        ap = _agent_params()
        ap.update(gt_drag=snap["gt_drag"].copy(), gt_lift=snap["gt_lift"].copy(), gt_time=np.array([SOLVER_STEPS * DT]), plot_dir=tmp)
        cfg = dict(flow_config=dict(flow_params=dict(mu=MU, rho=RHO, inflow=_dict(SCHED[key])),
                                    geometry_params=dict(mesh=os.path.join(GOLDEN, "ys930.npz")),
                                    solver_params=dict(dt=DT, solver_type="lu", smooth=True)),
                   agent_params=ap)
        cache[key] = dict(cfg=cfg, base=Env2DAirfoil(cfg), snap=snap, key=key)
        return cache[key]
    return case


def _venv(cfg, B, base, **kw):
    from meshdqn_amd.vec_env import VecEnv2DAirfoil
    return VecEnv2DAirfoil(cfg, B, base_env=base, nthreads=2, **kw)


# ---- helpers copied from tests/test_mixed_airfoils_gpu.py
def _env_state(st, b):
    e0, e1 = int(st["edge_ptr"][b]), int(st["edge_ptr"][b + 1])
    return (st["x"][b].cpu().numpy(), st["esrc"][e0:e1].cpu().numpy(), st["edst"][e0:e1].cpu().numpy())


def _same_state(s1, s2, where):
    for u, v in zip(s1, s2):
        assert u.shape == v.shape and np.array_equal(u, v), where


# (the script of tests/test_mixed_flow_gpu.py: removals, a window shift and episode ends; compared against the homogeneous
#  batches only, so no terminal flag is compared with an oracle's)
S1_ACTIONS = np.array([[30, 30, 141, 64],
                       [65, 40, 100, 114],
                       [40, 180, 108, 118],
                       [31, 165, 6, 107]], np.int64)


# ------------------------------------------------------------------ 8: S1
def test_s1_step_of_a_mixed_inflow_batch(inflow_cases):
    """S1: two configs on ys930 under schedules a and d (ground truths from the oracle under each), B = 4 (sources 0, 1, 0, 1),
    four scripted actions: rewards, dones, codes, nv, new_drags / new_lifts and the states bit for bit against the homogeneous
    B = 2 batch of each schedule."""
    cases = [inflow_cases("a"), inflow_cases("d")]
    cfgs, bases = [c["cfg"] for c in cases], [c["base"] for c in cases]
    assert not np.allclose(cases[0]["snap"]["gt_drag"], cases[1]["snap"]["gt_drag"], rtol=1e-3)
    acts, homo_acts = S1_ACTIONS, [S1_ACTIONS[:, a::2].copy() for a in range(2)]
    K, B = acts.shape
    kw = dict(auto_reset=False)
    mixed = _venv(cfgs, B, bases, mixed_inflow=True, **kw)
    assert mixed.A == 2 and mixed.airfoil.tolist() == [0, 1, 0, 1]
    assert mixed.inflow_of_env.shape == (B, 4) and mixed.inflow_of_env.tolist() == [list(SCHED["ad"[b % 2]]) for b in range(B)]
    homo = [_venv(cfgs[a], 2, bases[a], **kw) for a in range(2)]
    assert homo[1].inflow_of_env.tolist() == [list(SCHED["d"])] * 2                       # a single scheduled config: no flag
    st, hst = mixed.get_state(), [h.get_state() for h in homo]
    for b in range(B):
        _same_state(_env_state(st, b), _env_state(hst[b % 2], b // 2), ("initial", b))
    first = None
    for k in range(K):
        st, rew, done, info = mixed.step(acts[k])
        hout = [h.step(homo_acts[a][k]) for a, h in enumerate(homo)]
        for b in range(B):
            a, j = b % 2, b // 2
            hs, hr, hd, hi = hout[a]
            where = ("step", k, b)
            assert rew[b] == hr[j] and done[b] == hd[j] and info["code"][b] == hi["code"][j], where
            assert info["nv"][b] == hi["nv"][j] and mixed.nv[b] == homo[a].nv[j], where
            assert np.array_equal(info["new_drags"][b], hi["new_drags"][j]) and np.array_equal(info["new_lifts"][b], hi["new_lifts"][j]), where
            _same_state(_env_state(st, b), _env_state(hs, j), where)
        first = info["new_drags"].copy() if first is None else first
    assert not np.array_equal(first[0], first[1])                 # same mesh, same action (30), other inflow: other drags


# ------------------------------------------------------------------ 9: S3 flow leg
@pytest.mark.parametrize("overlap", [False, True])
def test_s3_flow_leg_of_a_mixed_inflow_batch(inflow_cases, overlap):
    """S3 (flow_steps=1): ys930 under a and under d in one B = 4 batch.  The IPCS step on every coarsened mesh agrees with the
    homogeneous batches to 1e-9 (mode 3: LDS atomics), status words 0; one environment per schedule against ONE oracle step
    on its very mesh, warm-started from the environment's last interpolated snapshot, under the factor a(51 dt) - the leg
    restarts at solver_steps * dt: <= 1e-7 of the force scale (the figures of the mixed-flow flow-leg test)."""
    cases = [inflow_cases("a"), inflow_cases("d")]
    cfgs, bases = [c["cfg"] for c in cases], [c["base"] for c in cases]
    B, K = 4, 3
    acts = np.random.default_rng(1370).integers(0, 181, size=(K, B))
    kw = dict(auto_reset=False, flow_steps=1, flow_rtol=1e-12, flow_overlap=overlap)
    envs = [_venv(cfgs, B, bases, mixed_inflow=True, **kw)] + [_venv(cfgs[a], 2, bases[a], **kw) for a in range(2)]
    want = np.array([[_a(SCHED["ad"[b % 2]], (SOLVER_STEPS + 1) * DT)] for b in range(B)])
    assert envs[0].flow.inflow_scale.shape == (B, 1) and np.allclose(envs[0].flow.inflow_scale.cpu().numpy(), want, rtol=1e-15, atol=0)
    assert np.array_equal(envs[1].flow.inflow_scale.cpu().numpy(), np.ones((2, 1)))       # schedule a spelled as a dict: ones
    res = []
    for venv, A in zip(envs, [acts] + [acts[:, a::2] for a in range(2)]):
        venv.get_state()
        for k in range(K):
            _, _, _, info = venv.step(A[k])
        fd, fl = venv.flow_wait() if overlap else (info["flow_drag"], info["flow_lift"])
        assert (venv.flow_status.cpu().numpy() == 0).all()
        assert np.isfinite(fd).all() and np.isfinite(fl).all()
        res.append((fd, fl))
    mixed = envs[0]
    for b in range(B):
        a, j = b % 2, b // 2
        assert np.allclose(res[0][0][b], res[1 + a][0][j], rtol=1e-9, atol=0), b
        assert np.allclose(res[0][1][b], res[1 + a][1][j], rtol=1e-9, atol=1e-12 * abs(res[1 + a][0][j][0])), b
    for b in (2, 3):                                              # one env per schedule against the oracle on its very mesh
        s = SCHED["ad"[b % 2]]
        nv, nt = int(mixed.nv[b]), int(mixed.nt[b])
        n2 = nv + int(mixed.h["ne"][b])
        o = _oracle(mixed.coords[b, :nv].copy(), mixed.cells[b, :nt].copy(), s, mu=MU, rho=RHO, dt=DT, smooth=False)
        assert o.th.np2 == n2
        o.u_n = _oracle_vel(mixed.u[b, mixed.S - 1, :n2].cpu().numpy())
        o.p_n = mixed.p[b, mixed.S - 1, :nv].cpu().numpy().copy()
        o.gtime = SOLVER_STEPS * DT                               # the step runs at t = 51 dt
        _, _, do, lo = o.evolve()
        scale = max(abs(do), abs(lo))
        fd, fl = res[0]
        print(f"flow leg env {b}: drag {fd[b, 0]:.10g} / oracle {do:.10g}, lift {fl[b, 0]:.10g} / {lo:.10g}")
        assert abs(fd[b, 0] - do) < 1e-7 * abs(do) and abs(fl[b, 0] - lo) < 1e-7 * scale, (b, fd[b, 0], do, fl[b, 0], lo)


def test_mixed_inflow_is_opt_in(inflow_cases):
    from meshdqn_amd.vec_env import VecEnv2DAirfoil
    cases = [inflow_cases("a"), inflow_cases("d")]
    with pytest.raises(ValueError, match="inflow"):
        VecEnv2DAirfoil([c["cfg"] for c in cases], 4)
    with pytest.raises(ValueError, match="inflow"):
        VecEnv2DAirfoil([c["cfg"] for c in cases], 4, mixed_flow=True)
    with pytest.raises(ValueError, match="inflow schedule must agree"):         # (handed the base environments directly)
        VecEnv2DAirfoil([cases[0]["cfg"]] * 2, 4, base_env=[c["base"] for c in cases])


# ------------------------------------------------------------------ 10: end to end
def _plain(cfg):
    return json.loads(json.dumps(cfg, default=lambda v: np.asarray(v).tolist()))


def test_train_py_with_the_mixed_inflow_flag(inflow_cases, tmp_path):
    """`train.py --config A --config B --mixed-inflow` (ys930 under a and under d) runs to the end and writes its log."""
    import yaml
    paths = []
    for c in (inflow_cases("a"), inflow_cases("d")):
        cfg = _plain(c["cfg"])
        cfg["agent_params"]["timesteps"] = 3                     # episodes end every 3 steps: the log gets entries
        p = os.path.join(str(tmp_path), f"{c['key']}.yaml")
        yaml.safe_dump(cfg, open(p, "w"))
        paths.append(p)
    assert yaml.safe_load(open(paths[1]))["flow_config"]["flow_params"]["inflow"] == _dict(SCHED["d"])
    save = os.path.join(str(tmp_path), "run")
    cmd = [sys.executable, "train.py", "--config", paths[0], "--config", paths[1], "--mixed-inflow", "--envs", "4", "--steps", "7",
           "--save-dir", save, "--save-every", "0"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run(["timeout", "-k", "10", "600"] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=660)
    assert out.returncode == 0, out.stderr[-4000:]
    af = np.load(os.path.join(save, "airfoil.npy"))
    assert len(af) >= 2 and set(af.tolist()) == {0, 1}


def test_batched_deployment_resimulates_under_the_schedule(inflow_cases, tmp_path):
    """`deploy()` on the config under schedule d: `batched=True` (all coarsened meshes as one `IpcsBatch`, which now gets the
    flow solver's schedule) writes the files of `batched=False` (one mesh at a time through the flow solver) bit for bit."""
    from meshdqn_amd.deploy import deploy
    from meshdqn_amd.env import Env2DAirfoil
    cfg = inflow_cases("d")["cfg"]
    outs, names = [], ("interpolate_drag_trajectory", "drag_trajectory", "complete_drags", "complete_lifts", "actions")
    for batched in (False, True):
        d = os.path.join(str(tmp_path), "batched" if batched else "sequential")
        outs.append(deploy(Env2DAirfoil(cfg), actions=[30, 65], save_dir=d, prefix="t_", stop_on_done=False, batched=batched))
    seq, bat = outs
    assert seq["resimulated_meshes"] == bat["resimulated_meshes"] >= 2           # a coarsened mesh + the final simulation
    for k in names:
        x, y = (np.load(os.path.join(str(tmp_path), w, f"t_{k}.npy")) for w in ("sequential", "batched"))
        assert x.shape == y.shape and np.array_equal(x, y), k
    assert seq["new_drag"] == bat["new_drag"]
    # the re-simulated coarsened meshes sit near the schedule's ground truth (not the constant parabola's, whose last drag is
    # that of schedule a)
    gd, ga = inflow_cases("d")["snap"]["gt_drag"][-1], inflow_cases("a")["snap"]["gt_drag"][-1]
    assert abs(bat["complete_drags"][1][-1] - gd) < 0.5 * abs(gd - ga)
