"""GPU: one batch over several flow conditions (per-environment mu, rho, dt: `mdq_ipcs_desc.env_phys`).  Every environment
of a mixed-flow batch must compute what the same environment computes in a batch of its own flow condition - bit for bit in
the reproducible operator modes, to round-off in the LDS-atomic mode 3 - and what the CPU oracle computes at that flow
condition; a table whose rows equal the scalars gives the bits of no table; the environment step, the S3 flow leg, the
learning loop and `train.py --mixed-flow` work end to end, also with two configs on the SAME mesh.

Flow conditions (mu, rho, dt): a = 1e-3, 1, 1e-3; b = 2e-3, 1, 1e-3; c = 4e-3, 1, 1e-3; d = 1e-3, 2, 5e-4.  The oracle's drag
on ys930 after 50 steps is -0.2398 / -0.3515 / -0.5089 / -0.3811 for a / b / c / d: a table that is ignored cannot pass."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

FLOWS = dict(a=(1e-3, 1.0, 1e-3), b=(2e-3, 1.0, 1e-3), c=(4e-3, 1.0, 1e-3), d=(1e-3, 2.0, 5e-4))
ABCD = [FLOWS[k] for k in "abcd"]
MU, RHO, DT = ([f[i] for f in ABCD] for i in range(3))
BITWISE_MODES = [0, 1, 2, 4, 5, 7]           # fixed summation order; mode 3 accumulates with LDS fp64 atomics
SOLVER_STEPS, SAVE_STEPS = 50, 10            # S = 5 snapshots, 17 node features: the stock shapes without 5000 steps


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
    """Per flow condition: the oracle's solver on ys930 and its first three steps (u, p, drag, lift), computed once."""
    from oracle.ipcs import OracleFlowSolver
    out = {}
    for key, (mu, rho, dt) in FLOWS.items():
        o = OracleFlowSolver(ys930["coords"], ys930["cells"], mu=mu, rho=rho, dt=dt)
        out[key] = dict(solver=o, steps=[tuple(np.copy(v) for v in o.evolve()) for _ in range(3)])
    assert len({round(float(s["steps"][2][2]), 9) for s in out.values()}) == 4           # four different drags
    return out


def _batch(ys930, n, **kw):
    from meshdqn_amd.ipcs_batch import IpcsBatch
    return IpcsBatch([ys930["t0"]] * n, [ys930["x0"]] * n, **kw)


def _run(batch, steps):
    """`steps` single-step launches -> drag, lift (B, steps), u_n, p_n, iters as numpy."""
    dl = [batch.evolve(1) for _ in range(steps)]
    torch.cuda.synchronize()
    drag = torch.cat([d for d, _ in dl], dim=1).cpu().numpy()
    lift = torch.cat([l for _, l in dl], dim=1).cpu().numpy()
    assert (batch.status.cpu().numpy() == 0).all()
    return drag, lift, batch.u_n.cpu().numpy(), batch.p_n.cpu().numpy(), batch.iters.cpu().numpy()


# ------------------------------------------------------------------ 1: S2, every operator mode
@pytest.mark.parametrize("mode,direct", [(0, False), (1, False), (2, False), (2, "device"), (3, False), (3, "device"),
                                         (4, False), (5, False), (7, False)])
def test_mixed_flow_batch_equals_one_setting_batches_and_the_oracle(ys930, oracle_first_steps, mode, direct):
    """Four environments on ys930 at a / b / c / d, three steps from rest, against four batches of one environment and one
    (scalar) setting in the same mode: u_n, p_n, drag, lift and iteration counts bit for bit in the reproducible modes; in
    mode 3 (LDS atomics: the order of a row's additions is not fixed) to 1e-9 - the figure the mixed-airfoil flow-leg test
    uses for mode 3 - with iteration counts within 2 (a stopping test at rtol 1e-12 sits on round-off).  And per step
    against the oracle at each setting: u, p, drag, lift <= 1e-8."""
    kw = dict(rtol=1e-12, mode=mode, pressure_direct=direct)
    mixed = _batch(ys930, 4, mu=MU, rho=RHO, dt=DT, **kw)
    assert mixed.env_phys is not None and mixed.env_phys.shape == (4, 4) and mixed.desc.env_phys == mixed.env_phys.data_ptr()
    assert (mixed.mu, mixed.rho, mixed.dt) == FLOWS["a"]                                  # the scalars: row 0
    ones = [_batch(ys930, 1, mu=mu, rho=rho, dt=dt, **kw) for mu, rho, dt in ABCD]
    assert all(o.env_phys is None and not o.desc.env_phys for o in ones)
    n2, nv = ys930["t0"].np2, ys930["t0"].nv
    for step in range(3):
        got = _run(mixed, 1)
        refs = [_run(o, 1) for o in ones]
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
            uo, po, do, lo = oracle_first_steps[key]["steps"][step]
            eu = np.abs(_oracle_vel(got[2][b][:n2]) - uo).max() / np.abs(uo).max()
            ep = np.abs(got[3][b][:nv] - po).max() / np.abs(po).max()
            ed, el = abs(got[0][b, 0] - do) / abs(do), abs(got[1][b, 0] - lo) / abs(lo)
            assert max(eu, ep, ed, el) <= 1e-8, (where, eu, ep, ed, el)
    it = mixed.iters.cpu().numpy()
    assert (it[:, 0] > 0).all() and ((it[:, 1] == 0) if direct else (it[:, 1] > 0)).all()
    if direct == "device":
        assert (mixed.pd_status.cpu().numpy() == 0).all()
    drag = got[0][:, 0]
    assert len(set(drag.tolist())) == 4                                                   # the settings really differ


@pytest.mark.parametrize("mode", BITWISE_MODES)
def test_table_of_equal_rows_gives_the_bits_of_no_table(ys930, mode):
    """rho / dt is formed on the device from the view in both cases: rows that repeat the scalars (setting d: rho / dt is
    not exact) give the bits of env_phys = NULL."""
    mu, rho, dt = FLOWS["d"]
    kw = dict(rtol=1e-12, mode=mode, pressure_direct=False)
    table = _batch(ys930, 2, mu=[mu, mu], rho=[rho, rho], dt=[dt, dt], **kw)
    plain = _batch(ys930, 2, mu=mu, rho=rho, dt=dt, **kw)
    assert table.env_phys is not None and plain.env_phys is None
    for g, r in zip(_run(table, 3), _run(plain, 3)):
        assert np.array_equal(g, r), mode


# ------------------------------------------------------------------ 2: refined mesh
@pytest.mark.parametrize("mode", [5, 7])
def test_mixed_flow_on_the_refined_mesh(ys930, mode):
    """ys930 red-refined (3 322 vertices: beyond the packed maps, so the non-packed tile paths and - mode 7 - the team
    barrier inside the XCD) twice beside the lab mesh, at a / b / c: two steps, bit for bit against the same batch at one
    (scalar) setting each."""
    from meshdqn_amd.ipcs_batch import IpcsBatch
    from meshdqn_amd.mesh_ops import red_refine
    from meshdqn_amd.topology import MeshTopology
    rc, rcells = red_refine(ys930["x0"], ys930["cells"])
    rt = MeshTopology(rc, rcells)
    assert (rt.nv, rt.nt) == (3322, 6280)
    topos, xs = [rt, rt, ys930["t0"]], [rc, rc, ys930["x0"]]
    kw = dict(rtol=1e-12, mode=mode, pressure_direct=False)
    mixed = IpcsBatch(topos, xs, mu=MU[:3], rho=RHO[:3], dt=DT[:3], **kw)
    got = _run(mixed, 2)
    assert np.isfinite(got[0]).all() and len(set(got[0][:, 1].tolist())) == 3
    for b, (mu, rho, dt) in enumerate(ABCD[:3]):
        ref = _run(IpcsBatch(topos, xs, mu=mu, rho=rho, dt=dt, **kw), 2)
        for g, r in zip(got, ref):
            assert np.array_equal(g[b], r[b]), (mode, b)


# ------------------------------------------------------------------ 3: probe
def test_probe_forces_with_per_environment_mu(ys930, oracle_first_steps):
    """`mdq_probe_forces` through `LightMeshBatch` with one mu per environment on one fixed (u, p) field: the scalar-mu
    launches bit for bit, the oracle's `forces` at that mu to 1e-10 relative."""
    from meshdqn_amd.mesh_ops import LightMeshBatch
    t0, x0 = ys930["t0"], ys930["x0"]
    rng = np.random.default_rng(0)
    F = 2
    u1, p1 = rng.standard_normal((1, F, t0.np2, 2)), rng.standard_normal((1, F, t0.nv))
    mus = [FLOWS[k][0] for k in "abca"]
    light = LightMeshBatch([t0] * 4, [x0] * 4, mus)
    assert light.env_phys is not None and light.env_phys[:, 0].cpu().tolist() == mus
    u4, p4 = torch.from_numpy(np.repeat(u1, 4, 0)).cuda(), torch.from_numpy(np.repeat(p1, 4, 0)).cuda()
    dr, li = (v.cpu().numpy() for v in light.probe_forces(u4, p4))
    for b, key in enumerate("abca"):
        one = LightMeshBatch([t0], [x0], mus[b])
        assert one.env_phys is None
        d1, l1 = (v.cpu().numpy() for v in one.probe_forces(torch.from_numpy(u1).cuda(), torch.from_numpy(p1).cuda()))
        assert np.array_equal(dr[b], d1[0]) and np.array_equal(li[b], l1[0]), b
        th = oracle_first_steps[key]["solver"].th
        for f in range(F):
            do, lo = th.forces(_oracle_vel(u1[0, f]), p1[0, f])
            assert abs(dr[b, f] - do) <= 1e-10 * abs(do) and abs(li[b, f] - lo) <= 1e-10 * abs(lo), (b, f)
    assert np.array_equal(dr[0], dr[3]) and not np.array_equal(dr[0], dr[1])


# ------------------------------------------------------------------ configs with the oracle's ground truth
def _agent_params():
    ap = dict(json.load(open(os.path.join(GOLDEN, "oracle_stock_ys930.json")))["agent_params"])
    ap.update(solver_steps=SOLVER_STEPS, save_steps=SAVE_STEPS)
    return ap


@pytest.fixture(scope="module")
def flow_cases(meshes, lib_built, tmp_path_factory):
    """(mesh, setting) -> dict(cfg, base, snap): the oracle's ground truth (50 IPCS steps, every 10th kept) computed once and
    loaded through the reference's snapshot-reload branch (as tests/test_stock_gpu.py `_snapshot_cfg` does), so that the
    GPU environment and the oracle share one ground truth."""
    from meshdqn_amd.env import Env2DAirfoil
    from oracle.ipcs import OracleFlowSolver
    cache = {}

    def case(mesh, key):
        if (mesh, key) in cache:
            return cache[(mesh, key)]
        mu, rho, dt = FLOWS[key]
        coords, cells = meshes[mesh]
        o = OracleFlowSolver(coords, cells, mu=mu, rho=rho, dt=dt)
        us, ps, drags, lifts = [], [], [], []
        for i in range(SOLVER_STEPS):
            u, p, drag, lift = o.evolve()
            if (i + 1) % SAVE_STEPS == 0:
                us.append(u.copy()), ps.append(p.copy()), drags.append(drag), lifts.append(lift)
        snap = dict(gt_drag=np.array(drags), gt_lift=np.array(lifts), u=np.array(us), p=np.array(ps))
        tmp = str(tmp_path_factory.mktemp(f"{mesh}_{key}"))
        sdir = os.path.join(tmp, "snapshots")
        os.makedirs(sdir)
        n2 = snap["u"].shape[1] // 2
        np.save(os.path.join(sdir, "save_velocities.npy"),
                np.stack([snap["u"][:, :n2], snap["u"][:, n2:]], axis=2).reshape(len(us), -1))
        np.save(os.path.join(sdir, "save_pressures.npy"), snap["p"])
        ap = _agent_params()
        ap.update(gt_drag=snap["gt_drag"].copy(), gt_lift=snap["gt_lift"].copy(), gt_time=np.array([SOLVER_STEPS * dt]), plot_dir=tmp)
        cfg = dict(flow_config=dict(flow_params=dict(mu=mu, rho=rho, inflow="constant"),
                                    geometry_params=dict(mesh=os.path.join(GOLDEN, f"{mesh}.npz")),
                                    solver_params=dict(dt=dt, solver_type="lu", smooth=True)),
                   agent_params=ap)
        cache[(mesh, key)] = dict(cfg=cfg, base=Env2DAirfoil(cfg), snap=snap, mesh=mesh, key=key)
        return cache[(mesh, key)]
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


# The S1 action script (6 steps, 4 environments; environment b runs setting a / b for b even / odd) is HAND-CHOSEN, not the draws
# of a generator.  default_rng(1370).integers(0, 181, (6, 4)) itself cannot be used: its first action of environment 1 (31, at
# setting b) leaves the oracle's relative drag error at 0.00099970 against the threshold 0.001 - a terminal flag on round-off -
# and its other first actions (141, 100, 108) end the episode at once at either setting, so no reward would be compared.  The script
# takes most of its values from those draws (30, 31, 40, 65, 90, 92, 165, ...), repeats some and adds 180 (shift the window: a
# step without a removal), arranged so that environments 0 and 1 run several non-terminal removals and then END inside the
# script (environment 0 at its 5th action, environment 1 at its 4th), every flag far from the threshold.
S1_ACTIONS = np.array([[30, 30, 141, 64],
                       [65, 40, 100, 114],
                       [40, 180, 108, 118],
                       [31, 165, 6, 107],
                       [92, 170, 74, 44],
                       [90, 92, 96, 22]], np.int64)
S1_ORACLE_END = (4, 3)       # the step (0-based) at which the oracle alone ends the episode of environment 0 / 1


def test_s1_step_of_a_mixed_flow_batch(flow_cases):
    """S1: two configs on the SAME mesh (ys930) at settings a and b, B = 4 (sources 0, 1, 0, 1), six scripted actions through
    `step()` and through `rollout_device(actions=...)`: rewards, dones, codes, nv, new_drags / new_lifts, the state's x and
    edge lists bit for bit against the homogeneous B = 2 batch of each setting.  Environments 0 and 1 also against `OracleEnv`
    with the same flow_params and the same ground truth, from the first action to the oracle's terminal step INCLUSIVE
    (5 steps at setting a, 4 at setting b; about 1.5 s of CPU per oracle step): new_drags / new_lifts <= 1e-7 relative, rewards
    <= 1e-6 on the non-terminal steps, the same terminal flag at every step.

    Margin of the script, measured with the oracle alone over exactly those steps: the largest relative drag error of a step is
    2.0e-4 .. 2.7e-4 on the four non-terminal steps of setting a and 3.05e-3 on its terminal step (action 92); 6.6e-4 .. 7.1e-4
    on the three non-terminal steps of setting b and 2.71e-3 on its terminal step (action 165); threshold 1e-3.  The smallest
    distance of any of the 5 drag errors of any of the 9 steps from the threshold is 1.363e-4 (setting b, terminal step).  The
    test recomputes that margin over all compared steps and asserts it is >= 1e-5: no terminal flag it compares sits on
    round-off."""
    from oracle.env import OracleEnv
    cases = [flow_cases("ys930", "a"), flow_cases("ys930", "b")]
    cfgs, bases = [c["cfg"] for c in cases], [c["base"] for c in cases]
    acts, homo_acts = S1_ACTIONS, [S1_ACTIONS[:, a::2].copy() for a in range(2)]
    K, B = acts.shape
    kw = dict(auto_reset=False)
    # ---- step()
    mixed = _venv(cfgs, B, bases, mixed_flow=True, **kw)
    assert mixed.A == 2 and mixed.airfoil.tolist() == [0, 1, 0, 1]
    assert mixed.flow_of_env.shape == (B, 3) and mixed.flow_of_env.tolist() == [list(FLOWS["ab"[b % 2]]) for b in range(B)]
    assert mixed.env_phys.shape == (B, 4) and mixed.mu == FLOWS["a"][0]
    homo = [_venv(cfgs[a], 2, bases[a], **kw) for a in range(2)]
    assert all(h.env_phys is None and h.flow_of_env is None for h in homo)
    st, hst = mixed.get_state(), [h.get_state() for h in homo]
    for b in range(B):
        _same_state(_env_state(st, b), _env_state(hst[b % 2], b // 2), ("initial", b))
    log = []
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
        log.append((rew.copy(), done.copy(), info["new_drags"].copy(), info["new_lifts"].copy(), info["nv"].copy()))
    assert not np.array_equal(log[0][2][0], log[0][2][1])         # same mesh, same action (30), other viscosity: other drags
    # ---- rollout_device
    mixed_r = _venv(cfgs, B, bases, mixed_flow=True, **kw)
    homo_r = [_venv(cfgs[a], 2, bases[a], **kw) for a in range(2)]
    mixed_r.get_state()
    for h in homo_r:
        h.get_state()
    k0 = 0
    for n in (1, 2, 3):
        out = mixed_r.rollout_device(None, n, actions=acts[k0:k0 + n])
        hout = [h.rollout_device(None, n, actions=homo_acts[a][k0:k0 + n]) for a, h in enumerate(homo_r)]
        st, hst = mixed_r.get_state(), [h.get_state() for h in homo_r]
        for b in range(B):
            a, j = b % 2, b // 2
            for key in ("rewards", "dones", "codes", "nv"):
                assert np.array_equal(out[key][:, b], hout[a][key][:, j]), ("rollout", key, b, k0)
            assert np.array_equal(mixed_r.new_drags[b], homo_r[a].new_drags[j]) and np.array_equal(mixed_r.new_lifts[b], homo_r[a].new_lifts[j])
            _same_state(_env_state(st, b), _env_state(hst[a], j), ("rollout", b, k0))
            for q in range(n):                                      # ... and the rollout == step(), to the reward's float32
                assert out["dones"][q, b] == log[k0 + q][1][b] and out["nv"][q, b] == log[k0 + q][4][b]
                assert abs(out["rewards"][q, b] - log[k0 + q][0][b]) <= 1e-6
        k0 += n
    # ---- the oracle at each setting, on the same ground truth
    threshold, margin = float(cases[0]["cfg"]["agent_params"]["threshold"]), np.inf
    z = np.load(os.path.join(GOLDEN, "ys930.npz"))
    for b in (0, 1):
        c = cases[b]
        mu, rho, dt = FLOWS[c["key"]]
        o = OracleEnv(z["coords"], z["cells"], _agent_params(), flow_params=dict(mu=mu, rho=rho), solver_params=dict(dt=dt),
                      snapshots=c["snap"])
        o.get_state()
        for k in range(S1_ORACLE_END[b] + 1):
            _, r, done, _ = o.step(int(acts[k, b]))
            rew, dn, drags, lifts, nv = log[k]
            where = ("oracle", b, k)
            err = np.abs(np.abs(o.gt_drag - o.new_drags) / o.gt_drag)
            margin = min(margin, float(np.abs(err - threshold).min()))
            print(f"oracle env {b} step {k} action {int(acts[k, b])}: done {bool(done)}, max drag error {err.max():.4e}, "
                  f"reward {r:.6f} / device {rew[b]:.6f}")
            assert bool(done) == (k == S1_ORACLE_END[b]), where              # the script ends where it says
            assert nv[b] == o.flow.mesh.nv and bool(dn[b]) == bool(done), where
            assert np.allclose(drags[b], o.new_drags, rtol=1e-7, atol=0), where
            assert np.allclose(lifts[b], o.new_lifts, rtol=1e-7, atol=0), where
            if not done:
                assert abs(rew[b] - r) <= 1e-6, (where, rew[b], r)
    print(f"oracle margin of the S1 script over all compared steps: {margin:.3e}")
    assert margin >= 1e-5, margin


# ------------------------------------------------------------------ 5: S3 flow leg
@pytest.mark.parametrize("overlap", [False, True])
def test_s3_flow_leg_of_a_mixed_flow_batch(flow_cases, overlap):
    """S3 (flow_steps=1): ys930 at a, ys930 at b and ah93w145 at c in one B = 6 batch - meshes AND constants mix.  The IPCS
    step on every coarsened mesh agrees with the homogeneous batches to 1e-9 (mode 3: LDS atomics), status words 0; one
    environment per setting against the sparse-LU oracle with that setting's mu, rho, dt, warm-started from the
    environment's last interpolated snapshot: <= 1e-7 of the force scale (the figures of the mixed-airfoil flow test)."""
    from oracle.ipcs import OracleFlowSolver
    cases = [flow_cases("ys930", "a"), flow_cases("ys930", "b"), flow_cases("ah93w145", "c")]
    cfgs, bases = [c["cfg"] for c in cases], [c["base"] for c in cases]
    B, K = 6, 4
    acts = np.random.default_rng(1370).integers(0, 181, size=(K, B))
    kw = dict(auto_reset=False, flow_steps=1, flow_rtol=1e-12, flow_overlap=overlap)
    envs = [_venv(cfgs, B, bases, mixed_flow=True, **kw)] + [_venv(cfgs[a], 2, bases[a], **kw) for a in range(3)]
    assert envs[0].flow.env_phys is envs[0].env_phys and envs[0].flow.desc.env_phys == envs[0].env_phys.data_ptr()
    res = []
    for venv, A in zip(envs, [acts] + [acts[:, a::3] for a in range(3)]):
        venv.get_state()
        for k in range(K):
            _, _, _, info = venv.step(A[k])
        fd, fl = venv.flow_wait() if overlap else (info["flow_drag"], info["flow_lift"])
        assert (venv.flow_status.cpu().numpy() == 0).all()
        assert np.isfinite(fd).all() and np.isfinite(fl).all()
        res.append((fd, fl))
    mixed = envs[0]
    for b in range(B):
        a, j = b % 3, b // 3
        assert np.allclose(res[0][0][b], res[1 + a][0][j], rtol=1e-9, atol=0), b
        assert np.allclose(res[0][1][b], res[1 + a][1][j], rtol=1e-9, atol=1e-12 * abs(res[1 + a][0][j][0])), b
    for b in (3, 4, 5):                                           # one env per setting against the oracle on its very mesh
        mu, rho, dt = FLOWS[cases[b % 3]["key"]]
        nv, nt = int(mixed.nv[b]), int(mixed.nt[b])
        n2 = nv + int(mixed.h["ne"][b])
        o = OracleFlowSolver(mixed.coords[b, :nv].copy(), mixed.cells[b, :nt].copy(), mu=mu, rho=rho, dt=dt, smooth=False)
        assert o.th.np2 == n2
        u0 = mixed.u[b, mixed.S - 1, :n2].cpu().numpy()
        o.u_n = _oracle_vel(u0)
        o.p_n = mixed.p[b, mixed.S - 1, :nv].cpu().numpy().copy()
        _, _, do, lo = o.evolve()
        scale = max(abs(do), abs(lo))
        fd, fl = res[0]
        assert abs(fd[b, 0] - do) < 1e-7 * abs(do) and abs(fl[b, 0] - lo) < 1e-7 * scale, (b, fd[b, 0], do, fl[b, 0], lo)


# ------------------------------------------------------------------ 6: refusals
def test_mixed_flow_is_opt_in_and_tables_are_checked_before_any_launch(ys930, flow_cases):
    from meshdqn_amd.vec_env import VecEnv2DAirfoil
    cases = [flow_cases("ys930", "a"), flow_cases("ys930", "b")]
    with pytest.raises(ValueError, match="mu"):
        VecEnv2DAirfoil([c["cfg"] for c in cases], 4)
    with pytest.raises(ValueError, match="mu, rho and dt must agree"):          # (handed the base environments directly)
        VecEnv2DAirfoil([cases[0]["cfg"]] * 2, 4, base_env=[c["base"] for c in cases])
    with pytest.raises(ValueError, match="^mu "):
        _batch(ys930, 4, mu=[1e-3, 1e-3, 1e-3])
    with pytest.raises(ValueError, match="^dt "):
        _batch(ys930, 4, dt=[1e-3, 1e-3, 0.0, 1e-3])


# ------------------------------------------------------------------ 7: end to end
def test_learning_loop_on_a_mixed_flow_batch(flow_cases):
    """`train_loop_device` on B = 8 environments of ys930 at a and b: finite losses and rewards."""
    import random
    from meshdqn_amd.trainer import DistContext, DQNTrainer, train_loop_device
    cases = [flow_cases("ys930", "a"), flow_cases("ys930", "b")]
    np.random.seed(5)
    random.seed(5)
    venv = _venv([c["cfg"] for c in cases], 8, [c["base"] for c in cases], mixed_flow=True)
    tr = DQNTrainer(n_actions=180, num_inputs=2 + 3 * (SOLVER_STEPS // SAVE_STEPS), ctx=DistContext(), batch_size=8, lr=1e-3)
    out = train_loop_device(tr, venv, 6, eps_decay=2, chunk=3)
    assert len(out["losses"]) >= 1 and np.isfinite(out["losses"]).all()
    assert np.isfinite(out["rewards"]).all() and out["rewards"].shape == (6, 8)


def test_train_py_with_the_mixed_flow_flag(flow_cases, tmp_path):
    """`train.py --config A --config B --mixed-flow` (the same mesh at a and b) runs to the end; the per-episode log
    `airfoil.npy` holds both config indices."""
    import yaml
    paths = []
    for c in (flow_cases("ys930", "a"), flow_cases("ys930", "b")):
        cfg = json.loads(json.dumps(c["cfg"], default=lambda v: np.asarray(v).tolist()))
        cfg["agent_params"]["timesteps"] = 3                     # episodes end every 3 steps: the log gets entries
        p = os.path.join(str(tmp_path), f"{c['key']}.yaml")
        yaml.safe_dump(cfg, open(p, "w"))
        paths.append(p)
    save = os.path.join(str(tmp_path), "run")
    cmd = [sys.executable, "train.py", "--config", paths[0], "--config", paths[1], "--mixed-flow", "--envs", "4", "--steps", "7",
           "--save-dir", save, "--save-every", "0"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run(["timeout", "-k", "10", "600"] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=660)
    assert out.returncode == 0, out.stderr[-4000:]
    af = np.load(os.path.join(save, "airfoil.npy"))
    assert len(af) >= 2 and set(af.tolist()) == {0, 1}
