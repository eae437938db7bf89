"""GPU: non-separable inflow profiles in the S3 flow leg.  `VecEnv2DAirfoil` with a callable `flow_params['inflow']` hands the
leg a static table of inlet values at the canonical inlet of every config's original mesh; on every coarsened, device-numbered
mesh `mdq_ipcs_build_inlet_map` (inlet_map_kernel) finds which dof is which inlet point and which rows touch one, and
`mdq_ipcs_evolve_fresh_profile` steps under the profile.  The map against a numpy restatement, its error codes without a fault,
the leg against the CPU oracle under the same callable on the very mesh, a mixed batch against homogeneous ones, the separable
special case against the schedule path, and an in-place reset.

Batches: ys930 under profile_a beside ah93w145 under profile_b (their inlets differ in size: the padding is exercised), B = 4,
three scripted steps.  At t = 51 dt profile_a is 5.6 x the constant parabola: a leg under the wrong inflow cannot pass.

Viscosity: mu = 1e-2, ten times the stock value.  profile_a accelerates the inflow to 5.5 x within the 50 steps of the ground
truth, and at mu = 1e-3, dt = 1e-3 the REFERENCE itself diverges on the way (the CPU oracle on ys930: max |u| 10 at step 35,
2e3 at step 40, NaN at step 48 - the explicit convection term); at mu = 1e-2 it stays regular (max |u| 8.4 at step 50, the
inflow's own peak).  Profiles, meshes, dt, step counts and bounds are untouched."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MU, RHO, DT = 1e-2, 1.0, 1e-3
SOLVER_STEPS, SAVE_STEPS = 50, 10            # S = 5 snapshots: the stock shapes without 5000 steps
B, K, FLOW_STEPS = 4, 3, 2
SCHED_C = (1.0, 0.5, 125.0, 0.0)


# ---- the profiles of tests/test_inflow_profile_gpu.py
def profile_a(x, y, t):
    return 6.0 * (0.5 + y) * (0.5 - y) * (1.0 + 0.6 * y * np.sin(2.0 * np.pi * 125.0 * t)) * (0.5 + 100.0 * t)


def profile_b(x, y, t):
    return 6.0 * (0.5 + y) * (0.5 - y) * (1.0 + 0.4 * y * np.sin(2.0 * np.pi * 50.0 * t))


def _a_c(t):
    return SCHED_C[0] * (1.0 + SCHED_C[1] * np.sin(2.0 * np.pi * SCHED_C[2] * t + SCHED_C[3]))


def profile_sep(x, y, t):
    """Schedule c spelled as a callable: a(t) * the parabola."""
    return _a_c(t) * 6.0 * (0.5 + y) * (0.5 - y)


# ---- helper copied from tests/oracle_util.py
def _oracle_vel(u):
    """device [dof][component] -> the oracle's [ux | uy]."""
    return np.concatenate([u[:, 0], u[:, 1]])


def _agent_params():
    ap = dict(json.load(open(os.path.join(GOLDEN, "oracle_stock_ys930.json")))["agent_params"])
    ap.update(solver_steps=SOLVER_STEPS, save_steps=SAVE_STEPS)
    return ap


@pytest.fixture(scope="module")
def cases(meshes, lib_built, tmp_path_factory):
    """(mesh, key) -> dict(cfg, base): the oracle's ground truth under that inflow (50 IPCS steps, every 10th kept) computed
    once and loaded through the reference's snapshot-reload branch (as `inflow_cases` of tests/test_inflow_gpu.py does), so
    that the GPU environment and the oracle share one ground truth.  Keys: "a" / "b" / "sep" the callables above, "none" the
    constant parabola, "sched" schedule c as a dict (the snapshots of "sep": the same inflow)."""
    from meshdqn_amd.env import Env2DAirfoil
    from oracle.ipcs import OracleFlowSolver
    inflows = dict(a=profile_a, b=profile_b, sep=profile_sep, none=None,
                   sched=dict(amplitude=SCHED_C[0], pulsation=SCHED_C[1], frequency=SCHED_C[2], phase=SCHED_C[3]))
    snaps, cache = {}, {}

    def snapshots(mesh, key):
        key = "sep" if key == "sched" else key
        if (mesh, key) not in snaps:
            coords, cells = meshes[mesh]
            o = OracleFlowSolver(coords, cells, mu=MU, rho=RHO, dt=DT, inflow=inflows[key])
            us, ps, drags, lifts = [], [], [], []
            for i in range(SOLVER_STEPS):
                u, p, drag, lift = o.evolve()
                if (i + 1) % SAVE_STEPS == 0:
                    us.append(u.copy()), ps.append(p.copy()), drags.append(drag), lifts.append(lift)
            snaps[(mesh, key)] = dict(gt_drag=np.array(drags), gt_lift=np.array(lifts), u=np.array(us), p=np.array(ps))
        return snaps[(mesh, key)]

    def case(mesh, key):
        if (mesh, key) in cache:
            return cache[(mesh, key)]
        snap = snapshots(mesh, key)
        tmp = str(tmp_path_factory.mktemp(f"{mesh}_{key}"))
        sdir = os.path.join(tmp, "snapshots")
        os.makedirs(sdir)
        n2 = snap["u"].shape[1] // 2
        np.save(os.path.join(sdir, "save_velocities.npy"),
                np.stack([snap["u"][:, :n2], snap["u"][:, n2:]], axis=2).reshape(len(snap["u"]), -1))
        np.save(os.path.join(sdir, "save_pressures.npy"), snap["p"])
        ap = _agent_params()
        ap.update(gt_drag=snap["gt_drag"].copy(), gt_lift=snap["gt_lift"].copy(), gt_time=np.array([SOLVER_STEPS * DT]), plot_dir=tmp)
        fp = dict(mu=MU, rho=RHO)
        if inflows[key] is not None:
            fp["inflow"] = inflows[key]
        cfg = dict(flow_config=dict(flow_params=fp, geometry_params=dict(mesh=os.path.join(GOLDEN, f"{mesh}.npz")),
                                    solver_params=dict(dt=DT, solver_type="lu", smooth=True)),
                   agent_params=ap)
        cache[(mesh, key)] = dict(cfg=cfg, base=Env2DAirfoil(cfg), profile=inflows[key])
        return cache[(mesh, key)]
    return case


def _venv(cfg, nenv, base, **kw):
    from meshdqn_amd.vec_env import VecEnv2DAirfoil
    kw.setdefault("flow_steps", FLOW_STEPS), kw.setdefault("flow_rtol", 1e-12), kw.setdefault("auto_reset", False)
    return VecEnv2DAirfoil(cfg, nenv, base_env=base, nthreads=2, **kw)


def _ab(cases):
    cs = [cases("ys930", "a"), cases("ah93w145", "b")]
    return [c["cfg"] for c in cs], [c["base"] for c in cs], [c["profile"] for c in cs]


def _actions():
    return np.random.default_rng(1370).integers(0, 181, size=(K, B))


def _roll(venv, acts, overlap):
    """The scripted steps; (drag, lift) (B, steps) of the LAST step's leg, status words checked."""
    venv.get_state()
    for k in range(acts.shape[0]):
        _, _, _, info = venv.step(acts[k])
    fd, fl = venv.flow_wait() if overlap else (info["flow_drag"], info["flow_lift"])
    torch.cuda.synchronize()
    assert (venv.flow_status.cpu().numpy() == 0).all()
    if venv.flow.map_status is not None:
        assert (venv.flow.map_status.cpu().numpy() == 0).all()
    assert np.isfinite(fd).all() and np.isfinite(fl).all()
    return fd, fl


def _close(got, ref, where):
    """The flow-leg figure between two batches (mode 3 sums with LDS atomics): 1e-9, the lift's absolute floor as in the twin
    test of tests/test_inflow_gpu.py."""
    (gd, gl), (rd, rl) = got, ref
    assert np.allclose(gd, rd, rtol=1e-9, atol=0), (where, gd, rd)
    assert np.allclose(gl, rl, rtol=1e-9, atol=1e-12 * np.abs(rd).max()), (where, gl, rl)


# ------------------------------------------------------------------ the map
class _Guarded:
    """The output arrays of mdq_ipcs_build_inlet_map carved out of ONE int32 buffer with guard cells behind each."""
    GUARD, SENT = 64, -777

    def __init__(self, nenv, NIN, NIR):
        sizes = dict(n_inlet=nenv, inlet_dofs=nenv * NIN, n_rows=nenv, rows=nenv * NIR, map_status=nenv)
        self.shape = dict(n_inlet=(nenv,), inlet_dofs=(nenv, NIN), n_rows=(nenv,), rows=(nenv, NIR), map_status=(nenv,))
        self.buf = torch.full((sum(sizes.values()) + self.GUARD * (len(sizes) + 1),), self.SENT, dtype=torch.int32, device="cuda")
        self.off, o = {}, self.GUARD
        for k, n in sizes.items():
            self.off[k] = (o, n)
            o += n + self.GUARD
        self.view("map_status").zero_()

    def view(self, k):
        o, n = self.off[k]
        return self.buf[o:o + n]

    def ptr(self, k):
        return self.view(k).data_ptr()

    def read(self):
        h = self.buf.cpu().numpy()
        live = np.zeros(h.size, bool)
        out = {}
        for k, (o, n) in self.off.items():
            live[o:o + n] = True
            out[k] = h[o:o + n].reshape(self.shape[k]).copy()
        assert (h[~live] == self.SENT).all(), "a guard cell was overwritten"
        return out


def _build_map(venv, n_ref, inlet_y, NIR):
    from meshdqn_amd import _lib
    NIN = inlet_y.shape[1]
    g = _Guarded(venv.B, NIN, NIR)
    nr, iy = torch.from_numpy(np.ascontiguousarray(n_ref, np.int32)).cuda(), torch.from_numpy(np.ascontiguousarray(inlet_y)).cuda()
    _lib.check(_lib.load().mdq_ipcs_build_inlet_map(C.byref(venv.flow.desc), NIN, NIR, nr.data_ptr(), iy.data_ptr(),
                                                    g.ptr("n_inlet"), g.ptr("inlet_dofs"), g.ptr("n_rows"), g.ptr("rows"),
                                                    g.ptr("map_status"), _lib.stream_ptr()), "mdq_ipcs_build_inlet_map")
    torch.cuda.synchronize()
    return g.read()


@pytest.fixture(scope="module")
def mapped(cases):
    """The mixed batch after the scripted steps, its topology run once more (bcu_gx is the constant parabola again: what the
    leg's map kernel sees, before any profile step), the mesh data downloaded, and the numpy restatement of the map."""
    cfgs, bases, _ = _ab(cases)
    venv = _venv(cfgs, B, bases, mixed_inflow=True)
    _roll(venv, _actions(), False)
    leg_map = {k: v.cpu().numpy() for k, v in venv.flow.inlet_map.items()}          # the last leg's own map
    venv.dtopo.run(check=True)
    torch.cuda.synchronize()
    dt = venv.dtopo
    cd, coords = dt.t["cell_dofs"].cpu().numpy(), dt.coords.cpu().numpy()
    flag, gx = dt.ti["bcu_flag"].cpu().numpy(), dt.ti["bcu_gx"].cpu().numpy()
    nv, nt, ne = dt.nv.cpu().numpy(), dt.nt.cpu().numpy(), dt.t["ne"].cpu().numpy()
    want = []
    for b in range(B):
        n2, c, x = nv[b] + ne[b], cd[b][:, :nt[b]].T, coords[b]
        inlet = np.zeros(n2, bool)
        inlet[:] = (flag[b, :n2] != 0) & (gx[b, :n2] != 0)
        y = np.full(n2, np.nan)
        y[:nv[b]] = x[:nv[b], 1]
        for k, (ea, eb) in enumerate(((1, 2), (0, 2), (0, 1))):
            y[c[:, 3 + k]] = 0.5 * (x[c[:, ea], 1] + x[c[:, eb], 1])
        ids = np.flatnonzero(inlet)
        touched = np.unique(c[inlet[c].any(axis=1)])
        want.append(dict(dofs=ids[np.argsort(y[ids], kind="stable")], rows=touched[flag[b, touched] == 0], y=y))
    ip = {k: v.cpu().numpy() for k, v in venv.flow.inflow_profile.items()}
    return dict(venv=venv, want=want, ip=ip, leg_map=leg_map)


def _check_env(got, b, w, NIN, NIR):
    ni, nr = len(w["dofs"]), len(w["rows"])
    assert got["n_inlet"][b] == ni and got["n_rows"][b] == nr, b
    assert np.array_equal(got["inlet_dofs"][b, :ni], w["dofs"]) and (got["inlet_dofs"][b, ni:] == -1).all(), b
    assert np.array_equal(got["rows"][b, :nr], w["rows"]) and (got["rows"][b, nr:] == -1).all(), b
    assert got["map_status"][b] == 0, b


def test_inlet_map_equals_the_numpy_restatement(mapped):
    venv, want, ip = mapped["venv"], mapped["want"], mapped["ip"]
    NIN, NIR = ip["inlet_y"].shape[1], venv.NP
    got = _build_map(venv, ip["n_ref"], ip["inlet_y"], NIR)
    assert ip["n_ref"][0] != ip["n_ref"][1] and NIN == ip["n_ref"].max()              # the padding is exercised
    for b in range(B):
        w = want[b]
        _check_env(got, b, w, NIN, NIR)
        assert got["n_inlet"][b] == ip["n_ref"][b]
        ys = w["y"][got["inlet_dofs"][b, :ip["n_ref"][b]]]
        assert np.array_equal(ys.view(np.uint64), ip["inlet_y"][b, :ip["n_ref"][b]].view(np.uint64)), b     # bit for bit
        assert len(w["rows"]) > len(w["dofs"]) and (np.diff(w["rows"]) > 0).all()
        print(f"env {b}: {len(w['dofs'])} inlet dofs, {len(w['rows'])} rows")
    for k in ("n_inlet", "inlet_dofs", "n_rows", "rows"):                              # the leg's own map of the same meshes
        assert np.array_equal(mapped["leg_map"][k], got[k]), k


def test_inlet_map_error_codes_leave_the_other_environments_alone(mapped):
    venv, want, ip = mapped["venv"], mapped["want"], mapped["ip"]
    NIN, NP = ip["inlet_y"].shape[1], venv.NP
    n_bad = ip["n_ref"].copy()
    n_bad[1] -= 1
    y_bad = ip["inlet_y"].copy()
    y_bad[1] += 1e-3
    nir_small = len(want[1]["rows"]) - 1
    for code, (n_ref, inlet_y, NIR) in enumerate([(n_bad, ip["inlet_y"], NP), (ip["n_ref"], y_bad, NP),
                                                   (ip["n_ref"], ip["inlet_y"], nir_small)], 1):
        got = _build_map(venv, n_ref, inlet_y, NIR)
        fails = [b for b in range(B) if code == 3 and len(want[b]["rows"]) > NIR] if code == 3 else [1]
        assert 1 in fails
        for b in range(B):
            if b in fails:
                assert got["map_status"][b] == code, (code, b, got["map_status"])
                assert got["n_inlet"][b] == 0 and got["n_rows"][b] == 0, (code, b)
                assert (got["inlet_dofs"][b] == -1).all() and (got["rows"][b] == -1).all(), (code, b)
            else:
                _check_env(got, b, want[b], NIN, NIR)


def test_entry_points_refuse_bad_arguments_before_any_launch(mapped):
    from meshdqn_amd import _lib
    venv, ip = mapped["venv"], mapped["ip"]
    lib = _lib.load()
    g = _Guarded(B, 65, 8)
    z = torch.zeros(B * 65, dtype=torch.float64, device="cuda")
    args = (z.data_ptr(), z.data_ptr(), g.ptr("n_inlet"), g.ptr("inlet_dofs"), g.ptr("n_rows"), g.ptr("rows"), g.ptr("map_status"),
            _lib.stream_ptr())
    assert lib.mdq_ipcs_build_inlet_map(C.byref(venv.flow.desc), 65, 8, *args) != 0 and b"NIN" in lib.mdq_last_error()
    assert lib.mdq_ipcs_build_inlet_map(C.byref(venv.flow.desc), 8, 0, *args) != 0
    assert lib.mdq_ipcs_build_inlet_map(C.byref(venv.flow.desc), 8, 8, None, *args[1:]) != 0 and b"null table" in lib.mdq_last_error()
    pr = _lib.InflowProfile()
    pr.NIN, pr.NIR = 8, 8                                                              # no tables
    out = torch.zeros((2, B, FLOW_STEPS), dtype=torch.float64, device="cuda")
    rc = lib.mdq_ipcs_evolve_fresh_profile(C.byref(venv.flow.desc), FLOW_STEPS, out[0].data_ptr(), out[1].data_ptr(), None,
                                           C.byref(pr), _lib.stream_ptr())
    assert rc != 0 and b"incomplete inflow profile" in lib.mdq_last_error()
    torch.cuda.synchronize()
    g.read()                                                                            # nothing was written


# ------------------------------------------------------------------ the leg
@pytest.fixture(scope="module")
def legs(cases):
    """overlap -> (mixed environment, its leg's forces, the forces of the homogeneous B = 2 batch of each config), run once."""
    cfgs, bases, _ = _ab(cases)
    cache = {}

    def run(overlap):
        if overlap not in cache:
            acts = _actions()
            mixed = _venv(cfgs, B, bases, mixed_inflow=True, flow_overlap=overlap)
            res = _roll(mixed, acts, overlap)
            homo = []
            for a in range(2):
                h = _venv(cfgs[a], 2, bases[a], flow_overlap=overlap)               # a single config with a callable: no flag
                homo.append(_roll(h, acts[:, a::2], overlap))
            cache[overlap] = (mixed, res, homo)
        return cache[overlap]
    return run


def _against_oracle(mixed, fd, fl, profiles, tag):
    """One environment per config against `OracleFlowSolver(inflow=profile)` on its very mesh, warm-started from the
    environment's last interpolated snapshot, gtime = solver_steps dt: drag and lift of BOTH steps within 1e-7 of the force
    scale (the flow-leg figure)."""
    from oracle.ipcs import OracleFlowSolver
    for b in (2, 3):
        nv, nt = int(mixed.nv[b]), int(mixed.nt[b])
        n2 = nv + int(mixed.h["ne"][b])
        o = OracleFlowSolver(mixed.coords[b, :nv].copy(), mixed.cells[b, :nt].copy(), inflow=profiles[b % 2], mu=MU, rho=RHO,
                             dt=DT, smooth=False)
        assert o.th.np2 == n2
        o.u_n = _oracle_vel(mixed.u[b, mixed.S - 1, :n2].cpu().numpy())
        o.p_n = mixed.p[b, mixed.S - 1, :nv].cpu().numpy().copy()
        o.gtime = SOLVER_STEPS * DT                               # the steps run at t = 51 dt, 52 dt
        for s in range(FLOW_STEPS):
            _, _, do, lo = o.evolve()
            scale = max(abs(do), abs(lo))
            print(f"{tag} env {b} step {s}: drag {fd[b, s]:.10g} / oracle {do:.10g} ({abs(fd[b, s] - do) / abs(do):.2e}), "
                  f"lift {fl[b, s]:.10g} / {lo:.10g} ({abs(fl[b, s] - lo) / scale:.2e} of the scale)")
            assert abs(fd[b, s] - do) < 1e-7 * abs(do) and abs(fl[b, s] - lo) < 1e-7 * scale, (b, s, fd[b, s], do, fl[b, s], lo)


@pytest.mark.parametrize("overlap", [False, True])
def test_s3_flow_leg_under_a_callable_matches_the_oracle(cases, legs, overlap):
    mixed, (fd, fl), _ = legs(overlap)
    _, _, profiles = _ab(cases)
    ip = mixed.flow.inflow_profile
    assert set(ip) == {"n_ref", "inlet_y", "values"} and ip["values"].shape[:2] == (B, FLOW_STEPS)
    assert mixed.flow.inflow_scale is None and fd.shape == (B, FLOW_STEPS)
    _against_oracle(mixed, fd, fl, profiles, f"overlap {overlap}")


def test_s3_flow_leg_on_the_host_index_engine_matches_the_oracle(cases):
    """The same batch with the HOST topology engine (its index arrays are copied into the leg's): the map kernel reads the
    same descriptor fields, whoever filled them."""
    cfgs, bases, profiles = _ab(cases)
    mixed = _venv(cfgs, B, bases, mixed_inflow=True, gpu_topology=False)
    assert mixed.flow.host_index and mixed.flow.inflow_profile is not None
    fd, fl = _roll(mixed, _actions(), False)
    _against_oracle(mixed, fd, fl, profiles, "host engine")


@pytest.mark.parametrize("overlap", [False, True])
def test_mixed_profile_batch_equals_the_homogeneous_batches(legs, overlap):
    _, (fd, fl), homo = legs(overlap)
    for b in range(B):
        a, j = b % 2, b // 2
        _close((fd[b], fl[b]), (homo[a][0][j], homo[a][1][j]), (overlap, b))
    assert abs(fd[0, 0] - fd[2, 0]) > 1e-6 * abs(fd[0, 0])                     # same config, other actions: other meshes


def test_separable_callable_equals_the_schedule_and_none_equals_the_plain_leg(cases):
    """[ys930 under schedule c spelled as a callable, ys930 under no inflow key] as one mixed batch: the callable's environments
    against the batch of the same schedule given as a dict (the factor path, no table of values), the `None` environments -
    which ride through the profile's table with the parabola's values - against the plain batch: 1e-9 each."""
    sep, none, sched = cases("ys930", "sep"), cases("ys930", "none"), cases("ys930", "sched")
    acts = _actions()
    mixed = _venv([sep["cfg"], none["cfg"]], B, [sep["base"], none["base"]], mixed_inflow=True)
    assert mixed.flow.inflow_profile is not None and mixed.flow.inflow_scale is None
    got = _roll(mixed, acts, False)
    refs = []
    for a, c in enumerate((sched, none)):
        h = _venv(c["cfg"], 2, c["base"])
        assert h.flow.inflow_profile is None and (h.flow.inflow_scale is None) == (a == 1)
        refs.append(_roll(h, acts[:, a::2], False))
    for b in range(B):
        a, j = b % 2, b // 2
        _close((got[0][b], got[1][b]), (refs[a][0][j], refs[a][1][j]), b)
    assert abs(_a_c(51 * DT) - 1.0) > 0.3 and abs(got[0][0, 0] - got[0][1, 0]) > 1e-3 * abs(got[0][1, 0])


def test_leg_after_an_in_place_reset(cases):
    """auto_reset: environment 1's episode ends at the second step (an action outside the selection), the third step's leg
    runs on its restarted mesh - finite, status words 0, and 1e-9 from the homogeneous batches run through the same script."""
    cfgs, bases, _ = _ab(cases)
    acts = _actions()
    acts[1, 1] = -1
    mixed = _venv(cfgs, B, bases, mixed_inflow=True, auto_reset=True)
    mixed.get_state()
    dones = [mixed.step(acts[k])[2] for k in range(2)]
    assert dones[1][1] and mixed.nv[1] == mixed.nv0s[1] and mixed.steps[1] == 0      # restarted in place
    _, _, _, info = mixed.step(acts[2])
    got = (info["flow_drag"], info["flow_lift"])
    torch.cuda.synchronize()
    assert (mixed.flow_status.cpu().numpy() == 0).all() and (mixed.flow.map_status.cpu().numpy() == 0).all()
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    for a in range(2):
        h = _venv(cfgs[a], 2, bases[a], auto_reset=True)
        ref = _roll(h, acts[:, a::2], False)
        for j in range(2):
            _close((got[0][2 * j + a], got[1][2 * j + a]), (ref[0][j], ref[1][j]), (a, j))
