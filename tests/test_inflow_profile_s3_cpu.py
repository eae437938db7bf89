"""CPU: the host side of non-separable inflow profiles in the S3 flow leg - the canonical inlet of a base mesh
(`inflow.canonical_inlet`), the leg's static table (`inflow.leg_profile_table`), the predicate that refuses a leg outside
operator mode 3 and the argument validation of `FlowLeg(inflow_profile=...)` (`flow_leg.check_leg_profile`, which needs no
device)."""
import numpy as np
import pytest

NAMES = ("ys930", "ah93w145")
SOLVER_STEPS, FLOW_STEPS = 50, 2
DTS = [1e-3, 5e-4]
SCHED = (0.8, 0.3, 50.0, 1.0)


def profile_a(x, y, t):
    return 6.0 * (0.5 + y) * (0.5 - y) * (1.0 + 0.6 * y * np.sin(2.0 * np.pi * 125.0 * t)) * (0.5 + 100.0 * t)


@pytest.fixture(scope="module")
def inlets(meshes):
    from meshdqn_amd.inflow import canonical_inlet, inlet_tables
    from meshdqn_amd.topology import MeshTopology
    out = []
    for n in NAMES:
        t = MeshTopology(*meshes[n])
        out.append(dict(topo=t, can=canonical_inlet(t, t.coords), tab=inlet_tables([t], [t.coords])[0]))
    return out


def test_canonical_inlet_is_the_inlet_table_sorted_by_y(inlets):
    assert len(inlets[0]["can"]["y"]) != len(inlets[1]["can"]["y"])           # the two airfoils exercise the padding
    for c in inlets:
        can, tab, t = c["can"], c["tab"], c["topo"]
        n = len(tab["dofs"])
        assert n > 2 and all(len(can[k]) == n for k in ("dofs", "xy", "gx0", "y"))
        assert (np.diff(can["y"]) > 0).all()
        assert sorted(can["dofs"].tolist()) == tab["dofs"].tolist()
        xy = t.dof_coords(t.coords)
        assert np.array_equal(can["xy"], xy[can["dofs"]]) and np.array_equal(can["y"], can["xy"][:, 1])
        assert (can["xy"][:, 0] == t.coords[:, 0].min()).all()
        bot, top = t.coords[:, 1].min(), t.coords[:, 1].max()
        y = can["y"]
        assert np.array_equal(can["gx0"], -4.0 * 1.5 * (y - bot) * (y - top) / (top - bot) / (top - bot))   # the parabola
        assert (can["gx0"] != 0).all() and bot < y[0] and y[-1] < top           # the overridden corners are not in it


def test_leg_table_times_gather_and_the_three_kinds(inlets):
    from meshdqn_amd.inflow import inflow_factors, leg_profile_table
    cans = [c["can"] for c in inlets]
    # three configs: a callable on ys930, a schedule on ah93w145, None on ys930
    cfg_inlets, profs, specs, dts = [cans[0], cans[1], cans[0]], [profile_a, None, None], [None, SCHED, None], [DTS[0], DTS[1], DTS[0]]
    airfoil = np.array([0, 1, 2, 1, 0], np.int32)
    tab = leg_profile_table(cfg_inlets, profs, specs, dts, airfoil, SOLVER_STEPS, FLOW_STEPS)
    n = [len(c["y"]) for c in cfg_inlets]
    NIN = max(n)
    assert tab["values"].shape == (5, FLOW_STEPS, NIN) and tab["inlet_y"].shape == (5, NIN)
    assert tab["n_ref"].dtype == np.int32 and tab["n_ref"].tolist() == [n[a] for a in airfoil]
    for k in ("n_ref", "inlet_y", "values"):
        assert tab[k].flags["C_CONTIGUOUS"]
    for b, a in enumerate(airfoil):
        c = cfg_inlets[a]
        assert np.array_equal(tab["inlet_y"][b, :n[a]], c["y"]) and (tab["inlet_y"][b, n[a]:] == 0).all()
        assert (tab["values"][b, :, n[a]:] == 0).all()
        for s in range(FLOW_STEPS):
            got = tab["values"][b, s, :n[a]]
            if a == 0:          # the callable at t = (solver_steps + s + 1) dt of its config
                t = float(SOLVER_STEPS + s + 1) * dts[a]
                assert np.array_equal(got, profile_a(c["xy"][:, 0], c["xy"][:, 1], t))
            elif a == 1:        # the schedule: its factor times the parabola, bit for bit
                f = inflow_factors(SCHED, dts[a], SOLVER_STEPS, FLOW_STEPS)[0, s]
                assert np.array_equal(got, f * c["gx0"]) and f != 1.0
            else:               # None: the parabola
                assert np.array_equal(got, c["gx0"])
    assert np.array_equal(tab["values"][0], tab["values"][4]) and np.array_equal(tab["values"][1], tab["values"][3])


def test_leg_table_refuses_a_profile_that_is_not_finite_or_has_the_wrong_shape(inlets):
    from meshdqn_amd.inflow import leg_profile_table
    cans = [c["can"] for c in inlets]
    t_bad = float(SOLVER_STEPS + 2) * DTS[0]

    def blows_up(x, y, t):
        return np.where(t == t_bad, np.nan, 1.0) * profile_a(x, y, t)

    with pytest.raises(ValueError, match=r"config 1 at step 1 .*not finite"):
        leg_profile_table(cans, [profile_a, blows_up], [None, None], [DTS[0], DTS[0]], np.array([0, 1]), SOLVER_STEPS, FLOW_STEPS)
    with pytest.raises(ValueError, match=r"config 0 at step 0 .*shape"):
        leg_profile_table(cans, [lambda x, y, t: 1.0, None], [None, None], DTS, np.array([0, 1]), SOLVER_STEPS, FLOW_STEPS)
    with pytest.raises(ValueError, match="per config"):
        leg_profile_table(cans, [profile_a], [None, None], DTS, np.array([0, 1]), SOLVER_STEPS, FLOW_STEPS)


def test_profile_leg_predicate_is_the_mode_3_limit():
    from meshdqn_amd.flow_leg import profile_leg_refusal
    # mode 3 keeps three velocity vectors in LDS: 3 402 rows, not the 3 584 of its row loops (ipcs_batch.operator_mode_limits)
    assert profile_leg_refusal(3402) is None and profile_leg_refusal(3322) is None
    for np_ in (3403, 3584, 3585):
        why = profile_leg_refusal(np_)
        assert why is not None and "per-step path" in why and str(np_) in why and "> 3402" in why


class _FakeDev:
    type = "cuda"


def _fake(shape, dtype):
    """A CPU tensor that reports a device of type 'cuda': the validation only inspects the tensors."""
    import torch

    class T(torch.Tensor):
        device = _FakeDev()
    return torch.zeros(shape, dtype=dtype).as_subclass(T)


def test_flow_leg_argument_validation():
    import torch
    from meshdqn_amd.flow_leg import check_leg_profile
    B, steps, NIN, NP = 4, 2, 13, 3322

    def prof(**over):
        p = dict(n_ref=_fake((B,), torch.int32), inlet_y=_fake((B, NIN), torch.float64), values=_fake((B, steps, NIN), torch.float64))
        p.update(over)
        return p

    check_leg_profile(prof(), None, B, steps, NP)                                               # the good one passes
    with pytest.raises(ValueError, match="mutually exclusive"):
        check_leg_profile(prof(), _fake((B, steps), torch.float64), B, steps, NP)
    with pytest.raises(ValueError, match="per-step path"):
        check_leg_profile(prof(), None, B, steps, 3585)
    with pytest.raises(ValueError, match=r"inflow_profile\['values'\]"):
        check_leg_profile(prof(values=_fake((B, steps + 1, NIN), torch.float64)), None, B, steps, NP)
    with pytest.raises(ValueError, match=r"inflow_profile\['values'\]"):
        check_leg_profile(prof(values=_fake((B, steps, NIN), torch.float32)), None, B, steps, NP)
    with pytest.raises(ValueError, match=r"inflow_profile\['n_ref'\]"):
        check_leg_profile(prof(n_ref=_fake((B,), torch.int64)), None, B, steps, NP)
    with pytest.raises(ValueError, match=r"inflow_profile\['inlet_y'\]"):
        check_leg_profile(prof(inlet_y=_fake((NIN, B), torch.float64).t()), None, B, steps, NP)  # not contiguous
    with pytest.raises(ValueError, match=r"inflow_profile\['n_ref'\]"):
        check_leg_profile(prof(n_ref=torch.zeros(B, dtype=torch.int32)), None, B, steps, NP)    # a host tensor
    with pytest.raises(ValueError, match="keys"):
        check_leg_profile(dict(values=_fake((B, steps, NIN), torch.float64)), None, B, steps, NP)
    with pytest.raises(ValueError, match="holds 64"):
        check_leg_profile(dict(n_ref=_fake((B,), torch.int32), inlet_y=_fake((B, 65), torch.float64),
                               values=_fake((B, steps, 65), torch.float64)), None, B, steps, NP)


def test_map_status_error_names_the_environments_and_the_code():
    from meshdqn_amd._lib import MeshDQNHipError
    from meshdqn_amd.flow_leg import check_flow_forces
    ok = np.ones((3, 2))
    check_flow_forces(ok, ok, "here", np.zeros(3, np.int32), np.zeros(3, np.int32))
    with pytest.raises(MeshDQNHipError) as e:
        check_flow_forces(ok, ok, "here", np.zeros(3, np.int32), np.array([0, 2, 0], np.int32))
    msg = str(e.value)
    assert "inlet map" in msg and "[1]" in msg and "code 2" in msg and "y differs" in msg and "team barrier" not in msg
