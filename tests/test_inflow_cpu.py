"""CPU tests of inflow schedules (per-environment, time-dependent separable inflow a(t) * parabola: `meshdqn_amd/inflow.py`,
`mdq_ipcs_evolve_inflow`): the spec parser, the factor table against the closed form, config validation with
`mixed_inflow=True`, `train.py` refusing configs that differ in `inflow` without `--mixed-inflow` before it touches a device,
and the new entry point within ABI 8."""
import copy
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# the schedules (amplitude, pulsation, frequency [Hz], phase [rad]) of the issue
SCHED = dict(a=(1.0, 0.0, 0.0, 0.0), b=(0.5, 0.0, 0.0, 0.0), c=(1.0, 0.5, 125.0, 0.0), d=(0.8, 0.3, 50.0, 1.0))


def _dict(s):
    return dict(amplitude=s[0], pulsation=s[1], frequency=s[2], phase=s[3])


# ---- helper copied from tests/test_mixed_airfoils_cpu.py
def _cfg(mesh, **agent):
    ap = dict(solver_steps=5000, episodes=10, timesteps=10000, threshold=0.001, N_closest=180, gt_drag=-1, gt_time=-1,
              u=-1, p=-1, do_nothing=True, time_reward=0.005, smoothing=True, save_steps=1000, goal_vertices=0.95, plot_dir="")
    ap.update(agent)
    return dict(flow_config=dict(flow_params=dict(mu=1e-3, rho=1.0, inflow="constant"),
                                 geometry_params=dict(mesh=os.path.join(GOLDEN, f"{mesh}.npz")),
                                 solver_params=dict(dt=0.001, solver_type="lu", smooth=True)),
                agent_params=ap)


def _inflow(cfg, inflow):
    cfg = copy.deepcopy(cfg)
    cfg["flow_config"]["flow_params"]["inflow"] = inflow
    return cfg


# ------------------------------------------------------------------ inflow_spec
def test_inflow_spec_defaults_and_constant():
    from meshdqn_amd.inflow import inflow_spec
    assert inflow_spec("constant") is None and inflow_spec(None) is None
    assert inflow_spec({}) == (1.0, 0.0, 0.0, 0.0)
    assert inflow_spec(dict(amplitude=0.5)) == (0.5, 0.0, 0.0, 0.0)
    assert inflow_spec(dict(amplitude=0.5, pulsation=0.2, frequency=2.0)) == (0.5, 0.2, 2.0, 0.0)
    assert inflow_spec(dict(pulsation=-0.25, phase=-1)) == (1.0, -0.25, 0.0, -1.0)
    assert inflow_spec(_dict(SCHED["d"])) == SCHED["d"]
    assert inflow_spec(SCHED["d"]) == SCHED["d"]                  # what the function returned passes through
    assert all(type(v) is float for v in inflow_spec(dict(amplitude=2, frequency=3)))


@pytest.mark.parametrize("bad,key", [(dict(amplitude=1.0, ampltude=2.0), "ampltude"), (dict(gust=1.0), "gust"),
                                     (dict(amplitude=float("nan")), "amplitude"), (dict(amplitude=float("inf")), "amplitude"),
                                     (dict(amplitude=0.0), "amplitude"), (dict(amplitude=-1.0), "amplitude"),
                                     (dict(amplitude="1"), "amplitude"), (dict(frequency=-2.0), "frequency"),
                                     (dict(frequency=float("inf")), "frequency"), (dict(pulsation=float("nan")), "pulsation"),
                                     (dict(phase=float("inf")), "phase"), (dict(phase=None), "phase")])
def test_inflow_spec_raises_value_error_naming_the_key(bad, key):
    from meshdqn_amd.inflow import inflow_spec
    with pytest.raises(ValueError, match=key):
        inflow_spec(bad)


@pytest.mark.parametrize("bad", ["ramp", "pulse", 1.5, [1.0, 0.0, 0.0, 0.0], (1.0, 0.0)])
def test_inflow_spec_raises_type_error_for_other_strings_and_types(bad):
    from meshdqn_amd.inflow import inflow_spec
    with pytest.raises(TypeError):
        inflow_spec(bad)


# ------------------------------------------------------------------ inflow_factors
def _closed_form(s, dt, k):
    A, eps, f, phi = s
    return A * (1.0 + eps * math.sin(2.0 * math.pi * f * (k * dt) + phi))


def test_inflow_factors_match_the_closed_form_with_per_environment_dt():
    from meshdqn_amd.inflow import inflow_factors
    specs = [SCHED[k] for k in "abcd"]
    dts = np.array([1e-3, 1e-3, 5e-4, 2e-3])
    F = inflow_factors(specs, dts, 0, 8)
    assert F.dtype == np.float64 and F.shape == (4, 8) and F.flags["C_CONTIGUOUS"]
    for b, s in enumerate(specs):
        for j in range(8):
            want = _closed_form(s, dts[b], j + 1)                 # the clock is advanced BEFORE the solve: s = 1 .. n
            assert abs(F[b, j] - want) <= 4 * np.finfo(float).eps * abs(want), (b, j)
    assert np.array_equal(F[0], np.ones(8)) and np.array_equal(F[1], np.full(8, 0.5))
    # schedule c at dt 5e-4: period 16 steps, sin(pi / 8 * k)
    assert abs(F[2, 3] - (1.0 + 0.5 * math.sin(math.pi / 2))) < 1e-15 and abs(F[2, 7] - 1.0) < 1e-15
    # one spec and a scalar dt; dicts in place of specs; None rows are ones
    assert np.array_equal(inflow_factors(SCHED["d"], 1e-3, 0, 8), inflow_factors([SCHED["d"]], [1e-3], 0, 8))
    G = inflow_factors([None, _dict(SCHED["d"]), "constant"], 1e-3, 5, 2)
    assert G.shape == (3, 2) and np.array_equal(G[0], [1.0, 1.0]) and np.array_equal(G[2], [1.0, 1.0])
    assert np.array_equal(G[1], inflow_factors(SCHED["d"], 1e-3, 0, 8)[0, 5:7])


def test_inflow_factors_of_split_launches_are_bitwise_the_factors_of_one():
    from meshdqn_amd.inflow import inflow_factors
    specs = [SCHED[k] for k in "abcd"]
    dts = np.array([1e-3, 1e-3, 5e-4, 1e-3])
    whole = inflow_factors(specs, dts, 0, 8)
    parts = np.concatenate([inflow_factors(specs, dts, 0, 3), inflow_factors(specs, dts, 3, 5)], axis=1)
    assert np.array_equal(whole, parts)


def test_inflow_factors_of_all_none_specs_is_none():
    from meshdqn_amd.inflow import inflow_factors
    assert inflow_factors([None, None, "constant"], 1e-3, 0, 4) is None
    assert inflow_factors(None, [1e-3, 2e-3], 0, 4) is None


# ------------------------------------------------------------------ configs
def test_mixed_inflow_configs_may_differ_in_inflow_also_on_one_mesh():
    from meshdqn_amd.vec_env import check_airfoil_configs
    a = _cfg("ys930")
    d = _inflow(a, _dict(SCHED["d"]))
    check_airfoil_configs([a, d], mixed_inflow=True)                                        # one mesh, two schedules
    check_airfoil_configs([a, d, _inflow(a, dict(amplitude=0.5))], mixed_inflow=True)
    check_airfoil_configs([a, _inflow(_cfg("ah93w145"), _dict(SCHED["c"]))], mixed_inflow=True)
    check_airfoil_configs([d, copy.deepcopy(d)])                                            # the same schedule: no flag needed
    for kw in (dict(), dict(mixed_inflow=False), dict(mixed_flow=True)):                    # its own opt-in
        with pytest.raises(ValueError, match="inflow") as e:
            check_airfoil_configs([a, d], **kw)
        assert "flow_config.flow_params.inflow" in str(e.value)
        assert "mixed_inflow=True / --mixed-inflow" in str(e.value)
    with pytest.raises(ValueError, match="inflow"):                                         # two schedules differ as well
        check_airfoil_configs([d, _inflow(a, _dict(SCHED["c"]))])


@pytest.mark.parametrize("section,key,value", [("agent_params", "N_closest", 120), ("agent_params", "save_steps", 500),
                                               ("agent_params", "solver_steps", 4000), ("flow_params", "inflow_profile", "x"),
                                               ("solver_params", "smooth", False), ("solver_params", "solver_type", "la_solve")])
def test_both_flags_keep_every_other_key_batch_wide(section, key, value):
    from meshdqn_amd.vec_env import check_airfoil_configs
    a, b = _cfg("ys930"), _inflow(_cfg("ys930"), _dict(SCHED["d"]))
    b["flow_config"]["flow_params"]["mu"] = 2e-3
    check_airfoil_configs([a, b], mixed_flow=True, mixed_inflow=True)
    if section == "agent_params":
        b["agent_params"][key] = value
    else:
        b["flow_config"][section][key] = value
    with pytest.raises(ValueError, match=key):
        check_airfoil_configs([a, b], mixed_flow=True, mixed_inflow=True)
    with pytest.raises(ValueError, match="mu"):                                             # mu needs ITS flag
        check_airfoil_configs([_cfg("ys930"), _inflow(b, "constant")], mixed_inflow=True)


def test_train_py_refuses_configs_that_differ_in_inflow_without_the_flag(tmp_path):
    """Two configs on the same mesh, constant inflow / schedule d, no --mixed-inflow: train.py ends with the ValueError that
    names `flow_config.flow_params.inflow` before any environment, ground truth or device work (it needs no GPU)."""
    import yaml
    paths = []
    for i, inflow in enumerate(("constant", dict(amplitude=0.5, pulsation=0.2, frequency=2.0))):
        p = os.path.join(str(tmp_path), f"cfg{i}.yaml")
        yaml.safe_dump(_inflow(_cfg("ys930"), inflow), open(p, "w"))
        paths.append(p)
    save = os.path.join(str(tmp_path), "run")
    cmd = [sys.executable, "train.py", "--config", paths[0], "--config", paths[1], "--envs", "4", "--steps", "2",
           "--save-dir", save, "--save-every", "0"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run(["timeout", "-k", "10", "120"] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=150)
    assert out.returncode not in (0, 124, 137), out.stderr[-2000:]
    assert "ValueError" in out.stderr and "flow_config.flow_params.inflow" in out.stderr, out.stderr[-2000:]
    assert "--mixed-inflow" in out.stderr                       # (the message says how to ask for it)
    assert not os.path.exists(save)                             # nothing was started


# ------------------------------------------------------------------ ABI
def test_the_inflow_entry_point_is_declared_within_abi_8():
    from meshdqn_amd import _lib, build
    assert "mdq_ipcs_evolve_inflow" in _lib.SYMBOLS
    assert "mdq_ipcs_evolve_inflow" in build.declared_symbols()
    assert sorted(_lib.SYMBOLS) == build.declared_symbols()
    assert _lib.ABI_VERSION == 8
    restype, argtypes = _lib.SYMBOLS["mdq_ipcs_evolve_inflow"]
    assert len(argtypes) == len(_lib.SYMBOLS["mdq_ipcs_evolve"][1]) + 1       # mdq_ipcs_evolve + the table
