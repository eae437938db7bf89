"""CPU tests of mixed-flow batches (per-environment mu, rho, dt: `mdq_ipcs_desc.env_phys`, appended within ABI 8): the
`flow_table` helper, config validation with `mixed_flow=True`, the layout of the grown descriptor against the header, and
`train.py` refusing configs that differ in `mu` without `--mixed-flow` before it touches a device."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


# ---- helper copied from tests/test_mixed_airfoils_cpu.py
def _cfg(mesh, **agent):
    ap = dict(solver_steps=5000, episodes=10, timesteps=10000, threshold=0.001, N_closest=180, gt_drag=-1, gt_time=-1,
              u=-1, p=-1, do_nothing=True, time_reward=0.005, smoothing=True, save_steps=1000, goal_vertices=0.95, plot_dir="")
    ap.update(agent)
    return dict(flow_config=dict(flow_params=dict(mu=1e-3, rho=1.0, inflow="constant"),
                                 geometry_params=dict(mesh=os.path.join(GOLDEN, f"{mesh}.npz")),
                                 solver_params=dict(dt=0.001, solver_type="lu", smooth=True)),
                agent_params=ap)


def _flow(cfg, mu=None, rho=None, dt=None):
    cfg = copy.deepcopy(cfg)
    for sec, key, val in (("flow_params", "mu", mu), ("flow_params", "rho", rho), ("solver_params", "dt", dt)):
        if val is not None:
            cfg["flow_config"][sec][key] = val
    return cfg


def test_flow_table_of_scalars_is_none():
    from meshdqn_amd.ipcs_batch import flow_table
    assert flow_table(1e-3, 1.0, 1e-3, 4) is None
    assert flow_table(np.float64(2e-3), 1, 5e-4, 1) is None


def test_flow_table_broadcasts_scalars_beside_sequences():
    from meshdqn_amd.ipcs_batch import flow_table
    t = flow_table([1e-3, 2e-3, 4e-3, 1e-3], 1.0, np.array([1e-3, 1e-3, 1e-3, 5e-4]), 4)
    assert t.dtype == np.float64 and t.shape == (4, 4) and t.flags["C_CONTIGUOUS"]
    assert np.array_equal(t, [[1e-3, 1.0, 1e-3, 0], [2e-3, 1.0, 1e-3, 0], [4e-3, 1.0, 1e-3, 0], [1e-3, 1.0, 5e-4, 0]])
    t = flow_table(1e-3, (1.0, 2.0), 1e-3, 2)                  # one sequence is enough for a table
    assert np.array_equal(t, [[1e-3, 1.0, 1e-3, 0], [1e-3, 2.0, 1e-3, 0]])
    t = flow_table([1e-3], 1.0, 1e-3, 1)                        # ... also for a batch of one
    assert np.array_equal(t, [[1e-3, 1.0, 1e-3, 0]])


@pytest.mark.parametrize("name", ["mu", "rho", "dt"])
@pytest.mark.parametrize("bad", [[1e-3, 1e-3, 1e-3], [1e-3, 0.0, 1e-3, 1e-3], [1e-3, 1e-3, -1e-3, 1e-3],
                                 [1e-3, 1e-3, 1e-3, float("nan")], [1e-3, float("inf"), 1e-3, 1e-3], [[1e-3] * 4] * 4],
                         ids=["length", "zero", "negative", "nan", "inf", "2d"])
def test_flow_table_raises_naming_the_argument(name, bad):
    from meshdqn_amd.ipcs_batch import flow_table
    args = dict(mu=1e-3, rho=1.0, dt=1e-3)
    args[name] = bad
    with pytest.raises(ValueError, match=rf"^{name} "):
        flow_table(B=4, **args)
    if np.ndim(bad) == 1 and len(bad) == 4:                     # the same values as scalars are refused too
        args[name] = [v for v in bad if not (np.isfinite(v) and v > 0)][0]
        with pytest.raises(ValueError, match=rf"^{name} "):
            flow_table(B=4, **args)


def test_mixed_flow_configs_may_differ_in_mu_rho_dt_also_on_one_mesh():
    from meshdqn_amd.vec_env import check_airfoil_configs
    a = _cfg("ys930")
    check_airfoil_configs([a, _flow(_cfg("ah93w145"), mu=2e-3, rho=2.0, dt=5e-4)], mixed_flow=True)
    check_airfoil_configs([a, _flow(a, mu=2e-3), _flow(a, rho=2.0, dt=5e-4)], mixed_flow=True)      # the same mesh thrice
    check_airfoil_configs([a, copy.deepcopy(a)], mixed_flow=True)
    for other, key in ((_flow(a, mu=2e-3), "mu"), (_flow(a, rho=2.0), "rho"), (_flow(a, dt=5e-4), "dt")):
        with pytest.raises(ValueError, match=key):              # the default stays strict: a typo in a yaml is an error
            check_airfoil_configs([a, other])
        with pytest.raises(ValueError, match=key):
            check_airfoil_configs([a, other], mixed_flow=False)


@pytest.mark.parametrize("section,key,value", [("agent_params", "N_closest", 120), ("agent_params", "save_steps", 500),
                                               ("agent_params", "solver_steps", 4000), ("flow_params", "inflow", "pulse"),
                                               ("solver_params", "smooth", False)])
def test_mixed_flow_keeps_every_other_key_batch_wide(section, key, value):
    from meshdqn_amd.vec_env import check_airfoil_configs
    a, b = _cfg("ys930"), _flow(_cfg("ys930"), mu=2e-3)
    if section == "agent_params":
        b["agent_params"][key] = value
    else:
        b["flow_config"][section][key] = value
    with pytest.raises(ValueError, match=key):
        check_airfoil_configs([a, b], mixed_flow=True)


# ---- helper copied from tests/test_mixed_airfoils_cpu.py (the header's layout through gcc)
def _c_layout(tmp_path, cname, cls):
    from meshdqn_amd import _lib
    hdr = os.path.join(os.path.dirname(_lib.HERE), "include", "meshdqn_hip.h")
    fields = [n for n, _ in cls._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{hdr}"', 'int main(){', f'printf("%zu\\n", sizeof({cname}));']
    src += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f in fields]
    src.append('return 0;}')
    cfile = tmp_path / f"{cname}.c"
    cfile.write_text("\n".join(src))
    exe = tmp_path / cname
    subprocess.check_call(["gcc", str(cfile), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    return vals[0], vals[1:], [getattr(cls, f).offset for f in fields]


def test_ipcs_desc_layout_matches_the_header_and_env_phys_is_its_last_field(tmp_path):
    """`env_phys` is appended: every earlier field keeps its offset, the new one is the struct's last (nothing but tail padding
    behind it) and the ABI version is still 8."""
    from meshdqn_amd import _lib
    cls = _lib.IpcsDesc
    size, c_off, py_off = _c_layout(tmp_path, "mdq_ipcs_desc", cls)
    assert size == C.sizeof(cls)
    assert c_off == py_off
    names = [n for n, _ in cls._fields_]
    assert names[-1] == "env_phys" and names[-2] == "status"
    assert cls.env_phys.offset == max(py_off) and cls.env_phys.offset + C.sizeof(C.c_void_p) == size
    assert cls.env_phys.offset == cls.status.offset + C.sizeof(C.c_void_p)
    assert _lib.ABI_VERSION == 8
    hdr = open(os.path.join(ROOT, "include", "meshdqn_hip.h")).read()
    assert "#define MDQ_ABI_VERSION 8" in hdr
    assert _lib.IpcsDesc().env_phys is None                     # a zero-initialised descriptor: the scalars hold


def test_no_entry_point_was_added_for_the_table():
    from meshdqn_amd import _lib, build
    assert sorted(_lib.SYMBOLS) == build.declared_symbols()
    assert not [n for n in _lib.SYMBOLS if "phys" in n or "flow_table" in n]


def test_train_py_refuses_configs_that_differ_in_mu_without_the_flag(tmp_path):
    """Two configs on the same mesh, mu 1e-3 / 2e-3, no --mixed-flow: train.py ends with the ValueError that names `mu`
    before any environment, ground truth or device work (it needs no GPU, so it runs here)."""
    import yaml
    paths = []
    for i, mu in enumerate((1e-3, 2e-3)):
        p = os.path.join(str(tmp_path), f"cfg{i}.yaml")
        yaml.safe_dump(_flow(_cfg("ys930"), mu=mu), open(p, "w"))
        paths.append(p)
    save = os.path.join(str(tmp_path), "run")
    cmd = [sys.executable, "train.py", "--config", paths[0], "--config", paths[1], "--envs", "4", "--steps", "2",
           "--save-dir", save, "--save-every", "0"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run(["timeout", "-k", "10", "120"] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=150)
    assert out.returncode not in (0, 124, 137), out.stderr[-2000:]
    assert "ValueError" in out.stderr and "flow_config.flow_params.mu" in out.stderr, out.stderr[-2000:]
    assert "--mixed-flow" in out.stderr                         # (the message says how to ask for it)
    assert not os.path.exists(save)                             # nothing was started
