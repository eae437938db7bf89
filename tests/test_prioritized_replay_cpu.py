"""Prioritized replay without a GPU: the numpy restatement of the three kernels (tests/per_ref.py) against properties it must
have, the ABI of the four new entry points, and the option's way through `DQNTrainer`, the loops and train.py."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import per_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "meshdqn_hip.h")


def _dyadic(rng, cap, zero_share=0.2):
    """Priorities k / 1024 with integer k < 1024: every fp64 sum of them is exact, in any order."""
    p = rng.integers(1, 1024, cap).astype(np.float32) / np.float32(1024)
    p[rng.random(cap) < zero_share] = 0
    return p


# ------------------------------------------------------------------ the reference against itself
def test_reference_draw_counts_follow_the_priorities_on_a_regular_grid():
    """u on a regular grid: the K * n targets are a regular grid of spacing total / (K n) over [0, total), so a record of
    priority p_i (an interval of that length) holds n_draws p_i / total of them, give or take one."""
    rng = np.random.default_rng(1)
    cap, n, K = 257, 256, 4
    prio = _dyadic(rng, cap)
    counts = np.zeros(cap, np.int64)
    for k in range(K):
        idx, w, total = per_ref.draw(prio, np.full(n, (k + 0.5) / K), 0.5)
        assert total == float(prio.astype(np.float64).sum())
        np.add.at(counts, idx, 1)
        assert (prio[idx] > 0).all() and w.max() == 1.0 and (w > 0).all()
        assert (np.diff(idx) >= 0).all()                          # stratified: draw i comes from the i-th n-th of the mass
    want = K * n * prio.astype(np.float64) / prio.astype(np.float64).sum()
    assert np.abs(counts - want).max() <= 1.0
    assert (counts[prio == 0] == 0).all()


def test_reference_draw_edge_rules():
    prio = np.array([0, 0, 0.5, 0, 0.25, 2.25, 0, 0], np.float32)      # total 3
    # u = 0: draw 0 aims at t = 0, the first record with a priority
    idx, w, total = per_ref.draw(prio, np.zeros(3), 1.0)
    assert total == 3.0 and idx.tolist() == [2, 5, 5]
    assert w.tolist() == [1.0, np.float32(0.5 / 2.25), np.float32(0.5 / 2.25)]
    # u = 1 - 2^-53: (2 + u) / 3 rounds to 1, t = total, no prefix sum exceeds it: the last record with a priority
    u = np.full(3, 1.0 - 2.0 ** -53)
    assert (2.0 + u[2]) / 3.0 == 1.0
    idx, w, _ = per_ref.draw(prio, u, 0.4)
    assert idx.tolist() == [5, 5, 5]
    # ... and with one draw the target stays below the total: the same record by the ordinary rule
    assert per_ref.draw(prio, u[:1], 0.4)[0].tolist() == [5]
    # all mass in one record
    one = np.zeros(9, np.float32)
    one[4] = 0.75
    idx, w, total = per_ref.draw(one, np.linspace(0, 0.99, 8), 0.7)
    assert (idx == 4).all() and (w == 1.0).all() and total == 0.75
    # nothing to draw from
    idx, w, total = per_ref.draw(np.zeros(6, np.float32), np.full(4, 0.3), 0.7)
    assert (idx == 0).all() and (w == 0).all() and total == 0.0
    # beta = 0: no correction
    assert (per_ref.draw(prio, np.full(4, 0.5), 0.0)[1] == 1.0).all()


def test_reference_update_rules():
    prio = np.full(8, 0.5, np.float32)
    idx = np.array([3, 1, 3, 6, 7, 3, -1, 8], np.int32)
    td = np.array([0.1, 2.0, 0.4, np.nan, np.inf, -0.9, 5.0, 5.0], np.float32)
    pmax = per_ref.update(prio, 1.0, idx, td, 0.6, 1e-6)
    assert prio[3] == np.float32((abs(float(np.float32(-0.9))) + 1e-6) ** 0.6)       # duplicates: the last one stays
    assert prio[1] == np.float32((2.0 + 1e-6) ** 0.6)
    assert prio[6] == 0.5 and prio[7] == 0.5                                        # NaN / Inf: untouched
    assert (prio[[0, 2, 4, 5]] == 0.5).all()                                        # out of range: skipped
    assert pmax == prio[1] and pmax > 1.0                                           # ... and not part of pmax
    # a duplicate whose later TD error is not finite keeps the earlier value
    p2 = np.zeros(4, np.float32)
    per_ref.update(p2, 1.0, np.array([2, 2], np.int32), np.array([0.5, np.nan], np.float32), 1.0, 0.25)
    assert p2[2] == 0.75
    # alpha = 0: exactly 1, whatever the TD error
    p3 = np.zeros(5, np.float32)
    pm = per_ref.update(p3, 1.0, np.arange(5, dtype=np.int32), np.array([0, 1e-30, 3.0, -7e8, 1e30], np.float32), 0.0, 1e-6)
    assert (p3 == 1.0).all() and pm == 1.0
    # pmax never falls
    pm = 1.0
    rng = np.random.default_rng(0)
    for _ in range(6):
        new = per_ref.update(p3, pm, np.arange(5, dtype=np.int32), rng.standard_normal(5).astype(np.float32) * 3, 0.8, 1e-6)
        assert new >= pm and new >= p3.max()
        pm = new


def test_reference_fill_rules():
    prio = np.full(10, 0.5, np.float32)
    per_ref.fill(prio, 2.0, 8, 4, 4, 3)                      # the new range wraps
    assert prio.tolist() == [2, 2, 0.5, 0.5, 0, 0, 0, 0.5, 2, 2]
    per_ref.fill(prio, 3.0, 0, 0, 9, 2)                      # zero-length new range, the zero range wraps
    assert prio.tolist() == [0, 2, 0.5, 0.5, 0, 0, 0, 0.5, 2, 0]
    per_ref.fill(prio, 3.0, 5, 0, 5, 0)
    for args in ((8, 4, 1, 2), (2, 3, 4, 2), (0, 11, 0, 0), (10, 1, 0, 0), (0, 5, 5, 6)):
        with pytest.raises(ValueError):
            per_ref.fill(prio.copy(), 1.0, *args)
    assert per_ref.ring_ranges(0, 5, 6) == (0, 0, 0, 6)
    assert per_ref.ring_ranges(7, 5, 6) == (6, 6, 12, 6)
    assert per_ref.ring_ranges(10, 5, 6, zero=False) == (24, 6, 0, 0)


# ------------------------------------------------------------------ ABI
def _c_layout(tmp_path, cname, cls):
    """(helper copied from tests/test_mixed_flow_cpu.py: the header's layout through the system compiler)"""
    fields = [n for n, _ in cls._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(){', f'printf("%zu\\n", sizeof({cname}));']
    src += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f in fields]
    src.append('return 0;}')
    cfile = tmp_path / f"{cname}.c"
    cfile.write_text("\n".join(src))
    exe = tmp_path / cname
    subprocess.check_call(["gcc", str(cfile), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    return vals[0], vals[1:], [getattr(cls, f).offset for f in fields]


CTYPE = {"int32_t": C.c_int32, "double": C.c_double}


def test_the_entry_points_are_declared_within_abi_8(tmp_path):
    from meshdqn_amd import _lib, build
    header = open(HEADER).read()
    assert _lib.ABI_VERSION == 8 and re.search(r"#define\s+MDQ_ABI_VERSION\s+8\b", header)
    assert sorted(_lib.SYMBOLS) == build.declared_symbols()
    want = {
        "mdq_gcn_train_step_weighted": ["const mdq_gcn_net* net", "const mdq_gcn_train_desc* d", "const float* weight", "float* td",
                                        "void* stream"],
        "mdq_replay_prio_fill": ["float* prio", "int32_t capacity", "int32_t base_new", "int32_t n_new", "int32_t base_zero",
                                 "int32_t n_zero", "const float* pmax", "void* stream"],
        "mdq_replay_prio_draw": ["const mdq_replay_prio_draw_desc* d", "void* stream"],
        "mdq_replay_prio_update": ["float* prio", "int32_t capacity", "int32_t n", "const int32_t* idx", "const float* td",
                                   "double alpha", "double eps", "float* pmax", "void* stream"],
    }
    for name, args in want.items():
        assert name in _lib.SYMBOLS and name in build.declared_symbols()
        decl = re.search(r"MDQ_API int " + name + r"\(([^)]*)\)", header).group(1)
        assert [" ".join(a.split()) for a in decl.split(",")] == args
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int and len(argtypes) == len(args)
        for a, ct in zip(args, argtypes):                       # scalars by their type, every pointer as a pointer
            typ = a.rsplit(" ", 1)[0]
            if "*" in typ:
                assert ct is C.c_void_p or ct == C.POINTER(_lib.ReplayPrioDrawDesc), (name, a)
            else:
                assert ct is CTYPE[typ], (name, a)
    # the old entry point is still there, unchanged
    assert re.search(r"MDQ_API int mdq_gcn_train_step\(const mdq_gcn_net\* net, const mdq_gcn_train_desc\* d, void\* stream\);", header)
    # the descriptor: field names, order and types from the header's text, size and offsets from the compiler
    body = re.search(r"typedef struct mdq_replay_prio_draw_desc \{(.*?)\} mdq_replay_prio_draw_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        typ, names = stmt.split(" ", 1) if "*" not in stmt else (stmt.rsplit(" ", 1)[0], stmt.rsplit(" ", 1)[1])
        if "*" in typ:
            fields.append((names, C.c_void_p))
        else:
            fields += [(n.strip(), CTYPE[typ]) for n in names.split(",")]
    assert fields == list(_lib.ReplayPrioDrawDesc._fields_)
    size, c_off, py_off = _c_layout(tmp_path, "mdq_replay_prio_draw_desc", _lib.ReplayPrioDrawDesc)
    assert size == C.sizeof(_lib.ReplayPrioDrawDesc) == 56 and c_off == py_off
    # the learning step's descriptor has not changed: the weights and the TD errors are arguments
    from meshdqn_amd.gcn_fused import GcnTrainDesc
    size, c_off, py_off = _c_layout(tmp_path, "mdq_gcn_train_desc", GcnTrainDesc)
    assert size == C.sizeof(GcnTrainDesc) and c_off == py_off
    assert not {"weight", "td"} & {n for n, _ in GcnTrainDesc._fields_}


# ------------------------------------------------------------------ the option
def _trainer(**kw):
    from meshdqn_amd.trainer import DistContext, DQNTrainer
    import torch
    return DQNTrainer(n_actions=20, num_inputs=17, ctx=DistContext(device=torch.device("cpu")), conv_width=32, **kw)


def test_trainer_validates_the_option_and_schedules_beta():
    assert _trainer().prioritized is None and _trainer(prioritized=None).prioritized is None
    tr = _trainer(prioritized={})
    assert tr.prioritized == dict(alpha=0.6, beta0=0.4, beta_steps=100000, eps=1e-6)
    tr = _trainer(prioritized=dict(alpha=0.0, beta0=1.0, beta_steps=10, eps=0.5))
    assert tr.prioritized == dict(alpha=0.0, beta0=1.0, beta_steps=10, eps=0.5) and tr.beta() == 1.0
    for bad in (dict(alpha=-0.1), dict(alpha=1.5), dict(beta0=0.0), dict(beta0=1.2), dict(beta_steps=0), dict(beta_steps=-5),
                dict(eps=0.0), dict(eps=-1e-6), dict(gamma=0.5), "yes", 3):
        with pytest.raises(ValueError, match="prioritized"):
            _trainer(prioritized=bad)
    _trainer(prioritized={}, batch_size=1024)
    with pytest.raises(ValueError, match="1024"):
        _trainer(prioritized={}, batch_size=1025)
    _trainer(batch_size=1025)                                       # (uniform replay: no such bound)
    # beta(g) = min(1, beta0 + (1 - beta0) g / beta_steps), g = num_grads, which a checkpoint carries
    tr = _trainer(prioritized=dict(beta0=0.4, beta_steps=1000))
    assert tr.beta() == 0.4 and tr.beta(0) == 0.4
    assert tr.beta(250) == min(1.0, 0.4 + (1 - 0.4) * 250 / 1000)
    assert tr.beta(1000) == 1.0 and tr.beta(5000) == 1.0
    tr.num_grads = 500
    assert tr.beta() == tr.beta(500) == 0.4 + 0.6 * 500 / 1000
    betas = [tr.beta(g) for g in range(0, 1500, 50)]
    assert all(b2 >= b1 for b1, b2 in zip(betas, betas[1:]))
    with pytest.raises(ValueError):
        _trainer().beta()


def test_trainer_state_round_trip_continues_the_beta_schedule(tmp_path):
    a = _trainer(prioritized=dict(beta_steps=200))
    a.num_grads = 77
    a.save(str(tmp_path), "p_")
    b = _trainer(prioritized=dict(beta_steps=200))
    b.load(str(tmp_path), "p_")
    assert b.num_grads == 77 and b.beta() == a.beta() == 0.4 + 0.6 * 77 / 200


def test_the_host_loops_refuse_a_prioritized_trainer():
    from meshdqn_amd.trainer import train_loop_per_worker, train_loop_vec
    tr = _trainer(prioritized={})
    with pytest.raises(ValueError, match="train_loop_device"):
        train_loop_vec(tr, None, 3)
    with pytest.raises(ValueError, match="train_loop_device"):
        train_loop_per_worker(tr, None, 1)
    # the device loop refuses a trace without the feature (and, here, a machine without a GPU) before any work
    from meshdqn_amd.trainer import train_loop_device
    with pytest.raises(ValueError, match="per_trace"):
        train_loop_device(_trainer(), None, 3, per_trace=True)


def test_train_script_parses_the_flag_and_the_yaml_block():
    import yaml
    spec = importlib.util.spec_from_file_location("mdq_train_script", os.path.join(ROOT, "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    cfg_path = os.path.join(ROOT, "configs", "ray_ys930.yaml")
    args = train.parser().parse_args(["--config", cfg_path])
    assert args.prioritized_replay is False
    cfg = yaml.safe_load(open(cfg_path))
    assert "replay" not in cfg and train.prioritized_options(False, cfg) is None       # the reference's config: uniform replay
    args = train.parser().parse_args(["--config", cfg_path, "--prioritized-replay"])
    assert args.prioritized_replay is True
    assert train.prioritized_options(True, cfg) == {}
    block = yaml.safe_load("replay: {prioritized: true, alpha: 0.7, beta0: 0.5, beta_steps: 2000, eps: 1.0e-5}")
    assert train.prioritized_options(False, block) == dict(alpha=0.7, beta0=0.5, beta_steps=2000.0, eps=1e-5)
    assert _trainer(prioritized=train.prioritized_options(False, block)).prioritized == dict(alpha=0.7, beta0=0.5, beta_steps=2000.0,
                                                                                              eps=1e-5)
    # numbers without the switch: uniform replay unless the flag is given, which then takes them
    block = yaml.safe_load("replay: {alpha: 0.3}")
    assert train.prioritized_options(False, block) is None and train.prioritized_options(True, block) == dict(alpha=0.3)
    assert train.prioritized_options(False, yaml.safe_load("replay: {prioritized: false}")) is None
    with pytest.raises(SystemExit, match="gamma"):
        train.prioritized_options(True, yaml.safe_load("replay: {prioritized: true, gamma: 0.3}"))
