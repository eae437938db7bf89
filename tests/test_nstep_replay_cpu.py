"""N-step returns without a GPU: the ABI of `mdq_replay_sample_nstep`, its numpy restatement (tests/nstep_ref.py) on
hand-written rings with the expected numbers spelled out, and the option's way through `DQNTrainer`, the loops and train.py."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import nstep_ref
from nstep_ref import Nstep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "meshdqn_hip.h")
CTYPE = {"int32_t": C.c_int32, "double": C.c_double}


# ------------------------------------------------------------------ ABI
def _c_layout(tmp_path, cname, cls):
    """(helper copied from tests/test_prioritized_replay_cpu.py: the header's layout through the system compiler)"""
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


def test_the_entry_point_is_declared_within_abi_8(tmp_path):
    from meshdqn_amd import _lib, build
    header = open(HEADER).read()
    assert _lib.ABI_VERSION == 8 and re.search(r"#define\s+MDQ_ABI_VERSION\s+8\b", header)
    assert sorted(_lib.SYMBOLS) == build.declared_symbols()
    name = "mdq_replay_sample_nstep"
    assert name in _lib.SYMBOLS and name in build.declared_symbols()
    decl = re.search(r"MDQ_API int " + name + r"\(([^)]*)\)", header).group(1)
    assert [" ".join(a.split()) for a in decl.split(",")] == ["const mdq_replay_sample_desc* d", "const mdq_replay_nstep* ns",
                                                              "void* stream"]
    restype, argtypes = _lib.SYMBOLS[name]
    assert restype is C.c_int and argtypes == [C.c_void_p, C.POINTER(_lib.ReplayNstepDesc), C.c_void_p]
    # the old entry point is still there, unchanged
    assert re.search(r"MDQ_API int mdq_replay_sample\(const mdq_replay_sample_desc\* d, void\* stream\);", header)
    assert _lib.SYMBOLS["mdq_replay_sample"] == (C.c_int, [C.c_void_p, C.c_void_p])
    # the descriptor: field names, order and types from the header's text, size and offsets from the compiler
    body = re.search(r"typedef struct mdq_replay_nstep \{(.*?)\} mdq_replay_nstep;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        typ, names = stmt.rsplit(" ", 1) if "*" in stmt else stmt.split(" ", 1)
        fields += [(names, C.c_void_p)] if "*" in typ else [(n.strip(), CTYPE[typ]) for n in names.split(",")]
    assert fields == list(_lib.ReplayNstepDesc._fields_)
    assert [n for n, _ in fields] == ["n_step", "W", "capacity", "head", "gamma", "steps"]
    size, c_off, py_off = _c_layout(tmp_path, "mdq_replay_nstep", _lib.ReplayNstepDesc)
    assert size == C.sizeof(_lib.ReplayNstepDesc) == 32 and c_off == py_off == [0, 4, 8, 12, 16, 24]
    # the sampling descriptor has not changed
    size, c_off, py_off = _c_layout(tmp_path, "mdq_replay_sample_desc", _lib.ReplaySampleDesc)
    assert size == C.sizeof(_lib.ReplaySampleDesc) == 16 + 13 * 8 and c_off == py_off
    # the header says where gamma^m is formed
    comment = header[header.index("The same sampling launch with the n-step"):header.index("typedef struct mdq_replay_nstep")]
    assert "float(gamma^(m-1)) * float(gamma)" in comment and "learning step" in comment


# ------------------------------------------------------------------ the reference on hand-written rings
NF, EM = 1, 1          # rec_len 11: [x(s) | x(s') | src(s) | dst(s) | src(s') | dst(s') | edges(s) edges(s') action reward done]


def _ring(done=()):
    """3 groups x 2 lanes (W = 2, capacity 6): record j = 2 g + lane carries reward 1, 2, 4 in group g = 0, 1, 2,
    x(s) = 10 j + 1, x(s') = 10 j + 2, one edge j -> j + 100 in s, one edge j -> j + 200 in s' (none if terminal), action j."""
    R = np.zeros((6, 11), np.float32)
    for j in range(6):
        dn = j in done
        R[j] = [10 * j + 1, 0 if dn else 10 * j + 2, j, j + 100, 0 if dn else j, 0 if dn else j + 200, 1, 0 if dn else 1, j,
                (1.0, 2.0, 4.0)[j // 2], 1.0 if dn else 0.0]
    return R


def test_reference_stops_at_a_terminal_in_the_middle():
    R = _ring(done=(3,))
    ns = Nstep(n_step=3, W=2, capacity=6, head=0, gamma=0.5)          # (head at group 0: groups 1 and 2 lie in front of it)
    # lane 1 from record 1: 1 -> 3, which is terminal; lane 0 from record 0 runs its three steps: 0 -> 2 -> 4
    out = nstep_ref.compose(R, NF, EM, ns, [1, 0])
    assert nstep_ref.walk(R, NF, EM, ns, 1) == [1, 3] and nstep_ref.walk(R, NF, EM, ns, 0) == [0, 2, 4]
    assert out["steps"].tolist() == [2, 3]
    assert out["reward"].tolist() == [1.0 + 0.5 * 2.0, 1.0 + 0.5 * 2.0 + 0.25 * 4.0] == [2.0, 3.0]
    assert out["nonfinal"].tolist() == [0.0, 0.25]
    assert out["x_s"].tolist() == [[11.0], [1.0]]
    assert out["x_n"].tolist() == [[11.0], [42.0]]                    # terminal: the own state of record 1; else s' of record 4
    assert out["action"].tolist() == [1, 0]
    assert out["esrc_s"].tolist() == [1, 0] and out["edst_s"].tolist() == [101, 100] and out["edge_ptr_s"].tolist() == [0, 1, 2]
    assert out["esrc_n"].tolist() == [1, 4] and out["edst_n"].tolist() == [101, 204] and out["edge_ptr_n"].tolist() == [0, 1, 2]
    # a terminal record drawn itself: one step, whatever n_step
    out = nstep_ref.compose(R, NF, EM, ns, [3])
    assert (out["steps"].tolist(), out["reward"].tolist(), out["nonfinal"].tolist(), out["x_n"].tolist()) == ([1], [2.0], [0.0], [[31.0]])


def test_reference_stops_at_the_head():
    R = _ring()
    ns = Nstep(n_step=3, W=2, capacity=6, head=4, gamma=0.5)
    out = nstep_ref.compose(R, NF, EM, ns, [0, 3])
    assert nstep_ref.walk(R, NF, EM, ns, 0) == [0, 2] and nstep_ref.walk(R, NF, EM, ns, 3) == [3]
    assert out["steps"].tolist() == [2, 1]
    assert out["reward"].tolist() == [2.0, 2.0] and out["nonfinal"].tolist() == [0.5, 1.0]      # not terminal: gamma^(m-1)
    assert out["x_n"].tolist() == [[22.0], [32.0]] and out["edst_n"].tolist() == [202, 203]
    # a drawn record of the head group is taken as it is, and the walk continues from it
    assert nstep_ref.walk(R, NF, EM, ns, 4) == [4, 0, 2]
    assert nstep_ref.compose(R, NF, EM, ns, [4])["reward"].tolist() == [4.0 + 0.5 * 1.0 + 0.25 * 2.0]


def test_reference_wraps_past_the_end_of_the_ring():
    R = _ring()
    ns = Nstep(n_step=3, W=2, capacity=6, head=2, gamma=0.5)
    out = nstep_ref.compose(R, NF, EM, ns, [5, 4, 1])
    assert nstep_ref.walk(R, NF, EM, ns, 5) == [5, 1] and nstep_ref.walk(R, NF, EM, ns, 4) == [4, 0]
    assert out["steps"].tolist() == [2, 2, 1]
    assert out["reward"].tolist() == [4.5, 4.5, 1.0] and out["nonfinal"].tolist() == [0.5, 0.5, 1.0]
    assert out["x_n"].tolist() == [[12.0], [2.0], [12.0]]
    assert out["esrc_n"].tolist() == [1, 0, 1] and out["edst_n"].tolist() == [201, 200, 201]
    # gamma = 0: only the first reward, and a factor 0 that is not a terminal's (m = 2: gamma^1)
    out = nstep_ref.compose(R, NF, EM, ns._replace(gamma=0.0), [5, 1])
    assert out["reward"].tolist() == [4.0, 1.0] and out["nonfinal"].tolist() == [0.0, 1.0] and out["x_n"].tolist() == [[12.0], [12.0]]


def test_reference_with_one_step_is_the_plain_sample():
    R = _ring(done=(2, 5))
    for head in (0, 2, 4):
        for gamma in (0.5, 0.0, 1.0):
            out = nstep_ref.compose(R, NF, EM, Nstep(1, 2, 6, head, gamma), [0, 2, 5, 5, 3])
            assert out["steps"].tolist() == [1] * 5
            assert out["reward"].tolist() == [1.0, 2.0, 4.0, 4.0, 2.0] and out["nonfinal"].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0]
            assert out["x_n"].tolist() == [[2.0], [21.0], [51.0], [51.0], [32.0]]
            assert out["edge_ptr_n"].tolist() == [0, 1, 2, 3, 4, 5] and out["edst_n"].tolist() == [200, 102, 105, 105, 203]


def test_reference_refuses_what_the_entry_point_refuses():
    good = Nstep(3, 2, 6, 4, 0.5)
    nstep_ref.check(good)
    for bad in (dict(n_step=0), dict(n_step=65), dict(W=0), dict(capacity=7), dict(capacity=2), dict(head=3), dict(head=6),
                dict(head=-2), dict(gamma=-0.1), dict(gamma=float("inf")), dict(gamma=float("nan"))):
        with pytest.raises(ValueError):
            nstep_ref.check(good._replace(**bad))


# ------------------------------------------------------------------ the option
def _trainer(**kw):
    from meshdqn_amd.trainer import DistContext, DQNTrainer
    import torch
    return DQNTrainer(n_actions=20, num_inputs=17, ctx=DistContext(device=torch.device("cpu")), conv_width=32, **kw)


def test_trainer_validates_the_option():
    assert _trainer().n_step == 1 and _trainer(n_step=1).n_step == 1
    assert _trainer(n_step=3).n_step == 3 and _trainer(n_step=64).n_step == 64
    for bad in (0, 65, 2.5, "3", -1, None, True):
        with pytest.raises(ValueError, match="n_step"):
            _trainer(n_step=bad)
    # a constructor option, not checkpointed state
    assert _trainer(n_step=3, prioritized={}).prioritized is not None


def test_trainer_state_round_trip_leaves_the_option_alone(tmp_path):
    a = _trainer(n_step=3)
    a.save(str(tmp_path), "n_")
    b = _trainer()
    b.load(str(tmp_path), "n_")
    assert b.n_step == 1


def test_the_host_loops_refuse_an_n_step_trainer():
    from meshdqn_amd.trainer import train_loop_device, train_loop_per_worker, train_loop_vec
    tr = _trainer(n_step=2)
    with pytest.raises(ValueError, match="train_loop_device"):
        train_loop_vec(tr, None, 3)                                  # (no environment: refused before touching it)
    with pytest.raises(ValueError, match="train_loop_device"):
        train_loop_per_worker(tr, None, 1)
    with pytest.raises(ValueError, match="nstep_trace"):
        train_loop_device(_trainer(), None, 3, nstep_trace=True)
    # the sampling call of an n-step trainer wants the step being written
    with pytest.raises(ValueError, match="head_step"):
        tr.optimize_device(None, [0, 1])


def test_train_script_parses_the_flag_and_the_yaml_key():
    import yaml
    spec = importlib.util.spec_from_file_location("mdq_train_script", os.path.join(ROOT, "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    cfg_path = os.path.join(ROOT, "configs", "ray_ys930.yaml")
    cfg = yaml.safe_load(open(cfg_path))
    assert "replay" not in cfg                                                      # the reference's config stays as it is
    args = train.parser().parse_args(["--config", cfg_path])
    assert args.n_step is None and train.n_step_option(args.n_step, cfg) == 1       # neither
    args = train.parser().parse_args(["--config", cfg_path, "--n-step", "3"])
    assert args.n_step == 3 and train.n_step_option(args.n_step, cfg) == 3          # the flag
    block = yaml.safe_load("replay: {n_step: 5}")
    assert train.n_step_option(None, block) == 5                                    # the block
    assert train.n_step_option(3, block) == 3                                       # both: the flag wins
    assert train.n_step_option(1, block) == 1
    assert isinstance(train.n_step_option(None, block), int)
    with pytest.raises(SystemExit, match="n_step"):
        train.n_step_option(None, yaml.safe_load("replay: {n_step: 2.5}"))
    # the prioritized block accepts and ignores the key
    assert train.prioritized_options(False, {"replay": {"n_step": 3}}) is None
    assert train.prioritized_options(True, {"replay": {"n_step": 3}}) == {}
    assert train.prioritized_options(False, yaml.safe_load("replay: {prioritized: true, alpha: 0.7, n_step: 3}")) == dict(alpha=0.7)
    with pytest.raises(SystemExit, match="gamma"):                                  # a genuinely unknown key still exits
        train.prioritized_options(False, yaml.safe_load("replay: {n_step: 3, gamma: 0.3}"))
    # out of range values reach the trainer's own check
    with pytest.raises(ValueError, match="n_step"):
        _trainer(n_step=train.n_step_option(65, cfg))
