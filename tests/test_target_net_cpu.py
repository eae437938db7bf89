"""The target network without a GPU: the numpy restatement of the two kernels (tests/target_net_ref.py) against the rules the
header states, the ABI of the two new entry points, and the option's way through `DQNTrainer`, the loops and train.py."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import target_net_ref as ref
from test_prioritized_replay_cpu import _c_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "meshdqn_hip.h")
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------ the restatement against the header's rules
def _sel(row):
    return int(ref.select(np.array([row], np.float32), np.zeros((1, len(row)), np.float32))[1][0])


def test_select_rules_on_hand_written_rows():
    assert _sel([1.0, 3.0, 2.0, 3.0]) == 1                          # the first of two equal maxima
    assert _sel([-1.0, -0.0, 0.0, -2.0]) == 1                       # -0 == +0: the first index wins
    assert _sel([-1.0, 0.0, -0.0, -2.0]) == 1
    assert _sel([0.5, 0.25, 0.125, 4.0]) == 3                       # the maximum in the last column
    assert _sel([NAN, 1.0, NAN, 0.5]) == 1                          # a NaN beside a finite maximum, on either side
    assert _sel([1.0, NAN]) == 0
    assert _sel([-INF, -INF, -INF]) == 0                            # nothing above -inf
    assert _sel([NAN, NAN, NAN]) == 0
    assert _sel([-INF, NAN, -INF]) == 0
    assert _sel([-INF, -3e38, -INF]) == 1 and _sel([-INF, INF, INF]) == 1 and _sel([7.0]) == 0
    # the value comes from the target's row and fills the row of q_sel
    qo = np.array([[0.1, 0.9, 0.3], [2.0, -1.0, 2.0]], np.float32)
    qt = np.array([[10.0, 20.0, 30.0], [-5.0, -6.0, -7.0]], np.float32)
    q_sel, sel, value = ref.select(qo, qt)
    assert sel.dtype == np.int32 and sel.tolist() == [1, 0] and value.tolist() == [20.0, -5.0]
    assert q_sel.dtype == np.float32 and q_sel.tolist() == [[20.0] * 3, [-5.0] * 3]
    # one array in both roles: the row's maximum, which the learning step's max over the broadcast row returns again
    rng = np.random.default_rng(0)
    q = rng.standard_normal((9, 181)).astype(np.float32)
    q_sel, sel, value = ref.select(q, q)
    assert np.array_equal(value, q.max(1)) and np.array_equal(sel, q.argmax(1)) and np.array_equal(q_sel.max(1), value)
    assert np.array_equal(sel, torch.from_numpy(q).argmax(1).numpy())


def test_polyak_rules():
    rng = np.random.default_rng(1)
    d, s = rng.standard_normal(1000).astype(np.float32), rng.standard_normal(1000).astype(np.float32)
    s[:3] = (-0.0, NAN, INF)
    s[3:4].view(np.uint32)[0] = 0x7FA12345                          # a signalling NaN with a payload
    out = ref.polyak(d, s, 1.0)
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), s.view(np.uint32))
    for tau in (0.5, 0.005):
        tf = np.float32(tau)
        want = np.array([np.float32(np.float32(a) + np.float32(tf * np.float32(np.float32(b) - np.float32(a))))
                         for a, b in zip(d[4:], s[4:])], np.float32)
        assert np.array_equal(ref.polyak(d[4:], s[4:], tau).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(ref.polyak(d[4:], d[4:], 0.3), d[4:])     # a fixed point
    for bad in (dict(n=0), dict(n=33), dict(lens=[3, -1]), dict(tau=0.0), dict(tau=1.5), dict(tau=-0.1), dict(tau=NAN),
                dict(tau=INF), dict(null=True), dict(same=True)):
        with pytest.raises(ValueError):
            ref.check(**dict(dict(n=2, lens=[3, 4], tau=0.5), **bad))
    ref.check(32, [0] * 32, 1.0)


# ------------------------------------------------------------------ ABI
CTYPE = {"int32_t": C.c_int32, "double": C.c_double}


def test_the_entry_points_are_declared_within_abi_8(tmp_path):
    from meshdqn_amd import _lib, build
    header = open(HEADER).read()
    assert _lib.ABI_VERSION == 8 and re.search(r"#define\s+MDQ_ABI_VERSION\s+8\b", header)
    assert sorted(_lib.SYMBOLS) == build.declared_symbols()
    want = {
        "mdq_double_q_select": ["int32_t B", "int32_t OUT", "const float* q_online", "const float* q_target", "float* q_sel",
                                "int32_t* sel", "void* stream"],
        "mdq_target_update": ["const mdq_target_update_desc* d", "void* stream"],
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
                assert ct is C.c_void_p or ct == C.POINTER(_lib.TargetUpdateDesc), (name, a)
            else:
                assert ct is CTYPE[typ], (name, a)
    assert int(re.search(r"#define\s+MDQ_DOUBLE_Q_ROWS\s+(\d+)", header).group(1)) == _lib.DOUBLE_Q_ROWS
    assert int(re.search(r"#define\s+MDQ_GCN_PACK_MAX\s+(\d+)", header).group(1)) == _lib.PACK_MAX == ref.PACK_MAX
    # the descriptor: field names and order from the header's text, size and offsets from the compiler
    body = re.search(r"typedef struct mdq_target_update_desc \{(.*?)\} mdq_target_update_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if stmt:
            names += [re.sub(r"\[.*", "", n.strip().split(" ")[-1].lstrip("*")) for n in stmt.split(",")]
    fields = _lib.TargetUpdateDesc._fields_
    assert names == [n for n, _ in fields] == ["n", "_pad", "dst", "src", "len", "tau"]
    assert [t for _, t in fields] == [C.c_int32, C.c_int32, C.c_void_p * 32, C.c_void_p * 32, C.c_int32 * 32, C.c_double]
    size, c_off, py_off = _c_layout(tmp_path, "mdq_target_update_desc", _lib.TargetUpdateDesc)
    assert size == C.sizeof(_lib.TargetUpdateDesc) == 8 + 256 + 256 + 128 + 8 and c_off == py_off
    # the learning step keeps its descriptor and its entry points: the selected row arrives as `q_other`
    from meshdqn_amd.gcn_fused import GcnTrainDesc
    size, c_off, py_off = _c_layout(tmp_path, "mdq_gcn_train_desc", GcnTrainDesc)
    assert size == C.sizeof(GcnTrainDesc) == 24 + 14 * 8 + 32 * 4 and c_off == py_off       # (264, as before the option)
    assert [n for n, _ in GcnTrainDesc._fields_] == ["B", "NMAX", "EMAX", "mode", "gamma", "x", "node_ptr", "esrc", "edst", "edge_ptr",
                                                     "q_other", "action", "reward", "nonfinal", "workspace", "partial", "grad",
                                                     "loss", "out", "layout"]
    assert re.search(r"MDQ_API int mdq_gcn_train_step\(const mdq_gcn_net\* net, const mdq_gcn_train_desc\* d, void\* stream\);", header)
    # the new kernels are a unit of their own: the replay unit's source is not part of it
    assert build.UNITS["target"] == ("mdq_target.hip", [], [])


# ------------------------------------------------------------------ the option
def _trainer(**kw):
    from meshdqn_amd.trainer import DistContext, DQNTrainer
    return DQNTrainer(n_actions=20, num_inputs=17, ctx=DistContext(device=torch.device("cpu")), conv_width=32, **kw)


def test_trainer_validates_the_option():
    assert _trainer().target_net is None and _trainer(target_net=None).target_net is None
    assert _trainer(target_net={}).target_net == dict(kind="double", period=50, tau=1.0)
    assert _trainer(target_net={}, target_update=7).target_net == dict(kind="double", period=7, tau=1.0)
    assert _trainer(target_net=dict(kind="max", period=3, tau=0.005)).target_net == dict(kind="max", period=3, tau=0.005)
    assert _trainer(target_net=dict(period=np.int64(4), tau=1)).target_net == dict(kind="double", period=4, tau=1.0)
    for bad in (dict(kind="dueling"), dict(kind=None), dict(kind=2), dict(period=0), dict(period=-3), dict(period=1.5),
                dict(period=True), dict(period="5"), dict(tau=0), dict(tau=0.0), dict(tau=1.5), dict(tau=-0.5), dict(tau=NAN),
                dict(tau=INF), dict(tau=True), dict(tau="1"), dict(gamma=0.5), dict(kind="double", alpha=1), "double", 3, True,
                ["double"]):
        with pytest.raises(ValueError, match="target_net"):
            _trainer(target_net=bad)


def _same(na, nb):
    return all(torch.equal(p, q) for (_, p), (_, q) in zip(na.state_dict().items(), nb.state_dict().items()))


def test_constructor_copies_the_online_network_into_the_target():
    base, tgt = _trainer(), _trainer(target_net=dict(kind="double"))
    assert len(base.policy_net_1.state_dict()) == len(tgt.policy_net_1.state_dict()) > 0
    assert _same(base.policy_net_1, tgt.policy_net_1)               # net 1: the default trainer's bits from the same seed
    assert _same(tgt.policy_net_1, tgt.policy_net_2)                # net 2: a copy of it
    assert not _same(base.policy_net_1, base.policy_net_2)          # ... which the default trainer's is not
    assert all(p.data_ptr() != q.data_ptr() for p, q in zip(tgt.policy_net_1.parameters(), tgt.policy_net_2.parameters()))
    assert tgt.select is True and tgt.num_grads == 0
    assert _same(_trainer(target_net=dict(kind="max")).policy_net_2, base.policy_net_1)


def test_checkpoint_keeps_a_different_target(tmp_path):
    a = _trainer(target_net=dict(period=5))
    with torch.no_grad():
        for p in a.policy_net_2.parameters():
            p.add_(0.25)
    a.num_grads = 13
    a.save(str(tmp_path), "t_")
    b = _trainer(target_net=dict(period=5))
    assert _same(b.policy_net_1, b.policy_net_2)
    b.load(str(tmp_path), "t_")
    assert _same(b.policy_net_2, a.policy_net_2) and _same(b.policy_net_1, a.policy_net_1)
    assert not _same(b.policy_net_1, b.policy_net_2)
    assert b.num_grads == 13 and b.select is True                   # the period continues where the checkpoint stopped


def test_the_host_paths_refuse_the_trainer():
    from meshdqn_amd.trainer import train_loop_device, train_loop_per_worker, train_loop_vec
    for kind in ("double", "max"):
        tr = _trainer(target_net=dict(kind=kind))
        with pytest.raises(ValueError, match="train_loop_device"):
            train_loop_vec(tr, None, 3)
        with pytest.raises(ValueError, match="train_loop_device"):
            train_loop_per_worker(tr, None, 1)
        with pytest.raises(ValueError, match="train_loop_device"):
            tr.optimize()
    # the trace needs the select launch: refused without the option and for the fixed-target kind, before any work
    with pytest.raises(ValueError, match="target_trace"):
        train_loop_device(_trainer(), None, 3, target_trace=True)
    with pytest.raises(ValueError, match="target_trace"):
        train_loop_device(_trainer(target_net=dict(kind="max")), None, 3, target_trace=True)


def test_train_script_parses_the_flags_and_the_yaml_block():
    import yaml
    spec = importlib.util.spec_from_file_location("mdq_train_script", os.path.join(ROOT, "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    cfg_path = os.path.join(ROOT, "configs", "ray_ys930.yaml")
    cfg = yaml.safe_load(open(cfg_path))

    def args(*extra):
        return train.parser().parse_args(["--config", cfg_path, *extra])
    a = args()
    assert a.target_net is None and a.target_tau is None and a.target_period is None
    assert "target_net" not in cfg and train.target_options(a, cfg) is None           # the reference's config: its toggle
    assert train.target_options(args("--target-net", "double"), cfg) == dict(kind="double")
    assert train.target_options(args("--target-net", "max", "--target-tau", "0.01", "--target-period", "1"), cfg) == \
        dict(kind="max", tau=0.01, period=1)
    with pytest.raises(SystemExit):
        args("--target-net", "dueling")
    with pytest.raises(SystemExit, match="target-net"):
        train.target_options(args("--target-tau", "0.5"), cfg)
    # the yaml block alone switches the option on; a flag wins over the block's key
    block = yaml.safe_load("target_net: {kind: double, tau: 0.5, period: 50}")
    assert train.target_options(a, block) == dict(kind="double", tau=0.5, period=50)
    assert train.target_options(args("--target-net", "max"), block) == dict(kind="max", tau=0.5, period=50)
    assert train.target_options(args("--target-period", "9"), block) == dict(kind="double", tau=0.5, period=9)
    assert train.target_options(a, yaml.safe_load("target_net: {}")) == {}
    assert _trainer(target_net=train.target_options(a, block)).target_net == dict(kind="double", period=50, tau=0.5)
    assert _trainer(target_net=train.target_options(args("--target-net", "max"), cfg)).target_net == dict(kind="max", period=50, tau=1.0)
    with pytest.raises(SystemExit, match="gamma"):
        train.target_options(a, yaml.safe_load("target_net: {kind: double, gamma: 0.3}"))
    with pytest.raises(SystemExit, match="target_net"):
        train.target_options(a, yaml.safe_load("target_net: double"))
    # the block is not part of `replay:`, whose own keys stay what they were
    with pytest.raises(SystemExit):
        train.prioritized_options(True, yaml.safe_load("replay: {prioritized: true, kind: double}"))
