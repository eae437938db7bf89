"""The Q-head option (`head` = "softmax" / "linear" / "dueling") without a GPU: the module against the fp64 reference of
tests/dueling_ref.py (forward, forward_dense, autograd gradients), the unchanged default, the header and its ctypes
mirrors, the option's way through `DQNTrainer` and train.py, and the input condition of the GPU learning-step cases.

Tolerances: MARGIN = 4 x the fp32 yardstick (the same reference run in float32, forced to the fp64 selection), the
largest over the graphs of the test, in the units of `gcn_path_cases._norm_dev` (outputs) and
`gcn_train_cases.grad_dev` (gradients); one fp32 ulp of the largest |q| where a yardstick is exactly 0.
"""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import dueling_ref as dref
import gcn_path_cases as cases
import gcn_ref64 as ref
import gcn_train_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "meshdqn_hip.h")
KW = dict(output_dim=181, conv_width=32, topk=0.5)
FIN0, SIZES = 17, (1, 9, 40)


# ------------------------------------------------------------------ the module against the reference
def _seeded_net(head, kw=KW, seed=41):
    from meshdqn_amd.airfoilgcnn import NodeRemovalNet
    from meshdqn_amd.gcn_fused import _levels_of
    net = NodeRemovalNet(**kw, head=head)
    net.set_num_nodes(FIN0)
    rng = np.random.default_rng(seed)
    sd = {k: torch.from_numpy(rng.standard_normal(tuple(v.shape)) * 0.3).float() for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    mods, softmax = _levels_of(net)
    assert softmax == (head == "softmax")
    names = {id(m): k for k, m in net.named_modules()}
    return net, sd, [(names[id(c)], names[id(p)]) for c, p in mods]


_CASES = {}


def _cases(head):
    """Network and graphs of 1, 9 and 40 nodes, drawn (seeded, like the families of gcn_train_cases) until no decision of
    the fp64 run is closer than KINK fp32 yardsticks to flipping: (net, sd, levels, [(x, ei, fp64 run, fp32 run)])."""
    if head not in _CASES:
        net, sd, levels = _seeded_net(head)
        rows = []
        for slot, n in enumerate(SIZES):
            for attempt in range(64):
                rng = np.random.default_rng([97, slot, attempt])
                x, ei = cases._graph(rng, n, FIN0, "none" if n == 1 else "random")
                a = dref.forward_graph(sd, levels, x, ei, KW["topk"], head, np.float64)
                b = dref.forward_graph(sd, levels, x, ei, KW["topk"], head, np.float32, a["perm"])
                if not tc.kink_violations(a, b, KW["topk"]):
                    break
            else:
                raise RuntimeError(f"no {n}-node graph without a close decision")
            rows.append((x, ei, a, b))
        _CASES[head] = (net, sd, levels, rows)
    return _CASES[head]


def _batch(x, ei):
    from meshdqn_amd.data import Batch, Data
    return Batch.from_data_list([Data(x=torch.from_numpy(x), edge_index=torch.from_numpy(ei))])


def _dense(x, ei):
    from meshdqn_amd.airfoilgcnn import dense_batch
    from meshdqn_amd.data import Data
    return dense_batch([Data(x=torch.from_numpy(x), edge_index=torch.from_numpy(ei))], max(ei.shape[1], 1))


def _out_bound(rows):
    yard = max(cases._norm_dev(b["out"], a["out"]) for _, _, a, b in rows)
    assert yard > 0
    return yard


@pytest.mark.parametrize("head", dref.HEADS)
def test_module_forward_against_fp64(head):
    net, sd, levels, rows = _cases(head)
    yard = _out_bound(rows)
    for x, ei, a, _ in rows:
        with torch.no_grad():
            got = {"forward": net(_batch(x, ei))[0].numpy(), "forward_dense": net.forward_dense(*_dense(x, ei))[0].numpy()}
        for path, q in got.items():
            d = cases._norm_dev(q, a["out"])
            print(f"head {head} {path} {len(x)} nodes: {d:.3e}, yardstick {yard:.3e}, ratio {d / yard:.2f}")
            assert q.shape == (KW["output_dim"],) and d <= dref.MARGIN * yard, (head, path, len(x), d, yard)
    if head == "softmax":
        assert all(abs(float(a["out"].sum()) - 1.0) < 1e-12 for _, _, a, _ in rows)
    if head == "dueling":   # the row's mean is the value, and the reference's own parts add up
        for _, _, a, _ in rows:
            assert abs(float(a["out"].mean()) - float(a["raw"][-1])) < 1e-12


@pytest.mark.parametrize("path", ["forward", "forward_dense"])
@pytest.mark.parametrize("head", dref.HEADS)
def test_autograd_gradients_against_fp64(head, path):
    net, sd, levels, rows = _cases(head)
    OUT = KW["output_dim"]
    rng = np.random.default_rng(5)
    qo = rng.standard_normal(OUT).astype(np.float32)
    steps = []
    for i, (x, ei, a, b) in enumerate(rows):
        act = (0, OUT - 1, 57)[i]
        args = (head, i % 2, act, np.float32(0.3), 1.0, 0.9, qo, 1, None)
        steps.append((dref.learning_step_graph(sd, levels, a, *args, np.float64),
                      dref.learning_step_graph(sd, levels, b, *args, np.float32), i % 2, act))
    yard = {k: max(tc.grad_dev(s32["grads"][k], s64["grads"], k) for s64, s32, _, _ in steps if s64["grads"][k] is not None and
                   np.any(s64["grads"][k])) for k in sd if any(s[0]["grads"][k] is not None and np.any(s[0]["grads"][k]) for s in steps)}
    if head == "dueling":
        assert "lin_v.weight" in yard and "lin_v.bias" in yard
    params = dict(net.named_parameters())
    for (x, ei, a, _), (s64, _, mode, act) in zip(rows, steps):
        net.zero_grad(set_to_none=True)
        out = (net(_batch(x, ei)) if path == "forward" else net.forward_dense(*_dense(x, ei)))[0]
        q = out[act] if mode == 0 else out.max()
        t = torch.tensor(0.3 + 0.9 * float(qo.max())) if mode == 0 else None
        loss = torch.nn.HuberLoss()(q, t) if mode == 0 else torch.nn.HuberLoss()(torch.tensor(float(qo[act])), 0.3 + 0.9 * q)
        loss.backward()
        for k, want in s64["grads"].items():
            g = params[k].grad
            if want is None:
                assert g is None or not bool(g.any()), k
                continue
            if not np.any(want):
                assert g is None or not bool(g.any()), k
                continue
            d = tc.grad_dev(g.numpy(), s64["grads"], k)
            assert d <= dref.MARGIN * yard[k], (head, path, len(x), k, d, yard[k])
    print(f"head {head} {path}: gradient yardsticks " + ", ".join(f"{k} {v:.1e}" for k, v in yard.items()))


def test_the_default_network_is_unchanged():
    from meshdqn_amd.airfoilgcnn import NodeRemovalNet
    kw = dict(output_dim=181, conv_width=128, topk=0.1)
    def make(*a, **k):     # (the pooling weights are drawn at construction, in front of the constructor's own seed)
        torch.manual_seed(3)
        return NodeRemovalNet(*a, **k)
    base, soft, duel, lin = make(**kw), make(**kw, head="softmax"), make(**kw, head="dueling"), make(181, 128, 0.1, None, "linear")
    keys = [f"conv{i}.{p}" for i in (1, 2, 3) for p in ("lin_l.weight", "lin_l.bias", "lin_r.weight")]
    keys = keys[:3] + ["pool1.weight"] + keys[3:6] + ["pool2.weight"] + keys[6:] + ["pool3.weight"]
    for i in (4, 5, 6):
        keys += [f"conv{i}.bias", f"conv{i}.lin.weight", f"pool{i}.weight"]
    keys += [f"lin{i}.{p}" for i in (1, 2, 3) for p in ("weight", "bias")]
    assert base.head == "softmax" and list(base.state_dict()) == keys == list(soft.state_dict()) == list(lin.state_dict())
    assert not hasattr(base, "lin_v") and not hasattr(lin, "lin_v")
    assert all(torch.equal(v, soft.state_dict()[k]) and torch.equal(v, lin.state_dict()[k]) for k, v in base.state_dict().items())
    assert all(torch.equal(v, duel.state_dict()[k]) for k, v in base.state_dict().items())
    for net in (base, soft, duel, lin):      # (conv1 re-created with the environment's 17 features: the trained network)
        net.set_num_nodes(17)
    assert sum(p.numel() for p in base.parameters()) == 173493 == sum(p.numel() for p in lin.parameters())
    # the value stream comes last - in the state_dict, in parameters() and in the draws of reset()
    assert list(duel.state_dict()) == keys + ["lin_v.weight", "lin_v.bias"]
    assert [k for k, _ in duel.named_parameters()][-2:] == ["lin_v.weight", "lin_v.bias"]
    assert sum(p.numel() for p in duel.parameters()) == 173493 + 65 and tuple(duel.lin_v.weight.shape) == (1, 64)
    assert bool(duel.lin_v.weight.any()) and bool(duel.lin_v.bias.any())
    for bad in ("Dueling", "", None, 3, "noisy"):
        with pytest.raises(ValueError, match="'softmax', 'linear', 'dueling'"):
            NodeRemovalNet(**kw, head=bad)


def test_dueling_output_ignores_a_constant_in_the_advantage_bias():
    net, sd, levels, rows = _cases("dueling")
    yard = _out_bound(rows)
    shifted, _, _ = _seeded_net("dueling")
    with torch.no_grad():
        shifted.lin3.bias.add_(2.5)
    for x, ei, a, _ in rows:
        with torch.no_grad():
            q0, q1 = net(_batch(x, ei))[0].numpy(), shifted(_batch(x, ei))[0].numpy()
        assert not np.array_equal(net.lin3.bias.detach().numpy(), shifted.lin3.bias.detach().numpy())
        d = cases._norm_dev(q1, q0.astype(np.float64))
        print(f"{len(x)} nodes: shift of 2.5 moves q by {d:.3e} of its largest value, yardstick {yard:.3e}")
        assert d <= dref.MARGIN * yard and cases._norm_dev(q1, a["out"]) <= dref.MARGIN * yard
    lin, _, _ = _seeded_net("linear")
    lin2, _, _ = _seeded_net("linear")
    with torch.no_grad():
        lin2.lin3.bias.add_(2.5)
        x, ei = rows[1][:2]
        assert float((lin2(_batch(x, ei)) - lin(_batch(x, ei))).abs().min()) > 2.0       # (the linear head does not)


def test_reference_parts():
    """The helper itself: OUT = 1 gives exactly v, the split gradients add up to the plain chain rule."""
    rng = np.random.default_rng(2)
    raw = rng.standard_normal(2)
    assert dref.aggregate(raw, np.float64)[0] == raw[1] and dref.aggregate(raw.astype(np.float32), np.float32)[0] == np.float32(raw[1])
    net, sd, levels, rows = _cases("dueling")
    x, ei, a, _ = rows[1]
    dq = rng.standard_normal(KW["output_dim"])
    grads, _ = dref.backward_graph(sd, levels, a, dq, "dueling")
    a2 = np.maximum(a["head_tape"][1][1], 0.0)
    assert np.allclose(grads["lin_v.bias"], dq.sum()) and np.allclose(grads["lin_v.weight"][0], dq.sum() * a2)
    assert np.allclose(grads["lin3.bias"], dq - dq.mean()) and abs(grads["lin3.bias"].sum()) < 1e-12
    assert grads["lin3.weight"].shape == (KW["output_dim"], 64) and grads["lin_v.weight"].shape == (1, 64)
    # finite differences through the whole reference, one entry of lin_v and one of lin3
    for key, idx in (("lin_v.weight", (0, 5)), ("lin3.bias", (7,)), ("lin1.weight", (3, 11))):
        h = 1e-6
        vals = []
        for s in (+1, -1):
            sd2 = {k: ref._arr(v, np.float64).copy() for k, v in sd.items()}
            sd2[key][idx] += s * h
            vals.append(float(dref.forward_graph(sd2, levels, x, ei, KW["topk"], "dueling", np.float64, a["perm"])["out"] @ dq))
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(fd - grads[key][idx]) <= 1e-6 * max(1.0, abs(fd)), (key, fd, grads[key][idx])


# ------------------------------------------------------------------ header and mirrors
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


def _header_fields(header, cname):
    body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if stmt:
            names += [re.sub(r"\[.*", "", n.strip().split(" ")[-1].lstrip("*")) for n in stmt.split(",")]
    return names


def test_header_and_mirrors(tmp_path):
    from meshdqn_amd import _lib, build
    from meshdqn_amd.gcn_fused import GcnGradLayout, GcnNet, GcnTrainDesc
    header = open(HEADER).read()
    assert _lib.ABI_VERSION == 8 and re.search(r"#define\s+MDQ_ABI_VERSION\s+8\b", header)
    assert sorted(_lib.SYMBOLS) == build.declared_symbols()
    net_fields = ["nlevels", "C", "fin0", "out_dim", "ratio", "softmax", "dueling", "levels", "lin1_w", "lin1_b", "lin2_w",
                  "lin2_b", "lin3_w", "lin3_b", "lin_v_w", "lin_v_b"]
    assert _header_fields(header, "mdq_gcn_net") == net_fields == [n for n, _ in GcnNet._fields_]
    size, c_off, py_off = _c_layout(tmp_path, "mdq_gcn_net", GcnNet)
    assert size == C.sizeof(GcnNet) == 32 + 6 * 40 + 8 * 8 and c_off == py_off
    assert GcnNet.dueling.offset == 28 and GcnNet.lin_v_w.offset == size - 16      # the old padding word; the last two fields
    lay_fields = ["w_l", "b", "w_r", "pool_w", "lin1_w", "lin1_b", "lin2_w", "lin2_b", "lin3_w", "lin3_b", "total", "lin_v"]
    assert _header_fields(header, "mdq_gcn_grad_layout") == lay_fields == [n for n, _ in GcnGradLayout._fields_]
    size, c_off, py_off = _c_layout(tmp_path, "mdq_gcn_grad_layout", GcnGradLayout)
    assert size == C.sizeof(GcnGradLayout) == 128 and c_off == py_off and GcnGradLayout.lin_v.offset == 124
    size, c_off, py_off = _c_layout(tmp_path, "mdq_gcn_train_desc", GcnTrainDesc)
    assert size == C.sizeof(GcnTrainDesc) == 264 and c_off == py_off
    assert GcnNet().dueling == 0 and not GcnNet().lin_v_w and GcnGradLayout().lin_v == 0       # zero-initialised: ABI 8's meaning


# ------------------------------------------------------------------ the option
def _trainer(**kw):
    from meshdqn_amd.trainer import DistContext, DQNTrainer
    return DQNTrainer(n_actions=20, num_inputs=17, ctx=DistContext(device=torch.device("cpu")), conv_width=32, **kw)


def _same(na, nb):
    a, b = na.state_dict(), nb.state_dict()
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_trainer_validates_the_option():
    base = _trainer()
    assert base.head == "softmax" and base.policy_net_1.head == base.policy_net_2.head == "softmax"
    assert _same(_trainer(head="softmax").policy_net_1, base.policy_net_1) and _same(_trainer(head="softmax").policy_net_2, base.policy_net_2)
    for head in ("linear", "dueling"):
        tr = _trainer(head=head)
        assert tr.head == tr.policy_net_1.head == tr.policy_net_2.head == head
        assert hasattr(tr.policy_net_1, "lin_v") == hasattr(tr.policy_net_2, "lin_v") == (head == "dueling")
    tr = _trainer(head="dueling", target_net={})
    assert _same(tr.policy_net_1, tr.policy_net_2) and "lin_v.bias" in tr.policy_net_2.state_dict()
    # the optimisers hold the value stream
    assert any(p is tr.policy_net_1.lin_v.weight for p in tr.opts[0].param_groups[0]["params"])
    for bad in ("duelling", "", None, 1, True, ["dueling"]):
        with pytest.raises(ValueError, match="'softmax', 'linear', 'dueling'"):
            _trainer(head=bad)


def test_checkpoints_round_trip_and_do_not_cross_heads(tmp_path):
    a = _trainer(head="dueling")
    with torch.no_grad():
        a.policy_net_1.lin_v.weight.add_(0.5)
        a.policy_net_2.lin_v.bias.add_(-0.25)
    a.num_grads = 9
    a.save(str(tmp_path), "d_")
    assert "lin_v.weight" in torch.load(os.path.join(str(tmp_path), "d_policy_net_1.pt"))
    b = _trainer(head="dueling")
    assert not _same(a.policy_net_1, b.policy_net_1)
    b.load(str(tmp_path), "d_")
    assert _same(a.policy_net_1, b.policy_net_1) and _same(a.policy_net_2, b.policy_net_2) and b.num_grads == 9
    for other in ("softmax", "linear"):
        with pytest.raises(RuntimeError, match=r"Unexpected key\(s\) in state_dict: \"lin_v.weight\", \"lin_v.bias\""):
            _trainer(head=other).load(str(tmp_path), "d_")
    _trainer(head="linear").save(str(tmp_path), "l_")
    with pytest.raises(RuntimeError, match=r"Missing key\(s\) in state_dict: \"lin_v.weight\", \"lin_v.bias\""):
        _trainer(head="dueling").load(str(tmp_path), "l_")
    _trainer(head="softmax").load(str(tmp_path), "l_")      # same keys: what the option means is not in the checkpoint


def test_train_script_flag_and_yaml_key():
    import yaml
    spec = importlib.util.spec_from_file_location("mdq_train_script", os.path.join(ROOT, "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    cfg_path = os.path.join(ROOT, "configs", "ray_ys930.yaml")
    cfg = yaml.safe_load(open(cfg_path))

    def args(*extra):
        return train.parser().parse_args(["--config", cfg_path, *extra])
    assert args().q_head is None and "q_head" not in cfg and train.q_head_option(None, cfg) == "softmax"
    for head in dref.HEADS:
        assert train.q_head_option(args("--q-head", head).q_head, cfg) == head
        assert train.q_head_option(None, yaml.safe_load(f"q_head: {head}")) == head
    assert train.q_head_option(args("--q-head", "linear").q_head, yaml.safe_load("q_head: dueling")) == "linear"   # the flag wins
    with pytest.raises(SystemExit):
        args("--q-head", "noisy")
    for bad in ("q_head: noisy", "q_head: 3", "q_head: [dueling]", "q_head: {kind: dueling}", "q_head: null"):
        with pytest.raises(SystemExit, match="q_head"):
            train.q_head_option(None, yaml.safe_load(bad))
    assert _trainer(head=train.q_head_option(None, yaml.safe_load("q_head: dueling"))).head == "dueling"


# ------------------------------------------------------------------ input condition of the GPU learning-step cases
@pytest.mark.parametrize("name", dref.FAMILIES)
def test_case_condition_of_the_dueling_families(name):
    """The embedding path of a dueling family is the existing family's (same weights, graphs and selections, asserted
    when the family is built), whose decisions sit at KINK yardsticks; the one decision the head changes, the mode-1
    first maximum, hangs on lin3's outputs alone and is more than KINK fp32 yardsticks of q wide in EVERY graph."""
    base, r64, r32, launches, st = tc.family(name)
    assert st["rejected"] / st["candidates"] <= tc.MAX_REJECTED
    fam = dref.family(name)
    assert fam.launches is launches and fam.graphs is base.graphs and len(fam.r64) == len(base.graphs)
    assert all(torch.equal(v, fam.sd[k]) for k, v in base.sd.items()) and list(fam.sd)[-2:] == ["lin_v.weight", "lin_v.bias"]
    closest = np.inf
    for g, (gap, yard) in enumerate(dref.argmax_gaps(fam)):
        assert np.array_equal(fam.r64[g]["emb"], r64[g]["emb"]) and fam.r64[g]["perm"] == r64[g]["perm"]
        assert yard > 0 and gap > tc.KINK * yard, (name, g, gap, yard)
        assert dref.first_max_of(fam.r64[g]) == dref.first_max_of(fam.r32[g])
        closest = min(closest, gap / yard)
    print(f"dueling family {name}: closest mode-1 argmax {closest:.0f} fp32 yardsticks of q (asserted: more than {tc.KINK:.0f})")
    for la in launches:
        assert tc.train_accepts(fam, la.nmax, la.emax) is None
    # the transition scheme: every Huber branch, terminal and non-terminal, first and last action, every weight, in both modes
    for mode in (0, 1):
        seen = dict(branch=set(), nf=set(), act=set(), w=set())
        for li in range(len(launches)):
            t = dref.transitions(fam, mode, li)
            for b, (s64, _) in enumerate(dref.steps(fam, mode, True)[li]):
                td = float(s64["td"])
                assert abs(td - t["want"][b]) < 1e-5, (mode, li, b, td)
                seen["branch"].add("mid" if abs(td) < 1 else "hi" if td > 1 else "lo")
                seen["nf"].add(float(t["nonfinal"][b])), seen["act"].add(int(t["action"][b])), seen["w"].add(float(t["weight"][b]))
        assert seen["branch"] == {"mid", "hi", "lo"} and seen["nf"] == {0.0, 1.0} and seen["w"] == set(tc.WEIGHTS), (mode, seen)
        assert {0, fam.out_dim - 1} <= seen["act"]
    assert any(la.gamma == 0.0 for la in launches) and any(la.gamma > 0.0 for la in launches)
    y = dref.yardsticks(fam)
    print(f"dueling family {name}: yardsticks out {y['out']:.2e} td {y['td']:.2e} loss {y['loss']:.2e} "
          f"lin_v.weight {y['grad']['lin_v.weight']:.2e} lin_v.bias {y['grad']['lin_v.bias']:.2e}")
    assert 0 < y["grad"]["lin_v.weight"] < 1e-3 and 0 <= y["grad"]["lin_v.bias"] < 1e-3
