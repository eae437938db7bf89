"""The "linear" and "dueling" Q-heads on the GPU: the three head kernels (`head_store`, meshdqn_amd/csrc/mdq_gcn.hip)
against the fp64 head restatement applied to the device's own embeddings, the refusals of both entry families, the
learning step (`gcn_train_kernel`) on the dueling versions of the families T-A, T-B, T-E32 and T-E256 against the fp64
reference of tests/dueling_ref.py, and the option's way through `optimize_device`, `train_loop_device` and train.py.

Tolerances: MARGIN = 4 x the fp32 yardstick (the reference in float32 on the same inputs / forced to the fp64
selection), in the units of `gcn_path_cases._norm_dev` and `gcn_train_cases.grad_dev`; one fp32 ulp of the largest |q|
where a yardstick is exactly 0.  The input conditions of the learning-step cases are asserted without a GPU in
test_dueling_head_cpu.py.
"""
import ctypes as C
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import dueling_ref as dref
import gcn_path_cases as cases
import gcn_train_cases as tc
import target_net_ref
from test_gcn_train_paths_gpu import _abi_buffers, _check_reduce, _run as _launch, _same, _slices
from test_nstep_replay_gpu import B_ENV, BATCH, PER, STEPS, _cfg, _run, _same_run, _trainer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = dref.EPS32
POISON = -777.25
FIN0 = 17
OUTS = (1, 2, 63, 64, 65, 181, 256)
BS = (1, 17, 33)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ 1. head shapes, isolated from TopK
@functools.lru_cache(maxsize=None)
def _head_net(OUT, Cw, head):
    from meshdqn_amd.airfoilgcnn import NodeRemovalNet
    from meshdqn_amd.gcn_fused import FusedGcn
    net = NodeRemovalNet(OUT, conv_width=Cw, topk=0.5, head=head)
    net.set_num_nodes(FIN0)
    rng = np.random.default_rng([1605, OUT, Cw])
    sd = {k: torch.from_numpy(rng.standard_normal(tuple(v.shape)) * 0.3).float() for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    fg = FusedGcn(net.cuda())
    fg._pack()
    torch.cuda.synchronize()
    return fg, sd


@functools.lru_cache(maxsize=None)
def _head_graphs(B):
    rng = np.random.default_rng(300 + B)
    graphs = [cases._graph(rng, 9, FIN0) for _ in range(B)]
    return cases.batch_arrays(graphs, range(B))


def _forward_abi(fg, B, desc=None, entry="mdq_gcn_forward_ex"):
    """One call of the C ABI on the 9-node graphs, into poisoned buffers with 40 rows behind the B the call may write:
    (return code, error text, emb rows, out rows) as numpy arrays of all B + 40 rows."""
    from meshdqn_amd import _lib
    x, node_ptr, esrc, edst, edge_ptr, nmax, emax = _head_graphs(B)
    d = fg.desc if desc is None else desc
    keep = [_dev(a) for a in (x, node_ptr, esrc, edst, edge_ptr)]
    rows = B + 40
    emb = torch.full((rows, 2 * d.C), POISON, dtype=torch.float32, device="cuda")
    out = torch.full((rows, d.out_dim), POISON, dtype=torch.float32, device="cuda")
    args = [C.byref(d), B, nmax, emax] + [k.data_ptr() for k in keep]
    if entry == "mdq_gcn_forward":
        rc = fg.lib.mdq_gcn_forward(*args, emb.data_ptr(), out.data_ptr(), _lib.stream_ptr(None))
    elif entry == "mdq_gcn_forward_ex":
        rc = fg.lib.mdq_gcn_forward_ex(*args, emb.data_ptr(), out.data_ptr(), None, None, _lib.stream_ptr(None))
    else:       # padded edge lists: (B, emax) slots and the counts
        ne = np.diff(edge_ptr)
        es, ed = np.zeros((B, emax), np.int32), np.zeros((B, emax), np.int32)
        for b in range(B):
            es[b, :ne[b]], ed[b, :ne[b]] = esrc[edge_ptr[b]:edge_ptr[b + 1]], edst[edge_ptr[b]:edge_ptr[b + 1]]
        keep += [_dev(es), _dev(ed), _dev(ne.astype(np.int32))]
        rc = fg.lib.mdq_gcn_forward_padded(C.byref(d), B, nmax, emax, keep[0].data_ptr(), keep[1].data_ptr(), keep[5].data_ptr(),
                                           keep[6].data_ptr(), keep[7].data_ptr(), emb.data_ptr(), out.data_ptr(), None, None,
                                           _lib.stream_ptr(None))
    torch.cuda.synchronize()
    return rc, (fg.lib.mdq_last_error() or b"").decode(), emb.cpu().numpy(), out.cpu().numpy()


def _check_head_rows(fg, sd, head, launches, tag):
    """Device q rows of `launches` ([(what, B, emb, out)], one network) against the fp64 head on the device's own
    embeddings.  The yardstick is the network's: the fp32 head against the fp64 head on the same embeddings, the largest over
    the rows of all its launches (one row, B = 1, is one sample of the rounding and no bound for another kernel's order of
    the same sums).  Rows past B keep the poison."""
    OUT = fg.desc.out_dim
    devs, yard = [], 0.0
    for what, B, emb, out in launches:
        assert (emb[B:] == POISON).all() and (out[B:] == POISON).all(), f"{tag} {what}: rows past B were written"
        assert np.isfinite(emb[:B]).all() and np.isfinite(out[:B]).all()
        q64 = [dref.head_of_embedding(sd, emb[b], head, np.float64) for b in range(B)]
        yard = max([yard] + [cases._norm_dev(dref.head_of_embedding(sd, emb[b], head, np.float32), q64[b]) for b in range(B)])
        devs.append((what, max(cases._norm_dev(out[b], q64[b]) for b in range(B))))
        if OUT > 1:
            assert np.ptp(out[:B], axis=1).min() > 0
    bound = dref.MARGIN * yard if yard > 0 else EPS32
    for what, d in devs:
        print(f"{tag} {what}: yardstick {yard:.3e}, device {d:.3e}, bound {bound:.3e}")
    for what, d in devs:
        assert d <= bound, (tag, what, d, bound)


def _exactly_v(fg, B, q):
    """One output: A - mean A is exactly 0 whatever lin3 holds, the row is exactly v.  The same launch with other device
    values in lin3's place (lin2's bias: 64 floats for the [64][1] weight, its first for the bias) gives the same bits."""
    other = fg.desc.__class__.from_buffer_copy(fg.desc)
    other.lin3_w = other.lin3_b = fg.desc.lin2_b
    rc, text, _, qs = _forward_abi(fg, B, desc=other)
    assert rc == 0 and np.array_equal(_bits(qs), _bits(q)), text


@pytest.mark.parametrize("head", ["dueling", "linear"])
@pytest.mark.parametrize("OUT", OUTS)
def test_head_kernels_against_fp64_on_the_device_embedding(lib_built, monkeypatch, OUT, head):
    monkeypatch.delenv("MDQ_HEAD_TILES", raising=False)
    wide, narrow = [], []
    for B in BS:
        # ---- C = 128: the 16-graph tiles (default), then the 32-graph tiles on the same inputs
        fg, sd = _head_net(OUT, 128, head)
        assert fg.desc.dueling == (head == "dueling") and fg.desc.softmax == 0 and fg.desc.C == 128
        rc, text, e16, q16 = _forward_abi(fg, B)
        assert rc == 0, text
        monkeypatch.setenv("MDQ_HEAD_TILES", "32")
        rc, text, e32, q32 = _forward_abi(fg, B)
        monkeypatch.delenv("MDQ_HEAD_TILES")
        assert rc == 0, text
        wide += [(f"B {B} c128-t16", B, e16, q16), (f"B {B} c128-t32", B, e32, q32)]
        assert np.array_equal(_bits(e16), _bits(e32))
        bad = _bits(q16) != _bits(q32)
        assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist())       # the two C = 128 kernels: bit for bit
        if head == "dueling" and OUT == 1:
            _exactly_v(fg, B, q16)
        # ---- C = 64: the generic kernel
        fg, sd = _head_net(OUT, 64, head)
        rc, text, e, q = _forward_abi(fg, B, entry="mdq_gcn_forward_padded" if B == 17 else "mdq_gcn_forward")
        assert rc == 0, text
        narrow.append((f"B {B} generic", B, e, q))
        if head == "dueling" and OUT == 1:
            _exactly_v(fg, B, q)
    _check_head_rows(*_head_net(OUT, 128, head), head, wide, f"{head} OUT {OUT}")
    _check_head_rows(*_head_net(OUT, 64, head), head, narrow, f"{head} OUT {OUT}")


def test_forward_arrays_of_the_module_is_the_abi_call(lib_built):
    """`forward_fused` / `forward_arrays` of a dueling module hand the same descriptor to the same entry point."""
    fg, sd = _head_net(181, 128, "dueling")
    B = 17
    x, node_ptr, esrc, edst, edge_ptr, nmax, emax = _head_graphs(B)
    q, emb = fg.forward_arrays(_dev(x), _dev(node_ptr), _dev(esrc), _dev(edst), _dev(edge_ptr), nmax, emax, return_embedding=True)
    _, _, e, o = _forward_abi(fg, B)
    assert np.array_equal(_bits(q.cpu().numpy()), _bits(o[:B])) and np.array_equal(_bits(emb.cpu().numpy()), _bits(e[:B]))


def test_fused_copy_refuses_a_value_stream_that_is_not_adjacent(lib_built):
    """`layout.lin_v` is ONE offset (the bias sits at + 64): a module whose two tensors are apart in `parameters()` order
    is refused when the packed copy is built."""
    from meshdqn_amd.airfoilgcnn import NodeRemovalNet
    from meshdqn_amd.gcn_fused import FusedGcn

    class Apart(torch.nn.Module):
        def __init__(self, lin):
            super().__init__()
            self.weight, self.between, self.bias = lin.weight, torch.nn.Parameter(torch.zeros(3)), lin.bias

    net = NodeRemovalNet(5, conv_width=32, topk=0.5, head="dueling")
    net.lin_v = Apart(net.lin_v)
    with pytest.raises(ValueError, match="adjacent"):
        FusedGcn(net.cuda())._pack()
    good = FusedGcn(NodeRemovalNet(5, conv_width=32, topk=0.5, head="dueling").cuda())
    good._pack()
    assert good.layout.lin_v == good.layout.total - 65 and good._table.n == 22 and good.desc.dueling == 1


# ------------------------------------------------------------------ 2. refusals
def _bad_descs(fg):
    out = {}
    for what in ("softmax", "lin_v_w", "lin_v_b"):
        d = fg.desc.__class__.from_buffer_copy(fg.desc)
        if what == "softmax":
            d.softmax = 1
        else:
            setattr(d, what, None)
        out[what] = d
    return out


@pytest.mark.parametrize("entry", ["mdq_gcn_forward", "mdq_gcn_forward_ex", "mdq_gcn_forward_padded"])
def test_forward_refuses_a_bad_dueling_descriptor(lib_built, entry):
    fg, _ = _head_net(181, 128, "dueling")
    for what, d in _bad_descs(fg).items():
        rc, text, emb, out = _forward_abi(fg, 17, desc=d, entry=entry)
        print(f"{entry}, dueling with {what}: return code {rc}, text '{text}'")
        assert rc < 0 and "mdq_gcn_forward" in text, (what, rc, text)
        assert (emb == POISON).all() and (out == POISON).all(), what
    rc, text, _, out = _forward_abi(fg, 17, entry=entry)
    assert rc == 0 and not (out[:17] == POISON).any(), text


def _train_abi(fg, fam, desc, layout, weighted, t):
    from meshdqn_amd import _lib
    from meshdqn_amd.gcn_fused import GcnTrainDesc
    rng = np.random.default_rng(5)
    graphs = [cases._graph(rng, 9, fam.fin0) for _ in range(2)]
    nmax, emax = 41, 82
    buf = _abi_buffers(fam, graphs, nmax, emax, 2)
    keep = [_dev(t["q_other"]), _dev(t["action"]), _dev(t["reward"]), _dev(t["nonfinal"]), _dev(np.ones(2, np.float32))]
    d = GcnTrainDesc()
    d.B, d.NMAX, d.EMAX, d.mode, d.gamma = 2, nmax, emax, 0, 0.9
    for k in ("x", "node_ptr", "esrc", "edst", "edge_ptr", "workspace", "partial", "grad", "loss", "out"):
        setattr(d, k, buf[k].data_ptr())
    d.q_other, d.action, d.reward, d.nonfinal = (k.data_ptr() for k in keep[:4])
    d.layout = layout
    if weighted:
        rc = fg.lib.mdq_gcn_train_step_weighted(C.byref(desc), C.byref(d), keep[4].data_ptr(), buf["td"].data_ptr(), _lib.stream_ptr(None))
    else:
        rc = fg.lib.mdq_gcn_train_step(C.byref(desc), C.byref(d), _lib.stream_ptr(None))
    torch.cuda.synchronize()
    return rc, (fg.lib.mdq_last_error() or b"").decode(), buf


@pytest.mark.parametrize("weighted", [False, True])
def test_train_step_refuses_a_bad_dueling_descriptor(lib_built, weighted):
    from meshdqn_amd.gcn_fused import FusedGcn
    fam = dref.family("T-E32")
    fg = FusedGcn(fam.net.cuda())
    fg._pack()
    assert tc.train_accepts(fam, 41, 82) is None and fg.desc.dueling == 1
    rng = np.random.default_rng(6)
    t = dict(q_other=rng.standard_normal((2, fam.out_dim)).astype(np.float32), action=np.zeros(2, dtype=np.int64),
             reward=np.zeros(2, dtype=np.float32), nonfinal=np.ones(2, dtype=np.float32))
    outputs = ("workspace", "partial", "grad", "loss", "out") + (("td",) if weighted else ())
    for what, d in _bad_descs(fg).items():
        rc, text, buf = _train_abi(fg, fam, d, fg.layout, weighted, t)
        print(f"train step (weighted {weighted}), dueling with {what}: return code {rc}, text '{text}'")
        assert rc < 0 and "mdq_gcn_train_step" in text, (what, rc, text)
        for k in outputs:
            assert bool((buf[k] == POISON).all()), (what, k)
    rc, text, buf = _train_abi(fg, fam, fg.desc, fg.layout, weighted, t)        # the call itself was a good one
    assert rc == 0 and not bool((buf["grad"] == POISON).any()), text
    # 300 outputs are refused as before the option
    from meshdqn_amd.airfoilgcnn import NodeRemovalNet
    big = NodeRemovalNet(300, conv_width=32, topk=0.5, head="dueling")
    big.set_num_nodes(fam.fin0)
    fb = FusedGcn(big.cuda())
    fb._pack()
    t300 = dict(t, q_other=rng.standard_normal((2, 300)).astype(np.float32))

    class _Fam300:
        fin0, out_dim, net = fam.fin0, 300, big
        levels, ratio, C = fam.levels, fam.ratio, fam.C
    assert tc.train_accepts(_Fam300, 41, 82) == "out_dim"
    rc, text, buf = _train_abi(fb, _Fam300, fb.desc, fb.layout, weighted, t300)
    assert rc < 0 and "mdq_gcn_train_step" in text and "256" in text, (rc, text)
    for k in outputs:
        assert bool((buf[k] == POISON).all()), k


# ------------------------------------------------------------------ 3. the learning step
@functools.lru_cache(maxsize=None)
def _fused_family(name, head="dueling", out_dim=None):
    from meshdqn_amd.gcn_fused import FusedGcn
    return FusedGcn(dref.family(name, head, out_dim).net.cuda())


def _compare_launch(fam, fg, mode, weighted, li, report):
    la, yard = fam.launches[li], dref.yardsticks(fam)
    t = dref.transitions(fam, mode, li)
    steps = dref.steps(fam, mode, weighted)[li]
    graphs = [fam.graphs[g] for g in la.idx]
    variant = "weighted" if weighted else "td"
    res = _launch(fg, graphs, la.nmax, la.emax, mode, t, la.gamma, variant)
    again = _launch(fg, graphs, la.nmax, la.emax, mode, t, la.gamma, variant)
    for k in ("loss", "grad", "out", "td", "partial"):
        assert _same(res[k], again[k]), f"{fam.name} launch {li}: a second identical launch differs in {k}"
    B = len(la.idx)
    slices, total = _slices(fam.net)
    assert total == res["partial"].shape[1] == fg.layout.total and fg.layout.lin_v == slices.get("lin_v.weight", (0,))[0]
    _check_reduce(res, B)
    _, offs = tc.tape_layout(fam, la.nmax, la.emax)
    loss64, tdfloor = 0.0, 0.0
    for b, g in enumerate(la.idx):
        s64 = steps[b][0]
        ints = res["ws"][b].view(np.int32)
        for l, nl in enumerate(fam.level_sizes(len(fam.graphs[g][0]))):       # the selection on the tape: the family's
            k = tc._ceil(fam.ratio, nl)
            assert ints[offs[l]["perm"]:offs[l]["perm"] + k].tolist() == fam.r64[g]["perm"][l], (fam.name, li, g, l)
        d_out = cases._norm_dev(res["out"][b], fam.r64[g]["out"])
        report["out"] = max(report.get("out", 0.0), d_out)
        if d_out > dref.MARGIN * yard["out"]:
            report["bad"].append(f"launch {li} graph {g} out: {d_out:.3e}, yardstick {yard['out']:.3e}")
        a = int(t["action"][b])
        q = float(fam.r64[g]["out"][a]) if mode == 0 else float(t["q_other"][b, a])
        floor = EPS32 * max(abs(q), abs(q - float(s64["td"])))
        tdfloor = max(tdfloor, floor)
        d_td = abs(float(res["td"][b]) - float(s64["td"]))
        report["td"] = max(report.get("td", 0.0), d_td)
        if d_td > max(dref.MARGIN * yard["td"], floor):
            report["bad"].append(f"launch {li} graph {g} td: {d_td:.3e}, yardstick {yard['td']:.3e}, floor {floor:.3e}")
        loss64 += float(s64["term"])
        if weighted and float(t["weight"][b]) == 0.0:
            assert not np.any(res["partial"][b]), f"{fam.name} launch {li} graph {g}: weight 0 left a gradient"
            report["zero"] = report.get("zero", 0) + 1
        for key, (lo, hi, shape) in slices.items():
            got, want = res["partial"][b, lo:hi].reshape(shape), s64["grads"][key]
            if want is None or not np.any(want):
                assert not np.any(got), f"{fam.name} launch {li} graph {g} {key}: reference exactly zero, device {np.abs(got).max():.3e}"
                continue
            if key.startswith("lin_v"):
                assert np.any(got), f"{fam.name} launch {li} graph {g}: {key} has no gradient"
                report["lin_v"] = report.get("lin_v", 0) + 1
            d = tc.grad_dev(got, s64["grads"], key)
            if d >= report["grad"].get(key, (0.0, None))[0]:
                report["grad"][key] = (d, (li, g))
            if d > dref.MARGIN * yard["grad"][key]:
                report["bad"].append(f"launch {li} graph {g} {key}: {d:.3e} of its unit, yardstick {yard['grad'][key]:.3e} "
                                     f"(ratio {d / yard['grad'][key]:.2f}, bound {dref.MARGIN})")
    d_loss = abs(float(res["loss"]) - loss64)
    report["loss"] = max(report.get("loss", 0.0), d_loss)
    if d_loss > max(dref.MARGIN * yard["loss"], tdfloor):
        report["bad"].append(f"launch {li} loss: {d_loss:.3e}, yardstick {yard['loss']:.3e}, floor {tdfloor:.3e}")


def _family_against_fp64(name, head, mode, weighted):
    fam, fg = dref.family(name, head), _fused_family(name, head)
    assert fg.net.head == head
    yard = dref.yardsticks(fam)
    report = dict(grad={}, bad=[])       # (every figure is printed before the bounds are asserted)
    for li, la in enumerate(fam.launches):
        assert tc.train_accepts(fam, la.nmax, la.emax) is None
        _compare_launch(fam, fg, mode, weighted, li, report)
    tag = f"{head} family {name} mode {mode} weighted {weighted}"
    for k in ("out", "td", "loss"):
        print(f"{tag} {k}: yardstick {yard[k]:.3e}, device {report[k]:.3e}, ratio {report[k] / max(yard[k], 1e-300):.2f}")
    for key, (d, where) in sorted(report["grad"].items()):
        y = yard["grad"][key]
        print(f"{tag} {key}: worst (launch, graph) {where}: yardstick {y:.3e}, device {d:.3e}, ratio {d / y:.2f} (bound {dref.MARGIN})")
    assert not report["bad"], f"{tag}: beyond {dref.MARGIN} x the fp32 yardstick:\n" + "\n".join(report["bad"])
    return report


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", dref.FAMILIES)
def test_dueling_learning_step_against_fp64(lib_built, name, mode, weighted):
    report = _family_against_fp64(name, "dueling", mode, weighted)
    assert report.get("lin_v", 0) > 0 and {"lin_v.weight", "lin_v.bias"} <= set(report["grad"])
    if weighted:
        assert report.get("zero", 0) > 0        # (every family's first launch holds a graph of weight 0)


@pytest.mark.parametrize("mode", [0, 1])
def test_linear_learning_step_against_fp64(lib_built, mode):
    """`head="linear"` is the kernels' existing branch without a softmax, reached through `NodeRemovalNet`."""
    fg = _fused_family("T-E32", "linear")
    fg._pack()
    assert fg.desc.softmax == 0 and fg.desc.dueling == 0 and fg.layout.lin_v == 0
    _family_against_fp64("T-E32", "linear", mode, True)


@pytest.mark.parametrize("mode", [0, 1])
def test_one_output_gives_exactly_v_and_no_lin3_gradient(lib_built, mode):
    fam, fg = dref.family("T-E32", "dueling", 1), _fused_family("T-E32", "dueling", 1)
    la = fam.launches[0]
    assert fam.out_dim == 1 and tc.train_accepts(fam, la.nmax, la.emax) is None
    t = dref.transitions(fam, mode, 0)
    res = _launch(fg, [fam.graphs[g] for g in la.idx], la.nmax, la.emax, mode, t, la.gamma, "td")
    slices, _ = _slices(fam.net)
    (w0, w1, _), (b0, b1, _), (v0, v1, _) = slices["lin3.weight"], slices["lin3.bias"], slices["lin_v.weight"]
    assert not np.any(res["partial"][:, w0:w1]) and not np.any(res["partial"][:, b0:b1])         # exactly zero
    live = [b for b in range(len(la.idx)) if mode == 0 or t["nonfinal"][b] != 0]
    assert live and all(np.any(res["partial"][b, v0:v1]) for b in live)
    yard = max(max(cases._norm_dev(a["out"], b["out"]) for a, b in zip(fam.r32, fam.r64)), EPS32)
    for b, g in enumerate(la.idx):
        assert cases._norm_dev(res["out"][b], fam.r64[g]["out"]) <= dref.MARGIN * yard
    # exactly v: other advantage weights, the same bits
    with torch.no_grad():
        keep = fam.net.lin3.weight.clone()
        fam.net.lin3.weight.add_(0.75)
    try:
        moved = _launch(fg, [fam.graphs[g] for g in la.idx], la.nmax, la.emax, mode, t, la.gamma, "td")
    finally:
        with torch.no_grad():
            fam.net.lin3.weight.copy_(keep)
    assert _same(moved["out"], res["out"]) and _same(moved["td"], res["td"])


# ------------------------------------------------------------------ 4. chain and loop
M_LOOP = STEPS - (-(-BATCH // B_ENV))


@pytest.fixture(scope="module")
def base_env(lib_built):
    from meshdqn_amd.env import Env2DAirfoil
    return Env2DAirfoil(_cfg())


@pytest.fixture(scope="module")
def run_default(base_env):
    return _run(base_env)


def _net_bits(net):
    return [p.detach().clone() for p in net.parameters()]


def _nets_equal(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


def test_dueling_double_chain_equals_the_learning_step_by_hand(run_default):
    rep = run_default[1].device_memory
    dev, N, EM = rep.R.device, rep.N, rep.e_max
    period = 3
    td, t1 = _trainer(target_net=dict(kind="double", period=period), head="dueling"), _trainer(head="dueling")
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in td.policy_net_2.parameters():
            p.add_((0.05 * torch.randn(p.shape, generator=g)).to(p.device))
    t1.policy_net_1.load_state_dict(td.policy_net_1.state_dict())
    t1.policy_net_2.load_state_dict(td.policy_net_2.state_dict())
    assert "lin_v.weight" in td.policy_net_1.state_dict() and not _nets_equal(_net_bits(td.policy_net_1), _net_bits(td.policy_net_2))
    random.seed(77)
    idx = rep.draw(9, BATCH)
    loss = torch.zeros(1, device=dev)
    target_v0 = td.policy_net_2.lin_v.weight.clone()
    td.optimize_device(rep, idx, loss_out=loss)
    torch.cuda.synchronize()
    flat_d = next(iter(td._fused_of(td.policy_net_1, "train")._train_bufs.values()))["grad"].clone()
    b = td._mb_bufs
    gs = (b["x_s"].clone(), b["node_ptr"], b["esrc_s"].clone(), b["edst_s"].clone(), b["edge_ptr_s"].clone())
    gn = (b["x_n"].clone(), b["node_ptr"], b["esrc_n"].clone(), b["edst_n"].clone(), b["edge_ptr_n"].clone())
    action, reward, nonfinal = b["action"].clone(), b["reward"].clone(), b["nonfinal"].clone()
    # ---- the same step by hand on the networks as they were
    q_t = t1._fused_of(t1.policy_net_2, "train").forward_arrays(*gn, N, EM).cpu().numpy()
    q_o = t1._fused_of(t1.policy_net_1, "train").forward_arrays(*gn, N, EM).cpu().numpy()
    assert q_o.shape == (BATCH, 181) and np.abs(q_o.sum(1) - 1).min() > 1e-3          # q rows, no probabilities
    want_q, _, _ = target_net_ref.select(q_o, q_t)
    loss_1, flat_1 = t1._fused_of(t1.policy_net_1, "train").train_step(*gs, N, EM, 0, torch.from_numpy(want_q).to(dev), action,
                                                                       reward, nonfinal, td.gamma)
    torch.cuda.synchronize()
    assert torch.equal(loss.view(torch.int32), loss_1.view(torch.int32)) and np.isfinite(float(loss))
    assert torch.equal(flat_d.view(torch.int32), flat_1.view(torch.int32))
    lo = td._fused_of(td.policy_net_1, "train").layout.lin_v
    assert lo == flat_d.numel() - 65 and float(flat_d[lo:lo + 64].abs().max()) > 0 and float(flat_d[lo + 64]) != 0
    # ---- mdq_adam_step moved lin_v ...
    assert not torch.equal(td.policy_net_1.lin_v.weight, t1.policy_net_1.lin_v.weight)
    assert not torch.equal(td.policy_net_1.lin_v.bias, t1.policy_net_1.lin_v.bias)
    act = td._fused_of(td.policy_net_1, "act")
    q_act1 = act.forward_arrays(*gn, N, EM).clone()          # (the acting copy packs the weights of one step)
    td.optimize_device(rep, idx)
    torch.cuda.synchronize()
    # ---- ... and after the next one the acting copy's forward shows the new weights, the value stream among them
    from meshdqn_amd.gcn_fused import FusedGcn
    q_act2 = act.forward_arrays(*gn, N, EM).clone()
    q_fresh = FusedGcn(td.policy_net_1).forward_arrays(*gn, N, EM).clone()
    assert torch.equal(q_act2.view(torch.int32), q_fresh.view(torch.int32)) and not torch.equal(q_act2, q_act1)
    with torch.no_grad():
        keep = td.policy_net_1.lin_v.bias.clone()
        td.policy_net_1.lin_v.bias.copy_(t1.policy_net_1.lin_v.bias)
    q_old_v = FusedGcn(td.policy_net_1).forward_arrays(*gn, N, EM).clone()
    with torch.no_grad():
        td.policy_net_1.lin_v.bias.copy_(keep)
    assert not torch.equal(q_old_v, q_act2)
    # ---- after `period` steps, and not before, the target's lin_v is the online one
    assert td.num_grads == period - 1 and torch.equal(td.policy_net_2.lin_v.weight, target_v0)
    td.optimize_device(rep, idx)
    torch.cuda.synchronize()
    assert td.num_grads == period and not torch.equal(td.policy_net_2.lin_v.weight, target_v0)
    assert torch.equal(td.policy_net_2.lin_v.weight, td.policy_net_1.lin_v.weight)
    assert torch.equal(td.policy_net_2.lin_v.bias, td.policy_net_1.lin_v.bias)
    assert _nets_equal(_net_bits(td.policy_net_2), _net_bits(td.policy_net_1))


def test_loop_dueling_prioritized_n_step_is_reproducible(base_env):
    """(Reproducibility only: the combined chain is held to an fp64 reference in tests/test_optimizer_chain_gpu.py.)"""
    a, ta = _run(base_env, prioritized=PER, n_step=3, head="dueling")
    b, tb = _run(base_env, prioritized=PER, n_step=3, head="dueling")
    _same_run(a, ta, b, tb)
    assert ta.head == "dueling" and len(a["losses"]) == M_LOOP and np.isfinite(a["losses"]).all() and np.isfinite(a["per"]["td"]).all()
    assert torch.equal(ta.device_memory.prio, tb.device_memory.prio)
    init = _trainer(head="dueling")
    assert not torch.equal(ta.policy_net_1.lin_v.weight, init.policy_net_1.lin_v.weight)        # the value stream was trained
    assert all(torch.isfinite(p).all() for p in ta.policy_net_1.parameters())


def test_loop_with_the_softmax_head_named_is_the_default_loop(base_env, run_default):
    out, tr = run_default
    assert tr.head == "softmax" and len(out["losses"]) == M_LOOP
    named, tn = _run(base_env, head="softmax")
    _same_run(out, tr, named, tn)
    assert [k for k, _ in tn.policy_net_1.named_parameters()] == [k for k, _ in tr.policy_net_1.named_parameters()]


def test_train_py_with_the_dueling_head(lib_built, tmp_path):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ray_ys930.yaml")))
    cfg["flow_config"]["geometry_params"]["mesh"] = os.path.join(ROOT, "tests", "golden", "ys930.npz")
    cfg["agent_params"].update(solver_steps=20, save_steps=4)
    cfg["optimizer"]["batch_size"] = BATCH
    cpath = os.path.join(str(tmp_path), "cfg.yaml")
    yaml.safe_dump(cfg, open(cpath, "w"))
    save = os.path.join(str(tmp_path), "run")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, "train.py", "--config", cpath, "--envs", str(B_ENV), "--steps", "6", "--q-head", "dueling",
                          "--save-dir", save, "--save-every", "0"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    losses = np.load(os.path.join(save, "losses.npy"))
    assert len(losses) == 6 - (-(-BATCH // B_ENV)) and np.isfinite(losses).all()
    sd = torch.load(os.path.join(save, "policy_net_1.pt"), map_location="cpu")
    assert list(sd)[-2:] == ["lin_v.weight", "lin_v.bias"] and tuple(sd["lin_v.weight"].shape) == (1, 64)
