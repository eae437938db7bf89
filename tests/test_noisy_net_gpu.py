"""Noisy networks on the GPU: `mdq_gcn_pack_noisy` against `mdq_gcn_pack` and the float32 restatement of the composition,
its noise against the fp64 restatement of tests/noisy_ref.py, `mdq_noisy_grad` against the float32 product, the learning
step of a copy that carries noise against the fp64 reference run on the composed weights (tests/dueling_ref.py, the
tolerances of tests/test_dueling_head_gpu.py: MARGIN x the fp32 yardstick), the refusals of both entry points, and the
option's way through `optimize_device`, `train_loop_device` and train.py.

EPS_TOL: the largest |device eps - fp64 eps| over the draws of this file was measured on an MI355X as EPS_MEASURED
(1.428e-07 in every pack test, 1.13e-07 .. 1.36e-07 in the families: about half a float32 unit in the last place of an
|eps| above 2); the bound is 4 x that for the spread between math-library versions (logf, cospif), and stays below the
1e-5 it may never pass.
"""
import copy
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import dueling_ref as dref
import gcn_path_cases as cases
import gcn_train_cases as tc
import noisy_ref as ref
from test_gcn_train_paths_gpu import _run as _launch, _same, _slices
from test_nstep_replay_gpu import B_ENV, BATCH, STEPS, _cfg, _run, _same_run, _trainer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = dref.EPS32
POISON = -777.25
FIN0 = 17
OUTS = (1, 5, 21, 64)
HEADS = ("softmax", "dueling")
EPS_MEASURED = 1.43e-7          # measured on the MI355X, see above
EPS_TOL = min(4 * EPS_MEASURED, 1e-5)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ 1. the pack and its noise
@functools.lru_cache(maxsize=None)
def _noisy_head_net(OUT, head, sigma_zero=False):
    """The small head network of tests/test_dueling_head_gpu.py (`_head_net`, conv width 32) with the noisy option: seeded
    means, sigmas that differ from entry to entry (or all zero)."""
    from meshdqn_amd.airfoilgcnn import NodeRemovalNet
    from meshdqn_amd.gcn_fused import FusedGcn
    net = NodeRemovalNet(OUT, conv_width=32, topk=0.5, head=head, noisy=0.5)
    net.set_num_nodes(FIN0)
    rng = np.random.default_rng([1611, OUT])
    sd = {k: torch.from_numpy(rng.standard_normal(tuple(v.shape)) * 0.3).float() for k, v in net.state_dict().items()}
    sd["noisy_sigma"] = torch.zeros_like(sd["noisy_sigma"]) if sigma_zero else sd["noisy_sigma"].abs() + 0.01
    net.load_state_dict(sd)
    return FusedGcn(net.cuda()), sd


def _plain_twin(net):
    """The plain network with the mean parameters of the noisy `net`, on the GPU."""
    from meshdqn_amd.airfoilgcnn import NodeRemovalNet
    twin = NodeRemovalNet(net.output_dim, conv_width=net.conv_width, topk=net.topk, head=net.head)
    twin.set_num_nodes(net.conv1.lin_l.weight.shape[1])
    twin.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items() if k != "noisy_sigma"})
    return twin.cuda()


def _packed(fg):
    """Copies of the packed segments of the copy's table, in table order."""
    torch.cuda.synchronize()
    return [fg._keep[s].cpu().numpy().copy() for s in range(fg._table.n)]


def _eps(fg):
    torch.cuda.synchronize()
    return {name: (a.cpu().numpy().copy(), b.cpu().numpy().copy()) for name, (a, b) in fg.eps.items()}


def _eps_deviation(fg, eps, stream, draw, seed=ref.SEED):
    want = ref.layer_noise64(seed, stream, draw, fg.net.noisy_layout())
    worst = 0.0
    for name, (e_in, e_out) in eps.items():
        for got, w in ((e_in, want[name][0]), (e_out, want[name][1])):
            assert got.dtype == np.float32 and got.shape == w.shape and np.abs(got).max() < ref.EPS_MAX
            worst = max(worst, float(np.abs(got.astype(np.float64) - w).max()))
    return worst


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("OUT", OUTS)
def test_pack_noisy_against_the_pack_and_the_restatement(lib_built, OUT, head):
    fg, sd = _noisy_head_net(OUT, head)
    net = fg.net
    fg.denoise()
    fg._pack()
    mean = _packed(fg)
    table, nz = fg._table, fg.noisy_desc
    lay = net.noisy_layout()
    assert nz.n == len(lay) == (4 if head == "dueling" else 3) and table.n == (22 if head == "dueling" else 20)
    noisy_segs = {nz.seg_w[l] for l in range(nz.n)} | {nz.seg_b[l] for l in range(nz.n)}
    assert len(noisy_segs) == 2 * nz.n
    sig = sd["noisy_sigma"].numpy()
    seen, worst = {}, 0.0
    for stream, draw in ref.DRAWS:
        fg.resample(ref.SEED, stream, draw)
        got, eps = _packed(fg), _eps(fg)
        seen[(stream, draw)] = (got, eps)
        worst = max(worst, _eps_deviation(fg, eps, stream, draw))
        for s in range(table.n):
            if s not in noisy_segs:
                assert np.array_equal(_bits(got[s]), _bits(mean[s])), f"segment {s} differs from mdq_gcn_pack's"
        for l, (name, o, i, off_w, off_b) in enumerate(lay):
            w, b = ref.compose32(sd[name + ".weight"].numpy(), sd[name + ".bias"].numpy(), sig[off_w:off_w + o * i].reshape(o, i),
                                 sig[off_b:off_b + o], *eps[name])
            bad = _bits(got[nz.seg_w[l]]) != _bits(w.T.reshape(-1))         # the packed layout is [in][out]
            assert not bad.any(), (name, "weight", int(bad.sum()), np.argwhere(bad)[:4].tolist())
            assert np.array_equal(_bits(got[nz.seg_b[l]]), _bits(b)), (name, "bias")
            assert not np.array_equal(_bits(got[nz.seg_w[l]]), _bits(mean[nz.seg_w[l]])), (name, "no noise arrived")
    print(f"OUT {OUT} {head}: largest |device eps - fp64 eps| over {len(ref.DRAWS)} draws {worst:.3e} (bound {EPS_TOL:.3e})")
    assert worst <= EPS_TOL
    # the same (seed, stream, draw) again: the same bits; another draw, stream or seed: other vectors
    first = ref.DRAWS[0]
    fg.resample(ref.SEED, *first)
    again, eps_again = _packed(fg), _eps(fg)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, seen[first][0]))
    for name in eps_again:
        for a, b in zip(eps_again[name], seen[first][1][name]):
            assert np.array_equal(_bits(a), _bits(b)), name
    fg.resample(ref.SEED + 1, *first)
    other_seed = _eps(fg)
    for name, (e_in, _) in seen[first][1].items():
        for key in ref.DRAWS[1:]:
            assert not np.array_equal(seen[key][1][name][0], e_in), (name, key)
        assert not np.array_equal(other_seed[name][0], e_in), name
    # `_pack()` neither undoes a resample nor keeps the noise after `denoise()`
    fg.resample(ref.SEED, *first)
    fg._pack()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(_packed(fg), seen[first][0]))
    fg.denoise()
    fg._pack()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(_packed(fg), mean))


@functools.lru_cache(maxsize=None)
def _head_graphs(B):
    rng = np.random.default_rng(310 + B)
    graphs = [cases._graph(rng, 9, FIN0) for _ in range(B)]
    return cases.batch_arrays(graphs, range(B))


def _forward(fg, B=17):
    x, node_ptr, esrc, edst, edge_ptr, nmax, emax = _head_graphs(B)
    q = fg.forward_arrays(_dev(x), _dev(node_ptr), _dev(esrc), _dev(edst), _dev(edge_ptr), nmax, emax)
    torch.cuda.synchronize()
    return q.cpu().numpy()


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("OUT", OUTS)
def test_forward_of_a_resampled_copy_is_the_composed_network(lib_built, OUT, head):
    """The fused forward reads the packed copy: with noise it gives the bits of a plain network that holds the composed
    weights; a copy that was never resampled, and one after `denoise()`, give the mean network's."""
    from meshdqn_amd.gcn_fused import FusedGcn
    fg, sd = _noisy_head_net(OUT, head)
    fg.denoise()
    twin = _plain_twin(fg.net)
    q_mean = _forward(FusedGcn(twin))
    assert np.array_equal(_bits(_forward(fg)), _bits(q_mean))
    assert np.array_equal(_bits(_forward(FusedGcn(fg.net))), _bits(q_mean))
    fg.resample(ref.SEED, *ref.DRAWS[0])
    q_noisy = _forward(fg)
    twin.load_state_dict(ref.composed_state_dict(fg.net, _eps(fg)))
    assert np.array_equal(_bits(q_noisy), _bits(_forward(FusedGcn(twin))))
    if not (head == "softmax" and OUT == 1):        # (one softmax output is 1 whatever the weights)
        assert not np.array_equal(_bits(q_noisy), _bits(q_mean))
    fg.denoise()
    assert np.array_equal(_bits(_forward(fg)), _bits(q_mean))


# ------------------------------------------------------------------ 2. the learning step
def _noisy_family(name, head, sigma_zero=False):
    """A dueling_ref family whose network is the noisy one (the family's means, seeded sigmas), on the GPU, resampled."""
    from meshdqn_amd.airfoilgcnn import NodeRemovalNet
    from meshdqn_amd.gcn_fused import FusedGcn
    base = dref.family(name, head)
    net = NodeRemovalNet(**base.kw, head=head, noisy=0.5)
    net.set_num_nodes(base.fin0)
    sd = dict(base.sd)
    rng = np.random.default_rng([1612, base.C])
    s0 = net.noisy_sigma.detach().numpy()
    sd["noisy_sigma"] = torch.from_numpy(np.zeros_like(s0) if sigma_zero else s0 * rng.uniform(0.5, 1.5, s0.shape).astype(np.float32))
    net.load_state_dict(sd)
    fg = FusedGcn(net.cuda())
    fg.resample(ref.SEED, *ref.DRAWS[0])
    return base, fg


@functools.lru_cache(maxsize=None)
def _composed_family(name, head):
    """(the family with the composed weights as its plain state dict and fresh fp64 / fp32 runs, the resampled copy, eps)."""
    base, fg = _noisy_family(name, head)
    eps = _eps(fg)
    dev_eps = _eps_deviation(fg, eps, *ref.DRAWS[0])
    print(f"{name} {head}: largest |device eps - fp64 eps| {dev_eps:.3e} (bound {EPS_TOL:.3e})")
    assert dev_eps <= EPS_TOL
    fam = copy.copy(base)
    fam.sd = ref.composed_state_dict(fg.net, eps)
    fam.net = fg.net
    fam.r64 = [dref.forward_graph(fam.sd, fam.levels, x, ei, fam.ratio, head, np.float64) for x, ei in fam.graphs]
    fam.r32 = [dref.forward_graph(fam.sd, fam.levels, x, ei, fam.ratio, head, np.float32, r["perm"])
               for (x, ei), r in zip(fam.graphs, fam.r64)]
    assert all(a["perm"] == b["perm"] for a, b in zip(fam.r64, base.r64))      # the embedding path carries no noise
    return fam, fg, eps


def _check_sigma_slice(fg, eps, grad, tag):
    """The sigmas' slice of a flat gradient: bit for bit the float32 product of the means' slice and the eps.  Returns
    whether every layer's slice holds a gradient (a launch with gamma 0 in mode 1 has none at all)."""
    lay, live = fg.noisy_layout, True
    for l, (name, o, i, _, _) in enumerate(fg.net.noisy_layout()):
        g_w = grad[lay.mu_w[l]:lay.mu_w[l] + o * i].reshape(o, i)
        g_b = grad[lay.mu_b[l]:lay.mu_b[l] + o]
        want_w, want_b = ref.sigma_grad32(g_w, g_b, *eps[name])
        assert np.array_equal(_bits(grad[lay.sig_w[l]:lay.sig_w[l] + o * i]), _bits(want_w.reshape(-1))), (tag, name, "sigma_w")
        assert np.array_equal(_bits(grad[lay.sig_b[l]:lay.sig_b[l] + o]), _bits(want_b)), (tag, name, "sigma_b")
        live = live and bool(np.any(want_w)) and bool(np.any(want_b))
    return live


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,head", [("T-E32", "softmax"), ("T-E32", "dueling"), ("T-E256", "dueling")])
def test_learning_step_of_a_noisy_copy_against_fp64(lib_built, name, head, mode, weighted):
    fam, fg, eps = _composed_family(name, head)
    yard = dref.yardsticks(fam)
    slices, total = _slices(fg.net)
    mean_total = slices["noisy_sigma"][0]
    assert total == fg.layout.total and slices["noisy_sigma"][1] == total
    steps = dref.steps(fam, mode, weighted)
    worst, bad, live = dict(out=0.0, td=0.0, loss=0.0, grad={}), [], 0
    for li, la in enumerate(fam.launches):
        assert tc.train_accepts(fam, la.nmax, la.emax) is None
        t = dref.transitions(fam, mode, li)
        graphs = [fam.graphs[g] for g in la.idx]
        res = _launch(fg, graphs, la.nmax, la.emax, mode, t, la.gamma, "weighted" if weighted else "td")
        B = len(la.idx)
        # ---- the reduction covers the means; the learning step left the sigmas' slice of every graph at zero, and
        # mdq_noisy_grad filled the flat gradient's from the means' gradients of this launch and this copy's eps
        s = np.zeros(mean_total, np.float32)
        for b in range(B):
            s = s + res["partial"][b, :mean_total]
        assert _same(res["grad"][:mean_total], s) and not np.any(res["partial"][:, mean_total:])
        live += _check_sigma_slice(fg, eps, res["grad"], f"{name} {head} launch {li}")
        loss64, tdfloor = 0.0, 0.0
        for b, g in enumerate(la.idx):
            s64 = steps[li][b][0]
            d_out = cases._norm_dev(res["out"][b], fam.r64[g]["out"])
            worst["out"] = max(worst["out"], d_out)
            if d_out > dref.MARGIN * yard["out"]:
                bad.append(f"launch {li} graph {g} out: {d_out:.3e}, yardstick {yard['out']:.3e}")
            a = int(t["action"][b])
            q = float(fam.r64[g]["out"][a]) if mode == 0 else float(t["q_other"][b, a])
            floor = EPS32 * max(abs(q), abs(q - float(s64["td"])))
            tdfloor = max(tdfloor, floor)
            d_td = abs(float(res["td"][b]) - float(s64["td"]))
            worst["td"] = max(worst["td"], d_td)
            if d_td > max(dref.MARGIN * yard["td"], floor):
                bad.append(f"launch {li} graph {g} td: {d_td:.3e}, yardstick {yard['td']:.3e}, floor {floor:.3e}")
            loss64 += float(s64["term"])
            for key, (lo, hi, shape) in slices.items():
                if key == "noisy_sigma":
                    continue
                got, want = res["partial"][b, lo:hi].reshape(shape), s64["grads"][key]
                if want is None or not np.any(want):
                    assert not np.any(got), f"launch {li} graph {g} {key}: reference exactly zero, device {np.abs(got).max():.3e}"
                    continue
                d = tc.grad_dev(got, s64["grads"], key)
                if d >= worst["grad"].get(key, (0.0, None))[0]:
                    worst["grad"][key] = (d, (li, g))
                if d > dref.MARGIN * yard["grad"][key]:
                    bad.append(f"launch {li} graph {g} {key}: {d:.3e} of its unit, yardstick {yard['grad'][key]:.3e} "
                               f"(ratio {d / yard['grad'][key]:.2f}, bound {dref.MARGIN})")
        d_loss = abs(float(res["loss"]) - loss64)
        worst["loss"] = max(worst["loss"], d_loss)
        if d_loss > max(dref.MARGIN * yard["loss"], tdfloor):
            bad.append(f"launch {li} loss: {d_loss:.3e}, yardstick {yard['loss']:.3e}, floor {tdfloor:.3e}")
    tag = f"noisy {head} family {name} mode {mode} weighted {weighted}"
    for k in ("out", "td", "loss"):
        print(f"{tag} {k}: yardstick {yard[k]:.3e}, device {worst[k]:.3e}, ratio {worst[k] / max(yard[k], 1e-300):.2f}")
    for key, (d, where) in sorted(worst["grad"].items()):
        y = yard["grad"][key]
        print(f"{tag} {key}: worst (launch, graph) {where}: yardstick {y:.3e}, device {d:.3e}, ratio {d / y:.2f} (bound {dref.MARGIN})")
    assert {"lin1.weight", "lin2.bias", "lin3.weight"} <= set(worst["grad"]) and live > 0
    assert not bad, f"{tag}: beyond {dref.MARGIN} x the fp32 yardstick:\n" + "\n".join(bad)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("head", HEADS)
def test_sigma_zero_is_the_plain_network_bit_for_bit(lib_built, head, mode):
    from meshdqn_amd.gcn_fused import FusedGcn
    base, fg = _noisy_family("T-E32", head, sigma_zero=True)
    plain = FusedGcn(_plain_twin(fg.net))
    mean_total, live = fg.noisy_layout.sig_w[0], 0
    for li, la in enumerate(base.launches):
        t = dref.transitions(base, mode, li)
        graphs = [base.graphs[g] for g in la.idx]
        got = _launch(fg, graphs, la.nmax, la.emax, mode, t, la.gamma, "weighted")
        want = _launch(plain, graphs, la.nmax, la.emax, mode, t, la.gamma, "weighted")
        assert want["grad"].shape[0] == mean_total == got["grad"].shape[0] - fg.net.noisy_sigma.numel()
        for k in ("loss", "out", "td"):
            assert _same(got[k], want[k]), (li, k)
        assert _same(got["grad"][:mean_total], want["grad"]) and _same(got["partial"][:, :mean_total], want["partial"])
        live += _check_sigma_slice(fg, _eps(fg), got["grad"], f"sigma 0 {head} launch {li}")   # (the sigmas still get theirs)
    assert live > 0


def test_noisy_grad_through_its_abi_leaves_every_other_slot(lib_built):
    """`mdq_noisy_grad` on a buffer of its own, 40 floats longer than `total`: the sigma slices are the float32 product,
    every other slot (the means, the conv parameters, the floats behind) keeps its bits."""
    from meshdqn_amd import _lib
    fg, _ = _noisy_head_net(21, "dueling")
    fg.resample(ref.SEED, *ref.DRAWS[1])
    eps, lay, total = _eps(fg), fg.noisy_layout, fg.layout.total
    rng = np.random.default_rng(8)
    before = rng.standard_normal(total + 40).astype(np.float32)
    buf = _dev(before)
    rc = fg.lib.mdq_noisy_grad(C.byref(fg.noisy_desc), C.byref(lay), buf.data_ptr(), _lib.stream_ptr(None))
    torch.cuda.synchronize()
    assert rc == 0, fg.lib.mdq_last_error()
    after = buf.cpu().numpy()
    want = before.copy()
    for l, (name, o, i, _, _) in enumerate(fg.net.noisy_layout()):
        w, b = ref.sigma_grad32(before[lay.mu_w[l]:lay.mu_w[l] + o * i].reshape(o, i), before[lay.mu_b[l]:lay.mu_b[l] + o], *eps[name])
        want[lay.sig_w[l]:lay.sig_w[l] + o * i], want[lay.sig_b[l]:lay.sig_b[l] + o] = w.reshape(-1), b
    assert np.array_equal(_bits(after), _bits(want)) and not np.array_equal(_bits(after), _bits(before))


# ------------------------------------------------------------------ 3. refusals
def _clone(st):
    return st.__class__.from_buffer_copy(st)


def test_pack_noisy_refuses_bad_arguments_before_any_launch(lib_built):
    from meshdqn_amd import _lib
    fg, _ = _noisy_head_net(64, "dueling")      # (lin2 and lin3 have 64 rows each: a weight segment can stand in for a bias)
    fg.denoise()
    fg._pack()
    table, nz = fg._table, fg.noisy_desc
    nz.seed, nz.stream, nz.draw = ref.SEED, 0, 0
    cases_ = {}

    def case(what, t=None, z=None, **kw):
        t, z = _clone(table) if t is None else t, _clone(nz) if z is None else z
        for k, v in kw.items():
            obj, field, *idx = k.split("__")
            target = getattr(t if obj == "t" else z, field)
            if idx:
                target[int(idx[0])] = v
            else:
                setattr(t if obj == "t" else z, field, v)
        cases_[what] = (t, z)
    case("n 0", z__n=0)
    case("n 5", z__n=5)
    case("n -1", z__n=-1)
    case("table n 0", t__n=0)
    case("table n 33", t__n=33)
    for f in ("sigma_w", "sigma_b", "eps_in", "eps_out"):
        case(f"NULL {f}", **{f"z__{f}__2": None})
    case("seg_w -1", z__seg_w__1=-1)
    case("seg_w behind the table", z__seg_w__1=table.n)
    case("seg_b behind the table", z__seg_b__3=table.n)
    case("seg_w twice", z__seg_w__1=nz.seg_w[0])
    case("seg_b twice", z__seg_b__1=nz.seg_b[2])
    case("seg_b is seg_w", z__seg_b__1=nz.seg_w[1])
    case("bias rows", z__seg_b__0=nz.seg_b[1])          # lin2's bias (64 rows) for lin1 (128 rows), lin2 then names it twice
    case("bias rows alone", z__n=1, z__seg_b__0=nz.seg_b[1])
    case("bias cols", z__n=1, z__seg_w__0=nz.seg_w[1], z__seg_b__0=nz.seg_w[2])
    case("weight rows 0", **{f"t__rows__{nz.seg_w[0]}": 0})
    outputs = list(fg._keep)        # every packed segment and the eps buffer
    for what, (t, z) in cases_.items():
        for o in outputs:
            o.fill_(POISON)
        rc = fg.lib.mdq_gcn_pack_noisy(C.byref(t), C.byref(z), _lib.stream_ptr(None))
        torch.cuda.synchronize()
        text = (fg.lib.mdq_last_error() or b"").decode()
        print(f"mdq_gcn_pack_noisy, {what}: return code {rc}, text '{text}'")
        assert rc != 0 and "mdq_gcn_pack_noisy" in text, (what, rc, text)
        assert all(bool((o == POISON).all()) for o in outputs), what
    for t, z, what in ((None, nz, "NULL table"), (table, None, "NULL nz")):
        rc = fg.lib.mdq_gcn_pack_noisy(None if t is None else C.byref(t), None if z is None else C.byref(z), _lib.stream_ptr(None))
        torch.cuda.synchronize()
        assert rc != 0 and "mdq_gcn_pack_noisy" in (fg.lib.mdq_last_error() or b"").decode(), what
        assert all(bool((o == POISON).all()) for o in outputs), what
    rc = fg.lib.mdq_gcn_pack_noisy(C.byref(table), C.byref(nz), _lib.stream_ptr(None))       # the call itself was a good one
    torch.cuda.synchronize()
    assert rc == 0 and not any(bool((o == POISON).any()) for o in outputs)
    fg._version = None


def test_noisy_grad_refuses_bad_arguments_before_any_launch(lib_built):
    from meshdqn_amd import _lib
    fg, _ = _noisy_head_net(5, "dueling")
    fg.resample(ref.SEED, *ref.DRAWS[0])
    nz, lay, total = fg.noisy_desc, fg.noisy_layout, fg.layout.total
    bad = {}

    def case(what, **kw):
        z, y = _clone(nz), _clone(lay)
        for k, v in kw.items():
            obj, field, *idx = k.split("__")
            if idx:
                getattr(z if obj == "z" else y, field)[int(idx[0])] = v
            else:
                setattr(z if obj == "z" else y, field, v)
        bad[what] = (z, y)
    case("n 0", z__n=0)
    case("n 5", z__n=5)
    case("NULL eps_in", z__eps_in__0=None)
    case("NULL eps_out", z__eps_out__3=None)
    case("out 0", y__out__1=0)
    case("in -1", y__in__1=-1)
    case("sig_w behind total", y__sig_w__3=total - 10)
    case("sig_b behind total", y__sig_b__3=total)
    case("mu_w negative", y__mu_w__0=-1)
    case("total too small", y__total=total - 1)
    case("sigma slice on its mean", y__sig_w__0=lay.mu_w[0])
    case("sigma slices of two layers overlap", y__sig_w__1=lay.sig_w[0] + 1)
    case("sig_b inside sig_w", y__sig_b__2=lay.sig_w[2])
    before = np.random.default_rng(3).standard_normal(total).astype(np.float32)
    buf = _dev(before)
    for what, (z, y) in bad.items():
        rc = fg.lib.mdq_noisy_grad(C.byref(z), C.byref(y), buf.data_ptr(), _lib.stream_ptr(None))
        torch.cuda.synchronize()
        text = (fg.lib.mdq_last_error() or b"").decode()
        print(f"mdq_noisy_grad, {what}: return code {rc}, text '{text}'")
        assert rc != 0 and "mdq_noisy_grad" in text, (what, rc, text)
        assert np.array_equal(_bits(buf.cpu().numpy()), _bits(before)), what
    for args, what in (((None, C.byref(lay), buf.data_ptr()), "NULL nz"), ((C.byref(nz), None, buf.data_ptr()), "NULL lay"),
                       ((C.byref(nz), C.byref(lay), None), "NULL grad")):
        rc = fg.lib.mdq_noisy_grad(*args, _lib.stream_ptr(None))
        torch.cuda.synchronize()
        assert rc != 0 and "mdq_noisy_grad" in (fg.lib.mdq_last_error() or b"").decode(), what
        assert np.array_equal(_bits(buf.cpu().numpy()), _bits(before)), what
    rc = fg.lib.mdq_noisy_grad(C.byref(nz), C.byref(lay), buf.data_ptr(), _lib.stream_ptr(None))
    torch.cuda.synchronize()
    assert rc == 0 and not np.array_equal(_bits(buf.cpu().numpy()), _bits(before))


# ------------------------------------------------------------------ 4. chain and loop
M_LOOP = STEPS - (-(-BATCH // B_ENV))
NOISY = dict(sigma0=0.5)


@pytest.fixture(scope="module")
def base_env(lib_built):
    from meshdqn_amd.env import Env2DAirfoil
    return Env2DAirfoil(_cfg())


@pytest.fixture(scope="module")
def run_default(base_env):
    return _run(base_env)


@pytest.fixture(scope="module")
def run_noisy(base_env, record_explore):
    record_explore.clear()
    out, tr = _run(base_env, noisy=NOISY)
    return out, tr, list(record_explore)


@pytest.fixture(scope="module")
def record_explore():
    """Every `explore` table the loop hands to `VecEnv2DAirfoil.rollout_begin` while the fixture lives (the stream
    calibration steps the environments with random tables of its own: not recorded)."""
    from meshdqn_amd.trainer import DQNTrainer
    from meshdqn_amd.vec_env import VecEnv2DAirfoil
    seen, calibrating, orig, orig_cal = [], [], VecEnv2DAirfoil.rollout_begin, DQNTrainer.calibrate_opt_stream

    def spy(self, steps, explore=None, rand_actions=None, actions=None):
        if explore is not None and not calibrating:
            seen.append(np.array(explore, copy=True))
        return orig(self, steps, explore, rand_actions, actions)

    def cal(self, *args, **kw):
        calibrating.append(1)
        try:
            return orig_cal(self, *args, **kw)
        finally:
            calibrating.pop()
    VecEnv2DAirfoil.rollout_begin, DQNTrainer.calibrate_opt_stream = spy, cal
    yield seen
    VecEnv2DAirfoil.rollout_begin, DQNTrainer.calibrate_opt_stream = orig, orig_cal


def test_noisy_double_chain_shares_one_draw_per_network(run_default):
    """`optimize_device` of a noisy Double-DQN trainer against the same chain by hand: the online network's forward on s'
    and its learning step see the draw the counters name, and the sigma slice of the flat gradient is built from that
    draw's eps."""
    import random
    import target_net_ref
    from meshdqn_amd.gcn_fused import FusedGcn
    rep = run_default[1].device_memory
    dev, N, EM = rep.R.device, rep.N, rep.e_max
    tr = _trainer(target_net=dict(kind="double", period=3), head="dueling", noisy=NOISY)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in tr.policy_net_2.parameters():
            p.add_((0.05 * torch.randn(p.shape, generator=g)).to(p.device))
    hand1, hand2 = FusedGcn(copy.deepcopy(tr.policy_net_1)), FusedGcn(copy.deepcopy(tr.policy_net_2))
    sigma1, sigma2 = tr.policy_net_1.noisy_sigma.detach().clone(), tr.policy_net_2.noisy_sigma.detach().clone()
    seed = tr.noisy["seed"]
    tr.noise_draws.update(train1=7, train2=(1 << 33) + 2)
    random.seed(77)
    idx = rep.draw(9, BATCH)
    loss, sel = torch.zeros(1, device=dev), torch.zeros(BATCH, dtype=torch.int32, device=dev)
    tr.optimize_device(rep, idx, loss_out=loss, sel_out=sel)
    torch.cuda.synchronize()
    assert tr.noise_draws == dict(act1=0, train1=8, train2=(1 << 33) + 3) and seed == 1370       # (the trainer's default seed)
    f1 = tr._fused_of(tr.policy_net_1, "train")
    flat = next(iter(f1._train_bufs.values()))["grad"].cpu().numpy()
    eps1 = _eps(f1)
    f2 = tr._fused_of(tr.policy_net_2, "train")
    devs = _eps_deviation(f1, eps1, 1, 7, seed=seed), _eps_deviation(f2, _eps(f2), 2, (1 << 33) + 2, seed=seed)
    print(f"chain: largest |device eps - fp64 eps| {max(devs):.3e} (bound {EPS_TOL:.3e})")
    assert max(devs) <= EPS_TOL
    assert _check_sigma_slice(f1, eps1, flat, "chain")
    b = tr._mb_bufs
    gs = (b["x_s"], b["node_ptr"], b["esrc_s"], b["edst_s"], b["edge_ptr_s"])
    gn = (b["x_n"], b["node_ptr"], b["esrc_n"], b["edst_n"], b["edge_ptr_n"])
    # ---- by hand on copies of the networks as they were, with the same draws
    hand1.resample(seed, 1, 7)
    hand2.resample(seed, 2, (1 << 33) + 2)
    q_o, q_t = hand1.forward_arrays(*gn, N, EM).cpu().numpy(), hand2.forward_arrays(*gn, N, EM).cpu().numpy()
    want_q, want_sel, _ = target_net_ref.select(q_o, q_t)
    assert np.array_equal(sel.cpu().numpy(), want_sel)
    loss_1, flat_1 = hand1.train_step(*gs, N, EM, 0, torch.from_numpy(want_q).to(dev), b["action"], b["reward"], b["nonfinal"], tr.gamma)
    torch.cuda.synchronize()
    assert torch.equal(loss.view(torch.int32), loss_1.view(torch.int32)) and np.isfinite(float(loss))
    assert np.array_equal(_bits(flat), _bits(flat_1.cpu().numpy()))
    # the mean network's forward chooses differently somewhere, or at least puts out other values
    hand1.denoise()
    assert not np.array_equal(hand1.forward_arrays(*gn, N, EM).cpu().numpy(), q_o)
    # mdq_adam_step took the sigmas as one more segment; after `period` steps mdq_target_update has copied them
    assert not torch.equal(tr.policy_net_1.noisy_sigma, sigma1) and torch.equal(tr.policy_net_2.noisy_sigma, sigma2)
    assert not torch.equal(sigma1, sigma2)
    tr.optimize_device(rep, idx)
    tr.optimize_device(rep, idx)
    torch.cuda.synchronize()
    assert tr.num_grads == 3 and torch.equal(tr.policy_net_2.noisy_sigma, tr.policy_net_1.noisy_sigma)
    assert all(torch.equal(p, q) for p, q in zip(tr.policy_net_1.parameters(), tr.policy_net_2.parameters()))


def test_loop_with_noisy_networks_is_reproducible(base_env, run_noisy):
    a, ta, explore = run_noisy
    b, tb = _run(base_env, noisy=NOISY)
    _same_run(a, ta, b, tb)
    assert ta.noisy == dict(sigma0=0.5, seed=1370) and len(a["losses"]) == M_LOOP and np.isfinite(a["losses"]).all()
    assert ta.noise_draws == dict(act1=STEPS, train1=M_LOOP, train2=M_LOOP) == tb.noise_draws
    init = _trainer(noisy=NOISY)
    for net, net0 in ((ta.policy_net_1, init.policy_net_1), (ta.policy_net_2, init.policy_net_2)):
        assert all(torch.isfinite(p).all() for p in net.parameters())
        assert not torch.equal(net.noisy_sigma, net0.noisy_sigma)            # the sigmas were trained
        assert not torch.equal(net.lin1.weight, net0.lin1.weight)
    # no epsilon-greedy: every table the loop handed to the environment is all false
    assert explore and sum(len(e) for e in explore) == STEPS and not any(e.any() for e in explore)
    # another noise seed: other actions
    c, tc_ = _run(base_env, noisy=dict(sigma0=0.5, seed=24))
    assert tc_.noisy["seed"] == 24 and not np.array_equal(c["actions"], a["actions"])


def test_loop_with_noisy_none_named_is_the_default_loop(base_env, run_default):
    out, tr = run_default
    assert tr.noisy is None and len(out["losses"]) == M_LOOP
    named, tn = _run(base_env, noisy=None)
    _same_run(out, tr, named, tn)
    assert [k for k, _ in tn.policy_net_1.named_parameters()] == [k for k, _ in tr.policy_net_1.named_parameters()]
    assert tn.noise_draws == dict(act1=0, train1=0, train2=0)
    assert tr._fused_of(tr.policy_net_1)._noise is None and tr._fused_of(tr.policy_net_1).noisy_desc is None


def test_inference_of_a_trained_noisy_network_is_its_mean(run_noisy):
    """After the loop `select_action` (the acting copy the loop resampled) and a fresh fused forward give the bits of the plain
    network that holds the mean parameters."""
    from meshdqn_amd.data import Data
    from meshdqn_amd.gcn_fused import FusedGcn
    _, tr, _ = run_noisy
    net = tr.policy_net_1
    twin = _plain_twin(net)
    rng = np.random.default_rng(12)
    x, ei = cases._graph(rng, 180, FIN0)
    data = Data(x=torch.from_numpy(x).float(), edge_index=torch.from_numpy(ei).long()).to("cuda")
    q_twin = twin.forward_fused(data)
    assert torch.equal(net.forward_fused(data).view(torch.int32), q_twin.view(torch.int32))
    assert tr.select_action(data) == int(q_twin.argmax().item())
    assert torch.equal(FusedGcn(net).forward(data).view(torch.int32), q_twin.view(torch.int32))
    act = tr._fused_of(net)
    act.resample(tr.noisy["seed"], 0, 5)
    assert not torch.equal(act.forward(data), q_twin)                      # (the copy does carry noise when asked)
    act.denoise()
    assert torch.equal(act.forward(data).view(torch.int32), q_twin.view(torch.int32))


def test_train_py_with_noisy_networks_and_a_restart(lib_built, tmp_path):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ray_ys930.yaml")))
    cfg["flow_config"]["geometry_params"]["mesh"] = os.path.join(ROOT, "tests", "golden", "ys930.npz")
    cfg["agent_params"].update(solver_steps=20, save_steps=4)
    cfg["optimizer"]["batch_size"] = BATCH
    cpath = os.path.join(str(tmp_path), "cfg.yaml")
    yaml.safe_dump(cfg, open(cpath, "w"))
    save = os.path.join(str(tmp_path), "run")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, "train.py", "--config", cpath, "--envs", str(B_ENV), "--steps", "6", "--noisy-net", "--save-dir", save,
           "--save-every", "0"]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    n_opt = 6 - (-(-BATCH // B_ENV))
    losses = np.load(os.path.join(save, "losses.npy"))
    assert len(losses) == n_opt and np.isfinite(losses).all()
    assert not np.load(os.path.join(save, "eps.npy")).any()                # the logged epsilon is 0
    # (the reference's toggle trains policy_net_2 in the first `target_update` = 50 gradient steps)
    sd = torch.load(os.path.join(save, "policy_net_2.pt"), map_location="cpu")
    assert list(torch.load(os.path.join(save, "policy_net_1.pt"), map_location="cpu"))[0] == "noisy_sigma"
    assert not torch.equal(sd["noisy_sigma"], torch.load(os.path.join(save, "policy_net_1.pt"), map_location="cpu")["noisy_sigma"])
    assert "noisy_sigma" in sd and tuple(sd["noisy_sigma"].shape) == (256 * 128 + 128 + 128 * 64 + 64 + 64 * 181 + 181,)
    st = torch.load(os.path.join(save, "trainer_state.pt"), map_location="cpu", weights_only=False)
    assert st["noise_draws"] == dict(act1=6, train1=n_opt, train2=n_opt)
    # the checkpoint restarts: the counters go on
    out = subprocess.run(cmd + ["--restart"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    st = torch.load(os.path.join(save, "restart_trainer_state.pt"), map_location="cpu", weights_only=False)
    assert st["noise_draws"]["act1"] == 12 and st["noise_draws"]["train1"] > n_opt
    sd2 = torch.load(os.path.join(save, "restart_policy_net_2.pt"), map_location="cpu")
    assert torch.isfinite(sd2["noisy_sigma"]).all() and not torch.equal(sd2["noisy_sigma"], sd["noisy_sigma"])
