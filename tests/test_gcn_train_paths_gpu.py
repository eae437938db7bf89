"""The fused learning step (gcn_train_kernel + gcn_grad_reduce_kernel, meshdqn_amd/csrc/mdq_gcn_train.hip), family by
family against the fp64 reference of tests/gcn_ref64.py (forward, loss term, backward).

The graphs of tests/gcn_train_cases.py were drawn until no decision of the fp64 run (relu of a kept row, first maximum
of a readout column, head relu, mode-1 argmax, TopK cut and order) is closer than 16 fp32 yardsticks to flipping, so
EVERY graph is compared, with no exclusion and no tie branch:
 * the selection on the tape (`perm` of every level, the readout's `amax`) equals the reference's exactly;
 * outputs, TD errors, loss and the per-graph gradient of every parameter (the caller-owned `partial` slices) are
   within MARGIN = 4 x the family's fp32 yardstick (fp32 run of the same reference against its fp64 run; the device
   uses other summation orders of the same lengths and its own tanhf / sqrtf / expf), each parameter in units of
   max(its own largest gradient, 1e-3 of the graph's largest);
 * blocks whose reference is exactly zero (the weight of an edgeless level, a mode-1 terminal graph, a weight of 0,
   parameters the forward never touches) are exactly zero on the device;
 * the flat gradient and the loss are bit for bit the sequential fp32 sums of the slices / loss terms in graph order.
The input conditions are asserted without a GPU in test_gcn_train_ref64_cpu.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gcn_path_cases as cases
import gcn_train_cases as tc

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
VARIANTS = ("plain", "td", "weighted")       # neither weight nor td (mdq_gcn_train_step) / td only / both


@functools.lru_cache(maxsize=None)
def _fused(name):
    from meshdqn_amd.gcn_fused import FusedGcn
    return FusedGcn(tc.family(name)[0].net.cuda())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _slices(net):
    out, off = {}, 0
    for k, p in net.named_parameters():
        out[k] = (off, off + p.numel(), tuple(p.shape))
        off += p.numel()
    return out, off


def _run(fg, graphs, nmax, emax, mode, t, gamma, variant="weighted", weight=None):
    """One launch through `FusedGcn.train_step` over `graphs` ((x, edge_index) pairs) with the transition arrays `t`:
    numpy copies of loss, grad, out, td, the per-graph slices `partial` and the workspace rows."""
    x, node_ptr, esrc, edst, edge_ptr, _, _ = cases.batch_arrays(graphs, range(len(graphs)))
    B = len(graphs)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    w = None
    if variant == "weighted":
        w = dev(t["weight"][:B] if weight is None else weight)
    td = torch.full((B,), 7.5, dtype=torch.float32, device="cuda") if variant != "plain" else None
    loss, grad, out = fg.train_step(dev(x), dev(node_ptr), dev(esrc), dev(edst), dev(edge_ptr), nmax, emax, mode,
                                    dev(t["q_other"][:B]), dev(t["action"][:B]), dev(t["reward"][:B]), dev(t["nonfinal"][:B]),
                                    gamma, want_out=True, weight=w, td_out=td)
    torch.cuda.synchronize()
    bufs = fg._train_bufs[(B, int(nmax), int(emax))]
    return dict(loss=loss.cpu().numpy()[0], grad=grad.cpu().numpy(), out=out.cpu().numpy(),
                td=None if td is None else td.cpu().numpy(), partial=bufs["partial"].cpu().numpy(), ws=bufs["ws"].cpu().numpy())


def _check_reduce(res, B):
    """`gcn_grad_reduce_kernel`, exactly: sums in graph order, in fp32."""
    s = np.zeros_like(res["partial"][0])
    term = np.float32(0)
    for b in range(B):
        s = s + res["partial"][b]
        term = term + res["ws"][b, 0]
    assert _same(res["grad"], s), "flat gradient is not the sequential fp32 sum of the slices"
    assert _same(res["loss"], term / np.float32(B)), (res["loss"], term / np.float32(B))


def _compare_launch(name, mode, variant, li, report):
    fam, r64, _, launches, _ = tc.family(name)
    la, yard = launches[li], tc.yardsticks(name)
    t = tc.transitions(name, mode, li)
    steps = tc.steps(name, mode, variant == "weighted")[li]
    fg = _fused(name)
    res = _run(fg, [fam.graphs[g] for g in la.idx], la.nmax, la.emax, mode, t, la.gamma, variant)
    B = len(la.idx)
    stride, offs = tc.tape_layout(fam, la.nmax, la.emax)
    assert stride == int(fg.lib.mdq_gcn_train_workspace(C.byref(fg.desc), la.nmax, la.emax)) == res["ws"].shape[1]
    slices, total = _slices(fam.net)
    assert total == res["partial"].shape[1]
    _check_reduce(res, B)
    loss64, tdfloor = 0.0, 0.0
    for b, g in enumerate(la.idx):
        s64 = steps[b][0]
        n = len(fam.graphs[g][0])
        # ---- selection on the tape
        ints = res["ws"][b].view(np.int32)
        for l, nl in enumerate(fam.level_sizes(n)):
            k = tc._ceil(fam.ratio, nl)
            perm = ints[offs[l]["perm"]:offs[l]["perm"] + k].tolist()
            assert perm == r64[g]["perm"][l], f"{name} launch {li} graph {g} level {l}: perm {perm}, reference {r64[g]['perm'][l]}"
            amax = ints[offs[l]["amax"]:offs[l]["amax"] + fam.C]
            live = r64[g]["tape"][l]["xp"].max(axis=0) != 0
            assert np.array_equal(amax[live], s64["amax"][l][live]), (name, li, g, l)
        # ---- outputs, TD error, loss term
        d_out = cases._norm_dev(res["out"][b], r64[g]["out"])
        report["out"] = max(report.get("out", 0.0), d_out)
        if d_out > tc.MARGIN * yard["out"]:
            report["bad"].append(f"launch {li} graph {g} out: {d_out:.3e}, yardstick {yard['out']:.3e}")
        a = int(t["action"][b])
        q = float(r64[g]["out"][a]) if mode == 0 else float(t["q_other"][b, a])
        floor = EPS32 * max(abs(q), abs(q - float(s64["td"])))
        tdfloor = max(tdfloor, floor)
        if res["td"] is not None:
            d_td = abs(float(res["td"][b]) - float(s64["td"]))
            report["td"] = max(report.get("td", 0.0), d_td)
            if d_td > max(tc.MARGIN * yard["td"], floor):
                report["bad"].append(f"launch {li} graph {g} td: {d_td:.3e}, yardstick {yard['td']:.3e}, floor {floor:.3e}")
        loss64 += float(s64["term"])
        # ---- the graph's gradient, parameter by parameter
        for key, (lo, hi, shape) in slices.items():
            got, want = res["partial"][b, lo:hi].reshape(shape), s64["grads"][key]
            if want is None or not np.any(want):
                assert not np.any(got), f"{name} launch {li} graph {g} {key}: reference exactly zero, device {np.abs(got).max():.3e}"
                continue
            d = tc.grad_dev(got, s64["grads"], key)
            cur = report["grad"].get(key, (0.0, None))
            if d >= cur[0]:
                report["grad"][key] = (d, (li, g))
            if d > tc.MARGIN * yard["grad"][key]:
                report["bad"].append(f"launch {li} graph {g} {key}: {d:.3e} of its unit, yardstick {yard['grad'][key]:.3e} "
                                     f"(ratio {d / yard['grad'][key]:.2f}, bound {tc.MARGIN})")
    d_loss = abs(float(res["loss"]) - loss64)
    report["loss"] = max(report.get("loss", 0.0), d_loss)
    if d_loss > max(tc.MARGIN * yard["loss"], tdfloor):
        report["bad"].append(f"launch {li} loss: {d_loss:.3e}, yardstick {yard['loss']:.3e}, floor {tdfloor:.3e}")
    return res


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", tc.FAMILIES)
def test_family_against_fp64(lib_built, name, mode, variant):
    fam, _, _, launches, _ = tc.family(name)
    yard = tc.yardsticks(name)
    report = dict(grad={}, bad=[])       # (every figure is printed before the bounds are asserted)
    forms = set()
    for li, la in enumerate(launches):
        assert tc.train_accepts(fam, la.nmax, la.emax) is None
        forms |= tc.launch_forms(fam, la)
        _compare_launch(name, mode, variant, li, report)
    assert tc.EXPECTED_FORMS[name] <= forms
    tag = f"family {name} mode {mode} {variant}"
    print(f"{tag}: forms {sorted(forms)}")
    for k in ("out", "td", "loss"):
        if k in report:
            print(f"{tag} {k}: yardstick {yard[k]:.3e}, device {report[k]:.3e}, ratio {report[k] / yard[k]:.2f}")
    classes = {}
    for key, (d, where) in report["grad"].items():
        r = d / yard["grad"][key]
        c = tc.param_class(key)
        if c not in classes or r > classes[c][0]:
            classes[c] = (r, key, yard["grad"][key], d, where)
    for c, (r, key, y, d, where) in sorted(classes.items()):
        print(f"{tag} {c}: worst {key} (launch, graph) {where}: yardstick {y:.3e}, device {d:.3e}, ratio {r:.2f} (bound {tc.MARGIN})")
    assert not report["bad"], f"{tag}: beyond {tc.MARGIN} x the fp32 yardstick:\n" + "\n".join(report["bad"])


@pytest.mark.parametrize("name", ["T-A", "T-C"])
def test_a_weight_table_of_ones_gives_the_bits_of_none(lib_built, name):
    fam, _, _, launches, _ = tc.family(name)
    la = launches[0]
    graphs = [fam.graphs[g] for g in la.idx]
    for mode in (0, 1):
        t = tc.transitions(name, mode, 0)
        a = _run(_fused(name), graphs, la.nmax, la.emax, mode, t, la.gamma, "td")
        b = _run(_fused(name), graphs, la.nmax, la.emax, mode, t, la.gamma, "weighted", weight=np.ones(len(graphs), dtype=np.float32))
        for k in ("loss", "grad", "out", "td", "partial"):
            assert _same(a[k], b[k]), (mode, k)
        assert np.any(a["grad"])


# ---------------------------------------------------------------------------------------------- refusals inside a launch
@pytest.mark.parametrize("what", ["nodes", "edges", "empty"])
def test_refused_graph_inside_a_launch(lib_built, what):
    """A graph with more nodes than NMAX, more edges than EMAX or no nodes at all in the middle of a T-B minibatch: NaN
    loss and TD error, an all-zero gradient slice (which held the harmless graph's gradient from the launch before), and
    every other graph's slice and TD error bitwise what the same launch gives with a harmless graph in that slot."""
    name = "T-B"
    fam, _, _, _, _ = tc.family(name)
    sizes = [len(x) for x, _ in fam.graphs]
    assert sizes[:6] == [77, 85, 155, 163, 180, 180] and fam.graphs[5][1].shape[1] == 360
    empty = (np.zeros((0, fam.fin0), dtype=np.float32), np.zeros((2, 0), dtype=np.int64))
    offender, nmax, emax = dict(nodes=(fam.graphs[4], 163, 360), edges=(fam.graphs[5], 180, 330), empty=(empty, 180, 360))[what]
    assert tc.train_accepts(fam, nmax, emax) is None
    rest = [fam.graphs[g] for g in (0, 1, 3, 2)]
    assert all(len(x) <= nmax and ei.shape[1] <= emax for x, ei in rest)
    assert len(offender[0]) > nmax or offender[1].shape[1] > emax or len(offender[0]) == 0
    t = tc.transitions(name, 0, 0)
    fg = _fused(name)
    good = _run(fg, rest[:2] + [fam.graphs[0]] + rest[2:], nmax, emax, 0, t, 0.9)
    assert np.isfinite(good["loss"]) and np.any(good["partial"][2])
    bad = _run(fg, rest[:2] + [offender] + rest[2:], nmax, emax, 0, t, 0.9)
    assert np.isnan(bad["loss"]) and np.isnan(bad["td"][2]) and np.isnan(bad["ws"][2, 0])
    assert not np.any(bad["partial"][2])
    for b in (0, 1, 3, 4):
        assert _same(bad["partial"][b], good["partial"][b]) and _same(bad["td"][b], good["td"][b]), b
        assert _same(bad["out"][b], good["out"][b])
    assert np.isfinite(bad["grad"]).all()
    s = np.zeros_like(bad["grad"])
    for b in range(5):
        s = s + bad["partial"][b]
    assert _same(bad["grad"], s)          # the refused graph adds nothing to the flat gradient


# ---------------------------------------------------------------------------------------------- the C ABI, directly
def _abi_buffers(fam, graphs, nmax, emax, B, guard=0, sentinel=-777.25):
    """Device arrays of one direct call: inputs of `graphs`, and sentinel-filled outputs with `guard` extra floats each."""
    x, node_ptr, esrc, edst, edge_ptr, _, _ = cases.batch_arrays(graphs, range(len(graphs)))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    stride, _ = tc.tape_layout(fam, nmax, emax)
    total = _slices(fam.net)[1]
    full = lambda n: torch.full((n + guard,), sentinel, dtype=torch.float32, device="cuda")   # noqa: E731
    nb = max(B, 1)
    return dict(x=dev(x), node_ptr=dev(node_ptr), esrc=dev(esrc), edst=dev(edst), edge_ptr=dev(edge_ptr), stride=stride, total=total,
                workspace=full(nb * stride), partial=full(nb * total), grad=full(total), loss=full(1), out=full(nb * fam.out_dim), td=full(nb))


def _abi_call(fg, buf, B, nmax, emax, mode, t, gamma, null=(), with_td=True):
    from meshdqn_amd import _lib
    from meshdqn_amd.gcn_fused import GcnTrainDesc
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    keep = [dev(t["q_other"]), dev(t["action"]), dev(t["reward"]), dev(t["nonfinal"])]
    d = GcnTrainDesc()
    d.B, d.NMAX, d.EMAX, d.mode, d.gamma = B, nmax, emax, mode, gamma
    for k in ("x", "node_ptr", "esrc", "edst", "edge_ptr", "workspace", "partial", "grad", "loss", "out"):
        setattr(d, k, None if k in null else buf[k].data_ptr())
    d.q_other, d.action, d.reward, d.nonfinal = (k.data_ptr() for k in keep)
    d.layout = fg.layout
    rc = fg.lib.mdq_gcn_train_step_weighted(C.byref(fg.desc), C.byref(d), None, buf["td"].data_ptr() if with_td else None,
                                            _lib.stream_ptr(None))
    torch.cuda.synchronize()
    return rc, (fg.lib.mdq_last_error() or b"").decode()


ENTRY_CASES = list(tc.REFUSALS) + ["no graphs", "no partial"]


@pytest.mark.parametrize("case", ENTRY_CASES)
def test_refusals_at_the_entry(lib_built, case):
    """One step past each limit of `mdq_gcn_train_step_weighted`: the call returns nonzero with a text and writes
    nothing - `grad`, `partial`, `loss`, `td`, `out` and the workspace keep their sentinels."""
    from meshdqn_amd.gcn_fused import FusedGcn
    if case in tc.REFUSALS:
        _, nmax, emax, limit, _ = tc.REFUSALS[case]
        fam = tc.refusal_network(case)
        assert tc.train_accepts(fam, nmax, emax) == limit
        B, null = 2, ()
    else:
        fam, nmax, emax, limit = tc.family("T-E32")[0], 41, 82, "arguments"
        assert tc.train_accepts(fam, nmax, emax) is None
        B, null = (0, ()) if case == "no graphs" else (2, ("partial",))
    fg = FusedGcn(fam.net.cuda())
    fg._pack()
    rng = np.random.default_rng(5)
    graphs = [cases._graph(rng, 9, fam.fin0) for _ in range(2)]
    t = dict(q_other=rng.random((2, fam.out_dim)).astype(np.float32), action=np.zeros(2, dtype=np.int64),
             reward=np.zeros(2, dtype=np.float32), nonfinal=np.ones(2, dtype=np.float32))
    buf = _abi_buffers(fam, graphs, nmax, emax, 2)
    rc, text = _abi_call(fg, buf, B, nmax, emax, 0, t, 0.9, null)
    print(f"entry refusal '{case}' (limit: {limit}): return code {rc}, text '{text}'")
    assert rc != 0 and text
    for k in ("workspace", "partial", "grad", "loss", "out", "td"):
        assert bool((buf[k] == -777.25).all()), k


def test_guard_floats_behind_every_output_stay_untouched(lib_built):
    """T-A's first launch through the C ABI with the workspace at exactly `mdq_gcn_train_workspace()` floats per graph
    and 1024 guard floats behind workspace, partial, grad, out and td, everything filled with a sentinel: the guards keep
    their value, and the results are bitwise those of `FusedGcn.train_step` in its zeroed buffers - the kernel reads
    nothing of the workspace it has not written."""
    name = "T-A"
    fam, _, _, launches, _ = tc.family(name)
    la = launches[0]
    graphs = [fam.graphs[g] for g in la.idx]
    B = len(graphs)
    fg = _fused(name)
    t = tc.transitions(name, 0, 0)
    want = _run(fg, graphs, la.nmax, la.emax, 0, t, la.gamma, "td")
    G = 1024
    buf = _abi_buffers(fam, graphs, la.nmax, la.emax, B, guard=G)
    assert buf["stride"] == int(fg.lib.mdq_gcn_train_workspace(C.byref(fg.desc), la.nmax, la.emax))
    rc, text = _abi_call(fg, buf, B, la.nmax, la.emax, 0, t, la.gamma)
    assert rc == 0, text
    for k in ("workspace", "partial", "grad", "out", "td"):
        assert bool((buf[k][-G:] == -777.25).all()), k
    # slots of the parameters the forward never touches are not written at all (`FusedGcn` hands over zeroed buffers)
    slices, total = _slices(fam.net)
    used = np.zeros(total, dtype=bool)
    for key, g in tc.steps(name, 0, False)[0][0][0]["grads"].items():
        if g is not None:
            used[slices[key][0]:slices[key][1]] = True
    assert used.any() and not used.all()
    grad, partial = buf["grad"][:-G].cpu().numpy(), buf["partial"][:-G].cpu().numpy().reshape(B, total)
    assert (partial[:, ~used] == -777.25).all()
    assert _same(grad[used], want["grad"][used]) and _same(partial[:, used], want["partial"][:, used])
    assert _same(buf["loss"][:1].cpu().numpy(), want["loss"])
    assert _same(buf["td"][:-G].cpu().numpy(), want["td"]) and _same(buf["out"][:-G].cpu().numpy(), want["out"].reshape(-1))


def test_stale_buffers_do_not_leak(lib_built):
    """Minibatch X and then minibatch Y in the same workspace / `partial`: bitwise the results of Y in fresh zeroed
    buffers (Y in mode 1 has terminal graphs, whose slices held X's gradients); a relaunch is bitwise equal."""
    from meshdqn_amd.gcn_fused import FusedGcn
    name = "T-C"
    fam, _, _, launches, _ = tc.family(name)
    la = launches[0]
    gx = [fam.graphs[g] for g in la.idx]
    gy = gx[::-1]
    tx, ty = tc.transitions(name, 0, 0), tc.transitions(name, 1, 0)
    assert (ty["nonfinal"] == 0).any()
    fg = _fused(name)
    x = _run(fg, gx, la.nmax, la.emax, 0, tx, 0.9)
    y = _run(fg, gy, la.nmax, la.emax, 1, ty, 0.9)
    y2 = _run(fg, gy, la.nmax, la.emax, 1, ty, 0.9)
    fresh = _run(FusedGcn(fam.net.cuda()), gy, la.nmax, la.emax, 1, ty, 0.9)
    assert np.any(x["partial"]) and np.any(y["partial"]) and not _same(x["grad"], y["grad"])
    for k in ("loss", "grad", "out", "td", "partial"):
        assert _same(y[k], fresh[k]), k
        assert _same(y2[k], y[k]), k


def test_forms_b_and_d_give_the_same_bits_in_the_training_instance(lib_built):
    """The same 40-node graph beside a copy of itself (NMAX 40: form (b)) and beside the 100-node graph (NMAX 100: form
    (d)), same B: its gradient slice, TD error and outputs bit for bit - DESIGN.md's claim that every dense form performs
    the same fma chain per output, for the instance of `run_level` the inference tests never launch."""
    name = "T-C"
    fam, _, _, launches, _ = tc.family(name)
    alone, wide = launches[2], launches[3]
    assert alone.idx == [7, 7] and wide.idx == [7, 0] and len(fam.graphs[7][0]) == 40
    fa, fw = fam.forms(7, alone.nmax), fam.forms(7, wide.nmax)
    print(f"40-node graph: NMAX {alone.nmax} {fa}, NMAX {wide.nmax} {fw}")
    assert any(a.startswith("b") and w.startswith("d") for a, w in zip(fa, fw))
    t = tc.transitions(name, 0, 2)
    fg = _fused(name)
    a = _run(fg, [fam.graphs[g] for g in alone.idx], alone.nmax, alone.emax, 0, t, 0.9)
    w = _run(fg, [fam.graphs[g] for g in wide.idx], wide.nmax, wide.emax, 0, t, 0.9)
    assert np.any(a["partial"][0])
    assert _same(a["out"][0], w["out"][0]) and _same(a["td"][0], w["td"][0]) and _same(a["ws"][0, 0], w["ws"][0, 0])
    assert _same(a["partial"][0], w["partial"][0]), float(np.abs(a["partial"][0] - w["partial"][0]).max())
