"""The fp64 reference of the learning step (tests/gcn_ref64.py: loss term + backward) checked without a GPU: against
central finite differences of its own forward, against the oracle's learning step - and the INPUT CONDITIONS the GPU
comparison of test_gcn_train_paths_gpu.py relies on (tests/gcn_train_cases.py): no decision of an accepted graph close
to flipping, few candidates rejected, every launch accepted by the restated limits, every refusal case one step past the
limit it names, the dispatch forms reached, every class of transition data present."""
import math

import numpy as np
import pytest
import torch

import gcn_ref64 as ref
import gcn_train_cases as tc

EPS64 = float(np.finfo(np.float64).eps)


def _term(fam, sd, x, ei, perm, args):
    res = ref.forward_graph(sd, fam.levels, x, ei, fam.ratio, fam.softmax, np.float64, perm)
    return float(ref.loss_graph(res["out"], *args)[0])


@pytest.mark.parametrize("name,g", [("T-E32", 3), ("T-C", 4)])
@pytest.mark.parametrize("mode,weight", [(0, None), (0, 3.5), (1, None), (1, 0.25)])
def test_backward_against_finite_differences(name, g, mode, weight):
    """d term / d parameter along 8 random directions per parameter against central differences of the fp64 forward +
    loss with the selection forced.  The bound comes from the step itself: D(h) - D(h/2) is three times the truncation
    error of D(h/2) when the error falls fourfold per halving (Richardson), so |D(h/2) - g.v| <= |D(h) - D(h/2)| + the
    round-off of a difference quotient; and the errors do fall about fourfold where they are above that round-off
    (measured: quartiles 3.99 ... 4.00 on the six-level net; the softmax net's gradients are so small that almost every
    direction already sits at the round-off)."""
    fam, r64, _, _, _ = tc.family(name)
    x, ei = fam.graphs[g]
    base = r64[g]
    rng = np.random.default_rng([7, mode, g])
    qo = rng.standard_normal(fam.out_dim)
    if fam.softmax:
        qo = np.exp(qo) / np.exp(qo).sum()
    act = fam.out_dim - 1
    want = 0.3 if mode == 0 else 2.5            # the quadratic branch in mode 0, the linear one in mode 1
    gamma, B = 0.9, 3
    r = (base["out"][act] - gamma * qo.max() - want) if mode == 0 else (qo[act] - gamma * base["out"].max() - want)
    args = (mode, act, r, 1.0, gamma, qo, B, weight, np.float64)
    step = ref.learning_step_graph(fam.sd, fam.levels, base, fam.softmax, *args)
    assert abs(float(step["td"]) - want) < 1e-12
    sd = {k: ref._arr(v, np.float64) for k, v in fam.sd.items()}
    f0 = _term(fam, sd, x, ei, base["perm"], args)
    assert f0 == float(step["term"]) and f0 > 0
    h = 1e-4
    ratios, worst = [], 0.0
    for key, grad in step["grads"].items():
        if grad is None:
            continue
        for _ in range(8):
            v = rng.standard_normal(grad.shape)
            v /= np.abs(v).max()
            exact = float((grad * v).sum())

            def quotient(t):
                hi = _term(fam, {**sd, key: sd[key] + t * v}, x, ei, base["perm"], args)
                lo = _term(fam, {**sd, key: sd[key] - t * v}, x, ei, base["perm"], args)
                return (hi - lo) / (2 * t)
            d1, d2 = quotient(h), quotient(h / 2)
            floor = 4 * EPS64 * max(f0, abs(float(r)), 1.0) / (h / 2)     # (the difference is formed at the size of the target)
            e1, e2 = abs(d1 - exact), abs(d2 - exact)
            assert e2 <= abs(d1 - d2) + floor, (key, exact, d1, d2)
            worst = max(worst, e2 / max(abs(exact), 1e-300))
            if e2 > 10 * floor:
                ratios.append(e1 / max(e2, 1e-300))
    med = float(np.median(ratios)) if ratios else float("nan")
    print(f"{name} graph {g} mode {mode} weight {weight}: largest |D(h/2) - g.v| / |g.v| {worst:.2e}, median error ratio per "
          f"halving {med:.2f} over {len(ratios)} directions above the round-off")
    # (a direction whose step crosses a relu breaks the fourfold fall of that one direction, not the bound above: the fall is
    #  asserted on the median, and only where enough directions stand clear of the round-off - the six-level net's do)
    assert len(ratios) < 8 or 3.0 < med < 5.0
    assert name != "T-C" or mode == 1 or len(ratios) >= 8


@pytest.mark.parametrize("select", [True, False])
def test_backward_agrees_with_the_oracle_learning_step(select):
    """`oracle.dqn.compute_gradients` (fp32 torch autograd over oracle/gcn.py) on T-E32's NodeRemovalNet: loss and every
    parameter's gradient inside what the kernels get - 4 x the fp32 yardstick of the parameter, summed over the graphs
    in each graph's own unit."""
    from meshdqn_amd.data import Data
    from oracle import gcn as ora
    from oracle.dqn import compute_gradients
    name = "T-E32"
    fam, r64, _, _, _ = tc.family(name)
    other = tc._network(*tc.SPECS[name][:3], 77, "other")
    yard = tc.yardsticks(name)
    nets = []
    for f in (fam, other):
        o = ora.NodeRemovalNet(**fam.kw)
        o.set_num_nodes(fam.fin0)
        o.load_state_dict(f.sd)
        nets.append(o)
    rng = np.random.default_rng(3)
    data = [Data(x=torch.from_numpy(x), edge_index=torch.from_numpy(ei)) for x, ei in fam.graphs]
    mine = list(range(len(fam.graphs)))
    theirs = [int(rng.integers(0, len(data))) for _ in mine]       # the graphs the other network sees
    terminal = [b % 3 == 1 for b in mine]
    action = [0, fam.out_dim - 1] + [int(rng.integers(0, fam.out_dim)) for _ in mine[2:]]
    reward = [float(v) for v in rng.uniform(-1, 1, len(mine)).astype(np.float32)]
    o64 = [ref.forward_graph(other.sd, other.levels, *fam.graphs[t], other.ratio, True, np.float64)["out"] for t in theirs]
    gamma, B = 0.9, len(mine)
    if select:      # this network evaluates the states, the other one the next states
        trans = [(data[g], action[b], None if terminal[b] else data[theirs[b]], reward[b]) for b, g in enumerate(mine)]
        loss_o, grads_o = compute_gradients(nets[0], nets[1], trans, True, gamma)
    else:           # the other network evaluates the states, this one the next states (with the gradient)
        trans = [(data[theirs[b]], action[b], None if terminal[b] else data[g], reward[b]) for b, g in enumerate(mine)]
        loss_o, grads_o = compute_gradients(nets[1], nets[0], trans, False, gamma)
    steps = [ref.learning_step_graph(fam.sd, fam.levels, r64[g], True, 0 if select else 1, action[b], np.float32(reward[b]),
                                     0.0 if terminal[b] else 1.0, gamma, o64[b], B) for b, g in enumerate(mine)]
    loss = sum(float(s["term"]) for s in steps)
    print(f"oracle learning step, select {select}: loss {loss_o:.6f}, fp64 reference {loss:.6f}")
    assert abs(loss - loss_o) <= tc.MARGIN * max(yard["loss"], float(np.finfo(np.float32).eps) * abs(loss))
    for key, go in grads_o.items():
        if go is None:
            assert all(s["grads"][key] is None for s in steps), key
            continue
        total = sum(s["grads"][key] for s in steps)
        bound = tc.MARGIN * yard["grad"][key] * sum(tc.grad_unit(s["grads"], key) for s in steps)
        dev = float(np.abs(go.numpy().astype(np.float64) - total).max())
        print(f"  {key}: |oracle - fp64| {dev:.2e}, bound {bound:.2e}")
        assert float(np.abs(total).max()) > 0 and dev <= bound, (key, dev, bound)


@pytest.mark.parametrize("name", tc.FAMILIES)
def test_family_input_conditions(name):
    fam, r64, r32, launches, st = tc.family(name)
    share = st["rejected"] / st["candidates"]
    print(f"family {name}: {len(fam.graphs)} graphs of {st['candidates']} candidates, {st['rejected']} rejected ({100 * share:.0f} %): "
          f"{[(s, a, [(w, l) for w, l, _, _ in bad]) for s, a, bad in st['log']]}")
    assert share <= tc.MAX_REJECTED
    # no accepted graph has a decision closer than KINK yardsticks; the rejected ones had
    closest = math.inf
    for g in range(len(fam.graphs)):
        assert tc.kink_violations(r64[g], r32[g], fam.ratio) == []
        assert r32[g]["perm"] == r64[g]["perm"]
        for what, l, dist, yard in tc.kink_margins(r64[g], r32[g], fam.ratio):
            assert dist > tc.KINK * yard, (g, what, l, dist, yard)
            if math.isfinite(dist) and yard > 0:
                closest = min(closest, dist / yard)
        assert max(float(np.abs(s).max()) for s in r32[g]["score"]) < 1.0       # tanh not saturated, in fp32 either
        x, ei = fam.graphs[g]
        assert ei.shape[1] == 0 or (0 <= ei.min() and ei.max() < len(x)), g
    assert all(bad for _, _, bad in st["log"])
    print(f"family {name}: closest decision of an accepted graph {closest:.1f} yardsticks away (rejection below {tc.KINK:.0f})")
    # rejection is deterministic
    tc.family.cache_clear()
    again = tc.family(name)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(again[0].graphs, fam.graphs))
    # every launch is accepted, fits its own graphs and the forms are reached
    for la in launches:
        assert tc.train_accepts(fam, la.nmax, la.emax) is None, (la.idx, la.nmax, la.emax)
        assert all(len(fam.graphs[g][0]) <= la.nmax and fam.graphs[g][1].shape[1] <= la.emax for g in la.idx)
        print(f"family {name}: launch {la.idx} NMAX {la.nmax} EMAX {la.emax} gamma {la.gamma}: {sorted(tc.launch_forms(fam, la))}")
    forms = tc.all_forms(name)
    assert tc.EXPECTED_FORMS[name] <= forms, sorted(tc.EXPECTED_FORMS[name] - forms)
    assert any(la.gamma == 0.0 for la in launches) and any(la.gamma > 0.0 for la in launches)
    # transition data: every Huber branch, terminal / non-terminal, first / last action, every weight class, in both modes
    for mode in (0, 1):
        seen = dict(branch=set(), nf=set(), act=set(), w=set())
        for li, la in enumerate(launches):
            t = tc.transitions(name, mode, li)
            for b, (s64, _) in enumerate(tc.steps(name, mode, True)[li]):
                td = float(s64["td"])
                assert abs(td - t["want"][b]) < 1e-5, (mode, li, b, td)
                seen["branch"].add("mid" if abs(td) < 1 else "hi" if td > 1 else "lo")
                seen["nf"].add(float(t["nonfinal"][b]))
                seen["act"].add(int(t["action"][b]))
                seen["w"].add(float(t["weight"][b]))
        assert seen["branch"] == {"mid", "hi", "lo"} and seen["nf"] == {0.0, 1.0} and seen["w"] == set(tc.WEIGHTS), (mode, seen)
        assert {0, fam.out_dim - 1} <= seen["act"]
    y = tc.yardsticks(name)
    print(f"family {name}: yardsticks out {y['out']:.2e} td {y['td']:.2e} loss {y['loss']:.2e}")
    for k, v in y["grad"].items():
        print(f"family {name}: yardstick {k} {v:.2e}")
        used = any(s64["grads"][k] is not None for s64, _ in tc.steps(name, 0, False)[0])
        assert (0 <= v < 1e-3) if used else v == 0.0, (k, v)      # (0: the weight of an edgeless level, exactly zero gradients)


def test_named_sizes_are_exactly_at_their_limits():
    """The sizes the families are there for: the smallest NMAX the entry point accepts (T-A: 12, T-E32: 41), E256 with
    2 KM C = 10 240 of 10 280 floats, F40 at the wide-input limit - and every refusal case on the refused side of
    exactly the limit it names, its neighbour accepted."""
    fa, fe32, fe256, ff40 = (tc.family(n)[0] for n in ("T-A", "T-E32", "T-E256", "T-F40"))
    assert tc.smallest_accepted_nmax(fa, 1) == 12 and tc.train_accepts(fa, 11, 1) == "backward-head"
    assert tc.smallest_accepted_nmax(fe32, 82) == 41
    assert tc.family("T-A")[3][1].nmax == 12 and tc.family("T-E32")[3][0].nmax == 41
    assert 2 * 20 * 256 == 10240 <= 40 * 257 == 10280 and tc.train_accepts(fe256, 40, 80) is None
    assert tc.train_accepts(fe256, 39, 80) == "backward-rows" and tc.train_accepts(fe256, 41, 80) == "backward-rows"
    assert tc.NACC * (tc.WGT // ff40.C) == 96 and tc.family("T-F40")[3][1].nmax == 96
    for case, (_, nmax, emax, limit, neighbour) in tc.REFUSALS.items():
        net = tc.refusal_network(case)
        assert tc.train_accepts(net, nmax, emax) == limit, case
        if neighbour is not None:
            assert tc.train_accepts(net, neighbour, emax) is None, case
    # the LDS case is past the byte count alone, and by less than one level buffer
    fc = tc.family("T-C")[0]
    assert tc.lds_bytes(fc, 180, 360) > tc.LDS_LIMIT >= tc.lds_bytes(fc, 100, 200)
    wide = tc.refusal_network("300 outputs")
    assert wide.out_dim == 300 and tc.refusal_network("conv width 48").C == 48


def test_tape_layout_restated():
    """Hand count of the workspace of a two-level net: slot 0 (4 floats), per level k C + k + 2 k fin + k + C, the edge
    lists from the second level on, rounded up to whole quads."""
    class Net:
        C, fin0, ratio, levels = 32, 5, 0.5, [0, 1]
    stride, offs = tc.tape_layout(Net, 9, 7)
    l0 = 5 * 32 + 5 + 2 * 5 * 5 + 5 + 32
    l1 = 3 * 32 + 3 + 2 * 3 * 32 + 3 + 32 + 2 * 7
    assert offs[0]["hsel"] == 4 and offs[0]["perm"] == 4 + 5 * 32 + 5 + 50 and offs[0]["esrc"] == -1
    assert offs[1]["hsel"] == 4 + l0 and offs[1]["edst"] == offs[1]["esrc"] + 7
    assert stride == (4 + l0 + l1 + 3) & ~3
