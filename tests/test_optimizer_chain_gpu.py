"""The optimiser chain with every option on - prioritized replay, n-step returns, a target network with Double-DQN targets,
the dueling head, noisy networks - held to ONE fp64 restatement (tests/chain_ref.py, itself held to the per-option
references and to autograd by tests/test_chain_ref_cpu.py):

 (a) the learning step alone, through `FusedGcn.train_step`, with the inputs only the composition produces: `nonfinal` in
     {0, 1, gamma, gamma^2}, importance weights, a `q_other` that is a select row (one value in every column, so its maximum
     is a tie across all lanes), TD errors on both Huber branches and 1e-3 on either side of |td| = 1;
 (b) three consecutive `optimize_device` calls on a hand-written ring (tests/chain_cases.py), every step judged from the
     device's own state in front of it: the draws, the composed minibatch, the draw counters, the priorities and the Polyak
     step exactly; eps, value, TD errors, loss, every tensor of the gradient and Adam's p, m, v against fp32 yardsticks;
 (c) `train_loop_device` with everything on, its three traces replayed through the references.

Sizes of (b): conv width 32, 17 features, minibatches of 8, 32 and 64 nodes (33 and 65 outputs: the learning kernel refuses
24 nodes at this width, 32 is the smallest it accepts).

Bounds: factor x the fp32 yardstick of the quantity, with the floors of the per-part tests (tests/test_gcn_train_paths_gpu.py,
tests/test_dueling_head_gpu.py: one float32 rounding of the operands of the TD error; for the loss the largest of them).  The
yardstick is |chain_ref in fp32 - chain_ref in fp64| per tensor - in (a) the family's (`dueling_ref.yardsticks`) -, Adam is held
by `adam_ref.within`, eps by EPS_TOL of tests/test_noisy_net_gpu.py.  The factor is MARGIN = 4, the per-part one, except where
FACTOR names a quantity that needed more: then it is 4 x the largest ratio measured on the MI355X over the cases of this file.
Every ratio of device deviation to yardstick is printed before it is asserted.  Measured on an MI355X, largest ratio per
quantity (what lies within its floor does not count):
  (a)  td 0.82, gradients 3.50, loss 8.39 (linear, mode 1, weighted; every other loss within its floor or below 1.71)
  (b)  dueling / double, 32 nodes:  value 1.14, td 0.74, loss 1.92, per-graph gradients 4.01 .. 4.26 (one graph, see FACTOR),
                                    flat gradient 1.73 .. 3.46, lin_v 2.62, sigma slice 1.85, Adam p 1.05, m 0.78, v 1.00
       dueling / double, 64 nodes:  value 1.01, td 0.90, loss within its floor, per-graph gradients 0.79 .. 1.33,
                                    flat gradient 1.11 .. 1.93, lin_v 1.00, sigma slice 1.96, Adam p 1.19, m 1.00, v 1.00
       softmax / max, 32 nodes:     td and loss within their floors, per-graph gradients 0.79 .. 2.62, flat gradient
                                    2.19 .. 5.49 (pool weight), sigma slice 1.30, Adam p 1.41, m 0.72, v 1.00
       eps: largest |device - fp64| 1.43e-7 (bound 5.72e-7)

Not covered here: several ranks, and the loop's last optimiser step against chain_ref - `on_every` fires between chunks of
batched steps, never in front of one optimiser step, so (c) leaves the float arithmetic of a step to (b)."""
import numpy as np
import pytest
import torch

import adam_ref
import chain_cases as cc
import chain_ref
import dueling_ref as dref
import gcn_train_cases as tc
import noisy_ref
import nstep_ref
import per_ref
import target_net_ref
from nstep_ref import Nstep
from test_gcn_train_paths_gpu import _run as _launch, _same, _slices
from test_noisy_net_gpu import EPS_TOL, NOISY, _check_sigma_slice, _eps, _eps_deviation
from test_nstep_replay_gpu import B_ENV, BATCH, PER, _cfg, _run

pytestmark = pytest.mark.gpu
EPS32 = dref.EPS32
MARGIN = tc.MARGIN
# quantity -> factor on its fp32 yardstick.  Whatever is not named keeps MARGIN = 4, the factor of the per-part tests; a named
# quantity needed more, and its factor is 4 x the largest ratio measured on the MI355X over the cases of this file (beside it)
FACTOR = {
    "a loss": 33.6,                 # measured 8.39: (a), linear head, mode 1, weighted - a weight of 3.5 on a term of the linear branch
    "graph conv bias": 16.5,        # measured 4.13  } (b), dueling, 32 nodes, third step: the graph with the smallest TD error of the
    "graph conv weight": 16.3,      # measured 4.07  } ring (|td| = 0.015, below 1: every gradient of the graph carries the factor td,
    "graph head": 16.2,             # measured 4.04  } so the TD error's rounding shows in all of them at 1 / |td|, the same relative
    "graph head (lin_v)": 16.0,     # measured 4.01  } deviation of 1.9e-5 in every tensor against yardsticks of 4.4e-6 .. 4.8e-6)
    "graph pool weight": 17.0,      # measured 4.26  }
    "flat pool weight": 22.0,       # measured 5.49: (b), softmax / max, 32 nodes
}


def _factor(what):
    return FACTOR.get(what, MARGIN)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ (a) the learning step with composed inputs
NF = (1.0, cc.GAMMA, 0.0, cc.GAMMA * cc.GAMMA)
NEAR = 1e-3                                       # distance of the near-kink TD errors from |td| = 1: 1000 td yardsticks and more
DIFFS = (0.3, 2.5, -1.7, 1 - NEAR, 1 + NEAR, -(1 - NEAR), -(1 + NEAR))
FAMILY = "T-E32"                                  # the smallest softmax family of gcn_train_cases, and its dueling / linear versions


def _composed_transitions(fam, mode, li):
    """The scheme of `dueling_ref.transitions` with what the composition hands the learning step: `nonfinal` carries
    gamma^(m-1), `q_other` is a select row, and the rewards are picked from the fp64 output so that the TD error lands on
    DIFFS - both Huber branches, and just below and just above |td| = 1 with fractional `nonfinal`."""
    la = fam.launches[li]
    B, OUT = len(la.idx), fam.out_dim
    rng = np.random.default_rng([sum(map(ord, fam.name)), mode, li, 11])
    value = rng.uniform(0.01, 0.2, B) if fam.head == "softmax" else rng.standard_normal(B)
    q_other = np.repeat(value.astype(np.float32)[:, None], OUT, axis=1)
    action, reward, nonfinal, weight, want = [], [], [], [], []
    for b, g in enumerate(la.idx):
        out = fam.r64[g]["out"]
        a = (0, OUT - 1, int(rng.integers(0, OUT)))[(b + li) % 3]
        nf = float(np.float32(NF[(b + li) % 4]))
        d = DIFFS[(b + 3 * mode + 2 * li) % len(DIFFS)]
        v = float(q_other[b, 0])
        r = float(out[a]) - la.gamma * nf * v - d if mode == 0 else v - la.gamma * nf * float(out.max()) - d
        action.append(a), reward.append(r), nonfinal.append(nf), weight.append(tc.WEIGHTS[(b + b // 4) % 4]), want.append(d)
    return dict(action=np.asarray(action, np.int64), reward=np.asarray(reward, np.float32), nonfinal=np.asarray(nonfinal, np.float32),
                weight=np.asarray(weight, np.float32), q_other=q_other, want=np.asarray(want))


_FUSED = {}


def _fused(fam):
    from meshdqn_amd.gcn_fused import FusedGcn
    if fam.head not in _FUSED:
        _FUSED[fam.head] = FusedGcn(fam.net.cuda())
    return _FUSED[fam.head]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("head", dref.HEADS)
def test_learning_step_with_composed_inputs(lib_built, head, mode, weighted):
    fam = dref.family(FAMILY, head)
    fg = _fused(fam)
    yard = dref.yardsticks(fam)
    slices, total = _slices(fam.net)
    worst, bad, seen_nf, seen_d = dict(td=0.0, loss=0.0, grad={}), [], set(), []
    for li, la in enumerate(fam.launches):
        assert tc.train_accepts(fam, la.nmax, la.emax) is None
        t = _composed_transitions(fam, mode, li)
        assert (t["q_other"] == t["q_other"][:, :1]).all()
        runs = [fam.r64[g] for g in la.idx]
        want = chain_ref.learning_step(fam.sd, fam.levels, head, runs, mode, t["action"], t["reward"], t["nonfinal"], la.gamma,
                                       t["q_other"], t["weight"] if weighted else None)
        live = (t["nonfinal"] > 0) | (mode == 0)
        if la.gamma > 0:                # the rewards put the fp64 TD errors where they were wanted
            assert np.allclose(want["td"], t["want"], rtol=0, atol=1e-5), (want["td"], t["want"])
            seen_d += [d for d, ok in zip(t["want"], live) if ok]
            seen_nf |= set(t["nonfinal"].tolist())
        res = _launch(fg, [fam.graphs[g] for g in la.idx], la.nmax, la.emax, mode, t, la.gamma, "weighted" if weighted else "td")
        tdfloor = 0.0
        for b, g in enumerate(la.idx):
            s64 = want["steps"][b]
            a = int(t["action"][b])
            q = float(fam.r64[g]["out"][a]) if mode == 0 else float(t["q_other"][b, a])
            floor = EPS32 * max(abs(q), abs(q - float(s64["td"])))
            tdfloor = max(tdfloor, floor)
            d_td = abs(float(res["td"][b]) - float(s64["td"]))
            if d_td > floor:
                worst["td"] = max(worst["td"], d_td)
            if d_td > max(_factor("a td") * yard["td"], floor):
                bad.append(f"launch {li} graph {g} td: {d_td:.3e}, yardstick {yard['td']:.3e}, floor {floor:.3e}")
            for key, (lo, hi, shape) in slices.items():
                got, ref_g = res["partial"][b, lo:hi].reshape(shape), s64["grads"][key]
                if ref_g is None or not np.any(ref_g):
                    assert not np.any(got), f"launch {li} graph {g} {key}: reference exactly zero, device {np.abs(got).max():.3e}"
                    continue
                d = tc.grad_dev(got, s64["grads"], key)
                if d >= worst["grad"].get(key, (0.0, None))[0]:
                    worst["grad"][key] = (d, (li, g))
                if d > _factor("a grad") * yard["grad"][key]:
                    bad.append(f"launch {li} graph {g} {key}: {d:.3e} of its unit, yardstick {yard['grad'][key]:.3e} "
                               f"(ratio {d / yard['grad'][key]:.2f}, bound {_factor('a grad')})")
        d_loss = abs(float(res["loss"]) - float(want["loss"]))
        if d_loss > tdfloor:
            worst["loss"] = max(worst["loss"], d_loss)
        if d_loss > max(_factor("a loss") * yard["loss"], tdfloor):
            bad.append(f"launch {li} loss: {d_loss:.3e}, yardstick {yard['loss']:.3e}, floor {tdfloor:.3e} "
                       f"(ratio {d_loss / yard['loss']:.2f}, bound {_factor('a loss')})")
    assert seen_nf == {float(np.float32(v)) for v in NF}
    assert any(abs(d) < 1 - 2 * NEAR for d in seen_d) and any(abs(d) > 1 + 2 * NEAR for d in seen_d)
    assert any(1 - 2 * NEAR < abs(d) < 1 for d in seen_d) and any(1 < abs(d) < 1 + 2 * NEAR for d in seen_d)
    tag = f"(a) {head} mode {mode} weighted {weighted}"
    for k in ("td", "loss"):
        print(f"{tag} {k}: yardstick {yard[k]:.3e}, device beyond its floor {worst[k]:.3e}, ratio {worst[k] / yard[k]:.2f} "
              f"(bound {_factor('a ' + k)})")
    for key, (d, where) in sorted(worst["grad"].items()):
        print(f"{tag} {key}: worst (launch, graph) {where}: yardstick {yard['grad'][key]:.3e}, device {d:.3e}, "
              f"ratio {d / yard['grad'][key]:.2f} (bound {_factor('a grad')})")
    assert {"lin1.weight", "lin3.weight", "conv1.lin_l.weight"} <= set(worst["grad"])
    assert not bad, f"{tag}: beyond the bounds:\n" + "\n".join(bad)


# ------------------------------------------------------------------ (b) three optimize_device calls with every option on
def _state(tr):
    """What the device holds in front of a step, read back."""
    a = tr._adam[0]
    opt = tr.opts[0]
    g = opt.param_groups[0]
    rep = tr.device_memory
    return dict(sd1=chain_ref.host_sd(tr.policy_net_1), sd2=chain_ref.host_sd(tr.policy_net_2), m=a["m"].cpu().numpy(),
                v=a["v"].cpu().numpy(), step=int(opt.state[a["params"][0]]["step"]), draws=dict(tr.noise_draws),
                hp=dict(lr=float(g["lr"]), wd=float(g["weight_decay"]), beta1=g["betas"][0], beta2=g["betas"][1], eps=float(g["eps"])),
                prio=rep.prio.cpu().numpy(), pmax=np.float32(rep.pmax.item()), num_grads=tr.num_grads)


def _ratio(report, what, dev, yard, floor=0.0):
    """Hold a deviation to its factor x the yardstick or to the floor of its float32 roundings, and record deviation /
    yardstick of everything beyond that floor.  A yardstick is taken to be one float32 epsilon at least (the convention of
    `adam_ref.yardstick`: the fp32 restatement of a single minibatch can hit the fp64 value of a short sum exactly, which
    the device's float32 result need not)."""
    if what.startswith(("graph ", "flat ")):        # (in units of the tensor's largest entry; td, loss and value are absolute)
        yard = max(yard, EPS32)
    r = dev / yard if yard > 0 else (0.0 if dev == 0 else float("inf"))
    if dev > floor:
        report["ratio"][what] = max(report["ratio"].get(what, 0.0), r)
    if dev > max(_factor(what) * yard, floor):
        report["bad"].append(f"{what}: device {dev:.3e}, yardstick {yard:.3e}, floor {floor:.3e} (ratio {r:.2f}, bound {_factor(what)})")


def _tensor_devs(got, want64, want32, keys):
    """Per tensor (deviation of `got`, deviation of the fp32 restatement) from the fp64 one, in `grad_unit`s."""
    out = {}
    for k in keys:
        if not np.any(want64[k]):
            assert not np.any(got[k]), f"{k}: reference exactly zero, device {np.abs(got[k]).max():.3e}"
            continue
        unit = tc.grad_unit(want64, k)
        out[k] = (float(np.abs(got[k].astype(np.float64) - want64[k]).max()) / unit,
                  float(np.abs(want32[k].astype(np.float64) - want64[k]).max()) / unit)
    return out


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: "-".join(map(str, c)))
def test_three_steps_with_every_option_on(lib_built, case):
    from meshdqn_amd.replay import SharedDeviceReplay
    head, kind, wanted = case
    hc = cc.host_case(*case)
    n, arch, R = hc["n"], hc["arch"], hc["R"]
    EM, nf = 2 * n, n * cc.F
    print(f"(b) {case}: {n} nodes, {n + 1} outputs" + (f" (the learning kernel refuses {wanted}: {hc['refused']})" if n != wanted else ""))
    assert tc.train_accepts(cc._shape(n), n, EM) is None
    tr = cc.trainer(head, kind, n)
    dev = tr.ctx.device
    assert chain_ref.arch_of(tr.policy_net_1) == arch
    for net, sd in ((tr.policy_net_1, hc["sd1"]), (tr.policy_net_2, hc["sd2"])):      # the parameters the CPU test looked at
        assert all(np.array_equal(_bits(v), _bits(sd[k])) for k, v in chain_ref.host_sd(net).items())
    offs, total = chain_ref.offsets(arch)
    mask = chain_ref.trained_mask(arch)
    means = [k for k, _, _ in arch["params"] if k != "noisy_sigma"]
    mean_total = offs["noisy_sigma"][0]
    rep = tr.device_memory = SharedDeviceReplay.grouped(None, cc.CAP, cc.W, n, cc.F, EM, dev)
    rep.R.copy_(_dev(R))
    rep.close(cc.HEAD_STEP)
    prio0, pmax0 = cc.priorities()
    rep._prio().copy_(_dev(prio0))
    rep.pmax.fill_(float(pmax0))
    rep.prio_fill(cc.HEAD_STEP)
    tr._adam_state(0, total)
    i32, f32 = torch.int32, torch.float32
    idx_d, w_d, td_d = torch.zeros(cc.BATCH, dtype=i32, device=dev), torch.zeros(cc.BATCH, device=dev), torch.zeros(cc.BATCH, device=dev)
    steps_d, sel_d, val_d = torch.zeros(cc.BATCH, dtype=i32, device=dev), torch.zeros(cc.BATCH, dtype=i32, device=dev), torch.zeros(cc.BATCH, device=dev)
    loss_d = torch.zeros(1, dtype=f32, device=dev)
    double = kind == "double"
    report = dict(ratio={}, bad=[])
    f1, f2 = tr._fused_of(tr.policy_net_1, "train"), tr._fused_of(tr.policy_net_2, "train")
    polyak_steps, branches = 0, set()
    for k in range(cc.STEPS):
        st = _state(tr)
        if k == 0:
            assert np.array_equal(_bits(st["prio"]), _bits(cc.filled())) and st["pmax"] == pmax0 and st["step"] == 0
            u = cc.uniforms()[0]
        else:
            try:
                u = cc.aim(st["prio"], cc.WANTED)               # the edge cases again, where the new priorities allow it
            except ValueError:
                u = cc.uniforms()[k]
        beta = tr.beta()
        rep.prio_draw(_dev(u), beta, idx_d, w_d)
        kw = dict(sel_out=sel_d, value_out=val_d) if double else {}
        tr.optimize_device(rep, idx_d, loss_out=loss_d, weight=w_d, td_out=td_d, head_step=cc.HEAD_STEP, steps_out=steps_d, **kw)
        torch.cuda.synchronize()
        idx, w, td, steps = idx_d.cpu().numpy(), w_d.cpu().numpy(), td_d.cpu().numpy(), steps_d.cpu().numpy()
        bufs = next(iter(f1._train_bufs.values()))
        flat, partial, terms = bufs["grad"].cpu().numpy(), bufs["partial"].cpu().numpy(), bufs["ws"][:, 0].cpu().numpy()
        mbd = {key: v.cpu().numpy() for key, v in tr._mb_bufs.items() if torch.is_tensor(v)}
        eps1, eps2 = _eps(f1), _eps(f2)
        rep.prio_update(idx_d, td_d, cc.PER["alpha"], cc.PER["eps"])
        torch.cuda.synchronize()
        after = _state(tr)
        tag = f"(b) {case} step {k}"
        # ---- the draw: bracketed by the reference's prefix sums, weights within one ulp
        S = per_ref.prefix(st["prio"])
        tol = cc.CAP * 2.0 ** -52 * S[-1]
        tt = per_ref.targets(S[-1], u)
        assert (st["prio"][idx] > 0).all() and (idx < cc.HEAD_STEP * cc.W).all(), tag
        assert (np.concatenate([[0.0], S])[idx] - tol <= tt).all() and (tt <= S[idx] + tol).all(), (tag, idx)
        ridx, rw, _ = per_ref.draw(st["prio"], u, beta)
        assert np.array_equal(idx, ridx), (tag, idx, ridx)        # (no target of these draws sits within `tol` of a boundary)
        assert per_ref.ulp_diff32(w, rw).max() <= 1, tag
        if k == 0:
            assert tuple(idx) == cc.WANTED and len(set(w.tolist())) > 3
        # ---- the restatement of this step, from the state the device held in front of it
        seed = tr.noisy["seed"]
        o64, o32, mg = chain_ref.chain_pair(
            R, n, cc.F, EM, cc.W, idx, cc.HEAD_STEP, cc.N_STEP, cc.GAMMA, arch,
            dict(sd=st["sd1"], draw=(seed, 1, st["draws"]["train1"])), dict(sd=st["sd2"], draw=(seed, 2, st["draws"]["train2"])),
            target_net=kind, weight=w, adam=dict(m=st["m"], v=st["v"], hp=st["hp"], step=st["step"] + 1), num_grads=st["num_grads"],
            period=cc.PERIOD, tau=cc.TAU)
        mb, keep = o64["mb"], o64["keep"]
        left_out = [b for b in range(cc.BATCH) if b not in keep]
        for b in left_out:
            print(f"{tag}: graph {b} (record {idx[b]}) left out: {mg[b]}")
        assert len(left_out) <= 1, f"{tag}: {len(left_out)} graphs sit on a kink: {[mg[b] for b in left_out]}"
        # ---- exact: the composed minibatch, the counters
        assert np.array_equal(steps, mb["steps"]), tag
        for key in ("reward", "nonfinal", "action", "edge_ptr_s", "edge_ptr_n"):
            assert np.array_equal(_bits(mbd[key]), _bits(mb[key])), (tag, key)
        for g in ("s", "n"):
            assert np.array_equal(_bits(mbd["x_" + g].reshape(cc.BATCH, nf)), _bits(mb["x_" + g])), (tag, g)
            ne = mb["edge_ptr_" + g][-1]
            assert np.array_equal(mbd["esrc_" + g][:ne], mb["esrc_" + g]) and np.array_equal(mbd["edst_" + g][:ne], mb["edst_" + g]), (tag, g)
        assert after["draws"] == dict(act1=0, train1=st["draws"]["train1"] + 1, train2=st["draws"]["train2"] + 1) and st["draws"]["train1"] == k
        assert after["num_grads"] == k + 1 and after["step"] == k + 1
        # ---- exact: the priorities after the update from the device's TD errors
        want_prio = st["prio"].copy()
        want_pmax = per_ref.update(want_prio, st["pmax"], idx, td, cc.PER["alpha"], cc.PER["eps"])
        assert np.array_equal(_bits(after["prio"]), _bits(want_prio)), (tag, per_ref.ulp_diff32(after["prio"], want_prio).max())
        assert np.float32(after["pmax"]) == np.float32(want_pmax), tag
        # ---- the noise of both copies
        d_eps = max(_eps_deviation(f1, eps1, 1, st["draws"]["train1"], seed=seed), _eps_deviation(f2, eps2, 2, st["draws"]["train2"], seed=seed))
        print(f"{tag} eps: largest |device eps - fp64 eps| {d_eps:.3e} (bound {EPS_TOL:.3e})")
        assert d_eps <= EPS_TOL, tag
        # ---- the Double-DQN choice and its value
        if double:
            sel, val = sel_d.cpu().numpy(), val_d.cpu().numpy()
            sure = [b for b in range(cc.BATCH) if not any(m[0] == "online" for m in mg[b])]
            assert len(sure) >= cc.BATCH - 1 and np.array_equal(sel[sure], o64["sel"][sure]), (tag, sel, o64["sel"])
            _ratio(report, "value", float(np.abs(val[keep] - o64["value"][keep]).max()),
                   float(np.abs(o32["value"][keep].astype(np.float64) - o64["value"][keep]).max()), EPS32 * float(np.abs(o64["value"][keep]).max()))
        # ---- TD errors, loss
        tdfloor, y_td = 0.0, float(np.abs(o32["td"][keep].astype(np.float64) - o64["td"][keep]).max())
        for b in keep:
            q = float(o64["runs_trained"][b]["out"][int(mb["action"][b])])
            floor = EPS32 * max(abs(q), abs(q - float(o64["td"][b])))
            tdfloor = max(tdfloor, floor)
            _ratio(report, "td", abs(float(td[b]) - float(o64["td"][b])), y_td, floor)
        s = np.float32(0)
        for b in keep:
            s = s + terms[b]
        loss_dev = float(loss_d.item()) if not left_out else float(s / np.float32(cc.BATCH))
        l64, l32 = chain_ref.reduce_loss(o64["steps"], keep), chain_ref.reduce_loss(o32["steps"], keep, np.float32)
        _ratio(report, "loss", abs(loss_dev - float(l64)), abs(float(l32) - float(l64)), tdfloor)
        branches |= {bool(abs(o64["td"][b]) > 1) for b in keep}
        # ---- the gradient of every graph, parameter by parameter
        yard = {}
        for b in keep:
            for key in means:
                g64 = o64["steps"][b]["grads"][key]
                if g64 is not None and np.any(g64):
                    yard[key] = max(yard.get(key, 0.0), tc.grad_dev(o32["steps"][b]["grads"][key], o64["steps"][b]["grads"], key))
        for b in keep:
            assert not np.any(partial[b, mean_total:]), tag                  # (the sigmas' slice belongs to mdq_noisy_grad)
            for key in means:
                lo, hi, shape = offs[key]
                got, g64 = partial[b, lo:hi].reshape(shape), o64["steps"][b]["grads"][key]
                if g64 is None or not np.any(g64):
                    assert not np.any(got), f"{tag} graph {b} {key}: reference exactly zero, device {np.abs(got).max():.3e}"
                    continue
                _ratio(report, "graph " + tc.param_class(key) + (" (lin_v)" if key.startswith("lin_v") else ""),
                       tc.grad_dev(got, o64["steps"][b]["grads"], key), yard[key])
        # ---- the flat gradient over the graphs that stay, tensor by tensor, the sigmas' slice included
        fsum = np.zeros(total, np.float32)
        for b in keep:
            fsum = fsum + partial[b]
        if not left_out:
            assert _same(flat[:mean_total], fsum[:mean_total]), tag
        assert _check_sigma_slice(f1, eps1, flat, tag)                       # the device's slice is the product of ITS means' slice and eps
        got = {key: fsum[offs[key][0]:offs[key][1]].reshape(offs[key][2]) for key in means}
        if left_out:                                                         # the slice the same product gives for the graphs that stay
            sig = np.zeros(total - mean_total, np.float32)
            for name, o, i, off_w, off_b in arch["noisy"]:
                gw, gb = noisy_ref.sigma_grad32(got[name + ".weight"], got[name + ".bias"], *eps1[name])
                sig[off_w:off_w + o * i], sig[off_b:off_b + o] = gw.reshape(-1), gb
            got["noisy_sigma"] = sig
        else:
            got["noisy_sigma"] = flat[mean_total:]
        g64, _ = chain_ref.reduce_grad(o64["steps"], keep, arch, o64["eps1"], np.float64)
        g32, _ = chain_ref.reduce_grad(o32["steps"], keep, arch, o32["eps1"], np.float32)
        devs = _tensor_devs(got, g64, g32, means + ["noisy_sigma"])
        assert {"noisy_sigma", "lin1.weight", "lin3.bias", "conv1.lin_r.weight", "pool5.weight"} <= set(devs), tag
        assert head != "dueling" or {"lin_v.weight", "lin_v.bias"} <= set(devs), tag
        for key, (d, y) in devs.items():
            what = "sigma slice" if key == "noisy_sigma" else "lin_v" if key.startswith("lin_v") else tc.param_class(key)
            _ratio(report, "flat " + what, d, y)
        # ---- Adam, judged alone: from the device's own flat gradient
        p0 = chain_ref.flat_of(st["sd1"], arch)
        hp = dict(st["hp"], step=st["step"] + 1)
        a64 = chain_ref.adam_apply(p0, st["m"], st["v"], flat, hp, mask, np.float64)
        a32 = chain_ref.adam_apply(p0, st["m"], st["v"], flat, hp, mask, np.float32)
        got_pmv = (chain_ref.flat_of(after["sd1"], arch), after["m"], after["v"])
        for key, (lo, hi, _) in offs.items():
            if not mask[lo]:                                                 # conv3 / pool3 / conv6 / pool6: never trained
                assert _same(got_pmv[0][lo:hi], p0[lo:hi]) and not np.any(got_pmv[1][lo:hi]) and not np.any(got_pmv[2][lo:hi]), (tag, key)
                continue
            for kind_, j in (("p", 0), ("m", 1), ("v", 2)):
                before = p0[lo:hi] if kind_ == "p" else None
                d = adam_ref.deviation(kind_, got_pmv[j][lo:hi], a64[j][lo:hi], before)
                d32 = adam_ref.deviation(kind_, a32[j][lo:hi], a64[j][lo:hi], before)
                report["ratio"]["adam " + kind_] = max(report["ratio"].get("adam " + kind_, 0.0), d / adam_ref.yardstick(d32))
                if not adam_ref.within(d, d32):
                    report["bad"].append(f"{tag} adam {kind_} {key}: {d:.3e}, fp32 restatement {d32:.3e} (bound {adam_ref.MARGIN} x)")
        assert not _same(got_pmv[0][mean_total:], p0[mean_total:]) and not _same(got_pmv[0][:mean_total], p0[:mean_total]), tag
        # ---- the target: the Polyak step where one is due, untouched otherwise
        t_before, t_after, online = chain_ref.flat_of(st["sd2"], arch), chain_ref.flat_of(after["sd2"], arch), got_pmv[0]
        if (k + 1) % cc.PERIOD == 0:
            polyak_steps += 1
            assert np.array_equal(_bits(t_after), _bits(target_net_ref.polyak(t_before, online, cc.TAU))), tag
            assert not _same(t_after, t_before) and not _same(t_after[mean_total:], t_before[mean_total:])
            assert o64["target_after"] is not None
        else:
            assert _same(t_after, t_before) and o64["target_after"] is None, tag
    assert polyak_steps == 1 and branches == {False, True}                   # both Huber branches occurred
    for what, r in sorted(report["ratio"].items()):
        print(f"(b) {case} {what}: largest device deviation / yardstick over {cc.STEPS} steps {r:.2f}")
    assert not report["bad"], f"(b) {case}: beyond the bounds:\n" + "\n".join(report["bad"])


# ------------------------------------------------------------------ (c) the loop with everything on, replayed
STEPS_C = 10                                       # 8 minibatches: the run ends on a multiple of the target's period
PERIOD_C = 4
M_LOOP = STEPS_C - (-(-BATCH // B_ENV))


@pytest.fixture(scope="module")
def loop_run(lib_built):
    from meshdqn_amd.env import Env2DAirfoil
    return _run(Env2DAirfoil(_cfg()), steps=STEPS_C, loop_kw=dict(target_trace=True), prioritized=PER, n_step=3,
                target_net=dict(kind="double", period=PERIOD_C, tau=1.0), head="dueling", noisy=NOISY)


def test_loop_replays_its_prioritized_trace_in_full(loop_run):
    """Fills by `ring_ranges`, draws from the traced u and beta (bracket bound of the generic draw test, weights within one
    ulp), updates from the traced TD errors: the final priority table and pmax bit for bit."""
    out, tr = loop_run
    per, rep = out["per"], tr.device_memory
    cap, G, t_first = rep.capacity, rep.G, -(-BATCH // B_ENV)
    assert rep.W == B_ENV and rep.steps_pushed == STEPS_C < G and len(out["losses"]) == M_LOOP == 8
    assert per["idx"].shape == per["u"].shape == per["weight"].shape == per["td"].shape == (M_LOOP, BATCH)
    assert np.array_equal(per["beta"], [min(1.0, PER["beta0"] + (1.0 - PER["beta0"]) * g / PER["beta_steps"]) for g in range(M_LOOP)])
    assert np.isfinite(per["td"]).all() and np.isfinite(out["losses"]).all()
    prio, pmax = np.zeros(cap, np.float32), np.float32(1.0)
    for t in range(STEPS_C):
        per_ref.fill(prio, pmax, *per_ref.ring_ranges(t, G, B_ENV))
        assert np.array_equal(prio > 0, np.arange(cap) < t * B_ENV), t
        if t < t_first:
            continue
        m = t - t_first
        idx = per["idx"][m]
        S = per_ref.prefix(prio)
        tol = cap * 2.0 ** -52 * S[-1]
        tt = per_ref.targets(S[-1], per["u"][m])
        assert (prio[idx] > 0).all(), m
        assert (np.concatenate([[0.0], S])[idx] - tol <= tt).all() and (tt <= S[idx] + tol).all(), (m, idx)
        wr = np.array([np.float32((float(prio[idx].min()) / float(prio[j])) ** per["beta"][m]) for j in idx])
        assert per_ref.ulp_diff32(per["weight"][m], wr).max() <= 1, m
        pmax = per_ref.update(prio, pmax, idx, per["td"][m], PER["alpha"], PER["eps"])
    per_ref.fill(prio, pmax, *per_ref.ring_ranges(STEPS_C, G, B_ENV, zero=False))
    got = rep.prio.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(prio)), per_ref.ulp_diff32(got, prio).max()
    assert np.float32(rep.pmax.item()) == np.float32(pmax)
    assert len(np.unique(got[:STEPS_C * B_ENV])) > 8 and not (per["weight"] == 1.0).all()


def test_loop_replays_its_n_step_and_target_traces(loop_run):
    """`reward`, `nonfinal` and `steps` of every minibatch against tests/nstep_ref.py on the final ring (`_replay_trace` of
    tests/test_nstep_replay_gpu.py for this run's length); the walks start from the prioritized draws; the choices are
    actions and their values finite."""
    out, tr = loop_run
    rep, tn, tt = tr.device_memory, out["nstep"], out["target"]
    R = rep.R.cpu().numpy()
    nf, EM, t_first = rep.N * rep.F, rep.e_max, -(-BATCH // B_ENV)
    assert np.array_equal(out["per"]["idx"], tn["idx"])
    for key in ("idx", "reward", "nonfinal", "steps"):
        assert tn[key].shape == (M_LOOP, BATCH), key
    terminal = np.zeros((M_LOOP, BATCH), bool)
    for m in range(M_LOOP):
        t = t_first + m
        assert tn["head"][m] == rep.group_base(t) == t * B_ENV
        ns = Nstep(3, rep.W, rep.capacity, int(tn["head"][m]), tr.gamma)
        idx = tn["idx"][m]
        assert ((0 <= idx) & (idx < tn["head"][m])).all()
        assert np.array_equal(tn["steps"][m], nstep_ref.steps(R, nf, EM, ns, idx)), m
        assert np.array_equal(_bits(tn["reward"][m]), _bits(nstep_ref.reward(R, nf, EM, ns, idx))), m
        assert np.array_equal(_bits(tn["nonfinal"][m]), _bits(nstep_ref.nonfinal(R, nf, EM, ns, idx))), m
        terminal[m] = [R[nstep_ref.walk(R, nf, EM, ns, j)[-1], -1] > 0.5 for j in idx]
    assert tn["steps"].max() == 3 and (tn["nonfinal"][terminal] == 0).all() and (tn["nonfinal"][~terminal] > 0).all()
    assert tt["sel"].shape == tt["value"].shape == (M_LOOP, BATCH) and tt["sel"].dtype == np.int32
    assert ((0 <= tt["sel"]) & (tt["sel"] < tr.n_actions + 1)).all() and np.isfinite(tt["value"]).all()


def test_loop_ends_with_its_counters_and_its_target_in_place(loop_run):
    """The draw counters count batched steps and minibatches; with tau = 1 and a run of 8 = 2 x 4 gradient steps the target
    is the online network (`on_every` fires between chunks only: no snapshot in front of a single optimiser step)."""
    from test_nstep_replay_gpu import _trainer
    out, tr = loop_run
    assert tr.noise_draws == dict(act1=STEPS_C, train1=M_LOOP, train2=M_LOOP)
    assert tr.num_grads == M_LOOP and M_LOOP % PERIOD_C == 0 and tr.select is True and len(tr.opts[1].state) == 0
    init = _trainer(target_net=dict(kind="double", period=PERIOD_C, tau=1.0), head="dueling", noisy=NOISY)
    names = [k for k, _ in tr.policy_net_1.named_parameters()]
    assert names[-1] == "noisy_sigma" and "lin_v.weight" in names
    for (k, p), q, p0 in zip(tr.policy_net_1.named_parameters(), tr.policy_net_2.parameters(), init.policy_net_1.parameters()):
        assert torch.equal(p, q), k
        assert torch.isfinite(p).all(), k
    for k in ("noisy_sigma", "lin_v.weight", "lin1.weight", "conv1.lin_l.weight"):
        assert not torch.equal(dict(tr.policy_net_1.named_parameters())[k], dict(init.policy_net_1.named_parameters())[k]), k
