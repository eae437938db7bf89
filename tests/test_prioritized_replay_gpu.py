"""GPU: proportional prioritized replay - the three ring kernels (mdq_replay_prio_fill / _draw / _update) against their numpy
restatement (tests/per_ref.py), the learning step with per-sample weights and TD errors (mdq_gcn_train_step_weighted) against
the unweighted one and torch autograd, and `train_loop_device` with a prioritized trainer against a replay of its own trace."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import per_ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
U_LAST = 1.0 - 2.0 ** -53          # the largest double below 1


# ------------------------------------------------------------------ the kernels, called through the C ABI
def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _draw(prio, u, beta):
    """One `mdq_replay_prio_draw` launch -> idx, weight, total (numpy)."""
    from meshdqn_amd import _lib
    n = len(u)
    p_d, u_d = _dev(prio, np.float32), _dev(u, np.float64)
    idx = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    w = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    tot = torch.full((1,), -7.0, dtype=torch.float64, device="cuda")
    d = _lib.ReplayPrioDrawDesc(capacity=len(prio), n=n, beta=beta, prio=p_d.data_ptr(), u=u_d.data_ptr(), idx=idx.data_ptr(),
                                weight=w.data_ptr(), total=tot.data_ptr())
    _lib.check(_lib.load().mdq_replay_prio_draw(C.byref(d), None), "mdq_replay_prio_draw")
    torch.cuda.synchronize()
    return idx.cpu().numpy(), w.cpu().numpy(), float(tot.item())


def _dyadic(rng, cap):
    """Priorities k / 1024, 0 < k < 1024: every fp64 sum of them is exact in any order, so the kernel's prefix sums ARE the
    reference's and the drawn records must be the same ones."""
    return rng.integers(1, 1024, cap).astype(np.float32) / np.float32(1024)


def _scenarios(rng, cap):
    """Priority tables of one capacity: full, zero windows at the start / in the middle / wrapping the end, all mass in the
    first / the last record, nothing at all."""
    out = dict(full=_dyadic(rng, cap))
    k = max(1, cap // 3)
    for name, zero in (("zero_start", range(0, k)), ("zero_middle", range(cap // 2 - k // 2, cap // 2 - k // 2 + k)),
                       ("zero_wrap", [j % cap for j in range(cap - k // 2 - 1, cap + k // 2)])):
        p = _dyadic(rng, cap)
        if k < cap:
            p[list(zero)] = 0
        out[name] = p
    for name, j in (("first_only", 0), ("last_only", cap - 1)):
        p = np.zeros(cap, np.float32)
        p[j] = 0.625
        out[name] = p
    out["nothing"] = np.zeros(cap, np.float32)
    return out


@pytest.mark.parametrize("cap", [1, 5, 1023, 1024, 1025, 2049, 10000])
def test_draw_equals_the_reference_on_exact_sums(lib_built, cap):
    """Dyadic priorities: idx and total bit for bit, the weights within one float ulp (one fp64 pow on each side, rounded
    once); 1 .. 1024 draws (more draws than records at capacity 5), both extreme u; a second launch is bitwise the first."""
    rng = np.random.default_rng(100 + cap)
    for name, prio in _scenarios(rng, cap).items():
        for n in (1, 8, 32, 1024):
            for kind in ("random", "zero", "last"):
                if kind != "random" and name not in ("full", "zero_wrap", "last_only"):
                    continue
                u = dict(random=rng.random(n), zero=np.zeros(n), last=np.full(n, U_LAST))[kind]
                beta = float(rng.choice([0.0, 0.4, 0.7, 1.0]))
                idx, w, total = _draw(prio, u, beta)
                ridx, rw, rtotal = per_ref.draw(prio, u, beta)
                tag = (cap, name, n, kind, beta)
                assert total == rtotal, tag
                assert np.array_equal(idx, ridx), (tag, np.flatnonzero(idx != ridx)[:5])
                assert per_ref.ulp_diff32(w, rw).max() <= 1, tag
                if rtotal > 0:
                    assert (prio[idx] > 0).all() and w.max() == 1.0, tag
                else:
                    assert (idx == 0).all() and (w == 0).all(), tag
                if n == 32:
                    idx2, w2, total2 = _draw(prio, u, beta)
                    assert np.array_equal(idx, idx2) and np.array_equal(w.view(np.int32), w2.view(np.int32)) and total == total2


@pytest.mark.parametrize("cap,n", [(2049, 32), (10000, 1024), (777, 1024)])
def test_draw_on_generic_priorities_is_bracketed_by_the_reference(lib_built, cap, n):
    """Random fp32 priorities over six decades: every drawn record has a priority, and the reference's exclusive and
    inclusive prefix sums at the drawn record bracket the target t_i within capacity * 2^-52 * total - the error bound of two
    fp64 sums of `capacity` non-negative terms (the kernel's, in its own order, and numpy's)."""
    rng = np.random.default_rng(cap + n)
    prio = (10.0 ** rng.uniform(-4, 2, cap)).astype(np.float32)
    prio[rng.random(cap) < 0.3] = 0
    prio[cap // 2:cap // 2 + cap // 10] = 0
    u = rng.random(n)
    idx, w, total = _draw(prio, u, 0.5)
    S = per_ref.prefix(prio)
    tol = cap * 2.0 ** -52 * S[-1]
    assert abs(total - S[-1]) <= tol
    assert (prio[idx] > 0).all()
    t = per_ref.targets(S[-1], u)
    excl = np.concatenate([[0.0], S])[idx]
    assert (excl - tol <= t).all() and (t <= S[idx] + tol).all()
    assert (np.diff(idx) >= 0).all()
    wr = np.array([np.float32((float(prio[idx].min()) / float(prio[j])) ** 0.5) for j in idx])
    assert per_ref.ulp_diff32(w, wr).max() <= 1
    idx2, w2, total2 = _draw(prio, u, 0.5)
    assert np.array_equal(idx, idx2) and np.array_equal(w.view(np.int32), w2.view(np.int32)) and total == total2


GUARD = 64


def _guarded(prio):
    """The priority array between two guard bands of a sentinel: (whole buffer, the view the kernels get)."""
    buf = torch.full((len(prio) + 2 * GUARD,), -3.0, dtype=torch.float32, device="cuda")
    buf[GUARD:GUARD + len(prio)] = _dev(prio, np.float32)
    return buf, buf[GUARD:GUARD + len(prio)]


def _guards_intact(buf):
    return bool((buf[:GUARD] == -3.0).all()) and bool((buf[-GUARD:] == -3.0).all())


def test_update_equals_the_reference(lib_built):
    """Duplicates with different TD errors (the last one stays), TD errors that are not finite (record untouched, not part of
    pmax), record numbers outside the array (skipped: the array and the guard bands around it are unchanged), 1 .. 1024 draws."""
    from meshdqn_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(8)
    for cap, n, alpha, eps in ((40, 8, 0.6, 1e-6), (40, 32, 1.0, 1e-3), (10000, 1024, 0.6, 1e-6), (7, 1024, 0.0, 1e-6), (1, 1, 0.5, 0.25),
                               (300, 70, 0.3, 1e-6)):
        prio = rng.random(cap).astype(np.float32)
        idx = rng.integers(0, cap, n).astype(np.int32)                 # (n > capacity / birthday: plenty of duplicates)
        td = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(np.float32)
        if n >= 8:
            td[[1, 5]] = [np.nan, -np.inf]
            idx[2], idx[6] = -1, cap                                   # just outside, on either side
            idx[3], idx[7] = -2 ** 31, 2 ** 31 - 1
            idx[n - 1] = idx[0]                                        # a duplicate for sure, with another TD error
            td[n - 1] = td[0] * 3 + 1
        if n >= 32:
            idx[20], td[20], td[21], idx[21] = idx[9], np.nan, 0.5, idx[10]   # a later NaN draw of a record keeps the earlier value
        for pmax0 in (1.0, 1e9):
            buf, view = _guarded(prio)
            pm = torch.full((1,), pmax0, dtype=torch.float32, device="cuda")
            idx_d, td_d = _dev(idx, np.int32), _dev(td, np.float32)
            _lib.check(lib.mdq_replay_prio_update(view.data_ptr(), cap, n, idx_d.data_ptr(), td_d.data_ptr(), alpha, eps,
                                                  pm.data_ptr(), None), "mdq_replay_prio_update")
            torch.cuda.synchronize()
            want = prio.copy()
            want_pm = per_ref.update(want, pmax0, idx, td, alpha, eps)
            got = view.cpu().numpy()
            assert _guards_intact(buf), (cap, n)
            touched = np.zeros(cap, bool)
            ok = np.isfinite(td) & (idx >= 0) & (idx < cap)
            touched[idx[ok]] = True
            assert np.array_equal(got[~touched], prio[~touched]), (cap, n)
            assert per_ref.ulp_diff32(got[touched], want[touched]).max(initial=0) <= 1, (cap, n)
            assert per_ref.ulp_diff32(pm.cpu().numpy(), np.float32(want_pm)).max() <= 1 and float(pm.item()) >= pmax0
            if alpha == 0.0:
                assert (got[touched] == 1.0).all()


def test_fill_equals_the_reference_and_refuses_bad_ranges(lib_built):
    from meshdqn_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(2)
    pm = torch.full((1,), 2.5, dtype=torch.float32, device="cuda")
    for cap, args in ((10, (8, 4, 4, 3)), (10, (0, 0, 9, 2)), (10, (3, 2, 0, 0)), (10, (5, 0, 5, 0)), (30, (24, 6, 0, 6)),
                      (1000, (900, 300, 200, 700)), (1000, (0, 1000, 0, 0)), (1, (0, 1, 0, 0)), (2, (1, 1, 0, 1))):
        prio = rng.random(cap).astype(np.float32)
        buf, view = _guarded(prio)
        _lib.check(lib.mdq_replay_prio_fill(view.data_ptr(), cap, *args, pm.data_ptr(), None), "mdq_replay_prio_fill")
        torch.cuda.synchronize()
        want = prio.copy()
        per_ref.fill(want, np.float32(2.5), *args)
        assert np.array_equal(view.cpu().numpy(), want), (cap, args)
        assert _guards_intact(buf)
    prio = rng.random(10).astype(np.float32)
    buf, view = _guarded(prio)
    for args, text in (((8, 4, 1, 2), "overlap"), ((2, 3, 4, 2), "overlap"), ((0, 5, 5, 6), "overlap|exceeds"), ((0, 11, 0, 0), "exceeds"),
                       ((10, 1, 0, 0), "exceeds"), ((0, 1, -1, 1), "exceeds"), ((0, -1, 0, 0), "bad arguments")):
        with pytest.raises(_lib.MeshDQNHipError, match=text):
            _lib.check(lib.mdq_replay_prio_fill(view.data_ptr(), 10, *args, pm.data_ptr(), None), "mdq_replay_prio_fill")
        with pytest.raises(ValueError):
            per_ref.fill(prio.copy(), 1.0, *args)
    torch.cuda.synchronize()
    assert np.array_equal(view.cpu().numpy(), prio) and _guards_intact(buf)        # refused before any launch


def test_the_ring_owns_its_priorities(lib_built):
    """`SharedDeviceReplay.prio_fill / prio_draw / prio_update`: allocated on first use, pmax starts at 1, the fill's ranges
    follow the ring's groups, across the wrap-around and for the `close` of a call."""
    from meshdqn_amd.replay import SharedDeviceReplay
    dev = torch.device("cuda")
    G, W = 5, 6
    rep = SharedDeviceReplay.grouped(None, G * W, W, 4, 3, 8, dev)
    assert rep.prio is None and rep.pmax is None
    ref, pmax = np.zeros(G * W, np.float32), np.float32(1.0)
    rng = np.random.default_rng(4)
    idx_d, w_d = torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros(8, device=dev)
    for t in range(9):
        rep.prio_fill(t)
        assert rep.prio_ranges(t) == per_ref.ring_ranges(t, G, W)
        per_ref.fill(ref, pmax, *per_ref.ring_ranges(t, G, W))
        torch.cuda.synchronize()
        assert float(rep.pmax.item()) == float(pmax) and np.array_equal(rep.prio.cpu().numpy(), ref), t
        assert (ref[(t % G) * W:(t % G + 1) * W] == 0).all()                       # the group being written
        assert int((ref > 0).sum()) == rep.finished(t)
        if t == 0:
            continue
        u, beta = rng.random(8), 0.3 + 0.05 * t
        rep.prio_draw(_dev(u, np.float64), beta, idx_d, w_d)
        ridx, rw, _ = per_ref.draw(ref, u, beta)
        torch.cuda.synchronize()
        assert np.array_equal(idx_d.cpu().numpy(), ridx) or t > 1      # (t = 1: every priority is still exactly 1)
        idx = idx_d.cpu().numpy()
        S = per_ref.prefix(ref)
        tol = len(ref) * 2.0 ** -52 * S[-1]
        tt = per_ref.targets(S[-1], u)
        assert (ref[idx] > 0).all() and (np.concatenate([[0.0], S])[idx] - tol <= tt).all() and (tt <= S[idx] + tol).all()
        td = (rng.standard_normal(8) * 2).astype(np.float32)
        rep.prio_update(idx_d, _dev(td, np.float32), 0.6, 1e-6)
        pmax = per_ref.update(ref, pmax, idx, td, 0.6, 1e-6)
        torch.cuda.synchronize()
        got = rep.prio.cpu().numpy()
        assert per_ref.ulp_diff32(got, ref).max() <= 1
        ref[:] = got                                                    # (continue from the device's bits)
        pmax = np.float32(rep.pmax.item())
    rep.prio_fill(9, zero=False)                                        # `close`: the last group is finished, none is opened
    per_ref.fill(ref, pmax, *per_ref.ring_ranges(9, G, W, zero=False))
    torch.cuda.synchronize()
    assert np.array_equal(rep.prio.cpu().numpy(), ref) and (ref > 0).all()
    with pytest.raises(ValueError):
        rep.prio_draw(_dev(np.zeros(8), np.float32), 0.5, idx_d, w_d)


# ------------------------------------------------------------------ the learning step with weights and TD errors
def _arrays(graphs, dev):
    """(helper copied from tests/test_gcn_train_gpu.py)"""
    x = torch.cat([g.x for g in graphs]).float().to(dev).contiguous()
    node_ptr = torch.tensor(np.concatenate([[0], np.cumsum([g.x.shape[0] for g in graphs])]), dtype=torch.int32, device=dev)
    edge_ptr = torch.tensor(np.concatenate([[0], np.cumsum([g.edge_index.shape[1] for g in graphs])]), dtype=torch.int32, device=dev)
    esrc = torch.cat([g.edge_index[0] for g in graphs]).to(torch.int32).to(dev).contiguous()
    edst = torch.cat([g.edge_index[1] for g in graphs]).to(torch.int32).to(dev).contiguous()
    return x, node_ptr, esrc, edst, edge_ptr


def _minibatch(rng, B, n=180, f=17, out=181, emin=200, emax=500):
    """(helper copied from tests/test_gcn_train_gpu.py)"""
    from meshdqn_amd.data import Data

    def graph():
        e = int(rng.integers(emin, emax))
        return Data(x=torch.from_numpy(rng.standard_normal((n, f))).float(),
                    edge_index=torch.from_numpy(rng.integers(0, n, size=(2, e))).long())
    return [(graph(), int(rng.integers(0, out)), None if i % 3 == 2 else graph(), float(rng.uniform(-1, 1))) for i in range(B)]


@pytest.mark.parametrize("select", [True, False])
def test_weighted_learning_step(lib_built, select):
    """`NodeRemovalNet(181, 128, 0.1)`, eight graphs.  A table of ones gives the bits of no table; random weights with one
    exact zero give the loss and gradient of torch autograd of (w * huber).mean() through the package's ragged layers, and an
    all-zero gradient slice for the zero-weight graph; the TD errors equal out / q_other / reward / nonfinal put together in
    fp64 on the host within 4 * 2^-24 * max(|q|, |target|, 1): the roundings of gamma * max, + reward and the final
    difference (gamma = 0.875 is a float)."""
    from meshdqn_amd.airfoilgcnn import NodeRemovalNet
    from meshdqn_amd.data import Batch
    from meshdqn_amd.gcn_fused import FusedGcn
    dev = torch.device("cuda")
    rng = np.random.default_rng(31)
    torch.manual_seed(9)
    nets = [NodeRemovalNet(181, conv_width=128, topk=0.1) for _ in range(2)]
    for m in nets:
        m.set_num_nodes(17)
        m.to(dev)
    B, gamma = 8, 0.875
    mb = _minibatch(rng, B)
    k = 0 if select else 1
    net, other = nets[k], nets[1 - k]
    states = [s for s, _, _, _ in mb]
    nexts = [(n if n is not None else s) for s, _, n, _ in mb]
    action = torch.tensor([a for _, a, _, _ in mb], dtype=torch.int64, device=dev)
    # (the outputs are softmax values: these rewards put TD errors on both sides of the Huber corner at 1)
    reward = torch.tensor([0.3, 2.5, -0.2, -3.0, 0.1, 1.8, -0.6, 2.2], dtype=torch.float32, device=dev)
    nonfinal = torch.tensor([0.0 if n is None else 1.0 for _, _, n, _ in mb], dtype=torch.float32, device=dev)
    f_net, f_other = FusedGcn(net), FusedGcn(other)
    mine, theirs = (states, nexts) if select else (nexts, states)
    qo = f_other.forward_arrays(*_arrays(theirs, dev), 180, 512).clone()
    arr = _arrays(mine, dev)
    mode = 0 if select else 1

    def step(**kw):
        res = f_net.train_step(*arr, 180, 512, mode, qo, action, reward, nonfinal, gamma, **kw)
        torch.cuda.synchronize()
        return [t.clone() for t in res]
    loss0, flat0 = step()
    ones, td = torch.ones(B, device=dev), torch.full((B,), 7.0, device=dev)
    loss1, flat1, out = step(weight=ones, td_out=td, want_out=True)
    assert torch.equal(loss0.view(torch.int32), loss1.view(torch.int32)) and torch.equal(flat0.view(torch.int32), flat1.view(torch.int32))
    loss2, flat2 = step(td_out=td)                              # (TD errors alone: no weights)
    assert torch.equal(loss0, loss2) and torch.equal(flat0, flat2)
    # ---- TD errors against fp64 on the host
    o64, q64, r64, n64 = (t.double().cpu().numpy() for t in (out, qo, reward, nonfinal))
    act = action.cpu().numpy()
    if select:
        q, target = o64[np.arange(B), act], r64 + gamma * n64 * q64.max(1)
    else:
        q, target = q64[np.arange(B), act], r64 + gamma * n64 * o64.max(1)
    bound = 4 * 2.0 ** -24 * np.maximum(np.maximum(np.abs(q), np.abs(target)), 1.0)
    assert (np.abs(td.double().cpu().numpy() - (q - target)) <= bound).all()
    assert float(td.abs().max()) > 1.0 > float(td.abs().min())  # both sides of the Huber corner
    # ---- random weights in [0, 1], one exactly 0, against autograd
    wnp = rng.random(B).astype(np.float32)
    wnp[3] = 0.0
    w = torch.from_numpy(wnp).to(dev)
    td_w = torch.zeros(B, device=dev)
    loss, flat = step(weight=w, td_out=td_w)
    assert torch.equal(td_w, td)                                 # the weights do not enter the TD error
    partial = next(iter(f_net._train_bufs.values()))["partial"]
    assert partial.shape[0] == B and float(partial[3].abs().max()) == 0.0
    assert float(partial[0].abs().max()) > 0.0                  # (graph 0: not terminal, so it has a gradient in both modes)
    net.zero_grad(set_to_none=True)
    bs, bn = Batch.from_data_list(states).to(dev), Batch.from_data_list(nexts).to(dev)
    huber = torch.nn.HuberLoss(reduction="none")
    if select:
        with torch.no_grad():
            nv = other(bn).max(1)[0] * nonfinal
        ref = (w * huber(net(bs).gather(1, action.reshape(-1, 1)).squeeze(1), nv * gamma + reward)).mean()
    else:
        with torch.no_grad():
            pred = other(bs).gather(1, action.reshape(-1, 1)).squeeze(1)
        ref = (w * huber(pred, net(bn).max(1)[0] * nonfinal * gamma + reward)).mean()
    ref.backward()
    assert abs(float(loss.item()) - float(ref.detach())) < 2e-5 * max(abs(float(ref.detach())), 1e-3)
    scale = max(float(p.grad.abs().max()) for p in net.parameters() if p.grad is not None)
    assert scale > 1e-7
    off = 0
    for name, p in net.named_parameters():
        g = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
        if p.grad is None:
            assert float(g.abs().max()) == 0.0, name
        else:
            own = float(p.grad.abs().max())
            assert float((g - p.grad).abs().max()) < 5e-4 * max(own, 1e-6 * scale), (select, name)
    # a graph beyond the edge capacity: its TD error is NaN (what the priority update then skips)
    ecnt = np.diff(arr[4].cpu().numpy())
    small = int(np.sort(ecnt)[B // 2 - 1])                      # an edge capacity that half of the graphs exceed
    big = ecnt > small
    assert big.any() and not big.all()
    td_r = torch.zeros(B, device=dev)
    f_net.train_step(*arr, 180, small, mode, qo, action, reward, nonfinal, gamma, weight=w, td_out=td_r)
    torch.cuda.synchronize()
    keep = torch.from_numpy(~big).to(dev)
    assert np.array_equal(np.isnan(td_r.cpu().numpy()), big) and torch.equal(td_r[keep], td[keep])


# ------------------------------------------------------------------ the loop
def _cfg():
    """(copied from tests/test_train_device_gpu.py)"""
    return dict(flow_config=dict(flow_params=dict(mu=1e-3, rho=1.0, inflow="constant"),
                                 geometry_params=dict(mesh=os.path.join(GOLDEN, "ys930.npz")),
                                 solver_params=dict(dt=0.001, solver_type="lu", smooth=True)),
                agent_params=dict(solver_steps=20, episodes=10, timesteps=10000, threshold=0.001, N_closest=180, gt_drag=-1,
                                  gt_time=-1, u=-1, p=-1, time_reward=0.005, save_steps=4, goal_vertices=0.95, plot_dir=""))


B_ENV, GROUPS, STEPS, BATCH = 6, 5, 12, 8


@pytest.fixture(scope="module")
def base_env(lib_built):
    from meshdqn_amd.env import Env2DAirfoil
    return Env2DAirfoil(_cfg())


def _run(base, prioritized, steps=STEPS, loop=None, seed=23, capacity=B_ENV * GROUPS, **kw):
    from meshdqn_amd.trainer import DistContext, DQNTrainer, train_loop_device
    from meshdqn_amd.vec_env import VecEnv2DAirfoil
    loop = loop or train_loop_device
    np.random.seed(seed)
    random.seed(seed)
    tr = DQNTrainer(n_actions=180, num_inputs=17, ctx=DistContext(), batch_size=BATCH, lr=1e-3, target_update=2,
                    replay_capacity=capacity, prioritized=prioritized)
    np.random.seed(seed)
    random.seed(seed)
    venv = VecEnv2DAirfoil(_cfg(), B_ENV, base_env=base, nthreads=2)
    if loop is train_loop_device:
        kw = dict(dict(chunk=5, per_trace=prioritized is not None), **kw)
    out = loop(tr, venv, steps, eps_decay=2, eps_end=0.6, **kw)
    torch.cuda.synchronize()
    return out, tr


def _first_opt_step():
    return -(-BATCH // B_ENV)             # the first step in front of which the ring holds a minibatch


@pytest.fixture(scope="module")
def per_runs(base_env):
    """Two runs of the prioritized device loop from the same seeds (alpha 0.6; beta from 0.4 to 1 within the run)."""
    opt = dict(alpha=0.6, beta0=0.4, beta_steps=8, eps=1e-6)
    return [_run(base_env, opt) for _ in range(2)]


def test_loop_with_alpha_zero_draws_uniformly_in_strata(base_env):
    """alpha = 0: every priority is exactly 1, so every weight is exactly 1 and draw i of a minibatch over M sampleable
    records is the floor((i + u_i) / 8 * M)-th of them in ring order."""
    out, tr = _run(base_env, dict(alpha=0.0, beta0=0.5, beta_steps=4))
    per = out["per"]
    t_first = _first_opt_step()
    assert per["idx"].shape == per["u"].shape == per["weight"].shape == per["td"].shape == (STEPS - t_first, BATCH)
    assert (per["weight"] == 1.0).all() and np.isfinite(per["td"]).all() and np.isfinite(out["losses"]).all()
    assert len(out["losses"]) == STEPS - t_first
    assert np.array_equal(per["beta"], [min(1.0, 0.5 + 0.5 * g / 4) for g in range(STEPS - t_first)])
    for m in range(STEPS - t_first):
        t = t_first + m
        groups = sorted(s % GROUPS for s in range(max(0, t - GROUPS + 1), t))        # every group but the one being written
        records = np.concatenate([np.arange(g * B_ENV, (g + 1) * B_ENV) for g in groups])
        M = len(records)
        want = [records[int(np.floor(M * ((i + per["u"][m, i]) / BATCH)))] for i in range(BATCH)]
        assert per["idx"][m].tolist() == want, m
    rep = tr.device_memory
    assert (rep.prio.cpu().numpy() == 1.0).all() and float(rep.pmax.item()) == 1.0


def test_loop_trace_replays_through_the_reference(per_runs):
    """Fills, draws with the traced u and updates with the traced TD errors, replayed through tests/per_ref.py: every drawn
    record within the bracket bound of the generic draw test, every weight and the final priorities within one float ulp."""
    out, tr = per_runs[0]
    per, rep = out["per"], tr.device_memory
    cap, t_first = B_ENV * GROUPS, _first_opt_step()
    assert rep.capacity == cap and rep.W == B_ENV and rep.G == GROUPS and rep.steps_pushed == STEPS
    prio, pmax = np.zeros(cap, np.float32), np.float32(1.0)
    assert np.array_equal(per["beta"], [min(1.0, 0.4 + (1.0 - 0.4) * g / 8) for g in range(STEPS - t_first)]) and per["beta"][-1] == 1.0
    assert np.isfinite(per["td"]).all() and float(np.abs(per["td"]).max()) > 0
    for t in range(STEPS):
        per_ref.fill(prio, pmax, *per_ref.ring_ranges(t, GROUPS, B_ENV))
        # the group being written and records never written: 0; every finished record: a priority
        live = np.zeros(cap, bool)
        for s in range(max(0, t - GROUPS + 1), t):
            live[(s % GROUPS) * B_ENV:(s % GROUPS + 1) * B_ENV] = True
        assert np.array_equal(prio > 0, live), t
        if t < t_first:
            continue
        m = t - t_first
        ridx, rw, _ = per_ref.draw(prio, per["u"][m], per["beta"][m])
        idx = per["idx"][m]
        S = per_ref.prefix(prio)
        tol = cap * 2.0 ** -52 * S[-1]
        tt = per_ref.targets(S[-1], per["u"][m])
        assert (prio[idx] > 0).all(), m
        assert (np.concatenate([[0.0], S])[idx] - tol <= tt).all() and (tt <= S[idx] + tol).all(), (m, idx, ridx)
        wr = np.array([np.float32((float(prio[idx].min()) / float(prio[j])) ** per["beta"][m]) for j in idx])
        assert per_ref.ulp_diff32(per["weight"][m], wr).max() <= 1, m
        pmax = per_ref.update(prio, pmax, idx, per["td"][m], 0.6, 1e-6)
    per_ref.fill(prio, pmax, *per_ref.ring_ranges(STEPS, GROUPS, B_ENV, zero=False))          # the close of the call
    got = rep.prio.cpu().numpy()
    assert (got > 0).all()                                           # the ring has wrapped: every record is finished
    assert per_ref.ulp_diff32(got, prio).max() <= 1
    assert per_ref.ulp_diff32(rep.pmax.cpu().numpy(), np.float32(pmax)).max() <= 1
    assert len(np.unique(got)) > cap // 3 and not (per["weight"] == 1.0).all()      # priorities that really differ
    assert len(out["losses"]) == STEPS - t_first and np.isfinite(out["losses"]).all()


def test_loop_short_run_leaves_unwritten_groups_without_priority(base_env):
    out, tr = _run(base_env, dict(alpha=0.6), steps=3)
    prio = tr.device_memory.prio.cpu().numpy()
    assert (prio[:3 * B_ENV] > 0).all() and (prio[3 * B_ENV:] == 0).all()
    assert out["per"]["idx"].shape == (3 - _first_opt_step(), BATCH) and (out["per"]["idx"] < 2 * B_ENV).all()


def test_loop_is_reproducible(per_runs):
    (a, ta), (b, tb) = per_runs
    assert np.array_equal(np.asarray(a["losses"], np.float32).view(np.int32), np.asarray(b["losses"], np.float32).view(np.int32))
    for key in ("u", "idx", "weight", "td", "beta"):
        assert a["per"][key].tobytes() == b["per"][key].tobytes(), key
    assert np.array_equal(a["actions"], b["actions"])
    for na, nb in ((ta.policy_net_1, tb.policy_net_1), (ta.policy_net_2, tb.policy_net_2)):
        for (name, p), q in zip(na.named_parameters(), nb.parameters()):
            assert torch.equal(p, q), name
    assert torch.equal(ta.device_memory.prio, tb.device_memory.prio)


def test_loop_without_the_feature_follows_the_host_loop(base_env):
    """prioritized=None: the device loop launches what it launched before - same actions, rewards and terminations as the
    host loop from the same seeds, losses and networks within the tolerance of the two backward implementations (the
    comparison of tests/test_train_device_gpu.py, on a ring that does not wrap: a wrapped host ring samples the group being
    written too); no priority array is ever allocated."""
    from meshdqn_amd.trainer import train_loop_vec
    a, ta = _run(base_env, None, loop=train_loop_vec, capacity=10000)
    b, tb = _run(base_env, None, capacity=10000)
    assert "per" not in b and tb.device_memory.prio is None and tb.device_memory.pmax is None
    assert np.array_equal(a["dones"], b["dones"])
    assert np.allclose(a["rewards"], b["rewards"], rtol=1e-9, atol=1e-12)
    assert len(a["losses"]) == len(b["losses"]) == STEPS - _first_opt_step() and np.isfinite(b["losses"]).all()
    assert np.allclose(a["losses"], b["losses"], rtol=2e-3, atol=1e-6), (a["losses"], b["losses"])
    assert np.array_equal(a["steps_done"], b["steps_done"])
    for n1, n2 in ((ta.policy_net_1, tb.policy_net_1), (ta.policy_net_2, tb.policy_net_2)):
        for (name, p), q in zip(n1.named_parameters(), n2.parameters()):
            assert float((p - q).detach().abs().max()) < 2e-4 * max(1e-2, float(p.detach().abs().max())), name
    assert ta.num_grads == tb.num_grads and ta.select == tb.select
