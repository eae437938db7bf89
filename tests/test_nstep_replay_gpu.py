"""GPU: n-step returns - `mdq_replay_sample_nstep` through the C ABI on synthetic rings against its numpy restatement
(tests/nstep_ref.py), bit for bit; `DQNTrainer.optimize_device` with `n_step` > 1 against the unchanged learning step fed with
what the restatement composes; `train_loop_device` against a replay of its own trace; `train.py --n-step`."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import nstep_ref
from nstep_ref import Nstep
from test_prioritized_replay_gpu import B_ENV, BATCH, GROUPS, STEPS
from test_prioritized_replay_gpu import _cfg as _cfg_per

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -7            # what every output buffer holds before a launch
GUARD = 16           # entries / rows behind the part a launch may write
OUTPUTS = ("x_s", "x_n", "esrc_s", "edst_s", "esrc_n", "edst_n", "edge_ptr_s", "edge_ptr_n", "action", "reward", "nonfinal")


# ------------------------------------------------------------------ the kernel, called through the C ABI
def _ring(rng, nf, EM, W, G, done_share, nodes=3):
    """A synthetic ring of G groups x W lanes: random features, node ids and rewards (one of them -0.0), edge counts in
    0 .. EM with 0 for s' of terminal records, `done` on about `done_share` of the records."""
    cap, tail = W * G, 2 * nf + 4 * EM
    R = rng.standard_normal((cap, tail + 5)).astype(np.float32)
    R[:, 2 * nf:tail] = rng.integers(0, nodes, (cap, 4 * EM))
    done = rng.random(cap) < done_share
    R[:, tail] = rng.integers(0, EM + 1, cap)
    R[:, tail + 1] = np.where(done, 0, rng.integers(0, EM + 1, cap))
    R[:, tail + 2] = rng.integers(0, nodes + 1, cap)
    R[:, tail + 3] = (rng.standard_normal(cap) * 3).astype(np.float32)
    R[cap // 2, tail + 3] = -0.0
    R[:, tail + 4] = done
    return R


class _Call:
    """The device side of one sampling call: the ring, the draws, sentinel-filled outputs with guard bands."""

    def __init__(self, R, idx, nf, EM):
        from meshdqn_amd import _lib
        n = len(idx)
        self.n, self.nf, self.EM = n, nf, EM
        self.R = torch.from_numpy(np.ascontiguousarray(R, np.float32)).cuda()
        self.idx = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).cuda()
        i32, f32 = torch.int32, torch.float32
        shapes = dict(x_s=((n + 1) * nf, f32), x_n=((n + 1) * nf, f32), esrc_s=(n * EM + GUARD, i32), edst_s=(n * EM + GUARD, i32),
                      esrc_n=(n * EM + GUARD, i32), edst_n=(n * EM + GUARD, i32), edge_ptr_s=(n + 1 + GUARD, i32),
                      edge_ptr_n=(n + 1 + GUARD, i32), action=(n + GUARD, torch.int64), reward=(n + GUARD, f32),
                      nonfinal=(n + GUARD, f32), steps=(n + GUARD, i32))
        self.out = {k: torch.full((m,), SENT, dtype=dt, device="cuda") for k, (m, dt) in shapes.items()}
        self.desc = _lib.ReplaySampleDesc(n=n, rec_len=R.shape[1], nf=nf, EM=EM, R=self.R.data_ptr(), idx=self.idx.data_ptr(),
                                          **{k: self.out[k].data_ptr() for k in OUTPUTS})

    def nstep(self, ns, steps=True):
        from meshdqn_amd import _lib
        return _lib.ReplayNstepDesc(n_step=ns.n_step, W=ns.W, capacity=ns.capacity, head=ns.head, gamma=ns.gamma,
                                    steps=self.out["steps"].data_ptr() if steps else None)

    def launch(self, ns=None, steps=True, plain=False):
        """-> (status, outputs as numpy); `plain`: through `mdq_replay_sample`, else through the new entry point (ns None: NULL)."""
        from meshdqn_amd import _lib
        lib = _lib.load()
        if plain:
            rc = lib.mdq_replay_sample(C.byref(self.desc), None)
        else:
            rc = lib.mdq_replay_sample_nstep(C.byref(self.desc), None if ns is None else C.byref(self.nstep(ns, steps)), None)
        torch.cuda.synchronize()
        return rc, {k: v.cpu().numpy() for k, v in self.out.items()}

    def untouched(self, got):
        return all((v == SENT).all() for v in got.values())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _assert_equals_reference(got, want, n, nf, EM, tag, steps=True):
    """Every output against the restatement, bit for bit, and the sentinel everywhere a launch must not write."""
    for k in ("x_s", "x_n"):
        assert np.array_equal(_bits(got[k][:n * nf]), _bits(want[k].reshape(-1))), (tag, k)
        assert (got[k][n * nf:] == SENT).all(), (tag, k)
    for g in ("s", "n"):
        ptr = want["edge_ptr_" + g]
        assert np.array_equal(got["edge_ptr_" + g][:n + 1], ptr), (tag, g)
        assert (got["edge_ptr_" + g][n + 1:] == SENT).all(), (tag, g)
        for k in ("esrc_" + g, "edst_" + g):
            assert np.array_equal(got[k][:ptr[n]], want[k]), (tag, k)
            assert (got[k][ptr[n]:] == SENT).all(), (tag, k)
    for k in ("action", "reward", "nonfinal") + (("steps",) if steps else ()):
        assert np.array_equal(_bits(got[k][:n]), _bits(want[k])), (tag, k, got[k][:n], want[k])
        assert (got[k][n:] == SENT).all(), (tag, k)
    if not steps:
        assert (got["steps"] == SENT).all(), tag


NF_S, EM_S, W_S, G_S = 6, 4, 4, 6         # 3 nodes x 2 features, rec_len 33, capacity 24


@pytest.fixture(scope="module")
def small_rings():
    rng = np.random.default_rng(5)
    return dict(quarter=_ring(rng, NF_S, EM_S, W_S, G_S, 0.25), none=_ring(rng, NF_S, EM_S, W_S, G_S, 0.0),
                all=_ring(rng, NF_S, EM_S, W_S, G_S, 1.0))


@pytest.fixture(scope="module")
def small_draws():
    """1, 7 and 300 draws with repetitions over the whole ring (300: a thread accumulates more than one earlier draw)."""
    rng = np.random.default_rng(6)
    return {n: rng.integers(0, W_S * G_S, n).astype(np.int32) for n in (1, 7, 300)}


@pytest.mark.parametrize("n_step", [1, 2, 3, 5, 8])
def test_sample_nstep_equals_the_reference_on_small_rings(lib_built, small_rings, small_draws, n_step):
    assert small_rings["quarter"].shape == (24, 33)
    seen = set()
    for name, R in small_rings.items():
        for n, idx in small_draws.items():
            call = _Call(R, idx, NF_S, EM_S)
            for gamma in (1.0, 0.9, 0.0):
                for hg in (0, 3, 5):
                    ns = Nstep(n_step, W_S, W_S * G_S, hg * W_S, gamma)
                    for out in call.out.values():
                        out.fill_(SENT)
                    rc, got = call.launch(ns)
                    assert rc == 0
                    want = nstep_ref.compose(R, NF_S, EM_S, ns, idx)
                    _assert_equals_reference(got, want, n, NF_S, EM_S, (name, n, n_step, gamma, hg))
                    seen.update(want["steps"].tolist())
                    if name == "all":
                        assert (want["steps"] == 1).all() and (want["nonfinal"] == 0).all()
                    if name == "none" and n_step == 8:       # six groups: every walk ends in front of the head (a draw
                        assert np.array_equal(want["steps"], (hg - idx // W_S - 1) % G_S + 1)   # OF the head group: all six)
    assert seen == set(range(1, min(n_step, G_S) + 1))


def test_sample_nstep_on_the_workloads_record_shape(lib_built):
    N, F, EM, W, G, n = 180, 17, 1536, 8, 4, 32
    rng = np.random.default_rng(7)
    R = _ring(rng, N * F, EM, W, G, 0.25, nodes=N)
    idx = rng.integers(0, W * G, n).astype(np.int32)
    ns = Nstep(3, W, W * G, 2 * W, 0.9)
    call = _Call(R, idx, N * F, EM)
    rc, got = call.launch(ns)
    assert rc == 0
    want = nstep_ref.compose(R, N * F, EM, ns, idx)
    _assert_equals_reference(got, want, n, N * F, EM, "workload")
    assert set(want["steps"].tolist()) == {1, 2, 3}
    rc, again = call.launch(ns)                                      # run-to-run identical
    assert rc == 0 and all(np.array_equal(_bits(got[k]), _bits(again[k])) for k in got)


def test_one_step_and_null_are_the_plain_sample(lib_built, small_rings, small_draws):
    """n_step = 1 through the new entry point, for several W / head / gamma, and ns = NULL: the bits of `mdq_replay_sample`."""
    for name, R in small_rings.items():
        for n, idx in small_draws.items():
            call = _Call(R, idx, NF_S, EM_S)
            rc, plain = call.launch(plain=True)
            assert rc == 0
            _assert_equals_reference(plain, nstep_ref.compose(R, NF_S, EM_S, Nstep(1, W_S, 24, 0, 1.0), idx), n, NF_S, EM_S,
                                     (name, n, "plain"), steps=False)
            variants = [None] + [Nstep(1, W, 24, head, gamma) for W, head, gamma in
                                 ((4, 0, 1.0), (4, 20, 0.0), (1, 23, 0.9), (2, 6, 123.5), (12, 12, 0.5), (8, 16, 1.0))]
            for ns in variants:
                for out in call.out.values():
                    out.fill_(SENT)
                rc, got = call.launch(ns)
                assert rc == 0
                for k in OUTPUTS:
                    assert np.array_equal(_bits(got[k]), _bits(plain[k])), (name, n, ns, k)
                assert (got["steps"] == SENT).all() if ns is None else (got["steps"][:n] == 1).all()


def test_steps_may_be_null(lib_built, small_rings, small_draws):
    R, idx = small_rings["quarter"], small_draws[7]
    ns = Nstep(3, W_S, 24, 3 * W_S, 0.9)
    call = _Call(R, idx, NF_S, EM_S)
    rc, got = call.launch(ns, steps=False)
    assert rc == 0
    _assert_equals_reference(got, nstep_ref.compose(R, NF_S, EM_S, ns, idx), 7, NF_S, EM_S, "no steps", steps=False)


def test_bad_arguments_are_refused_before_any_launch(lib_built, small_rings, small_draws):
    """Host-side argument checks only: a negative status, a text, and outputs that still hold the sentinel."""
    from meshdqn_amd import _lib
    lib = _lib.load()
    R, idx = small_rings["quarter"], small_draws[7]
    call = _Call(R, idx, NF_S, EM_S)
    good = Nstep(3, W_S, 24, 8, 0.9)
    for bad, text in ((dict(n_step=0), "n_step"), (dict(n_step=65), "n_step"), (dict(n_step=-3), "n_step"), (dict(W=0), "W"),
                      (dict(W=-4), "W"), (dict(capacity=26), "capacity"), (dict(capacity=4), "capacity"), (dict(W=24), "capacity"),
                      (dict(head=6), "head"), (dict(head=24), "head"), (dict(head=-4), "head"), (dict(gamma=-0.5), "gamma"),
                      (dict(gamma=float("inf")), "gamma"), (dict(gamma=float("nan")), "gamma")):
        ns = good._replace(**bad)
        with pytest.raises(ValueError):
            nstep_ref.check(ns)
        rc, got = call.launch(ns)
        msg = lib.mdq_last_error().decode()
        assert rc < 0 and "mdq_replay_sample_nstep" in msg and text in msg, (bad, rc, msg)
        assert call.untouched(got), bad
    # what mdq_replay_sample refuses, through both entry points
    for field, value in (("n", 0), ("rec_len", 34), ("x_n", None), ("idx", None), ("nonfinal", None)):
        keep = getattr(call.desc, field)
        setattr(call.desc, field, value)
        for kw in (dict(ns=good), dict(ns=None), dict(plain=True)):
            rc, got = call.launch(**kw)
            assert rc < 0 and b"bad arguments" in lib.mdq_last_error(), (field, kw)
            assert call.untouched(got), (field, kw)
        setattr(call.desc, field, keep)
    rc, got = call.launch(good)                                      # ... and the call itself was a good one
    assert rc == 0 and not call.untouched(got)


# ------------------------------------------------------------------ trainer and loop
GAMMA = 0.9
BIG = 10000          # a ring that does not wrap within a run
THRESHOLD = 0.02     # see `_cfg`


def _cfg():
    """The `_cfg` of tests/test_prioritized_replay_gpu.py with a wider accuracy threshold.  With its 0.001 and 20 solver steps
    every removal misses the ground-truth drag by more than the threshold and ends its episode at once (measured on the
    MI355X: 6 of 6 environments done in 29 of 30 batched steps, 5 in the other), so no walk could ever pass its first
    record and no n-step assertion below could hold.  0.02 gives episodes of a few steps that still end inside a run
    (measured, 12 steps of 6 environments: 12 terminations; at 0.01 there are 29, at 0.05 four, at 0.1 none)."""
    cfg = _cfg_per()
    cfg["agent_params"]["threshold"] = THRESHOLD
    return cfg


@pytest.fixture(scope="module")
def base_env(lib_built):
    from meshdqn_amd.env import Env2DAirfoil
    return Env2DAirfoil(_cfg())


def _trainer(seed=23, capacity=BIG, **kw):
    from meshdqn_amd.trainer import DistContext, DQNTrainer
    np.random.seed(seed)
    random.seed(seed)
    return DQNTrainer(n_actions=180, num_inputs=17, ctx=DistContext(), batch_size=BATCH, lr=1e-3, target_update=2,
                      replay_capacity=capacity, gamma=GAMMA, **kw)


def _run(base, steps=STEPS, seed=23, capacity=BIG, loop_kw=None, **kw):
    """(the `_run` of tests/test_prioritized_replay_gpu.py with the trainer's options handed through)"""
    from meshdqn_amd.trainer import train_loop_device
    from meshdqn_amd.vec_env import VecEnv2DAirfoil
    tr = _trainer(seed, capacity, **kw)
    np.random.seed(seed)
    random.seed(seed)
    venv = VecEnv2DAirfoil(_cfg(), B_ENV, base_env=base, nthreads=2)
    lkw = dict(chunk=5, per_trace=tr.prioritized is not None, nstep_trace=tr.n_step > 1)
    out = train_loop_device(tr, venv, steps, eps_decay=2, eps_end=0.6, **dict(lkw, **(loop_kw or {})))
    torch.cuda.synchronize()
    return out, tr


def _same_run(a, ta, b, tb):
    assert np.array_equal(np.asarray(a["losses"], np.float32).view(np.int32), np.asarray(b["losses"], np.float32).view(np.int32))
    assert np.array_equal(a["actions"], b["actions"]) and a["rewards"].tobytes() == b["rewards"].tobytes()
    assert np.array_equal(a["dones"], b["dones"])
    for na, nb in ((ta.policy_net_1, tb.policy_net_1), (ta.policy_net_2, tb.policy_net_2)):
        for (name, p), q in zip(na.named_parameters(), nb.parameters()):
            assert torch.equal(p, q), name
    assert torch.equal(ta.device_memory.R, tb.device_memory.R)
    for key in ("per", "nstep"):
        assert (key in a) == (key in b)
        for k in a.get(key, {}):
            assert a[key][k].tobytes() == b[key][k].tobytes(), (key, k)


PER = dict(alpha=0.6, beta0=0.4, beta_steps=8, eps=1e-6)


@pytest.fixture(scope="module")
def run_one_step(base_env):
    return _run(base_env)


@pytest.fixture(scope="module")
def run_three_steps(base_env):
    return _run(base_env, n_step=3)


@pytest.fixture(scope="module")
def run_three_steps_prioritized(base_env):
    return _run(base_env, n_step=3, prioritized=PER)


def test_n_step_one_is_todays_loop(base_env, run_one_step):
    """`DQNTrainer(n_step=1)` against the default constructor from the same seeds, bitwise: losses, actions, rewards, both
    networks, the ring; the same pair with prioritized replay on, its trace included."""
    out, tr = run_one_step
    assert tr.n_step == 1 and "nstep" not in out
    _same_run(out, tr, *_run(base_env, n_step=1))
    a, ta = _run(base_env, prioritized=PER)
    b, tb = _run(base_env, prioritized=PER, n_step=1)
    assert "per" in a and np.isfinite(a["per"]["td"]).all()
    _same_run(a, ta, b, tb)
    assert torch.equal(ta.device_memory.prio, tb.device_memory.prio)


def _replay_trace(out, tr, n_step):
    """`reward`, `nonfinal` and `steps` of every traced minibatch against the restatement on the FINAL ring (which has not
    wrapped: a finished record keeps its contents); -> per draw, whether its walk ended at a terminal record."""
    rep, tn = tr.device_memory, out["nstep"]
    R = rep.R.cpu().numpy()
    nf, EM = rep.N * rep.F, rep.e_max
    t_first = -(-BATCH // B_ENV)
    M = len(out["losses"])
    assert M == STEPS - t_first and rep.steps_pushed == STEPS < rep.G and rep.W == B_ENV
    for key in ("idx", "reward", "nonfinal", "steps"):
        assert tn[key].shape == (M, BATCH), key
    assert tn["head"].shape == (M,)
    terminal = np.zeros((M, BATCH), bool)
    for m in range(M):
        t = t_first + m
        assert tn["head"][m] == rep.group_base(t) == t * B_ENV
        ns = Nstep(n_step, rep.W, rep.capacity, int(tn["head"][m]), tr.gamma)
        idx = tn["idx"][m]
        assert ((0 <= idx) & (idx < tn["head"][m])).all()
        assert np.array_equal(tn["steps"][m], nstep_ref.steps(R, nf, EM, ns, idx)), m
        assert np.array_equal(_bits(tn["reward"][m]), _bits(nstep_ref.reward(R, nf, EM, ns, idx))), m
        assert np.array_equal(_bits(tn["nonfinal"][m]), _bits(nstep_ref.nonfinal(R, nf, EM, ns, idx))), m
        terminal[m] = [R[nstep_ref.walk(R, nf, EM, ns, j)[-1], -1] > 0.5 for j in idx]
    return terminal


def test_loop_trace_replays_through_the_reference(run_one_step, run_three_steps):
    out, tr = run_three_steps
    terminal = _replay_trace(out, tr, 3)
    steps = out["nstep"]["steps"]
    assert steps.max() == 3 and steps.min() >= 1
    assert (steps[~terminal] < 3).any()                              # cut short by the head
    assert (steps[terminal] < 3).any()                               # ... and by the end of an episode
    assert (out["nstep"]["nonfinal"][terminal] == 0).all()
    assert set(np.unique(out["nstep"]["nonfinal"][~terminal]).tolist()) == {1.0, float(np.float32(GAMMA)), float(np.float32(GAMMA * GAMMA))}
    assert np.isfinite(out["losses"]).all()
    one = run_one_step[0]
    assert len(one["losses"]) == len(out["losses"]) and not np.array_equal(one["losses"], out["losses"])
    assert "per" not in out and tr.device_memory.prio is None


def test_loop_on_a_ring_that_wraps(base_env):
    """capacity = B_ENV * GROUPS: records are overwritten within the run, so only what survives that is asserted."""
    cap = B_ENV * GROUPS
    a, ta = _run(base_env, capacity=cap, n_step=3)
    b, tb = _run(base_env, capacity=cap, n_step=3)
    _same_run(a, ta, b, tb)
    tn = a["nstep"]
    assert ta.device_memory.capacity == cap and STEPS > GROUPS
    assert tn["steps"].min() >= 1 and tn["steps"].max() <= 3 and np.isfinite(a["losses"]).all()
    t_first = -(-BATCH // B_ENV)
    assert np.array_equal(tn["head"], [(t % GROUPS) * B_ENV for t in range(t_first, STEPS)])
    for m in range(len(tn["head"])):
        for j, k in zip(tn["idx"][m], tn["steps"][m]):
            visited = (int(j) + B_ENV * np.arange(int(k))) % cap
            assert not ((tn["head"][m] <= visited) & (visited < tn["head"][m] + B_ENV)).any(), (m, j, k)


def test_loop_with_prioritized_replay(base_env, run_three_steps_prioritized):
    """(The prioritized trace of such a run is replayed in full, and the chain held to fp64, in tests/test_optimizer_chain_gpu.py.)"""
    out, tr = run_three_steps_prioritized
    assert np.isfinite(out["per"]["td"]).all() and np.isfinite(out["losses"]).all()
    assert np.array_equal(out["per"]["idx"], out["nstep"]["idx"])     # the drawn records are the ones the walks start from
    terminal = _replay_trace(out, tr, 3)
    assert out["nstep"]["steps"].max() == 3 and (out["nstep"]["nonfinal"][terminal] == 0).all()
    again, tr2 = _run(base_env, n_step=3, prioritized=PER)
    _same_run(out, tr, again, tr2)
    assert torch.equal(tr.device_memory.prio, tr2.device_memory.prio)


@pytest.mark.parametrize("select", [True, False])
def test_optimize_device_composes_and_leaves_the_learning_step_alone(run_three_steps, select):
    """Two fresh trainers from one seed on the ring a loop run has filled: loss and flat gradient of `optimize_device` of the
    n-step one equal, bit for bit, those of `train_step` called directly on what the restatement composes from the ring's
    host copy (and the fused forward of the other network on those arrays)."""
    rep = run_three_steps[1].device_memory
    dev = rep.R.device
    nf, EM, N = rep.N * rep.F, rep.e_max, rep.N
    tn, t1 = _trainer(n_step=3), _trainer()
    for tr in (tn, t1):
        tr.num_grads, tr.select = 1, select                           # (no toggle in front of this step)
    t = 9                                                             # head at group 9: walks of 1, 2 and 3 records
    random.seed(77)
    idx = rep.draw(t, BATCH)
    idx[0], idx[1], idx[2] = (t - 1) * B_ENV, (t - 2) * B_ENV + 1, 2
    loss_n = torch.zeros(1, device=dev)
    steps = torch.zeros(BATCH, dtype=torch.int32, device=dev)
    tn.optimize_device(rep, idx, loss_out=loss_n, head_step=t, steps_out=steps)
    torch.cuda.synchronize()
    net_n = tn.policy_net_1 if select else tn.policy_net_2
    flat_n = next(iter(tn._fused_of(net_n, "train")._train_bufs.values()))["grad"].clone()
    # ---- the same step by hand
    ns = Nstep(3, rep.W, rep.capacity, rep.group_base(t), GAMMA)
    want = nstep_ref.compose(rep.R.cpu().numpy(), nf, EM, ns, idx)
    assert np.array_equal(steps.cpu().numpy(), want["steps"]) and want["steps"][0] == 1 and want["steps"].max() == 3
    arr = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in want.items()}
    node_ptr = torch.arange(BATCH + 1, dtype=torch.int32, device=dev) * N
    gs = (arr["x_s"].reshape(BATCH, N, -1), node_ptr, arr["esrc_s"], arr["edst_s"], arr["edge_ptr_s"])
    gn = (arr["x_n"].reshape(BATCH, N, -1), node_ptr, arr["esrc_n"], arr["edst_n"], arr["edge_ptr_n"])
    net, other = (t1.policy_net_1, t1.policy_net_2) if select else (t1.policy_net_2, t1.policy_net_1)
    go, gd = (gn, gs) if select else (gs, gn)
    qo = t1._fused_of(other, "train").forward_arrays(*go, N, EM)
    loss_1, flat_1 = t1._fused_of(net, "train").train_step(*gd, N, EM, 0 if select else 1, qo, arr["action"], arr["reward"],
                                                          arr["nonfinal"], GAMMA)
    torch.cuda.synchronize()
    assert torch.equal(loss_n.view(torch.int32), loss_1.view(torch.int32))
    assert torch.equal(flat_n.view(torch.int32), flat_1.view(torch.int32)) and float(flat_n.abs().max()) > 0
    with pytest.raises(ValueError, match="head_step"):
        tn.optimize_device(rep, idx)


def test_train_py_with_n_step(lib_built, tmp_path):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ray_ys930.yaml")))
    cfg["flow_config"]["geometry_params"]["mesh"] = os.path.join(ROOT, "tests", "golden", "ys930.npz")
    cfg["agent_params"].update(solver_steps=20, save_steps=4)
    cfg["optimizer"]["batch_size"] = BATCH
    cpath = os.path.join(str(tmp_path), "cfg.yaml")
    yaml.safe_dump(cfg, open(cpath, "w"))
    save = os.path.join(str(tmp_path), "run")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, "train.py", "--config", cpath, "--envs", str(B_ENV), "--steps", "6", "--n-step", "3",
                          "--save-dir", save, "--save-every", "0"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    losses = np.load(os.path.join(save, "losses.npy"))
    assert len(losses) == 6 - (-(-BATCH // B_ENV)) and np.isfinite(losses).all()
