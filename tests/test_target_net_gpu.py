"""The target network on the GPU: `mdq_double_q_select` and `mdq_target_update` bit for bit against the numpy restatement
(tests/target_net_ref.py), the chain of `DQNTrainer.optimize_device` against the learning step called by hand, and the
option's way through `train_loop_device` and train.py.  Both kernels are select / copy arithmetic: no tolerance anywhere."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import target_net_ref as ref
from test_nstep_replay_gpu import B_ENV, BATCH, PER, STEPS, _cfg, _run, _same_run, _trainer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT_F, SENT_I = -7.5, -7      # what every output buffer holds before a launch
GUARD = 64                     # entries in front of and behind the part a launch may write
NAN, INF = float("nan"), float("inf")
M_LOOP = STEPS - (-(-BATCH // B_ENV))      # minibatches of a loop run: one per batched step once the ring holds a batch


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _lib_():
    from meshdqn_amd import _lib
    return _lib, _lib.load()


def _stream():
    from meshdqn_amd import _lib
    return _lib.stream_ptr()


class _Guarded:
    """A device buffer of `n` entries inside guard bands, everything filled with the sentinel."""

    def __init__(self, n, dtype, sent):
        self.n, self.sent = n, sent
        self.buf = torch.full((n + 2 * GUARD,), sent, dtype=dtype, device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD * self.buf.element_size()

    def body(self):
        return self.buf[GUARD:GUARD + self.n].cpu().numpy()

    def guards_intact(self):
        h = self.buf.cpu().numpy()
        return bool((h[:GUARD] == self.sent).all() and (h[GUARD + self.n:] == self.sent).all())

    def untouched(self):
        return bool((self.buf.cpu().numpy() == self.sent).all())


# ------------------------------------------------------------------ mdq_double_q_select
def _rows(rng, B, OUT, first):
    """Random rows with a planted case per row, cycling through the list from `first` on: ties inside one 64-stride and
    across strides, the maximum in the last column, infinities, NaNs, rows with nothing above -inf."""
    q = rng.standard_normal((B, OUT)).astype(np.float32)
    plants = []
    for j1, j2 in ((5, 9), (5, 69), (64, 128), (0, OUT - 1)):
        if j2 < OUT and j1 != j2:
            plants.append(("tie", j1, j2))
    plants += [("last",), ("+inf",), ("-inf",), ("nan",), ("nan beside",), ("all -inf",), ("all nan",), ("zeros",)]
    for b in range(B):
        p = plants[(first + b) % len(plants)]
        if p[0] == "tie":
            q[b, p[1]] = q[b, p[2]] = np.float32(5.0)
        elif p[0] == "last":
            q[b, OUT - 1] = np.float32(6.0)
        elif p[0] == "+inf":
            q[b, rng.integers(0, OUT, 2)] = INF
        elif p[0] == "-inf":
            q[b, rng.random(OUT) < 0.5] = -INF
        elif p[0] == "nan":
            q[b, rng.random(OUT) < 0.3] = NAN
        elif p[0] == "nan beside":
            j = int(rng.integers(0, OUT))
            q[b, j] = np.float32(7.0)
            q[b, max(j - 1, 0):j] = NAN
            q[b, j + 1:j + 2] = NAN
        elif p[0] == "all -inf":
            q[b] = -INF
        elif p[0] == "all nan":
            q[b] = NAN
        elif p[0] == "zeros":                # -0 and +0 are equal: the first one wins
            q[b] = -np.abs(q[b]) - 1
            q[b, rng.integers(0, OUT, 3)] = (-0.0, 0.0, -0.0)
    return q


def _select(qo_d, qt_d, B, OUT, sel=True):
    _, lib = _lib_()
    q_sel, s = _Guarded(B * OUT, torch.float32, SENT_F), _Guarded(B, torch.int32, SENT_I)
    rc = lib.mdq_double_q_select(B, OUT, qo_d.data_ptr(), qt_d.data_ptr(), q_sel.ptr, s.ptr if sel else None, _stream())
    torch.cuda.synchronize()
    return rc, q_sel, s


@pytest.mark.parametrize("OUT", [1, 2, 63, 64, 65, 128, 181, 300])
def test_select_equals_the_restatement(lib_built, OUT):
    from meshdqn_amd import _lib
    R = _lib.DOUBLE_Q_ROWS
    rng = np.random.default_rng(OUT)
    for n_case, B in enumerate((1, 33, R - 1, R, R + 1)):
        qo = _rows(rng, B, OUT, first=3 * n_case)
        qt = rng.standard_normal((B, OUT)).astype(np.float32)
        qt[rng.random((B, OUT)) < 0.02] = NAN                       # (the value is handed on whatever it is)
        want_q, want_s, want_v = ref.select(qo, qt)
        qo_d, qt_d = torch.from_numpy(qo).cuda(), torch.from_numpy(qt).cuda()
        rc, q_sel, s = _select(qo_d, qt_d, B, OUT)
        assert rc == 0, (OUT, B)
        assert np.array_equal(s.body(), want_s), (OUT, B)
        assert np.array_equal(_bits(q_sel.body()), _bits(want_q.reshape(-1))), (OUT, B)
        assert q_sel.guards_intact() and s.guards_intact(), (OUT, B)
        # (the inputs are only read)
        assert np.array_equal(_bits(qo_d.cpu().numpy()), _bits(qo)) and np.array_equal(_bits(qt_d.cpu().numpy()), _bits(qt))
        rc2, q_sel2, s2 = _select(qo_d, qt_d, B, OUT)               # a second launch: identical bits
        assert rc2 == 0 and torch.equal(q_sel.buf.view(torch.int32), q_sel2.buf.view(torch.int32)) and torch.equal(s.buf, s2.buf)
        rc3, q_sel3, s3 = _select(qo_d, qt_d, B, OUT, sel=False)    # sel = NULL: the same rows, the sel buffer stays as it was
        assert rc3 == 0 and s3.untouched() and torch.equal(q_sel.buf.view(torch.int32), q_sel3.buf.view(torch.int32))
        # one array in both roles: the row's maximum wherever the row has one
        rc4, q_sel4, s4 = _select(qo_d, qo_d, B, OUT)
        want_q4, want_s4, _ = ref.select(qo, qo)
        assert rc4 == 0 and np.array_equal(s4.body(), want_s4) and np.array_equal(_bits(q_sel4.body()), _bits(want_q4.reshape(-1)))


def test_select_refuses_bad_arguments_before_any_launch(lib_built):
    _, lib = _lib_()
    B, OUT = 5, 70
    q = torch.randn(3 * B * OUT + 8, device="cuda")
    qo, qt = q[:B * OUT], q[B * OUT:2 * B * OUT]
    out, s = _Guarded(B * OUT, torch.float32, SENT_F), _Guarded(B, torch.int32, SENT_I)
    before = q.clone()
    good = dict(B=B, OUT=OUT, q_online=qo.data_ptr(), q_target=qt.data_ptr(), q_sel=out.ptr)
    for bad in (dict(B=0), dict(B=-1), dict(OUT=0), dict(OUT=-5), dict(q_online=None), dict(q_target=None), dict(q_sel=None),
                dict(q_sel=qo.data_ptr()), dict(q_sel=qt.data_ptr()), dict(q_sel=qo.data_ptr() + 4),
                dict(q_sel=qt.data_ptr() - 4 * (B * OUT - 1)), dict(q_sel=qt.data_ptr() + 4 * (B * OUT - 1))):
        a = dict(good, **bad)
        rc = lib.mdq_double_q_select(a["B"], a["OUT"], a["q_online"], a["q_target"], a["q_sel"], s.ptr, _stream())
        torch.cuda.synchronize()
        assert rc < 0 and b"mdq_double_q_select" in lib.mdq_last_error(), (bad, rc)
        assert out.untouched() and s.untouched() and torch.equal(q, before), bad
    # q_sel directly behind an input is no overlap, and the call itself was a good one
    rc = lib.mdq_double_q_select(B, OUT, qo.data_ptr(), qt.data_ptr(), qt.data_ptr() + 4 * B * OUT, s.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == 0 and not s.untouched() and torch.equal(q[:2 * B * OUT], before[:2 * B * OUT])


# ------------------------------------------------------------------ mdq_target_update
LENS = (0, 1, 255, 256, 257, 8193)


def _values(rng, n):
    """Normal-range floats: standard normal times 10^[-3, 3].  No denormals on either side of the arithmetic - the smallest
    magnitudes here are some 1e-10, and a difference either cancels to an exact zero or stays a normal number."""
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)


class _Segments:
    """`lens[s]` floats per tensor, every tensor inside guard bands of one destination / one source buffer."""

    def __init__(self, rng, lens, special=False):
        from meshdqn_amd import _lib
        self.lens = list(lens)
        self.off = np.cumsum([GUARD] + [n + GUARD for n in self.lens])[:-1]
        total = int(self.off[-1] + self.lens[-1] + GUARD)
        self.dst0 = np.full(total, SENT_F, np.float32)
        self.src0 = np.full(total, SENT_F, np.float32)
        for o, n in zip(self.off, self.lens):
            self.dst0[o:o + n], self.src0[o:o + n] = _values(rng, n), _values(rng, n)
            if special and n >= 5:           # what only a copy of the bits hands on
                self.src0[o:o + 3] = (-0.0, 0.0, INF)
                self.src0[o + 3:o + 5].view(np.uint32)[:] = (0x7FA12345, 0xFFC00001)
        self.dst, self.src = torch.from_numpy(self.dst0).cuda(), torch.from_numpy(self.src0).cuda()
        d = self.desc = _lib.TargetUpdateDesc()
        d.n = len(self.lens)
        for s, (o, n) in enumerate(zip(self.off, self.lens)):
            d.dst[s], d.src[s], d.len[s] = self.dst.data_ptr() + 4 * int(o), self.src.data_ptr() + 4 * int(o), n

    def launch(self, tau):
        _, lib = _lib_()
        self.desc.tau = tau
        rc = lib.mdq_target_update(C.byref(self.desc), _stream())
        torch.cuda.synchronize()
        return rc

    def want(self, tau, dst0=None):
        out = (self.dst0 if dst0 is None else dst0).copy()
        for o, n in zip(self.off, self.lens):
            out[o:o + n] = ref.polyak(out[o:o + n], self.src0[o:o + n], tau)
        return out

    def untouched(self):
        return np.array_equal(_bits(self.dst.cpu().numpy()), _bits(self.dst0)) and \
            np.array_equal(_bits(self.src.cpu().numpy()), _bits(self.src0))


@pytest.mark.parametrize("n", [1, 2, 32])
def test_target_update_equals_the_restatement(lib_built, n):
    rng = np.random.default_rng(n)
    for k, tau in enumerate((1.0, 0.5, 0.005)):
        lens = [8193] if n == 1 and k == 0 else [LENS[(s + k + n) % len(LENS)] for s in range(n)]
        seg = _Segments(rng, lens, special=tau == 1.0)
        ref.check(n, lens, tau)
        assert seg.launch(tau) == 0, (n, tau)
        got = seg.dst.cpu().numpy()
        want = seg.want(tau)
        assert np.array_equal(_bits(got), _bits(want)), (n, tau, lens)                 # the guard bands are part of `want`
        assert np.array_equal(_bits(seg.src.cpu().numpy()), _bits(seg.src0))
        if tau == 1.0:
            for o, m in zip(seg.off, seg.lens):
                assert np.array_equal(_bits(got[o:o + m]), _bits(seg.src0[o:o + m]))   # src's bits, NaN payloads and -0 included
        else:                                                                          # a second step from where the first ended
            assert seg.launch(tau) == 0
            assert np.array_equal(_bits(seg.dst.cpu().numpy()), _bits(seg.want(tau, want))), (n, tau)


def test_target_update_on_the_networks_parameters(lib_built):
    from meshdqn_amd import _lib
    from meshdqn_amd.airfoilgcnn import NodeRemovalNet
    nets = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        net = NodeRemovalNet(181, 128, 0.1).float()
        net.set_num_nodes(17)
        nets.append(net.cuda())
    online, target = nets
    assert sum(p.numel() for p in online.parameters()) == 173493 and len(list(online.parameters())) <= _lib.PACK_MAX
    d = _lib.TargetUpdateDesc()
    src, dst = list(online.parameters()), list(target.parameters())
    d.n = len(src)
    for i, (p, q) in enumerate(zip(src, dst)):
        d.src[i], d.dst[i], d.len[i] = p.data_ptr(), q.data_ptr(), p.numel()
    lib = _lib.load()
    host_src = [p.detach().cpu().numpy().reshape(-1) for p in src]
    host_dst = [q.detach().cpu().numpy().reshape(-1) for q in dst]
    assert any(not np.array_equal(a, b) for a, b in zip(host_src, host_dst))
    for tau in (0.005, 1.0):
        d.tau = tau
        assert lib.mdq_target_update(C.byref(d), _stream()) == 0
        torch.cuda.synchronize()
        host_dst = [ref.polyak(b, a, tau) for a, b in zip(host_src, host_dst)]
        for i, (p, q) in enumerate(zip(src, dst)):
            assert np.array_equal(_bits(q.detach().cpu().numpy().reshape(-1)), _bits(host_dst[i])), (tau, i)
            assert np.array_equal(_bits(p.detach().cpu().numpy().reshape(-1)), _bits(host_src[i])), (tau, i)
    assert all(torch.equal(p, q) for p, q in zip(src, dst))


def test_target_update_refuses_bad_arguments_before_any_launch(lib_built):
    _, lib = _lib_()
    seg = _Segments(np.random.default_rng(5), [257, 0, 1])
    d = seg.desc

    def refused(tau=0.5, what=""):
        rc = seg.launch(tau)
        assert rc < 0 and b"mdq_target_update" in lib.mdq_last_error(), (what, rc, lib.mdq_last_error())
        assert seg.untouched(), what
    for n in (0, -1, 33):
        d.n = n
        with pytest.raises(ValueError):
            ref.check(n, seg.lens, 0.5)
        refused(what=("n", n))
    d.n = 3
    for tau in (0.0, -0.5, 1.5, 1.0000001, NAN, INF, -INF):
        with pytest.raises(ValueError):
            ref.check(3, seg.lens, tau)
        refused(tau, ("tau", tau))
    for field, s, value in (("dst", 0, None), ("src", 2, None), ("dst", 1, None), ("len", 0, -1), ("len", 2, -(2 ** 31))):
        keep = getattr(d, field)[s]
        getattr(d, field)[s] = value
        refused(what=(field, s, value))
        getattr(d, field)[s] = keep
    keep = d.dst[2]
    d.dst[2] = d.src[2]
    refused(what="dst == src")
    d.dst[2] = keep
    assert lib.mdq_target_update(None, _stream()) < 0 and b"mdq_target_update" in lib.mdq_last_error() and seg.untouched()
    d.n = 1                                  # only the first n tensors are looked at
    d.dst[1] = None
    assert seg.launch(0.5) == 0 and not seg.untouched()


# ------------------------------------------------------------------ the chain of optimize_device
@pytest.fixture(scope="module")
def base_env(lib_built):
    from meshdqn_amd.env import Env2DAirfoil
    return Env2DAirfoil(_cfg())


@pytest.fixture(scope="module")
def run_toggle(base_env):
    """The default trainer's run: the reference point of the loop tests, and its ring feeds the chain tests."""
    return _run(base_env)


def _net_bits(net):
    return [p.detach().clone() for p in net.parameters()]


def _nets_equal(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


def _perturb(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.add_((0.05 * torch.randn(p.shape, generator=g)).to(p.device))


def _grad_of(tr):
    return next(iter(tr._fused_of(tr.policy_net_1, "train")._train_bufs.values()))["grad"].clone()


def _graphs(tr, N):
    b = tr._mb_bufs
    gs = (b["x_s"].clone(), b["node_ptr"], b["esrc_s"].clone(), b["edst_s"].clone(), b["edge_ptr_s"].clone())
    gn = (b["x_n"].clone(), b["node_ptr"], b["esrc_n"].clone(), b["edst_n"].clone(), b["edge_ptr_n"].clone())
    return gs, gn, b["action"].clone(), b["reward"].clone(), b["nonfinal"].clone()


def test_double_chain_equals_the_learning_step_by_hand(run_toggle):
    """`optimize_device` of a "double" trainer whose target differs from its online network, on the ring a loop run has
    filled: loss and flat gradient equal, bit for bit, `train_step` called by hand with `q_other` = the restatement applied to
    the two forwards' read-back outputs; `sel_out` / `value_out` are the restatement's; the target follows after `period`
    steps and not before, its next forward shows the new weights, and its optimiser never steps."""
    rep = run_toggle[1].device_memory
    dev, N, EM = rep.R.device, rep.N, rep.e_max
    period = 3
    td, t1 = _trainer(target_net=dict(kind="double", period=period)), _trainer()
    _perturb(td.policy_net_2, 5)
    t1.policy_net_1.load_state_dict(td.policy_net_1.state_dict())
    t1.policy_net_2.load_state_dict(td.policy_net_2.state_dict())
    target0 = _net_bits(td.policy_net_2)
    assert not _nets_equal(target0, _net_bits(td.policy_net_1))
    random.seed(77)
    idx = rep.draw(9, BATCH)
    loss = torch.zeros(1, device=dev)
    sel, val = torch.full((BATCH,), -1, dtype=torch.int32, device=dev), torch.full((BATCH,), NAN, device=dev)
    td.optimize_device(rep, idx, loss_out=loss, sel_out=sel, value_out=val)
    torch.cuda.synchronize()
    assert td.select is True and td.num_grads == 1
    flat_d = _grad_of(td)
    # ---- the same step by hand, on the arrays the sampling launch left behind
    gs, gn, action, reward, nonfinal = _graphs(td, N)
    q_t = t1._fused_of(t1.policy_net_2, "train").forward_arrays(*gn, N, EM).cpu().numpy()
    q_o = t1._fused_of(t1.policy_net_1, "train").forward_arrays(*gn, N, EM).cpu().numpy()
    want_q, want_s, want_v = ref.select(q_o, q_t)
    assert q_o.shape == (BATCH, 181) and not np.array_equal(q_o, q_t)
    assert np.array_equal(sel.cpu().numpy(), want_s) and np.array_equal(_bits(val.cpu().numpy()), _bits(want_v))
    assert not np.array_equal(want_v, q_t.max(1))                       # the case Double DQN exists for: not the target's own max
    assert ((0 <= want_s) & (want_s < 181)).all() and np.isfinite(want_v).all()
    loss_1, flat_1 = t1._fused_of(t1.policy_net_1, "train").train_step(*gs, N, EM, 0, torch.from_numpy(want_q).to(dev), action,
                                                                       reward, nonfinal, td.gamma)
    torch.cuda.synchronize()
    assert torch.equal(loss.view(torch.int32), loss_1.view(torch.int32))
    assert torch.equal(flat_d.view(torch.int32), flat_1.view(torch.int32)) and float(flat_d.abs().max()) > 0
    # ---- the period: one step earlier the target is what it was, then it is the online network
    q_before = td._fused_of(td.policy_net_2, "train").forward_arrays(*gn, N, EM).clone()
    td.optimize_device(rep, idx)
    torch.cuda.synchronize()
    assert td.num_grads == period - 1 and _nets_equal(_net_bits(td.policy_net_2), target0)
    td.optimize_device(rep, idx)
    torch.cuda.synchronize()
    online = _net_bits(td.policy_net_1)
    assert td.num_grads == period and _nets_equal(_net_bits(td.policy_net_2), online) and not _nets_equal(online, target0)
    # ... and the target's packed copy has followed (the version bump): its forward is the online network's
    q_after = td._fused_of(td.policy_net_2, "train").forward_arrays(*gn, N, EM)
    q_online = td._fused_of(td.policy_net_1, "train").forward_arrays(*gn, N, EM)
    torch.cuda.synchronize()
    assert torch.equal(q_after.view(torch.int32), q_online.view(torch.int32)) and not torch.equal(q_after, q_before)
    assert len(td.opts[1].state) == 0 and td.scheds[1].last_epoch == 0 and len(td.opts[0].state) > 0
    assert td.scheds[0].last_epoch == period and td.select is True
    for kw in (dict(sel_out=sel), dict(value_out=val)):                  # the hand-through belongs to the select launch
        with pytest.raises(ValueError, match="sel_out"):
            t1.optimize_device(rep, idx, **kw)


def test_polyak_chain_moves_the_target_every_period(run_toggle):
    rep = run_toggle[1].device_memory
    tau = 0.25
    tp = _trainer(target_net=dict(kind="double", period=1, tau=tau))
    _perturb(tp.policy_net_2, 6)
    random.seed(78)
    idx = rep.draw(9, BATCH)
    for _ in range(2):
        before = [q.detach().cpu().numpy().reshape(-1) for q in tp.policy_net_2.parameters()]
        tp.optimize_device(rep, idx)
        torch.cuda.synchronize()
        for i, (p, q) in enumerate(zip(tp.policy_net_1.parameters(), tp.policy_net_2.parameters())):
            want = ref.polyak(before[i], p.detach().cpu().numpy().reshape(-1), tau)
            assert np.array_equal(_bits(q.detach().cpu().numpy().reshape(-1)), _bits(want)), i


def test_max_chain_is_the_existing_step_with_select_held(run_toggle):
    """A "max" trainer against a default trainer held at `select = True` whose net 2 was given net 1's weights: the new
    path launches what the existing one launches, so loss, gradient and the updated online network agree bit for bit."""
    rep = run_toggle[1].device_memory
    dev = rep.R.device
    tm, t0 = _trainer(target_net=dict(kind="max", period=100)), _trainer()
    t0.policy_net_2.load_state_dict(t0.policy_net_1.state_dict())
    for tr in (tm, t0):
        _perturb(tr.policy_net_2, 9)
        tr.num_grads, tr.select = 1, True                                # (target_update = 2: no toggle in front of this step)
    random.seed(79)
    idx = rep.draw(9, BATCH)
    lm, l0 = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    tm.optimize_device(rep, idx, loss_out=lm)
    t0.optimize_device(rep, idx, loss_out=l0)
    torch.cuda.synchronize()
    assert t0.select is True and tm.select is True
    assert torch.equal(lm.view(torch.int32), l0.view(torch.int32)) and float(lm) > 0
    assert torch.equal(_grad_of(tm).view(torch.int32), _grad_of(t0).view(torch.int32))
    assert _nets_equal(_net_bits(tm.policy_net_1), _net_bits(t0.policy_net_1))
    assert _nets_equal(_net_bits(tm.policy_net_2), _net_bits(t0.policy_net_2))
    assert "q_sel" not in tm._mb_bufs                                    # no select launch, no buffer for one
    with pytest.raises(ValueError, match="sel_out"):
        tm.optimize_device(rep, idx, sel_out=torch.zeros(BATCH, dtype=torch.int32, device=dev))


# ------------------------------------------------------------------ the loop
DOUBLE = dict(kind="double", period=100)       # a period the run never reaches


def _run_target(base, target_net, **kw):
    trace = target_net is not None and target_net.get("kind", "double") == "double"
    return _run(base, loop_kw=dict(target_trace=True) if trace else None, target_net=target_net, **kw)


def _same_target_trace(a, b):
    assert ("target" in a) == ("target" in b)
    for k in a.get("target", {}):
        assert a["target"][k].tobytes() == b["target"][k].tobytes(), k


@pytest.fixture(scope="module")
def run_double(base_env):
    return _run_target(base_env, DOUBLE)


def test_loop_without_the_option_is_todays_loop(base_env, run_toggle):
    out, tr = run_toggle
    assert tr.target_net is None and "target" not in out and len(out["losses"]) == M_LOOP
    _same_run(out, tr, *_run_target(base_env, None))


def test_loop_double_is_reproducible_and_traces_its_choices(base_env, run_double, run_toggle):
    out, tr = run_double
    again, tr2 = _run_target(base_env, DOUBLE)
    _same_run(out, tr, again, tr2)
    _same_target_trace(out, again)
    tt = out["target"]
    assert tt["sel"].shape == tt["value"].shape == (M_LOOP, BATCH) and len(out["losses"]) == M_LOOP
    assert tt["sel"].dtype == np.int32 and tt["value"].dtype == np.float32
    assert ((0 <= tt["sel"]) & (tt["sel"] < 181)).all() and np.isfinite(tt["value"]).all() and np.isfinite(out["losses"]).all()
    # a period beyond the run: the target is still the initial online network, which is the default trainer's initial net 1
    init = _net_bits(_trainer().policy_net_1)
    assert _nets_equal(_net_bits(tr.policy_net_2), init) and not _nets_equal(_net_bits(tr.policy_net_1), init)
    assert tr.num_grads == M_LOOP and tr.select is True and len(tr.opts[1].state) == 0
    # the same environments as the toggle's run until the first optimiser step, other losses from then on
    assert not np.array_equal(np.asarray(out["losses"]), np.asarray(run_toggle[0]["losses"]))


def test_loop_period_one_ends_with_the_target_equal_to_the_online_network(base_env):
    out, tr = _run_target(base_env, dict(kind="double", period=1, tau=1.0))
    assert _nets_equal(_net_bits(tr.policy_net_2), _net_bits(tr.policy_net_1)) and np.isfinite(out["losses"]).all()
    assert not _nets_equal(_net_bits(tr.policy_net_1), _net_bits(_trainer().policy_net_1))
    # the fixed-target kind runs the same loop without the trace, which it refuses
    from meshdqn_amd.trainer import train_loop_device
    om, tm = _run_target(base_env, dict(kind="max", period=1))
    assert np.isfinite(om["losses"]).all() and "target" not in om and _nets_equal(_net_bits(tm.policy_net_2), _net_bits(tm.policy_net_1))
    with pytest.raises(ValueError, match="target_trace"):
        train_loop_device(tm, None, 3, target_trace=True)


def test_loop_with_prioritized_replay_and_n_step(base_env):
    """(Reproducibility only: the combined chain is held to an fp64 reference in tests/test_optimizer_chain_gpu.py.)"""
    a, ta = _run_target(base_env, DOUBLE, prioritized=PER, n_step=3)
    b, tb = _run_target(base_env, DOUBLE, prioritized=PER, n_step=3)
    _same_run(a, ta, b, tb)
    _same_target_trace(a, b)
    assert torch.equal(ta.device_memory.prio, tb.device_memory.prio)
    assert np.isfinite(a["losses"]).all() and np.isfinite(a["per"]["td"]).all() and np.isfinite(a["target"]["value"]).all()
    assert np.array_equal(a["per"]["idx"], a["nstep"]["idx"])             # the drawn records are the ones the walks start from
    assert a["nstep"]["steps"].max() == 3 and a["target"]["sel"].shape == (M_LOOP, BATCH)
    toggle, _ = _run(base_env, prioritized=PER, n_step=3)
    assert len(toggle["losses"]) == len(a["losses"]) and not np.array_equal(np.asarray(toggle["losses"]), np.asarray(a["losses"]))


def test_train_py_with_a_target_network(lib_built, tmp_path):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ray_ys930.yaml")))
    cfg["flow_config"]["geometry_params"]["mesh"] = os.path.join(ROOT, "tests", "golden", "ys930.npz")
    cfg["agent_params"].update(solver_steps=20, save_steps=4)
    cfg["optimizer"]["batch_size"] = BATCH
    cpath = os.path.join(str(tmp_path), "cfg.yaml")
    yaml.safe_dump(cfg, open(cpath, "w"))
    save = os.path.join(str(tmp_path), "run")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, "train.py", "--config", cpath, "--envs", str(B_ENV), "--steps", "6", "--target-net", "double",
                          "--n-step", "3", "--save-dir", save, "--save-every", "0"], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    losses = np.load(os.path.join(save, "losses.npy"))
    assert len(losses) == 6 - (-(-BATCH // B_ENV)) and np.isfinite(losses).all()
