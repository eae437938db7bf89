"""The Adam kernel on the GPU, through `mdq_adam_step` itself: every launch against the fp64 restatement of tests/adam_ref.py,
within MARGIN = 4 yardsticks (the fp32 restatement's own deviation from fp64, at least one float32 epsilon; per segment and per
quantity: v elementwise relative, m in units of the segment's largest |m|, p in units of its largest update).  The kernel does
the restatement's operations in the restatement's order; it differs by contraction into fused multiply-adds and by its own
sqrt / division, one rounding each - four yardsticks is another formula (test_adam_step_cpu.py: every wrong formula of its
table leaves the bound on these cases).  Every comparison prints `ADAM <case> <quantity>: yardstick, device, ratio` first.
Then the trainer's plumbing (`DQNTrainer._adam_step_device`) on the real network, against the same restatement and bound."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import adam_ref as ref

pytestmark = pytest.mark.gpu
SENT = -7.5                    # what every buffer holds wherever no launch may write
GUARD = 64                     # floats behind every parameter tensor
F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _lib_():
    from meshdqn_amd import _lib
    return _lib, _lib.load()


class _Launch:
    """The caller's side of one `mdq_adam_step`: flat grad / exp_avg / exp_avg_sq with the segments at `offsets` (scattered:
    not monotone in s, gaps between them) and one parameter tensor per segment inside one sentinel-filled buffer, each with
    GUARD floats behind it; tensors whose index is in `odd` start at an odd float offset (4-byte aligned only)."""

    def __init__(self, segs, hp, offsets=None, odd=(), shared_param=False):
        _lib, _ = _lib_()
        self.segs, self.hp = segs, hp
        self.lens = [len(sg["p"]) for sg in segs]
        if offsets is None:
            offsets, total = ref.scattered_layout(self.lens)
        else:
            total = max(o + n for o, n in zip(offsets, self.lens)) + 9
        self.off, n = list(offsets), len(segs)
        flat = {k: np.full(total, SENT, F32) for k in "gmv"}
        self.written = np.zeros(total, bool)
        for sg, o, ln in zip(segs, self.off, self.lens):
            for k in "gmv":
                flat[k][o:o + ln] = sg[k]
            assert not self.written[o:o + ln].any()
            self.written[o:o + ln] = True
        if shared_param:               # one tensor, the segments are consecutive slices of it
            self.pstart = [int(x) for x in np.cumsum([2] + self.lens[:-1])]
            ptotal = self.pstart[-1] + self.lens[-1] + GUARD
        else:
            self.pstart, cur = [], 2
            for s, ln in enumerate(self.lens):
                start = cur | 1 if s in odd else (cur + 3) & ~3
                self.pstart.append(start)
                cur = start + ln + GUARD
            ptotal = cur
        par = np.full(ptotal, SENT, F32)
        self.pwritten = np.zeros(ptotal, bool)
        for sg, st, ln in zip(segs, self.pstart, self.lens):
            par[st:st + ln] = sg["p"]
            self.pwritten[st:st + ln] = True
        self.host = dict(flat, p=par)
        self.dev = {k: torch.from_numpy(a).cuda() for k, a in self.host.items()}
        d = self.desc = _lib.AdamDesc()
        d.n = n
        for s in range(n):
            d.param[s], d.offset[s], d.len[s] = self.dev["p"].data_ptr() + 4 * self.pstart[s], self.off[s], self.lens[s]
        d.grad, d.exp_avg, d.exp_avg_sq = (self.dev[k].data_ptr() for k in "gmv")
        self.set_hp(hp)

    def set_hp(self, hp):
        d = self.desc
        d.lr, d.beta1, d.beta2, d.eps, d.weight_decay = hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"]
        d.bias_correction1, d.bias_correction2 = ref.bias_corrections(hp)

    def launch(self):
        _lib, lib = _lib_()
        rc = lib.mdq_adam_step(C.byref(self.desc), _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def read(self):
        """-> (p, m, v): per segment lists, and the whole buffers for the sentinel checks."""
        self.now = {k: a.cpu().numpy() for k, a in self.dev.items()}
        p = [self.now["p"][st:st + ln] for st, ln in zip(self.pstart, self.lens)]
        m = [self.now["m"][o:o + ln] for o, ln in zip(self.off, self.lens)]
        v = [self.now["v"][o:o + ln] for o, ln in zip(self.off, self.lens)]
        return p, m, v

    def assert_only_the_segments_were_written(self, what):
        now = self.now
        assert np.array_equal(_bits(now["g"]), _bits(self.host["g"])), (what, "grad was written")
        for k in "mv":
            assert (now[k][~self.written] == SENT).all(), (what, k, "a gap lost its sentinel")
        assert (now["p"][~self.pwritten] == SENT).all(), (what, "a guard float behind a parameter tensor lost its sentinel")

    def untouched(self):
        return all(np.array_equal(_bits(a.cpu().numpy()), _bits(self.host[k])) for k, a in self.dev.items())


def _hold(name, segs, refs, p, m, v):
    """Print the worst segment per quantity, then hold every segment to the bound; exact zeros of the fp64 update leave p's bits."""
    worst, fails = {}, []
    for s, (sg, r) in enumerate(zip(segs, refs)):
        for q, (d32, d) in ref.segment_deviations(sg, r, p[s], m[s], v[s]).items():
            y = ref.yardstick(d32)
            if q not in worst or d / y > worst[q][2]:
                worst[q] = (y, d, d / y, sg["label"])
            if not ref.within(d, d32):
                fails.append((sg["label"], q, y, d, d / y))
        zero = r["upd64"] == 0
        if not np.array_equal(_bits(p[s])[zero], _bits(sg["p"])[zero]):
            fails.append((sg["label"], "p changed where the fp64 update is exactly zero"))
    for q in "vmp":
        if q in worst:
            y, d, ratio, label = worst[q]
            print(f"ADAM {name} {q}: yardstick {y:.3e}, device {d:.3e}, ratio {ratio:.2f} (segment {label})")
    assert not fails, (name, fails[:6])


def _run_case(case, refs, **layout):
    L = _Launch(case["segs"], case["hp"], **layout)
    assert L.launch() == 0, case["name"]
    p, m, v = L.read()
    L.assert_only_the_segments_were_written(case["name"])
    _hold(case["name"], case["segs"], refs, p, m, v)
    return L


# ------------------------------------------------------------------ single steps from a given state
@pytest.mark.parametrize("hname", list(ref.HYPER))
def test_single_steps_against_fp64(lib_built, hname):
    """20 segments, one per (gradient band, parameter band), at steps 1, 2, 10, 1000 and 2 000 000."""
    for t in ref.STEPS:
        _run_case(ref.single_case(hname, t), ref.single_reference(hname, t), odd=(1, 6, 11))


# ------------------------------------------------------------------ geometry
@pytest.mark.parametrize("n", ref.GEOM_LENS_1)
def test_one_segment_of_every_length_around_the_stride(lib_built, n):
    _run_case(ref.geometry_case((n,)), ref.geometry_reference((n,)), offsets=[5], odd=(0,) if n % 2 else ())


def test_32_segments_scattered_over_the_flat_buffers(lib_built):
    lens = ref.GEOM_LENS_32
    L = _run_case(ref.geometry_case(lens), ref.geometry_reference(lens), odd=tuple(range(1, 32, 3)))
    assert L.desc.n == ref.PACK_MAX and L.off != sorted(L.off)
    assert any(L.pstart[s] % 4 for s in range(32)) and any(L.pstart[s] % 4 == 0 for s in range(32))


# ------------------------------------------------------------------ the chain
def test_chain_of_25_launches_follows_the_fp64_chain(lib_built):
    """The kernel's own output fed back, fresh gradients per step, two lr milestones on the way; after every step against the
    fp64 chain, in units of the fp32 chain's drift at that step."""
    c = ref.chain_case()
    c64, c32 = ref.chain_reference()
    z = np.zeros_like(c["p"])
    cuts = np.cumsum((0,) + c["lens"])
    sl = [slice(int(a), int(b)) for a, b in zip(cuts, cuts[1:])]
    L = _Launch([dict(label=f"s{i}", p=c["p"][s], m=z[s], v=z[s], g=z[s]) for i, s in enumerate(sl)], dict(c["hp"], step=1))
    p0 = c["p"].astype(np.float64)
    for k, g in enumerate(c["grads"]):
        for s, o in zip(sl, L.off):
            L.dev["g"][o:o + s.stop - s.start] = torch.from_numpy(g[s]).cuda()
        L.host["g"] = L.dev["g"].cpu().numpy()
        L.set_hp(dict(c["hp"], step=k + 1, lr=c["lrs"][k]))
        assert L.launch() == 0, k
        p, m, v = L.read()
        L.assert_only_the_segments_were_written(("chain", k))
        before = p0 if k == 0 else c64[k - 1][0]
        fails = []
        for q, i, got in (("v", 2, v), ("m", 1, m), ("p", 0, p)):
            rows = []
            for j, s in enumerate(sl):
                base = before[s] if q == "p" else None
                d32, d = ref.deviation(q, c32[k][i][s], c64[k][i][s], base), ref.deviation(q, got[j], c64[k][i][s], base)
                rows.append((d / ref.yardstick(d32), ref.yardstick(d32), d, j))
                if not ref.within(d, d32):
                    fails.append((k + 1, q, j, d32, d))
            ratio, y, d, j = max(rows)
            print(f"ADAM chain/step{k + 1} {q}: yardstick {y:.3e}, device {d:.3e}, ratio {ratio:.2f} (segment s{j})")
        assert not fails, fails


# ------------------------------------------------------------------ exact properties
def _flat_case(n_total=20003):
    case = ref.geometry_case((n_total,))
    return case, case["segs"][0]


def _split(sg, n):
    cuts = np.linspace(0, len(sg["p"]), n + 1).astype(int)
    cuts[1] = cuts[0]                                            # (one empty segment among them)
    return [dict(label=f"s{i}", **{k: sg[k][a:b] for k in "pmvg"}) for i, (a, b) in enumerate(zip(cuts, cuts[1:]))], cuts


def test_one_segment_32_segments_and_a_relaunch_give_the_same_bits(lib_built):
    case, sg = _flat_case()
    one = _Launch([sg], case["hp"], offsets=[0])
    again = _Launch([sg], case["hp"], offsets=[0])
    parts, cuts = _split(sg, 32)
    many = _Launch(parts, case["hp"], offsets=[int(c) for c in cuts[:-1]], shared_param=True)
    assert one.launch() == 0 and again.launch() == 0 and many.launch() == 0
    p1, m1, v1 = (a[0] for a in one.read())
    p2, m2, v2 = (a[0] for a in again.read())
    p3, m3, v3 = (np.concatenate(a) for a in many.read())
    for a, b, c in ((p1, p2, p3), (m1, m2, m3), (v1, v2, v3)):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))
    assert not np.array_equal(_bits(p1), _bits(sg["p"]))
    for L in (one, again, many):
        L.assert_only_the_segments_were_written("same bits")


def test_nothing_to_do_leaves_every_bit(lib_built):
    """g = m = v = 0 and wd = 0: p keeps its bits (the sign of a zero included), m and v stay +0."""
    rng = np.random.default_rng(8)
    n = 8193 + 300
    p = ref.band(rng, 1.0, n)
    p[:6] = (0.0, -0.0, 1e-30, -3e38, 1.0, -1.0)
    z = np.zeros(n, F32)
    for t in (1, 7):
        L = _Launch([dict(label="z", p=p, m=z, v=z, g=z)], dict(ref.HYPER["wd0"], step=t), offsets=[3])
        assert L.launch() == 0
        pd, md, vd = (a[0] for a in L.read())
        assert np.array_equal(_bits(pd), _bits(p)) and not _bits(md).any() and not _bits(vd).any()
        L.assert_only_the_segments_were_written("zeros")


def test_a_nan_gradient_stays_in_its_element(lib_built):
    case, sg = _flat_case(8192 + 500)
    where = (0, 255, 256, 8191, 8192, len(sg["p"]) - 1)
    bad = dict(sg, g=sg["g"].copy())
    bad["g"][list(where)] = np.nan
    parts_f, cuts = _split(sg, 5)
    parts_n, _ = _split(bad, 5)
    offs = [int(c) + 11 * i for i, c in enumerate(cuts[:-1])]
    fin, nan = _Launch(parts_f, case["hp"], offsets=offs), _Launch(parts_n, case["hp"], offsets=offs)
    assert fin.launch() == 0 and nan.launch() == 0
    keep = np.ones(len(sg["p"]), bool)
    keep[list(where)] = False
    for a, b in zip(fin.read(), nan.read()):
        a, b = np.concatenate(a), np.concatenate(b)
        assert np.isnan(b[~keep]).all() and np.isfinite(a).all()
        assert np.array_equal(_bits(a)[keep], _bits(b)[keep])
    assert (nan.now["p"][~nan.pwritten] == SENT).all() and (nan.now["m"][~nan.written] == SENT).all()


# ------------------------------------------------------------------ refusals
def _refusal_launch():
    case = ref.geometry_case(ref.REFUSAL_LENS)
    return case, _Launch(case["segs"], case["hp"])


@pytest.mark.parametrize("rid,field,change", ref.REFUSALS, ids=[r[0] for r in ref.REFUSALS])
def test_refuses_bad_arguments_before_any_launch(lib_built, rid, field, change):
    """Only arguments the entry point refuses are passed: nothing out of range is ever launched."""
    _lib, lib = _lib_()
    _, L = _refusal_launch()
    d = L.desc
    for k, val in change.items():
        if k in ("param", "len", "offset"):
            getattr(d, k)[val[0]] = val[1]
        else:
            setattr(d, k, val)
    rc = lib.mdq_adam_step(C.byref(d), _lib.stream_ptr())
    torch.cuda.synchronize()
    msg = lib.mdq_last_error().decode()
    assert rc != 0 and "mdq_adam_step" in msg and re.search(r"\b" + field + r"\b", msg), (rid, rc, msg)
    assert L.untouched(), rid


def test_accepts_an_empty_segment_whatever_its_pointer(lib_built):
    _lib, lib = _lib_()
    case, L = _refusal_launch()
    assert L.lens[1] == 0
    L.desc.param[1] = None
    assert L.launch() == 0
    p, m, v = L.read()
    L.assert_only_the_segments_were_written("empty segment")
    _hold("refusal-base", case["segs"], ref.geometry_reference(ref.REFUSAL_LENS), p, m, v)
    L.desc.n = 1                               # only the first n segments are looked at
    L.desc.param[2], L.desc.len[2], L.desc.offset[2] = None, -1, -1
    assert L.launch() == 0
    assert lib.mdq_adam_step(None, _lib.stream_ptr()) != 0 and b"mdq_adam_step" in lib.mdq_last_error()


# ------------------------------------------------------------------ the trainer's plumbing, on the real network
def _trainer(**kw):
    from meshdqn_amd.trainer import DistContext, DQNTrainer
    return DQNTrainer(n_actions=180, num_inputs=17, ctx=DistContext(device=torch.device("cuda")), **kw)


def _trainer_step(tr, rng, name, lr_expected=None):
    """One `_adam_step_device(0, flat)` with a fresh gradient, every trained parameter tensor held to the restatement from the
    state the trainer held before; unused parameters keep their bits."""
    net, opt = tr.policy_net_1, tr.opts[0]
    total = sum(q.numel() for q in net.parameters())
    a = tr._adam_state(0, total)
    grp = opt.param_groups[0]
    hp = dict(lr=float(grp["lr"]), beta1=grp["betas"][0], beta2=grp["betas"][1], eps=float(grp["eps"]), wd=float(grp["weight_decay"]),
              step=int(opt.state[a["params"][0]]["step"]) + 1)
    if lr_expected is not None:
        assert hp["lr"] == lr_expected, (name, hp["lr"], lr_expected)
    flat = ref.band(rng, 0.1, total)
    m0, v0 = a["m"].cpu().numpy(), a["v"].cpu().numpy()
    trained = {id(q) for q in a["params"]}
    rest = [(q, q.detach().clone()) for q in net.parameters() if id(q) not in trained]
    segs = []
    for i, q in enumerate(a["params"]):
        o, ln = a["views"][id(q)][2], q.numel()
        segs.append(dict(label=f"param{i}/len{ln}", p=q.detach().cpu().numpy().reshape(-1).copy(), m=m0[o:o + ln], v=v0[o:o + ln],
                         g=flat[o:o + ln]))
    tr._adam_step_device(0, torch.from_numpy(flat).cuda())
    torch.cuda.synchronize()
    m1, v1 = a["m"].cpu().numpy(), a["v"].cpu().numpy()
    p = [q.detach().cpu().numpy().reshape(-1) for q in a["params"]]
    m = [m1[a["views"][id(q)][2]:][:q.numel()] for q in a["params"]]
    v = [v1[a["views"][id(q)][2]:][:q.numel()] for q in a["params"]]
    _hold(name, segs, ref.reference(dict(hp=hp, segs=segs)), p, m, v)
    assert all(torch.equal(q, w) for q, w in rest) and all(q not in opt.state for q, _ in rest)
    assert all(float(opt.state[q]["step"]) == hp["step"] for q in a["params"])
    return hp


def test_trainer_crosses_lr_milestones(lib_built):
    """A step uses the lr in force BEFORE `sched.step()`: with milestones [2, 3] the five steps run at lr, lr, lr/10, lr/100, lr/100."""
    tr = _trainer(lr=3e-3, weight_decay=1e-2)
    tr.scheds[0] = torch.optim.lr_scheduler.MultiStepLR(tr.opts[0], milestones=[2, 3], gamma=0.1)
    rng = np.random.default_rng(31)
    lr, used = 3e-3, []
    for k in range(5):
        used.append(_trainer_step(tr, rng, f"trainer/milestones/step{k + 1}", lr_expected=lr)["lr"])
        if k + 1 in (2, 3):
            lr = lr * 0.1
    assert used[0] == used[1] == 3e-3 and used[2] == 3e-3 * 0.1 and used[3] == used[4] == 3e-3 * 0.1 * 0.1


@pytest.mark.parametrize("kw", [dict(weight_decay=0.0), dict()], ids=["wd0", "defaults"])
def test_trainer_hyper_parameter_sets(lib_built, kw):
    tr = _trainer(**kw)
    rng = np.random.default_rng(32)
    for k in range(3):
        hp = _trainer_step(tr, rng, f"trainer/{'wd0' if kw else 'defaults'}/step{k + 1}")
        assert hp["lr"] == 1e-5 and hp["wd"] == (0.0 if kw else 1e-6) and hp["step"] == k + 1


def test_trainer_follows_a_reseated_parameter(lib_built):
    """The storage of a LATER parameter is replaced between two steps: the next step lands in the tensor the network owns now,
    and the abandoned storage keeps its bits."""
    tr = _trainer(lr=3e-3, weight_decay=1e-2)
    rng = np.random.default_rng(33)
    _trainer_step(tr, rng, "trainer/reseat/step1")
    prm = tr._adam[0]["params"]
    moved = [prm[3], prm[len(prm) - 1]]
    old = [q.data for q in moved]
    kept = [o.clone() for o in old]
    for q in moved:
        q.data = q.data.clone()
    assert all(q.data_ptr() != o.data_ptr() for q, o in zip(moved, old))
    _trainer_step(tr, rng, "trainer/reseat/step2")
    assert all(torch.equal(o.view(torch.int32), k.view(torch.int32)) for o, k in zip(old, kept))
    first = prm[0]                              # ... and the first one too, as before
    first.data = first.data.clone()
    _trainer_step(tr, rng, "trainer/reseat/step3")
