"""The Adam step without a GPU: the conditions under which test_adam_step_gpu.py means something.  The fp64 restatement
(tests/adam_ref.py) is torch.optim.Adam in float64, its fp32 run has torch's fp32 constants, every case of the tables is
well-conditioned for fp32 (no denormal anywhere), and every case table has bite: a table of wrong formulas, each of which
at least one case puts beyond the bound the kernel is held to."""
import math
import os
import re

import numpy as np
import pytest
import torch

import adam_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
TINY32 = float(np.finfo(np.float32).tiny)
ULPS = 4.0       # torch's own operation order ((alpha t1) t2 in addcmul / addcdiv, its two-sided lerp) may differ by a rounding


# ------------------------------------------------------------------ the fp64 restatement is torch.optim.Adam
def _torch_step(p, m, v, g, hp, dtype):
    """One `torch.optim.Adam.step` (single-tensor implementation) on the CPU from the state (m, v, step - 1)."""
    w = torch.nn.Parameter(torch.from_numpy(np.array(p, dtype)))
    opt = torch.optim.Adam([w], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], weight_decay=hp["wd"], foreach=False)
    if hp["step"] > 1:
        opt.state[w] = dict(step=torch.tensor(float(hp["step"] - 1)), exp_avg=torch.from_numpy(np.array(m, dtype)),
                            exp_avg_sq=torch.from_numpy(np.array(v, dtype)))
    else:
        assert not np.any(m) and not np.any(v)
    w.grad = torch.from_numpy(np.array(g, dtype))
    opt.step()
    st = opt.state[w]
    assert float(st["step"]) == float(hp["step"])
    return w.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def _ulps(got, want, scale):
    """Largest |got - want| in units of the spacing of fp64 at `scale` (elementwise, at least |want|)."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    if got.size == 0:
        return 0.0
    return float((np.abs(got - want) / np.spacing(np.maximum(np.maximum(np.abs(want), np.abs(got)), scale))).max())


def _scales(p, m, v, g, hp, got):
    """The magnitude one rounding is taken at, per quantity.  torch may round g + wd p once where the restatement rounds
    twice, and orders its products differently; such a rounding is half a spacing of the LARGEST term of the sum it
    belongs to, not of a result that the terms cancel in.  So exp_avg is measured at max(|m|, |g|, |wd p|), exp_avg_sq at
    max(b2 v, w2 max(|g|, |wd p|)^2), and p at max(|p|, the update formed from exp_avg's scale in place of exp_avg)."""
    w1, w2, b2, lr_c, bc2s, eps, wd = ref.scalars(hp)
    p, m, v, g = (np.abs(np.asarray(a, F64)) for a in (p, m, v, g))
    gmax = np.maximum(g, wd * p)
    sm = np.maximum(m, gmax)
    sv = np.maximum(b2 * v, w2 * gmax * gmax)
    with np.errstate(all="ignore"):
        upd = lr_c * (sm / (np.sqrt(np.asarray(got[2], F64)) / bc2s + eps))
    return dict(p=np.maximum(p, np.where(np.isfinite(upd), upd, 0.0)), m=sm, v=sv)


def _cat(case, key):
    return np.concatenate([sg[key] for sg in case["segs"]])


def test_fp64_restatement_equals_torch_adam_in_float64():
    worst = dict(p=(0.0, ""), m=(0.0, ""), v=(0.0, ""))
    cases = ref.single_cases() + [ref.geometry_case(ref.GEOM_LENS_32), ref.geometry_case((ref.GEOM_LENS_1[-1],))]
    for case in cases:
        p, m, v, g = (_cat(case, k) for k in "pmvg")
        want = _torch_step(p, m, v, g, case["hp"], F64)
        got = ref.step(p, m, v, g, case["hp"], F64)
        sc = _scales(p, m, v, g, case["hp"], got)
        for k, a, b in zip("pmv", got, want):
            worst[k] = max(worst[k], (_ulps(a, b, sc[k]), case["name"]))
    # the chain: torch keeps its own state over 25 steps, the lr changes twice
    c = ref.chain_case()
    w = torch.nn.Parameter(torch.from_numpy(c["p"].astype(F64)))
    opt = torch.optim.Adam([w], lr=c["hp"]["lr"], betas=(c["hp"]["beta1"], c["hp"]["beta2"]), eps=c["hp"]["eps"],
                           weight_decay=c["hp"]["wd"], foreach=False)
    prev = (c["p"].astype(F64), np.zeros(len(c["p"])), np.zeros(len(c["p"])))
    for k, g in enumerate(c["grads"]):          # torch runs free; every step of it is the restatement's step from torch's state
        opt.param_groups[0]["lr"] = hp_lr = c["lrs"][k]
        w.grad = torch.from_numpy(g.astype(F64))
        opt.step()
        st = opt.state[w]
        hp = dict(c["hp"], step=k + 1, lr=hp_lr)
        got = ref.step(*prev, g, hp, F64)
        now = (w.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy())
        sc = _scales(*prev, g, hp, got)
        for key, a, b in zip("pmv", got, now):
            worst[key] = max(worst[key], (_ulps(a, b, sc[key]), f"chain/step{k + 1}"))
        prev = now
    # ... and the free-running fp64 chain of the restatement stays beside it (the drift of 25 steps of roundings)
    drift = max(float(np.abs(a - b).max()) for a, b in zip(ref.chain_reference()[0][-1], prev))
    print(f"ADAM-CPU free-running fp64 chain against torch after {ref.CHAIN_K} steps: largest difference {drift:.2e}")
    assert drift < 1e-12
    for k in "pmv":
        print(f"ADAM-CPU fp64 restatement against torch float64, {k}: {worst[k][0]:.2f} ulp at {worst[k][1]}")
    for k in "pmv":
        assert worst[k][0] <= ULPS, (k, worst[k])


def test_fp32_restatement_has_torchs_fp32_constants():
    one, zero = np.ones(1, F32), np.zeros(1, F32)
    hp = dict(ref.HYPER["wd0"], step=1)
    _, m1, v1 = ref.step(zero, zero, zero, one, hp, F32)
    assert v1.dtype == F32 and int(v1.view(np.uint32)[0]) == int(F32(0.001).view(np.uint32)) == 981668463
    assert int(m1.view(np.uint32)[0]) == int(F32(1.0 - 0.9).view(np.uint32))
    _, tm, tv = _torch_step(zero, zero, zero, one, hp, F32)
    assert int(tv.view(np.uint32)[0]) == 981668463 and int(tm.view(np.uint32)[0]) == int(m1.view(np.uint32)[0])
    # ... which the weights formed in float are not: 1.f - (float)0.999 is 1.29e-5 of itself below
    assert int((F32(1.0) - F32(0.999)).view(np.uint32)) == 981668352
    _, _, vm = _mutant("float weights", zero, zero, zero, one, hp)
    assert int(vm.view(np.uint32)[0]) == 981668352
    # float64: the run is the plain double formula
    p64, m64, v64 = ref.step(zero, zero, zero, one, hp, F64)
    assert p64.dtype == F64 and m64[0] == 1.0 - 0.9 and v64[0] == 1.0 - 0.999
    assert p64[0] == 0.0 - (1e-5 / (1.0 - 0.9)) * (m64[0] / (math.sqrt(v64[0]) / math.sqrt(1.0 - 0.999) + 1e-8))


# ------------------------------------------------------------------ no denormal anywhere
def _all_normal_or_zero(trace):
    if "decay" in trace:    # g' = g + wd p is no cancelling sum (one rounding there may be contracted away by the kernel)
        terms = np.abs(np.asarray(trace["g0"], F64)) + np.abs(np.asarray(trace["decay"], F64))
        assert (terms <= ref.CANCEL * np.abs(np.asarray(trace["g"], F64))).all()
    for k, a in trace.items():
        a = np.abs(np.asarray(a, F64))
        assert np.isfinite(a).all(), k
        bad = (a != 0) & (a < TINY32)
        assert not bad.any(), (k, float(a[bad].min()))


def test_every_case_is_well_conditioned_for_fp32():
    n = 0
    cases = ref.single_cases() + [ref.geometry_case(ref.GEOM_LENS_32)] + [ref.geometry_case((ln,)) for ln in ref.GEOM_LENS_1]
    for case in cases:
        for sg in case["segs"]:
            for a in (sg["p"], sg["m"], sg["v"], sg["g"]):
                assert a.dtype == F32
            assert (sg["v"] >= 0).all()
            t32 = {}
            ref.step(sg["p"], sg["m"], sg["v"], sg["g"], case["hp"], F32, t32)
            _all_normal_or_zero(dict(t32, p0=sg["p"], m0=sg["m"], v0=sg["v"], g0=sg["g"]))
            n += 1
    c = ref.chain_case()
    p, m, v = c["p"], np.zeros_like(c["p"]), np.zeros_like(c["p"])
    for k, g in enumerate(c["grads"]):
        t32 = {}
        p, m, v = ref.step(p, m, v, g, dict(c["hp"], step=k + 1, lr=c["lrs"][k]), F32, t32)
        _all_normal_or_zero(dict(t32, g0=g))
    assert n == (len(ref.HYPER) * len(ref.STEPS)) * 20 + 32 + len(ref.GEOM_LENS_1)
    # every scalar of every hyper-parameter set is a normal float32 too, and the tables hold what they claim
    for case in ref.single_cases():
        assert all(x == 0 or abs(float(F32(x))) >= TINY32 for x in ref.scalars(case["hp"]))
        ref.check(len(case["segs"]), [ref.SEG_LEN] * 20, [0] * 20, dict(case["hp"], bias_correction1=ref.bias_corrections(case["hp"])[0],
                                                                      bias_correction2=ref.bias_corrections(case["hp"])[1]))
    assert sorted(set(ref.GEOM_LENS_32)) == [0, 1, 7, 256, 8193] and len(ref.GEOM_LENS_32) == ref.PACK_MAX
    assert max(sum(ref.GEOM_LENS_32), max(ref.GEOM_LENS_1), sum(ref.CHAIN_LENS)) < 10 ** 5
    assert ref.GEOM_LENS_1 == (1, 255, 256, 257, ref.STRIDE - 1, ref.STRIDE, ref.STRIDE + 1, 2 * ref.STRIDE + 1, 3 * ref.STRIDE + 77)
    off, total = ref.scattered_layout(ref.GEOM_LENS_32)
    spans = sorted((o, o + n_) for o, n_ in zip(off, ref.GEOM_LENS_32) if n_)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and any(a[1] < b[0] for a, b in zip(spans, spans[1:]))
    assert off != sorted(off) and spans[-1][1] <= total


# ------------------------------------------------------------------ the tables have bite
MUTANTS = ("float weights", "eps inside the root", "bc2 without its root", "bc1 omitted", "eps dropped", "decoupled decay",
           "v from the undecayed g")


def _mutant(kind, p, m, v, g, hp):
    """The fp32 restatement with one thing wrong."""
    assert kind in MUTANTS
    T = F32
    w1, w2, b2, lr_c, bc2s, eps, wd = (T(x) for x in ref.scalars(hp))
    if kind == "float weights":
        w1, w2 = T(1) - T(hp["beta1"]), T(1) - T(hp["beta2"])
    if kind == "bc2 without its root":
        bc2s = T(ref.bias_corrections(hp)[1])
    if kind == "bc1 omitted":
        lr_c = T(hp["lr"])
    p, m, v, g = (np.asarray(a, T) for a in (p, m, v, g))
    with np.errstate(all="ignore"):
        g_raw = g
        if wd != 0 and kind != "decoupled decay":
            g = g + wd * p
        m1 = m + w1 * (g - m)
        gv = g_raw if kind == "v from the undecayed g" else g
        v1 = b2 * v + w2 * (gv * gv)
        if kind == "eps inside the root":
            denom = (np.sqrt(v1) + eps) / bc2s
        elif kind == "eps dropped":
            denom = np.sqrt(v1) / bc2s
        else:
            denom = np.sqrt(v1) / bc2s + eps
        if kind == "decoupled decay":
            p = p - (T(hp["lr"]) * wd) * p
        return p - lr_c * (m1 / denom), m1, v1


def test_the_unmutated_formula_is_the_restatement():
    case = ref.single_case("lr3e-3_wd1e-2", 10)
    for sg in case["segs"]:
        want = ref.step(sg["p"], sg["m"], sg["v"], sg["g"], case["hp"], F32)
        with np.errstate(all="ignore"):
            T = F32
            w1, w2, b2, lr_c, bc2s, eps, wd = (T(x) for x in ref.scalars(case["hp"]))
            g = sg["g"] + wd * sg["p"]
            m1 = sg["m"] + w1 * (g - sg["m"])
            v1 = b2 * sg["v"] + w2 * (g * g)
            p1 = sg["p"] - lr_c * (m1 / (np.sqrt(v1) / bc2s + eps))
        for a, b in zip(want, (p1, m1, v1)):
            assert a.dtype == F32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _caught_by(kind, case, refs):
    """The first (segment, quantity, ratio) at which the mutant leaves the kernel's bound, or None."""
    for sg, r in zip(case["segs"], refs):
        p, m, v = _mutant(kind, sg["p"], sg["m"], sg["v"], sg["g"], case["hp"])
        for q, (d32, d) in ref.segment_deviations(sg, r, p, m, v).items():
            assert ref.within(d32, d32)                           # (the restatement itself always passes)
            if not ref.within(d, d32):
                return sg["label"], q, d / ref.yardstick(d32)
    return None


@pytest.mark.parametrize("kind", MUTANTS)
def test_every_mutant_is_caught(kind):
    hits = []
    for h in ref.HYPER:
        for t in ref.STEPS:
            hit = _caught_by(kind, ref.single_case(h, t), ref.single_reference(h, t))
            if hit:
                hits.append((f"{h}/t{t}",) + hit)
    geom = _caught_by(kind, ref.geometry_case(ref.GEOM_LENS_32), ref.geometry_reference(ref.GEOM_LENS_32))
    print(f"ADAM-CPU mutant '{kind}': caught by {len(hits)} of {len(ref.HYPER) * len(ref.STEPS)} single-step cases"
          f"{', by the 32-segment case' if geom else ''}; first: {hits[0] if hits else None}")
    assert hits, kind
    if kind == "float weights":     # the deviation the kernel carried: every first step with beta2 = 0.999 sees it in v
        first = {h: _caught_by(kind, ref.single_case(h, 1), ref.single_reference(h, 1)) for h in ref.HYPER}
        for h, hit in first.items():
            if ref.HYPER[h]["beta2"] == 0.999:
                assert hit and hit[1] == "v" and hit[2] > 40, (h, hit)


def test_the_chain_catches_the_float_weights():
    c = ref.chain_case()
    c64, c32 = ref.chain_reference()
    p, m, v = c["p"], np.zeros_like(c["p"]), np.zeros_like(c["p"])
    ratios = []
    for k, g in enumerate(c["grads"]):
        p, m, v = _mutant("float weights", p, m, v, g, dict(c["hp"], step=k + 1, lr=c["lrs"][k]))
        ratios.append(ref.deviation("v", v, c64[k][2]) / ref.yardstick(ref.deviation("v", c32[k][2], c64[k][2])))
    print("ADAM-CPU chain, v of the float-weights mutant in yardsticks: first %.1f, last %.1f" % (ratios[0], ratios[-1]))
    assert min(ratios) > ref.MARGIN


# ------------------------------------------------------------------ the refusals, as the header lists them
def test_refusal_table_matches_the_restatement_and_the_header():
    good = dict(dict(ref.HYPER["workload"], step=3), bias_correction1=1 - 0.9 ** 3, bias_correction2=1 - 0.999 ** 3)
    ref.check(3, ref.REFUSAL_LENS, (0, 257, 300), good)
    ref.check(32, [0] * 32, [0] * 32, good, null_param=range(32))          # len 0: whatever the pointer
    names = dict(weight_decay="wd")
    for rid, field, change in ref.REFUSALS:
        n, lens, offs, hp, kw = 3, list(ref.REFUSAL_LENS), [0, 257, 300], dict(good), {}
        for k, val in change.items():
            if k == "n":
                n = val
            elif k in ("grad", "exp_avg", "exp_avg_sq"):
                kw["null_flat"] = True
            elif k == "param":
                kw["null_param"] = (val[0],)
            elif k == "len":
                lens[val[0]] = val[1]
            elif k == "offset":
                offs[val[0]] = val[1]
            else:
                hp[names.get(k, k)] = val
        with pytest.raises(ValueError):
            ref.check(n, lens + [0] * 30, offs + [0] * 30, hp, **kw)
    header = open(os.path.join(ROOT, "include", "meshdqn_hip.h")).read()
    comment = header[:header.index("typedef struct mdq_adam_desc")].rsplit("/*", 1)[1]
    for field in sorted({f for _, f, _ in ref.REFUSALS}):
        assert re.search(r"\b" + field + r"\b", comment), field
    assert "formed in double" in comment and "rounded once" in comment
    assert len({rid for rid, _, _ in ref.REFUSALS}) == len(ref.REFUSALS)
