"""Numpy restatement of `mdq_adam_step` (include/meshdqn_hip.h), written from the header's text and not from the kernel, the
bound the kernel is held to, and the case tables of test_adam_step_cpu.py / test_adam_step_gpu.py.

    g' = g + wd p  (only if wd != 0);   m' = m + w1 (g' - m);   v' = b2 v + w2 (g' g');
    p' = p - (lr / bc1) (m' / (sqrt(v') / sqrt(bc2) + eps))

w1 = 1 - beta1, w2 = 1 - beta2, bc1 = 1 - beta1^step, bc2 = 1 - beta2^step, lr / bc1 and sqrt(bc2) are formed in double.  With
dtype = float64 this is the reference; with dtype = float32 every scalar is rounded ONCE to float32 and every elementwise
operation is rounded on its own (no fused multiply-add): the yardstick run.  Everything below is generated from fixed seeds, so
the CPU and the GPU file see the same numbers."""
import functools
import math

import numpy as np

PACK_MAX = 32                                   # MDQ_GCN_PACK_MAX
STRIDE = 32 * 256                               # elements one pass of a segment's 32 workgroups covers
EPS32 = float(np.finfo(np.float32).eps)         # 2^-23
MARGIN = 4.0                                    # what the kernel gets, in fp32 yardsticks (as tests/gcn_train_cases.py)


# ------------------------------------------------------------------ the restatement
def scalars(hp):
    """The doubles of one step: (w1, w2, b2, lr / bc1, sqrt(bc2), eps, wd)."""
    b1, b2, t = float(hp["beta1"]), float(hp["beta2"]), float(hp["step"])
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    return 1.0 - b1, 1.0 - b2, b2, float(hp["lr"]) / bc1, math.sqrt(bc2), float(hp["eps"]), float(hp["wd"])


def bias_corrections(hp):
    """What the caller of mdq_adam_step puts into the descriptor."""
    t = float(hp["step"])
    return 1.0 - float(hp["beta1"]) ** t, 1.0 - float(hp["beta2"]) ** t


def step(p, m, v, g, hp, dtype, trace=None):
    """-> (p', m', v') in `dtype`.  `trace`: a dict that receives every intermediate of the run."""
    T = np.dtype(dtype).type
    w1, w2, b2, lr_c, bc2s, eps, wd = (T(x) for x in scalars(hp))
    p, m, v, g = (np.asarray(a, dtype=T) for a in (p, m, v, g))
    with np.errstate(all="ignore"):
        if wd != 0:
            decay = wd * p
            g = g + decay
        diff = g - m
        m_inc = w1 * diff
        m1 = m + m_inc
        gg = g * g
        v_old = b2 * v
        v_inc = w2 * gg
        v1 = v_old + v_inc
        root = np.sqrt(v1)
        hat = root / bc2s
        denom = hat + eps
        quot = m1 / denom
        upd = lr_c * quot
        p1 = p - upd
    if trace is not None:
        trace.update(g=g, diff=diff, m_inc=m_inc, m=m1, gg=gg, v_old=v_old, v_inc=v_inc, v=v1, root=root, hat=hat, denom=denom,
                     quot=quot, upd=upd, p=p1)
        if wd != 0:
            trace["decay"] = decay
    return p1, m1, v1


def chain(p, m, v, grads, hp, dtype, first_step=1, lrs=None):
    """K = len(grads) steps with the state fed back and `step` counting up from `first_step`; `lrs[k]` replaces hp["lr"] in
    step k.  -> the list of (p, m, v) after every step."""
    out = []
    for k, g in enumerate(grads):
        h = dict(hp, step=first_step + k)
        if lrs is not None:
            h["lr"] = lrs[k]
        p, m, v = step(p, m, v, g, h, dtype)
        out.append((p, m, v))
    return out


def check(n, lens, offsets, hp, null_flat=False, null_param=()):
    """What mdq_adam_step refuses before any launch, as a ValueError that names the field."""
    if not 1 <= n <= PACK_MAX:
        raise ValueError("n outside 1 .. 32")
    if null_flat:
        raise ValueError("grad / exp_avg / exp_avg_sq is NULL")
    for s in range(n):
        if int(lens[s]) < 0:
            raise ValueError("negative len")
        if int(offsets[s]) < 0:
            raise ValueError("negative offset")
        if int(offsets[s]) + int(lens[s]) > 2 ** 31 - 1:
            raise ValueError("offset + len beyond int32")
        if int(lens[s]) > 0 and s in null_param:
            raise ValueError("param is NULL")
    for k in ("lr", "eps", "wd"):
        if not (math.isfinite(hp[k]) and hp[k] >= 0.0):
            raise ValueError(k + " must be finite and not negative")
    for k in ("beta1", "beta2"):
        if not 0.0 <= hp[k] < 1.0:
            raise ValueError(k + " outside [0, 1)")
    for k in ("bias_correction1", "bias_correction2"):
        if not 0.0 < hp[k] <= 1.0:
            raise ValueError(k + " outside (0, 1]")


# ------------------------------------------------------------------ the bound
def deviation(kind, got, want, before=None):
    """Deviation of one segment's `got` from the fp64 `want`, in the unit of its quantity: "v" elementwise relative where
    want > 0 (and `got` must be exactly 0 where want is 0), "m" in units of the segment's largest |want|, "p" in units of the
    segment's largest |want - before|.  A unit of 0 admits only want's own values; a NaN or a miss of an exact zero is inf."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return math.inf
    err = np.abs(got - want)
    if kind == "v":
        pos = want > 0
        if (got[~pos] != 0).any():
            return math.inf
        return float((err[pos] / want[pos]).max()) if pos.any() else 0.0
    unit = float(np.abs(want).max()) if kind == "m" else float(np.abs(want - np.asarray(before, np.float64)).max())
    if unit == 0.0:
        return 0.0 if not err.any() else math.inf
    return float(err.max() / unit)


def yardstick(dev32):
    """The fp32 restatement's own deviation, floored at one float32 epsilon."""
    return max(dev32, EPS32)


def within(dev, dev32):
    return dev <= MARGIN * yardstick(dev32)


# ------------------------------------------------------------------ case tables
BASE = dict(lr=1e-5, wd=1e-6, beta1=0.9, beta2=0.999, eps=1e-8)
HYPER = {
    "workload": dict(BASE),                                       # the trainer's defaults
    "lr3e-3_wd1e-2": dict(BASE, lr=3e-3, wd=1e-2),
    "wd0": dict(BASE, wd=0.0),
    "lr1e-8": dict(BASE, lr=1e-8),                                # after the three milestones
    "betas.5_.9": dict(BASE, lr=3e-3, wd=1e-2, beta1=0.5, beta2=0.9),
    "beta1_0": dict(BASE, beta1=0.0),
    "betas.9_.99": dict(BASE, lr=3e-3, wd=0.0, beta2=0.99),
    "eps1e-3": dict(BASE, eps=1e-3),
}
STEPS = (1, 2, 10, 1000, 2000000)
G_BANDS = (1e2, 1e-1, 1e-4, 1e-8, 0.0)          # |g| around ...; at 1e-8 sqrt(v^) is comparable to eps = 1e-8
P_BANDS = ("zero", "lr", 1.0, 1e3)              # |p| exactly 0, around lr, around 1, around 1e3
SEG_LEN = 300                                   # per (g band, p band) segment: more than one workgroup, no multiple of 256
PRE = 4                                         # steps of the fp64 chain that produce the state of a step > 1
CANCEL = 8.0                                    # (|g| + |wd p|) / |g + wd p| of any element of any case stays under this


def band(rng, scale, n):
    """n float32 values of either sign with |x| in [scale / 2, 2 scale); scale 0: exact zeros."""
    if scale == 0.0:
        return np.zeros(n, np.float32)
    return (scale * rng.uniform(0.5, 2.0, n) * rng.choice((-1.0, 1.0), n)).astype(np.float32)


def _state_before(rng, p, gscale, hp, t, n):
    """float32 (m, v) as `t - 1` steps would have left them: a constant gradient of the band for the first t - 1 - PRE steps
    (closed form), then PRE steps of the fp64 restatement with fresh gradients, p held."""
    if t == 1:
        return np.zeros(n, np.float32), np.zeros(n, np.float32)
    k = min(t - 1, PRE)
    s0 = t - 1 - k
    g0 = band(rng, gscale, n).astype(np.float64)
    if hp["wd"] != 0:
        g0 = g0 + hp["wd"] * p.astype(np.float64)
    m = (1.0 - hp["beta1"] ** s0) * g0
    v = (1.0 - hp["beta2"] ** s0) * g0 * g0
    for s in range(s0 + 1, t):
        _, m, v = step(p, m, v, band(rng, gscale, n), dict(hp, step=s), np.float64)
    return m.astype(np.float32), v.astype(np.float32)


@functools.lru_cache(maxsize=None)
def single_case(hname, t):
    """One launch: 20 segments, one per (g band, p band).  -> dict(name, hp, segs) with segs a list of dicts(label, p, m, v, g)
    of float32 arrays."""
    hp = dict(HYPER[hname], step=t)
    rng = np.random.default_rng([sorted(HYPER).index(hname), t])
    segs = []
    for gs in G_BANDS:
        for pb in P_BANDS:
            ps = 0.0 if pb == "zero" else hp["lr"] if pb == "lr" else pb
            p = band(rng, ps, SEG_LEN)
            m, v = _state_before(rng, p, gs, hp, t, SEG_LEN)
            g = band(rng, gs, SEG_LEN)
            if gs and 1.0 / CANCEL < hp["wd"] * ps / gs < CANCEL:
                # the bands of g and wd p overlap: opposite signs would make g' = g + wd p a cancelling sum, and an
                # elementwise relative error of v' = ... + w2 g'^2 is then whatever |wd p| / |g'| makes of ONE rounding (the
                # kernel may contract g + wd p into one fused multiply-add, the restatement rounds twice).  Same sign here.
                g = np.copysign(g, p)
            segs.append(dict(label=f"g{gs:g}/p{pb}", p=p, m=m, v=v, g=g))
    return dict(name=f"{hname}/t{t}", hp=hp, segs=segs)


def single_cases():
    return [single_case(h, t) for h in HYPER for t in STEPS]


GEOM_HP = dict(HYPER["lr3e-3_wd1e-2"], step=3)
GEOM_LENS_1 = (1, 255, 256, 257, 8191, 8192, 8193, 16385, 3 * 8192 + 77)
GEOM_LENS_32 = tuple((0, 1, 7, 256, 8193, 7, 1, 0)[s % 8] for s in range(32))


@functools.lru_cache(maxsize=None)
def geometry_case(lens):
    """Segments of the given lengths at step 3 of (lr 3e-3, wd 1e-2): |g| around 0.1, |p| around 1."""
    rng = np.random.default_rng([77, len(lens), sum(lens)])
    segs = []
    for s, n in enumerate(lens):
        p = band(rng, 1.0, n)
        m, v = _state_before(rng, p, 0.1, GEOM_HP, GEOM_HP["step"], n)
        segs.append(dict(label=f"s{s}/len{n}", p=p, m=m, v=v, g=band(rng, 0.1, n)))
    return dict(name="geom/" + ("n1/len%d" % lens[0] if len(lens) == 1 else "n%d" % len(lens)), hp=dict(GEOM_HP), segs=segs)


def scattered_layout(lens, seed=5):
    """Offsets into the flat buffers that are not monotone in s and leave gaps, as unused parameters do in the trainer.
    -> (offsets, total)."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(lens))
    off, cur = [0] * len(lens), 3
    for s in order:
        off[s] = cur
        cur += lens[s] + int(rng.choice((0, 1, 5, 64, 300)))
    return off, cur + 9


CHAIN_HP = dict(HYPER["lr3e-3_wd1e-2"])
CHAIN_K = 25
CHAIN_LENS = (8193, 7, 11800)
CHAIN_LRS = tuple(3e-3 * (0.1 if k >= 10 else 1.0) * (0.1 if k >= 20 else 1.0) for k in range(CHAIN_K))   # two milestones


@functools.lru_cache(maxsize=None)
def chain_case():
    """25 steps from zero state on 20 000 elements: |p0| around 1, a fresh |g| around 0.1 per step."""
    rng = np.random.default_rng(4242)
    n = sum(CHAIN_LENS)
    return dict(name="chain", hp=dict(CHAIN_HP), lens=CHAIN_LENS, lrs=CHAIN_LRS, p=band(rng, 1.0, n),
                grads=[band(rng, 0.1, n) for _ in range(CHAIN_K)])


def reference(case):
    """fp64 and fp32 runs of a single-launch case, per segment: list of dicts(p64, m64, v64, upd64, p32, m32, v32, trace32)."""
    out = []
    for sg in case["segs"]:
        t64, t32 = {}, {}
        p64, m64, v64 = step(sg["p"], sg["m"], sg["v"], sg["g"], case["hp"], np.float64, t64)
        p32, m32, v32 = step(sg["p"], sg["m"], sg["v"], sg["g"], case["hp"], np.float32, t32)
        out.append(dict(p64=p64, m64=m64, v64=v64, upd64=t64["upd"], p32=p32, m32=m32, v32=v32, trace32=t32))
    return out


@functools.lru_cache(maxsize=None)
def single_reference(hname, t):
    return reference(single_case(hname, t))


@functools.lru_cache(maxsize=None)
def geometry_reference(lens):
    return reference(geometry_case(lens))


@functools.lru_cache(maxsize=None)
def chain_reference():
    """-> (fp64 chain, fp32 chain): lists of (p, m, v) after every step, computed once."""
    c = chain_case()
    z = np.zeros_like(c["p"])
    return (chain(c["p"], z, z, c["grads"], c["hp"], np.float64, lrs=c["lrs"]),
            chain(c["p"], z, z, c["grads"], c["hp"], np.float32, lrs=c["lrs"]))


# (id, the field the refusal names, what to change in an accepted call of n = 3 segments with len 257, 0, 1)
NAN, INF = float("nan"), float("inf")
REFUSALS = (
    ("n=0", "n", dict(n=0)), ("n=-1", "n", dict(n=-1)), ("n=33", "n", dict(n=33)),
    ("grad=NULL", "grad", dict(grad=None)), ("exp_avg=NULL", "exp_avg", dict(exp_avg=None)),
    ("exp_avg_sq=NULL", "exp_avg_sq", dict(exp_avg_sq=None)),
    ("param[0]=NULL", "param", dict(param=(0, None))), ("param[2]=NULL", "param", dict(param=(2, None))),
    ("len[0]=-1", "len", dict(len=(0, -1))), ("len[1]=-1", "len", dict(len=(1, -1))), ("len[2]=-2^31", "len", dict(len=(2, -2 ** 31))),
    ("offset[0]=-1", "offset", dict(offset=(0, -1))), ("offset[1]=-4", "offset", dict(offset=(1, -4))),
    ("offset[2]=2^31-1", "offset", dict(offset=(2, 2 ** 31 - 1))),
    ("lr=-1e-5", "lr", dict(lr=-1e-5)), ("lr=nan", "lr", dict(lr=NAN)), ("lr=inf", "lr", dict(lr=INF)),
    ("eps=-1e-8", "eps", dict(eps=-1e-8)), ("eps=nan", "eps", dict(eps=NAN)), ("eps=inf", "eps", dict(eps=INF)),
    ("wd=-1e-6", "weight_decay", dict(weight_decay=-1e-6)), ("wd=nan", "weight_decay", dict(weight_decay=NAN)),
    ("wd=inf", "weight_decay", dict(weight_decay=INF)),
    ("beta1=-0.1", "beta1", dict(beta1=-0.1)), ("beta1=1", "beta1", dict(beta1=1.0)), ("beta1=nan", "beta1", dict(beta1=NAN)),
    ("beta2=-0.5", "beta2", dict(beta2=-0.5)), ("beta2=1", "beta2", dict(beta2=1.0)), ("beta2=1.5", "beta2", dict(beta2=1.5)),
    ("beta2=nan", "beta2", dict(beta2=NAN)),
    ("bc1=0", "bias_correction1", dict(bias_correction1=0.0)), ("bc1=-0.1", "bias_correction1", dict(bias_correction1=-0.1)),
    ("bc1=1.5", "bias_correction1", dict(bias_correction1=1.5)), ("bc1=nan", "bias_correction1", dict(bias_correction1=NAN)),
    ("bc2=0", "bias_correction2", dict(bias_correction2=0.0)), ("bc2=1+", "bias_correction2", dict(bias_correction2=1.0000001)),
    ("bc2=nan", "bias_correction2", dict(bias_correction2=NAN)),
)
REFUSAL_LENS = (257, 0, 1)


def segment_deviations(sg, r, p, m, v):
    """{"v" | "m" | "p": (deviation of the fp32 restatement, deviation of (p, m, v))} of one segment against its fp64 run."""
    return {"v": (deviation("v", r["v32"], r["v64"]), deviation("v", v, r["v64"])),
            "m": (deviation("m", r["m32"], r["m64"]), deviation("m", m, r["m64"])),
            "p": (deviation("p", r["p32"], r["p64"], sg["p"]), deviation("p", p, r["p64"], sg["p"]))}
