"""Case families of the learning-step path tests (helper of test_gcn_train_ref64_cpu.py and
test_gcn_train_paths_gpu.py), chosen by the fp64 reference of tests/gcn_ref64.py alone:

 * the limits of `mdq_gcn_train_step_weighted` and its `tape_layout` (meshdqn_amd/csrc/mdq_gcn_train.hip) restated in
   Python, so that every launch can be shown to be accepted and every refusal case to sit one step past the limit it
   names;
 * seeded networks and graphs that are DRAWN UNTIL NO DECISION IS CLOSE: the gradient of the learning step is
   discontinuous where a relu of a kept row, the first maximum of a readout column, a head relu, the mode-1 argmax or
   the TopK cut / order flips.  A candidate whose free-running fp64 run has any such decision closer than KINK = 16 x
   the fp32 yardstick of that quantity (fp32 run of the same reference, forced to the fp64 selection, against the fp64
   run) is rejected, deterministically.  16 is 4 x the margin the kernel gets, so a flip on the device is an error and
   the GPU comparison needs neither an exclusion rule nor a tie branch;
 * transition data that is chosen, not drawn blindly: every Huber branch (reward picked from the reference's output),
   terminal and non-terminal graphs, first and last action, the weights 0, 0.25, 1, 3.5, one launch with gamma = 0;
 * the fp64 / fp32 learning steps of every launch, computed once per family, and the fp32 yardsticks per parameter.
"""
import functools
import math

import numpy as np

import gcn_path_cases as cases
import gcn_ref64 as ref

WGT = cases.WGT
NACC = 24            # accumulators per thread of the feature-outer convolution (mdq_gcn.hip)
LDS_LIMIT = 160 * 1024
KINK = 16.0          # rejection distance of a decision, in fp32 yardsticks of its quantity
MARGIN = 4.0         # what the kernel gets, in fp32 yardsticks
MAX_REJECTED = 0.25  # share of a family's candidates that may be rejected
GAMMA = 0.9
WEIGHTS = (1.0, 0.25, 3.5, 0.0)
DIFFS = (0.3, 2.5, -1.7)          # |diff| < 1, diff > 1, diff < -1: wanted TD errors, the rewards follow from them


# ------------------------------------------------------------------ limits of the entry point, restated
def _ceil(ratio, n):
    return int(math.ceil(ratio * float(n)))


def xs_floats(fam, nmax):
    """`mdq_gcn_xs`: floats of the level-input / aggregation buffers."""
    return (max(nmax * fam.fin0, _ceil(fam.ratio, nmax) * fam.C) + 3) & ~3


def backward_head_floats(fam):
    outp = (fam.out_dim + 3) & ~3
    return 2 * fam.C + 128 + 64 + 2 * outp + 64 + 128 + WGT + 4


def lds_bytes(fam, nmax, emax):
    C, km = fam.C, _ceil(fam.ratio, nmax)
    floats = xs_floats(fam, nmax) * 2 + nmax * (C + 1) + nmax + max(nmax, C) + 2 * C + ((km + 3) & ~3)
    ints = nmax + 4 + 3 * (emax + 3) + nmax + 8 + WGT // 64
    return 4 * floats + 4 * ints + 16


def train_accepts(fam, nmax, emax):
    """None when `mdq_gcn_train_step_weighted` accepts a launch of this network with (NMAX, EMAX), else the name of the
    first limit that refuses it, in the order of the entry point's checks."""
    C = fam.C
    if C not in (32, 64, 128, 256):
        return "width"
    if fam.out_dim > 256:
        return "out_dim"
    if fam.fin0 > 32 and nmax > NACC * (WGT // C):
        return "wide-input"
    n = nmax
    for l in range(len(fam.levels)):
        fin = fam.fin0 if l == 0 else C
        if fin > 32 and n > NACC * (WGT // C):
            return "wide-level"
        n = _ceil(fam.ratio, n)
    km = _ceil(fam.ratio, nmax)
    if nmax * (C + 1) < 2 * km * C:
        return "backward-rows"
    if nmax * (C + 1) < backward_head_floats(fam):
        return "backward-head"
    if xs_floats(fam, nmax) < km * C:
        return "xs"
    if lds_bytes(fam, nmax, emax) > LDS_LIMIT:
        return "lds"
    return None


def tape_layout(fam, nmax, emax):
    """(floats of one graph's workspace, per level the offsets of hsel, ssel, aggsel, xsel, perm, amax, esrc, edst in
    4-byte units): slot 0 holds the graph's loss term, the tape of every level is sized for NMAX nodes / EMAX edges."""
    pos, n, offs = 4, nmax, []
    for l in range(len(fam.levels)):
        k, fin, C = _ceil(fam.ratio, n), (fam.fin0 if l == 0 else fam.C), fam.C
        o = {}
        for key, size in (("hsel", k * C), ("ssel", k), ("aggsel", k * fin), ("xsel", k * fin), ("perm", k), ("amax", C)):
            o[key] = pos
            pos += size
        o["esrc"] = o["edst"] = -1
        if l > 0:
            o["esrc"], o["edst"] = pos, pos + emax
            pos += 2 * emax
        offs.append(o)
        n = k
    return (pos + 3) & ~3, offs


def smallest_accepted_nmax(fam, emax):
    return next(n for n in range(1, 1024) if train_accepts(fam, n, emax) is None)


# ------------------------------------------------------------------ kinks
def _absdev(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max())


def level_yardsticks(r32, r64):
    """What fp32 arithmetic alone costs on one graph, per quantity a decision hangs on (largest absolute deviation of the
    fp32 run, forced to the fp64 selection, from the fp64 run): pre-activations, scores and pooled features per level,
    the head's pre-activations, the outputs."""
    nl = len(r64["pre"])
    return dict(pre=[_absdev(r32["pre"][l], r64["pre"][l]) for l in range(nl)],
                score=[_absdev(r32["score"][l], r64["score"][l]) for l in range(nl)],
                xp=[_absdev(r32["tape"][l]["xp"], r64["tape"][l]["xp"]) for l in range(nl)],
                head=[_absdev(a[1], b[1]) for a, b in zip(r32["head_tape"][:2], r64["head_tape"][:2])],
                out=_absdev(r32["out"], r64["out"]))


def kink_margins(r64, r32, ratio):
    """Every decision of the free-running fp64 run: [(what, level or layer, distance at which it flips, fp32 yardstick
    of the quantity it hangs on)] (distance inf where there is nothing to flip).  The yardsticks are the level's, except
    for the readout's maximum: a pooled feature is x' = h s, so its fp32 error is at most |s| Y(pre) + |h| Y(score) + one
    rounding of x', from the level's yardsticks Y of the pre-activations and the scores - entry by entry, because the
    columns that come close are those of small entries, far below the level's largest error.  Per level the column
    with the smallest distance in yardsticks is reported."""
    y = level_yardsticks(r32, r64)
    eps = float(np.finfo(np.float32).eps)
    out = []
    gaps = ref.score_gaps(r64, ratio)
    for l, pre in enumerate(r64["pre"]):
        perm, xp = r64["perm"][l], r64["tape"][l]["xp"]
        out.append(("relu", l, float(np.abs(pre[perm]).min()), y["pre"][l]))
        gap, yard = math.inf, y["xp"][l]
        if xp.shape[0] > 1:
            order = np.argsort(xp, axis=0, kind="stable")
            cols = np.arange(xp.shape[1])
            r1, r2 = order[-1], order[-2]                # rows of the two largest entries of every column
            v1, v2 = xp[r1, cols], xp[r2, cols]
            ent = (np.abs(r64["score"][l][perm])[:, None] * y["pre"][l] + np.maximum(pre[perm], 0.0) * y["score"][l]
                   + eps * np.abs(xp))
            yy = np.maximum(ent[r1, cols], ent[r2, cols])
            live = ~((v1 == 0) & (v2 == 0))              # rows switched off by the relu: whichever is "first" gets nothing
            if live.any():
                c = int(np.argmin(np.where(live, (v1 - v2) / yy, np.inf)))
                gap, yard = float(v1[c] - v2[c]), float(yy[c])
        out.append(("readout-max", l, gap, yard))
        out.append(("topk-cut", l, gaps[l][0], y["score"][l]))
        out.append(("topk-order", l, gaps[l][1], y["score"][l]))
    for j, (_, z) in enumerate(r64["head_tape"][:2]):
        out.append(("head-relu", j, float(np.abs(z).min()), y["head"][j]))
    o = np.sort(r64["out"])
    out.append(("mode1-argmax", 0, float(o[-1] - o[-2]) if len(o) > 1 else math.inf, y["out"]))
    return out


def kink_violations(r64, r32, ratio, factor=KINK):
    """The decisions closer than `factor` x the fp32 yardstick of their quantity: [(what, level, distance, yardstick)]."""
    return [m for m in kink_margins(r64, r32, ratio) if not m[2] > factor * m[3]]


# ------------------------------------------------------------------ families
NRN = "NodeRemovalNet"
AIR = "AirfoilGCNN"

# name -> (class, kwargs, input features, seed of the weights, feature scale, [(nodes, kind)], launches)
# a launch: (graph numbers, NMAX or None: the largest graph / "min": the smallest NMAX the entry point accepts, gamma)
SPECS = {
    # level 0: form (c) from 16 rows on, (a)<17> below; no edges, one self loop, duplicates, a star (in-degree 2n)
    "T-A": (NRN, dict(output_dim=181, conv_width=128, topk=0.1), 17, 31, 0.1,
            [(1, "none"), (2, "selfloop"), (15, "star"), (16, "dup"), (17, "random"), (64, "none"), (180, "star"), (180, "random")],
            [(list(range(8)), None, GAMMA), ([0, 1, 1, 0], "min", 0.0)]),
    # first pooled level of 8 ... 18 rows; "dense": 16 n edges in a launch of EMAX 1024, the only graph of a ratio-0.1
    # family whose second level still has an edge into its kept row (with 2 n edges that level's edge list is nearly empty:
    # SAGEConv's backward along edges with an in-degree above 1 is the business of the ratio-0.5 families)
    "T-B": (NRN, dict(output_dim=181, conv_width=128, topk=0.1), 17, 32, 0.1,
            [(77, "random"), (85, "random"), (155, "random"), (163, "random"), (180, "random"), (180, "dup"), (64, "dense")],
            [(list(range(6)), None, GAMMA), ([0, 1], 180, 0.0), ([6, 2, 6, 4], None, GAMMA)]),
    # six levels, SAGE + GCN, one output, no softmax; levels of 2 and 1 rows
    "T-C": (AIR, dict(conv_width=128), 2, 33, 0.1,
            [(100, "random"), (66, "random"), (34, "random"), (33, "dup"), (17, "random"), (3, "random"), (1, "none"), (40, "random")],
            [(list(range(7)), None, GAMMA), ([4, 5, 6, 5], 100, 0.0), ([7, 7], None, GAMMA), ([7, 0], None, GAMMA)]),
    "T-D": (AIR, dict(conv_width=64), 2, 34, 0.3,
            [(180, "random"), (90, "random"), (37, "random"), (3, "random"), (37, "dup"), (3, "selfloop")],
            [(list(range(6)), None, GAMMA), ([3, 5, 2], 180, 0.0)]),
    # NMAX 41: the smallest the entry point accepts for this width (40 is refused by the backward-buffer check)
    "T-E32": (NRN, dict(output_dim=181, conv_width=32, topk=0.5), 17, 35, 0.1,
              [(41, "random"), (40, "random"), (17, "random"), (9, "random"), (17, "dup"), (9, "star")],
              [(list(range(6)), "min", GAMMA), ([3, 5], "min", 0.0)]),
    # NMAX 40: 2 KM C = 10 240 of the 10 280 floats of the conv-output area
    "T-E256": (NRN, dict(output_dim=181, conv_width=256, topk=0.5), 17, 36, 0.1,
               [(40, "random"), (17, "random"), (9, "random"), (17, "star"), (9, "dup"), (5, "random")],
               [(list(range(6)), 40, GAMMA), ([3, 5], 40, 0.0)]),
    # 40 input features: NMAX 96 = NACC WGT / C is the wide-input limit
    "T-F40": (NRN, dict(output_dim=181, conv_width=128, topk=0.1), 40, 37, 0.1,
              [(30, "random"), (9, "random"), (30, "dup"), (9, "star"), (96, "random")],
              [([0, 1, 2, 3], None, GAMMA), ([4, 0, 2, 1], None, GAMMA), ([1, 3], 30, 0.0)]),
}
FAMILIES = tuple(SPECS)

# forms every family has to reach in its launches (a change of the dispatch that empties one shows).  The in-level form
# of the pooling norms needs NMAX (C + 1) < levels x C floats, which the backward-buffer check of the learning step
# refuses for every width: the training instance always takes the norms from `pool_norms`.
EXPECTED_FORMS = {
    "T-A": {"c", "a<17>", "norms:pre", "b<1>", "b<5>", "head:c128-t16"},
    "T-B": {"c", "b<1>", "b<5>", "d:sage:0x16+9", "d:sage:1x16+0", "d:sage:1x16+1", "d:sage:1x16+2"},
    "T-C": {"c", "a<2>", "b<8>:r0-loop", "b<5>", "b<1>", "d:sage:1x16+1", "d:sage:0x16+9", "d:gcn:0x16+13", "d:gcn:0x16+9"},
    "T-D": {"a<2>", "b<8>", "b<8>:r0-loop", "d:sage:1x16+3", "d:gcn:0x16+12", "head:generic"},
    "T-E32": {"a<17>", "a<0>", "head:generic"},
    "T-E256": {"a<17>", "b<8>:r0-loop", "b<5>", "b<1>", "head:generic"},
    "T-F40": {"b<8>", "b<8>:r0-loop", "d:sage:0x16+9", "d:sage:1x16+14"},
}

# refusals at the entry: name -> (family whose network is launched or a spec of its own, NMAX, EMAX, the limit it names,
# the accepted neighbour (NMAX) or None where the limit is not one of size)
REFUSALS = {
    "E32 at NMAX 40": ("T-E32", 40, 128, "backward-head", 41),
    "conv width 48": ((NRN, dict(output_dim=181, conv_width=48, topk=0.5), 17), 64, 128, "width", None),
    "300 outputs": ((NRN, dict(output_dim=300, conv_width=128, topk=0.1), 17), 64, 128, "out_dim", None),
    "40 features at NMAX 97": ("T-F40", 97, 200, "wide-input", 96),
    "six levels of 128 at NMAX 180": ("T-C", 180, 360, "lds", None),
}


def draw_graph(rng, n, fin, kind, scale):
    """The kinds of `gcn_path_cases._graph` and "dense": 16 n random edges."""
    x, ei = cases._graph(rng, n, fin, "random" if kind == "dense" else kind, scale)
    if kind == "dense":
        ei = rng.integers(0, n, size=(2, 16 * n)).astype(np.int64)
    return x, ei


class Launch:
    def __init__(self, idx, nmax, emax, gamma):
        self.idx, self.nmax, self.emax, self.gamma = idx, nmax, emax, gamma


def _network(cls, kw, fin0, seed, name="net"):
    return cases.Family(name, cls, kw, fin0, [], [], seed)


@functools.lru_cache(maxsize=None)
def refusal_network(name):
    who = REFUSALS[name][0]
    return family(who)[0] if isinstance(who, str) else _network(*who, 99, name)


@functools.lru_cache(maxsize=None)
def family(name):
    """(family with its accepted graphs, free-running fp64 runs, fp32 runs forced to the fp64 selections, launches,
    draw statistics dict(candidates, rejected, log))."""
    cls, kw, fin0, seed, scale, slots, launches = SPECS[name]
    fam = _network(cls, kw, fin0, seed, name)
    r64, r32, log, cand = [], [], [], 0
    for slot, (n, kind) in enumerate(slots):
        for attempt in range(64):
            cand += 1
            rng = np.random.default_rng([seed, slot, attempt])
            x, ei = draw_graph(rng, n, fin0, kind, scale)
            a = ref.forward_graph(fam.sd, fam.levels, x, ei, fam.ratio, fam.softmax, np.float64)
            b = ref.forward_graph(fam.sd, fam.levels, x, ei, fam.ratio, fam.softmax, np.float32, a["perm"])
            bad = kink_violations(a, b, fam.ratio)
            if not bad:
                break
            log.append((slot, attempt, bad))
        else:
            raise RuntimeError(f"family {name} slot {slot}: no candidate without a close decision")
        fam.graphs.append((x, ei))
        r64.append(a)
        r32.append(b)
    out = []
    for idx, nmax, gamma in launches:
        emax = max(max(fam.graphs[g][1].shape[1] for g in idx), 1)
        if nmax is None:
            nmax = max(len(fam.graphs[g][0]) for g in idx)
        elif nmax == "min":
            nmax = smallest_accepted_nmax(fam, emax)
        out.append(Launch(list(idx), nmax, emax, gamma))
    fam.batches = [l.idx for l in out]
    return fam, r64, r32, out, dict(candidates=cand, rejected=cand - len(slots), log=log)


def launch_forms(fam, launch):
    forms = {cases.head_form(fam.C, fam.out_dim), cases.norms_form(fam.C, len(fam.levels), launch.nmax)}
    for g in launch.idx:
        forms.update(fam.forms(g, launch.nmax))
    return forms


def all_forms(name):
    fam, _, _, launches, _ = family(name)
    out = set()
    for la in launches:
        out |= launch_forms(fam, la)
    return out


# ------------------------------------------------------------------ transition data
def transitions(name, mode, li):
    """Chosen transition data of launch `li` in `mode`: dict of (B,) arrays action (int64), reward, nonfinal, weight
    (float32), q_other (B, out) float32 and, for the record, the wanted TD error of every graph.  The reward is picked
    from the fp64 reference's output so that the TD error lands on the wanted Huber branch."""
    fam, r64, _, launches, _ = family(name)
    la = launches[li]
    B, OUT = len(la.idx), fam.out_dim
    rng = np.random.default_rng([sum(map(ord, name)), mode, li])
    qo = rng.standard_normal((B, OUT))
    if fam.softmax:                                   # a probability row, like the other network's output
        qo = np.exp(qo)
        qo = qo / qo.sum(axis=1, keepdims=True)
    qo = qo.astype(np.float32)
    action, reward, nonfinal, weight, want = [], [], [], [], []
    for b, g in enumerate(la.idx):
        out = r64[g]["out"]
        a = (0, OUT - 1, int(rng.integers(0, OUT)))[(b + li) % 3]
        nf = 0.0 if b % 4 == 1 else 1.0
        d = DIFFS[(b + mode) % 3]
        if mode == 0:
            r = float(out[a]) - la.gamma * nf * float(qo[b].max()) - d
        else:
            r = float(qo[b, a]) - la.gamma * nf * float(out.max()) - d
        action.append(a), reward.append(r), nonfinal.append(nf), weight.append(WEIGHTS[(b + b // 4) % 4]), want.append(d)
    return dict(action=np.asarray(action, dtype=np.int64), reward=np.asarray(reward, dtype=np.float32),
                nonfinal=np.asarray(nonfinal, dtype=np.float32), weight=np.asarray(weight, dtype=np.float32),
                q_other=qo, want=np.asarray(want))


@functools.lru_cache(maxsize=None)
def steps(name, mode, weighted):
    """Per launch the learning step of every graph in fp64 and in fp32 (forced to the fp64 selection):
    [[(fp64 dict, fp32 dict), ...], ...] with the dicts of `gcn_ref64.learning_step_graph`."""
    fam, r64, r32, launches, _ = family(name)
    out = []
    for li, la in enumerate(launches):
        t = transitions(name, mode, li)
        rows = []
        for b, g in enumerate(la.idx):
            w = float(t["weight"][b]) if weighted else None
            args = (fam.softmax, mode, int(t["action"][b]), t["reward"][b], t["nonfinal"][b], la.gamma, t["q_other"][b], len(la.idx), w)
            rows.append((ref.learning_step_graph(fam.sd, fam.levels, r64[g], *args, np.float64),
                         ref.learning_step_graph(fam.sd, fam.levels, r32[g], *args, np.float32)))
        out.append(rows)
    return out


def grad_unit(grads, name):
    """The unit a parameter's deviation is measured in: its own largest gradient, but not less than 1e-3 of the
    largest gradient of any parameter of the graph."""
    top = max(float(np.abs(g).max()) for g in grads.values() if g is not None)
    return max(float(np.abs(grads[name]).max()), 1e-3 * top)


def grad_dev(g, grads64, name):
    """Largest |g - fp64 gradient| of parameter `name` in its unit (0 where the whole graph has no gradient)."""
    unit = grad_unit(grads64, name)
    return 0.0 if unit == 0.0 else float(np.abs(np.asarray(g, dtype=np.float64) - grads64[name]).max()) / unit


@functools.lru_cache(maxsize=None)
def yardsticks(name):
    """The family's fp32 yardsticks, the largest over both modes, weighted or not, every launch and graph:
    `out` (in units of the graph's largest |out|), `td` and `loss` (absolute), `grad` {parameter: in its unit}."""
    fam, r64, r32, launches, _ = family(name)
    y = dict(out=max(cases._norm_dev(a["out"], b["out"]) for a, b in zip(r32, r64)), td=0.0, loss=0.0,
             grad={k: 0.0 for k in fam.sd})
    for mode in (0, 1):
        for weighted in (False, True):
            for rows in steps(name, mode, weighted):
                l64, l32 = 0.0, np.float32(0)
                for s64, s32 in rows:
                    y["td"] = max(y["td"], abs(float(s32["td"]) - float(s64["td"])))
                    l64, l32 = l64 + float(s64["term"]), l32 + s32["term"]
                    for k, g in s64["grads"].items():
                        if g is not None:
                            y["grad"][k] = max(y["grad"][k], grad_dev(s32["grads"][k], s64["grads"], k))
                y["loss"] = max(y["loss"], abs(float(l32) - l64))
    return y


def param_class(key):
    """The class a parameter's figures are reported under: conv weight, conv bias, pool weight or head."""
    if key.startswith("pool"):
        return "pool weight"
    if key.startswith("lin"):
        return "head"
    return "conv bias" if key.endswith("bias") else "conv weight"
