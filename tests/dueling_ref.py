"""fp64 reference of the "linear" and "dueling" Q-heads of `NodeRemovalNet` (test helper, numpy only), on top of
tests/gcn_ref64.py as it stands, and the dueling versions of the case families of tests/gcn_train_cases.py.

The dueling head is two linear maps of the same 64 values, so the reference runs `gcn_ref64.forward_graph(...,
softmax=False)` on a state dict whose `lin3` has `lin_v`'s row appended: the OUT + 1 outputs are the advantages A and
the value v, and q_c = v + (A_c - mean A) (the mean a sequential sum divided once by OUT).  The backward hands
`gcn_ref64.backward_graph` the matching gradient of the OUT + 1 outputs - dq_c - mean(dq) for the advantage rows,
sum(dq) for the value row - and splits the `lin3` gradients back.

The families: networks, graphs and launches of T-A, T-B, T-E32 and T-E256 (`gcn_train_cases.family`) with a seeded
`lin_v` added.  The embedding path does not depend on the head, so every TopK, relu and readout decision is the one the
existing families hold at KINK yardsticks; the head's one decision, the mode-1 argmax, is asserted by
test_dueling_head_cpu.py.
"""
import functools

import numpy as np
import torch

import gcn_path_cases as cases
import gcn_ref64 as ref
import gcn_train_cases as tc

HEADS = ("softmax", "linear", "dueling")
FAMILIES = ("T-A", "T-B", "T-E32", "T-E256")
MARGIN = tc.MARGIN
EPS32 = float(np.finfo(np.float32).eps)


# ------------------------------------------------------------------ the heads
def extended_sd(sd):
    """The state dict with `lin_v`'s row appended to `lin3` (and without `lin_v`)."""
    out = {k: v for k, v in sd.items() if not k.startswith("lin_v.")}
    out["lin3.weight"] = np.concatenate([ref._arr(sd["lin3.weight"], np.float64), ref._arr(sd["lin_v.weight"], np.float64)])
    out["lin3.bias"] = np.concatenate([ref._arr(sd["lin3.bias"], np.float64), ref._arr(sd["lin_v.bias"], np.float64)])
    return out


def aggregate(raw, dtype):
    """q = v + (A - mean A) from the OUT + 1 outputs [A, v], in `dtype`."""
    dt = np.dtype(dtype).type
    adv, v = raw[:-1], raw[-1]
    s = dt(0)
    for c in range(len(adv)):
        s = s + adv[c]
    return (v + (adv - s / dt(len(adv)))).astype(dt)


def _finish(res, head, dtype):
    if head == "dueling":
        res["raw"] = res["out"]
        res["out"] = aggregate(res["raw"], dtype)
    return res


def _sd_of(sd, head):
    return extended_sd(sd) if head == "dueling" else sd


def forward_graph(sd, levels, x, edge_index, ratio, head, dtype=np.float64, forced_perm=None):
    """`gcn_ref64.forward_graph` for a network with `head`: `out` holds the graph's q row (dueling: `raw` the OUT + 1
    outputs [A, v] it was formed from)."""
    res = ref.forward_graph(_sd_of(sd, head), levels, x, edge_index, ratio, head == "softmax", dtype, forced_perm)
    return _finish(res, head, dtype)


def head_of_embedding(sd, emb, head, dtype=np.float64):
    """The q row of a graph from its embedding alone (what the head kernels compute)."""
    dt = np.dtype(dtype).type
    res = dict(out=ref.head(ref._arr(emb, dt), _sd_of(sd, head), head == "softmax", dt))
    return _finish(res, head, dtype)["out"]


def backward_graph(sd, levels, res, dq, head, dtype=np.float64):
    """Gradient of every parameter of the network (`lin_v` included) for the run `res`, given d loss / d q."""
    dt = np.dtype(dtype).type
    dq = ref._arr(dq, dt)
    if head != "dueling":
        return ref.backward_graph(sd, levels, res, dq, head == "softmax", dtype)
    s = dt(0)
    for c in range(len(dq)):
        s = s + dq[c]
    dout = np.concatenate([dq - s / dt(len(dq)), [s]]).astype(dt)
    run = dict(res, out=res["raw"])
    grads, amax = ref.backward_graph(extended_sd(sd), levels, run, dout, False, dtype)
    w, b = grads["lin3.weight"], grads["lin3.bias"]
    grads["lin3.weight"], grads["lin_v.weight"] = w[:-1], w[-1:]
    grads["lin3.bias"], grads["lin_v.bias"] = b[:-1], b[-1:]
    return grads, amax


def learning_step_graph(sd, levels, res, head, mode, action, reward, nonfinal, gamma, q_other, B, weight=None, dtype=np.float64):
    """`gcn_ref64.learning_step_graph` for a network with `head`."""
    term, td, dq = ref.loss_graph(res["out"], mode, action, reward, nonfinal, gamma, q_other, B, weight, dtype)
    grads, amax = backward_graph(sd, levels, res, dq, head, dtype)
    return dict(term=term, td=td, grads=grads, amax=amax)


# ------------------------------------------------------------------ networks
def seeded_sd(sd, seed):
    """`sd` (a family's) with a seeded `lin_v` in the families' scale, registered last."""
    rng = np.random.default_rng([seed, 64])
    out = dict(sd)
    out["lin_v.weight"] = torch.from_numpy(rng.standard_normal((1, 64)) * 0.3).float()
    out["lin_v.bias"] = torch.from_numpy(rng.standard_normal(1) * 0.3).float()
    return out


def network(kw, fin0, sd, head):
    from meshdqn_amd.airfoilgcnn import NodeRemovalNet
    net = NodeRemovalNet(**kw, head=head)
    net.set_num_nodes(fin0)
    net.load_state_dict(sd)
    return net


class HeadFamily:
    """A family of gcn_train_cases with another head: the same graphs, launches and embedding weights."""

    def __init__(self, name, head, out_dim=None):
        base, r64, _, launches, _ = tc.family(name)
        self.name, self.head, self.base, self.launches = name, head, base, launches
        self.kw, self.fin0, self.levels, self.ratio, self.C = dict(base.kw), base.fin0, base.levels, base.ratio, base.C
        self.graphs, self.level_sizes = base.graphs, base.level_sizes
        sd = dict(base.sd)
        if out_dim is not None:     # another number of outputs: the first rows of the family's lin3
            self.kw["output_dim"] = out_dim
            sd["lin3.weight"], sd["lin3.bias"] = sd["lin3.weight"][:out_dim].clone(), sd["lin3.bias"][:out_dim].clone()
        self.out_dim = self.kw["output_dim"]
        self.sd = seeded_sd(sd, tc.SPECS[name][3]) if head == "dueling" else sd
        self.net = network(self.kw, self.fin0, self.sd, head)
        # free-running fp64 runs (the family's own selections: the embedding path is the family's) and the fp32 yardstick runs
        self.r64 = [forward_graph(self.sd, self.levels, x, ei, self.ratio, head, np.float64) for x, ei in self.graphs]
        self.r32 = [forward_graph(self.sd, self.levels, x, ei, self.ratio, head, np.float32, r["perm"])
                    for (x, ei), r in zip(self.graphs, self.r64)]
        assert all(a["perm"] == b["perm"] for a, b in zip(self.r64, r64))


@functools.lru_cache(maxsize=None)
def family(name, head="dueling", out_dim=None):
    return HeadFamily(name, head, out_dim)


def first_max_of(res):
    """Index of the first maximum of a run's q row (the mode-1 decision)."""
    return ref.first_max(res["out"])


def argmax_gaps(fam):
    """Per graph (gap between the two largest lin3 outputs in fp64 - what the mode-1 first maximum of q hangs on, v is
    common to the row -, fp32 yardstick of q: largest |fp32 q - fp64 q| of the graph)."""
    out = []
    for a, b in zip(fam.r64, fam.r32):
        adv = np.sort(a["raw"][:-1] if fam.head == "dueling" else a["out"])
        out.append((float(adv[-1] - adv[-2]), tc._absdev(b["out"], a["out"])))
    return out


# ------------------------------------------------------------------ transition data, learning steps, yardsticks
def transitions(fam, mode, li):
    """The scheme of `gcn_train_cases.transitions` for a q head: the other network's rows are plain values (no
    probabilities), the rewards are picked from the fp64 q so that the TD error lands on the wanted Huber branch."""
    la = fam.launches[li]
    B, OUT = len(la.idx), fam.out_dim
    rng = np.random.default_rng([sum(map(ord, fam.name)), mode, li, 7])
    qo = rng.standard_normal((B, OUT)).astype(np.float32)
    action, reward, nonfinal, weight, want = [], [], [], [], []
    for b, g in enumerate(la.idx):
        out = fam.r64[g]["out"]
        a = (0, OUT - 1, int(rng.integers(0, OUT)))[(b + li) % 3]
        nf = 0.0 if b % 4 == 1 else 1.0
        d = tc.DIFFS[(b + mode) % 3]
        if mode == 0:
            r = float(out[a]) - la.gamma * nf * float(qo[b].max()) - d
        else:
            r = float(qo[b, a]) - la.gamma * nf * float(out.max()) - d
        action.append(a), reward.append(r), nonfinal.append(nf), weight.append(tc.WEIGHTS[(b + b // 4) % 4]), want.append(d)
    return dict(action=np.asarray(action, dtype=np.int64), reward=np.asarray(reward, dtype=np.float32),
                nonfinal=np.asarray(nonfinal, dtype=np.float32), weight=np.asarray(weight, dtype=np.float32),
                q_other=qo, want=np.asarray(want))


@functools.lru_cache(maxsize=None)
def steps(fam, mode, weighted):
    """Per launch [(fp64 learning step, fp32 learning step forced to the fp64 selection) per graph]."""
    out = []
    for li, la in enumerate(fam.launches):
        t = transitions(fam, mode, li)
        rows = []
        for b, g in enumerate(la.idx):
            w = float(t["weight"][b]) if weighted else None
            args = (fam.head, mode, int(t["action"][b]), t["reward"][b], t["nonfinal"][b], la.gamma, t["q_other"][b], len(la.idx), w)
            rows.append((learning_step_graph(fam.sd, fam.levels, fam.r64[g], *args, np.float64),
                         learning_step_graph(fam.sd, fam.levels, fam.r32[g], *args, np.float32)))
        out.append(rows)
    return out


@functools.lru_cache(maxsize=None)
def yardsticks(fam):
    """`gcn_train_cases.yardsticks` for the family with its head: `out` in units of the graph's largest |q|
    (`gcn_path_cases._norm_dev`), `td` and `loss` absolute, `grad` per parameter in `gcn_train_cases.grad_dev` units."""
    y = dict(out=max(cases._norm_dev(a["out"], b["out"]) for a, b in zip(fam.r32, fam.r64)), td=0.0, loss=0.0,
             grad={k: 0.0 for k in fam.sd})
    for mode in (0, 1):
        for weighted in (False, True):
            for rows in steps(fam, mode, weighted):
                l64, l32 = 0.0, np.float32(0)
                for s64, s32 in rows:
                    y["td"] = max(y["td"], abs(float(s32["td"]) - float(s64["td"])))
                    l64, l32 = l64 + float(s64["term"]), l32 + s32["term"]
                    for k, g in s64["grads"].items():
                        if g is not None and np.any(g):
                            y["grad"][k] = max(y["grad"][k], tc.grad_dev(s32["grads"][k], s64["grads"], k))
                y["loss"] = max(y["loss"], abs(float(l32) - l64))
    return y
