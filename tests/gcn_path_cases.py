"""Case families of the Q-forward path tests (helper of test_gcn_ref64_cpu.py and test_gcn_paths_gpu.py): seeded
networks and graphs, the dispatch conditions of `run_level` (meshdqn_amd/csrc/mdq_gcn.hip) restated in Python so that
every test can name the forms its cases reach, and the fp64 / fp32 reference runs, computed once per family."""
import functools
import math

import numpy as np
import torch

import gcn_ref64 as ref

WGT = 512            # threads of gcn_embed_kernel (MDQ_GCN_WG)
FORMC_MAXFIN = 32    # MDQ_GCN_FORMC_MAXFIN
CAP = 0.10           # share of a family's graphs that may sit on a near-tie


# ------------------------------------------------------------------ dispatch conditions, restated
def level_form(C, conv_type, fin, n, nmax):
    """The dense form `run_level` picks for a level with `n` rows in a batch launched with `nmax` (weights of torch
    allocations: 64-byte aligned; L.h is 16-byte aligned because the level buffers are whole quads)."""
    G = WGT // C
    if C == 16 * (WGT // 64) and n >= 16 and fin <= FORMC_MAXFIN:
        return "c"
    if fin <= 32:
        return "a<%d>" % (fin if fin in (17, 2) else 0)
    kp = 2 * fin if conv_type == "sage" else fin
    stage = ((n + 15) >> 4) * 64 * ((kp >> 2) + 4)
    if (8 < n <= 32 and C % 16 == 0 and fin % (8 if conv_type == "sage" else 16) == 0
            and ((n * (C + 1) + 3) & ~3) + stage <= nmax * (C + 1)):
        return "d:%s:%dx16+%d" % (conv_type, n // 16, n % 16)
    per = (n + G - 1) // G
    return "b<%d>" % (1 if per <= 1 else 5 if per <= 5 else 8) + (":r0-loop" if per > 8 else "")


def head_form(C, out_dim):
    return "head:c128-t16" if C == 128 and out_dim <= 256 else "head:generic"


def norms_form(C, nlevels, nmax):
    return "norms:pre" if nlevels <= 7 and nmax * (C + 1) >= nlevels * ((C + 3) & ~3) else "norms:in-level"


class Family:
    """A network, its graphs and the batches (lists of graph numbers, one kernel launch each) they run in."""

    def __init__(self, name, cls, kw, fin0, graphs, batches, seed):
        from meshdqn_amd import airfoilgcnn as prod
        from meshdqn_amd.gcn_fused import _levels_of
        self.name, self.cls, self.kw, self.fin0, self.graphs, self.batches = name, cls, kw, fin0, graphs, batches
        net = getattr(prod, cls)(**kw)
        if cls == "NodeRemovalNet":
            net.set_num_nodes(fin0)
        rng = np.random.default_rng(seed)
        sd = {k: torch.from_numpy(rng.standard_normal(tuple(v.shape)) * 0.3).float() for k, v in net.state_dict().items()}
        net.load_state_dict(sd)
        self.net, self.sd = net, sd
        mods, self.softmax = _levels_of(net)
        names = {id(m): k for k, m in net.named_modules()}
        self.levels = [(names[id(c)], names[id(p)]) for c, p in mods]
        self.types = ["sage" if c + ".lin_l.weight" in sd else "gcn" for c, _ in self.levels]
        self.ratio = float(mods[0][1].ratio)
        self.C = kw.get("conv_width", 64)
        self.out_dim = sd["lin3.weight"].shape[0]

    def level_sizes(self, n):
        out = []
        for _ in self.levels:
            out.append(n)
            n = int(math.ceil(self.ratio * n))
        return out

    def forms(self, g, nmax):
        """Forms graph `g` reaches in a launch with `nmax`: one per level."""
        fins = [self.fin0] + [self.C] * (len(self.levels) - 1)
        return [level_form(self.C, t, f, n, nmax) for t, f, n in zip(self.types, fins, self.level_sizes(len(self.graphs[g][0])))]

    def nmax(self, batch):
        return max(len(self.graphs[g][0]) for g in batch)

    def all_forms(self):
        out = set()
        for b in self.batches:
            nm = self.nmax(b)
            out.add(norms_form(self.C, len(self.levels), nm))
            for g in b:
                out.update(self.forms(g, nm))
        out.add(head_form(self.C, self.out_dim))
        return out

    def run(self, dtype, forced=None):
        return ref.forward(self.sd, self.levels, self.graphs, self.ratio, self.softmax, dtype, forced)


def batch_arrays(graphs, idx):
    """Packed arrays of the C ABI for the graphs `idx`: x, node_ptr, esrc, edst, edge_ptr (numpy), nmax, emax."""
    xs = np.concatenate([graphs[g][0] for g in idx]).astype(np.float32)
    nn = [len(graphs[g][0]) for g in idx]
    ne = [graphs[g][1].shape[1] for g in idx]
    ei = np.concatenate([graphs[g][1] for g in idx], axis=1).astype(np.int32)
    ptr = lambda c: np.concatenate([[0], np.cumsum(c)]).astype(np.int32)  # noqa: E731
    return xs, ptr(nn), np.ascontiguousarray(ei[0]), np.ascontiguousarray(ei[1]), ptr(ne), max(nn), max(max(ne), 1)


# features 0.1 N(0, 1): with weights 0.3 N(0, 1) and features N(0, 1) the activations grow about fivefold per level and
# tanh saturates (scores of exactly 1.0f from the second level on: fp32 ties that fp64 does not have)
XSCALE = 0.1


def _graph(rng, n, fin, kind="random", scale=XSCALE):
    x = (scale * rng.standard_normal((n, fin))).astype(np.float32)
    ei = rng.integers(0, n, size=(2, 2 * n)).astype(np.int64)
    if kind == "none":
        ei = np.zeros((2, 0), dtype=np.int64)
    elif kind == "selfloop":
        ei = np.array([[n // 2], [n // 2]], dtype=np.int64)
    elif kind == "dup":
        ei = np.repeat(ei[:, :n], 2, axis=1)
    elif kind == "star":
        ei[1, :] = 0
    return x, ei


def _family(name):
    rng = np.random.default_rng(1000 + sum(map(ord, name)))
    nrn = dict(output_dim=181, conv_width=128, topk=0.1)
    if name == "A":     # level 0: form (c) from 16 rows on, (a)<17> below; launches of 180 and of 2 rows
        graphs = [_graph(rng, n, 17) for n in (1, 2, 15, 16, 17, 63, 64, 65, 128, 180) for _ in range(2)]
        graphs += [_graph(rng, 64, 17, kind="none"), _graph(rng, 17, 17, kind="selfloop"), _graph(rng, 65, 17, kind="dup"),
                   _graph(rng, 63, 17, kind="star"), _graph(rng, 15, 17, kind="star"), _graph(rng, 180, 17, kind="dup")]
        return Family(name, "NodeRemovalNet", nrn, 17, graphs, [list(range(len(graphs))), [0, 1, 2, 3]], 21)
    if name == "B":     # first pooled level: n1 = ceil(0.1 n) rows
        graphs = [_graph(rng, n, 17) for n in (7, 33, 47, 77, 85, 155, 163, 180) for _ in range(3)]
        return Family(name, "NodeRemovalNet", nrn, 17, graphs, [list(range(len(graphs)))], 22)
    if name == "C":
        graphs = [_graph(rng, n, 2) for n in (100, 96, 66, 34, 33, 17) for _ in range(2)]
        return Family(name, "AirfoilGCNN", dict(conv_width=128), 2, graphs, [list(range(len(graphs)))], 23)
    if name == "D":
        # (two input features through 64 channels: scores of a few 0.01 at scale 0.1, two of twelve graphs on a near-tie)
        graphs = [_graph(rng, n, 2, scale=0.3) for n in (180, 90, 37, 3) for _ in range(3)]
        return Family(name, "AirfoilGCNN", dict(conv_width=64), 2, graphs, [list(range(len(graphs)))], 24)
    if name in ("E32", "E256"):
        graphs = [_graph(rng, n, 17) for n in (40, 17, 9) for _ in range(4)]
        return Family(name, "NodeRemovalNet", dict(output_dim=181, conv_width=int(name[1:]), topk=0.5), 17, graphs,
                      [list(range(len(graphs)))], 25)
    if name in ("F5", "F40"):
        fin = int(name[1:])
        graphs = [_graph(rng, n, fin) for n in (30, 9) for _ in range(5)]
        batches = [list(range(len(graphs)))]
        if fin == 40:   # the same 30-row graphs beside a 96-row one: the launch is wide enough to stage form (d)
            graphs.append(_graph(rng, 96, fin))
            batches.append([10, 0, 1, 2, 3, 4])
        return Family(name, "NodeRemovalNet", nrn, fin, graphs, batches, 26)
    if name == "G":     # the generic head beside the C = 128 embedding: 300 outputs, 1 / 31 / 33 graphs
        graphs = [_graph(rng, 20, 17) for _ in range(33)]
        return Family(name, "NodeRemovalNet", dict(output_dim=300, conv_width=128, topk=0.1), 17, graphs,
                      [[0], list(range(31)), list(range(33))], 27)
    if name == "H":     # form equivalence: the same graph in launches of different NMAX
        graphs = [_graph(rng, 40, 2), _graph(rng, 64, 2), _graph(rng, 100, 2)]
        return Family(name, "AirfoilGCNN", dict(conv_width=128), 2, graphs, [[0], [0, 2], [1], [1, 2]], 28)
    raise KeyError(name)


FAMILIES = ("A", "B", "C", "D", "E32", "E256", "F5", "F40", "G")

# forms every family has to reach (checked against `Family.all_forms`: a change of the dispatch that empties one shows)
EXPECTED_FORMS = {
    "A": {"c", "a<17>", "norms:pre", "norms:in-level", "head:c128-t16"},
    "B": {"b<1>", "b<5>", "d:sage:0x16+9", "d:sage:1x16+0", "d:sage:1x16+1", "d:sage:1x16+2"},
    "C": {"c", "b<8>:r0-loop", "d:sage:1x16+9", "d:sage:1x16+1", "d:sage:0x16+9", "d:gcn:0x16+13", "d:gcn:0x16+9",
          "b<5>", "b<1>"},
    "D": {"a<2>", "b<8>", "b<8>:r0-loop", "d:sage:1x16+3", "d:gcn:0x16+12", "head:generic"},
    "E32": {"a<17>", "a<0>", "head:generic"},
    "E256": {"a<17>", "b<8>:r0-loop", "b<5>", "b<1>", "head:generic"},
    "F5": {"c", "a<0>"},
    "F40": {"b<8>", "d:sage:0x16+9", "d:sage:1x16+14"},
    "G": {"c", "head:generic"},
    "H": {"b<5>", "b<8>", "d:sage:1x16+4", "d:sage:2x16+0", "d:sage:0x16+10"},
}


def _norm_dev(a, b):
    """Largest |a - b| in units of the largest |b| (of ONE graph)."""
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(float(np.abs(b).max()), 1e-300))


def yardsticks(r32, r64):
    """What fp32 arithmetic alone costs on one graph: fp32 run against the fp64 run of the same forced selection."""
    return dict(emb=_norm_dev(r32["emb"], r64["emb"]), out=_norm_dev(r32["out"], r64["out"]),
                score=max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(r32["score"], r64["score"])))


@functools.lru_cache(maxsize=None)
def reference(name):
    """(family, free-running fp64 results, fp32 results forced to the fp64 selection, per-graph yardsticks)."""
    fam = _family(name)
    r64 = fam.run(np.float64)
    r32 = fam.run(np.float32, [r["perm"] for r in r64])
    return fam, r64, r32, [yardsticks(a, b) for a, b in zip(r32, r64)]


def family_yardstick(yards):
    return {k: max(y[k] for y in yards) for k in ("emb", "out", "score")}


def tie_stats(name):
    """Input conditions of the GPU comparison, from the reference alone: the tie margin (4 x the score yardstick), the
    smallest boundary / order gap of the family, and the graphs whose order gap at some level is below the margin."""
    fam, r64, _, yards = reference(name)
    margin = 4.0 * family_yardstick(yards)["score"]
    gaps = [ref.score_gaps(r, fam.ratio) for r in r64]
    near = [g for g, gl in enumerate(gaps) if min(o for _, o in gl) <= margin]
    return dict(margin=margin, min_boundary=min(b for gl in gaps for b, _ in gl), min_order=min(o for gl in gaps for _, o in gl),
                near=near, share=len(near) / len(gaps))
