"""Plain reference of the graph Q-networks' forward with a FORCED TopK selection (test helper, numpy only).

A third statement of the operation (besides `meshdqn_amd/airfoilgcnn.py` and `oracle/gcn.py`, neither of which it
imports), written from the docstring of `oracle/gcn.py`:

  SAGEConv     h_i = W_l mean_{j->i} x_j + b_l + W_r x_i      mean over incoming edges, duplicates count, isolated -> 0
  GCNConv      h_i = W sum_{j->i or j=i} d_j^-1/2 d_i^-1/2 x_j + b,   d = in-degree + 1 (the self loop)
  relu, score = tanh(h . w / |w|), k = ceil(ratio n), stable descending top-k `perm`
  x' = h[perm] * score[perm], edges with both ends kept (edge order preserved, relabelled)
  readout [max || mean] over the kept rows, summed over the levels; head lin1-relu-lin2-relu-lin3 (-softmax)

Every floating-point operation runs in `dtype` (float64: the reference; float32: the yardstick of what fp32 arithmetic
alone costs), sums are plain sequential loops (over edges, features, channels), never a library reduction.

TopKPooling is discontinuous: one swapped node changes everything downstream.  `forced_perm` (one index list per
level) makes the reference keep exactly those nodes in that order, while `perm_own` still reports the choice its own
scores would have made - so a kernel's selection can be judged against the scores (ties) and its values against a
reference that went the same way.
"""
import math

import numpy as np


def _arr(t, dtype):
    """state_dict entry (torch tensor or array) -> numpy array of `dtype` (fp32 values are exact in both)."""
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.asarray(t).astype(dtype)


def _affine(rows, w, acc):
    """acc[i, :] += sum_f rows[i, f] * w[:, f], one feature after the other (w is the torch layout [out][in])."""
    for f in range(w.shape[1]):
        acc = acc + rows[:, f:f + 1] * w[:, f][None, :]
    return acc


def sage_conv(x, src, dst, w_l, b_l, w_r):
    n, dt = x.shape[0], x.dtype
    agg = np.zeros_like(x)
    cnt = np.zeros(n, dtype=np.int64)
    for e in range(len(src)):
        agg[dst[e]] = agg[dst[e]] + x[src[e]]
        cnt[dst[e]] += 1
    for i in range(n):
        if cnt[i] > 0:
            agg[i] = agg[i] / dt.type(cnt[i])
    acc = np.zeros((n, w_l.shape[0]), dtype=dt)
    acc = _affine(agg, w_l, acc)
    acc = _affine(x, w_r, acc)
    return acc + b_l[None, :]


def gcn_conv(x, src, dst, w, b):
    n, dt = x.shape[0], x.dtype
    deg = np.ones(n, dtype=np.int64)
    for e in range(len(src)):
        deg[dst[e]] += 1
    dis = np.array([dt.type(1) / np.sqrt(dt.type(d)) for d in deg], dtype=dt)
    agg = np.zeros_like(x)
    for i in range(n):
        agg[i] = dis[i] * dis[i] * x[i]
    for e in range(len(src)):
        agg[dst[e]] = agg[dst[e]] + dis[src[e]] * dis[dst[e]] * x[src[e]]
    acc = _affine(agg, w, np.zeros((n, w.shape[0]), dtype=dt))
    return acc + b[None, :]


def pool_scores(h, pw):
    """tanh(h . w / |w|) of every row of `h` (after relu)."""
    dt = h.dtype
    sp = np.zeros(h.shape[0], dtype=dt)
    wn = dt.type(0)
    for c in range(h.shape[1]):
        sp = sp + h[:, c] * pw[c]
        wn = wn + pw[c] * pw[c]
    return np.tanh(sp / np.sqrt(wn)).astype(dt)


def topk_perm(score, ratio):
    """Stable descending top-k: higher score first, equal scores by lower index; k = ceil(ratio n)."""
    k = int(math.ceil(ratio * len(score)))
    order = sorted(range(len(score)), key=lambda i: (-float(score[i]), i))
    return [int(i) for i in order[:k]]


def filter_edges(src, dst, perm, n):
    new_id = [-1] * n
    for r, i in enumerate(perm):
        new_id[i] = r
    s2, d2 = [], []
    for e in range(len(src)):
        s, d = new_id[src[e]], new_id[dst[e]]
        if s >= 0 and d >= 0:
            s2.append(s)
            d2.append(d)
    return np.asarray(s2, dtype=np.int64), np.asarray(d2, dtype=np.int64)


def readout(xp):
    dt = xp.dtype
    mx = xp[0].copy()
    sm = np.zeros(xp.shape[1], dtype=dt)
    for r in range(xp.shape[0]):
        mx = np.maximum(mx, xp[r])
        sm = sm + xp[r]
    return np.concatenate([mx, sm / dt.type(xp.shape[0])])


def head(emb, sd, softmax, dtype):
    v = emb[None, :]
    for name, relu in (("lin1", True), ("lin2", True), ("lin3", False)):
        w, b = _arr(sd[name + ".weight"], dtype), _arr(sd[name + ".bias"], dtype)
        v = _affine(v, w, np.zeros((1, w.shape[0]), dtype=dtype)) + b[None, :]
        if relu:
            v = np.maximum(v, dtype(0))
    v = v[0]
    if softmax:
        ex = np.exp(v - v.max()).astype(dtype)
        s = dtype(0)
        for c in range(len(ex)):
            s = s + ex[c]
        v = ex / s
    return v


def forward_graph(sd, levels, x, edge_index, ratio, softmax, dtype=np.float64, forced_perm=None):
    """One graph.  `levels`: [(conv name, pool name), ...] in the order the network runs them; the conv kind is read off
    the state_dict keys (`<conv>.lin_l.weight`: SAGE, `<conv>.lin.weight`: GCN).  `x` (n, F), `edge_index` (2, E) local
    node ids.  Returns a dict: per level `pre` (pre-activation rows), `score` (all nodes entering the level), `perm` (the
    nodes kept: `forced_perm[l]` when given), `perm_own` (what the scores of this run select), `readout`; and `emb`,
    `out`."""
    dtype = np.dtype(dtype).type
    x = _arr(x, dtype)
    ei = np.asarray(edge_index.detach().cpu().numpy() if hasattr(edge_index, "detach") else edge_index).reshape(2, -1)
    src, dst = ei[0].astype(np.int64), ei[1].astype(np.int64)
    res = dict(pre=[], score=[], perm=[], perm_own=[], readout=[])
    emb = None
    for l, (conv, pool) in enumerate(levels):
        n = x.shape[0]
        if conv + ".lin_l.weight" in sd:
            pre = sage_conv(x, src, dst, _arr(sd[conv + ".lin_l.weight"], dtype), _arr(sd[conv + ".lin_l.bias"], dtype),
                            _arr(sd[conv + ".lin_r.weight"], dtype))
        else:
            pre = gcn_conv(x, src, dst, _arr(sd[conv + ".lin.weight"], dtype), _arr(sd[conv + ".bias"], dtype))
        h = np.maximum(pre, dtype(0))
        score = pool_scores(h, _arr(sd[pool + ".weight"], dtype).reshape(-1))
        own = topk_perm(score, ratio)
        perm = own if forced_perm is None else [int(i) for i in forced_perm[l]]
        if len(perm) != len(own) or len(set(perm)) != len(perm) or min(perm) < 0 or max(perm) >= n:
            raise ValueError(f"level {l}: forced perm {perm} is no selection of {len(own)} of {n} nodes")
        xp = h[perm] * score[perm][:, None]
        src, dst = filter_edges(src, dst, perm, n)
        ro = readout(xp)
        emb = ro if emb is None else emb + ro
        res["pre"].append(pre), res["score"].append(score), res["perm"].append(perm), res["perm_own"].append(own)
        res["readout"].append(ro)
        x = xp
    res["emb"] = emb
    res["out"] = head(emb, sd, softmax, dtype)
    return res


def forward(sd, levels, graphs, ratio, softmax, dtype=np.float64, forced_perm=None):
    """`graphs`: [(x, edge_index), ...]; `forced_perm`: None or one per-level list per graph.  One dict per graph."""
    return [forward_graph(sd, levels, x, ei, ratio, softmax, dtype, None if forced_perm is None else forced_perm[g])
            for g, (x, ei) in enumerate(graphs)]


def score_gaps(res, ratio):
    """Per level (boundary, order): the gap between the k-th and the (k+1)-th score, and the smallest gap between any two
    neighbours among the k + 1 best - what decides the ORDER of `perm` as well (inf where there is no such pair)."""
    gaps = []
    for score in res["score"]:
        s = sorted((float(v) for v in score), reverse=True)
        k = int(math.ceil(ratio * len(s)))
        top = s[:k + 1]
        gaps.append((s[k - 1] - s[k] if k < len(s) else math.inf,
                     min((a - b for a, b in zip(top, top[1:])), default=math.inf)))
    return gaps
