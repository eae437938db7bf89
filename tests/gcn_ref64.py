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

The learning step (second half of the file) is the backward of exactly this forward, by hand and in the same style,
around the loss term of one graph of a minibatch of B (Huber, delta 1; `w`: importance weight or none):
  mode 0   huber(out[a] - (r + gamma nf max q_other)) w / B
  mode 1   huber(q_other[a] - (r + gamma nf max out)) w / B, differentiated through the FIRST maximum of `out`
The selection is the one the forward run kept (forced or not); the mean readout hands 1/k to every kept row, the max
readout its gradient to the first maximal row of each column; parameters the forward never touches get None.
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


def sage_aggregate(x, src, dst):
    """(mean of the incoming rows, in-degree) of every node; isolated nodes get 0."""
    n, dt = x.shape[0], x.dtype
    agg = np.zeros_like(x)
    cnt = np.zeros(n, dtype=np.int64)
    for e in range(len(src)):
        agg[dst[e]] = agg[dst[e]] + x[src[e]]
        cnt[dst[e]] += 1
    for i in range(n):
        if cnt[i] > 0:
            agg[i] = agg[i] / dt.type(cnt[i])
    return agg, cnt


def sage_conv(x, src, dst, w_l, b_l, w_r):
    n, dt = x.shape[0], x.dtype
    agg, _ = sage_aggregate(x, src, dst)
    acc = np.zeros((n, w_l.shape[0]), dtype=dt)
    acc = _affine(agg, w_l, acc)
    acc = _affine(x, w_r, acc)
    return acc + b_l[None, :]


def gcn_aggregate(x, src, dst):
    """(rows summed over the incoming edges and the self loop with d^-1/2 on both sides, d^-1/2 of every node)."""
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
    return agg, dis


def gcn_conv(x, src, dst, w, b):
    n, dt = x.shape[0], x.dtype
    agg, _ = gcn_aggregate(x, src, dst)
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


def head(emb, sd, softmax, dtype, tape=None):
    """`tape`: a list that receives (input, pre-activation) of the three layers (what the backward needs)."""
    v = emb[None, :]
    for name, relu in (("lin1", True), ("lin2", True), ("lin3", False)):
        w, b = _arr(sd[name + ".weight"], dtype), _arr(sd[name + ".bias"], dtype)
        vin = v[0]
        v = _affine(v, w, np.zeros((1, w.shape[0]), dtype=dtype)) + b[None, :]
        if tape is not None:
            tape.append((vin, v[0]))
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
    `out`; `tape` / `head_tape`: what `backward_graph` needs of the run (level inputs, edges, pooled rows; head layers)."""
    dtype = np.dtype(dtype).type
    x = _arr(x, dtype)
    ei = np.asarray(edge_index.detach().cpu().numpy() if hasattr(edge_index, "detach") else edge_index).reshape(2, -1)
    src, dst = ei[0].astype(np.int64), ei[1].astype(np.int64)
    res = dict(pre=[], score=[], perm=[], perm_own=[], readout=[], tape=[], head_tape=[])
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
        res["tape"].append(dict(x=x, src=src, dst=dst, xp=xp))      # the level's input, its edges, its pooled output
        src, dst = filter_edges(src, dst, perm, n)
        ro = readout(xp)
        emb = ro if emb is None else emb + ro
        res["pre"].append(pre), res["score"].append(score), res["perm"].append(perm), res["perm_own"].append(own)
        res["readout"].append(ro)
        x = xp
    res["emb"] = emb
    res["out"] = head(emb, sd, softmax, dtype, res["head_tape"])
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


# ------------------------------------------------------------------ the learning step: loss term and backward
def huber(diff):
    """HuberLoss with delta 1 of one difference and its slope, in the type of `diff`."""
    t = type(diff)
    if abs(diff) < t(1):
        return t(0.5) * diff * diff, diff
    return abs(diff) - t(0.5), (t(1) if diff > 0 else t(-1))


def first_max(v):
    """Index of the first maximum of a vector (where torch's max sends the gradient)."""
    j = 0
    for c in range(1, len(v)):
        if v[c] > v[j]:
            j = c
    return j


def loss_graph(out, mode, action, reward, nonfinal, gamma, q_other, B, weight=None, dtype=np.float64):
    """The loss term of one graph of a minibatch of `B` and its gradient with respect to the network's outputs `out`.
      mode 0: huber(out[a] - (r + gamma nf max q_other));  mode 1: huber(q_other[a] - (r + gamma nf max out)), through the
      first maximum of `out`;  times `weight` when given, divided by B.  Returns (term, td = the difference, d term / d out)."""
    dt = np.dtype(dtype).type
    out, qo = _arr(out, dt), _arr(q_other, dt).reshape(-1)
    r, nf, gam = dt(reward), dt(nonfinal), dt(gamma)
    if mode == 0:
        j, sign = int(action), dt(1)
        diff = out[j] - (r + gam * nf * qo[first_max(qo)])
    else:
        j, sign = first_max(out), -(gam * nf)
        diff = qo[int(action)] - (r + gam * nf * out[j])
    term, slope = huber(diff)
    dq = sign * slope
    if weight is not None:
        term, dq = term * dt(weight), dq * dt(weight)
    dout = np.zeros(len(out), dtype=dt)
    dout[j] = dq / dt(B)
    return term / dt(B), diff, dout


def _affine_back(d, w):
    """din[i, f] = sum_j d[i, j] w[j, f], one output channel after the other (w in the torch layout [out][in])."""
    acc = np.zeros((d.shape[0], w.shape[1]), dtype=d.dtype)
    for j in range(w.shape[0]):
        acc = acc + d[:, j:j + 1] * w[j][None, :]
    return acc


def _outer_sum(d, rows):
    """g[j, f] = sum_i d[i, j] rows[i, f], one row after the other (the torch layout [out][in] of a weight gradient)."""
    g = np.zeros((d.shape[1], rows.shape[1]), dtype=d.dtype)
    for i in range(d.shape[0]):
        g = g + d[i][:, None] * rows[i][None, :]
    return g


def _row_sum(d):
    s = np.zeros(d.shape[1], dtype=d.dtype)
    for i in range(d.shape[0]):
        s = s + d[i]
    return s


def first_max_rows(xp):
    """Per column the first row holding the column's maximum."""
    best, arg = xp[0].copy(), np.zeros(xp.shape[1], dtype=np.int64)
    for r in range(1, xp.shape[0]):
        better = xp[r] > best
        arg[better] = r
        best = np.where(better, xp[r], best)
    return arg


def backward_graph(sd, levels, res, dout, softmax, dtype=np.float64):
    """Gradient of every parameter (torch layout; None: the forward never touches it) for the run `res` of
    `forward_graph` in the same `dtype`, given d loss / d out.  The selection is the one the run kept (forced or not):
    TopKPooling passes gradients to the kept rows only.  Also returns per level the readout's first-maximum rows."""
    dt = np.dtype(dtype).type
    grads = {k: None for k in sd}
    dout = _arr(dout, dt)
    out = res["out"]
    if softmax:                                  # d softmax: p_i (d_i - sum_c d_c p_c)
        s = dt(0)
        for c in range(len(out)):
            s = s + dout[c] * out[c]
        dz = out * (dout - s)
    else:
        dz = dout
    for name, (vin, _), below in zip(("lin3", "lin2", "lin1"), res["head_tape"][::-1], res["head_tape"][-2::-1] + [None]):
        w = _arr(sd[name + ".weight"], dt)
        grads[name + ".weight"] = dz[:, None] * vin[None, :]
        grads[name + ".bias"] = dz.copy()
        dz = _affine_back(dz[None, :], w)[0]
        if below is not None:                    # the relu in front of this layer
            dz = np.where(below[1] > dt(0), dz, dt(0))
    gemb = dz
    C = len(gemb) // 2
    dxp, amax = None, [None] * len(levels)
    for l in range(len(levels) - 1, -1, -1):
        conv, pool = levels[l]
        t = res["tape"][l]
        x, src, dst, xp = t["x"], t["src"], t["dst"], t["xp"]
        pre, score, perm = res["pre"][l], res["score"][l], res["perm"][l]
        n, k, fin = x.shape[0], len(perm), x.shape[1]
        # readout: mean 1/k to every kept row, max to the first maximal row of each column
        g = np.zeros((k, C), dtype=dt) if dxp is None else dxp
        g = g + (gemb[C:] / dt(k))[None, :]
        amax[l] = first_max_rows(xp)
        for c in range(C):
            g[amax[l][c], c] = g[amax[l][c], c] + gemb[c]
        # TopKPooling: x' = h[perm] s[perm], s = tanh(raw), raw = h . w / |w|
        pw = _arr(sd[pool + ".weight"], dt).reshape(-1)
        hs, ss = np.maximum(pre[perm], dt(0)), score[perm]
        wn2 = dt(0)
        for c in range(C):
            wn2 = wn2 + pw[c] * pw[c]
        wn = np.sqrt(wn2)
        ds, raw = np.zeros(k, dtype=dt), np.zeros(k, dtype=dt)
        for c in range(C):
            ds = ds + g[:, c] * hs[:, c]
            raw = raw + hs[:, c] * pw[c]
        raw = raw / wn
        draw = ds * (dt(1) - ss * ss)
        dh = g * ss[:, None] + draw[:, None] * (pw / wn)[None, :]
        gpw = np.zeros(C, dtype=dt)
        for r in range(k):
            gpw = gpw + draw[r] * (hs[r] / wn - raw[r] * pw / wn2)
        grads[pool + ".weight"] = gpw.reshape(np.shape(sd[pool + ".weight"]))
        dpre = np.where(pre[perm] > dt(0), dh, dt(0))          # the relu
        newid = [-1] * n
        for r, i in enumerate(perm):
            newid[i] = r
        dx = np.zeros((n, fin), dtype=dt)
        if conv + ".lin_l.weight" in sd:         # SAGEConv
            agg, cnt = sage_aggregate(x, src, dst)
            grads[conv + ".lin_l.weight"] = _outer_sum(dpre, agg[perm])
            grads[conv + ".lin_l.bias"] = _row_sum(dpre)
            grads[conv + ".lin_r.weight"] = _outer_sum(dpre, x[perm])
            if l > 0:
                dagg = _affine_back(dpre, _arr(sd[conv + ".lin_l.weight"], dt))
                droot = _affine_back(dpre, _arr(sd[conv + ".lin_r.weight"], dt))
                for r, i in enumerate(perm):
                    dx[i] = dx[i] + droot[r]
                for e in range(len(src)):
                    r = newid[dst[e]]
                    if r >= 0:
                        dx[src[e]] = dx[src[e]] + dagg[r] / dt(cnt[dst[e]])
        else:                                    # GCNConv
            agg, dis = gcn_aggregate(x, src, dst)
            grads[conv + ".lin.weight"] = _outer_sum(dpre, agg[perm])
            grads[conv + ".bias"] = _row_sum(dpre)
            if l > 0:
                dagg = _affine_back(dpre, _arr(sd[conv + ".lin.weight"], dt))
                for r, i in enumerate(perm):
                    dx[i] = dx[i] + dis[i] * dis[i] * dagg[r]
                for e in range(len(src)):
                    r = newid[dst[e]]
                    if r >= 0:
                        dx[src[e]] = dx[src[e]] + dis[src[e]] * dis[dst[e]] * dagg[r]
        dxp = dx
    return grads, amax


def learning_step_graph(sd, levels, res, softmax, mode, action, reward, nonfinal, gamma, q_other, B, weight=None,
                        dtype=np.float64):
    """Loss term, TD error and parameter gradients of one graph of a minibatch of `B`, from its forward run `res` (same
    `dtype`): dict(term, td, grads {name: array or None}, amax [per level])."""
    term, td, dout = loss_graph(res["out"], mode, action, reward, nonfinal, gamma, q_other, B, weight, dtype)
    grads, amax = backward_graph(sd, levels, res, dout, softmax, dtype)
    return dict(term=term, td=td, grads=grads, amax=amax)
