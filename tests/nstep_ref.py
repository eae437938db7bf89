"""Restatement of `mdq_replay_sample_nstep` (include/meshdqn_hip.h) in numpy: fp64, plain loops, one function per output.
`R` is the record ring as a (capacity, rec_len) float32 array, rec_len = 2 nf + 4 EM + 5; `ns` any object with the fields
of `mdq_replay_nstep` that matter here (n_step, W, capacity, head, gamma).  What the kernel is tested against, bit for bit:
Python floats are IEEE doubles and every `*` and `+` below rounds on its own, in the kernel's order."""
from collections import namedtuple

import numpy as np

Nstep = namedtuple("Nstep", "n_step W capacity head gamma")


def check(ns):
    """Refuses what the entry point refuses of its `ns` argument."""
    if not 1 <= ns.n_step <= 64:
        raise ValueError("n_step outside 1 .. 64")
    if ns.W < 1:
        raise ValueError("W must be positive")
    if ns.capacity % ns.W or ns.capacity < 2 * ns.W:
        raise ValueError("capacity must be a multiple of W and at least 2 W")
    if ns.head % ns.W or not 0 <= ns.head < ns.capacity:
        raise ValueError("head must be a multiple of W in [0, capacity)")
    if not (np.isfinite(ns.gamma) and ns.gamma >= 0):
        raise ValueError("gamma must be finite and not negative")


def _tail(R, nf, EM, j):
    """edges(s), edges(s'), action, reward, done of record j."""
    return R[j, 2 * nf + 4 * EM:2 * nf + 4 * EM + 5]


def walk(R, nf, EM, ns, j0):
    """The records j_0 .. j_(m-1) taken for a draw of record j0."""
    js = [int(j0)]
    while True:
        j = js[-1]
        if len(js) == ns.n_step or _tail(R, nf, EM, j)[4] > 0.5:
            break
        nxt = (j + ns.W) % ns.capacity
        if ns.head <= nxt < ns.head + ns.W:
            break
        js.append(nxt)
    return js


def steps(R, nf, EM, ns, idx):
    return np.array([len(walk(R, nf, EM, ns, j)) for j in idx], np.int32)


def reward(R, nf, EM, ns, idx):
    out = np.zeros(len(idx), np.float32)
    for i, j0 in enumerate(idx):
        g, acc = 1.0, None
        for k, j in enumerate(walk(R, nf, EM, ns, j0)):
            if k:
                g = g * float(ns.gamma)
            term = g * float(_tail(R, nf, EM, j)[3])
            acc = term if acc is None else acc + term
        out[i] = np.float32(acc)
    return out


def nonfinal(R, nf, EM, ns, idx):
    out = np.zeros(len(idx), np.float32)
    for i, j0 in enumerate(idx):
        js = walk(R, nf, EM, ns, j0)
        g = 1.0
        for _ in js[1:]:
            g = g * float(ns.gamma)
        out[i] = np.float32(0.0) if _tail(R, nf, EM, js[-1])[4] > 0.5 else np.float32(g)
    return out


def action(R, nf, EM, ns, idx):
    return np.array([int(_tail(R, nf, EM, j)[2]) for j in idx], np.int64)


def x_s(R, nf, EM, ns, idx):
    return np.stack([R[j, :nf] for j in idx])


def x_n(R, nf, EM, ns, idx):
    rows = []
    for j0 in idx:
        L = walk(R, nf, EM, ns, j0)[-1]
        rows.append(R[j0, :nf] if _tail(R, nf, EM, L)[4] > 0.5 else R[L, nf:2 * nf])
    return np.stack(rows)


def _packed(lists):
    ptr = np.zeros(len(lists) + 1, np.int32)
    for i, (s, _) in enumerate(lists):
        ptr[i + 1] = ptr[i] + len(s)
    cat = [np.concatenate([l[k] for l in lists]).astype(np.int32) if lists else np.zeros(0, np.int32) for k in (0, 1)]
    return cat[0], cat[1], ptr


def _edges_of(R, nf, EM, j, k):
    """(src, dst) of graph k (0: s, 1: s') of record j."""
    cnt = int(_tail(R, nf, EM, j)[k])
    base = 2 * nf + 2 * EM * k
    return R[j, base:base + cnt], R[j, base + EM:base + EM + cnt]


def edges_s(R, nf, EM, ns, idx):
    """-> esrc_s, edst_s (packed back to back), edge_ptr_s (n + 1,)."""
    return _packed([_edges_of(R, nf, EM, j, 0) for j in idx])


def edges_n(R, nf, EM, ns, idx):
    """-> esrc_n, edst_n, edge_ptr_n: s' of the walk's last record, the own state of idx[i] where that one is terminal."""
    lists = []
    for j0 in idx:
        L = walk(R, nf, EM, ns, j0)[-1]
        lists.append(_edges_of(R, nf, EM, j0, 0) if _tail(R, nf, EM, L)[4] > 0.5 else _edges_of(R, nf, EM, L, 1))
    return _packed(lists)


def compose(R, nf, EM, ns, idx):
    """Every output of the entry point, named like the fields of its descriptors."""
    check(ns)
    R = np.asarray(R, np.float32)
    es, ds, ps = edges_s(R, nf, EM, ns, idx)
    en, dn, pn = edges_n(R, nf, EM, ns, idx)
    return dict(x_s=x_s(R, nf, EM, ns, idx), x_n=x_n(R, nf, EM, ns, idx), esrc_s=es, edst_s=ds, edge_ptr_s=ps, esrc_n=en,
                edst_n=dn, edge_ptr_n=pn, action=action(R, nf, EM, ns, idx), reward=reward(R, nf, EM, ns, idx),
                nonfinal=nonfinal(R, nf, EM, ns, idx), steps=steps(R, nf, EM, ns, idx))
