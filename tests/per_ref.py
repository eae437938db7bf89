"""Restatement of the prioritized-replay kernels (mdq_replay_prio_fill / _draw / _update, include/meshdqn_hip.h) in numpy:
fp64, plain loops, prefix sums a plain `np.cumsum` in index order.  What the kernels are tested against."""
import math

import numpy as np


def fill(prio, pmax, base_new, n_new, base_zero, n_zero):
    """In place; refuses what the entry point refuses."""
    cap = len(prio)
    if n_new < 0 or n_zero < 0 or n_new > cap or n_zero > cap:
        raise ValueError("a range exceeds the capacity")
    if (n_new and not 0 <= base_new < cap) or (n_zero and not 0 <= base_zero < cap):
        raise ValueError("a range exceeds the capacity")
    new = [(base_new + i) % cap for i in range(n_new)]
    zero = [(base_zero + i) % cap for i in range(n_zero)]
    if set(new) & set(zero):
        raise ValueError("the two ranges overlap")
    for j in new:
        prio[j] = pmax
    for j in zero:
        prio[j] = 0.0


def prefix(prio):
    """Inclusive prefix sums S_j of the priorities in fp64."""
    return np.cumsum(np.asarray(prio, np.float64))


def targets(total, u):
    """t_i = total * ((i + u_i) / n), evaluated as written in fp64."""
    n = len(u)
    return np.array([float(total) * ((float(i) + float(u[i])) / float(n)) for i in range(n)], np.float64)


def draw(prio, u, beta):
    """-> idx (n,) int32, weight (n,) float32, total (float)."""
    prio = np.asarray(prio, np.float32)
    n = len(u)
    S = prefix(prio)
    total = float(S[-1])
    idx, w = np.zeros(n, np.int32), np.zeros(n, np.float32)
    if total == 0.0:
        return idx, w, total
    last = int(np.flatnonzero(prio > 0)[-1])
    t = targets(total, u)
    for i in range(n):
        j = int(np.searchsorted(S, t[i], side="right"))      # the smallest j with S_j > t_i (S is sorted)
        idx[i] = j if j < len(prio) else last
    pmin = min(float(prio[j]) for j in idx)
    for i in range(n):
        w[i] = np.float32(math.pow(pmin / float(prio[idx[i]]), float(beta)))
    return idx, w, total


def update(prio, pmax, idx, td, alpha, eps):
    """In place on `prio`; returns the new pmax."""
    cap = len(prio)
    pmax = np.float32(pmax)
    for i in range(len(idx)):
        j, d = int(idx[i]), float(td[i])
        if not math.isfinite(d) or not 0 <= j < cap:
            continue
        v = np.float32(math.pow(abs(d) + float(eps), float(alpha)))
        prio[j] = v
        pmax = max(pmax, v)
    return pmax


def ring_ranges(t, G, W, new=True, zero=True):
    """The ranges `SharedDeviceReplay.prio_fill(t)` hands to the fill: group (t - 1) % G is new, group t % G is being written."""
    n_new = W if (new and t > 0) else 0
    return (((t - 1) % G) * W if n_new else 0, n_new, (t % G) * W if zero else 0, W if zero else 0)


def ulp_diff32(a, b):
    """Distance in float32 units in the last place (finite non-negative numbers)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
