"""Numpy restatement of `mdq_double_q_select` and `mdq_target_update` (include/meshdqn_hip.h), written from the header's text
and not from the kernels: plain loops in the declared order, float32 arithmetic with one rounding per operation."""
import math

import numpy as np

PACK_MAX = 32      # MDQ_GCN_PACK_MAX


def select(q_online, q_target):
    """-> (q_sel [B][OUT] float32, sel [B] int32, value [B] float32).  Per row: best = -inf, j* = 0; column j replaces the
    pair only if q_online[b][j] > best (first maximum, never a NaN, nothing above -inf: column 0); value = q_target[b][j*],
    broadcast over the row of q_sel."""
    qo, qt = np.asarray(q_online, np.float32), np.asarray(q_target, np.float32)
    if qo.ndim != 2 or qo.shape != qt.shape or qo.shape[0] < 1 or qo.shape[1] < 1:
        raise ValueError("select: two [B][OUT] arrays with B, OUT >= 1")
    B, OUT = qo.shape
    sel = np.zeros(B, np.int32)
    for b in range(B):
        best, js = -math.inf, 0
        for j in range(OUT):
            q = float(qo[b, j])
            if q > best:
                best, js = q, j
        sel[b] = js
    value = qt[np.arange(B), sel].copy()
    q_sel = np.repeat(value[:, None], OUT, axis=1)
    return q_sel, sel, value


def polyak(dst, src, tau):
    """-> the new dst (float32).  tau == 1: src's bits.  Otherwise dst + tf * (src - dst) with tf = float32(tau), three
    float32 operations, each rounded on its own."""
    d, s = np.asarray(dst, np.float32), np.asarray(src, np.float32)
    if d.shape != s.shape:
        raise ValueError("polyak: shapes differ")
    if tau == 1.0:
        return s.view(np.uint32).copy().view(np.float32)       # (through the words: a float copy may quieten a NaN)
    tf = np.float32(tau)
    with np.errstate(all="ignore"):
        diff = (s - d).astype(np.float32)
        step = (tf * diff).astype(np.float32)
        return (d + step).astype(np.float32)


def check(n, lens, tau, null=False, same=False):
    """What mdq_target_update refuses before any launch, as a ValueError."""
    if not 1 <= n <= PACK_MAX:
        raise ValueError("n outside 1 .. 32")
    if null:
        raise ValueError("NULL tensor")
    if any(int(v) < 0 for v in list(lens)[:n]):
        raise ValueError("negative len")
    if not (math.isfinite(tau) and 0.0 < tau <= 1.0):
        raise ValueError("tau must lie in (0, 1]")
    if same:
        raise ValueError("dst equals src")
