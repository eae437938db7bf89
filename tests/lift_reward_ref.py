"""Restatement of the env step's reward / terminal logic with the lift part (include/meshdqn_hip.h: mdq_env_result_forces;
meshdqn_amd/reward.py) in plain Python loops: Python floats are IEEE doubles, every operation rounds on its own, in the
order the header writes.  What `reward.rewards`, `mdq_env_result_forces` and `mdq_env_finish` are tested against -
`oracle/env.py` restates the reference, which has no lift part.  Also the seeded case generator both test files share."""
import math

import numpy as np


def fmax(a, b):
    """C's fmax: the other operand where one is a NaN."""
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def step(drags, gt_drag, nv, nv0, code, steps_before, threshold, time_reward, goal_vertices, timesteps, negative_reward,
         lifts=None, gt_lift=None, w=0.0, T=math.inf, F=0.0):
    """One environment: (reward, done, reason, steps_after_without_reset).  `code` is the final error code (0 / 1 / other)."""
    S = len(gt_drag)
    drag_factor = -2.0 * math.log(0.5) / threshold
    ss, acc = 0.0, False
    for s in range(S):
        g, d = float(gt_drag[s]), float(drags[s])
        e = abs(g - d) / abs(g)
        ss += e * e
        acc = acc or abs(abs(g - d) / g) > threshold
    drag_reward = 2.0 * math.exp(-drag_factor * math.sqrt(ss)) - 1.0 if ss == ss else float("nan")
    tr = float(nv0 - nv) * time_reward
    vert = float(nv) < goal_vertices * float(nv0)
    accl = False
    r_ok = drag_reward + tr
    if lifts is not None:
        lift_factor = -2.0 * math.log(0.5) / T
        sl = 0.0
        for s in range(S):
            g, l = float(gt_lift[s]), float(lifts[s])
            el = abs(g - l) / fmax(abs(g), F)
            sl += el * el
            accl = accl or el > T
        lift_reward = 2.0 * math.exp(-lift_factor * math.sqrt(sl)) - 1.0 if sl == sl else float("nan")
        r_ok = (drag_reward + w * lift_reward) / (1.0 + w) + tr
    ok = code == 0
    st = steps_before + 1
    limit = st >= timesteps
    if ok:
        reward, reason = r_ok, (1 if acc else 0) | (2 if accl else 0) | (4 if vert else 0)
    else:
        reward, reason = negative_reward, (8 if code != 1 else 0)
    if limit:
        reason |= 16
    return reward, reason != 0, reason, st


def batch(drags, gt_drag, nv, nv0, code, steps_before, par, lifts=None, gt_lift=None, lift=None):
    """`step` over a batch: gt_drag / gt_lift (S,) or (B, S), nv0 scalar or (B,); `par` = dict(threshold, time_reward,
    goal_vertices, timesteps, negative_reward), `lift` = None or (w, T, F).  Returns rewards f64, dones bool, reasons i32,
    steps_after i64 (without the reset to 0)."""
    B = len(code)
    gd = np.broadcast_to(np.asarray(gt_drag, dtype=np.float64), np.shape(drags))
    gl = None if lifts is None else np.broadcast_to(np.asarray(gt_lift, dtype=np.float64), np.shape(lifts))
    n0 = np.broadcast_to(np.asarray(nv0), (B,))
    out = [step(drags[b], gd[b], int(nv[b]), int(n0[b]), int(code[b]), int(steps_before[b]), par["threshold"], par["time_reward"],
                par["goal_vertices"], par["timesteps"], par["negative_reward"],
                *((None, None) if lifts is None else (lifts[b], gl[b])), *((0.0, math.inf, 0.0) if lift is None else lift))
           for b in range(B)]
    return (np.array([o[0] for o in out], np.float64), np.array([o[1] for o in out], bool),
            np.array([o[2] for o in out], np.int32), np.array([o[3] for o in out], np.int64))


PAR = dict(threshold=1e-3, time_reward=0.005, goal_vertices=0.95, timesteps=10, negative_reward=-1.0)


def final_codes(code_in, rstat, tstat, nsel, N):
    """The error codes after the step's checks (mdq_env_result): a failed re-triangulation, a failed topology run or a
    short selection turn into code 2."""
    c = np.array(code_in, np.int32)
    c[(np.asarray(rstat) != 0) | (np.asarray(nsel) < N) | (np.asarray(tstat) != 0)] = 2
    return c


def random_case(seed, B, S, N=24, NV=96, T=1e-3, F=0.0, A=1, with_tstat=True, special=None):
    """Seeded inputs of one step for B environments over A airfoils: relative drag / lift errors on both sides of their
    thresholds (and none within 1e-9, relative, of one: the stop flags are compared exactly), every code 0 / 1 / 2, a failing
    `rstat`, a short selection (`nsel < N`) and the step limit each at least once where B allows (B >= 8), the rest code 0
    (B >= 9: one of them stops on its lift alone, next to one that goes on);
    a smaller batch takes ONE of them on environment 0 (`special` = 0 .. 5: code 1 at the step limit, code 2, rstat, nsel, the
    step limit, topology status; None: a plain step).
    gt_lift has small entries so that a `lift_floor` F above some |gl_s| changes the denominators.  numpy arrays."""
    rng = np.random.default_rng(seed)
    thr = PAR["threshold"]
    gt_drag = -(0.1 + rng.random((A, S)))
    gt_lift = np.where(rng.random((A, S)) < 0.4, 0.02, 1.0) * (0.1 + rng.random((A, S))) * np.where(rng.random((A, S)) < 0.5, -1.0, 1.0)
    if S > 1:
        gt_lift[:, 0] *= 0.02 / np.where(np.abs(gt_lift[:, 0]) < 0.03, 0.02, 1.0)     # (at least one small entry per airfoil)
    airfoil = (np.arange(B) % A).astype(np.int32)
    while True:
        ed = 4.0 * thr * (rng.random((B, S)) - 0.5)                 # |e| up to twice the threshold, half of them beyond it
        ed[rng.random(B) < 0.5] *= 0.2                              # ... and whole environments inside it
        el = 4.0 * (T if math.isfinite(T) else 1e-3) * (rng.random((B, S)) - 0.5)
        el[rng.random(B) < 0.5] *= 0.2
        drags = gt_drag[airfoil] * (1.0 + ed)
        lifts = gt_lift[airfoil] + el * np.fmax(np.abs(gt_lift[airfoil]), F)
        e = np.abs(gt_drag[airfoil] - drags) / np.abs(gt_drag[airfoil])
        l = np.abs(gt_lift[airfoil] - lifts) / np.fmax(np.abs(gt_lift[airfoil]), F)
        near = (np.abs(e - thr) < 1e-9 * thr).any() or (math.isfinite(T) and (np.abs(l - T) < 1e-9 * T).any())
        if not near:
            break
    nv0 = np.array([NV - 3 * a for a in range(A)], np.int32)
    nv = rng.integers(int(0.93 * NV), NV - 3 * (A - 1) + 1, B).astype(np.int32)
    rstat = np.zeros(B, np.int32)
    tstat = np.zeros(B, np.int32)
    nsel = np.full(B, N, np.int32)
    code = np.zeros(B, np.int32)
    steps = rng.integers(0, 8, B).astype(np.int32)
    if B >= 8:
        pick = rng.permutation(B)
        code[pick[0]], code[pick[1]] = 1, 2
        rstat[pick[2]] = -3
        nsel[pick[3]] = N - 3
        steps[pick[4]] = PAR["timesteps"] - 1                      # the step limit, on a code-0 environment
        steps[pick[0]] = 0                                         # (code 1 away from the limit: -1, not terminal, reason 0)
        code[pick[6]], steps[pick[6]] = 2, PAR["timesteps"] - 1    # ... and on a failed one (reason 8 | 16)
        if with_tstat:
            tstat[pick[5]] = 7
        if B >= 9 and math.isfinite(T):                            # a stop on the lift ALONE (reason 2) and a plain step beside it
            for e, rel in ((pick[7], 1.5), (pick[8], 0.1)):
                a = airfoil[e]
                drags[e] = gt_drag[a] * (1.0 + 1e-4)
                lifts[e] = gt_lift[a] + 0.1 * T * np.fmax(np.abs(gt_lift[a]), F)
                lifts[e, S - 1] = gt_lift[a, S - 1] + rel * T * np.fmax(np.abs(gt_lift[a, S - 1]), F)
                nv[e], steps[e] = nv0[a], 2
    elif special is not None:
        if special == 0:
            code[0], steps[0] = 1, PAR["timesteps"] - 1
        elif special == 1:
            code[0] = 2
        elif special == 2:
            rstat[0] = -3
        elif special == 3:
            nsel[0] = N - 3
        elif special == 4:
            steps[0] = PAR["timesteps"] - 1
        elif with_tstat:
            tstat[0] = 7
    return dict(B=B, S=S, N=N, NV=NV, A=A, gt_drag=gt_drag, gt_lift=gt_lift, airfoil=airfoil, drags=drags, lifts=lifts, nv=nv,
                nv0=nv0, rstat=rstat, tstat=tstat, nsel=nsel, code=code, steps=steps)
