"""Reward and terminal logic of the env step on the host - the one owner of the formula `Env2DAirfoil.calculate_reward`
(Env2DAirfoil.py:380-428) and `VecEnv2DAirfoil.step_end` evaluate, and of its opt-in LIFT part (not in the reference, whose
`calculate_reward` fills `new_lifts` and ignores them; the device side is `mdq_env_result_forces` / `mdq_env_finish`).

With gl_s = gt_lift[s], nl_s = new_lifts[b][s] and the parameters w = `lift_weight`, T = `lift_threshold`, F = `lift_floor`
(agent_params), everything in fp64 and in this order:

    el_s        = |gl_s - nl_s| / fmax(|gl_s|, F)
    sl          = sum_s el_s^2  (s ascending),    accl = any_s (el_s > T)
    lift_reward = 2 exp(-(2 ln 2 / T) sqrt(sl)) - 1
    reward (code 0) = (drag_reward + w lift_reward) / (1 + w) + time_reward,    done (code 0) = acc || accl || vert

Switched off (neither `lift_weight` nor `lift_threshold` in the config) the functions evaluate exactly the numpy expressions
of the drag-only step; `w = 0, T = inf` gives the same bits.  `reason` is the bitmask of what ended a step (REASON_*):
`done == (reason != 0)`.

The opt-in MESH QUALITY part (`QualitySpec`; device side: `mdq_mesh_quality` measures, `mdq_env_result_quality` /
`mdq_env_finish` decide): with q_min / cot_max the smallest shape quality and the largest cotangent of a smallest angle over
the cells of the environment's mesh, q_ref the q_min of its airfoil's initial mesh, wq = `quality_weight`, Qm = `min_quality`
and max_cot = 1 / tan(radians(`min_angle`)) (+inf for 0):

    quality_reward = 2 fmin(q_min / q_ref, 1) - 1,    accq = (q_min < Qm) || (cot_max > max_cot)
    num = drag_reward;  den = 1;   lift on: num += w lift_reward, den += w;   quality on: num += wq quality_reward, den += wq
    reward (code 0) = num / den + time_reward,    done (code 0) = acc || accl || accq || vert

`wq = 0, Qm = 0, min_angle = 0` with a finite quality gives the bits of "off"."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

REASON_DRAG = 1         # drag accuracy: a relative drag error above `threshold` (code 0)
REASON_LIFT = 2         # lift accuracy: a relative lift error above `lift_threshold` (code 0)
REASON_VERTICES = 4     # vertex goal: nv < goal_vertices nv0 (code 0)
REASON_FAILED = 8       # failed step (code neither 0 nor 1)
REASON_STEP_LIMIT = 16  # step limit `timesteps` reached (any code)
REASON_QUALITY = 32     # mesh quality: q_min below `min_quality` or a smallest angle below `min_angle` (code 0)


def _number(ap, key):
    v = ap[key]
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"agent_params.{key}: a number, not {v!r}")
    return float(v)


@dataclass(frozen=True)
class LiftSpec:
    """The lift part of the reward: `on` False = the reference's drag-only step."""
    on: bool = False
    weight: float = 0.0
    threshold: float = math.inf
    floor: float = 0.0

    def __post_init__(self):
        w, T, F = self.weight, self.threshold, self.floor
        if not (w >= 0.0) or math.isinf(w):
            raise ValueError(f"lift_weight must be finite and >= 0, not {w!r}")
        if not (T > 0.0):
            raise ValueError(f"lift_threshold must be > 0 (inf: no lift stop), not {T!r}")
        if not (F >= 0.0) or math.isinf(F):
            raise ValueError(f"lift_floor must be finite and >= 0, not {F!r}")

    @classmethod
    def from_config(cls, agent_params) -> "LiftSpec":
        """`lift_weight`, `lift_threshold`, `lift_floor` of agent_params.  Neither of the first two: off.  Only `lift_weight`:
        T = `threshold`.  Only `lift_threshold`: w = 0, a pure stop criterion.  `lift_floor` defaults to 0."""
        ap = agent_params
        floor = _number(ap, "lift_floor") if "lift_floor" in ap else 0.0
        if "lift_weight" not in ap and "lift_threshold" not in ap:
            return cls(False, 0.0, math.inf, floor)
        w = _number(ap, "lift_weight") if "lift_weight" in ap else 0.0
        T = _number(ap, "lift_threshold") if "lift_threshold" in ap else _number(ap, "threshold")
        return cls(True, w, T, floor)

    def check_gt_lift(self, gt_lift, S: int, names=None):
        """`gt_lift` (S,) or (A, S) as the formula needs it: S values per airfoil, no zero denominator max(|gl_s|, F).
        Raises ValueError naming the airfoil and the snapshot.  Nothing is asked of it while the spec is off."""
        if not self.on:
            return
        gl = np.asarray(gt_lift, dtype=np.float64)
        if gl.ndim == 0 or gl.shape[-1] != S or gl.ndim > 2:
            raise ValueError(f"lift-aware reward: gt_lift needs {S} values per airfoil (one per snapshot), got shape {gl.shape}")
        gl = gl.reshape(-1, S)
        bad = np.argwhere(np.fmax(np.abs(gl), self.floor) == 0.0)
        if bad.size:
            a, s = (int(v) for v in bad[0])
            name = names[a] if names is not None else a
            raise ValueError(f"lift-aware reward: gt_lift of airfoil {name}, snapshot {s} is 0 and lift_floor is 0 - the relative "
                             "lift error has no denominator (set lift_floor)")


OFF = LiftSpec()

QUALITY_KEYS = ("quality_weight", "min_quality", "min_angle")


@dataclass(frozen=True)
class QualitySpec:
    """The mesh-quality part of the reward: `on` False = no quality launch, no quality term, no quality stop."""
    on: bool = False
    weight: float = 0.0
    min_quality: float = 0.0
    min_angle: float = 0.0      # degrees

    def __post_init__(self):
        w, Qm, ang = self.weight, self.min_quality, self.min_angle
        if not (w >= 0.0) or math.isinf(w):
            raise ValueError(f"quality_weight must be finite and >= 0, not {w!r}")
        if not (0.0 <= Qm < 1.0):
            raise ValueError(f"min_quality must lie in [0, 1) (0: no stop), not {Qm!r}")
        if not (0.0 <= ang < 60.0):
            raise ValueError(f"min_angle must lie in [0, 60) degrees (0: no stop), not {ang!r}")

    @property
    def max_cot(self) -> float:
        """1 / tan(radians(min_angle)), +inf for 0: the ONE double the host formula and the kernels compare cot_max with."""
        return math.inf if self.min_angle == 0.0 else 1.0 / math.tan(math.radians(self.min_angle))

    @classmethod
    def from_config(cls, agent_params) -> "QualitySpec":
        """`quality_weight`, `min_quality`, `min_angle` of agent_params; none of them: off.  A missing key is 0."""
        ap = agent_params
        if not any(k in ap for k in QUALITY_KEYS):
            return cls()
        w, Qm, ang = (_number(ap, k) if k in ap else 0.0 for k in QUALITY_KEYS)
        return cls(True, w, Qm, ang)

    def check_q_ref(self, q_ref, names=None):
        """`q_ref` (A,): the q_min of every airfoil's initial mesh, the denominator of quality_reward.  Raises ValueError
        naming the airfoil whose initial mesh has a degenerate cell.  Nothing is asked of it while the spec is off."""
        if not self.on:
            return
        q = np.atleast_1d(np.asarray(q_ref, dtype=np.float64))
        bad = np.flatnonzero(~(q > 0.0))
        if bad.size:
            a = int(bad[0])
            name = names[a] if names is not None else a
            raise ValueError(f"mesh-quality reward: the initial mesh of airfoil {name} has q_min = {q[a]!r} (a degenerate or "
                             "broken cell) - quality_reward has no denominator")


QUALITY_OFF = QualitySpec()


def min_angle_degrees(cot_max):
    """The smallest angle in degrees from the cotangent the quality kernel reports (+inf: 0)."""
    return np.degrees(np.arctan2(1.0, np.asarray(cot_max, dtype=np.float64)))


def _quality_terms(qspec, quality, q_ref):
    """(quality_reward, accq) for `quality` (..., 2) = (q_min, cot_max) and q_ref (scalar or (B,))."""
    qual = np.asarray(quality, dtype=np.float64)
    q_min, cot_max = qual[..., 0], qual[..., 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        quality_reward = 2 * np.fmin(q_min / np.asarray(q_ref, dtype=np.float64), 1.0) - 1
    return quality_reward, (q_min < qspec.min_quality) | (cot_max > qspec.max_cot)


def accuracy_terms(spec, gt_drag, new_drags, threshold, gt_lift=None, new_lifts=None, *, qspec=QUALITY_OFF, quality=None,
                   q_ref=None):
    """The accuracy part of a code-0 step, for one environment ((S,) arrays) or a batch ((B, S); ground truth (S,) or
    (B, S)): (value, acc, accl) - `value` the reward without its time term, `acc` / `accl` the drag / lift stop.  With
    `qspec` on (`quality` (2,) or (B, 2), `q_ref` scalar or (B,)) a fourth value follows: accq, the quality stop."""
    one = np.ndim(new_drags) == 1
    drag_factor = -2 * np.log(0.5) / threshold
    err = np.abs(gt_drag - new_drags) / np.abs(gt_drag)
    drag_reward = 2 * np.exp(-drag_factor * (np.linalg.norm(err) if one else np.linalg.norm(err, axis=1))) - 1
    acc = (np.abs(np.abs(gt_drag - new_drags) / gt_drag) > threshold).any(axis=-1)
    if qspec.on:
        quality_reward, accq = _quality_terms(qspec, quality, q_ref)
    if not spec.on:
        if qspec.on:
            return (drag_reward + qspec.weight * quality_reward) / (1.0 + qspec.weight), acc, np.zeros_like(acc), accq
        return drag_reward, acc, np.zeros_like(acc)
    gl, nl = np.asarray(gt_lift, dtype=np.float64), np.asarray(new_lifts, dtype=np.float64)
    el = np.abs(gl - nl) / np.fmax(np.abs(gl), spec.floor)
    sl = np.zeros(el.shape[:-1])
    for s in range(el.shape[-1]):       # (s ascending, like the kernels: S is a handful)
        sl = sl + el[..., s] * el[..., s]
    with np.errstate(divide="ignore"):
        lift_factor = -2 * np.log(0.5) / np.float64(spec.threshold)
    lift_reward = 2 * np.exp(-lift_factor * np.sqrt(sl)) - 1
    accl = (el > spec.threshold).any(axis=-1)
    if qspec.on:
        num, den = drag_reward + spec.weight * lift_reward, 1.0 + spec.weight
        return (num + qspec.weight * quality_reward) / (den + qspec.weight), acc, accl, accq
    return (drag_reward + spec.weight * lift_reward) / (1.0 + spec.weight), acc, accl


def rewards(spec, gt_drag, new_drags, nv, nv0, code, steps, threshold, time_reward, goal_vertices, timesteps,
            negative_reward=-1.0, gt_lift=None, new_lifts=None, *, qspec=QUALITY_OFF, quality=None, q_ref=None):
    """The step's rewards (B,) f64, dones (B,) bool and reasons (B,) int32 for `new_drags` / `new_lifts` (B, S): `nv` the
    vertex counts, `nv0` the initial ones (scalar or (B,)), `code` the error codes (0 removed, 1 "already removed": -1 and
    not terminal, else failed: -1 and terminal), `steps` the step counters INCLUDING this step."""
    code = np.asarray(code)
    terms = accuracy_terms(spec, gt_drag, new_drags, threshold, gt_lift, new_lifts, qspec=qspec, quality=quality, q_ref=q_ref)
    value, acc, accl = terms[:3]
    accq = terms[3] if qspec.on else np.zeros_like(acc)
    B = len(code)
    rew = np.zeros(B)
    dones = np.zeros(B, bool)
    tr = (nv0 - nv) * time_reward
    vert = nv < goal_vertices * nv0
    ok = code == 0
    rew[ok] = (value + tr)[ok]
    dones[ok] = (acc | accl | accq | vert)[ok]
    rew[~ok] = negative_reward
    dones[~ok] = code[~ok] != 1        # (code 1 = "already removed": -1, not terminal, Env2DAirfoil.py:359-360; never produced)
    limit = np.asarray(steps) >= timesteps
    dones |= limit
    reasons = np.where(ok, acc * REASON_DRAG | accl * REASON_LIFT | vert * REASON_VERTICES | accq * REASON_QUALITY,
                       (code != 1) * REASON_FAILED)
    reasons = (reasons | limit * REASON_STEP_LIMIT).astype(np.int32)
    return rew, dones, reasons
