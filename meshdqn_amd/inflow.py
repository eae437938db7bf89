"""Inflow schedules: per-environment, time-dependent SEPARABLE inflows u_x(inlet, t) = a(t) * parabola(y).

A schedule is `(amplitude A, pulsation eps, frequency f [Hz], phase phi [rad])`:

    a(t) = A * (1 + eps * sin(2 pi f t + phi))

which covers another mean velocity (A), a pulsation (eps, f, phi) and, through explicit factors handed to
`IpcsBatch.evolve(inflow_scale=...)`, a recorded gust series.  Every velocity boundary condition but the inlet is zero
and the symmetric elimination is linear in the Dirichlet vector, so the factor a(t) of a step - one number per
environment - applied inside the evolve kernels (`mdq_ipcs_evolve_inflow`, include/meshdqn_hip.h) is the whole
time-dependent inflow: nothing is rebuilt, and K steps run per launch as under the constant inflow.

The factors are built HERE, on the host, in numpy: no trigonometry runs on the device, the factors are bit-equal to what
a numpy reference computes, and - the library cannot read a device table - this is where they are validated.
A callable `profile(x, y, t)` (`flow_params['inflow']`, any non-separable profile) is not handled here: it keeps the
per-step path of `FlowSolver.evolve` / `IpcsBatch.update_inflow`.
"""
from __future__ import annotations

import math
import numbers

import numpy as np

KEYS = ("amplitude", "pulsation", "frequency", "phase")
_DEFAULTS = dict(amplitude=1.0, pulsation=0.0, frequency=0.0, phase=0.0)


def _is_one(value) -> bool:
    """One schedule (not a sequence of them): None, a string, a dict, or a tuple `inflow_spec` returned."""
    return value is None or isinstance(value, (str, dict)) or (
        isinstance(value, tuple) and len(value) == 4 and all(isinstance(v, numbers.Real) for v in value))


def inflow_spec(value):
    """None (the reference's constant parabola: `None` or "constant") or the schedule (amplitude, pulsation, frequency,
    phase) of a dict with those keys - amplitude (default 1.0) finite and > 0, pulsation (0) finite, frequency in Hz (0)
    finite and >= 0, phase in rad (0) finite.  A tuple this function returned passes through.  An unknown key or a bad
    value raises ValueError naming the key; any other string or type raises TypeError."""
    if value is None or (isinstance(value, str) and value == "constant"):
        return None
    if isinstance(value, tuple) and len(value) == 4 and all(isinstance(v, numbers.Real) for v in value):
        value = dict(zip(KEYS, value))
    if not isinstance(value, dict):
        raise TypeError(f"inflow must be 'constant', None, a schedule dict with keys {KEYS} or a callable profile(x, y, t), "
                        f"got {value!r}")
    for k in value:
        if k not in KEYS:
            raise ValueError(f"unknown inflow key {k!r} (known: {', '.join(KEYS)})")
    out = []
    for k in KEYS:
        v = value.get(k, _DEFAULTS[k])
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(float(v)):
            raise ValueError(f"inflow {k} must be a finite number, got {v!r}")
        v = float(v)
        if k == "amplitude" and not v > 0.0:
            raise ValueError(f"inflow amplitude must be > 0, got {v!r}")
        if k == "frequency" and v < 0.0:
            raise ValueError(f"inflow frequency must be >= 0, got {v!r}")
        out.append(v)
    return tuple(out)


def batch_specs(inflow, B: int):
    """The B specs of a batch from one spec / dict / None (broadcast) or a sequence of B of them; None when all are None."""
    if _is_one(inflow):
        specs = [inflow_spec(inflow)] * int(B)
    else:
        if callable(inflow):
            raise TypeError("a callable inflow profile is not a schedule (FlowSolver steps it through IpcsBatch.update_inflow)")
        specs = [inflow_spec(v) for v in inflow]
        if len(specs) != B:
            raise ValueError(f"inflow must be one schedule or a sequence of length {B} (one per environment), got {len(specs)}")
    return None if all(s is None for s in specs) else specs


def spec_table(specs) -> np.ndarray | None:
    """(B, 4) float64 rows A, eps, f, phi (a None row: 1, 0, 0, 0), or None when there is no schedule at all."""
    if specs is None or all(s is None for s in specs):
        return None
    return np.array([(1.0, 0.0, 0.0, 0.0) if s is None else s for s in specs], np.float64)


def inflow_factors(specs, dt, first_step: int, nsteps: int) -> np.ndarray | None:
    """The factors a_b of steps first_step + 1 .. first_step + nsteps: float64 (B, nsteps) with

        a_b = A_b * (1 + eps_b * sin(2 pi f_b t + phi_b))   at   t = (first_step + s) * dt_b,  s = 1 .. nsteps

    - the clock of `evolve`, advanced BEFORE the solve (flow_solver.py:366-371).  `specs`: one spec or a sequence of B
    (a None row gives 1.0); `dt`: a scalar or (B,).  Returns None when every spec is None.  Every factor depends on its
    own step index only: the factors of (0, 8) are those of (0, 3) followed by those of (3, 5), bit for bit."""
    specs = [inflow_spec(s) for s in ([specs] if _is_one(specs) else specs)]
    tab = spec_table(specs)
    dt = np.asarray(dt, np.float64)
    if tab is None:
        return None
    if dt.ndim > 1 or (dt.ndim == 1 and dt.shape[0] not in (1, tab.shape[0]) and tab.shape[0] != 1):
        raise ValueError(f"dt must be a scalar or one value per environment, got shape {dt.shape}")
    B = max(tab.shape[0], dt.shape[0] if dt.ndim == 1 else 1)
    tab = np.broadcast_to(tab, (B, 4))
    dtb = np.broadcast_to(dt.reshape(-1), (B,))
    k = (int(first_step) + np.arange(1, int(nsteps) + 1)).astype(np.float64)
    t = k[None, :] * dtb[:, None]
    A, eps, f, phi = (tab[:, j:j + 1] for j in range(4))
    return np.ascontiguousarray(A * (1.0 + eps * np.sin(2.0 * np.pi * f * t + phi)))
