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

A callable `profile(x, y, t)` (`flow_params['inflow']`, any NON-SEPARABLE profile of position and time) is the second kind
(`IpcsBatch(inflow_profile=...)`, `mdq_ipcs_evolve_profile`): it depends on (x, y, t) only, never on the flow state, so all
K steps of a call are evaluated here, up front, at the inlet dofs (`profile_values`: a few dozen values per environment and
step, uploaded once), and a small kernel between the steps rewrites what depends on them - bcu_gx at the inlet dofs and the
lifting vectors on the rows that share a cell with one (`inlet_tables`).  In the operator modes that loop over the steps
inside one kernel it keeps the per-step path of `FlowSolver.evolve` / `IpcsBatch.update_inflow`.

The S3 flow leg of `VecEnv2DAirfoil` takes a callable as well.  Its meshes are numbered on the device, so the host hands over
values at the CANONICAL inlet of every config's original mesh (`canonical_inlet`, `leg_profile_table`: the inlet points never
change during an episode, and the leg always restarts at t = solver_steps * dt) and the device finds the dofs and rows on every
new mesh (`mdq_ipcs_build_inlet_map`).
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
            raise TypeError("a callable inflow profile is not a schedule (it goes to IpcsBatch(inflow_profile=...))")
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


# ------------------------------------------------------------------ non-separable profiles: profile(x, y, t)
def batch_profiles(inflow_profile, B: int):
    """The B profiles of a batch from one callable (broadcast) or a sequence of B callables / None (None: that environment
    keeps the constant parabola); None when there is no callable at all."""
    if inflow_profile is None:
        return None
    if callable(inflow_profile):
        return [inflow_profile] * int(B)
    if isinstance(inflow_profile, (str, dict)):
        raise TypeError(f"inflow_profile must be a callable profile(x, y, t) or a sequence of callables / None, got {inflow_profile!r} "
                        "(a schedule goes to inflow=)")
    profs = list(inflow_profile)
    if len(profs) != B:
        raise ValueError(f"inflow_profile must be one callable or a sequence of length {B} (one per environment), got {len(profs)}")
    for b, p in enumerate(profs):
        if p is not None and not callable(p):
            raise TypeError(f"inflow_profile of environment {b} must be a callable profile(x, y, t) or None, got {p!r}")
    return None if all(p is None for p in profs) else profs


def inlet_tables(topos, coords_list) -> list:
    """Per environment what an inflow profile touches, as a dict:

        dofs  int32 (n_inlet,)   the inlet dofs (`MeshTopology.boundary_conditions(...)["inlet_dofs"]`: scalar P2 dofs whose
                                 value is the profile's - the ones the airfoil / wall conditions do not override), ascending
        xy    float64 (n_inlet, 2)   their coordinates
        gx0   float64 (n_inlet,)     their set-up values (the constant parabola, `["bcu_gx"]` at `dofs`)
        rows  int32 (n_rows,)    the non-Dirichlet P2 rows that share a cell with an inlet dof, ascending: the only rows whose
                                 lifting vectors A1[:, bc] g and M[:, bc] g depend on the inlet values

    Environments that share a topology object and a coordinate array (one airfoil) share one dict."""
    cache, out = {}, []
    for t, x in zip(topos, coords_list):
        key = (id(t), id(x))
        if key not in cache:
            bc = t.boundary_conditions(x)
            dofs = np.asarray(bc["inlet_dofs"], np.int64)
            is_inlet = np.zeros(t.np2, bool)
            is_inlet[dofs] = True
            cd = np.asarray(t.cell_dofs)                                  # (nt, 6)
            touched = np.unique(cd[is_inlet[cd].any(axis=1)])             # every dof of a cell that holds an inlet dof
            rows = touched[bc["bcu_flag"][touched] == 0]
            cache[key] = dict(dofs=dofs.astype(np.int32), xy=np.ascontiguousarray(t.dof_coords(x)[dofs], np.float64),
                              gx0=np.asarray(bc["bcu_gx"], np.float64)[dofs].copy(), rows=rows.astype(np.int32))
        out.append(cache[key])
    return out


def padded(tables, key: str) -> tuple:
    """(counts int32 (B,), int32 (B, cap) padded with -1) of the per-environment lists `key` ('dofs' / 'rows') of
    `inlet_tables`; the capacity is at least 1."""
    n = np.array([len(t[key]) for t in tables], np.int32)
    out = np.full((len(tables), max(int(n.max(initial=0)), 1)), -1, np.int32)
    for b, t in enumerate(tables):
        out[b, :n[b]] = t[key]
    return n, out


def canonical_inlet(topo, coords) -> dict:
    """The inlet of a base mesh in the order the device's inlet map uses (`mdq_ipcs_build_inlet_map`): `inlet_tables` on the
    ORIGINAL topology sorted by y - dict(dofs int32 (n,), xy float64 (n, 2), gx0 float64 (n,), y float64 (n,) ascending).
    Boundary vertices are never removed or moved, so these points are the inlet points of every mesh of an episode; only
    their dof numbers change."""
    tab = inlet_tables([topo], [coords])[0]
    order = np.argsort(tab["xy"][:, 1], kind="stable")
    xy = np.ascontiguousarray(tab["xy"][order])
    return dict(dofs=tab["dofs"][order].copy(), xy=xy, gx0=tab["gx0"][order].copy(), y=xy[:, 1].copy())


def leg_profile_table(inlets, profiles, specs, dts, airfoil, first_step: int, nsteps: int) -> dict:
    """The static inflow table of the S3 flow leg, which always restarts at t = first_step * dt_b: per CONFIG a the values of
    steps first_step + 1 .. first_step + nsteps at its canonical inlet (`inlets[a]`: `canonical_inlet`), gathered by
    `airfoil` (B,) to the batch.  A config contributes `profiles[a](x, y, t)` at `step_times`, or - the one table serves a
    batch that mixes the kinds - `inflow_factors(specs[a], ...) * gx0` for a schedule and `gx0` for None.  `dts`: dt per config.
    Returns dict(n_ref int32 (B,), inlet_y float64 (B, NIN) zero-padded, values float64 (B, nsteps, NIN) zero-padded).
    Validation as in `profile_values`: a result of another shape or a non-finite one raises ValueError naming the config
    and the step."""
    A = len(inlets)
    if not (len(profiles) == len(specs) == len(dts) == A):
        raise ValueError(f"leg_profile_table: one profile, one schedule and one dt per config ({A})")
    NIN = max(max(len(t["y"]) for t in inlets), 1)
    vals = np.zeros((A, int(nsteps), NIN), np.float64)
    ys = np.zeros((A, NIN), np.float64)
    for a, (tab, p, s, dt) in enumerate(zip(inlets, profiles, specs, dts)):
        n = len(tab["y"])
        ys[a, :n] = tab["y"]
        if p is not None:
            try:
                vals[a, :, :n] = profile_values([p], [tab], step_times(dt, first_step, nsteps, 1))[0, :, :n]
            except ValueError as exc:
                raise ValueError(str(exc).replace("environment 0", f"config {a}")) from None
        elif s is not None:
            vals[a, :, :n] = inflow_factors(s, dt, first_step, nsteps)[0][:, None] * tab["gx0"][None, :]
        else:
            vals[a, :, :n] = tab["gx0"]
    airfoil = np.asarray(airfoil, np.int64)
    n_ref = np.array([len(t["y"]) for t in inlets], np.int32)[airfoil]
    return dict(n_ref=np.ascontiguousarray(n_ref), inlet_y=np.ascontiguousarray(ys[airfoil]),
                values=np.ascontiguousarray(vals[airfoil]))


def step_times(dt, first_step: int, nsteps: int, B: int) -> np.ndarray:
    """float64 (B, nsteps): t = (first_step + s) * dt_b, s = 1 .. nsteps - the clock of `inflow_factors` (`dt`: a scalar or
    (B,)).  Every time depends on its own step index only: the times of (0, 8) are those of (0, 3) followed by those of
    (3, 5), bit for bit."""
    dtb = np.broadcast_to(np.asarray(dt, np.float64).reshape(-1), (int(B),))
    k = (int(first_step) + np.arange(1, int(nsteps) + 1)).astype(np.float64)
    return np.ascontiguousarray(k[None, :] * dtb[:, None])


def profile_values(profiles, inlet, times) -> np.ndarray:
    """The table `values` of `mdq_inflow_profile`: float64 (B, K, NIN), row [b][s] = profile_b(x, y, times[b, s]) at the
    inlet dofs of environment b (`inlet`: what `inlet_tables` returned), padded with zeros to NIN = the largest inlet.
    `profiles`: one callable or a sequence of B callables / None; a None profile yields that environment's set-up values
    (the constant parabola) at every step.  `times`: (K,) for every environment or (B, K).

    A profile is evaluated once per distinct (callable, inlet point set, time) and the row reused: environments of one
    airfoil share their inlet points.  The library cannot read a device table, so this is where the values are validated:
    a result that has not the shape (n_inlet,) or is not finite raises ValueError naming the environment and the step."""
    B = len(inlet)
    profs = batch_profiles(profiles, B) or [None] * B
    times = np.asarray(times, np.float64)
    if times.ndim == 1:
        times = np.broadcast_to(times, (B, times.shape[0]))
    if times.ndim != 2 or times.shape[0] != B or times.shape[1] == 0:
        raise ValueError(f"inflow times must have shape (nsteps,) or ({B}, nsteps), got {times.shape}")
    if not np.isfinite(times).all():
        raise ValueError("inflow times must be finite")
    K = times.shape[1]
    NIN = max(max(len(t["dofs"]) for t in inlet), 1)
    out = np.zeros((B, K, NIN), np.float64)
    done = {}
    for b, (p, tab) in enumerate(zip(profs, inlet)):
        n = len(tab["dofs"])
        if p is None:
            out[b, :, :n] = tab["gx0"]
            continue
        try:
            hash(p)
            pk = p
        except TypeError:
            pk = id(p)
        x, y = tab["xy"][:, 0], tab["xy"][:, 1]
        pts = tab["xy"].tobytes()
        for s in range(K):
            t = float(times[b, s])
            key = (pk, pts, t)
            if key not in done:
                v = np.asarray(p(x, y, t), dtype=np.float64)
                if v.shape != (n,):
                    raise ValueError(f"inflow profile of environment {b} at step {s} (t = {t!r}) must return shape ({n},) "
                                     f"(one x-velocity per inlet dof), got {v.shape}")
                if not np.isfinite(v).all():
                    raise ValueError(f"inflow profile of environment {b} at step {s} (t = {t!r}) is not finite")
                done[key] = v
            out[b, s, :n] = done[key]
    return out
