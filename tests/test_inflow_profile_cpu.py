"""CPU tests of non-separable inflow profiles (`meshdqn_amd/inflow.py`: `inlet_tables`, `profile_values`;
`mdq_ipcs_evolve_profile`): the inlet / row tables against a brute-force construction from the cells on both golden meshes,
the values table against direct evaluation (None rows, split calls, dedup, validation), the new entry point within ABI 8,
and the refusals of `IpcsBatch` that need no device."""
import re

import numpy as np
import pytest

import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# the profiles of the issue, on the channel y in [-0.5, 0.5]: non-separable, two shape terms with different time factors
def profile_a(x, y, t):
    return 6.0 * (0.5 + y) * (0.5 - y) * (1.0 + 0.6 * y * np.sin(2.0 * np.pi * 125.0 * t)) * (0.5 + 100.0 * t)


def profile_b(x, y, t):          # another frequency, no ramp
    return 6.0 * (0.5 + y) * (0.5 - y) * (1.0 + 0.4 * y * np.sin(2.0 * np.pi * 50.0 * t))


@pytest.fixture(scope="module")
def topos(meshes):
    from meshdqn_amd.topology import MeshTopology
    return [MeshTopology(*meshes[k]) for k in ("ys930", "ah93w145")]


@pytest.fixture(scope="module")
def tables(topos):
    from meshdqn_amd.inflow import inlet_tables
    return inlet_tables(topos, [t.coords for t in topos])


# ------------------------------------------------------------------ inlet_tables
def test_inlet_tables_equal_a_brute_force_construction_from_the_cells(topos, tables):
    from meshdqn_amd.inflow import padded
    for t, tab in zip(topos, tables):
        bc = t.boundary_conditions(t.coords)
        assert np.array_equal(tab["dofs"], bc["inlet_dofs"]) and tab["dofs"].dtype == np.int32
        assert np.array_equal(tab["xy"], t.dof_coords(t.coords)[bc["inlet_dofs"]])
        assert abs(tab["xy"][:, 1]).max() <= 0.5 and tab["xy"][:, 1].min() < -0.4 and tab["xy"][:, 1].max() > 0.4     # the channel
        inlet = set(int(d) for d in bc["inlet_dofs"])
        want = set()
        for cell in np.asarray(t.cell_dofs):                     # brute force: every cell, every dof
            if any(int(j) in inlet for j in cell):
                want.update(int(i) for i in cell if not bc["bcu_flag"][int(i)])
        rows = tab["rows"]
        assert rows.dtype == np.int32 and len(rows) > 0 and np.all(np.diff(rows) > 0)
        assert set(rows.tolist()) == want                        # every listed row qualifies and none is missing
        assert not bc["bcu_flag"][rows].any() and not (set(rows.tolist()) & inlet)
        assert 0 < len(rows) < t.np2 // 10                        # a short list: what makes the kernel cheap
    for key in ("dofs", "rows"):
        n, arr = padded(tables, key)
        assert n.dtype == np.int32 and arr.dtype == np.int32 and arr.shape == (2, max(len(t[key]) for t in tables))
        assert n[0] != n[1]                                       # the two meshes exercise the padding
        for b, tab in enumerate(tables):
            assert n[b] == len(tab[key]) and np.array_equal(arr[b, :n[b]], tab[key]) and (arr[b, n[b]:] == -1).all()


def test_environments_of_one_airfoil_share_their_table(topos):
    from meshdqn_amd.inflow import inlet_tables
    x = topos[0].coords
    tabs = inlet_tables([topos[0], topos[1], topos[0]], [x, topos[1].coords, x])
    assert tabs[0] is tabs[2] and tabs[0] is not tabs[1]


# ------------------------------------------------------------------ profile_values
def test_profile_values_equal_direct_evaluation(tables):
    from meshdqn_amd.inflow import profile_values, step_times
    times = step_times([1e-3, 5e-4], 0, 6, 2)
    assert times.shape == (2, 6) and times[1, 3] == 4.0 * 5e-4
    V = profile_values([profile_a, profile_b], tables, times)
    NIN = max(len(t["dofs"]) for t in tables)
    assert V.dtype == np.float64 and V.shape == (2, 6, NIN) and V.flags["C_CONTIGUOUS"]
    for b, (p, tab) in enumerate(zip((profile_a, profile_b), tables)):
        n = len(tab["dofs"])
        for s in range(6):
            assert np.array_equal(V[b, s, :n], p(tab["xy"][:, 0], tab["xy"][:, 1], float(times[b, s]))), (b, s)
        assert (V[b, :, n:] == 0.0).all()
    # one callable for the whole batch, one row of times for every environment
    W = profile_values(profile_a, tables, times[0])
    assert np.array_equal(W[0], V[0])
    n1 = len(tables[1]["dofs"])
    assert np.array_equal(W[1, 2, :n1], profile_a(tables[1]["xy"][:, 0], tables[1]["xy"][:, 1], float(times[0, 2])))
    # non-separable: the rows of two steps are not multiples of each other
    q = V[0, 3, :len(tables[0]["dofs"])] / V[0, 0, :len(tables[0]["dofs"])]
    q = q[np.isfinite(q)]
    assert q.max() - q.min() > 1e-2


def test_none_rows_are_the_set_up_values_bit_for_bit(topos, tables):
    from meshdqn_amd.inflow import profile_values
    V = profile_values([None, profile_b], tables, np.array([1e-3, 2e-3, 3e-3]))
    gx = topos[0].boundary_conditions(topos[0].coords)["bcu_gx"]
    n = len(tables[0]["dofs"])
    for s in range(3):
        assert np.array_equal(V[0, s, :n], gx[tables[0]["dofs"]])
    assert np.array_equal(tables[0]["gx0"], gx[tables[0]["dofs"]]) and gx[tables[0]["dofs"]].max() == pytest.approx(1.5, abs=1e-2)
    assert not np.array_equal(V[1, 0], V[1, 1])


def test_values_of_split_calls_are_bitwise_the_values_of_one(tables):
    from meshdqn_amd.inflow import profile_values, step_times
    dts = np.array([1e-3, 5e-4])
    whole = profile_values([profile_a, profile_b], tables, step_times(dts, 0, 8, 2))
    parts = np.concatenate([profile_values([profile_a, profile_b], tables, step_times(dts, 0, 3, 2)),
                            profile_values([profile_a, profile_b], tables, step_times(dts, 3, 5, 2))], axis=1)
    assert np.array_equal(whole, parts)
    from meshdqn_amd.inflow import inflow_factors                 # the clock is the schedules'
    sched = (1.0, 0.5, 125.0, 0.0)
    assert np.array_equal(inflow_factors([sched, sched], dts, 3, 5),
                          1.0 * (1.0 + 0.5 * np.sin(2.0 * np.pi * 125.0 * step_times(dts, 3, 5, 2) + 0.0)))


def test_a_profile_is_called_once_per_distinct_inlet_set_and_step(topos):
    from meshdqn_amd.inflow import inlet_tables, profile_values
    calls = []

    def counting(x, y, t):
        calls.append((len(x), t))
        return profile_a(x, y, t)

    x0, x1 = topos[0].coords, topos[1].coords
    tabs = inlet_tables([topos[0], topos[0], topos[1], topos[0]], [x0, x0, x1, x0])
    times = np.array([1e-3, 2e-3, 3e-3])
    V = profile_values([counting, counting, counting, None], tabs, times)
    assert len(calls) == 2 * 3                                    # two distinct inlet sets x three steps, not 3 x 3
    assert sorted(set(calls)) == sorted(calls)
    assert np.array_equal(V[0], V[1]) and not np.array_equal(V[0], V[3])
    del calls[:]
    profile_values([counting, counting, None, None], tabs, np.array([[1e-3, 2e-3], [1e-3, 3e-3], [0, 0], [0, 0]]))
    assert len(calls) == 3                                        # the same points at another time are another row


@pytest.mark.parametrize("bad,what", [(lambda x, y, t: np.ones(len(x) + 1), "shape"), (lambda x, y, t: 1.0, "shape"),
                                      (lambda x, y, t: np.ones((len(x), 1)), "shape"),
                                      (lambda x, y, t: np.where(t > 1.5e-3, np.nan, 1.0) * np.ones(len(x)), "finite"),
                                      (lambda x, y, t: np.where(t > 1.5e-3, np.inf, 1.0) * np.ones(len(x)), "finite")])
def test_a_wrong_shape_or_a_value_that_is_not_finite_names_environment_and_step(tables, bad, what):
    from meshdqn_amd.inflow import profile_values
    with pytest.raises(ValueError, match=what) as e:
        profile_values([profile_a, bad], tables, np.array([1e-3, 2e-3, 3e-3]))
    assert "environment 1" in str(e.value)
    assert ("step 1" if what == "finite" else "step 0") in str(e.value)
    with pytest.raises(ValueError, match="times"):
        profile_values(profile_a, tables, np.ones((3, 4)))
    with pytest.raises(ValueError, match="finite"):
        profile_values(profile_a, tables, np.array([1e-3, np.nan]))


def test_batch_profiles():
    from meshdqn_amd.inflow import batch_profiles
    assert batch_profiles(None, 3) is None and batch_profiles([None, None], 2) is None
    assert batch_profiles(profile_a, 3) == [profile_a] * 3
    assert batch_profiles((None, profile_b), 2) == [None, profile_b]
    with pytest.raises(ValueError, match="length 3"):
        batch_profiles([profile_a, profile_b], 3)
    with pytest.raises(TypeError):
        batch_profiles([profile_a, 1.0], 2)
    with pytest.raises(TypeError):
        batch_profiles(dict(amplitude=1.0), 2)


# ------------------------------------------------------------------ ABI
def test_the_profile_entry_point_is_declared_within_abi_8():
    import ctypes as C
    from meshdqn_amd import _lib, build
    name = "mdq_ipcs_evolve_profile"
    assert name in _lib.SYMBOLS and name in build.declared_symbols()
    assert sorted(_lib.SYMBOLS) == build.declared_symbols()
    assert _lib.ABI_VERSION == 8
    header = open(os.path.join(ROOT, "include", "meshdqn_hip.h")).read()
    assert re.search(r"#define\s+MDQ_ABI_VERSION\s+8\b", header)
    # the argument list of the header against the ctypes declaration
    decl = re.search(r"MDQ_API int " + name + r"\(([^)]*)\)", header).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["const mdq_ipcs_desc* d", "int32_t nsteps", "double* drag", "double* lift", "int32_t* iters",
                    "const mdq_inflow_profile* prof", "void* stream"]
    restype, argtypes = _lib.SYMBOLS[name]
    assert restype is C.c_int
    assert argtypes == [C.POINTER(_lib.IpcsDesc), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_lib.InflowProfile),
                        C.c_void_p]
    # the struct of the header against its mirror: names, order, types
    body = re.search(r"typedef struct mdq_inflow_profile \{(.*?)\} mdq_inflow_profile;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        typ, names = stmt.rsplit(" ", 1)[0], stmt
        if stmt.startswith("int32_t "):
            fields += [(n.strip(), C.c_int32) for n in stmt[len("int32_t "):].split(",")]
        else:
            assert typ in ("const int32_t*", "const double*"), stmt
            fields.append((names.rsplit(" ", 1)[1], C.c_void_p))
    assert fields == list(_lib.InflowProfile._fields_)
    assert C.sizeof(_lib.InflowProfile) == 8 + 5 * 8


# ------------------------------------------------------------------ refusals that need no device
def test_a_batch_refuses_a_profile_beside_schedules_and_a_sequence_of_the_wrong_length(topos, lib_built):
    from meshdqn_amd.ipcs_batch import IpcsBatch
    two = [topos[0], topos[1]]
    with pytest.raises(ValueError, match="one kind of time-dependent inflow"):
        IpcsBatch(two, inflow_profile=profile_a, inflow=dict(amplitude=0.5))
    with pytest.raises(ValueError, match="one kind of time-dependent inflow"):
        IpcsBatch(two, inflow_profile=[None, profile_b], inflow=[None, dict(pulsation=0.2, frequency=2.0)])
    with pytest.raises(ValueError, match="length 2"):
        IpcsBatch(two, inflow_profile=[profile_a, profile_b, profile_a])
    with pytest.raises(ValueError, match="length 2"):
        IpcsBatch(two, inflow_profile=[profile_a])


def test_evolve_refuses_explicit_factors_beside_a_profile_before_any_launch():
    """`evolve(inflow_scale=...)` on a batch with profiles: ValueError before anything touches the library or a device (the
    batch here is a bare object with the attributes the check reads)."""
    from meshdqn_amd.ipcs_batch import IpcsBatch
    b = IpcsBatch.__new__(IpcsBatch)
    b.B, b.inflow, b.inflow_profile, b.steps_done = 2, None, [profile_a, None], 0
    with pytest.raises(ValueError, match="inflow_scale cannot be combined with inflow_profile"):
        b.evolve(2, inflow_scale=np.ones((2, 2)))
    assert b.steps_done == 0
    b.inflow_profile = None
    with pytest.raises(ValueError, match="inflow_times"):
        b.evolve(2, inflow_times=np.array([1e-3, 2e-3]))


def test_which_operator_modes_serve_a_profile():
    from meshdqn_amd.ipcs_batch import IpcsBatch
    assert [m for m in range(8) if IpcsBatch.mode_serves_profile(m, 3000)] == [2, 3]
    assert IpcsBatch.mode_serves_profile(-1, 3584) and IpcsBatch.mode_serves_profile(-2, 3555)
    assert not IpcsBatch.mode_serves_profile(-1, 3585) and not IpcsBatch.mode_serves_profile(-2, 12924)
