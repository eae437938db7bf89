"""CPU: the size ladder of the IPCS tests (tests/golden/ipcs_ladder.npz) is what its generator builds, every case sits on
the size it was built for and is a flow problem the ORACLE ALONE steps stably; the Python mirror of the kernels' LDS plan
(`ipcs_batch.operator_mode_limits`) agrees with a table of the capacity edges worked out by hand from `lds_plan` and the entry
point's conditions (160 KB of LDS, 512 B of reduction scratch, 16 B per row and vector)."""
import importlib.util
import os

import numpy as np
import pytest

from ipcs_ladder_cases import CASES, EDGES, GOLDEN, MID, SMALL, TARGETS, load_ladder, sizes


@pytest.fixture(scope="module")
def ladder():
    return load_ladder()


def _generator():
    spec = importlib.util.spec_from_file_location("make_ipcs_ladder", os.path.join(GOLDEN, "make_ipcs_ladder.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_is_small_and_complete(ladder):
    path = os.path.join(GOLDEN, "ipcs_ladder.npz")
    assert os.path.getsize(path) < 1 << 20
    z = np.load(path)
    assert sorted(z.files) == sorted(f"{n}/{k}" for n in CASES if n != "hand" for k in ("coords", "cells"))
    for n in CASES:
        c, t = ladder[n]
        assert c.dtype == np.float64 and c.ndim == 2 and c.shape[1] == 2 and np.isfinite(c).all(), n
        assert t.dtype == np.int32 and t.ndim == 2 and t.shape[1] == 3 and t.min() == 0 and t.max() == len(c) - 1, n
    # every case belongs to a batch of the GPU tests
    assert set(SMALL) | set(MID) | set(EDGES) == set(CASES)
    assert all(sizes(*ladder[n])["n2"] <= 2400 for n in SMALL) and all(sizes(*ladder[n])["n2"] > 2400 for n in MID + EDGES)
    assert max(len(ladder[n][0]) for n in SMALL) < 1024        # capacity NV of the small batch: under the padded NVp


@pytest.mark.parametrize("name", CASES)
def test_case_hits_its_size_and_is_a_tagged_channel(ladder, name):
    from meshdqn_amd.topology import TAG_AIRFOIL, TAG_INFLOW, TAG_OUTFLOW, TAG_WALL, MeshTopology
    c, t = ladder[name]
    kind, target = TARGETS[name]
    s = sizes(c, t)
    assert s[kind] == target
    nv, nt = s["nv"], s["nt"]
    assert np.array_equal(np.unique(t), np.arange(nv))                                    # every point is used
    x = c[t]
    e1, e2 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0]
    area = 0.5 * np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])                        # (cells are stored with sorted rows)
    assert area.min() > 1e-9 and abs(area.sum() - (3.5 - _hole_area(c, t))) < 1e-9
    topo = MeshTopology(c, t)
    assert (topo.nv, topo.nt, topo.np2) == (nv, nt, s["n2"])
    nb = int(topo.on_boundary.sum())
    assert nt == 2 * nv - nb and s["n2"] == 4 * nv - nb                                   # one hole
    tags = topo.facet_tags()
    assert set(tags.tolist()) == {TAG_WALL, TAG_AIRFOIL, TAG_INFLOW, TAG_OUTFLOW}


def _hole_area(c, t):
    """Area of the hole: shoelace over the ring of boundary edges strictly inside the channel."""
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [0, 2]]]), axis=1)
    ue, cnt = np.unique(e, axis=0, return_counts=True)
    be = ue[cnt == 1]
    mid = 0.5 * (c[be[:, 0]] + c[be[:, 1]])
    inner = be[(mid[:, 0] > -0.5 + 1e-9) & (mid[:, 0] < 3 - 1e-9) & (np.abs(mid[:, 1]) < 0.5 - 1e-9)]
    nxt = {}
    for a, b in inner:
        nxt.setdefault(int(a), []).append(int(b))
        nxt.setdefault(int(b), []).append(int(a))
    ring, prev = [int(inner[0, 0])], None
    while True:
        cand = [v for v in nxt[ring[-1]] if v != prev]
        prev = ring[-1]
        if cand[0] == ring[0] and len(ring) > 2:
            break
        ring.append(cand[0])
    p = c[ring]
    return 0.5 * abs(np.sum(p[:, 0] * np.roll(p[:, 1], -1) - np.roll(p[:, 0], -1) * p[:, 1]))


@pytest.mark.parametrize("name", CASES)
def test_oracle_alone_steps_the_case_stably(ladder, name):
    """Three steps from rest of the sparse-LU oracle: bounded velocity, and a drag that is not round-off of the pressure (so that
    a relative force bound means something)."""
    from oracle.ipcs import OracleFlowSolver
    o = OracleFlowSolver(*ladder[name])
    assert o.th.np2 == sizes(*ladder[name])["n2"]
    for step in range(3):
        u, p, drag, lift = o.evolve()
        assert np.isfinite(u).all() and np.abs(u).max() <= 5.0, (step, np.abs(u).max())
        assert abs(drag) >= 1e-3 * np.abs(p).max(), (step, drag, np.abs(p).max())


def test_outflow_cases_cross_the_entry_loop_and_collide(ladder):
    from meshdqn_amd.ipcs_batch import IpcsBatch
    from meshdqn_amd.topology import MeshTopology
    rows = {}
    for name in ("outflow_heavy", "outflow_collide"):
        c, t = ladder[name]
        h = IpcsBatch._host_arrays(MeshTopology(c, t), c)
        assert int((h["cell_outflow"] >= 0).sum()) >= 44 and h["bo_col"].size > 768      # entries beyond both kernel widths
        rows[name] = h["bo_rows"]
    assert np.bincount(rows["outflow_collide"] % 512, minlength=512).max() >= 3           # what the host check used to refuse
    # the same mesh, renumbered
    a, b = ladder["outflow_heavy"], ladder["outflow_collide"]
    assert np.allclose(np.sort(a[0].view(np.complex128).ravel()), np.sort(b[0].view(np.complex128).ravel()), rtol=0, atol=0)


# N2 -> (mode 1, mode 2, mode 3 accepted, auto, reproducible auto): by hand from 512 + k * 16 * N2p <= 163 840 with N2p = N2
# rounded up to even (k = 3 vectors: N2p <= 3 402; k = 2: N2p <= 5 104; mode 2: 16 * (N2p + 6 144) and N2 <= 7 * 512 = 3 584)
EDGE_TABLE = {
    152: (True, True, True, 3, 2), 3322: (True, True, True, 3, 2), 3401: (True, True, True, 3, 2), 3402: (True, True, True, 3, 2),
    3403: (True, True, False, 2, 2), 3404: (True, True, False, 2, 2), 3584: (True, True, False, 2, 2),
    3585: (True, False, False, 1, 1), 3586: (True, False, False, 1, 1), 4096: (True, False, False, 1, 1),
    4098: (True, False, False, 1, 1), 5103: (True, False, False, 1, 1), 5104: (True, False, False, 1, 1),
    5105: (False, False, False, 0, 0), 5106: (False, False, False, 0, 0), 12924: (False, False, False, 0, 0),
}


def test_mode_limits_mirror_matches_the_edge_table():
    from meshdqn_amd.ipcs_batch import MODE3_MAX_N2, lds_plan, operator_mode_limits
    assert MODE3_MAX_N2 == 3402
    for n2, (m1, m2, m3, auto, repro) in EDGE_TABLE.items():
        lim = operator_mode_limits(n2)
        assert (lim["mode1"], lim["mode2"], lim["mode3"], lim["auto"], lim["auto_repro"]) == (m1, m2, m3, auto, repro), n2
        assert lim["per_step"] == (auto in (2, 3))
    # the padded lengths: NVp = max(NV, 1024) rounded up to a multiple of 64, N2p even
    assert [lds_plan(100, nv)["NVp"] for nv in (44, 578, 1024, 1025, 1088, 1089, 3322)] == [1024, 1024, 1024, 1088, 1088, 1152, 3328]
    assert [lds_plan(n2, 10)["N2p"] for n2 in (152, 153, 3402, 3403)] == [152, 154, 3402, 3404]
    # the pressure vectors leave the LDS at 5 * 8 * NVp + 512 > 163 840: NVp > 4 083, i.e. NV > 4 032
    assert not operator_mode_limits(16000, 4032)["pressure_global"] and operator_mode_limits(16000, 4033)["pressure_global"]
    # the Laplacian beside them (Krylov solve), NV = 876 (NVp = 1 024, 16 slice offsets): 512 + 40 960 + 12 * NSE1 + 64 <= 163 840
    assert operator_mode_limits(3322, 876, 10190)["k1_lds"] and not operator_mode_limits(3322, 876, 10200)["k1_lds"]


def test_python_callers_take_their_limits_from_the_mirror():
    from meshdqn_amd.flow_leg import profile_leg_refusal
    from meshdqn_amd.ipcs_batch import IpcsBatch
    # a flow leg has no tile pointers: only mode 3 runs its steps one launch sequence each
    assert profile_leg_refusal(3402) is None and profile_leg_refusal(3322) is None
    for n2 in (3403, 3404, 3584, 3586):
        why = profile_leg_refusal(n2)
        assert why is not None and "> 3402" in why and str(n2) in why
    # an IpcsBatch carries them: auto serves a profile through mode 3 up to 3 402 rows and through mode 2 up to 3 584
    assert all(IpcsBatch.mode_serves_profile(m, n2) for m in (-1, -2) for n2 in (3402, 3404, 3584))
    assert not any(IpcsBatch.mode_serves_profile(m, n2) for m in (-1, -2, 0, 1, 4, 5, 7) for n2 in (3585, 3586, 5104))


def test_generator_reproduces_the_committed_sizes(ladder):
    gen = _generator()
    assert set(gen.TARGETS) | {"outflow_collide", "hand"} == set(CASES)
    built = gen.build_all()
    for name, (c, t) in built.items():
        assert sizes(c, t) == sizes(*ladder[name]), name
        assert c.shape == ladder[name][0].shape and t.shape == ladder[name][1].shape
        assert (gen.TARGETS.get(name) or gen.TARGETS[gen.COLLIDE_OF])[:2] == TARGETS[name]
