"""GPU: every operator mode of the IPCS step against the sparse-LU oracle on the size ladder (tests/ipcs_ladder_cases.py):
meshes ON the kernels' size switches - fewer triangles than a wave, one / two / three rounds of `atomic_accumulate` at both
widths of the mode-3 velocity kernel, one tile of MF_CH = 1 024 triangles and its exact multiple, more outflow entries than
threads, outflow rows that share a residue mod 512, a capacity NV under the padded 1 024, and the capacity edges of the modes
(N2 = 3 402 / 3 404, 3 584 / 3 586, 4 096 / 4 098, 5 104 / 5 106).

Protocol of test_ipcs_gpu.py::test_first_steps_match_oracle: rtol = 1e-12, three single steps from rest; after every step u
and p within 1e-8 of the oracle's maximum, drag and lift within 1e-8 of max(|drag|, |lift|) of the oracle at that step (the lift
of a nearly symmetric channel is near zero); status words zero, iteration counters positive where a Krylov solve ran.

One batch object serves every mode of a test group (the descriptor's mode is read per call; `reset_state` returns to rest), so
the host-side index build is paid once per group.  The mode the entry point selected is read back from what it does: only
mode 3 accepts `evolve_timed`, and the reproducible modes give the bits of the explicit mode.  Every line `LADDER ...` printed
below is a measured figure (errors against the oracle, iteration counts)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ipcs_ladder_cases as lad

pytestmark = pytest.mark.gpu

TOL = 1e-8
REPRODUCIBLE = (0, 1, 2, 5)


@pytest.fixture(scope="module")
def ladder():
    return lad.load_ladder()


@pytest.fixture(scope="module")
def refs(ladder):
    """name -> the oracle's (u, p, drag, lift) after each of the three steps; computed once per case."""
    from oracle.ipcs import OracleFlowSolver
    cache = {}

    def get(name):
        if name not in cache:
            o = OracleFlowSolver(*ladder[name])
            cache[name] = [o.evolve() for _ in range(lad.STEPS)]
        return cache[name]
    return get


@pytest.fixture(scope="module")
def batches(ladder, lib_built):
    """(names, pressure, copy) -> IpcsBatch, built on first use."""
    cache = {}

    def get(names, pressure=False, copy=0):
        key = (tuple(names), pressure, copy)
        if key not in cache:
            cache[key] = lad.make_batch(ladder, names, pressure_direct=pressure)
        return cache[key]
    return get


def run_mode(batch, mode):
    batch.desc.mode = int(mode)
    batch.reset_state()
    batch.status.zero_()
    return lad.run_steps(batch)


def hold_to_oracle(res, names, refs, label, krylov_pressure=None):
    """Prints the figures of every case, then asserts the bounds."""
    rows = []
    for b, name in enumerate(names):
        ref = refs(name)
        eu = ep = ef = 0.0
        for s, (uo, po, do, lo) in enumerate(ref):
            n2, nv = uo.size // 2, po.size
            u = res["u"][s, b]
            ug = np.concatenate([u[:n2, 0], u[:n2, 1]])
            eu = max(eu, np.abs(ug - uo).max() / np.abs(uo).max())
            ep = max(ep, np.abs(res["p"][s, b, :nv] - po).max() / np.abs(po).max())
            ef = max(ef, max(abs(res["drag"][s, b] - do), abs(res["lift"][s, b] - lo)) / max(abs(do), abs(lo)))
        rows.append((name, eu, ep, ef, res["iters"][b].tolist(), int(res["status"][b])))
        print(f"LADDER {label} {name}: u {eu:.2e} p {ep:.2e} forces {ef:.2e} iters {res['iters'][b].tolist()}")
    for b, (name, eu, ep, ef, it, st) in enumerate(rows):
        assert np.isfinite([eu, ep, ef]).all() and eu < TOL and ep < TOL and ef < TOL, (label, name, eu, ep, ef)
        assert st == 0 and it[0] > 0 and it[2] > 0, (label, name, it, st)
        if krylov_pressure is not None:
            assert (it[1] > 0) == bool(krylov_pressure[b]), (label, name, it, krylov_pressure[b])


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("u", "p", "drag", "lift", "iters"))


def refused(batch, mode, match):
    """An explicit mode the entry point must refuse: an error that names the limit, and nothing stepped."""
    import torch
    from meshdqn_amd import _lib
    batch.desc.mode = int(mode)
    before = batch.u_n.clone()
    with pytest.raises(_lib.MeshDQNHipError, match=match):
        batch.evolve(1)
    torch.cuda.synchronize()
    assert torch.equal(batch.u_n, before)


def runs_mode_3(batch, mode):
    """Whether the entry point selects the three-kernel mode 3 for `mode`: only that one accepts per-kernel timing."""
    from meshdqn_amd import _lib
    batch.desc.mode = int(mode)
    batch.reset_state()
    try:
        batch.evolve_timed(1)
    except _lib.MeshDQNHipError as e:
        assert "mode 3 only" in str(e)
        return False
    return True


# ------------------------------------------------------------------ the small batch: every case of at most 2 400 rows
@pytest.mark.parametrize("pressure", [False, "device"], ids=["cg", "device"])
@pytest.mark.parametrize("mode", [3, -1, 2, 1, 0, 5, 7])
def test_small_batch_matches_oracle(batches, refs, mode, pressure):
    batch = batches(lad.SMALL, pressure)
    assert batch.cap["NV"] < 1024 and batch.cap["NT"] == 1025
    res = run_mode(batch, mode)
    krylov = np.ones(batch.B, bool)
    if pressure == "device":
        # a mesh beyond the factorisation's limits reports through pd_status and keeps the Krylov solve
        st = batch.pd_status.cpu().numpy()
        hdr = batch.t["pd_hdr"].cpu().numpy()
        print("LADDER small pd_status", dict(zip(lad.SMALL, st.tolist())), "parts", hdr[:, 2].tolist())
        assert ((st == 0) == (hdr[:, 2] > 0)).all() and (st <= 0).all()
        krylov = st < 0
    hold_to_oracle(res, lad.SMALL, refs, f"small/{'device' if pressure else 'cg'}/mode{mode}", krylov)
    if mode == -1:
        assert runs_mode_3(batch, -1)
    if mode in REPRODUCIBLE:            # a second batch gives the same bits
        assert same_bits(res, run_mode(batches(lad.SMALL, pressure, copy=1), mode))


def test_outflow_rows_that_share_a_residue_run_mode_3(batches, ladder):
    """No kernel owns outflow rows per thread any more: three of them on one residue mod 512 are no reason to refuse mode 3 or to
    demote auto (the small batch above holds the case to the oracle in both)."""
    b = lad.SMALL.index("outflow_collide")
    batch = batches(lad.SMALL, False)
    rows = batch.host["bo_rows"][b][:batch.host["nbo"][b]]
    assert np.bincount(rows % 512, minlength=512).max() >= 3
    # entries beyond both kernel widths on the two outflow cases, within one pass on the others
    nbe = batch.host["bo_ptr"][np.arange(batch.B), batch.host["nbo"]]
    heavy = [b, lad.SMALL.index("outflow_heavy")]
    assert (nbe[heavy] > 768).all() and (np.delete(nbe, heavy) < 512).all()
    assert runs_mode_3(batch, 3) and runs_mode_3(batch, -1)


# ------------------------------------------------------------------ two / three rounds of the 768-wide kernel, two tiles
@pytest.mark.parametrize("mode,pressure", [(3, False), (3, "device"), (-1, False), (2, False), (1, False), (5, False)])
def test_mid_batch_matches_oracle(batches, refs, mode, pressure):
    batch = batches(lad.MID, pressure)
    res = run_mode(batch, mode)
    krylov = (batch.pd_status.cpu().numpy() < 0) if pressure == "device" else np.ones(batch.B, bool)
    hold_to_oracle(res, lad.MID, refs, f"mid/{'device' if pressure else 'cg'}/mode{mode}", krylov)
    if mode in REPRODUCIBLE:
        assert same_bits(res, run_mode(batch, mode))


# ------------------------------------------------------------------ the 512-wide velocity kernel (MDQ_AT_WG=512, a fresh child)
@pytest.fixture(scope="module")
def width_run(lib_built, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ipcs_ladder") / "wg512.npz")
    env = dict(os.environ, MDQ_AT_WG="512")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [lad.__file__, path]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    return dict(np.load(path))


@pytest.mark.parametrize("key", list(lad.WIDTH_BATCHES))
def test_512_wide_velocity_kernel_matches_oracle(width_run, refs, key):
    names = lad.WIDTH_BATCHES[key]
    res = {k: width_run[f"{key}/{k}"] for k in ("u", "p", "drag", "lift", "iters", "status")}
    hold_to_oracle(res, names, refs, f"wg512/{key}/mode3", np.ones(len(names), bool))


# ------------------------------------------------------------------ the capacity edges, one single-mesh batch each
# name -> (modes that run, explicit modes refused with the text their error must carry, what auto / -2 select)
EDGE_PLAN = {
    "n2_3402": ((3, -1, -2, 2, 1, 0), {}, 3, 2),
    "n2_3404": ((-1, -2, 2, 1, 0), {3: "N2 <= 3402"}, 2, 2),
    "n2_3584": ((-1, -2, 2, 1, 0), {3: "N2 <= 3402"}, 2, 2),
    "n2_3586": ((-1, -2, 0, 1, 4, 5, 7), {3: "N2 <= 3402", 2: "N2 <= 3584"}, 1, 1),
    "n2_4096": ((-1, -2, 0, 1, 4, 5, 7), {3: "N2 <= 3402", 2: "N2 <= 3584"}, 1, 1),
    "n2_4098": ((-1, -2, 0, 1, 4, 5, 7), {3: "N2 <= 3402", 2: "N2 <= 3584"}, 1, 1),
    "n2_5104": ((-1, -2, 0, 1, 4, 5, 7), {3: "N2 <= 3402", 2: "N2 <= 3584"}, 1, 1),
    "n2_5106": ((-1, -2, 0, 4, 5, 7), {3: "N2 <= 3402", 2: "N2 <= 3584", 1: "N2 <= 5104"}, 7, 7),
}


@pytest.mark.parametrize("name", lad.EDGES)
def test_capacity_edge_matches_oracle_in_every_mode_that_fits(batches, refs, ladder, name):
    from meshdqn_amd.ipcs_batch import operator_mode_limits
    run, refuse, auto, repro = EDGE_PLAN[name]
    batch = batches((name,), False)
    n2 = lad.sizes(*ladder[name])["n2"]
    assert batch.N2 == n2 == lad.TARGETS[name][1]
    lim = operator_mode_limits(n2, batch.cap["NV"], batch.cap["NSE1"])
    assert (lim["auto"] or 7, lim["auto_repro"] or 7) == (auto, repro)        # (beyond the LDS-resident modes: the tiles, as a team)
    assert [m for m in (1, 2, 3) if not lim[f"mode{m}"]] == sorted(refuse)
    got = {}
    for mode in run:
        got[mode] = run_mode(batch, mode)
        hold_to_oracle(got[mode], (name,), refs, f"edge/{name}/mode{mode}", [True])
    # what auto selected: only mode 3 accepts per-kernel timing; the reproducible modes give the explicit mode's bits
    assert runs_mode_3(batch, -1) == (auto == 3) and not runs_mode_3(batch, -2)
    if auto != 3:
        assert same_bits(got[-1], got[auto])
    assert same_bits(got[-2], got[repro])
    got_again = run_mode(batch, repro)
    assert same_bits(got_again, got[repro])
    for mode, text in refuse.items():
        refused(batch, mode, text)
    # the device factorisation beside the edge: within its limits or reported, the step matches either way
    bd = batches((name,), "device")
    res = run_mode(bd, -1)
    st = bd.pd_status.cpu().numpy()
    print(f"LADDER edge/{name} pd_status {st.tolist()}")
    hold_to_oracle(res, (name,), refs, f"edge/{name}/device/auto", st < 0)


# ------------------------------------------------------------------ a descriptor without assembled operators (a flow leg's)
ASSEMBLED = ("A1", "Ms", "sl2_off", "sl2_col", "rowptr2", "colidx2", "asm2_ptr", "asm2_src", "rowptr1", "colidx1", "asm1_ptr",
             "asm1_src")
TILE_MAPS = ("mf_tptr", "mf_scat", "mf_rlist", "mf_rcnt", "mf_lpos")


@pytest.mark.parametrize("without_maps", [False, True], ids=["tile_maps", "slot_lists"])
@pytest.mark.parametrize("name", ["n2_3586", "n2_5104"])
def test_matrix_free_only_descriptor_goes_to_the_element_tiles(batches, refs, name, without_maps):
    """What a `FlowLeg` hands over: no assembled velocity / mass operators (and, on device-built index data, no tile maps: the
    dof <- slot lists).  N2 is within the LDS vectors of mode 1, which auto takes for a full descriptor; here auto must go to the
    element tiles, and the assembled modes are refused before anything is launched."""
    import torch
    from meshdqn_amd import _lib
    batch = batches((name,), False)
    full = run_mode(batch, 7)
    hold_to_oracle(full, (name,), refs, f"matfree/{name}/full/mode7", [True])
    d = _lib.IpcsDesc.from_buffer_copy(batch.desc)
    for k in ASSEMBLED + (TILE_MAPS if without_maps else ()):
        setattr(d, k, None)
    keep, batch.desc = batch.desc, d
    try:
        res = run_mode(batch, -1)
        label = f"matfree/{name}/{'slot_lists' if without_maps else 'tile_maps'}/auto"
        hold_to_oracle(res, (name,), refs, label, [True])
        if not without_maps:
            assert same_bits(res, full)                                 # the team tiles on the same maps
        assert same_bits(res, run_mode(batch, 7)) and not runs_mode_3(batch, -1)
        hold_to_oracle(run_mode(batch, 5), (name,), refs, label.replace("auto", "mode5"), [True])
        for mode in (1, 0, 4):
            refused(batch, mode, "assembled operators")
    finally:
        batch.desc = keep
    torch.cuda.synchronize()
