"""CPU tests: the synthetic cases of the device pressure factorisation and the numpy restatement of its rule are sound
(tests/pressure_factor_cases.py) - a valid separator, a balanced bisection, factors that solve, and every case on the
side of every limit of `mdq_ipcs_factorize_pressure` that its table entry claims."""
import numpy as np
import pytest

import pressure_factor_cases as pc

ACCEPTED = [c.name for c in pc.CASES if c.status == 0]


@pytest.fixture(scope="module")
def sizes():
    return {c.name: pc.sizes_reference(*pc.make(c.name)) for c in pc.CASES}


@pytest.mark.parametrize("name", [c.name for c in pc.CASES])
def test_case_is_scaled_spd_and_well_conditioned(name):
    coords, K = pc.make(name)
    assert np.array_equal(K, K.T) and (np.diag(K) == 1.0).all()
    assert np.array_equal(coords * 16, np.round(coords * 16))       # multiples of 2^-4: the 51-bit key loses nothing
    ev = np.linalg.eigvalsh(K)
    print(f"{name}: nv {K.shape[0]}, cond(K) = {ev[-1] / ev[0]:.1f}")
    assert ev[0] > 0 and ev[-1] / ev[0] <= 1e4


@pytest.mark.parametrize("name", [c.name for c in pc.CASES])
def test_case_sits_where_its_table_entry_says(sizes, name):
    """The derived sizes put the case on the claimed side of each limit: a change to a generator cannot quietly turn a
    limit case into an ordinary one."""
    c, sz = pc.CASE[name], sizes[name]
    print(name, sz)
    assert sz["nv"] == c.nv and sz["nparts"] == c.nparts
    if isinstance(c.m, list):
        assert sz["m"] == c.m
    elif c.m is not None:
        assert max(sz["m"]) == c.m
    if c.nG is not None:
        assert sz["nG"] == c.nG
    if c.gs is not None:
        assert max(sz["gs"]) == c.gs
    assert pc.status_reference(sz) == c.status
    # which limit a refused case breaks, and that it breaks no earlier one
    if name == "grid(904,1)":
        assert max(sz["m"]) == pc.MMAX + 1 and sz["nG"] <= pc.NGMAX
    if name == "grid(28,32)":
        assert max(sz["m"]) <= pc.MMAX and sz["nG"] == pc.NGMAX + 1
    if name == "line_clusters(60,49)":
        assert max(sz["m"]) <= pc.MMAX and sz["nG"] <= pc.NGMAX and sz["kgi"] <= pc.CAP["NPGK"] and sz["gs"][0] == pc.GMAX + 1
    if name == "line_clusters(112,48)":
        assert sz["m"][0] * sz["gs"][0] == pc.MMAX * pc.GMAX == 5376 > 5 * 1024       # the sixth value per thread of the F stage


def test_cases_cover_the_branches_of_the_kernel(sizes):
    ok = [sizes[n] for n in ACCEPTED]
    assert {m % 4 for n in ("grid(9,9)", "grid(13,11)") for m in sizes[n]["m"]} == {0, 1, 2, 3}    # tile edges of invert_spd
    assert {s["nG"] % 4 for s in ok} == {0, 1, 2, 3}
    assert any(s["nG"] == 0 for s in ok) and any(s["nparts"] < 8 for s in ok) and any(0 in s["gs"] for s in ok)
    assert max(max(s["m"]) for s in ok) == pc.MMAX and max(max(s["gs"]) for s in ok) == pc.GMAX
    assert any(all(m == pc.MMAX for m in s["m"]) for s in ok)                                # NPW filled to the last double
    assert any(s["nv"] == pc.NVMAX for s in sizes.values())
    assert any(m * g > 1024 for s in ok for m, g in zip(s["m"], s["gs"]))                    # more than one F value per thread
    assert sorted({c.status for c in pc.CASES}) == [-4, -2, 0]
    # the two orderings that only the tie-break decides give the partition of the plain line
    a, b = (pc.partition_reference(*pc.make(n))[2] for n in ("line_clusters(20,5,shift=-75.5)", "line_clusters(20,5,same_x)"))
    c = pc.partition_reference(*pc.line_clusters(20, 5))[2]
    assert np.array_equal(a, c) and np.array_equal(b, c)
    assert (pc.make("line_clusters(20,5,shift=-75.5)")[0][:, 0] < 0).sum() == 76    # both signs of the coordinate key


@pytest.mark.parametrize("name", ACCEPTED)
def test_reference_partition_is_valid_and_balanced(name):
    coords, K = pc.make(name)
    part, sep, node = pc.partition_reference(coords, K)
    nv = K.shape[0]
    assert sorted(node.tolist()) == list(range(nv))
    # no coupling between the interiors of two parts
    ip = np.where(sep, -1, part)
    cross = (K != 0) & (ip[:, None] != ip[None, :]) & (ip[:, None] >= 0) & (ip[None, :] >= 0)
    assert not cross.any()
    # sizes differ by at most one at every level
    for level in (1, 2, 3):
        cnt = np.bincount(part >> (3 - level), minlength=1 << level)
        for g in range(1 << (level - 1)):
            a, b = cnt[2 * g], cnt[2 * g + 1]
            assert (a, b) == ((a + b) // 2, (a + b) - (a + b) // 2) or (a + b == 1 and (a, b) == (1, 0)), (level, g)


@pytest.mark.parametrize("name", ACCEPTED)
def test_reference_factors_solve(name):
    """`solve_reference` on the tables of `factor_reference` reproduces x_true to the 1e-11 the host twin is held to."""
    coords, K = pc.make(name)
    pd = pc.factor_reference(coords, K)
    assert pd["nI"] + pd["nG"] == K.shape[0] and pd["meta"].size == 6 * pd["nparts"]
    e = pc.solve_error(pd, K)
    print(f"{name}: e_ref = {e:.3e}")
    assert e < 1e-11
    res = pc.block_residuals(pd, K)
    assert all(r < 1e-11 for r, _ in res["W"] + res["F"]) and (res["S"] is None or res["S"][0] < 1e-11)


def test_packing_keeps_stored_zeros_and_pads_with_the_row():
    coords, K = pc.make("grid(13,11)")
    Z = pc.stored_zero_pattern(K)
    part, sep, _ = pc.partition_reference(coords, K)
    assert (Z & (part[:, None] != part[None, :])).any()           # stored zeros cross parts
    for zeros in (None, Z):
        off, col, val = pc.pack(K, zeros)
        D, stored = pc.unpack(off, col, val, K.shape[0])
        assert np.array_equal(D, K)
        assert np.array_equal(stored, (K != 0) | (Z if zeros is not None else False))
    h, NV, NSE1 = pc.batch_arrays([pc.make("grid(5,4)"), 0, (coords, K, Z)])
    assert NV == 192 and h["nv"].tolist() == [20, 0, 143] and h["sl1_off"].shape == (3, NV // 64 + 2)
