"""GPU tests: what `mdq_ipcs_factorize_pressure` WRITES - status, header, every integer table bit for bit, every double
against fp64 LAPACK factors of the same partition - on synthetic SPD matrices at the sizes the kernel branches on
(tests/pressure_factor_cases.py), driven through the C ABI with no mesh behind them.

Every pd_* buffer starts as a sentinel (NaN / -77) with one guard stride behind the last environment, so a write
outside the documented extents, into a neighbour or past the batch shows; refused environments sit between accepted
ones in every launch.

Accuracy: e = relative max error of `pressure_direct.solve_reference` (the numpy emulation of the flow kernel's solve
phases) on a right-hand side K x_true formed in long double; e_dev with the tables the device wrote, e_ref with
`factor_reference`'s (same partition, LAPACK inverses).  Required: e_dev <= MARGIN max(e_ref, 4 nv 2^-53), and the same
margin per block on max|W K_II - I|, max|F - W K_IG| / max|F| and max|Sinv S - I| (S recomputed from the device's own
partition), each against the same quantity of the reference factors.  Gauss-Jordan without pivoting on an SPD block
has growth factor 1, so the device factors differ from LAPACK's by summation order only.
The per-block floors are one rounding of the entries (pc.block_residuals): they decide only where the reference's
residual is (nearly) exactly 0 - blocks of one or two nodes, and F, whose LAPACK residual is below 2^-53 max|F| in
most blocks.

Measured on an MI355X (18 synthetic cases + the two fixture meshes), device / reference:
  solve   largest e_dev / e_ref 3.01 at grid(903,1) (2.6e-14 against 8.7e-15), 2.49 at line_clusters(112,48), 2.19 at
          grid(40,22), <= 1.6 elsewhere, 0.82 / 0.41 on ys930 / ah93w145; largest e_dev / bound-floor 1.57 (grid(7,1));
  W       largest 4.02 (line_clusters(112,48)), 3.99 (grid(40,22)), 3.54 (grid(112,8)); 2.9 .. 3.2 on the other cases
          with blocks of ~100 nodes and on the two meshes, 2.1 .. 2.4 with blocks of 10 .. 20, 1.42 on grid(9,9) (4 .. 10);
  Sinv    largest 3.19 (grid(40,22)), 2.73 (grid(56,16)), <= 2.03 elsewhere, 1.79 / 1.94 on the meshes;
  F       against max(reference, 2^-53): largest 1.18 (ah93w145), 1.02 (grid(9,9)), < 1 elsewhere; where the reference's
          residual is above 2^-53 the plain ratio is at most 0.96.
These are above 2 and they are real: the W ratio grows with the block size.  That is what the two algorithms predict:
Gauss-Jordan rounds every entry of the block once per elimination step, m times in all, where LAPACK's LU + triangular
inverse accumulates an entry in dot products; with growth factor 1 that is a residual that grows like sqrt(m) u max|W|
against a few u - a factor 3 to 4 at m ~ 100 - and the solve and Sinv ratios (<= 3.2) inherit it.  All are within the margin
of 8 the check started with, which therefore stays."""
import ctypes as C

import numpy as np
import pytest

import pressure_factor_cases as pc

pytestmark = pytest.mark.gpu

MARGIN = 8.0
SENT = -77
F64 = ("pd_W", "pd_F", "pd_Sinv", "pd_gk_val")
ZERO_VARIANT = "grid(13,11)+stored zeros"
# every launch mixes small cases, cases at a limit and refused ones
LAUNCHES = [
    ["grid(1,1)", "grid(904,1)", "grid(2,1)", "grid(56,16)", "grid(5,4)"],
    ["grid(3,1)", "grid(28,32)", "grid(9,9)", "grid(903,1)", ZERO_VARIANT],
    ["grid(13,11)", "grid(1024,1)", "grid(40,22)", "line_clusters(20,5,shift=-75.5)", "line_clusters(112,48)"],
    ["line_clusters(20,5,same_x)", "line_clusters(60,49)", "grid(112,8)", "grid(7,1)"],
]
ALL = [n for names in LAUNCHES for n in names]
ACCEPTED = [n for n in ALL if n == ZERO_VARIANT or pc.CASE[n].status == 0]


def _item(name):
    if name == ZERO_VARIANT:
        coords, K = pc.make("grid(13,11)")
        return coords, K, pc.stored_zero_pattern(K)
    return pc.make(name)


def _expected_status(name):
    return 0 if name == ZERO_VARIANT else pc.CASE[name].status


class Launch:
    """One call of mdq_ipcs_factorize_pressure on `items` (see pc.batch_arrays) and what it left in the buffers."""

    def __init__(self, items, cap=None, NV=None, tables=None):
        import torch
        from meshdqn_amd import _lib
        self.cap = cap = dict(pc.CAP, **(cap or {}))
        h, NV, NSE1 = pc.batch_arrays(items, NV)
        self.B, self.NV = B, NV = len(items), NV
        self.stride = dict(pd_hdr=4, pd_node=NV, pd_meta=cap["NPART"] * 6, pd_rowblk=NV, pd_W=cap["NPW"], pd_F=cap["NPF"],
                           pd_gidx=cap["NPGI"], pd_Sinv=cap["NPS"], pd_gk_ptr=NV + 1, pd_gk_col=cap["NPGK"],
                           pd_gk_val=cap["NPGK"])
        inputs = {k: torch.from_numpy(v).cuda() for k, v in h.items()}
        if tables is None:          # fresh: sentinels everywhere, one guard stride behind the last environment
            tables = {k: (torch.full(((B + 1) * s,), float("nan"), dtype=torch.float64, device="cuda") if k in F64 else
                          torch.full(((B + 1) * s,), SENT, dtype=torch.int32, device="cuda")) for k, s in self.stride.items()}
        assert all(tables[k].numel() == (B + 1) * s for k, s in self.stride.items())
        self.tables = tables
        status = torch.full((B + 1,), SENT, dtype=torch.int32, device="cuda")
        d = _lib.IpcsDesc()
        d.B, d.NV, d.NSE1 = B, NV, NSE1
        for k, v in inputs.items():
            setattr(d, k, v.data_ptr())
        for k, v in tables.items():
            setattr(d, k, v.data_ptr())
        for k, v in cap.items():
            setattr(d, k, v)
        _lib.check(_lib.load().mdq_ipcs_factorize_pressure(C.byref(d), status.data_ptr(), _lib.stream_ptr()),
                   "mdq_ipcs_factorize_pressure")
        torch.cuda.synchronize()
        self.status = status.cpu().numpy()
        self.host = {k: v.cpu().numpy() for k, v in tables.items()}

    def env(self, b):
        return {k: self.host[k][b * s:(b + 1) * s] for k, s in self.stride.items()}

    def raw(self):
        return {k: v.tobytes() for k, v in self.host.items()}


def _sent(a):
    return np.isnan(a) if a.dtype == np.float64 else a == SENT


def check_guard(L):
    """nothing behind the last environment was written"""
    assert L.status[L.B] == SENT
    for k, a in L.env(L.B).items():
        assert _sent(a).all(), k


def check_refused(L, b, code, sz=None):
    """status and zero header; with the sizes `sz` of the case (pc.sizes_reference), also that the refusal came before
    anything later was written: past what the kernel has done by then, the environment's buffers hold the sentinel."""
    assert L.status[b] == code
    e = L.env(b)
    assert e["pd_hdr"].tolist() == [0, 0, 0, 0]
    if sz is None:
        return
    ref_code, stop = pc.refusal_reference(sz, L.cap)
    assert ref_code == code
    nG = sz["nG"]
    if code == -2:          # after the ordering: node / rowblk only
        clean = dict(pd_meta=0, pd_W=0, pd_F=0, pd_gidx=0, pd_Sinv=0, pd_gk_ptr=0, pd_gk_col=0, pd_gk_val=0)
    elif code == -3:        # after the zeroed K_GG: before any K[G, I] entry
        clean = dict(pd_meta=0, pd_W=0, pd_F=0, pd_gidx=0, pd_Sinv=nG * nG, pd_gk_ptr=0, pd_gk_col=0, pd_gk_val=0)
    else:                   # -4 at subdomain `stop`: the subdomains before it are complete (gidx of `stop` may be there too)
        m, gs = np.array(sz["m"][:stop], np.int64), np.array(sz["gs"][:stop], np.int64)
        clean = dict(pd_meta=6 * stop, pd_W=int((m * m).sum()), pd_F=int((m * gs).sum()), pd_gidx=int(gs.sum()) + sz["gs"][stop],
                     pd_gk_ptr=nG + 1, pd_gk_col=sz["kgi"], pd_gk_val=sz["kgi"], pd_Sinv=pc.NGMAX ** 2 + stop * pc.GMAX ** 2)
        assert _sent(e["pd_Sinv"][nG * nG:pc.NGMAX ** 2]).all()
    for k, n in clean.items():
        assert _sent(e[k][n:]).all(), (k, n)
    assert _sent(e["pd_node"][sz["nv"]:]).all() and _sent(e["pd_rowblk"][sz["nv"] - nG:]).all()


def check_untouched(L, b):
    for k, a in L.env(b).items():
        if k != "pd_hdr":
            assert _sent(a).all(), k


def cut_tables(e, nv):
    """One environment's pd_* slices `e` as `solve_reference` takes them, cut at the extents its own header and meta give."""
    nI, nG, nparts, _ = (int(x) for x in e["pd_hdr"])
    meta = e["pd_meta"][:6 * nparts].reshape(-1, 6).astype(np.int64)
    nW, nF, nGI = int((meta[:, 1] ** 2).sum()), int((meta[:, 1] * meta[:, 4]).sum()), int(meta[:, 4].sum())
    cnt = int(e["pd_gk_ptr"][nG])
    return dict(n=nv, nI=nI, nG=nG, nparts=nparts, hdr=e["pd_hdr"], node=e["pd_node"][:nv], meta=e["pd_meta"][:6 * nparts],
                rowblk=e["pd_rowblk"][:nI], W=e["pd_W"][:nW], F=e["pd_F"][:nF], gidx=e["pd_gidx"][:nGI],
                Sinv=e["pd_Sinv"][:nG * nG], gk_ptr=e["pd_gk_ptr"][:nG + 1], gk_col=e["pd_gk_col"][:cnt],
                gk_val=e["pd_gk_val"][:cnt])


def device_tables(L, b, nv):
    return cut_tables(L.env(b), nv)


INT_TABLES = ("hdr", "node", "rowblk", "meta", "gidx", "gk_ptr", "gk_col")
ALL_TABLES = INT_TABLES + ("gk_val", "W", "F", "Sinv")


def check_accepted(L, b, ref, fresh=True):
    """status 0; header and integer tables bit-equal to the reference, gk_val to the matrix entries; with `fresh`
    buffers every element past the documented extents still the sentinel.  Returns the device tables."""
    assert L.status[b] == 0
    e = L.env(b)
    assert e["pd_hdr"].tolist() == ref["hdr"].tolist()
    pd = device_tables(L, b, ref["n"])
    for k in INT_TABLES + ("gk_val",):
        assert pd[k].dtype == ref[k].dtype and np.array_equal(pd[k], ref[k]), k
    for k in ("W", "F", "Sinv"):
        assert pd[k].size == ref[k].size and np.isfinite(pd[k]).all(), k
    if fresh:
        nG = ref["nG"]
        ext = dict(pd_node=ref["n"], pd_rowblk=ref["nI"], pd_meta=ref["meta"].size, pd_gidx=ref["gidx"].size,
                   pd_gk_ptr=nG + 1, pd_gk_col=ref["gk_col"].size, pd_gk_val=ref["gk_val"].size, pd_W=ref["W"].size,
                   pd_F=ref["F"].size)
        for k, n in ext.items():
            assert _sent(e[k][n:]).all(), k
        # Sinv: the inverse in front, the subdomains' Schur slices from 112^2 on, nothing in between
        # (slice s: the gs x gs Schur term of subdomain s at 112^2 + s 48^2)
        assert _sent(e["pd_Sinv"][nG * nG:pc.NGMAX * pc.NGMAX]).all()
        for sub, gs in enumerate(ref["meta"].reshape(-1, 6)[:, 4]):
            o = pc.NGMAX ** 2 + sub * pc.GMAX ** 2
            assert np.isfinite(e["pd_Sinv"][o:o + gs * gs]).all() and _sent(e["pd_Sinv"][o + gs * gs:o + pc.GMAX ** 2]).all(), sub
        assert _sent(e["pd_Sinv"][pc.NGMAX ** 2 + ref["nparts"] * pc.GMAX ** 2:]).all()
    return pd


def same_tables(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ALL_TABLES)


@pytest.fixture(scope="module")
def refs():
    out = {n: pc.factor_reference(*pc.make(n)) for n in ALL if n != ZERO_VARIANT and pc.CASE[n].status == 0}
    out[ZERO_VARIANT] = out["grid(13,11)"]          # stored zeros are no couplings: the same factors
    return out


@pytest.fixture(scope="module")
def runs(lib_built):
    from meshdqn_amd.ipcs_batch import IpcsBatch
    assert pc.CAP == IpcsBatch.PD_DEVICE_CAP
    out = {}
    for names in LAUNCHES:
        L = Launch([_item(n) for n in names])
        for b, n in enumerate(names):
            out[n] = (L, b)
    return out


@pytest.mark.parametrize("name", ALL)
def test_status_header_tables_and_sentinels(runs, refs, name):
    L, b = runs[name]
    check_guard(L)
    st = _expected_status(name)
    print(f"{name}: status {L.status[b]} (expected {st}), header {L.env(b)['pd_hdr'].tolist()}")
    if st == 0:
        check_accepted(L, b, refs[name])
    else:
        check_refused(L, b, st, pc.sizes_reference(*pc.make(name)))


@pytest.mark.parametrize("name", ACCEPTED)
def test_inverses_are_exactly_symmetric(runs, refs, name):
    L, b = runs[name]
    pd = device_tables(L, b, refs[name]["n"])
    for q0, m, woff, foff, g, gioff in pd["meta"].reshape(-1, 6):
        W = pd["W"][woff:woff + m * m].reshape(m, m)
        assert np.array_equal(W, W.T)
    S = pd["Sinv"].reshape(pd["nG"], pd["nG"])
    assert np.array_equal(S, S.T)


def accuracy(name, pd, ref, K):
    """prints every figure, then holds the device tables to MARGIN x the reference's (see pc.block_residuals for the floors)"""
    nv = K.shape[0]
    e_dev, e_ref = pc.solve_error(pd, K), pc.solve_error(ref, K)
    bound = max(e_ref, 4 * nv * pc.U)
    rd, rr = pc.block_residuals(pd, K), pc.block_residuals(ref, K)
    pairs = {k: list(zip(rd[k], rr[k])) for k in ("W", "F")}
    pairs["S"] = [(rd["S"], rr["S"])] if rd["S"] is not None else []
    assert all(len(rd[k]) == len(rr[k]) for k in ("W", "F"))
    # dev / ref: the plain ratio over the blocks whose reference residual is above its floor; dev / bound: what is asserted
    plain = {k: max([d[0] / r[0] for d, r in v if r[0] > r[1]], default=0.0) for k, v in pairs.items()}
    held = {k: max([d[0] / max(r) for d, r in v], default=0.0) for k, v in pairs.items()}
    print(f"ACCURACY {name}: nv {nv} e_dev {e_dev:.3e} e_ref {e_ref:.3e} e_dev/e_ref {e_dev / e_ref if e_ref else 0.0:.3f} "
          f"e_dev/bound {e_dev / bound:.3f} | block dev/ref W {plain['W']:.3f} F {plain['F']:.3f} Sinv {plain['S']:.3f} | "
          f"block dev/max(ref, floor) W {held['W']:.3f} F {held['F']:.3f} Sinv {held['S']:.3f}")
    assert e_dev <= MARGIN * bound
    for k, v in pairs.items():
        for blk, (d, r) in enumerate(v):
            assert d[0] <= MARGIN * max(r), (k, blk, d, r)


@pytest.mark.parametrize("name", ACCEPTED)
def test_factors_solve_as_well_as_lapack_factors(runs, refs, name):
    L, b = runs[name]
    K = _item(name)[1]
    accuracy(name, check_accepted(L, b, refs[name]), refs[name], K)


NEIGHBOURS = ("grid(5,4)", "grid(7,1)")         # at most 3 subdomains: accepted at NPART = 4 too


@pytest.fixture(scope="module")
def refusal_base(lib_built, refs):
    names = [NEIGHBOURS[0], "grid(13,11)", NEIGHBOURS[1]]
    L = Launch([_item(n) for n in names])
    return names, L, [check_accepted(L, b, refs[n]) for b, n in enumerate(names)]


@pytest.mark.parametrize("which,code", [("NPGK", -3), ("NPF", -4), ("NPGI", -4), ("NPART", -2), ("NPS", -2)])
def test_capacity_refusals_leave_the_neighbours_alone(refusal_base, refs, which, code):
    """grid(13,11) one short of what it needs of one capacity, between two accepted environments whose tables must equal,
    bit for bit, those of the launch with room for everything."""
    names, base, base_pd = refusal_base
    ref = refs["grid(13,11)"]
    meta = ref["meta"].reshape(-1, 6).astype(np.int64)
    value = dict(NPGK=ref["gk_col"].size - 1, NPF=int((meta[:, 1] * meta[:, 4]).sum()) - 1, NPGI=int(meta[:, 4].sum()) - 1,
                 NPART=4, NPS=pc.NGMAX ** 2 + 8 * pc.GMAX ** 2 - 1)[which]
    assert ref["nparts"] == 8 and value > 0
    L = Launch([_item(n) for n in names], cap={which: value})
    print(f"{which} = {value}: status {L.status[:3].tolist()}")
    check_guard(L)
    check_refused(L, 1, code, pc.sizes_reference(*pc.make("grid(13,11)")))
    for b in (0, 2):
        assert same_tables(check_accepted(L, b, refs[names[b]]), base_pd[b]), (which, b)


def test_nv_out_of_range_writes_nothing(lib_built, refs):
    L = Launch([0, _item("grid(5,4)"), 1025], NV=1088)
    print("status", L.status[:3].tolist())
    check_guard(L)
    for b in (0, 2):
        check_refused(L, b, -1)
        check_untouched(L, b)
    check_accepted(L, 1, refs["grid(5,4)"])


def test_second_launch_is_bit_equal(runs, lib_built):
    first = runs[LAUNCHES[0][0]][0]
    again = Launch([_item(n) for n in LAUNCHES[0]])
    assert again.status.tobytes() == first.status.tobytes()
    assert again.raw() == first.raw()


def test_stale_buffers_do_not_leak_into_a_smaller_case(lib_built, refs):
    big = Launch([_item("grid(56,16)")])
    check_accepted(big, 0, refs["grid(56,16)"])
    small = Launch([_item("grid(5,4)")], NV=big.NV, tables=big.tables)
    fresh = Launch([_item("grid(5,4)")], NV=big.NV)
    ref = refs["grid(5,4)"]
    pd = check_accepted(small, 0, ref, fresh=False)
    assert same_tables(pd, check_accepted(fresh, 0, ref))
    # what the small case does not own is what the large one left
    e, eb = small.env(0), big.env(0)
    assert e["pd_W"][ref["W"].size:].tobytes() == eb["pd_W"][ref["W"].size:].tobytes()
    assert e["pd_node"][ref["n"]:].tobytes() == eb["pd_node"][ref["n"]:].tobytes()


def test_stored_zeros_are_no_couplings(runs, refs):
    (La, a), (Lb, b) = runs["grid(13,11)"], runs[ZERO_VARIANT]
    n = refs["grid(13,11)"]["n"]
    assert same_tables(device_tables(La, a, n), device_tables(Lb, b, n))


def test_factors_of_an_assembled_mesh(meshes, lib_built):
    """The same checks on what `mdq_ipcs_assemble` really writes: the two fixture meshes through
    IpcsBatch(pressure_direct="device"), the scaled matrix read back from the device's `sl1_off` / `sl1_col` / `K1s` by the
    walk the kernel makes of a row (pc.unpack, which also holds the padding to its rule)."""
    import torch
    from meshdqn_amd.ipcs_batch import IpcsBatch, smooth_coords
    from meshdqn_amd.topology import MeshTopology
    names = ["ys930", "ah93w145"]
    topos = [MeshTopology(*meshes[n]) for n in names]
    batch = IpcsBatch(topos, [smooth_coords(t, 50) for t in topos], device="cuda", pressure_direct="device")
    batch.assemble()
    torch.cuda.synchronize()
    assert (batch.pd_status.cpu().numpy() == 0).all()
    t = {k: batch.t[k].cpu().numpy() for k in ("sl1_off", "sl1_col", "K1s", "sdiagK", "coords") + tuple(batch._pd_dev)}
    for b, name in enumerate(names):
        nv = topos[b].nv
        # (K1s IS the scaled matrix: sdiagK is never multiplied in, so nothing is divided out and gk_val stays bit-comparable)
        K, _ = pc.unpack(t["sl1_off"][b], t["sl1_col"][b], t["K1s"][b], nv)
        assert np.array_equal(K, K.T) and np.abs(np.diag(K) - 1.0).max() < 1e-14 and (t["sdiagK"][b][:nv] > 0).all()
        ref = pc.factor_reference(t["coords"][b][:nv], K)
        pd = cut_tables({k: t[k][b] for k in batch._pd_dev}, nv)
        meta = pd["meta"].reshape(-1, 6)
        print(f"{name}: header {pd['hdr'].tolist()}, m {meta[:, 1].tolist()}, gs {meta[:, 4].tolist()}")
        for k in INT_TABLES + ("gk_val",):
            assert np.array_equal(pd[k], ref[k]), (name, k)
        accuracy(name, pd, ref, K)
