"""The two fp64 kernels every environment step runs before its reward exists, against independent fp64 references
(tests/oracle_util.py: signed-area barycentrics, written-out P2 / P1 bases, a scan over all cells, the divergence theorem):

  * `mdq_interpolate_snapshots` (interpolate_kernel), driven through its descriptor so that the tests choose the target
    points and read the located cells (`out_cell`): random points in cells, every source vertex and edge midpoint, points
    along edges, the lines and corners of the location grid, the P2 dof points of both golden episodes; the gather path
    without the cell records, ragged batches with spare capacity, the split point counts, per-environment sources (ABI 8),
    the error returns, and points outside the domain (bin-local extrapolation);
  * `mdq_probe_forces` (probe_kernel) on one ragged batch of five meshes: random fields against oracle/fem.py, and the
    fields whose drag / lift the divergence theorem gives in closed form.

Tolerances: values within 1e-12 of the field's largest value; a located cell must contain its point up to barycentrics
of -1e-12."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle_util import (airfoil_area, barycentrics, brute_locate, closed_form_fields, interleaved_to_oracle_vel,
                         p2_cell_dofs, p2p1_eval, quadratic)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
S = 4            # snapshots 0, 1: random dof values; 2, 3: nodal values of a random quadratic u / linear p
TOL = 1e-12      # values: relative to the largest value of the snapshot
BAND = 1e-12     # containment: smallest barycentric of the located cell
MU = 1e-3
CELL_SENTINEL = -7


class Src:
    """A source mesh (smoothed coordinates), its S snapshots and the product's location grid (SnapshotInterpolator)."""

    def __init__(self, topo, seed):
        from meshdqn_amd.mesh_ops import SnapshotInterpolator
        self.topo, self.x = topo, topo.coords
        self.dofs = p2_cell_dofs(topo)
        rng = np.random.default_rng(seed)
        dc = topo.dof_coords()
        self.poly_u = rng.standard_normal((2, 2, 6))      # (snapshot, component, coefficient)
        self.poly_p = rng.standard_normal((2, 3))
        u = rng.standard_normal((S, topo.np2, 2))
        p = rng.standard_normal((S, topo.nv))
        for j in range(2):
            u[2 + j] = np.stack([quadratic(self.poly_u[j, c], dc) for c in range(2)], axis=1)
            p[2 + j] = quadratic(self.poly_p[j], dc[:topo.nv])
        self.u, self.p = u, p
        self.interp = SnapshotInterpolator(topo, topo.coords, torch.from_numpy(u), torch.from_numpy(p), device="cuda")
        self.gnx, self.gny, self.x0, self.y0, self.inv_hx, self.inv_hy = self.interp.grid
        self.bin_ptr = self.interp.t["bin_ptr"].cpu().numpy()
        self.bin_cells = self.interp.t["bin_cells"].cpu().numpy()

    def exact(self, pts):
        """The polynomial snapshots' exact values at pts: u (2, m, 2), p (2, m)."""
        return (np.stack([np.stack([quadratic(self.poly_u[j, c], pts) for c in range(2)], axis=1) for j in range(2)]),
                np.stack([quadratic(self.poly_p[j], pts) for j in range(2)]))

    def bin_of(self, pts):
        """The kernel's bin rule: floor((x - x0) * inv_h), clamped to the grid."""
        gx = np.clip(np.floor((pts[:, 0] - self.x0) * self.inv_hx).astype(np.int64), 0, self.gnx - 1)
        gy = np.clip(np.floor((pts[:, 1] - self.y0) * self.inv_hy).astype(np.int64), 0, self.gny - 1)
        return gy * self.gnx + gx

    def fill(self, r, cellrec=True):
        """The source fields of an InterpDesc / InterpSrc."""
        r.src_nv, r.src_nt, r.src_n2 = self.topo.nv, self.topo.nt, self.topo.np2
        r.gnx, r.gny, r.x0, r.y0, r.inv_hx, r.inv_hy = self.interp.grid
        for k, v in self.interp.t.items():
            setattr(r, k, v.data_ptr())
        if not cellrec:
            r.src_cellrec = None


@pytest.fixture(scope="module")
def sources(meshes, lib_built):
    from meshdqn_amd.ipcs_batch import smooth_coords
    from meshdqn_amd.mesh_ops import red_refine
    from meshdqn_amd.topology import MeshTopology
    out = {}
    for seed, name in enumerate(("ys930", "ah93w145")):
        t = MeshTopology(*meshes[name])
        out[name] = Src(MeshTopology(smooth_coords(t, 50), t.cells), seed)
    # ys930 smoothed, red-refined once, smoothed again (3 322 vertices: bins hold more candidates than one batch of the kernel)
    coords, cells = meshes["ys930"]
    rc, rcells = red_refine(smooth_coords(MeshTopology(coords, cells), 50), cells)
    t = MeshTopology(rc, rcells)
    out["ys930_refined"] = Src(MeshTopology(smooth_coords(t, 50), t.cells), 2)
    assert out["ys930_refined"].topo.nv == 3322
    assert np.diff(out["ys930_refined"].bin_ptr).max() > 6
    return out


@functools.lru_cache(maxsize=None)
def _episode(fixture):
    """The meshes of a golden episode, replayed as Env2DAirfoil steps them (smooth(50) at load; per step: the recorded
    vertex removed by Qhull Delaunay, then smooth(50)) -> [MeshTopology after every step]."""
    from meshdqn_amd.ipcs_batch import smooth_coords
    from meshdqn_amd.mesh_ops import remove_vertex_delaunay
    from meshdqn_amd.topology import MeshTopology
    ep = json.load(open(os.path.join(GOLDEN, fixture)))
    z = np.load(os.path.join(GOLDEN, f"{ep['mesh']}.npz"))
    t = MeshTopology(z["coords"], z["cells"])
    t = MeshTopology(smooth_coords(t, 50), t.cells)
    out = []
    for g in ep["steps"]:
        x, cells = remove_vertex_delaunay(t.coords, np.flatnonzero(t.on_boundary), g["removed_vertex"])
        t = MeshTopology(x, cells)
        t = MeshTopology(smooth_coords(t, 50), t.cells)
        assert (t.nv, t.nt) == (g["nv"], g["nt"])
        out.append(t)
    return ep["mesh"], out


def _interpolate(src, pts, np1=None, NP=None, NP1=None, cellrec=True, split=False, src_of_env=None):
    """One `mdq_interpolate_snapshots` launch over B = len(pts) point sets.  `src`: one Src (the shared source) or a list
    of them + `src_of_env` (ABI 8).  np1[b] (default: all points) = points that also get a pressure; `split`: pass np1 as
    `npts` and the rest as `npts_extra`.  Outputs start as NaN / CELL_SENTINEL.  -> host (out_u, out_p, out_cell)."""
    from meshdqn_amd import _lib
    lib = _lib.load()
    B = len(pts)
    npts = np.array([len(q) for q in pts], np.int32)
    np1 = npts.copy() if np1 is None else np.asarray(np1, np.int32)
    NP = NP or int(npts.max())
    NP1 = NP1 or NP
    h = np.zeros((B, NP, 2))
    for b, q in enumerate(pts):
        h[b, :len(q)] = q
    dev = torch.device("cuda")
    keep = dict(points=torch.from_numpy(h).to(dev),
                npts=torch.from_numpy(np1 if split else npts).to(dev),
                extra=torch.from_numpy(npts - np1).to(dev),
                np1=torch.from_numpy(np1).to(dev),
                out_u=torch.full((B, S, NP, 2), float("nan"), dtype=torch.float64, device=dev),
                out_p=torch.full((B, S, NP1), float("nan"), dtype=torch.float64, device=dev),
                out_cell=torch.full((B, NP), CELL_SENTINEL, dtype=torch.int32, device=dev))
    d = _lib.InterpDesc()
    d.B, d.S, d.NP, d.NP1 = B, S, NP, NP1
    if src_of_env is None:
        src.fill(d, cellrec)
    else:
        recs = (_lib.InterpSrc * len(src))()
        for r, s in zip(recs, src):
            s.fill(r, cellrec)
        keep["srcs"] = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(dev)
        keep["src_of_env"] = torch.tensor(src_of_env, dtype=torch.int32, device=dev)
        d.n_src, d.srcs, d.src_of_env = len(src), keep["srcs"].data_ptr(), keep["src_of_env"].data_ptr()
    d.points, d.npts, d.np1 = keep["points"].data_ptr(), keep["npts"].data_ptr(), keep["np1"].data_ptr()
    if split:
        d.npts_extra = keep["extra"].data_ptr()
    d.out_u, d.out_p, d.out_cell = keep["out_u"].data_ptr(), keep["out_p"].data_ptr(), keep["out_cell"].data_ptr()
    _lib.check(lib.mdq_interpolate_snapshots(C.byref(d), _lib.stream_ptr()), "mdq_interpolate_snapshots")
    torch.cuda.synchronize()
    return keep["out_u"].cpu().numpy(), keep["out_p"].cpu().numpy(), keep["out_cell"].cpu().numpy()


def _check(src, pts, u, p, cell, np1=None, what=""):
    """One environment's outputs (u (S, >=m, 2), p (S, >=np1), cell (>=m,)) against the brute-force reference.
    -> the global violation of every point (0 inside a cell, < 0 outside all of them)."""
    m = len(pts)
    np1 = m if np1 is None else np1
    u, p, cell = u[:, :m], p[:, :np1], cell[:m]
    ref_cell, lam, viol = brute_locate(pts, src.x, src.topo.cells, device="cuda")
    U, P = p2p1_eval(lam, src.dofs[ref_cell], src.u, src.p)
    for s in range(S):
        su, sp = np.abs(src.u[s]).max(), np.abs(src.p[s]).max()
        eu, ep = np.abs(u[s] - U[s]).max(), np.abs(p[s] - P[s, :np1]).max(initial=0.0)
        assert eu <= TOL * su and ep <= TOL * sp, (what, s, eu / su, ep / sp)
    Ue, Pe = src.exact(pts)
    for j in range(2):
        s = 2 + j
        eu, ep = np.abs(u[s] - Ue[j]).max(), np.abs(p[s] - Pe[j, :np1]).max(initial=0.0)
        assert eu <= TOL * np.abs(src.u[s]).max() and ep <= TOL * np.abs(src.p[s]).max(), (what, "polynomial", s, eu, ep)
    assert ((cell >= 0) & (cell < src.topo.nt)).all(), what
    got = barycentrics(pts, src.x, src.topo.cells, cell).min(axis=1)
    assert got.min() >= -BAND, (what, int(np.argmin(got)), got.min(), viol[np.argmin(got)])
    return viol


def _point_sets(src, rng):
    """(a) random points in random cells, (b) every vertex and edge midpoint, (c) random fractions along edges,
    (d) the location grid's lines and corners that lie in the domain (up to round-off)."""
    t, x = src.topo, src.x
    cid = rng.integers(0, t.nt, 2000)
    a = np.einsum("mk,mkc->mc", rng.dirichlet(np.ones(3), cid.size), x[t.cells[cid]])
    b = t.dof_coords()
    e = t.edges[rng.integers(0, t.ne, 2500)]
    f = rng.random((e.shape[0], 1))
    c = x[e[:, 0]] + f * (x[e[:, 1]] - x[e[:, 0]])
    gxs = src.x0 + np.arange(src.gnx + 1) / src.inv_hx
    gys = src.y0 + np.arange(src.gny + 1) / src.inv_hy
    lo, hi = x.min(axis=0), x.max(axis=0)
    corners = np.stack(np.meshgrid(gxs, gys, indexing="ij"), axis=-1).reshape(-1, 2)
    vlines = np.stack([np.repeat(gxs, 8), rng.uniform(lo[1], hi[1], 8 * gxs.size)], axis=1)
    hlines = np.stack([rng.uniform(lo[0], hi[0], 8 * gys.size), np.repeat(gys, 8)], axis=1)
    d = np.concatenate([corners, vlines, hlines])
    _, _, viol = brute_locate(d, x, t.cells, device="cuda")
    return dict(a=a, b=b, c=c, d=d[viol >= -BAND])


@pytest.mark.parametrize("name", ["ys930", "ah93w145", "ys930_refined"])
def test_interpolation_matches_brute_force(sources, name):
    """Sets (a)-(d) of `_point_sets` as four environments of one launch: values, polynomial snapshots, located cells."""
    src = sources[name]
    sets = _point_sets(src, np.random.default_rng(100))
    assert len(sets["d"]) > 1000
    u, p, cell = _interpolate(src, list(sets.values()))
    for b, (k, pts) in enumerate(sets.items()):
        viol = _check(src, pts, u[b], p[b], cell[b], what=f"{name} set {k}")
        assert viol.min() >= -BAND, (k, viol.min())
        print(f"{name} set {k}: {len(pts)} points, {(viol < 0).sum()} in the round-off band (worst {viol.min():.2e})")


@pytest.mark.parametrize("fixture", ["oracle_episode.json", "oracle_episode_ah93w145.json"])
def test_golden_episode_dof_points(sources, fixture):
    """The real workload: the P2 dof points of the coarsened mesh after every step of a golden episode (48 environments of
    one launch, ragged), vertices with pressures.  None of them lies outside every source cell by more than round-off."""
    mesh, topos = _episode(fixture)
    src = sources[mesh]
    pts = [t.dof_coords() for t in topos]
    np1 = [t.nv for t in topos]
    u, p, cell = _interpolate(src, pts, np1=np1, NP1=max(np1))
    viol = np.concatenate([_check(src, q, u[b], p[b], cell[b], np1=np1[b], what=f"{fixture} step {b}")
                           for b, q in enumerate(pts)])
    band = int((viol < 0).sum())
    print(f"{fixture}: {viol.size} target points, {band} ({100 * band / viol.size:.1f} %) outside every source cell by "
          f"round-off only, worst {viol.min():.2e}")
    assert viol.min() >= -BAND
    assert 0 < band < 0.05 * viol.size      # (shared / boundary edges: the band the "no containing cell" branch serves)


def test_cell_records_and_gather_path_agree(sources):
    """`src_cellrec` NULL (candidate data gathered from src_cell_dofs / src_coords / src_geom) against the record table."""
    src = sources["ys930_refined"]
    sets = _point_sets(src, np.random.default_rng(7))
    pts = [sets["a"], sets["b"], sets["d"]]
    r = _interpolate(src, pts)
    g = _interpolate(src, pts, cellrec=False)
    for b, q in enumerate(pts):
        _check(src, q, g[0][b], g[1][b], g[2][b], what=f"gather path, set {b}")
    # the same candidates in the same order with the same doubles (the records copy src_coords / src_geom): the same bits
    for x, y in zip(r, g):
        assert np.array_equal(x, y, equal_nan=True)


def test_ragged_batch_with_spare_capacity(sources):
    """B = 6, point counts that are no multiples of 256 (one env with a single point, one without pressures), NP / NP1
    beyond every count: what lies beyond npts / np1 keeps its NaN; the split counts (np1 as npts + the rest as
    npts_extra) give the same bits."""
    src = sources["ys930"]
    rng = np.random.default_rng(3)
    pool = np.concatenate(list(_point_sets(src, rng).values()))
    counts, np1 = [1, 255, 257, 1000, 37, 600], [1, 100, 257, 999, 0, 311]
    pts = [pool[rng.choice(len(pool), n, replace=False)] for n in counts]
    NP, NP1 = 1000 + 45, 1000 + 64
    u, p, cell = _interpolate(src, pts, np1=np1, NP=NP, NP1=NP1)
    for b, q in enumerate(pts):
        _check(src, q, u[b], p[b], cell[b], np1=np1[b], what=f"env {b}")
        assert np.isnan(u[b][:, counts[b]:]).all() and np.isnan(p[b][:, np1[b]:]).all(), b
        assert (cell[b][counts[b]:] == CELL_SENTINEL).all(), b
        assert np.isfinite(u[b][:, :counts[b]]).all() and np.isfinite(p[b][:, :np1[b]]).all(), b
    us, ps, cs = _interpolate(src, pts, np1=np1, NP=NP, NP1=NP1, split=True)
    assert np.array_equal(u, us, equal_nan=True) and np.array_equal(p, ps, equal_nan=True) and np.array_equal(cell, cs)


def test_per_environment_sources(sources):
    """ABI 8: srcs / src_of_env over the three sources, interleaved; every environment against its own source."""
    names = ["ys930", "ah93w145", "ys930_refined"]
    srcs = [sources[n] for n in names]
    of_env = [2, 0, 1, 0, 2]
    rng = np.random.default_rng(8)
    pts = []
    for b, i in enumerate(of_env):
        sets = _point_sets(srcs[i], rng)
        q = np.concatenate([sets["a"], sets["b"]])
        pts.append(q[rng.choice(len(q), 700 + 131 * b, replace=False)])
    np1 = [n // 3 for n in map(len, pts)]
    u, p, cell = _interpolate(srcs, pts, np1=np1, src_of_env=of_env)
    for b, (i, q) in enumerate(zip(of_env, pts)):
        _check(srcs[i], q, u[b], p[b], cell[b], np1=np1[b], what=f"env {b} <- {names[i]}")


def test_error_returns_launch_nothing(sources):
    from meshdqn_amd import _lib
    lib = _lib.load()
    src = sources["ys930"]
    dev = torch.device("cuda")
    pts = torch.from_numpy(src.topo.dof_coords()[None, :300].copy()).to(dev)
    n = torch.tensor([300], dtype=torch.int32, device=dev)
    out_u = torch.full((1, S, 300, 2), float("nan"), dtype=torch.float64, device=dev)
    out_p = torch.full((1, S, 300), float("nan"), dtype=torch.float64, device=dev)
    out_c = torch.full((1, 300), CELL_SENTINEL, dtype=torch.int32, device=dev)
    of_env = torch.zeros(1, dtype=torch.int32, device=dev)

    def desc(**kw):
        d = _lib.InterpDesc()
        d.B, d.S, d.NP, d.NP1 = 1, S, 300, 300
        src.fill(d)
        d.points, d.npts, d.np1 = pts.data_ptr(), n.data_ptr(), n.data_ptr()
        d.out_u, d.out_p, d.out_cell = out_u.data_ptr(), out_p.data_ptr(), out_c.data_ptr()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    r = _lib.InterpSrc()
    src.fill(r)
    recs = torch.frombuffer(bytearray(r), dtype=torch.uint8).to(dev)
    bad = {"B = 0": (desc(B=0), "bad arguments"), "B < 0": (desc(B=-2), "bad arguments"),
           "S = 0": (desc(S=0), "bad arguments"), "S < 0": (desc(S=-1), "bad arguments"),
           "sparse without af_facets": (desc(sparse=1, naf=n.data_ptr(), cell_dofs=src.interp.t["src_cell_dofs"].data_ptr(),
                                             NT=src.topo.nt, NAF=4), "af_facets"),
           "srcs without src_of_env": (desc(srcs=recs.data_ptr(), n_src=1), "src_of_env"),
           "src_of_env without srcs": (desc(src_of_env=of_env.data_ptr(), n_src=1), "src_of_env")}
    for what, (d, msg) in bad.items():
        rc = lib.mdq_interpolate_snapshots(C.byref(d), _lib.stream_ptr())
        err = (lib.mdq_last_error() or b"").decode()
        assert rc != 0 and msg in err and "mdq_interpolate_snapshots" in err, (what, rc, err)
    torch.cuda.synchronize()
    assert torch.isnan(out_u).all() and torch.isnan(out_p).all() and (out_c == CELL_SENTINEL).all()
    # (the same descriptor, well formed, does launch)
    assert lib.mdq_interpolate_snapshots(C.byref(desc()), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out_u).all() and (out_c >= 0).all()


@pytest.mark.parametrize("name", ["ys930", "ah93w145"])
def test_points_outside_the_domain_extrapolate_bin_locally(sources, name):
    """The contract outside the domain (never reached by the environment, see test_golden_episode_dof_points): beyond the
    far-field box the bin is clamped to the grid's edge, deep inside the airfoil the bin is empty and holds only the cell
    with the centroid nearest to the bin's centre; the kernel extrapolates the P2 / P1 fields of the least violated
    candidate of that bin - finite values, a valid cell, exactly that cell's polynomials."""
    src = sources[name]
    t, x = src.topo, src.x
    lo, hi = x.min(axis=0), x.max(axis=0)
    s = np.linspace(0.0, 1.0, 9)
    far = np.concatenate([np.stack([np.full(9, lo[0] - 0.7), lo[1] + s * (hi[1] - lo[1])], 1),
                          np.stack([np.full(9, hi[0] + 1.3), lo[1] - 0.2 + s * (hi[1] - lo[1] + 0.4)], 1),
                          np.stack([lo[0] + s * (hi[0] - lo[0]), np.full(9, lo[1] - 0.4)], 1),
                          np.stack([lo[0] - 0.3 + s * (hi[0] - lo[0] + 0.6), np.full(9, hi[1] + 2.0)], 1),
                          [lo - 1.0, hi + 1.0, (lo[0] - 5.0, hi[1] + 5.0)]])
    # centres of the bins that no cell's bounding box touches (one candidate) and that lie well outside every cell
    gy, gx = np.divmod(np.arange(src.gnx * src.gny), src.gnx)
    centres = np.stack([src.x0 + (gx + 0.5) / src.inv_hx, src.y0 + (gy + 0.5) / src.inv_hy], axis=1)
    one = np.diff(src.bin_ptr) == 1
    _, _, v = brute_locate(centres[one], x, t.cells, device="cuda")
    hole = centres[one][v < -0.05]
    X = x[t.cells]
    X0, X1 = X.min(axis=1), X.max(axis=1)
    bins = src.bin_of(hole)
    bgy, bgx = np.divmod(bins, src.gnx)
    blo = np.stack([src.x0 + bgx / src.inv_hx, src.y0 + bgy / src.inv_hy], 1)
    bhi = np.stack([src.x0 + (bgx + 1) / src.inv_hx, src.y0 + (bgy + 1) / src.inv_hy], 1)
    touched = ((X0[None] <= bhi[:, None] + 1e-6) & (X1[None] >= blo[:, None] - 1e-6)).all(axis=2).any(axis=1)
    hole = hole[~touched]
    assert len(hole) >= 3, len(hole)
    pts = np.concatenate([far, hole])
    _, _, viol = brute_locate(pts, x, t.cells, device="cuda")
    assert viol.max() < -1e-3
    u, p, cell = _interpolate(src, [pts])
    u, p, cell = u[0], p[0], cell[0]
    assert np.isfinite(u).all() and np.isfinite(p).all()
    assert ((cell >= 0) & (cell < t.nt)).all()
    # the cell: the least violated candidate of the point's (clamped) bin
    bins = src.bin_of(pts)
    for k, b in enumerate(bins):
        cand = src.bin_cells[src.bin_ptr[b]:src.bin_ptr[b + 1]]
        assert cell[k] in cand, k
        m = barycentrics(np.repeat(pts[k:k + 1], len(cand), 0), x, t.cells, cand).min(axis=1)
        mk = m[list(cand).index(cell[k])]
        assert mk >= m.max() - 1e-9 * abs(m.max()), (k, mk, m.max())
    # in the empty bins: the cell whose centroid is nearest to the bin's centre
    cent = X.mean(axis=1)
    nh = len(hole)
    nearest = np.argmin(((hole[:, None] - cent[None]) ** 2).sum(-1), axis=1)
    assert np.array_equal(cell[-nh:], nearest)
    # the values: that cell's P2 / P1 polynomials, evaluated far from it
    lam = barycentrics(pts, x, t.cells, cell)
    U, P = p2p1_eval(lam, src.dofs[cell], src.u, src.p)
    grow = (1.0 + np.abs(lam).max(axis=1)) ** 2
    for s in range(S):
        assert (np.abs(u[s] - U[s]).max(axis=1) <= 1e-12 * grow * np.abs(src.u[s]).max()).all(), s
        assert (np.abs(p[s] - P[s]) <= 1e-12 * grow * np.abs(src.p[s]).max()).all(), s
    print(f"{name}: {len(far)} points beyond the far field, {nh} in empty bins of the airfoil, worst violation "
          f"{viol.min():.2f}")


def test_probe_forces_on_a_ragged_batch(sources):
    """One LightMeshBatch (the probes of the env step) over stock ys930, ah93w145, two ys930 meshes of the golden episode
    and the red-refined ys930, 8 fields: 3 random (against oracle/fem.py) + the 5 closed forms; dofs beyond every mesh
    are NaN (an index into another environment's or the padding's entries shows)."""
    from meshdqn_amd.mesh_ops import LightMeshBatch
    from oracle.fem import TaylorHood
    from oracle.mesh import OracleMesh
    _, ep = _episode("oracle_episode.json")
    topos = [sources["ys930_refined"].topo, ep[46], sources["ah93w145"].topo, sources["ys930"].topo, ep[10]]
    lb = LightMeshBatch(topos, [t.coords for t in topos], MU, device="cuda")
    B, NR = len(topos), 3
    rng = np.random.default_rng(21)
    cases, ths = [], []
    F = NR + 5
    u = np.full((B, F, lb.N2, 2), np.nan)
    p = np.full((B, F, lb.cap["NV"]), np.nan)
    for b, t in enumerate(topos):
        th = TaylorHood(OracleMesh(t.coords, t.cells), mu=MU)
        assert np.array_equal(th.mesh.edges, t.edges)
        ths.append(th)
        area = airfoil_area(t.coords, t.cells, [th.mesh.edge_cells[e][0] for e in th.airfoil_facets()])
        u[b, :NR, :t.np2] = rng.standard_normal((NR, t.np2, 2))
        p[b, :NR, :t.nv] = rng.standard_normal((NR, t.nv))
        cf = closed_form_fields(t.dof_coords(), t.nv, MU, area)
        for f, (_, uf, pf, _, _) in enumerate(cf):
            u[b, NR + f, :t.np2], p[b, NR + f, :t.nv] = uf, pf
        cases.append((area, cf))
    drag, lift = lb.probe_forces(torch.from_numpy(u).cuda(), torch.from_numpy(p).cuda())
    drag, lift = drag.cpu().numpy(), lift.cpu().numpy()
    for b, (t, th, (area, cf)) in enumerate(zip(topos, ths, cases)):
        for f in range(NR):
            do, lo = th.forces(interleaved_to_oracle_vel(u[b, f, :t.np2]), p[b, f, :t.nv])
            assert abs(drag[b, f] - do) <= 1e-12 * max(1.0, abs(do)), (b, f, drag[b, f], do)
            assert abs(lift[b, f] - lo) <= 1e-12 * max(1.0, abs(lo)), (b, f, lift[b, f], lo)
        for f, (what, _, _, dr, li) in enumerate(cf):
            tol = 1e-12 * max(1.0, area)
            assert abs(drag[b, NR + f] - dr) <= tol and abs(lift[b, NR + f] - li) <= tol, (b, what, drag[b, NR + f], dr,
                                                                                          lift[b, NR + f], li)
