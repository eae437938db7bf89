"""Generator of tests/golden/ipcs_ladder.npz: a ladder of synthetic channel meshes whose sizes sit ON the size switches
of the IPCS kernels (`python tests/golden/make_ipcs_ladder.py [OUT.npz]`).

Every mesh is the channel [-0.5, 3] x [-0.5, 0.5] with one convex hole (a polygon on an ellipse round (0.3, 0)), so that
`MeshTopology.facet_tags` finds walls, airfoil, inflow and outflow.  Boundary points are equally spaced at about the interior
spacing h; interior points are thrown (seeded `numpy.random.default_rng`) with a minimum distance of 0.75 h from each other
and 0.6 h from the boundaries and the hole; `scipy.spatial.Delaunay` triangulates, the cells whose centroid lies inside the
hole are dropped.  With one hole nt = 2 nv - nb and n2 = nv + ne = 4 nv - nb (nb boundary vertices): nb is adjusted through
the number of points on the outlet until the target is reachable, then the interior point count follows.

The targets (TARGETS below; tests/ipcs_ladder_cases.py names them the same way):
  nv64, nv65                      fewer triangles than two waves, fewer rows than threads
  nt512 ... nt1537                the round edges of atomic_accumulate (512- and 768-wide) and the tile size MF_CH = 1024
  outflow_heavy, outflow_collide  more than 768 outflow entries; the same mesh renumbered so that three outflow rows share a
                                  residue mod 512
  n2_3402 ... n2_5106             the capacity edges of the operator modes (ipcs_batch.operator_mode_limits)
The seeds are the first ones at which the oracle alone (tests/test_ipcs_ladder_cpu.py) stays bounded for three steps."""
import os
import sys

import numpy as np
from scipy.spatial import Delaunay

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

X0, X1, Y0, Y1 = -0.5, 3.0, -0.5, 0.5
HOLE_C, HOLE_A, HOLE_B = (0.3, 0.0), 0.16, 0.08

# name -> (kind of target, target, seed, outlet segments or None = about 1 / h)
TARGETS = {
    "nv64": ("nv", 64, 0, None), "nv65": ("nv", 65, 0, None),
    "nt512": ("nt", 512, 0, None), "nt513": ("nt", 513, 0, None), "nt768": ("nt", 768, 0, None), "nt769": ("nt", 769, 0, None),
    "nt1024": ("nt", 1024, 0, None), "nt1025": ("nt", 1025, 0, None), "nt1536": ("nt", 1536, 0, None),
    "nt1537": ("nt", 1537, 0, None),
    "outflow_heavy": ("n2", 1135, 0, 48),
    "n2_3402": ("n2", 3402, 0, None), "n2_3404": ("n2", 3404, 0, None), "n2_3584": ("n2", 3584, 0, None),
    "n2_3586": ("n2", 3586, 0, None), "n2_4096": ("n2", 4096, 0, None), "n2_4098": ("n2", 4098, 0, None),
    "n2_5104": ("n2", 5104, 0, None), "n2_5106": ("n2", 5106, 0, None),
}
COLLIDE_OF, COLLIDE_SEED = "outflow_heavy", 0


def hole_polygon(m):
    """m points on the ellipse, equally spaced in arc length, counter-clockwise."""
    t = np.linspace(0.0, 2.0 * np.pi, 20001)
    x, y = HOLE_C[0] + HOLE_A * np.cos(t), HOLE_C[1] + HOLE_B * np.sin(t)
    s = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(x), np.diff(y)))])
    at = np.interp(np.arange(m) * s[-1] / m, s, t)
    return np.stack([HOLE_C[0] + HOLE_A * np.cos(at), HOLE_C[1] + HOLE_B * np.sin(at)], axis=1)


def _perimeter():
    p = hole_polygon(2000)
    return float(np.hypot(*(np.roll(p, -1, axis=0) - p).T).sum())


HOLE_PERIMETER = _perimeter()


def inside_convex(poly, pts, margin=0.0):
    """pts strictly inside the counter-clockwise convex polygon grown by `margin` (distance to every edge line)."""
    a, b = poly, np.roll(poly, -1, axis=0)
    e = b - a
    n = np.stack([e[:, 1], -e[:, 0]], axis=1) / np.hypot(e[:, 0], e[:, 1])[:, None]     # outward normals
    d = ((pts[:, None, :] - a[None]) * n[None]).sum(axis=2)                             # signed distance to every edge line
    return (d < margin).all(axis=1)


def boundary_counts(h):
    """Segments on each wall, on the inlet and round the hole at spacing h."""
    return max(3, int(round((X1 - X0) / h))), max(2, int(round((Y1 - Y0) / h))), max(6, int(round(HOLE_PERIMETER / h)))


def boundary_points(h, nout):
    nx, nin, nh = boundary_counts(h)
    xs, yin, yout = np.linspace(X0, X1, nx + 1), np.linspace(Y0, Y1, nin + 1), np.linspace(Y0, Y1, nout + 1)
    outer = np.concatenate([np.stack([xs[:-1], np.full(nx, Y0)], 1), np.stack([np.full(nout, X1), yout[:-1]], 1),
                            np.stack([xs[:0:-1], np.full(nx, Y1)], 1), np.stack([np.full(nin, X0), yin[:0:-1]], 1)])
    return outer, hole_polygon(nh)


def plan(kind, target, nout_fixed):
    """The first spacing h (descending) at which the target is reachable with an interior point count at 70 - 85 % of one
    point per h x h: (h, outlet segments, nv, interior points)."""
    for h in np.geomspace(0.5, 0.02, 4000):
        base = nout_fixed if nout_fixed else max(2, int(round((Y1 - Y0) / h)))
        for nout in range(base, base + 4):
            nx, nin, nh = boundary_counts(h)
            nb = 2 * nx + nin + nout + nh
            if kind == "nv":
                nv = target
            elif (target + nb) % (2 if kind == "nt" else 4):
                continue
            else:
                nv = (target + nb) // (2 if kind == "nt" else 4)
            ni = nv - nb
            room = (X1 - X0 - 1.2 * h) * (Y1 - Y0 - 1.2 * h) - np.pi * (HOLE_A + 0.6 * h) * (HOLE_B + 0.6 * h)
            if ni > 0 and 0.70 <= ni * h * h / room <= 0.85:
                return float(h), nout, nv, ni
    raise RuntimeError(f"no spacing for {kind} = {target}")


def throw_interior(rng, h, ni, outer, hole):
    pts = np.zeros((ni, 2))
    fixed = np.concatenate([outer, hole])
    n = 0
    for _ in range(4000):
        cand = np.stack([rng.uniform(X0 + 0.6 * h, X1 - 0.6 * h, 256), rng.uniform(Y0 + 0.6 * h, Y1 - 0.6 * h, 256)], axis=1)
        ok = ~inside_convex(hole, cand, 0.6 * h)
        ok &= np.hypot(cand[:, None, 0] - fixed[None, :, 0], cand[:, None, 1] - fixed[None, :, 1]).min(axis=1) >= 0.6 * h
        for p in cand[ok]:
            if n and np.hypot(pts[:n, 0] - p[0], pts[:n, 1] - p[1]).min() < 0.75 * h:
                continue
            pts[n] = p
            n += 1
            if n == ni:
                return pts
    raise RuntimeError("interior points do not fit")


def make_mesh(kind, target, seed, nout_fixed=None):
    h, nout, nv, ni = plan(kind, target, nout_fixed)
    outer, hole = boundary_points(h, nout)
    rng = np.random.default_rng(seed)
    coords = np.concatenate([outer, hole, throw_interior(rng, h, ni, outer, hole)])
    tri = Delaunay(coords).simplices
    keep = ~inside_convex(hole, coords[tri].mean(axis=1))
    cells = np.sort(tri[keep], axis=1).astype(np.int32)
    check_mesh(coords, cells, len(outer) + len(hole), nout)
    sizes = mesh_sizes(coords, cells)
    assert sizes[kind] == target, (kind, target, sizes)
    return coords, cells


def mesh_sizes(coords, cells):
    e = np.sort(np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [0, 2]]]), axis=1)
    ne = len(np.unique(e, axis=0))
    return dict(nv=len(coords), nt=len(cells), ne=ne, n2=len(coords) + ne)


def cell_areas(coords, cells):
    x = coords[cells]
    e1, e2 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0]
    return 0.5 * np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])


def check_mesh(coords, cells, nb, nout):
    """Every point used, no flat cell, the boundary is exactly the nb boundary points (one outer ring + the hole), the outlet
    has its nout facets, and the counts obey nt = 2 nv - nb."""
    nv = len(coords)
    assert np.array_equal(np.unique(cells), np.arange(nv)), "a point is not used"
    assert cell_areas(coords, cells).min() > 1e-9, "flat cell"
    e = np.sort(np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [0, 2]]]), axis=1)
    ue, cnt = np.unique(e, axis=0, return_counts=True)
    assert cnt.max() == 2
    be = ue[cnt == 1]
    assert len(be) == nb and np.array_equal(np.unique(be), np.arange(nb)), "boundary edges are not the boundary polygons"
    assert (np.bincount(be.ravel(), minlength=nb) == 2).all()
    assert int((coords[be][:, :, 0] > X1 - 1e-12).all(axis=1).sum()) == nout
    assert len(cells) == 2 * nv - nb and len(ue) == 3 * nv - nb


def outflow_rows(coords, cells):
    """The P2 rows on the outlet: the vertices of the outflow facets and nv + edge id, in the edge numbering of MeshTopology."""
    from meshdqn_amd.topology import TAG_OUTFLOW, MeshTopology
    topo = MeshTopology(coords, cells)
    es = topo.boundary_edges[topo.facet_tags() == TAG_OUTFLOW]
    return np.unique(np.concatenate([topo.edges[es].ravel(), topo.nv + es]))


def renumber_to_collide(coords, cells, seed):
    """The same mesh with its vertices renumbered (a seeded permutation, the first of a sequence) such that at least three outflow
    rows share a residue mod 512."""
    rng = np.random.default_rng(seed)
    for _ in range(20000):
        perm = rng.permutation(len(coords))          # new id of old vertex i
        c2 = np.zeros_like(coords)
        c2[perm] = coords
        t2 = np.sort(perm[cells], axis=1).astype(np.int32)
        if np.bincount(outflow_rows(c2, t2) % 512, minlength=512).max() >= 3:
            return c2, t2
    raise RuntimeError("no colliding numbering found")


def build_all():
    out = {}
    for name, (kind, target, seed, nout) in TARGETS.items():
        out[name] = make_mesh(kind, target, seed, nout)
    out["outflow_collide"] = renumber_to_collide(*out[COLLIDE_OF], COLLIDE_SEED)
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "ipcs_ladder.npz")
    meshes = build_all()
    arrays = {}
    for name, (c, t) in meshes.items():
        arrays[f"{name}/coords"], arrays[f"{name}/cells"] = c.astype(np.float64), t.astype(np.int32)
        print(name, mesh_sizes(c, t), "outflow rows", len(outflow_rows(c, t)))
    np.savez_compressed(path, **arrays)
