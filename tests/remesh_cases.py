"""Hand-built meshes for the vertex removal (`mdq_remesh` on the device, `mdq_remesh_host` on the host) and its oracle, the
reference's `_remove_vertex` (Env2DAirfoil.py:452-512): drop the vertex, Delaunay-triangulate ALL remaining points with
scipy / Qhull, drop the simplices made of boundary vertices only.  numpy and scipy only, fixed seeds, no files.

Every mesh is `interior` points plus boundary points ON A CIRCLE, triangulated once by `scipy.spatial.Delaunay`, cells
ascending, int32.  Three boundary points have the boundary circle as their circumcircle and that circle holds every interior
point, so Qhull never forms an all-boundary simplex: the reference's filter drops nothing before or after a removal, and the
engines' premise that the boundary never changes holds by construction.  The builders assert that (and that every point is
used, and that the oracle returns `nt - 2` cells for every valid removal) instead of trusting it: a seed that breaks a
precondition is replaced, the assertion stays.

Vertex order: first half of the interior points, the boundary, second half of the interior points - so id 0 and id `nv - 1`
are both interior (the two ends of the engines' renumbering) and the boundary ids shift when a low id leaves.

No case comes near the engines' guard of 200 000 work-list pops: the host counts every interior edge against it and the
device only the violating ones, so the codes of the two differ there.  That mismatch is known and not tested."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np
from scipy.spatial import Delaunay

SENTINEL_ID = -7                      # rows beyond nt; rows beyond nv hold NaN


@dataclass
class Case:
    name: str
    coords: np.ndarray                # (nv, 2) f8
    cells: np.ndarray                 # (nt, 3) i4, every row ascending
    boundary: np.ndarray              # ids of the vertices on the circle
    removals: tuple                   # the valid removals of this case
    info: dict = field(default_factory=dict)

    @property
    def nv(self):
        return self.coords.shape[0]

    @property
    def nt(self):
        return self.cells.shape[0]

    @property
    def interior(self):
        return np.setdiff1d(np.arange(self.nv), self.boundary)


# ------------------------------------------------------------------------------------------------ geometry helpers
def circle(n: int, radius: float, phase: float = 0.0) -> np.ndarray:
    a = 2.0 * np.pi * (np.arange(n) + phase) / n
    return radius * np.stack([np.cos(a), np.sin(a)], axis=1)


def disc(rng, n: int, radius: float) -> np.ndarray:
    r = radius * np.sqrt(rng.random(n))
    a = 2.0 * np.pi * rng.random(n)
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=1)


def orient2d(x, cells):
    """Doubled signed areas, operation by operation as the engines compute them."""
    a, b, c = x[cells[:, 0]], x[cells[:, 1]], x[cells[:, 2]]
    return (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])


def canon(cells) -> np.ndarray:
    """Cells as a set: every row ascending, rows in lexicographic order (equal arrays <=> equal multisets of cells)."""
    c = np.sort(np.asarray(cells, dtype=np.int64), axis=1)
    return c[np.lexsort((c[:, 2], c[:, 1], c[:, 0]))]


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """Bitwise equality (NaN padding included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def edge_pairs(cells):
    """Interior edges of a triangle list: (t, u, a, b, c, d) arrays - cells t < u share edge (b, c), a is t's third vertex,
    d is u's.  Raises when an edge has more than two owners."""
    cells = np.asarray(cells, dtype=np.int64)
    nt = cells.shape[0]
    t = np.repeat(np.arange(nt), 3)
    k = np.tile(np.arange(3), nt)
    apex = cells[t, k]
    e0, e1 = cells[t, (k + 1) % 3], cells[t, (k + 2) % 3]
    key = np.minimum(e0, e1) * (cells.max() + 1) + np.maximum(e0, e1)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    uniq, start, count = np.unique(ks, return_index=True, return_counts=True)
    if (count > 2).any():
        raise ValueError("an edge with more than two owners")
    first = order[start[count == 2]]
    second = order[start[count == 2] + 1]
    single = order[start[count == 1]]
    bnd = np.stack([np.minimum(e0, e1)[single], np.maximum(e0, e1)[single]], axis=1)
    return (t[first], t[second], apex[first], e0[first], e1[first], apex[second]), bnd


def violating_edges(x, cells) -> int:
    """Interior edges that fail the empty-circle test, with the engines' floating-point incircle."""
    (t, u, a, b, c, d), _ = edge_pairs(cells)
    A, B, Cc, D = x[a], x[b], x[c], x[d]
    s = np.sign((B[:, 0] - A[:, 0]) * (Cc[:, 1] - A[:, 1]) - (B[:, 1] - A[:, 1]) * (Cc[:, 0] - A[:, 0]))
    ax, ay = A[:, 0] - D[:, 0], A[:, 1] - D[:, 1]
    bx, by = B[:, 0] - D[:, 0], B[:, 1] - D[:, 1]
    cx, cy = Cc[:, 0] - D[:, 0], Cc[:, 1] - D[:, 1]
    det = (ax * ax + ay * ay) * (bx * cy - by * cx) - (bx * bx + by * by) * (ax * cy - ay * cx) \
        + (cx * cx + cy * cy) * (ax * by - ay * bx)
    return int((s * det > 0).sum())


def ring_of(case: Case, rv: int):
    """The star polygon of an interior vertex, counter-clockwise."""
    x, nxt = case.coords, {}
    for row in case.cells[(case.cells == rv).any(axis=1)].tolist():
        k = row.index(rv)
        a, b = row[(k + 1) % 3], row[(k + 2) % 3]
        if (x[a, 0] - x[rv, 0]) * (x[b, 1] - x[rv, 1]) - (x[a, 1] - x[rv, 1]) * (x[b, 0] - x[rv, 0]) < 0:
            a, b = b, a
        nxt[a] = b
    start = min(nxt)
    ring, cur = [start], nxt[start]
    while cur != start:
        ring.append(cur)
        cur = nxt[cur]
    assert len(ring) == len(nxt)
    return ring


def reflex_corners(case: Case, rv: int) -> int:
    ring = ring_of(case, rv)
    p = case.coords[ring]
    a, b, c = np.roll(p, 1, axis=0), p, np.roll(p, -1, axis=0)
    return int(((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0]) <= 0).sum())


def degree(case: Case, v: int) -> int:
    return int((case.cells == v).any(axis=1).sum())


# ------------------------------------------------------------------------------------------------ the oracle
def _delaunay(points, boundary):
    """(cells ascending int32, number of all-boundary simplices the reference's filter drops)."""
    s = Delaunay(points).simplices
    allb = np.sum(np.isin(s, boundary), axis=1) == 3
    return np.sort(s[~allb], axis=1).astype(np.int32), int(allb.sum())


_ORACLE = {}


def oracle(case: Case, rv: int):
    """The reference's `_remove_vertex`: (coords, cells) of the global scipy / Qhull Delaunay without vertex rv.  Computed once
    per (case, rv), shared by the tests and never written to; asserts the preconditions of a valid removal."""
    key = (case.name, int(rv))
    if key not in _ORACLE:
        bv = case.boundary.copy()
        bv[bv > rv] -= 1
        keep = np.ones(case.nv, dtype=bool)
        keep[rv] = False
        pts = case.coords[keep]
        cells, dropped = _delaunay(pts, bv)
        assert dropped == 0, (key, dropped)
        assert cells.shape[0] == case.nt - 2, (key, cells.shape[0], case.nt)
        assert np.unique(cells).size == case.nv - 1, key
        pts.setflags(write=False)
        cells.setflags(write=False)
        _ORACLE[key] = (pts, cells)
    return _ORACLE[key]


def _mesh(name, interior, boundary, removals=None, **info) -> Case:
    ni, h = interior.shape[0], interior.shape[0] // 2
    pts = np.ascontiguousarray(np.concatenate([interior[:h], boundary, interior[h:]]))
    bv = np.arange(h, h + boundary.shape[0])
    cells, dropped = _delaunay(pts, bv)
    assert dropped == 0, (name, dropped)
    assert np.unique(cells).size == pts.shape[0], name
    assert cells.shape[0] == 2 * ni + boundary.shape[0] - 2, name
    case = Case(name, pts, cells, bv, (), dict(info))
    case.removals = tuple(removals(case)) if removals else ()
    return case


# ------------------------------------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=None)
def hub(n: int) -> Case:
    """A hub of degree n at the origin: n ring points at radius 1 and 2n at radius 2 (radial jitter 1e-3), 48 boundary points
    at radius 3.  Removing the hub leaves a near-cocircular n-gon: ear clipping makes a fan that Lawson largely undoes.  The
    star buffer holds 64 cells: 63 and 64 are removed, 65 is refused (-1)."""
    rng = np.random.default_rng(1000 + n)
    r1 = circle(n, 1.0) * (1.0 + 1e-3 * (2.0 * rng.random(n) - 1.0))[:, None]
    r2 = circle(2 * n, 2.0, 0.25) * (1.0 + 1e-3 * (2.0 * rng.random(2 * n) - 1.0))[:, None]
    case = _mesh(f"hub{n}", np.concatenate([np.zeros((1, 2)), r1, r2]), circle(48, 3.0, 0.5),
                 removals=lambda c: (0,) if n <= 64 else ())
    assert np.array_equal(case.coords[0], [0.0, 0.0]) and degree(case, 0) == n
    case.info.update(hub_degree=n, violating=violating_edges(case.coords, case.cells))
    return case


SHAKEN_SEED = 7
AREA_FLOOR = 0.05                     # of the mean cell area: the smallest cell the shaking may leave (a cell that was
AREA_KEEP = 0.25                      # smaller before keeps this share of its own area)


@functools.lru_cache(maxsize=None)
def shaken() -> Case:
    """300 random points in a disc inside a 64-point circle, every interior vertex then moved by up to half the mean cell size
    (a vertex' displacement is halved while one of its cells would flip or fall under the area floor): a valid triangulation
    that is neither Delaunay nor star-convex.  Removals: the lowest, a middle and the highest interior id."""
    rng = np.random.default_rng(SHAKEN_SEED)
    base = _mesh("shaken", disc(rng, 300, 0.85), circle(64, 1.0))
    x0, cells = base.coords, base.cells.astype(np.int64)
    area0 = orient2d(x0, cells)
    sign = np.sign(area0)
    assert (sign != 0).all()
    mean2 = np.abs(area0).mean()                          # doubled mean area
    h = np.sqrt(mean2)                                    # ~ an edge length
    ang = 2.0 * np.pi * rng.random(base.nv)
    disp = (0.5 * h * rng.random(base.nv))[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    disp[base.boundary] = 0.0
    floor = np.minimum(AREA_FLOOR * mean2, AREA_KEEP * np.abs(area0))
    for _ in range(60):
        bad = sign * orient2d(x0 + disp, cells) < floor
        if not bad.any():
            break
        disp[np.unique(cells[bad])] *= 0.5
    x = x0 + disp
    assert (sign * orient2d(x, cells) >= floor).all() and (floor > 0).all()
    assert (np.hypot(x[:, 0], x[:, 1])[base.interior] < 0.97).all()
    inter = base.interior
    case = Case("shaken", np.ascontiguousarray(x), base.cells, base.boundary,
                (int(inter[0]), int(inter[inter.size // 2]), int(inter[-1])))
    assert case.removals[0] == 0 and case.removals[2] == case.nv - 1
    nviol = violating_edges(case.coords, case.cells)
    # (a condition, not a measurement: the device sorts its initial work list by insertion on one lane, and these tests are
    # not a timing test of that sort)
    assert 100 <= nviol <= 512, nviol
    reflex = [reflex_corners(case, rv) for rv in case.removals]
    assert max(reflex) >= 1, reflex
    case.info.update(violating=nviol, reflex=reflex, degrees=[degree(case, rv) for rv in case.removals])
    return case


FULL_BOUNDARY = {1024: 96, 4096: 192, 16384: 384}


@functools.lru_cache(maxsize=None)
def full(NV: int) -> Case:
    """A mesh of exactly NV vertices, the vertex limit of one capacity instance of the device kernel (ids up to NV - 1 in the
    edge keys; 12 093 edges in the 16 384-slot hash at NV = 4096).  Removals: id 0 and the last interior id, NV - 1."""
    nb = FULL_BOUNDARY[NV]
    rng = np.random.default_rng(NV)
    case = _mesh(f"full{NV}", disc(rng, NV - nb, 0.98), circle(nb, 1.0), removals=lambda c: (0, c.nv - 1))
    assert case.nv == NV and case.nt == 2 * NV - nb - 2
    assert not np.isin(case.removals, case.boundary).any()
    case.info.update(violating=violating_edges(case.coords, case.cells))
    return case


@functools.lru_cache(maxsize=None)
def grid() -> Case:
    """A 9 x 9 lattice of spacing 1/8 inside a 40-point unit circle: exact incircle ties, so the Delaunay triangulation is NOT
    unique and neither scipy nor the other engine is a reference - the result goes through `check_delaunay_exact`.  Removal:
    the centre."""
    g = (np.arange(9) - 4) / 8.0
    lattice = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    case = _mesh("grid", lattice, circle(40, 1.0, 0.5))
    centre = int(np.flatnonzero((case.coords == 0.0).all(axis=1))[0])
    assert centre not in case.boundary
    case.removals = (centre,)
    case.info.update(violating=violating_edges(case.coords, case.cells), degrees=[degree(case, centre)])
    return case


@functools.lru_cache(maxsize=None)
def duplicated() -> tuple:
    """The shaken mesh with one cell outside the star (and the ring) of the removed vertex appended a second time: its edges
    have three owners, which both engines refuse with -11 AFTER the cavity has been re-triangulated."""
    base = shaken()
    rv = base.removals[1]
    near = np.unique(base.cells[(base.cells == rv).any(axis=1)])
    far = np.flatnonzero(~np.isin(base.cells, near).any(axis=1) & ~np.isin(base.cells, base.boundary).any(axis=1))
    cells = np.concatenate([base.cells, base.cells[far[:1]]])
    return Case("duplicated", base.coords, cells, base.boundary, ()), rv


def refusals():
    """(name, case, rv, status): removals that must be refused with exactly this code and leave the mesh untouched ("nothing",
    rv = -1, is no refusal: status 0, mesh untouched).  -4 and -12 need invalid geometry or tens of thousands of flips and are
    not reached."""
    s = shaken()
    dup, rv = duplicated()
    return [("boundary", s, int(s.boundary[5]), -3),
            ("absent", s, s.nv + 3, -2),
            ("nothing", s, -1, 0),
            ("hub65", hub(65), 0, -1),
            ("duplicated", dup, rv, -11)]


def valid():
    """(case, rv) of every removal that is compared with the oracle at the smallest capacity."""
    return [(c, rv) for c in (hub(63), hub(64), shaken()) for rv in c.removals]


# ------------------------------------------------------------------------------------------------ padded arrays
def pad(case: Case, NV: int, NT: int):
    """(coords (NV, 2), cells (NT, 3)) of a case in arrays of the given capacities, the rows beyond nv / nt a sentinel: NaN
    coordinates, ids of -7."""
    assert case.nv <= NV and case.nt <= NT, (case.name, NV, NT)
    x = np.full((NV, 2), np.nan)
    c = np.full((NT, 3), SENTINEL_ID, dtype=np.int32)
    x[:case.nv] = case.coords
    c[:case.nt] = case.cells
    return x, c


def batch(items, NV: int, NT: int):
    """Padded arrays of a list of (case, rv): coords (B, NV, 2), cells (B, NT, 3), nv, nt, rv (B,) int32."""
    xs, cs = zip(*(pad(c, NV, NT) for c, _ in items))
    return (np.stack(xs), np.stack(cs), np.array([c.nv for c, _ in items], np.int32),
            np.array([c.nt for c, _ in items], np.int32), np.array([rv for _, rv in items], np.int32))


def padding_intact(x, c, nv: int, nt: int) -> bool:
    return bool(np.isnan(x[nv:]).all() and same_bits(x[nv:], np.full_like(x[nv:], np.nan)) and (c[nt:] == SENTINEL_ID).all())


def mixed_batch():
    """The eight environments of the mixed launch: three hubs (the third refused), the shaken mesh with its three removals,
    a boundary refusal and a do-nothing.  (case, rv, status)."""
    s = shaken()
    return [(hub(63), 0, 0), (hub(64), 0, 0), (hub(65), 0, -1)] + [(s, rv, 0) for rv in s.removals] \
        + [(s, int(s.boundary[5]), -3), (s, -1, 0)]


# ------------------------------------------------------------------------------------------------ exact checker
def check_delaunay_exact(before: Case, rv: int, coords, cells) -> None:
    """Exact (rational arithmetic on the float coordinates) check of a removal's result where the Delaunay triangulation is
    not unique: nt - 2 non-degenerate cells on every remaining vertex, a manifold with the boundary edges of the mesh before
    the removal, the same total area, and every interior edge locally Delaunay (incircle <= 0)."""
    cells = np.asarray(cells, dtype=np.int64)
    assert coords.shape == (before.nv - 1, 2) and cells.shape == (before.nt - 2, 3)
    assert np.unique(cells).size == before.nv - 1 and cells.min() == 0 and cells.max() == before.nv - 2
    P = [(Fraction(float(px)), Fraction(float(py))) for px, py in coords]

    def orient(a, b, c):
        return (P[b][0] - P[a][0]) * (P[c][1] - P[a][1]) - (P[b][1] - P[a][1]) * (P[c][0] - P[a][0])

    def incircle(a, b, c, d):
        ax, ay, bx, by, cx, cy = (P[a][0] - P[d][0], P[a][1] - P[d][1], P[b][0] - P[d][0], P[b][1] - P[d][1],
                                  P[c][0] - P[d][0], P[c][1] - P[d][1])
        return (ax * ax + ay * ay) * (bx * cy - by * cx) - (bx * bx + by * by) * (ax * cy - ay * cx) \
            + (cx * cx + cy * cy) * (ax * by - ay * bx)

    def doubled_area(pts, cc):
        Q = [(Fraction(float(px)), Fraction(float(py))) for px, py in pts]
        tot = Fraction(0)
        for a, b, c in np.asarray(cc).tolist():
            w = (Q[b][0] - Q[a][0]) * (Q[c][1] - Q[a][1]) - (Q[b][1] - Q[a][1]) * (Q[c][0] - Q[a][0])
            assert w != 0
            tot += abs(w)
        return tot

    assert doubled_area(coords, cells) == doubled_area(before.coords, before.cells)
    (t, u, a, b, c, d), bnd = edge_pairs(cells)          # (raises on a third owner of an edge)
    _, bnd0 = edge_pairs(before.cells)
    assert not (bnd0 == rv).any()
    bnd0 = bnd0 - (bnd0 > rv)
    assert {tuple(e) for e in bnd.tolist()} == {tuple(e) for e in bnd0.tolist()}
    for a_, b_, c_, d_ in zip(a.tolist(), b.tolist(), c.tolist(), d.tolist()):
        s = orient(a_, b_, c_)
        assert s != 0 and orient(d_, c_, b_) * s > 0, "cells on one side of their common edge"
        if s < 0:
            b_, c_ = c_, b_
        assert incircle(a_, b_, c_, d_) <= 0, (a_, b_, c_, d_)
