"""Helpers shared by the parity tests (oracle <-> HIP layouts)."""
import numpy as np
import scipy.sparse as sp


def oracle_vel_to_interleaved(u, n2):
    """oracle velocity [ux | uy] (2*n2) -> ours (n2, 2)."""
    return np.stack([u[:n2], u[n2:]], axis=1)


def interleaved_to_oracle_vel(u):
    return np.concatenate([u[:, 0], u[:, 1]])


def device_velocity_matrix(rowptr, colidx, A1, idiag1, pos):
    """Rebuild the (unscaled) velocity operator in the oracle's [ux|uy] ordering
    from the device SELL block arrays (A1 is row-scaled by idiag1); `pos` maps
    CSR non-zeros to SELL positions."""
    n2 = rowptr.size - 1
    nnz = rowptr[-1]
    rows = np.repeat(np.arange(n2), np.diff(rowptr))
    cols = colidx[:nnz]
    blocks = []
    for c in range(2):
        row_blocks = []
        for d in range(2):
            vals = A1[pos, 2 * c + d] / idiag1[rows, c]
            row_blocks.append(sp.coo_matrix((vals, (rows, cols)), shape=(n2, n2)))
        blocks.append(row_blocks)
    return sp.bmat(blocks).tocsr()


def device_sym_matrix(rowptr, colidx, vals, sdiag, pos):
    n = rowptr.size - 1
    nnz = rowptr[-1]
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    cols = colidx[:nnz]
    v = vals[pos] * sdiag[rows] * sdiag[cols]
    return sp.coo_matrix((v, (rows, cols)), shape=(n, n)).tocsr()


# ---------------------------------------------------------------- independent fp64 references of the mesh-side kernels
# (point location + P2 / P1 evaluation of mdq_interpolate_snapshots, the airfoil area behind the closed forms of
# mdq_probe_forces).  Nothing here uses oracle/ or a stored Jacobian: barycentric coordinates are ratios of signed areas
# of the vertex coordinates, the bases are written out, and point location scans every cell.


def _cross(ax, ay, bx, by):
    return ax * by - ay * bx


def barycentrics(pts, coords, cells, which):
    """(m, 3) barycentric coordinates of pts (m, 2) in the cells `which` (m,), from signed areas."""
    X = np.asarray(coords, np.float64)[np.asarray(cells)[np.asarray(which)]]  # (m,3,2)
    a, b, c = X[:, 0] - pts, X[:, 1] - pts, X[:, 2] - pts
    e1, e2 = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
    det = _cross(e1[:, 0], e1[:, 1], e2[:, 0], e2[:, 1])
    return np.stack([_cross(b[:, 0], b[:, 1], c[:, 0], c[:, 1]), _cross(c[:, 0], c[:, 1], a[:, 0], a[:, 1]),
                     _cross(a[:, 0], a[:, 1], b[:, 0], b[:, 1])], axis=1) / det[:, None]


def brute_locate(pts, coords, cells, device="cpu", pairs=1 << 24):
    """Point location by a scan over ALL cells -> (cell, lam, viol) per point: the cell whose smallest barycentric
    coordinate is largest (the deepest containing cell), its barycentrics (m, 3), and the global violation
    min(0, max over cells of the smallest barycentric) - 0 when some cell contains the point, < 0 outside every cell.
    The points x cells scan runs as fp64 torch element-wise operations (IEEE-exact, the same numbers as numpy) on
    `device`: a golden episode is ~10^8 (point, cell) pairs."""
    import torch
    X = torch.as_tensor(np.asarray(coords, np.float64)[np.asarray(cells)], device=device)  # (nt,3,2)
    e1, e2 = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
    det = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    P = torch.as_tensor(np.asarray(pts, np.float64), device=device)
    cell = torch.empty(P.shape[0], dtype=torch.int64, device=device)
    best = torch.empty(P.shape[0], dtype=torch.float64, device=device)
    step = max(1, pairs // X.shape[0])
    for s in range(0, P.shape[0], step):
        px, py = P[s:s + step, 0:1], P[s:s + step, 1:2]
        ax, ay = X[None, :, 0, 0] - px, X[None, :, 0, 1] - py
        bx, by = X[None, :, 1, 0] - px, X[None, :, 1, 1] - py
        cx, cy = X[None, :, 2, 0] - px, X[None, :, 2, 1] - py
        mn = torch.minimum(torch.minimum((bx * cy - by * cx) / det, (cx * ay - cy * ax) / det), (ax * by - ay * bx) / det)
        best[s:s + step], cell[s:s + step] = mn.max(dim=1)
    cell = cell.cpu().numpy()
    return cell, barycentrics(pts, coords, cells, cell), np.minimum(best.cpu().numpy(), 0.0)


def p2_cell_dofs(topo):
    """The (nt, 6) P2 dof table of a MeshTopology, checked against the layout the formulas of `p2p1_eval` assume:
    dofs 0-2 the cell's vertices, dof 3 + k the midpoint of the edge OPPOSITE vertex k (edge dof = nv + edge id)."""
    cd = np.asarray(topo.cell_dofs)
    c = np.asarray(topo.cells)
    assert np.array_equal(cd[:, :3], c)
    for k, (a, b) in enumerate(((1, 2), (0, 2), (0, 1))):
        e = np.sort(topo.edges[cd[:, 3 + k] - topo.nv], axis=1)
        assert np.array_equal(e, np.sort(c[:, [a, b]], axis=1)), k
    return cd


def p2p1_eval(lam, dofs, u, p):
    """P2 velocity / P1 pressure of S snapshots at points given by their cell's dofs (m, 6) and barycentrics (m, 3):
    u (S, n2, 2), p (S, nv) -> (S, m, 2), (S, m)."""
    l0, l1, l2 = lam[:, 0], lam[:, 1], lam[:, 2]
    phi = np.stack([l0 * (2 * l0 - 1), l1 * (2 * l1 - 1), l2 * (2 * l2 - 1), 4 * l1 * l2, 4 * l0 * l2, 4 * l0 * l1], axis=1)
    return np.einsum("mk,smkc->smc", phi, u[:, dofs]), np.einsum("mk,smk->sm", lam, p[:, dofs[:, :3]])


def quadratic(c, xy):
    """c[0] + c[1] x + c[2] y + c[3] x^2 + c[4] x y + c[5] y^2 (c may have fewer than 6 entries: a lower degree)."""
    x, y = xy[..., 0], xy[..., 1]
    terms = (np.ones_like(x), x, y, x * x, x * y, y * y)
    return sum(ci * t for ci, t in zip(c, terms))


def airfoil_area(coords, cells, facets):
    """Area of the polygon bounded by the airfoil facets, (cell, local facet k = the edge opposite vertex k) of the FLUID
    cells: shoelace formula with every facet oriented so that the fluid (the cell's opposite vertex) lies on its right -
    the airfoil's boundary counter-clockwise.  Also checks that the facets close a ring (every end point used twice)."""
    x = np.asarray(coords, np.float64)
    c = np.asarray(cells)
    area = 0.0
    ends = []
    for cell, k in facets:
        v = c[cell]
        a, b, o = x[v[(k + 1) % 3]], x[v[(k + 2) % 3]], x[v[k]]
        if _cross(*(b - a), *(o - a)) > 0:
            a, b = b, a
        area += 0.5 * _cross(a[0], a[1], b[0], b[1])
        ends += [v[(k + 1) % 3], v[(k + 2) % 3]]
    assert (np.bincount(ends) <= 2).all() and (np.bincount(ends)[np.unique(ends)] == 2).all(), "airfoil facets do not close"
    return area


def closed_form_fields(dof_xy, nv, mu, area):
    """The force-probe cases with a closed form (divergence theorem over the airfoil, whose facet normals point INTO it):
    [(name, u (n2, 2) nodal values, p (nv,) nodal values, drag, lift)]."""
    x, y = dof_xy[:, 0], dof_xy[:, 1]
    z = np.zeros_like(x)
    return [("p=1", np.stack([z, z], 1), np.ones(nv), 0.0, 0.0),
            ("p=x", np.stack([z, z], 1), x[:nv].copy(), area, 0.0),
            ("p=y", np.stack([z, z], 1), y[:nv].copy(), 0.0, area),
            ("u=(x-2y,3x+y)", np.stack([x - 2 * y, 3 * x + y], 1), np.zeros(nv), 0.0, 0.0),
            ("u=(x^2,0)", np.stack([x * x, z], 1), np.zeros(nv), -4.0 * mu * area, 0.0)]
