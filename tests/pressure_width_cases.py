"""The meshes of the pressure-width tests and their SELL-64 width class, on the host.

The first-step pressure CG of the three-kernel mode keeps the rows of the P1 Laplacian in registers at 10, 12 or 16 slots per
row - the smallest that holds the mesh's widest SELL-64 slice, i.e. its longest row (largest vertex degree + 1) - and
falls back to the LDS-resident CG beyond 16.  The lab meshes are in the first class; the wider ones are ys930 after scripted
vertex removals (host engine: removal, Delaunay restoration, smooth(50) each) that pile neighbours onto one hub.  The script
was found by a greedy search on the host: of the neighbours of the vertex of the largest degree, remove the one that
leaves the largest degree in the mesh.  Two such searches of 80 removals did not get beyond 16 entries per row (Delaunay
restoration works against it), so the class > 16 is left out."""
import numpy as np

CLASSES = ("<= 10", "11-12", "13-16", "> 16")

# vertex indices, removed one after the other from ys930 (indices are those of the mesh at that moment)
HUB_SCRIPT = [393, 427, 244, 332, 281, 278, 345, 217, 509, 616, 258, 781, 258, 543, 506, 506, 578, 608, 698, 576, 504, 504,
              742, 760, 671, 538, 403, 839, 571, 283, 501, 513, 263, 500, 517, 726, 500, 257, 507, 525, 264, 779]

# name -> (golden mesh, removals of HUB_SCRIPT, expected class, expected widest row)
CASES = {
    "ys930": ("ys930", 0, "<= 10", 9),
    "ah93w145": ("ah93w145", 0, "<= 10", 9),
    "ys930-hub20": ("ys930", 20, "11-12", 12),
    "ys930-hub42": ("ys930", 42, "13-16", 14),
}


def width_class(width):
    return CLASSES[0 if width <= 10 else 1 if width <= 12 else 2 if width <= 16 else 3]


def widest_row(cells, nv):
    """Longest row of the P1 Laplacian: the largest number of distinct neighbours of a vertex, plus the diagonal."""
    e = np.concatenate([cells[:, [0, 1]], cells[:, [1, 2]], cells[:, [0, 2]]])
    e = np.unique(np.sort(e, axis=1), axis=0)
    return int(np.bincount(e.ravel(), minlength=nv).max()) + 1


def case_mesh(meshes, name):
    """(coords, cells, smoothed) of a case: a golden mesh as it is (not smoothed yet), or ys930 after its removals (smoothed
    by the host engine after every removal)."""
    from meshdqn_amd.mesh_ops import remesh_batch
    base, removals, _, _ = CASES[name]
    coords, cells = meshes[base]
    if removals == 0:
        return np.asarray(coords, np.float64), np.asarray(cells, np.int32), False
    c = np.ascontiguousarray(coords[None], np.float64).copy()
    t = np.ascontiguousarray(cells[None], np.int32).copy()
    nv, nt = np.array([coords.shape[0]], np.int32), np.array([cells.shape[0]], np.int32)
    for idx in HUB_SCRIPT[:removals]:
        assert remesh_batch(c, t, nv, nt, np.array([idx], np.int32))[0] == 0
    assert nv[0] == coords.shape[0] - removals
    return c[0, :nv[0]].copy(), t[0, :nt[0]].copy(), True
