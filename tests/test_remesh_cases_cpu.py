"""CPU: the host engine's vertex removal (`mdq_remesh_host`, smooth_iters = 0) on the hand-built meshes of
tests/remesh_cases.py against the reference's `_remove_vertex` (Env2DAirfoil.py:452-512) - a global scipy / Qhull Delaunay,
`mesh_ops.remove_vertex_delaunay`: hubs at the star buffer's limit, a shaken (non-Delaunay, non-convex) mesh, meshes at the
vertex limit of every capacity instance, a lattice with incircle ties, and the refusals with their exact codes and the
promise "mesh untouched".  The builders' preconditions run here, so a broken seed shows up without a GPU.  Every comparison
is exact."""
import numpy as np
import pytest

import remesh_cases as rc


def _host(items, NV, NT):
    from meshdqn_amd.mesh_ops import remesh_batch
    x, c, nv, nt, rem = rc.batch(items, NV, NT)
    before = (x.copy(), c.copy(), nv.copy(), nt.copy())
    st = remesh_batch(x, c, nv, nt, rem, 0, 1)
    return (x, c, nv, nt, st), before


def _assert_equals_oracle(case, rv, x, c, nv, nt):
    from meshdqn_amd.mesh_ops import remove_vertex_delaunay
    ox, oc = rc.oracle(case, rv)
    assert (nv, nt) == (case.nv - 1, case.nt - 2)
    assert np.array_equal(rc.canon(c[:nt]), rc.canon(oc)), (case.name, rv)
    assert np.array_equal(c[:nt], np.sort(c[:nt], axis=1))                     # canonical rows
    assert rc.same_bits(x[:nv], np.delete(case.coords, rv, axis=0)) and rc.same_bits(x[:nv], ox)
    # the row the removal vacates keeps what it held; the padding is the sentinel
    assert rc.padding_intact(x, c, nv + 1, nt + 2)
    # the builders' oracle is the project's statement of the reference, call for call
    mx, mc = remove_vertex_delaunay(case.coords, case.boundary, rv)
    assert rc.same_bits(mx, ox) and np.array_equal(rc.canon(mc), rc.canon(oc))


def test_builders_keep_their_preconditions():
    """Every builder asserts its own preconditions (every point used, the filter drops nothing, nt - 2 cells after every valid
    removal); here are the figures that the cases are built for."""
    assert [(rc.hub(n).nv, rc.hub(n).nt, rc.degree(rc.hub(n), 0)) for n in (63, 64, 65)] == \
        [(238, 426, 63), (241, 432, 64), (244, 438, 65)]
    s = rc.shaken()
    assert (s.nv, s.nt) == (364, 662) and 100 <= s.info["violating"] <= 512 and max(s.info["reflex"]) >= 1
    assert s.removals == (0, int(s.interior[s.interior.size // 2]), s.nv - 1)
    assert [(rc.full(n).nv, rc.full(n).nt) for n in (1024, 4096, 16384)] == [(1024, 1950), (4096, 7998), (16384, 32382)]
    assert [rc.full(n).removals for n in (1024, 4096, 16384)] == [(0, 1023), (0, 4095), (0, 16383)]
    assert 3 * rc.full(4096).nt // 2 + 96 == 12093                            # edges in the 16 384-slot hash of K = 4
    g = rc.grid()
    assert (g.nv, g.nt) == (121, 200)
    for case, rv in rc.valid() + [(rc.full(n), rv) for n in (1024, 4096, 16384) for rv in rc.full(n).removals]:
        rc.oracle(case, rv)
    dup, rv = rc.duplicated()
    assert dup.nt == s.nt + 1 and not (dup.cells[-1] == rv).any()
    with pytest.raises(ValueError):
        rc.edge_pairs(dup.cells)


def test_exact_checker_refuses_a_non_delaunay_and_a_broken_result():
    """The checker of the lattice case is itself checked: it accepts scipy's own triangulation of the lattice and refuses a
    missing cell, a moved vertex and one flipped edge (still a triangulation of the same area, no longer Delaunay)."""
    g = rc.grid()
    rv = g.removals[0]
    ox, oc = rc.oracle(g, rv)
    rc.check_delaunay_exact(g, rv, ox, oc)
    with pytest.raises(AssertionError):
        rc.check_delaunay_exact(g, rv, ox, oc[:-1])
    moved = ox.copy()
    moved[0, 0] += 2.0 ** -20
    with pytest.raises(AssertionError):
        rc.check_delaunay_exact(g, rv, moved, oc)

    def cross(o, p, q):
        return (p[0] - o[0]) * (q[1] - o[1]) - (p[1] - o[1]) * (q[0] - o[0])
    (t, u, a, b, c, d), _ = rc.edge_pairs(oc)
    flips = 0
    for i in range(t.size):
        A, B, Cc, D = ox[a[i]], ox[b[i]], ox[c[i]], ox[d[i]]
        tied = abs(np.hypot(*(A - D)) - np.hypot(*(B - Cc))) < 1e-6          # (a lattice square: both diagonals are Delaunay)
        if cross(A, D, B) * cross(A, D, Cc) < 0 and not tied:                 # a convex quadrilateral: the flip is a mesh
            flipped = oc.copy()
            flipped[t[i]] = np.sort([a[i], b[i], d[i]])
            flipped[u[i]] = np.sort([a[i], d[i], c[i]])
            with pytest.raises(AssertionError):
                rc.check_delaunay_exact(g, rv, ox, flipped)
            flips += 1
    assert flips > 50


@pytest.mark.parametrize("capacity", [(1024, 2048), (1500, 2600)])
def test_host_removal_equals_qhull_on_hubs_and_the_shaken_mesh(lib_built, capacity):
    items = rc.valid()
    (x, c, nv, nt, st), _ = _host(items, *capacity)
    assert st.tolist() == [0] * len(items)
    for b, (case, rv) in enumerate(items):
        _assert_equals_oracle(case, rv, x[b], c[b], int(nv[b]), int(nt[b]))


@pytest.mark.parametrize("NV", [1024, 4096, 16384])
def test_host_removal_equals_qhull_at_the_vertex_limits(lib_built, NV):
    case = rc.full(NV)
    items = [(case, rv) for rv in case.removals]
    (x, c, nv, nt, st), _ = _host(items, NV, 2 * NV)
    assert st.tolist() == [0, 0]
    for b, (case, rv) in enumerate(items):
        _assert_equals_oracle(case, rv, x[b], c[b], int(nv[b]), int(nt[b]))


def test_host_removal_on_the_lattice_is_delaunay_exactly(lib_built):
    g = rc.grid()
    rv = g.removals[0]
    (x, c, nv, nt, st), _ = _host([(g, rv)], 1024, 2048)
    assert st.tolist() == [0] and (nv[0], nt[0]) == (g.nv - 1, g.nt - 2)
    assert rc.same_bits(x[0, :nv[0]], np.delete(g.coords, rv, axis=0))
    rc.check_delaunay_exact(g, rv, x[0, :nv[0]], c[0, :nt[0]])
    assert rc.padding_intact(x[0], c[0], nv[0] + 1, nt[0] + 2)


@pytest.mark.parametrize("which", ["boundary", "absent", "nothing", "hub65", "duplicated"])
def test_host_refusals_return_their_code_and_leave_the_mesh_untouched(lib_built, which):
    """-3 boundary vertex, -2 vertex in no cell, 0 do nothing, -1 more than 64 cells at the vertex, -11 an edge with three
    owners (found by make_delaunay AFTER the cavity has been re-triangulated): coordinates, cells, counts and the sentinel
    padding are bitwise the input."""
    name, case, rv, code = next(r for r in rc.refusals() if r[0] == which)
    (x, c, nv, nt, st), (x0, c0, nv0, nt0) = _host([(case, rv)], 1024, 2048)
    assert st.tolist() == [code]
    assert (nv.tolist(), nt.tolist()) == (nv0.tolist(), nt0.tolist())
    assert rc.same_bits(c, c0), np.flatnonzero((c != c0).any(axis=2)[0])[:8]
    assert rc.same_bits(x, x0)
