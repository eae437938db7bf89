"""CPU: the meshes of the topology-section test are what they are meant to be, and the counting argument about vertex
degrees holds on them.

`cells at v + on_boundary(v)` is the number of edges at vertex v of a triangulation whose boundary is a manifold, is never
above it, and the estimates add up to 2 ne exactly when all of them are exact.  (A form of the SELL section that took its row
lengths from this estimate, with the atomic count as the fall-back, gained 1.3 us per launch and is not in the kernel; the
meshes keep the pinched vertex that would take the fall-back.)  Here, against `MeshTopology`: per vertex the estimate is at
most the degree, and the sums are equal on every test mesh except the one with a pinched boundary vertex, where the estimate is
short by exactly one at exactly that vertex."""
import numpy as np
import pytest

import topo_section_cases as tc


@pytest.fixture(scope="module")
def all_meshes(meshes):
    names = sorted({n for b in tc.BATCHES.values() for n in b})
    return {n: tc.mesh(meshes, n) for n in names}


def test_channels_have_the_counts_they_are_there_for(all_meshes):
    for name, (_, want) in tc.CASES.items():
        c, t = all_meshes[name]
        nv, nt, ne = tc.counts(t)
        assert nv == len(c) and all(dict(nv=nv, nt=nt, ne=ne)[k] == v for k, v in want.items()), (name, nv, nt, ne)
        assert nv <= 1024 and nt <= 2048 and ne <= 3072                    # the K = 1 instance
        a, b, d = c[t[:, 0]], c[t[:, 1]], c[t[:, 2]]
        area2 = np.abs((b[:, 0] - a[:, 0]) * (d[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (d[:, 0] - a[:, 0]))
        assert area2.min() > 1e-6 and len(np.unique(t, axis=0)) == nt, name
    # both sides of every size at which the kernel's pass counts change
    n = {name: tc.counts(all_meshes[name][1]) for name in tc.CASES}
    assert {n["nv63"][0], n["nv64"][0], n["nv65"][0]} == {63, 64, 65}
    assert 3 * n["nt341"][1] < 1024 < 3 * n["nt342"][1] and 3 * n["nt682"][1] < 2048 < 3 * n["nt683"][1]
    assert n["ne1024"][2] == 1024 and n["ne1025"][2] == 1025 and n["ne2048"][2] == 2048 and n["ne2049"][2] == 2049
    assert n["nt1024"][1] == 1024 and n["nt1025"][1] == 1025 and n["nv1023"][0] == 1023 and n["nv1024"][0] == 1024


def test_cells_plus_boundary_is_the_degree_unless_the_boundary_is_pinched(all_meshes):
    from meshdqn_amd.topology import MeshTopology
    for name, (c, t) in all_meshes.items():
        mt = MeshTopology(c, t)
        assert set(mt.edge_ncells.tolist()) == {1, 2}, name
        cells = np.bincount(t.ravel(), minlength=mt.nv)
        degree = np.bincount(mt.edges.ravel(), minlength=mt.nv)
        estimate = cells + mt.on_boundary.astype(np.int64)
        assert (estimate <= degree).all(), name
        short = np.flatnonzero(estimate < degree)
        if name == "pinch":
            (nx, ny, _, _, _, (pi, pj)), _ = tc.CASES[name]
            xs, ys = np.linspace(-0.5, 3.0, nx), np.linspace(-0.5, 0.5, ny)
            assert len(short) == 1 and tuple(c[short[0]]) == (xs[pi + 1], ys[pj + 1])
            assert degree[short[0]] - estimate[short[0]] == 1 and estimate.sum() == 2 * mt.ne - 1
            # four boundary edges meet there
            be = mt.edges[mt.boundary_edges]
            assert (be == short[0]).sum() == 4
        else:
            assert len(short) == 0 and estimate.sum() == 2 * mt.ne, name
