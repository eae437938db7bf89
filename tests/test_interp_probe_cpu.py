"""CPU checks of the fp64 references that tests/test_interp_probe_gpu.py holds the interpolation and force-probe kernels
to (tests/oracle_util.py: brute-force point location, written-out P2 / P1 bases, airfoil area): a wrong sign or factor in
a reference fails here, not on the GPU."""
import numpy as np
import pytest

from oracle_util import (airfoil_area, brute_locate, closed_form_fields, interleaved_to_oracle_vel, p2_cell_dofs,
                         p2p1_eval)

MU = 1e-3


def _taylor_hood(meshes, name):
    from oracle.fem import TaylorHood
    from oracle.mesh import OracleMesh
    return TaylorHood(OracleMesh(*meshes[name]), mu=MU)


def _oracle_af_facets(th):
    return [th.mesh.edge_cells[e][0] for e in th.airfoil_facets()]


@pytest.mark.parametrize("name", ["ys930", "ah93w145"])
def test_closed_form_forces_hold_for_the_oracle(meshes, name):
    """(drag, lift) = -int_airfoil div(sigma) dA for the fields of `closed_form_fields`, through oracle/fem.py's facet
    integrals: p = 1 -> 0, p = x -> (A, 0), p = y -> (0, A), a linear u -> 0, u = (x^2, 0) -> (-4 mu A, 0)."""
    th = _taylor_hood(meshes, name)
    m = th.mesh
    area = airfoil_area(m.coords, m.cells, _oracle_af_facets(th))
    assert 0.01 < area < 0.5, area        # (a thin airfoil of unit chord)
    tol = 1e-12 * max(1.0, area)
    for what, u, p, drag, lift in closed_form_fields(th.dof_coords, th.nv, MU, area):
        d, l = th.forces(interleaved_to_oracle_vel(u), p)
        assert abs(d - drag) < tol and abs(l - lift) < tol, (what, d, drag, l, lift)


@pytest.mark.parametrize("name", ["ys930", "ah93w145"])
def test_brute_force_evaluator_agrees_with_p2p1_evaluator(meshes, name):
    """Random points inside random cells: the signed-area barycentrics + written-out bases of oracle_util against
    oracle/env.py's P2P1Evaluator (stored Jinv, oracle/fem.py's bases), random P2 / P1 dof values."""
    from meshdqn_amd.topology import MeshTopology
    from oracle.env import P2P1Evaluator
    coords, cells = meshes[name]
    th = _taylor_hood(meshes, name)
    topo = MeshTopology(coords, cells)
    assert np.array_equal(topo.edges, th.mesh.edges)
    rng = np.random.default_rng(11)
    cid = rng.integers(0, topo.nt, 1500)
    w = rng.dirichlet(np.ones(3), cid.size)
    pts = np.einsum("mk,mkc->mc", w, topo.coords[topo.cells[cid]])
    u = rng.standard_normal((2, topo.np2, 2))
    p = rng.standard_normal((2, topo.nv))
    cell, lam, viol = brute_locate(pts, topo.coords, topo.cells)
    assert viol.min() >= -1e-12
    U, P = p2p1_eval(lam, p2_cell_dofs(topo)[cell], u, p)
    ev = P2P1Evaluator(th)
    oc, oref = ev.locate(pts)
    for s in range(2):
        Uo = ev.eval_p2(interleaved_to_oracle_vel(u[s]), oc, oref)
        Po = ev.eval_p1(p[s], oc, oref)
        assert np.abs(U[s] - Uo).max() < 1e-13 * np.abs(u[s]).max()
        assert np.abs(P[s] - Po).max() < 1e-13 * np.abs(p[s]).max()
