"""GPU: the large-mesh smoothing kernels (`mdq_smooth_big.hip`) on meshes small enough to check by hand.

The kernels for more than 1024 vertices are chosen by the CAPACITY of the batch (NV / NT), not by the size of the mesh in it,
so the fan meshes of `test_env_gpu.py` padded to a capacity reach every path, each of which ends in the same exact update:

    1025 / 2048   `smooth_flow_kernel` first (skewed schedule); a hub of 18 cells is handed back to `smooth_big_kernel<1>`,
                  whose general loop (more than 16 cells at a vertex) takes it
    1025 / 2100   NT > 2 NVp skips the skewed kernel: `smooth_big_kernel<1>` directly - level sweeps for the hub of 12,
                  the general loop for the hub of 18
    4097 / 8192   `smooth_big_kernel<4>`, the 16 384-vertex instance (positions in global memory)

Reference: the plain DOLFIN loop of `oracle/mesh.py`, once per mesh and sweep count, to 1e-12 - the tolerance
`test_gpu_smoothing_exact_path` holds the same meshes to.  At most 7 sweeps: the strongly jittered fans are made for the
first sweeps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MESHES = [(12, 0), (12, 1), (12, 2), (18, 1), (18, 3), (18, 9)]      # (hub degree, seed)
SWEEPS = (1, 3, 7)
CAPS = {"skew": (1025, 2048), "level": (1025, 2100), "big4": (4097, 8192)}
PAD = -77.25                                                          # what the padding rows of the coordinates hold


def _pack(batch, NV, NT):
    B = len(batch)
    coords, cells = np.full((B, NV, 2), PAD), np.zeros((B, NT, 3), np.int32)
    nv, nt = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b, (c, t) in enumerate(batch):
        coords[b, :len(c)], cells[b, :len(t)], nv[b], nt[b] = c, t, len(c), len(t)
    return coords, cells, nv, nt


def _smooth(batch, iters, cap):
    """One launch of `mdq_smooth` over `batch` padded to the capacity `cap`; returns the whole coordinate array."""
    import torch
    from meshdqn_amd.mesh_ops import smooth_batch_gpu
    coords, cells, nv, nt = _pack(batch, *CAPS[cap])
    dev = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    tc = dev(coords)
    smooth_batch_gpu(tc, dev(cells), dev(nv), dev(nt), dev(np.asarray(iters, np.int32)), fast=False)
    torch.cuda.synchronize()
    return tc.cpu().numpy()


@pytest.fixture(scope="module")
def fans(lib_built):
    """Per (degree, seed): the mesh and the oracle's positions after 1, 3 and 7 sweeps - computed once."""
    from oracle.mesh import OracleMesh
    from test_env_gpu import _fan_mesh
    out = {}
    for n, seed in MESHES:
        coords, cells = _fan_mesh(seed, n=n)
        assert coords.shape == (2 * n + 1, 2) and cells.shape == (3 * n, 3)
        m = OracleMesh(coords, cells)
        assert max(len(w) for w in m.nbrs) == n
        ref = {s: OracleMesh(coords, cells).smooth(s).coords for s in SWEEPS}
        assert all(np.isfinite(r).all() for r in ref.values()), (n, seed)
        out[n, seed] = dict(mesh=(coords, cells), ref=ref)
    return out


@pytest.mark.parametrize("n,seed", MESHES)
def test_every_large_path_matches_the_oracle_with_the_same_bits(fans, n, seed):
    f = fans[n, seed]
    nv = len(f["mesh"][0])
    for s in SWEEPS:
        outs = {}
        for cap in CAPS:
            out = _smooth([f["mesh"]], [s], cap)
            err = np.abs(out[0, :nv] - f["ref"][s]).max()
            print(f"hub {n} seed {seed} sweeps {s} {cap}: against the oracle {err:.2e}")
            assert err < 1e-12, (n, seed, s, cap, err)
            assert (out[0, nv:] == PAD).all(), (n, seed, s, cap)                    # padding rows untouched
            assert np.array_equal(out, _smooth([f["mesh"]], [s], cap)), (n, seed, s, cap)   # two runs: the same bits
            outs[cap] = out[0, :nv]
        assert np.array_equal(outs["skew"], outs["level"]) and np.array_equal(outs["skew"], outs["big4"]), (n, seed, s)


@pytest.mark.parametrize("cap", sorted(CAPS))
def test_a_mesh_without_sweeps_is_left_alone(fans, cap):
    """A batch of two with sweep counts (3, 0): the first mesh as on its own, the second untouched."""
    batch = [fans[18, 1]["mesh"], fans[12, 0]["mesh"]]
    start = _pack(batch, *CAPS[cap])[0]
    out = _smooth(batch, [3, 0], cap)
    nv0 = len(batch[0][0])
    assert np.abs(out[0, :nv0] - fans[18, 1]["ref"][3]).max() < 1e-12
    assert np.array_equal(out[0], _smooth(batch[:1], [3], cap)[0])
    assert np.array_equal(out[1], start[1])
