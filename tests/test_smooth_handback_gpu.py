"""GPU: the hand-back of `mdq_smooth_fast` inside its own launch.

A mesh beyond the limits of the blocked solve (here: a hub of 18 cells, the fan mesh of `test_env_gpu.py`) is walked vertex
by vertex by the environment's own workgroup of `smooth_linear_kernel` - 768 threads around a walk written for 256 - where
a second launch of at most four workgroups used to pick it up.  Batches of 1, 2, 5 and 6 environments with refused and
ordinary meshes interleaved: five refused meshes in one launch, a refused mesh in the last slot, environments with no
sweeps at all.  `mdq_smooth` alone (the walk as its own kernel) is the reference, computed once per batch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (kind, seed, sweeps): R = hub of 18 cells (refused by the blocked solve), O = hub of 12 cells (ordinary)
# (at most 7 sweeps: the strongly jittered fans are made for the first sweeps - some collapse under 50 of them, in the walk
#  itself; the reference must be finite for the comparison to mean anything)
BATCHES = {
    1: [("R", 1, 5)],
    2: [("O", 2, 5), ("R", 3, 3)],
    5: [("R", 4, 7), ("O", 5, 7), ("R", 6, 0), ("O", 7, 0), ("R", 8, 1)],
    6: [("R", 9, 2), ("R", 10, 5), ("O", 11, 7), ("R", 12, 7), ("R", 13, 4), ("R", 14, 3)],
}


def _mesh(kind, seed):
    from test_env_gpu import _fan_mesh
    return _fan_mesh(seed, n=18) if kind == "R" else _fan_mesh(seed)


def _pack(batch):
    B = len(batch)
    NV, NT = max(len(c) for c, _ in batch), max(len(t) for _, t in batch)
    coords, cells = np.zeros((B, NV, 2)), np.zeros((B, NT, 3), np.int32)
    nv, nt = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b, (c, t) in enumerate(batch):
        coords[b, :len(c)], cells[b, :len(t)], nv[b], nt[b] = c, t, len(c), len(t)
    return coords, cells, nv, nt


def _smooth(batch, iters, fast):
    """(result, diagnostics or None) of one launch of mdq_smooth_fast / mdq_smooth over `batch`."""
    import torch
    from meshdqn_amd.mesh_ops import smooth_batch_gpu, smooth_fast_stats
    coords, cells, nv, nt = _pack(batch)
    dev = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    tc = dev(coords.copy())
    smooth_batch_gpu(tc, dev(cells), dev(nv), dev(nt), dev(np.asarray(iters, np.int32)), fast=fast)
    torch.cuda.synchronize()
    return tc.cpu().numpy(), (smooth_fast_stats(tc.device, len(batch), coords.shape[1]) if fast else None)


@pytest.fixture(scope="module")
def cases(lib_built):
    """Per batch size: the meshes, the sweep counts and the walk's result (mdq_smooth alone) - computed once."""
    out = {}
    for B, spec in BATCHES.items():
        batch = [_mesh(k, s) for k, s, _ in spec]
        iters = [n for _, _, n in spec]
        out[B] = dict(spec=spec, batch=batch, iters=iters, walk=_smooth(batch, iters, False)[0], start=_pack(batch)[0])
        assert np.isfinite(out[B]["walk"]).all(), B
    return out


@pytest.mark.parametrize("B", sorted(BATCHES))
def test_refused_meshes_are_walked_inside_the_launch(cases, B):
    c = cases[B]
    fast, st = _smooth(c["batch"], c["iters"], True)
    again, st2 = _smooth(c["batch"], c["iters"], True)
    for b, (kind, _, n) in enumerate(c["spec"]):
        nvb = len(c["batch"][b][0])
        if n == 0:
            assert np.array_equal(fast[b], c["start"][b]), (B, b)               # no sweeps: untouched
        if kind == "R":
            assert np.array_equal(fast[b], c["walk"][b]), (B, b)                # the walk's own result, bit for bit
            assert st[b, 0] == n, (B, b, st)                                    # all its sweeps handed back, exactly
        else:
            err = np.abs(fast[b, :nvb] - c["walk"][b, :nvb]).max()
            print(f"B {B} env {b}: blocked solve against the walk {err:.2e}")
            assert err < 1e-13, (B, b, err)
            assert st[b, 0] == 0, (B, b, st)
            # the same mesh in a batch of its own: the neighbours in the launch do not matter
            alone, _ = _smooth([c["batch"][b]], [n], True)
            assert np.array_equal(alone[0, :nvb], fast[b, :nvb]), (B, b)
    assert np.array_equal(fast, again) and np.array_equal(st, st2), B          # two runs: bitwise equal
    if B == 6:
        assert sum(k == "R" and n > 0 for k, _, n in c["spec"]) > 4            # more than the four workgroups of the old walk
    assert c["spec"][-1][0] == "R"                                             # a refused mesh in the last slot


@pytest.mark.parametrize("B", sorted(BATCHES))
def test_env_entry_point_switches_single_environments_off(cases, B):
    """`mdq_smooth_fast_env`: `iterations` sweeps where the removal succeeded (rem >= 0 and rstat == 0), nothing elsewhere -
    refused and ordinary meshes alike.  Reference: the walk with that sweep count for the environments that are on."""
    import torch
    from meshdqn_amd.mesh_ops import smooth_env_gpu, smooth_fast_stats
    c = cases[B]
    S = 5
    # environment b is on unless b % 3 == 1 (rem < 0: no removal) or b % 3 == 2 and b > 2 (rstat != 0: the removal failed)
    rem = np.array([-1 if b % 3 == 1 else 10 + b for b in range(B)], np.int32)
    rstat = np.array([3 if (b % 3 == 2 and b > 2) else 0 for b in range(B)], np.int32)
    on = (rem >= 0) & (rstat == 0)
    if B == 1:
        on[:] = True
        rem[:], rstat[:] = 0, 0
    walk, _ = _smooth(c["batch"], [S if o else 0 for o in on], False)
    assert np.isfinite(walk).all()
    coords, cells, nv, nt = _pack(c["batch"])
    dev = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    outs = []
    for _ in range(2):
        tc = dev(coords.copy())
        smooth_env_gpu(tc, dev(cells), dev(nv), dev(nt), dev(rem), dev(rstat), S)
        torch.cuda.synchronize()
        outs.append(tc.cpu().numpy())
    st = smooth_fast_stats(tc.device, B, coords.shape[1])
    assert np.array_equal(outs[0], outs[1])
    for b, (kind, _, _) in enumerate(c["spec"]):
        nvb = nv[b]
        if not on[b]:
            assert np.array_equal(outs[0][b], coords[b]) and st[b, 0] == 0, (B, b, st)
        elif kind == "R":
            assert np.array_equal(outs[0][b], walk[b]) and st[b, 0] == S, (B, b, st)
        else:
            assert np.abs(outs[0][b, :nvb] - walk[b, :nvb]).max() < 1e-13 and st[b, 0] == 0, (B, b, st)
