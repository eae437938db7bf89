"""GPU: `mdq_remesh` on the hand-built meshes of tests/remesh_cases.py against the reference's `_remove_vertex`
(Env2DAirfoil.py:452-512), a global scipy / Qhull Delaunay called here directly: hubs at the limit of the 64-entry star
buffer, a shaken (non-Delaunay, non-convex) mesh, every capacity instance (Cap<1>, Cap<4>, Cap<16>) with the small cases and
at its vertex limit, one launch with mixed outcomes, the refusals with their exact codes and the promise "mesh untouched".
Every comparison is exact: cells as sets, coordinates bit for bit (the kernel only moves them) - no tolerance anywhere.
(`mdq_remesh_act` is not repeated here: test_env_finish_gpu.py pins it to `mdq_env_act` followed by `mdq_remesh`.)

Results are never compared slot for slot with the host engine: the two Lawson loops pop different stacks, sets are the
contract.  No case is near the guard of 200 000 work-list pops, where the codes of the two engines are known to differ (the
host counts every interior edge against it, the device only the violating ones)."""
import time

import numpy as np
import pytest
import torch

import remesh_cases as rc

pytestmark = pytest.mark.gpu
SMALL = (1024, 2048)
# both sides of 1024 / 2048 and of 4096 / 8192, in vertices and in triangles; the largest instance
INSTANCES = [(1025, 2048), (1024, 2049), (4096, 8192), (4097, 8192), (4096, 8193), (16384, 32768)]


def _device(items, NV, NT, cells=None):
    """One launch on the padded batch of (case, rv): ((coords, cells, nv, nt, status) after, (coords, cells, nv, nt) before)."""
    from meshdqn_amd.mesh_ops import remesh_batch_gpu
    x, c, nv, nt, rem = rc.batch(items, NV, NT)
    if cells is not None:
        c = cells
    dev = [torch.from_numpy(a).cuda() for a in (x, c, nv, nt, rem)]
    st = torch.full((len(items),), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    remesh_batch_gpu(*dev, st)
    torch.cuda.synchronize()
    print(f"[remesh] {'+'.join(f'{case.name}:{rv}' for case, rv in items)} at {(NV, NT)}: "
          f"{1e3 * (time.perf_counter() - t0):.2f} ms")
    return tuple(a.cpu().numpy() for a in dev[:4]) + (st.cpu().numpy(),), (x, c, nv, nt)


_RUNS = {}


def _run(key, items, NV, NT):
    """Launches shared between tests (computed once, never written to)."""
    k = (key, NV, NT)
    if k not in _RUNS:
        _RUNS[k] = _device(items, NV, NT)
        for a in _RUNS[k][0] + _RUNS[k][1]:
            a.setflags(write=False)
    return _RUNS[k]


def _single(case, rv):
    return _run((case.name, rv), [(case, rv)], *SMALL)


def _mixed(NV, NT):
    return _run("mixed", [(case, rv) for case, rv, _ in rc.mixed_batch()], NV, NT)


def _assert_equals_oracle(case, rv, x, c, nv, nt):
    ox, oc = rc.oracle(case, rv)
    assert (nv, nt) == (case.nv - 1, case.nt - 2)
    assert np.array_equal(rc.canon(c[:nt]), rc.canon(oc)), (case.name, rv)
    assert np.array_equal(c[:nt], np.sort(c[:nt], axis=1))
    assert rc.same_bits(x[:nv], ox)
    assert rc.padding_intact(x, c, nv + 1, nt + 2)


def _assert_untouched(after, before, b):
    for got, want in zip(after[:4], before):
        assert rc.same_bits(got[b], want[b])


def _assert_same_result(a, b, ia, ib, case):
    """Environment ia of run a holds what environment ib of run b holds: counts, status, every cell row and coordinate row
    that the mesh had before the removal (bit for bit: the kernel is deterministic), the sentinel behind them."""
    assert (a[2][ia], a[3][ia], a[4][ia]) == (b[2][ib], b[3][ib], b[4][ib])
    assert rc.same_bits(a[0][ia, :case.nv], b[0][ib, :case.nv]) and rc.same_bits(a[1][ia, :case.nt], b[1][ib, :case.nt])
    assert rc.padding_intact(a[0][ia], a[1][ia], case.nv, case.nt) and rc.padding_intact(b[0][ib], b[1][ib], case.nv, case.nt)


def test_device_removal_equals_qhull_on_hubs_and_the_shaken_mesh(lib_built):
    """Degree 63 and 64 at the star buffer's limit (the ear-clipped fan of a near-cocircular polygon, largely undone by
    Lawson); the lowest, a middle and the highest interior id of a mesh with > 100 violating edges and reflex star corners."""
    for case, rv in rc.valid():
        (x, c, nv, nt, st), _ = _single(case, rv)
        assert st.tolist() == [0]
        _assert_equals_oracle(case, rv, x[0], c[0], int(nv[0]), int(nt[0]))


def test_device_removal_on_the_lattice_is_delaunay_exactly(lib_built):
    g = rc.grid()
    rv = g.removals[0]
    (x, c, nv, nt, st), _ = _single(g, rv)
    assert st.tolist() == [0] and (nv[0], nt[0]) == (g.nv - 1, g.nt - 2)
    assert rc.same_bits(x[0, :nv[0]], np.delete(g.coords, rv, axis=0))
    rc.check_delaunay_exact(g, rv, x[0, :nv[0]], c[0, :nt[0]])
    assert rc.padding_intact(x[0], c[0], nv[0] + 1, nt[0] + 2)


@pytest.mark.parametrize("which", ["boundary", "absent", "nothing", "hub65", "duplicated"])
def test_device_refusals_return_the_hosts_code_and_leave_the_mesh_untouched(lib_built, which):
    from meshdqn_amd.mesh_ops import remesh_batch
    name, case, rv, code = next(r for r in rc.refusals() if r[0] == which)
    after, before = _single(case, rv)
    assert after[4].tolist() == [code]
    hx, hc, hnv, hnt, hrem = rc.batch([(case, rv)], *SMALL)
    assert remesh_batch(hx, hc, hnv, hnt, hrem, 0, 1).tolist() == [code]
    _assert_untouched(after, before, 0)
    _assert_untouched((hx, hc, hnv, hnt), before, 0)


def test_one_launch_with_mixed_outcomes_equals_the_single_launches(lib_built):
    """B = 8 different environments in one launch: two hubs removed and one refused, three removals on the shaken mesh, a
    boundary refusal and a do-nothing - every environment holds what its own launch gives, padding included."""
    mixed = rc.mixed_batch()
    after, before = _mixed(*SMALL)
    assert after[4].tolist() == [code for _, _, code in mixed]
    for b, (case, rv, code) in enumerate(mixed):
        _assert_same_result(after, _single(case, rv)[0], b, 0, case)
        if code != 0 or rv < 0:
            _assert_untouched(after, before, b)


@pytest.mark.parametrize("capacity", INSTANCES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_every_instance_gives_the_result_of_the_smallest(lib_built, capacity):
    """The mixed batch in arrays of other capacities: tables in LDS or on the slab (one slab per environment, different
    meshes side by side), hashes of 8 192, 16 384 and 131 072 slots, 10-, 12- and 14-bit edge keys."""
    from meshdqn_amd import _lib
    mixed = rc.mixed_batch()
    assert _lib.load().mdq_remesh_workspace_bytes(len(mixed), *capacity) > 0
    ref, _ = _mixed(*SMALL)
    after, before = _mixed(*capacity)
    for b, (case, rv, code) in enumerate(mixed):
        _assert_same_result(after, ref, b, b, case)
        if code != 0 or rv < 0:
            _assert_untouched(after, before, b)


def test_capacities_beyond_the_largest_instance_launch_nothing(lib_built):
    from meshdqn_amd import _lib
    from meshdqn_amd.mesh_ops import remesh_batch_gpu
    lib = _lib.load()
    NV, NT = 16385, 32768
    assert lib.mdq_remesh_workspace_bytes(1, NV, NT) == -1 and lib.mdq_remesh_workspace_bytes(1, 16384, 32769) == -1
    s = rc.shaken()
    host = rc.batch([(s, s.removals[0])], NV, NT)
    dev = [torch.from_numpy(a).cuda() for a in host]
    st = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    assert lib.mdq_remesh(1, NV, NT, *(a.data_ptr() for a in dev), st.data_ptr(), ws.data_ptr(), ws.numel(),
                          _lib.stream_ptr()) != 0
    with pytest.raises(_lib.MeshDQNHipError):
        remesh_batch_gpu(*dev, st)
    torch.cuda.synchronize()
    assert st.tolist() == [77]
    for got, want in zip(dev, host):
        assert rc.same_bits(got.cpu().numpy(), want)


@pytest.mark.parametrize("NV", [1024, 4096, 16384])
def test_every_instance_at_its_vertex_limit_equals_qhull(lib_built, NV):
    """nv == NV exactly (ids up to NV - 1 in the edge keys; 12 093 edges in the 16 384-slot LDS hash of Cap<4>): id 0, the
    last id (both interior: the two ends of the renumbering) and a do-nothing in one launch."""
    case = rc.full(NV)
    items = [(case, case.removals[0]), (case, case.removals[1]), (case, -1)]
    after, before = _device(items, NV, 2 * NV)
    x, c, nv, nt, st = after
    assert st.tolist() == [0, 0, 0]
    for b in range(2):
        _assert_equals_oracle(case, items[b][1], x[b], c[b], int(nv[b]), int(nt[b]))
    _assert_untouched(after, before, 2)


@pytest.mark.parametrize("capacity", [SMALL, (4097, 8192)], ids=lambda c: f"{c[0]}x{c[1]}")
def test_two_identical_launches_give_identical_bits(lib_built, capacity):
    first, _ = _mixed(*capacity)
    again, _ = _device([(case, rv) for case, rv, _ in rc.mixed_batch()], *capacity)
    for a, b in zip(first, again):
        assert rc.same_bits(a, b)


def test_cells_given_in_any_vertex_order_give_the_same_set(lib_built):
    """The kernel orients its input itself: clockwise and counter-clockwise rows mixed, on the 64-hub and the shaken mesh."""
    items = [(rc.hub(64), 0)] + [(rc.shaken(), rv) for rv in rc.shaken().removals]
    _, c0, _, _, _ = rc.batch(items, *SMALL)
    rng = np.random.default_rng(5)
    shuffled = c0.copy()
    for b, (case, _) in enumerate(items):
        shuffled[b, :case.nt] = rng.permuted(c0[b, :case.nt], axis=1)
    assert (shuffled != c0).any() and (rc.orient2d(items[1][0].coords, shuffled[1, :items[1][0].nt]) < 0).sum() > 100
    (x, c, nv, nt, st), _ = _device(items, *SMALL, cells=shuffled)
    assert st.tolist() == [0] * len(items)
    for b, (case, rv) in enumerate(items):
        _assert_equals_oracle(case, rv, x[b], c[b], int(nv[b]), int(nt[b]))
