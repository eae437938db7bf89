"""GPU: the dof <- slot gather lists and the SELL pattern of the IPCS index section of the device topology engine - edge-dof
rows written straight from the edge tables, short lists ranked in registers - against the host engine and against the
same launches on the parent's code paths.

`MDQ_TOPO_INDEX_PARENT=3` (read once per process) selects the general count / fill / sort path for every dof and the
ranking loops in LDS.  Two fresh child processes, one per setting, run every batch of tests/flow_index_cases.py through the
flow stream's engine with both edge numberings (its own hash table, `take_edges_from`); the cases below hold `g2_ptr`,
`g2_src`, `g1_ptr`, `g1_src`, `sl1_off`, `sl1_col`, `cell_dofs` and `ne` array-equal to the host engine
(`HostTopologyBatch`) and array-equal between the two settings.

Meshes: a hand-built channel with a pentagonal hole whose vertex lists have every length from 1 to 8 and one of 10, with
boundary edges on every tag; ys930 raw and after 20 and 42 scripted removals; ah93w145 - two batches of three, the
hand-built mesh in the last slot."""
import os
import subprocess
import sys

import numpy as np
import pytest

import flow_index_cases as fic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runs(lib_built, tmp_path_factory):
    """(default, MDQ_TOPO_INDEX_PARENT=3): every batch, each setting in a fresh process."""
    out = []
    for name, parent in (("default", None), ("parent", "3")):
        path = str(tmp_path_factory.mktemp("flow_index") / f"{name}.npz")
        env = {k: v for k, v in os.environ.items() if k != "MDQ_TOPO_INDEX_PARENT"}
        if parent:
            env["MDQ_TOPO_INDEX_PARENT"] = parent
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [fic.__file__, path]
        res = subprocess.run(cmd, env=env, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        out.append(dict(np.load(path)))
    return out


@pytest.fixture(scope="module")
def host(lib_built, meshes):
    """batch -> (meshes, host engine after its run)."""
    from meshdqn_amd.mesh_ops import HostTopologyBatch
    out = {}
    for key in fic.BATCHES:
        ms, args = fic.batch(meshes, key)
        hb = HostTopologyBatch(*args, ipcs=True)
        fic.fill(hb, ms)
        hb.run(2)
        out[key] = (ms, hb)
    return out


def test_hand_built_mesh_is_what_it_is_meant_to_be():
    """On the host: a valid triangulation of the channel minus the hole, vertex lists of every length 1 ... 8 and one longer,
    boundary edges with one owner on the walls, the inlet, the outlet and the hole."""
    c, t = fic.hand_mesh()
    a, b, d = c[t[:, 0]], c[t[:, 1]], c[t[:, 2]]
    area2 = np.abs((b[:, 0] - a[:, 0]) * (d[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (d[:, 0] - a[:, 0]))
    h = c[list(fic.HAND_HOLE)]
    hole = 0.5 * abs(np.sum(h[:, 0] * np.roll(h[:, 1], -1) - np.roll(h[:, 0], -1) * h[:, 1]))
    assert area2.min() > 1e-3 and abs(0.5 * area2.sum() - (3.5 - hole)) < 1e-12
    lists = np.bincount(t.ravel(), minlength=len(c))
    assert set(range(1, 9)) <= set(lists.tolist()) and lists.max() == 10
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [0, 2]]]), axis=1)
    ue, cnt = np.unique(e, axis=0, return_counts=True)
    assert set(cnt.tolist()) == {1, 2}
    mid = c[ue[cnt == 1]].mean(axis=1)
    walls, inlet, outlet = np.abs(mid[:, 1]) == 0.5, mid[:, 0] == -0.5, mid[:, 0] == 3.0
    inner = ~(walls | inlet | outlet)
    assert walls.sum() == 12 and inlet.sum() == 4 and outlet.sum() == 3 and inner.sum() == 5
    assert set(ue[cnt == 1][inner].ravel().tolist()) == set(fic.HAND_HOLE)


@pytest.mark.parametrize("key", list(fic.BATCHES))
@pytest.mark.parametrize("numbering", ["hash", "given"])
@pytest.mark.parametrize("setting", [0, 1])
def test_lists_equal_the_host_engine(runs, host, key, numbering, setting):
    run = runs[setting]
    ms, hb = host[key]
    for b, (c, t) in enumerate(ms):
        nv, nt, ne = len(c), len(t), int(hb.h["ne"][b])
        n2 = nv + ne
        g = lambda k: run[f"{key}/{numbering}/{k}"][b]   # noqa: E731
        assert g("ne") == ne == fic.edge_count(t), (key, b)
        assert np.array_equal(g("cell_dofs")[:, :nt], hb.h["cell_dofs"][b][:, :nt]), (key, b)
        lens = dict(g1_ptr=nv + 1, g1_src=3 * nt, g2_ptr=n2 + 1, g2_src=6 * nt, sl1_off=(nv + 63) // 64 + 1)
        for k, n in lens.items():
            assert np.array_equal(g(k)[:n], hb.hi[k][b][:n]), (key, b, k)
        nse = int(hb.hi["sl1_off"][b][(nv + 63) // 64])
        assert nse > 0 and np.array_equal(g("sl1_col")[:nse], hb.hi["sl1_col"][b][:nse]), (key, b)
        # what the lists are: ascending slots per dof, the vertex rows first, every slot exactly once
        ptr, src = g("g2_ptr")[:n2 + 1], g("g2_src")[:6 * nt]
        assert ptr[0] == 0 and ptr[-1] == 6 * nt and np.array_equal(np.sort(src), np.arange(6 * nt))
        assert set(np.diff(ptr)[nv:].tolist()) == {1, 2}
        for d in range(n2):
            row = src[ptr[d]:ptr[d + 1]]
            assert (np.diff(row) > 0).all() and (hb.h["cell_dofs"][b][row % 6, row // 6] == d).all(), (key, b, d)


@pytest.mark.parametrize("key", list(fic.BATCHES))
def test_lists_equal_the_parent_paths_and_both_numberings(runs, key):
    new, old = runs
    assert sorted(new) == sorted(old)
    for k in fic.KEYS_T + fic.KEYS_TI:
        for numbering in ("hash", "given"):
            a, b = new[f"{key}/{numbering}/{k}"], old[f"{key}/{numbering}/{k}"]
            assert a.dtype == b.dtype and np.array_equal(a, b), (key, numbering, k)
        assert np.array_equal(new[f"{key}/hash/{k}"], new[f"{key}/given/{k}"]), (key, k)


def test_vertex_lists_of_the_batches_cross_the_register_limit(host):
    """Lists of at most 8 entries are ranked in registers, longer ones by the loops in LDS: both occur, in one batch."""
    for key, (ms, hb) in host.items():
        longest = [int(np.bincount(t.ravel()).max()) for _, t in ms]
        shortest = [int(np.bincount(t.ravel(), minlength=len(c)).min()) for c, t in ms]
        print(key, "longest vertex lists", longest, "shortest", shortest)
        assert max(longest) > 8 and min(shortest) == 1
