"""CPU tests of batches that mix several airfoils (ABI 8): config validation, the airfoil of every global env id, the host
topology engine with one polygon per airfoil, and the ctypes mirrors of the new C structs."""
import copy
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

from meshdqn_amd.topology import MeshTopology

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _cfg(mesh, **agent):
    ap = dict(solver_steps=5000, episodes=10, timesteps=10000, threshold=0.001, N_closest=180, gt_drag=-1, gt_time=-1,
              u=-1, p=-1, do_nothing=True, time_reward=0.005, smoothing=True, save_steps=1000, goal_vertices=0.95, plot_dir="")
    ap.update(agent)
    return dict(flow_config=dict(flow_params=dict(mu=1e-3, rho=1.0, inflow="constant"),
                                 geometry_params=dict(mesh=os.path.join(GOLDEN, f"{mesh}.npz")),
                                 solver_params=dict(dt=0.001, solver_type="lu", smooth=True)),
                agent_params=ap)


@pytest.mark.parametrize("section,key,value", [("agent_params", "N_closest", 120), ("agent_params", "save_steps", 500),
                                               ("flow_params", "mu", 2e-3), ("solver_params", "dt", 5e-4)])
def test_mismatched_configs_raise_naming_the_key(section, key, value):
    from meshdqn_amd.vec_env import check_airfoil_configs
    a, b = _cfg("ys930"), _cfg("ah93w145")
    if section == "agent_params":
        b["agent_params"][key] = value
    else:
        b["flow_config"][section][key] = value
    with pytest.raises(ValueError, match=key):
        check_airfoil_configs([a, b])


def test_vec_env_refuses_mismatched_configs_before_any_work(lib_built):
    from meshdqn_amd.vec_env import VecEnv2DAirfoil
    a, b = _cfg("ys930"), _cfg("ah93w145", N_closest=90)
    with pytest.raises(ValueError, match="N_closest"):
        VecEnv2DAirfoil([a, b], 4)
    with pytest.raises(ValueError, match="config"):
        VecEnv2DAirfoil([], 4)


def test_per_airfoil_keys_may_differ():
    from meshdqn_amd.vec_env import check_airfoil_configs
    a = _cfg("ys930", gt_drag=np.array([1.0, 2.0]), gt_lift=np.array([0.1, 0.2]), gt_time=np.array([5.0]), plot_dir="/tmp/a")
    b = _cfg("ah93w145", gt_drag=np.array([3.0, 4.0]), gt_lift=np.array([0.3, 0.4]), gt_time=np.array([6.0]), plot_dir="/tmp/b",
             u=[1], p=[2])
    check_airfoil_configs([a, b])
    check_airfoil_configs([a, copy.deepcopy(a)])
    c = copy.deepcopy(a)
    c["flow_config"]["geometry_params"]["extra"] = 1     # a key only one of them has (not one of the per-airfoil ones)
    with pytest.raises(ValueError, match="extra"):
        check_airfoil_configs([a, c])


@pytest.mark.parametrize("envs,A", [(8, 2), (6, 3), (5, 2)])
def test_airfoil_of_global_env_ids_under_two_ranks(envs, A):
    """train.py: env id g = rank * envs + b steps airfoil g mod A; every rank's contiguous shard (DistContext.shard over the
    global ids) holds exactly those ids, and sees every airfoil."""
    from meshdqn_amd.trainer import DistContext
    from meshdqn_amd.vec_env import airfoil_assignment
    world = 2
    seen = []
    for rank in range(world):
        ids = list(DistContext.shard(types.SimpleNamespace(rank=rank, world=world), world * envs))
        assert ids == list(range(rank * envs, (rank + 1) * envs))
        af = airfoil_assignment(envs, A, rank * envs)
        assert af.dtype == np.int32 and af.tolist() == [g % A for g in ids]
        assert set(af.tolist()) == set(range(A))
        seen += af.tolist()
    assert seen == [g % A for g in range(world * envs)]
    assert airfoil_assignment(envs, A).tolist() == [b % A for b in range(envs)]      # the VecEnv default: b mod A


def _airfoil(meshes, name):
    from meshdqn_amd.ipcs_batch import smooth_coords
    coords, cells = meshes[name]
    t0 = MeshTopology(coords, cells)
    x0 = smooth_coords(t0, 50)
    polygon = x0[[v for v in range(t0.nv) if t0.on_boundary[v] and -0.5 < x0[v, 0] < 3 and -0.5 < x0[v, 1] < 0.5]]
    tags = t0.facet_tags(x0)
    return t0, x0, np.sort(cells, axis=1), polygon, int((tags == 1).sum())


def test_host_topology_with_per_env_polygons_equals_per_airfoil_calls(meshes, lib_built):
    """mdq_env_topology_host on a batch that alternates ys930 / ah93w145 (concatenated polygons + poly_ptr + src_of_env) ==
    one single-polygon call per airfoil at the same capacities, bit for bit - every output incl. the IPCS index data, on the
    smoothed meshes and on meshes with one vertex removed."""
    from meshdqn_amd.mesh_ops import HostTopologyBatch, remesh_batch
    air = [_airfoil(meshes, n) for n in ("ys930", "ah93w145")]
    NV = max(a[0].nv for a in air)
    NT = max(a[0].nt for a in air)
    NE = max(a[0].ne for a in air)
    NAF = max(a[4] for a in air)
    assert air[0][3].shape[0] != air[1][3].shape[0]           # (the polygons differ in length as well)
    B = 6
    af = np.array([0, 1, 0, 1, 1, 0], np.int32)

    def batch(polygon, which, airfoil=None):
        hb = HostTopologyBatch(len(which), NV, NT, NE, NAF, 180, 1536, polygon, ipcs=True, airfoil=airfoil)
        for b, a in enumerate(which):
            t0, x0, cells, _, _ = air[a]
            hb.coords[b, :t0.nv], hb.cells[b, :t0.nt], hb.nv[b], hb.nt[b] = x0, cells, t0.nv, t0.nt
            hb.offset[b] = b % 3
        rem = np.array([-1 if b < 2 else np.flatnonzero(~air[a][0].on_boundary)[10 * b] for b, a in enumerate(which)], np.int32)
        status = remesh_batch(hb.coords, hb.cells, hb.nv, hb.nt, rem, 50, 2)
        assert (status == 0).all()
        hb.run(2)
        return hb

    mixed = batch([a[3] for a in air], af, af)
    homo = [batch(air[a][3], af) for a in range(2)]          # every env on the same mesh rows, one polygon for all
    for b in range(B):
        ref = homo[af[b]]
        assert mixed.nv[b] == ref.nv[b] and mixed.nt[b] == ref.nt[b]
        for k in mixed.h:
            assert np.array_equal(mixed.h[k][b], ref.h[k][b]), (b, k)
        for k in mixed.hi:
            assert np.array_equal(mixed.hi[k][b], ref.hi[k][b]), (b, k)
    # ... and the two airfoils really select differently (the polygon matters)
    assert not np.array_equal(homo[0].h["coord_map"][0], homo[1].h["coord_map"][0])


def test_host_topology_rejects_bad_polygon_tables(meshes, lib_built):
    from meshdqn_amd.mesh_ops import HostTopologyBatch
    t0, _, _, poly, naf = _airfoil(meshes, "ys930")
    with pytest.raises(ValueError):
        HostTopologyBatch(2, t0.nv, t0.nt, t0.ne, naf, 180, 1536, [poly, poly])                       # no airfoil list
    with pytest.raises(ValueError):
        HostTopologyBatch(2, t0.nv, t0.nt, t0.ne, naf, 180, 1536, [poly, poly], airfoil=[0, 2])       # airfoil out of range


def _c_layout(tmp_path, cname, cls):
    from meshdqn_amd import _lib
    hdr = os.path.join(os.path.dirname(_lib.HERE), "include", "meshdqn_hip.h")
    fields = [n for n, _ in cls._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{hdr}"', 'int main(){', f'printf("%zu\\n", sizeof({cname}));']
    src += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f in fields]
    src.append('return 0;}')
    cfile = tmp_path / f"{cname}.c"
    cfile.write_text("\n".join(src))
    exe = tmp_path / cname
    subprocess.check_call(["gcc", str(cfile), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    return vals[0], vals[1:], [getattr(cls, f).offset for f in fields]


@pytest.mark.parametrize("cname,pyname", [("mdq_interp_src", "InterpSrc"), ("mdq_interp_desc", "InterpDesc"),
                                          ("mdq_env_topo_desc", "EnvTopoDesc"), ("mdq_env_finish_desc", "EnvFinishDesc")])
def test_new_struct_layouts_match_the_header(tmp_path, cname, pyname):
    """the ABI 8 struct (mdq_interp_src) and the three descriptors that gained per-airfoil fields: size and every offset."""
    from meshdqn_amd import _lib
    cls = getattr(_lib, pyname)
    size, c_off, py_off = _c_layout(tmp_path, cname, cls)
    assert size == C.sizeof(cls)
    assert c_off == py_off
    assert _lib.ABI_VERSION == 8
    names = {n for n, _ in cls._fields_}
    want = dict(InterpSrc={"src_cellrec", "bin_ptr"}, InterpDesc={"n_src", "src_of_env", "srcs"},
                EnvTopoDesc={"poly_ptr", "src_of_env"}, EnvFinishDesc={"src_of_env", "nv0_of", "src_stride"})[pyname]
    assert want <= names


def test_per_airfoil_restore_entry_points_are_declared():
    from meshdqn_amd import _lib, build
    for name in ("mdq_restore_rows_src", "mdq_restore_rows_masked_src"):
        assert name in build.declared_symbols() and name in _lib.SYMBOLS
