"""GPU: one batch over two airfoils (ys930 + ah93w145, ABI 8 per-airfoil sources).  Every environment of a mixed batch must
step exactly as the same environment of a batch of its own airfoil - through `step()` and `rollout_device` - and as its own
airfoil's oracle episode (tests/golden/oracle_stock_<mesh>.{json,npz}, loaded through the reference's snapshot-reload
branch, so no ground truth is recomputed here); resets go back to the environment's own airfoil; the S3 flow leg agrees with
the homogeneous batches and the sparse-LU oracle; a one-element config list is today's batch bit for bit; and the learning
loop, `train.py --config A --config B` and `deploy()` of the mixed-trained network work end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MESHES = ["ys930", "ah93w145"]
NV0 = {"ys930": 876, "ah93w145": 797}


# ---- helpers copied from tests/test_stock_gpu.py (snapshot-reload configs of the oracle's stock episodes)
def _fixture(mesh):
    ep = json.load(open(os.path.join(GOLDEN, f"oracle_stock_{mesh}.json")))
    z = np.load(os.path.join(GOLDEN, f"oracle_stock_{mesh}.npz"))
    return ep, z


def _cfg(mesh, ep, **agent):
    ap = dict(ep["agent_params"])
    ap.update(agent)
    return dict(flow_config=dict(flow_params=dict(mu=1e-3, rho=1.0, inflow="constant"),
                                 geometry_params=dict(mesh=os.path.join(GOLDEN, f"{mesh}.npz")),
                                 solver_params=dict(dt=0.001, solver_type="lu", smooth=True)),
                agent_params=ap)


def _snapshot_cfg(mesh, ep, z, tmp):
    """Config of an env that reloads the ORACLE's ground truth (the reference's second-and-later-episode branch)."""
    snap = os.path.join(str(tmp), "snapshots")
    os.makedirs(snap, exist_ok=True)
    u, p = z["u"], z["p"]                       # (5, 2 n2) in the oracle's [ux | uy] order, (5, nv)
    n2 = u.shape[1] // 2
    np.save(os.path.join(snap, "save_velocities.npy"), np.stack([u[:, :n2], u[:, n2:]], axis=2).reshape(len(u), -1))
    np.save(os.path.join(snap, "save_pressures.npy"), p)
    return _cfg(mesh, ep, gt_drag=z["gt_drag"].copy(), gt_lift=z["gt_lift"].copy(), gt_time=np.array([5.0]),
                plot_dir=str(tmp))


def _check_step(g, removed, nv, E, r, done, drags, lifts, where):
    assert bool(done) == g["done"], where
    assert abs(r - g["reward"]) < 1e-6, (where, r, g["reward"])
    assert nv == g["nv"], where
    if E is not None:
        assert E == g["E"], where
    if removed is not None:
        assert removed == g["removed_vertex"], where
    if "nt" in g and drags is not None:
        assert np.allclose(drags, g["new_drags"], rtol=1e-7, atol=0), where
        assert np.allclose(lifts, g["new_lifts"], rtol=1e-7, atol=0), where


# ---- the two airfoils, built once per module
@pytest.fixture(scope="module")
def airfoils(lib_built, tmp_path_factory):
    from meshdqn_amd.env import Env2DAirfoil
    out = []
    for mesh in MESHES:
        ep, z = _fixture(mesh)
        cfg = _snapshot_cfg(mesh, ep, z, tmp_path_factory.mktemp(mesh))
        out.append(dict(mesh=mesh, ep=ep, z=z, cfg=cfg, base=Env2DAirfoil(cfg)))
    return out


def _episodes(air):
    """(names, actions (K, #episodes)) of one airfoil's stock episodes; an env whose episode is over keeps shifting (180)."""
    names = list(air["ep"]["episodes"])
    return names, [[g["action"] for g in air["ep"]["episodes"][n]["steps"]] for n in names]


def _mixed_script(airfoils):
    """B = 8, airfoils alternate (env b: airfoil b % 2), env b replays episode b // 2 (mod #episodes) of its airfoil.  -> acts (K, 8),
    per env (airfoil, episode name), and per airfoil the (K, 4) actions of its homogeneous batch (env j = mixed env 2 j + a)."""
    eps = [_episodes(a) for a in airfoils]
    B = 8
    K = max(len(s) for _, e in eps for s in e)
    acts = np.full((K, B), 180, np.int64)
    who = []
    for b in range(B):
        a = b % 2
        e = (b // 2) % len(eps[a][1])
        s = eps[a][1][e]
        acts[:len(s), b] = s
        who.append((a, eps[a][0][e]))
    homo = [acts[:, a::2].copy() for a in range(2)]
    return acts, who, homo


def _venv(cfg, B, base, **kw):
    from meshdqn_amd.vec_env import VecEnv2DAirfoil
    return VecEnv2DAirfoil(cfg, B, base_env=base, nthreads=2, **kw)


def _env_state(st, b):
    e0, e1 = int(st["edge_ptr"][b]), int(st["edge_ptr"][b + 1])
    return (st["x"][b].cpu().numpy(), st["esrc"][e0:e1].cpu().numpy(), st["edst"][e0:e1].cpu().numpy())


def _same_state(s1, s2, where):
    for u, v in zip(s1, s2):
        assert u.shape == v.shape and np.array_equal(u, v), where


def test_mixed_batch_steps_like_homogeneous_batches_and_the_oracle(airfoils):
    """S1, `step()`: every env of the alternating B = 8 batch == the same env of the batch of its own airfoil, bit for bit
    (rewards, dones, codes, nv / nt, coord_map / n_closest, the state's x and edge lists, new_drags / new_lifts), and ==
    its airfoil's oracle episode (removals exact, rewards <= 1e-6, terminal at the 44th / 40th removal of far_field)."""
    acts, who, homo_acts = _mixed_script(airfoils)
    K, B = acts.shape
    cfgs, bases = [a["cfg"] for a in airfoils], [a["base"] for a in airfoils]
    mixed = _venv(cfgs, B, bases, auto_reset=False)
    assert mixed.A == 2 and mixed.airfoil.tolist() == [0, 1] * 4 and len(mixed.bases) == 2
    homo = [_venv(cfgs[a], 4, bases[a], auto_reset=False) for a in range(2)]
    assert mixed.NV == max(h.NV for h in homo) and mixed.NT == max(h.NT for h in homo)
    st, hst = mixed.get_state(), [h.get_state() for h in homo]
    removals = np.zeros(B, int)
    for k in range(K):
        removed = [int(st["coord_map"][b][acts[k, b]]) if acts[k, b] != 180 else -1 for b in range(B)]
        st, rew, done, info = mixed.step(acts[k])
        hout = [h.step(homo_acts[a][k]) for a, h in enumerate(homo)]
        for b in range(B):
            a, j = b % 2, b // 2
            hs, hr, hd, hi = hout[a]
            h = homo[a]
            where = (MESHES[a], who[b][1], k)
            assert rew[b] == hr[j] and done[b] == hd[j] and info["code"][b] == hi["code"][j], where
            assert mixed.nv[b] == h.nv[j] and mixed.nt[b] == h.nt[j], where
            assert np.array_equal(st["coord_map"][b], hs["coord_map"][j]) and np.array_equal(st["n_closest"][b], hs["n_closest"][j])
            _same_state(_env_state(st, b), _env_state(hs, j), where)
            assert np.array_equal(info["new_drags"][b], hi["new_drags"][j]) and np.array_equal(info["new_lifts"][b], hi["new_lifts"][j])
            s = airfoils[a]["ep"]["episodes"][who[b][1]]["steps"]
            if k < len(s):
                _check_step(s[k], removed[b], int(info["nv"][b]), int(st["edge_ptr"][b + 1] - st["edge_ptr"][b]), rew[b], done[b],
                            info["new_drags"][b], info["new_lifts"][b], where)
                removals[b] += acts[k, b] != 180
        assert info["nv"][0::2].max() <= NV0["ys930"] and info["nv"][1::2].max() <= NV0["ah93w145"]
    ff = [b for b in range(B) if who[b][1] == "far_field"]
    assert {b % 2 for b in ff} == {0, 1} and all(removals[b] == (44, 40)[b % 2] for b in ff)


def test_mixed_device_rollout_equals_homogeneous_rollouts(airfoils):
    """S1, `rollout_device(actions=...)` (mdq_env_finish with per-airfoil gt_drag / nv0): per-step rewards, dones, codes and
    vertex counts bit for bit against the homogeneous batches; coord_map / n_closest / forces / state where a chunk ends; and
    the oracle's rewards and vertex counts."""
    acts, who, homo_acts = _mixed_script(airfoils)
    K, B = acts.shape
    cfgs, bases = [a["cfg"] for a in airfoils], [a["base"] for a in airfoils]
    mixed = _venv(cfgs, B, bases, auto_reset=False)
    homo = [_venv(cfgs[a], 4, bases[a], auto_reset=False) for a in range(2)]
    mixed.get_state()
    for h in homo:
        h.get_state()
    k0, chunks = 0, [1, 3, 16, 100]
    while k0 < K:
        n = min(chunks.pop(0) if chunks else 128, K - k0)
        out = mixed.rollout_device(None, n, actions=acts[k0:k0 + n])
        hout = [h.rollout_device(None, n, actions=homo_acts[a][k0:k0 + n]) for a, h in enumerate(homo)]
        for b in range(B):
            a, j = b % 2, b // 2
            for key in ("rewards", "dones", "codes", "nv"):
                assert np.array_equal(out[key][:, b], hout[a][key][:, j]), (key, b, k0)
            for key in ("coord_map", "n_closest", "nsel", "nedges"):
                assert np.array_equal(mixed.h[key][b], homo[a].h[key][j]), (key, b, k0)
            assert np.array_equal(mixed.new_drags[b], homo[a].new_drags[j]) and np.array_equal(mixed.new_lifts[b], homo[a].new_lifts[j])
            s = airfoils[a]["ep"]["episodes"][who[b][1]]["steps"]
            for q in range(n):
                if k0 + q < len(s):
                    assert out["codes"][q, b] == 0
                    _check_step(s[k0 + q], None, int(out["nv"][q, b]), None, out["rewards"][q, b], out["dones"][q, b], None, None,
                                (MESHES[a], b, k0 + q))
        st, hst = mixed.get_state(), [h.get_state() for h in homo]
        for b in range(B):
            _same_state(_env_state(st, b), _env_state(hst[b % 2], b // 2), (b, k0))
        k0 += n


def test_terminated_environments_reset_to_their_own_airfoil(airfoils):
    """auto_reset: the far_field episodes end on the vertex criterion (44th / 40th removal); the environment comes back with
    its OWN airfoil's vertex count (876 / 797) and its next state equals that airfoil's initial state bit for bit - through
    `step()` (host reset logic) and through the device-resident rollout (mdq_env_finish: per-airfoil cached rows and
    features, mdq_restore_rows_src)."""
    cfgs, bases = [a["cfg"] for a in airfoils], [a["base"] for a in airfoils]
    ff = [[g["action"] for g in a["ep"]["episodes"]["far_field"]["steps"]] for a in airfoils]
    B = 4                                               # airfoils 0, 1, 0, 1: every env replays far_field of its airfoil
    K = max(len(s) for s in ff)
    acts = np.full((K, B), 180, np.int64)
    for b in range(B):
        acts[:len(ff[b % 2]), b] = ff[b % 2]
    end = [len(ff[b % 2]) - 1 for b in range(B)]        # the step at which env b terminates
    for path in ("step", "rollout"):
        venv = _venv(cfgs, B, bases, auto_reset=True)
        st0 = venv.get_state()
        init = [_env_state(st0, b) for b in range(B)]
        assert venv.nv.tolist() == [NV0["ys930"], NV0["ah93w145"]] * 2
        if path == "step":
            for k in range(K):
                st, rew, done, info = venv.step(acts[k])
                for b in range(B):
                    if k == end[b]:
                        assert done[b] and info["nv"][b] < 0.95 * NV0[MESHES[b % 2]], (b, k)
                        assert venv.nv[b] == NV0[MESHES[b % 2]], (b, k)
                        _same_state(_env_state(st, b), init[b], (path, b))
                    elif k < end[b]:
                        assert not done[b], (b, k)
        else:
            k0 = 0
            for k_end in sorted(set(end)):
                n = k_end + 1 - k0
                ro = venv.rollout_begin(n, actions=acts[k0:k_end + 1])
                for _ in range(n):
                    venv.rollout_step(ro, None)
                x_dev = ro["state"]["x"].cpu().numpy()          # the node features mdq_env_finish wrote for the next state
                out = venv.rollout_end(ro)
                st = venv.get_state()
                for b in range(B):
                    if end[b] == k_end:
                        assert out["dones"][-1, b] and venv.nv[b] == NV0[MESHES[b % 2]], (b, k_end)
                        assert np.array_equal(x_dev[b], init[b][0]), (path, b)
                        _same_state(_env_state(st, b), init[b], (path, b))
                    assert not out["dones"][:-1, b].any() or end[b] < k0
                k0 = k_end + 1


@pytest.mark.parametrize("overlap", [False, True])
def test_s3_flow_leg_of_a_mixed_batch(airfoils, overlap):
    """S3 (flow_steps=1): the IPCS step on every coarsened mesh of the mixed batch (warm start from its own airfoil's
    interpolated snapshots, inflow profile from its own mesh) agrees with the homogeneous batches (mode 3 accumulates with
    LDS fp64 atomics: round-off, not bits) and with the sparse-LU oracle on one sampled env per airfoil; status words 0."""
    from oracle.ipcs import OracleFlowSolver
    acts, who, homo_acts = _mixed_script(airfoils)
    K = 6
    cfgs, bases = [a["cfg"] for a in airfoils], [a["base"] for a in airfoils]
    kw = dict(auto_reset=False, flow_steps=1, flow_overlap=overlap)
    envs = [_venv(cfgs, 8, bases, **kw)] + [_venv(cfgs[a], 4, bases[a], **kw) for a in range(2)]
    res = []
    for venv, A in zip(envs, [acts, homo_acts[0], homo_acts[1]]):
        venv.get_state()
        for k in range(K):
            _, _, _, info = venv.step(A[k])
        if overlap:
            fd, fl = venv.flow_wait()
        else:
            fd, fl = info["flow_drag"], info["flow_lift"]
        assert (venv.flow_status.cpu().numpy() == 0).all()
        assert np.isfinite(fd).all() and np.isfinite(fl).all()
        res.append((fd, fl))
    mixed = envs[0]
    for b in range(8):
        a, j = b % 2, b // 2
        assert np.allclose(res[0][0][b], res[1 + a][0][j], rtol=1e-9, atol=0), b
        assert np.allclose(res[0][1][b], res[1 + a][1][j], rtol=1e-9, atol=1e-12 * abs(res[1 + a][0][j][0])), b
    for b in (6, 7):                                          # one env of each airfoil against the oracle on its very mesh
        nv, nt = int(mixed.nv[b]), int(mixed.nt[b])
        n2 = nv + int(mixed.h["ne"][b])
        o = OracleFlowSolver(mixed.coords[b, :nv].copy(), mixed.cells[b, :nt].copy(), smooth=False)
        assert o.th.np2 == n2
        u0 = mixed.u[b, mixed.S - 1, :n2].cpu().numpy()
        o.u_n = np.concatenate([u0[:, 0], u0[:, 1]])
        o.p_n = mixed.p[b, mixed.S - 1, :nv].cpu().numpy().copy()
        _, _, do, lo = o.evolve()
        scale = max(abs(do), abs(lo))
        fd, fl = res[0]
        assert abs(fd[b, 0] - do) < 1e-7 * abs(do) and abs(fl[b, 0] - lo) < 1e-7 * scale, (b, fd[b, 0], do, fl[b, 0], lo)


@pytest.mark.parametrize("flow_steps", [0, 1])
def test_one_element_config_list_is_todays_batch(airfoils, flow_steps):
    """`VecEnv2DAirfoil([cfg], ...)` == `VecEnv2DAirfoil(cfg, ...)` bit for bit over a scripted rollout (step() and
    rollout_device), S1 and S3 (the flow forces: to round-off of mode 3's LDS atomics)."""
    air = airfoils[0]
    names, eps = _episodes(air)
    B, K = 4, 12
    acts = np.full((2 * K, B), 180, np.int64)
    for b in range(B):
        s = eps[b][:2 * K]
        acts[:len(s), b] = s
    kw = dict(auto_reset=True, flow_steps=flow_steps)
    one, lst = _venv(air["cfg"], B, air["base"], **kw), _venv([air["cfg"]], B, [air["base"]], **kw)
    assert lst.A == 1 and lst.airfoil.tolist() == [0] * B and lst.initial_num_node == one.initial_num_node == NV0["ys930"]
    s1, s2 = one.get_state(), lst.get_state()
    for k in range(K):
        s1, r1, d1, i1 = one.step(acts[k])
        s2, r2, d2, i2 = lst.step(acts[k])
        assert np.array_equal(r1, r2) and np.array_equal(d1, d2) and np.array_equal(i1["code"], i2["code"]), k
        assert np.array_equal(i1["nv"], i2["nv"]) and np.array_equal(i1["new_drags"], i2["new_drags"])
        for b in range(B):
            _same_state(_env_state(s1, b), _env_state(s2, b), (b, k))
        if flow_steps:
            assert np.allclose(i1["flow_drag"], i2["flow_drag"], rtol=1e-9, atol=0)
    o1 = one.rollout_device(None, K, actions=acts[K:])
    o2 = lst.rollout_device(None, K, actions=acts[K:])
    for key in ("rewards", "dones", "codes", "nv", "actions"):
        assert np.array_equal(o1[key], o2[key]), key
    assert np.array_equal(one.new_drags, lst.new_drags) and np.array_equal(one.h["coord_map"], lst.h["coord_map"])


def test_learning_loop_on_a_mixed_batch(airfoils):
    """`train_loop_device` on B = 16 environments of both airfoils: finite losses after a few optimiser steps, and the
    replay ring holds transitions of both airfoils (state features of the first env of each airfoil found in it)."""
    import random
    from meshdqn_amd.trainer import DistContext, DQNTrainer, train_loop_device
    cfgs, bases = [a["cfg"] for a in airfoils], [a["base"] for a in airfoils]
    np.random.seed(5)
    random.seed(5)
    venv = _venv(cfgs, 16, bases)
    x0 = venv.get_state()["x"].cpu()
    tr = DQNTrainer(n_actions=180, num_inputs=17, ctx=DistContext(), batch_size=8, lr=1e-3)
    out = train_loop_device(tr, venv, 6, eps_decay=2, chunk=3)
    assert len(out["losses"]) >= 4 and np.isfinite(out["losses"]).all()
    assert np.isfinite(out["rewards"]).all() and out["rewards"].shape == (6, 16)
    rep = tr.device_memory
    ring = rep.R[:min(6 * 16, rep.capacity)].cpu()
    for a in range(2):                       # the initial state of an airfoil-a env is the state part of its first record
        xa = x0[a].reshape(-1)
        assert any(torch.equal(ring[r, :xa.numel()], xa) for r in range(16)), a


def test_train_py_with_two_configs_and_deploy_per_airfoil(airfoils, tmp_path):
    """`train.py --config A --config B`: checkpoints, the per-airfoil episode log (`airfoil.npy`, one entry per finished
    episode, both airfoils), then the mixed-trained `policy_net_1.pt` deployed on each airfoil with today's `deploy()`."""
    import yaml
    from meshdqn_amd.deploy import deploy
    from meshdqn_amd.env import Env2DAirfoil
    from meshdqn_amd.trainer import DistContext, DQNTrainer
    paths = []
    for a in airfoils:
        cfg = json.loads(json.dumps(a["cfg"], default=lambda v: np.asarray(v).tolist()))
        cfg["agent_params"]["timesteps"] = 3                     # episodes end every 3 steps: the log gets entries
        p = os.path.join(str(tmp_path), f"{a['mesh']}.yaml")
        yaml.safe_dump(cfg, open(p, "w"))
        paths.append(p)
    save = os.path.join(str(tmp_path), "run")
    cmd = [sys.executable, "train.py", "--config", paths[0], "--config", paths[1], "--envs", "4", "--steps", "7",
           "--save-dir", save, "--save-every", "0"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run(["timeout", "-k", "10", "600"] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=660)
    assert out.returncode == 0, out.stderr[-4000:]
    for f in ("policy_net_1.pt", "policy_net_2.pt", "config.yaml", "config_1.yaml", "step_rewards.npy", "reward.npy", "airfoil.npy"):
        assert os.path.exists(os.path.join(save, f)), f
    af = np.load(os.path.join(save, "airfoil.npy"))
    rewards = np.load(os.path.join(save, "reward.npy"))
    assert af.shape == rewards.shape and len(af) >= 4 and set(af.tolist()) == {0, 1}
    tr = DQNTrainer(n_actions=180, num_inputs=17, ctx=DistContext())
    tr.load(save)
    for a in airfoils:
        env = Env2DAirfoil(a["cfg"])
        res = deploy(env, tr.policy_net_1, complete_traj=False, max_steps=3, final_sim=False)
        assert 1 <= len(res["actions"]) <= 3
        assert len(env.flow_solver.mesh.coordinates()) <= NV0[a["mesh"]]
