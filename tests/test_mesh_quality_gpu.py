"""GPU: the mesh-quality kernel (`mdq_mesh_quality`) against the plain-loop restatement tests/quality_ref.py BIT FOR BIT (the
metric has fixed arithmetic: no contraction, no sqrt, no transcendental, order-independent reductions), the quality part
of the env step's reward / stop through the C ABI (`mdq_env_result_quality`, `mdq_env_finish` with the appended descriptor
fields) against the same file, and end to end through `VecEnv2DAirfoil`: `step()` (host formula, meshdqn_amd/reward.py)
against `rollout_device(actions=...)` (kernel), the stop on the smallest angle, and "off" == "neutral" bit for bit.

Tolerance of the rewards: 1e-12, the argument of tests/test_lift_reward_gpu.py (O(1) values; one `log`, two `exp`, two
`sqrt` within a few ulp each; the quality part adds correctly rounded operations only).  Everything else exactly."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import quality_ref as ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PAR = ref.PAR
f64, i32, u8 = torch.float64, torch.int32, torch.uint8
GUARD_F, GUARD_I, GUARD_B = -777.25, -77777, 0xA5
INF = math.inf


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------- 1: the kernel
NTS = [0, 1, 63, 64, 65, 255, 256, 257, 511, 1025, 1100, 1100]


def _planted_case():
    """B = 12, NV = 96, NT = 1100: seeded points, cells as random distinct triples below nv[b], and per environment (where
    nt[b] leaves room) the planted cells the issue lists.  Rows behind nt[b] hold (0, 0, 0); coordinates behind nv[b] hold NaN
    except the three a planted cell would - wrongly - read an equilateral triangle from."""
    rng = np.random.default_rng(2024)
    B, NV, NT = 12, 96, 1100
    nt = np.array(NTS, np.int32)
    nv = np.array([40, 17, 96, 50, 64, 33, 96, 72, 80, 90, 96, 61], np.int32)
    coords = np.full((B, NV, 2), np.nan)
    cells = np.zeros((B, NT, 3), np.int32)
    planted = {}
    h = math.sqrt(3.0) / 2.0
    for b in range(B):
        n, m = int(nv[b]), int(nt[b])
        coords[b, :n] = rng.random((n, 2)) * [2.0, 1.0] + [0.25, 0.25]
        for t in range(m):
            cells[b, t] = rng.choice(n, 3, replace=False)
        if n + 3 <= NV:             # what a missing range check would read: q = 1, better than any cell
            coords[b, n:n + 3] = [[0.0, 0.0], [1.0, 0.0], [0.5, h]]
        slots = list(rng.permutation(m)[:8]) if m >= 16 else []
        if slots:
            s = [int(v) for v in slots]
            # a collinear cell (three points on the line y = 0.5 x, exactly representable)
            coords[b, 0], coords[b, 1], coords[b, 2] = [0.5, 0.25], [1.0, 0.5], [1.5, 0.75]
            cells[b, s[0]] = 0, 1, 2
            cells[b, s[1]] = 5, 9, 5                                     # a repeated vertex ... and s = 0:
            cells[b, s[2]] = 7, 7, 7
            # two congruent cells, the second shifted by an exact power of two: the same q and cot, bit for bit
            coords[b, 10], coords[b, 11], coords[b, 12] = [0.5, 0.5], [0.75, 0.5], [0.5, 0.5625]
            coords[b, 13:16] = coords[b, 10:13] + 2.0
            lo, hi = sorted((s[3], s[4]))
            cells[b, hi], cells[b, lo] = (10, 11, 12), (13, 14, 15)
            if n + 3 <= NV:
                cells[b, s[5]] = n, n + 1, n + 2                          # ids in [nv, NV)
            cells[b, s[6]] = 3, -1, 4                                    # id -1
            cells[b, s[7]] = 3, 4, NV                                    # id NV
            planted[b] = s
    return B, NV, NT, coords, cells, nv, nt, planted


def _launch(coords, cells, nv, nt, q_floor):
    """One launch on arrays with a guard environment row in front of and behind `coords` (equilateral triangles everywhere: a
    missing range check shows as a wrong number, never as a fault) and guard words behind qual / qinfo."""
    from meshdqn_amd import _lib
    lib = _lib.load()
    B, NV, NT = coords.shape[0], coords.shape[1], cells.shape[1]
    h = math.sqrt(3.0) / 2.0
    big = np.tile(np.array([[0.0, 0.0], [1.0, 0.0], [0.5, h]]), ((B + 2) * NV // 3 + 1, 1))[:(B + 2) * NV].reshape(B + 2, NV, 2)
    big[1:B + 1] = coords
    t_big = _dev(big)
    t_cells, t_nv, t_nt = _dev(cells), _dev(nv), _dev(nt)
    qual = torch.full((B + 1, 2), GUARD_F, dtype=f64, device="cuda")
    qinfo = torch.full((B + 1, 4), GUARD_I, dtype=i32, device="cuda")
    rc = lib.mdq_mesh_quality(B, NV, NT, t_big[1:].data_ptr(), t_cells.data_ptr(), t_nv.data_ptr(), t_nt.data_ptr(), q_floor,
                              qual.data_ptr(), qinfo.data_ptr(), _lib.stream_ptr())
    assert rc == 0, lib.mdq_last_error()
    torch.cuda.synchronize()
    qual, qinfo = qual.cpu().numpy(), qinfo.cpu().numpy()
    assert (qual[B] == GUARD_F).all() and (qinfo[B] == GUARD_I).all()
    return qual[:B], qinfo[:B]


def test_kernel_equals_the_loop_reference_bit_for_bit(lib_built):
    B, NV, NT, coords, cells, nv, nt, planted = _planted_case()
    q_floor = 0.25
    want_q, want_i = ref.batch_mesh(coords, cells, nv, nt, q_floor)
    got_q, got_i = _launch(coords, cells, nv, nt, q_floor)
    for b in range(B):
        print(f"b={b} nt={nt[b]} nv={nv[b]}: kernel {got_q[b].tolist()} {got_i[b].tolist()}  reference {want_q[b].tolist()} {want_i[b].tolist()}")
    assert np.array_equal(_bits(got_q), _bits(want_q))
    assert np.array_equal(got_i, want_i)
    # what the planted cells must have done: nt = 0 reports the empty mesh; every environment with planted cells is at its worst,
    # at the LOWEST worst index (a planted one, unless a random triple in front of it happens to be degenerate as well); the
    # congruent pair ties exactly and all of them count as below the floor
    assert got_q[0].tolist() == [0.0, INF] and got_i[0].tolist() == [-1, -1, 0, 0]
    for b, s in planted.items():
        worst = [t for t in s if ref.mesh(coords[b], cells[b][t:t + 1], nv[b], 1)[:2] == (0.0, INF)]
        assert len(worst) >= 5 and got_q[b].tolist() == [0.0, INF] and got_i[b, 0] == got_i[b, 1] <= min(worst)
        pair = [t for t in range(nt[b]) if tuple(cells[b, t]) in ((10, 11, 12), (13, 14, 15))]
        a, c = (ref.mesh(coords[b], cells[b][t:t + 1], nv[b], 1)[:2] for t in pair)
        assert len(pair) == 2 and a == c and 0.0 < a[0] < 1.0
        assert got_i[b, 2] >= len(worst)
    # ... and without the worst cells the tie decides: the two congruent cells alone, the lower index wins either way round
    b = 10
    for order in ((0, 1), (1, 0)):
        two = np.zeros((1, 2, 3), np.int32)
        two[0, order[0]], two[0, order[1]] = (10, 11, 12), (13, 14, 15)
        q2, i2 = _launch(coords[b:b + 1], two, nv[b:b + 1], np.array([2], np.int32), 0.0)
        w2, wi2 = ref.batch_mesh(coords[b:b + 1], two, nv[b:b + 1], [2], 0.0)
        assert np.array_equal(_bits(q2), _bits(w2)) and i2[0].tolist() == wi2[0].tolist() == [0, 0, 0, 0]
    # a second launch: identical bits
    again_q, again_i = _launch(coords, cells, nv, nt, q_floor)
    assert np.array_equal(_bits(again_q), _bits(got_q)) and np.array_equal(again_i, got_i)
    # the same meshes with the worst cells taken out again (random triples in their rows; the congruent pair stays): now the
    # reductions carry real numbers in every environment, spread over one to four waves and up to five cells per thread
    rng = np.random.default_rng(7)
    plain = cells.copy()
    for b in planted:          # (the planted ones, and a random triple that happens to be (0, 1, 2))
        for t in range(nt[b]):
            if ref.mesh(coords[b], plain[b][t:t + 1], nv[b], 1)[0] == 0.0:
                plain[b, t] = rng.choice(np.arange(16, int(nv[b])), 3, replace=False)
    want_q, want_i = ref.batch_mesh(coords, plain, nv, nt, q_floor)
    got_q, got_i = _launch(coords, plain, nv, nt, q_floor)
    assert np.array_equal(_bits(got_q), _bits(want_q)) and np.array_equal(got_i, want_i)
    assert (got_q[1:, 0] > 0.0).all() and np.isfinite(got_q[1:, 1]).all() and len(set(got_q[1:, 0])) == B - 1


# ---------------------------------------------------------------------------------------------------------- 2: real meshes
@pytest.fixture(scope="module")
def real_meshes(lib_built):
    """name -> (coords, cells) as read back from the device: ys930 and ah93w145 after 50 sweeps of mdq_smooth, the red-refined
    and the twice-refined ys930 as committed."""
    from meshdqn_amd.mesh_ops import smooth_batch_gpu
    out = {}
    for name in ("ys930", "ah93w145"):
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        c, t = _dev(z["coords"][None]), _dev(z["cells"][None].astype(np.int32))
        nv, nt = _dev(np.array([c.shape[1]], np.int32)), _dev(np.array([t.shape[1]], np.int32))
        smooth_batch_gpu(c, t, nv, nt, _dev(np.array([50], np.int32)), fast=False)
        torch.cuda.synchronize()
        out[name] = (c[0].cpu().numpy(), t[0].cpu().numpy())
        assert not np.array_equal(out[name][0], z["coords"])
    for name in ("oracle_stock_ys930_refined", "oracle_stock_ys930_refined2"):
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        out[name] = (np.ascontiguousarray(z["coords"], dtype=np.float64), np.ascontiguousarray(z["cells"], dtype=np.int32))
    assert len(out["oracle_stock_ys930_refined"][1]) == 6280
    return out


@pytest.mark.parametrize("name", ["ys930", "ah93w145", "oracle_stock_ys930_refined", "oracle_stock_ys930_refined2"])
def test_real_meshes_alone_and_inside_a_batch(real_meshes, name):
    from meshdqn_amd.mesh_ops import mesh_quality_gpu
    coords, cells = real_meshes[name]
    nv, nt = len(coords), len(cells)
    q_floor = 0.6
    want = ref.mesh(coords, cells, nv, nt, q_floor)
    print(f"{name}: nv {nv} nt {nt} q_min {want[0]!r} (cell {want[2]}) smallest angle {ref.min_angle_deg(want[1]):.4f} deg "
          f"(cell {want[3]}) cells below {q_floor}: {want[4]}")
    assert 0.0 < want[0] < 1.0 and 0 < want[4] < nt
    qual, qinfo = mesh_quality_gpu(_dev(coords[None]), _dev(cells[None]), _dev(np.array([nv], np.int32)),
                                   _dev(np.array([nt], np.int32)), q_floor)
    one = (qual.cpu().numpy(), qinfo.cpu().numpy())
    assert np.array_equal(_bits(one[0][0]), _bits(want[:2])) and one[1][0].tolist() == [want[2], want[3], want[4], 0]
    # environment 3 of B = 5, at a larger capacity, between the smoothed ys930 (rows padded with NaN / zeros behind nv / nt)
    other_c, other_t = real_meshes["ys930"]
    B, NV, NT = 5, max(nv, len(other_c)) + 7, max(nt, len(other_t)) + 5
    bc, bt = np.full((B, NV, 2), np.nan), np.zeros((B, NT, 3), np.int32)
    bnv, bnt = np.full(B, len(other_c), np.int32), np.full(B, len(other_t), np.int32)
    bc[:, :len(other_c)], bt[:, :len(other_t)] = other_c, other_t
    bc[3], bt[3] = np.nan, 0
    bc[3, :nv], bt[3, :nt], bnv[3], bnt[3] = coords, cells, nv, nt
    qual, qinfo = mesh_quality_gpu(_dev(bc), _dev(bt), _dev(bnv), _dev(bnt), q_floor)
    assert np.array_equal(_bits(qual[3].cpu().numpy()), _bits(one[0][0])) and np.array_equal(qinfo[3].cpu().numpy(), one[1][0])
    w0 = ref.mesh(other_c, other_t, len(other_c), len(other_t), q_floor)
    for b in (0, 1, 2, 4):
        assert np.array_equal(_bits(qual[b].cpu().numpy()), _bits(w0[:2])) and qinfo[b].tolist() == [w0[2], w0[3], w0[4], 0]


# ---------------------------------------------------------------------------------------------------------- 3: refusals
BAD_QUALITY_CALL = [("B", 0), ("NV", 0), ("NT", -1), ("coords", None), ("cells", None), ("nv", None), ("nt", None), ("qual", None),
                    ("qinfo", None), ("q_floor", -0.1), ("q_floor", 1.5), ("q_floor", math.nan), ("q_floor", math.inf)]


@pytest.mark.parametrize("what,value", BAD_QUALITY_CALL)
def test_mesh_quality_refuses_before_the_launch(lib_built, what, value):
    from meshdqn_amd import _lib
    lib = _lib.load()
    z = np.load(os.path.join(GOLDEN, "ys930.npz"))
    t = dict(coords=_dev(z["coords"][None]), cells=_dev(z["cells"][None].astype(np.int32)), nv=_dev(np.array([876], np.int32)),
             nt=_dev(np.array([1570], np.int32)), qual=torch.full((1, 2), GUARD_F, dtype=f64, device="cuda"),
             qinfo=torch.full((1, 4), GUARD_I, dtype=i32, device="cuda"))
    a = dict(B=1, NV=876, NT=1570, q_floor=0.5, **{k: v.data_ptr() for k, v in t.items()})
    a[what] = value
    rc = lib.mdq_mesh_quality(a["B"], a["NV"], a["NT"], a["coords"], a["cells"], a["nv"], a["nt"], a["q_floor"], a["qual"], a["qinfo"],
                              _lib.stream_ptr())
    assert rc != 0 and b"mdq_mesh_quality" in lib.mdq_last_error()
    torch.cuda.synchronize()
    assert (t["qual"] == GUARD_F).all() and (t["qinfo"] == GUARD_I).all()
    a[what] = dict(B=1, NV=876, NT=1570, q_floor=1.0).get(what, t[what].data_ptr() if what in t else None)
    assert lib.mdq_mesh_quality(a["B"], a["NV"], a["NT"], a["coords"], a["cells"], a["nv"], a["nt"], a["q_floor"], a["qual"], a["qinfo"],
                                _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert 0.0 < float(t["qual"][0, 0]) < 1.0 and int(t["qinfo"][0, 3]) == 0


# ---------------------------------------------------------------------------------------------------------- 4: the result
def _outputs(B):
    return dict(rew=torch.full((B + 2,), GUARD_F, dtype=f64, device="cuda"), done=torch.full((B + 8,), GUARD_B, dtype=u8, device="cuda"),
                reason=torch.full((B + 2,), GUARD_I, dtype=i32, device="cuda"), err=torch.zeros(1, dtype=i32, device="cuda"),
                nvo=torch.full((B,), GUARD_I, dtype=i32, device="cuda"))


def _result(c, lift, auto_reset, quality=None, q_ref=None, qpar=(0.0, 0.0, INF), entry="quality", only=None):
    """One launch of mdq_env_result_forces (entry "forces") or mdq_env_result_quality on case `c` (airfoil 0's ground truth);
    `lift` = None or (w, T, F); `only` = "quality" / "quality_ref": that pointer alone."""
    from meshdqn_amd import _lib
    lib = _lib.load()
    B, N, S = c["B"], c["N"], c["S"]
    o = _outputs(B)
    t = dict(drags=_dev(c["drags"]), gt=_dev(c["gt_drag"][0]), nv=_dev(c["nv"]), rstat=_dev(c["rstat"]), tstat=_dev(c["tstat"]),
             nsel=_dev(c["nsel"]), code=_dev(c["code"]), steps=_dev(c["steps"]), lifts=_dev(c["lifts"]), gl=_dev(c["gt_lift"][0]))
    head = (B, N, S, t["drags"].data_ptr(), t["gt"].data_ptr(), t["nv"].data_ptr(), int(c["nv0"][0]), t["rstat"].data_ptr(),
            t["tstat"].data_ptr(), t["nsel"].data_ptr(), t["code"].data_ptr(), t["steps"].data_ptr(), PAR["threshold"],
            PAR["time_reward"], PAR["goal_vertices"], PAR["timesteps"], PAR["negative_reward"], int(auto_reset), o["rew"].data_ptr(),
            o["done"].data_ptr(), o["err"].data_ptr(), o["nvo"].data_ptr(), _ptr(t["lifts"] if lift else None),
            _ptr(t["gl"] if lift else None), *(lift or (0.0, 0.0, 0.0)), o["reason"].data_ptr())
    if entry == "forces":
        rc = lib.mdq_env_result_forces(*head, _lib.stream_ptr())
    else:
        tq = None if quality is None else _dev(quality)
        tr = None if q_ref is None else _dev(np.array([q_ref], np.float64))
        rc = lib.mdq_env_result_quality(*head, _ptr(None if only == "quality_ref" else tq), _ptr(None if only == "quality" else tr),
                                        *qpar, _lib.stream_ptr())
    msg = lib.mdq_last_error() if rc != 0 else b""
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in o.items()}
    out.update(code=t["code"].cpu(), steps=t["steps"].cpu(), rc=rc, msg=msg)
    return out


@pytest.mark.parametrize("B", [1, 129, 130])
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("lift", [None, (0.5, 1e-3, 0.05)])
def test_env_result_quality_against_the_loop_reference(lib_built, B, S, lift):
    """The seeded cases of the lift test (one block of the 128-thread kernel, and two with the second nearly empty), extended by
    quality columns on both sides of both thresholds."""
    qpar, q_ref = (0.75, 0.3, ref.max_cot(12.0)), 0.45
    seen = 0
    for auto_reset in (0, 1):
        for special in ([None] + list(range(6)) if B < 8 else [None]):
            c = ref.random_case(1000 * B + 10 * S + auto_reset, B, S, T=1e-3, F=0.05, special=special)
            quality = ref.quality_columns(B + S + auto_reset, B, Qm=qpar[1], mc=qpar[2], q_ref=q_ref)
            o = _result(c, lift, auto_reset, quality, q_ref, qpar)
            assert o["rc"] == 0, o["msg"]
            code = ref.final_codes(c["code"], c["rstat"], c["tstat"], c["nsel"], c["N"])
            rew, done, reason, st = ref.batch(c["drags"], c["gt_drag"][0], c["nv"], c["nv0"][0], code, c["steps"], PAR,
                                              *((None, None, None) if lift is None else (c["lifts"], c["gt_lift"][0], lift)),
                                              quality, q_ref, qpar)
            steps = np.where(done & bool(auto_reset), 0, st).astype(np.int32)
            print(f"B={B} S={S} lift={lift} auto_reset={auto_reset} special={special}: largest reward error "
                  f"{np.abs(o['rew'][:B].numpy() - rew).max():.3e}")
            assert np.abs(o["rew"][:B].numpy() - rew).max() <= 1e-12
            assert np.array_equal(o["done"][:B].numpy().astype(bool), done) and np.array_equal(o["reason"][:B].numpy(), reason)
            assert np.array_equal(o["code"].numpy(), code) and np.array_equal(o["steps"].numpy(), steps)
            assert np.array_equal(o["nvo"].numpy(), c["nv"]) and int(o["err"][0]) == int((c["tstat"] != 0).any())
            assert (o["rew"][B:] == GUARD_F).all() and (o["done"][B:] == GUARD_B).all() and (o["reason"][B:] == GUARD_I).all()
            seen |= int(np.bitwise_or.reduce(reason))
    assert B < 8 or (seen & 32 and seen & 29 == 29)


@pytest.mark.parametrize("B,S", [(1, 5), (129, 1), (130, 5)])
@pytest.mark.parametrize("lift", [None, (0.5, 1e-3, 0.05)])
def test_null_quality_is_env_result_forces_and_neutral_parameters_are_null(lib_built, B, S, lift):
    for auto_reset in (0, 1):
        c = ref.random_case(60 + B + S + auto_reset, B, S, T=1e-3, F=0.05, special=4 if B < 8 else None)
        quality = ref.quality_columns(B, B)
        quality[-1] = 0.3, 4.0          # (a finite quality everywhere)
        plain = _result(c, lift, auto_reset, entry="forces")
        null = _result(c, lift, auto_reset, None, None, (7.0, 3.0, -9.0))           # (the three numbers are not read)
        neutral = _result(c, lift, auto_reset, quality, 0.45, (0.0, 0.0, INF))
        assert plain["rc"] == null["rc"] == neutral["rc"] == 0
        for k in ("rew", "done", "reason", "code", "steps", "nvo", "err"):
            assert torch.equal(plain[k], null[k]) and torch.equal(plain[k], neutral[k]), k
        on = _result(c, lift, auto_reset, quality, 0.45, (1.0, 0.0, INF))          # ... and a weight alone changes rewards only
        ok = plain["code"] == 0
        assert torch.equal(on["done"], plain["done"]) and torch.equal(on["reason"], plain["reason"])
        assert not ok.any() or not torch.equal(on["rew"][:B][ok], plain["rew"][:B][ok])


BAD_QUALITY = [("only_quality", None), ("only_quality_ref", None), ("wq", -0.5), ("wq", INF), ("wq", math.nan), ("Qm", -0.1),
               ("Qm", 1.0), ("Qm", math.nan), ("mc", 0.0), ("mc", -2.0), ("mc", math.nan)]


def _finish(c, r, o, code_o, steps_o, x, t, NP, quality, q_ref, qpar, lift=None, src=None, xinit=None, auto_reset=0):
    """`mdq_env_finish` on case `c` with the row arrays `r` (no hand-over), built as tests/test_env_finish_gpu.py builds it; with
    `src` (per-airfoil cached rows) the environments that end are reset in place."""
    from meshdqn_amd import _lib
    B, N, S, NV, A = c["B"], c["N"], c["S"], c["NV"], c["A"]
    d = _lib.EnvFinishDesc()
    d.B, d.N, d.S, d.NV, d.NP = B, N, S, NV, NP
    d.nv0, d.timesteps, d.auto_reset = int(c["nv0"][0]), PAR["timesteps"], int(auto_reset)
    d.threshold, d.time_reward, d.goal_vertices, d.negative_reward = (PAR["threshold"], PAR["time_reward"], PAR["goal_vertices"],
                                                                      PAR["negative_reward"])
    d.new_drags, d.gt_drag, d.nv, d.rstat = t["drags"].data_ptr(), t["gt"].data_ptr(), r["nv"].data_ptr(), t["rstat"].data_ptr()
    d.topo_status, d.nsel, d.code_in, d.code_out = t["tstat"].data_ptr(), r["nsel"].data_ptr(), t["code"].data_ptr(), code_o.data_ptr()
    d.steps_in, d.steps_out = t["steps"].data_ptr(), steps_o.data_ptr()
    d.reward, d.done, d.err_flag, d.nv_out = o["rew"].data_ptr(), o["done"].data_ptr(), o["err"].data_ptr(), o["nvo"].data_ptr()
    d.coords, d.u, d.p, d.n_closest, d.x = r["coords"].data_ptr(), r["u"].data_ptr(), r["p"].data_ptr(), r["ncl"].data_ptr(), x.data_ptr()
    d.reason = o["reason"].data_ptr()
    if lift is not None:
        d.new_lifts, d.gt_lift = t["lifts"].data_ptr(), t["gl"].data_ptr()
        d.lift_weight, d.lift_threshold, d.lift_floor = lift
    d.quality, d.quality_ref = _ptr(quality), _ptr(q_ref)
    d.quality_weight, d.min_quality, d.max_cot = qpar
    if A > 1:
        d.src_of_env, d.nv0_of = t["airfoil"].data_ptr(), t["nv0"].data_ptr()
    n = 0
    if src is not None:
        for k in r:
            d.dst[n], d.src[n] = r[k].data_ptr(), src[k].data_ptr()
            d.row_bytes[n] = d.src_stride[n] = r[k][0].numel() * r[k].element_size()
            n += 1
        d.x_init = xinit.data_ptr()
    d.n_rows = n
    keep = torch.zeros(B, dtype=i32, device="cuda")
    d.arrive = keep.data_ptr()
    return d, keep


def _finish_arrays(c, seed, NP):
    B, N, S, NV, A = c["B"], c["N"], c["S"], c["NV"], c["A"]
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *sh: torch.rand(sh, dtype=f64, generator=g)                     # noqa: E731
    ri = lambda hi, *sh: torch.randint(0, hi, sh, generator=g, dtype=i32)         # noqa: E731
    rows = dict(u=rnd(B, S, NP, 2), p=rnd(B, S, NV), coords=rnd(B, NV, 2), nv=torch.from_numpy(c["nv"].copy()), ncl=ri(NV, B, N),
                nsel=torch.from_numpy(c["nsel"].copy()))
    src = dict(u=rnd(A, S, NP, 2), p=rnd(A, S, NV), coords=rnd(A, NV, 2), nv=torch.from_numpy(c["nv0"].copy()), ncl=ri(NV, A, N),
               nsel=torch.full((A,), N, dtype=i32))
    xinit = torch.rand((A, N, 2 + 3 * S), generator=g)
    t = dict(drags=_dev(c["drags"]), gt=_dev(c["gt_drag"]), lifts=_dev(c["lifts"]), gl=_dev(c["gt_lift"]), rstat=_dev(c["rstat"]),
             tstat=_dev(c["tstat"]), code=_dev(c["code"]), steps=_dev(c["steps"]), airfoil=_dev(c["airfoil"]), nv0=_dev(c["nv0"]))
    return rows, src, xinit, t


@pytest.mark.parametrize("what,value", BAD_QUALITY)
def test_quality_arguments_are_refused_before_any_launch(lib_built, what, value):
    """Both entry points: non-zero, a message with the entry point's name and the argument's, no output written."""
    from meshdqn_amd import _lib
    lib = _lib.load()
    B, N, S, NV, NP = 9, 7, 2, 33, 101
    par = dict(wq=1.0, Qm=0.3, mc=4.0)
    if what in par:
        par[what] = value
    word = dict(only_quality="go together", only_quality_ref="go together", wq="quality_weight", Qm="min_quality", mc="max_cot")[what]
    c = ref.random_case(5, B, S, N=N, NV=NV)
    quality = ref.quality_columns(5, B)
    only = dict(only_quality="quality", only_quality_ref="quality_ref").get(what)
    o = _result(c, None, 1, quality, 0.45, (par["wq"], par["Qm"], par["mc"]), only=only)
    assert o["rc"] != 0 and b"mdq_env_result_quality" in o["msg"] and word.encode() in o["msg"]
    assert (o["rew"] == GUARD_F).all() and (o["done"] == GUARD_B).all() and (o["reason"] == GUARD_I).all() and (o["nvo"] == GUARD_I).all()
    assert int(o["err"][0]) == 0 and np.array_equal(o["code"].numpy(), c["code"]) and np.array_equal(o["steps"].numpy(), c["steps"])
    rows, _, _, t = _finish_arrays(c, 5, NP)
    r = {k: v.clone().cuda() for k, v in rows.items()}
    o = _outputs(B)
    steps_o, code_o = torch.full((B,), GUARD_I, dtype=i32, device="cuda"), torch.full((B,), GUARD_I, dtype=i32, device="cuda")
    x = torch.full((B, N, 2 + 3 * S), -5.0, dtype=torch.float32, device="cuda")
    tq, tr = _dev(quality), _dev(np.array([0.45]))
    d, keep = _finish(c, r, o, code_o, steps_o, x, t, NP, None if only == "quality_ref" else tq, None if only == "quality" else tr,
                      (par["wq"], par["Qm"], par["mc"]))
    rc = lib.mdq_env_finish(C.byref(d), _lib.stream_ptr())
    assert rc != 0 and b"mdq_env_finish" in lib.mdq_last_error() and word.encode() in lib.mdq_last_error()
    torch.cuda.synchronize()
    assert (o["rew"] == GUARD_F).all() and (o["done"] == GUARD_B).all() and (o["reason"] == GUARD_I).all()
    assert (o["nvo"] == GUARD_I).all() and int(o["err"][0]) == 0 and (steps_o == GUARD_I).all() and (code_o == GUARD_I).all()
    assert (x == -5.0).all()
    # ... and the same descriptor is accepted once the argument is put right (max_cot = +inf, no angle stop, included)
    d.quality, d.quality_ref = tq.data_ptr(), tr.data_ptr()
    d.quality_weight, d.min_quality, d.max_cot = 1.0, 0.0, INF
    _lib.check(lib.mdq_env_finish(C.byref(d), _lib.stream_ptr()), "mdq_env_finish")
    torch.cuda.synchronize()
    assert not (o["reason"][:B] & 32).any() and torch.equal(o["done"][:B] != 0, o["reason"][:B] != 0)


@pytest.mark.parametrize("shape", [(9, 7, 2, 33, 101), (37, 24, 5, 96, 300)])
@pytest.mark.parametrize("lift", [None, (0.5, 1e-3, 0.05)])
def test_env_finish_takes_the_reference_quality_of_the_environments_airfoil(lib_built, shape, lift):
    """Two airfoils (`src_of_env`): quality_ref [A] is read at the environment's airfoil - the two values differ by 0.15, which
    moves the rewards by O(0.1) - and a stop on the quality alone resets its environment in place like any other."""
    from meshdqn_amd import _lib
    lib = _lib.load()
    B, N, S, NV, NP = shape
    A = 2
    qpar, q_refs = (1.0, 0.3, ref.max_cot(12.0)), np.array([0.45, 0.3])
    c = ref.random_case(17 * B, B, S, N=N, NV=NV, T=1e-3, F=0.05, A=A)
    quality = ref.quality_columns(B, B, Qm=qpar[1], mc=qpar[2])
    rows, src, xinit, t = _finish_arrays(c, B, NP)
    r = {k: v.clone().cuda().contiguous() for k, v in rows.items()}
    s_ = {k: v.clone().cuda().contiguous() for k, v in src.items()}
    o = _outputs(B)
    steps_o, code_o = torch.full((B,), GUARD_I, dtype=i32, device="cuda"), torch.full((B,), GUARD_I, dtype=i32, device="cuda")
    x = torch.zeros((B, N, 2 + 3 * S), dtype=torch.float32, device="cuda")
    tq, tr, xi = _dev(quality), _dev(q_refs), xinit.cuda()
    d, keep = _finish(c, r, o, code_o, steps_o, x, t, NP, tq, tr, qpar, lift=lift, src=s_, xinit=xi, auto_reset=1)
    _lib.check(lib.mdq_env_finish(C.byref(d), _lib.stream_ptr()), "mdq_env_finish")
    torch.cuda.synchronize()
    assert int(keep.abs().sum()) == 0
    a = c["airfoil"]
    code = ref.final_codes(c["code"], c["rstat"], c["tstat"], c["nsel"], c["N"])
    rew, done, reason, st = ref.batch(c["drags"], c["gt_drag"][a], c["nv"], c["nv0"][a], code, c["steps"], PAR,
                                      *((None, None, None) if lift is None else (c["lifts"], c["gt_lift"][a], lift)),
                                      quality, q_refs[a], qpar)
    got = o["rew"][:B].cpu().numpy()
    print(f"shape {shape} lift {lift}: largest reward error {np.abs(got - rew).max():.3e}")
    assert np.abs(got - rew).max() <= 1e-12
    assert np.array_equal(o["done"][:B].cpu().numpy().astype(bool), done) and np.array_equal(o["reason"][:B].cpu().numpy(), reason)
    assert np.array_equal(code_o.cpu().numpy(), code) and np.array_equal(steps_o.cpu().numpy(), np.where(done, 0, st).astype(np.int32))
    assert (o["rew"][B:] == GUARD_F).all() and (o["reason"][B:] == GUARD_I).all()
    # with airfoil 0's value for everybody the rewards of airfoil 1's code-0 environments would be off by far more than 1e-12
    wrong = ref.batch(c["drags"], c["gt_drag"][a], c["nv"], c["nv0"][a], code, c["steps"], PAR,
                      *((None, None, None) if lift is None else (c["lifts"], c["gt_lift"][a], lift)), quality, q_refs[0], qpar)[0]
    sel = (a == 1) & (code == 0) & (quality[:, 0] < 0.45)
    assert sel.any() and np.abs(wrong - rew)[sel].min() > 1e-6
    # stops on the quality alone: reset in place from the rows of their own airfoil, features from the cached ones
    alone = np.flatnonzero(reason == 32)
    assert B < 37 or ((reason & 32).any() and (reason == 0).any())      # (the nine environments are mostly failed steps)
    for e in alone:
        for k in rows:
            assert torch.equal(r[k][e].cpu(), src[k][a[e]]), (e, k)
        assert torch.equal(x[e].cpu(), xinit[a[e]])
    for e in np.flatnonzero(reason == 0):
        for k in rows:
            assert torch.equal(r[k][e].cpu(), rows[k][e]), (e, k)


# ---------------------------------------------------------------------------------------------------------- 5: end to end
STEPS = 6


@pytest.fixture(scope="module")
def stock(lib_built, tmp_path_factory):
    """ys930 at the stock values on the oracle's ground truth (the snapshot-reload branch), as tests/test_lift_reward_gpu.py
    builds it: one base environment, the scripted heads of the four stock episodes, and a cache of the runs below."""
    from meshdqn_amd.env import Env2DAirfoil
    tmp = tmp_path_factory.mktemp("quality")
    ep = json.load(open(os.path.join(GOLDEN, "oracle_stock_ys930.json")))
    z = np.load(os.path.join(GOLDEN, "oracle_stock_ys930.npz"))
    snap = os.path.join(str(tmp), "snapshots")
    os.makedirs(snap, exist_ok=True)
    u, p = z["u"], z["p"]
    n2 = u.shape[1] // 2
    np.save(os.path.join(snap, "save_velocities.npy"), np.stack([u[:, :n2], u[:, n2:]], axis=2).reshape(len(u), -1))
    np.save(os.path.join(snap, "save_pressures.npy"), p)
    ap = dict(ep["agent_params"])
    ap.update(gt_drag=z["gt_drag"].copy(), gt_lift=z["gt_lift"].copy(), gt_time=np.array([5.0]), plot_dir=str(tmp))

    def cfg(**agent):
        return dict(flow_config=dict(flow_params=dict(mu=1e-3, rho=1.0, inflow="constant"),
                                     geometry_params=dict(mesh=os.path.join(GOLDEN, "ys930.npz")),
                                     solver_params=dict(dt=0.001, solver_type="lu", smooth=True)), agent_params=dict(ap, **agent))
    acts = np.full((STEPS, 4), 180, np.int64)
    for b, n in enumerate(["random_1370", "random_1371", "random_1372", "far_field"]):
        s = ep["episodes"][n]["steps"][:STEPS]
        acts[:len(s), b] = [g["action"] for g in s]
    return dict(cfg=cfg, acts=acts, base=Env2DAirfoil(cfg()), runs={})


def _host_run(stock, **agent):
    """STEPS scripted `step()` calls; per step: rewards, dones, reasons, codes, node features, the kernel's quality (where on) and
    the reference quality of the meshes read back (NaN rows for environments the step reset: their meshes are gone)."""
    from meshdqn_amd.vec_env import VecEnv2DAirfoil
    key = ("host", tuple(sorted(agent.items())))
    if key in stock["runs"]:
        return stock["runs"][key]
    acts = stock["acts"]
    K, B = acts.shape
    env = VecEnv2DAirfoil(stock["cfg"](**agent), B, base_env=stock["base"], nthreads=2)
    x0 = env.get_state()["x"].cpu().numpy()
    hs = dict(env=env, x0=x0, rewards=np.zeros((K, B)), dones=np.zeros((K, B), bool), reasons=np.zeros((K, B), np.int32),
              codes=np.zeros((K, B), np.int32), x=[], q_min=np.full((K, B), np.nan), cells=np.full((K, B), -1),
              ref=np.full((K, B, 2), np.nan), ref_cell=np.full((K, B), -1), angle=np.full((K, B), np.nan))
    for k in range(K):
        state, rew, done, info = env.step(acts[k])
        hs["rewards"][k], hs["dones"][k], hs["reasons"][k], hs["codes"][k] = rew, done, info["reason"], info["code"]
        hs["x"].append(state["x"].cpu().numpy())
        if env.quality.on:
            hs["q_min"][k], hs["cells"][k], hs["angle"][k] = info["q_min"], info["quality_cell"], info["min_angle"]
        else:
            assert "q_min" not in info and "min_angle" not in info and "quality_cell" not in info
        for b in np.flatnonzero(~done):
            m = ref.mesh(env.coords[b], env.cells[b], env.nv[b], env.nt[b])
            hs["ref"][k, b], hs["ref_cell"][k, b] = m[:2], m[2]
    stock["runs"][key] = hs
    return hs


def _device_run(stock, **agent):
    from meshdqn_amd.vec_env import VecEnv2DAirfoil
    acts = stock["acts"]
    K, B = acts.shape
    env = VecEnv2DAirfoil(stock["cfg"](**agent), B, base_env=stock["base"], nthreads=2)
    env.get_state()
    out = env.rollout_device(None, K, actions=acts)
    return env, out


def test_step_and_device_rollout_agree_and_report_the_reference_quality(stock):
    """`step()` evaluates reward.py on the host, `rollout_device` the kernel, on the same device quality; both report what the
    loop reference computes on the meshes read back, bit for bit."""
    keys = dict(quality_weight=0.5, min_quality=0.05)
    hs = _host_run(stock, **keys)
    env, out = _device_run(stock, **keys)
    assert env.quality.on and env.q_ref.shape == (1,) and 0.0 < env.q_ref[0] < 1.0
    print("reasons", out["reasons"].tolist(), "\nq_min", out["quality"][:, :, 0].tolist())
    print("|reward(step) - reward(rollout)| max", np.abs(hs["rewards"] - out["rewards"]).max())
    assert np.array_equal(out["codes"], hs["codes"]) and (hs["codes"] == 0).sum() >= 3 * STEPS
    assert np.abs(hs["rewards"] - out["rewards"]).max() <= 1e-12
    assert np.array_equal(hs["dones"], out["dones"]) and np.array_equal(hs["reasons"], out["reasons"])
    assert np.array_equal(out["dones"], out["reasons"] != 0) and not (out["reasons"] & 32).any()
    # the kernel's q_min of every step: step() and rollout alike, and the reference on the meshes read back
    assert out["quality"].shape == (STEPS, 4, 2)
    assert np.array_equal(_bits(out["quality"][:, :, 0]), _bits(hs["q_min"]))
    assert np.array_equal(_bits(np.degrees(np.arctan2(1.0, out["quality"][:, :, 1]))), _bits(hs["angle"]))
    live = ~hs["dones"]
    assert live.sum() >= 3 * STEPS
    assert np.array_equal(_bits(hs["q_min"][live]), _bits(hs["ref"][:, :, 0][live]))
    assert np.array_equal(_bits(out["quality"][live]), _bits(hs["ref"][live]))
    assert np.array_equal(hs["cells"][live], hs["ref_cell"][live])
    want_angle = np.degrees(np.arctan2(1.0, hs["ref"][:, :, 1][live]))
    assert np.array_equal(_bits(hs["angle"][live]), _bits(want_angle))
    # q_ref is the reference's q_min of the initial mesh, and the last step's meshes after the rollout give the last row
    x0, t0 = env._x0s[0], env._cells0s[0]
    assert _bits(env.q_ref)[0] == _bits([ref.mesh(x0, t0, env.nv0s[0], env.nt0s[0])[0]])[0]
    for b in np.flatnonzero(~out["dones"][-1]):
        m = ref.mesh(env.coords[b], env.cells[b], env.nv[b], env.nt[b])
        assert np.array_equal(_bits(out["quality"][-1, b]), _bits(m[:2])) and np.array_equal(_bits(env.mesh_quality[b]), _bits(m[:2]))
    # the weight moved the rewards of the code-0 steps against a run with the weight at zero
    hs0 = _host_run(stock, quality_weight=0.0, min_quality=0.0, min_angle=0.0)
    ok = (hs["codes"] == 0) & (hs0["codes"] == 0)
    assert np.abs(hs["rewards"] - hs0["rewards"])[ok].max() > 1e-6


def test_off_and_neutral_runs_agree_bit_for_bit(stock):
    off = _host_run(stock)
    neutral = _host_run(stock, quality_weight=0.0, min_quality=0.0, min_angle=0.0)
    assert not off["env"].quality.on and neutral["env"].quality.on and np.isnan(off["q_min"]).all()
    assert off["rewards"].tobytes() == neutral["rewards"].tobytes()
    assert np.array_equal(off["dones"], neutral["dones"]) and np.array_equal(off["reasons"], neutral["reasons"])
    assert np.array_equal(off["x0"], neutral["x0"]) and all(np.array_equal(a, b) for a, b in zip(off["x"], neutral["x"]))
    _, d_off = _device_run(stock)
    _, d_neu = _device_run(stock, quality_weight=0.0, min_quality=0.0, min_angle=0.0)
    assert "quality" not in d_off and d_neu["quality"].shape == (STEPS, 4, 2)
    for k in ("rewards", "dones", "reasons", "codes", "actions", "nv"):
        assert d_off[k].tobytes() == d_neu[k].tobytes(), k


def test_the_smallest_angle_stops_exactly_one_environment_at_the_chosen_step(stock):
    """A first run (weight 0, no stop) records the reference's cot_max of every step; `min_angle` is then set halfway, in cot,
    between two consecutive steps of one environment whose cot_max crosses there for the first time - that environment ends at
    exactly that step with reason 32, is reset in place and shows the initial features; the others go on."""
    first = _host_run(stock, quality_weight=0.0, min_quality=0.0, min_angle=0.0)
    cot, K, B = first["ref"][:, :, 1], STEPS, 4
    cot0 = ref.mesh(first["env"]._x0s[0], first["env"]._cells0s[0], first["env"].nv0s[0], first["env"].nt0s[0])[1]
    print("reference cot_max per step and environment:\n", cot, "\ninitial", cot0, "\nreasons", first["reasons"].tolist())
    pick = None
    for k in range(1, K):
        for b in range(B):
            if first["dones"][:k + 1].any() or np.isnan(cot[:k + 1]).any():
                continue
            mid = 0.5 * (cot[k - 1, b] + cot[k, b])
            others = np.delete(cot[:k + 1], b, axis=1)
            if cot[k, b] > mid > cot[k - 1, b] and (cot[:k, b] < mid).all() and (others < mid).all() and mid - cot[k - 1, b] > 1e-9 * mid:
                pick = pick or (k, b, mid)
    assert pick is not None, "no environment's cot_max rises above every earlier value of the batch within the scripted steps"
    k, b, mid = pick
    angle = math.degrees(math.atan2(1.0, mid))
    assert cot[k - 1, b] < ref.max_cot(angle) < cot[k, b]
    keys = dict(quality_weight=0.0, min_angle=angle)
    hs = _host_run(stock, **keys)
    env, out = _device_run(stock, **keys)
    for name, reasons, dones in (("step()", hs["reasons"], hs["dones"]), ("rollout_device", out["reasons"], out["dones"])):
        print(name, "stop at step", k, "environment", b, "min_angle", angle, "reasons", reasons.tolist())
        assert reasons[k, b] == 32 and dones[k, b] and not dones[:k].any()
        assert not np.delete(dones[:k + 1], b, axis=1).any() and not (np.delete(reasons, b, axis=1)[:k + 1] & 32).any()
    assert np.array_equal(hs["reasons"], out["reasons"]) and np.array_equal(hs["dones"], out["dones"])
    assert np.abs(hs["rewards"] - out["rewards"]).max() <= 1e-12
    # weight 0: the stop changes no reward up to and including its step
    assert hs["rewards"][:k + 1].tobytes() == first["rewards"][:k + 1].tobytes()
    # reset in place: the initial features in its rows, the others' rows as in the first run
    assert np.array_equal(hs["x"][k][b], hs["x0"][b]) and not np.array_equal(first["x"][k][b], first["x0"][b])
    others = [e for e in range(B) if e != b]
    assert np.array_equal(hs["x"][k][others], first["x"][k][others])
    assert hs["env"].steps[b] <= STEPS - 1 - k and env.steps[b] == hs["env"].steps[b]       # (its counter restarted at the stop)


def test_single_environment_and_deploy_report_and_stop_on_the_quality(stock):
    """`Env2DAirfoil`: the same kernel with B = 1 on its light mesh batch - `q_ref`, `mesh_quality`, `quality_cell` and the rows of
    `deploy()["est_quality"]` are the loop reference's bits on the environment's meshes, and `min_angle` set halfway (in cot, from
    the reference's numbers) in front of the first step whose cot_max exceeds everything before it ends the episode exactly there,
    with bit 32 in `end_reason`."""
    from meshdqn_amd.deploy import deploy
    from meshdqn_amd.env import Env2DAirfoil
    acts = [int(a) for a in stock["acts"][:4, 0]]

    def current(e):
        c, t = np.asarray(e.flow_solver.mesh.coordinates()), np.asarray(e.flow_solver.mesh.cells())
        return ref.mesh(c, t, len(c), len(t))

    def row(m):
        return [m[0], np.degrees(np.arctan2(1.0, m[1]))]

    env = Env2DAirfoil(stock["cfg"](quality_weight=0.5))
    m0 = current(env)
    assert env.quality.on and _bits(env.q_ref) == _bits(m0[0]) and np.array_equal(_bits(env.mesh_quality), _bits(m0[:2]))
    out = deploy(env, actions=acts, complete_traj=False, final_sim=False, stop_on_done=False)
    rows, m = out["est_quality"], current(env)
    print("est_quality", rows.tolist())
    assert rows.shape == (len(acts) + 1, 2) and np.array_equal(_bits(rows[0]), _bits(row(m0))) and np.array_equal(_bits(rows[-1]), _bits(row(m)))
    assert np.array_equal(_bits(env.mesh_quality), _bits(m[:2])) and env.quality_cell == m[2] and not env.end_reason & 32
    # without the keys deploy() reports the same rows (the metric does not depend on the reward's switches)
    off = Env2DAirfoil(stock["cfg"]())
    assert not off.quality.on and off.q_ref is None
    off.get_state()
    seq = [current(off)[1]]
    for a in acts:
        off.step(a)
        assert off.end_reason == 0 and off.mesh_quality is None
        seq.append(current(off)[1])
    assert np.array_equal(_bits(np.degrees(np.arctan2(1.0, np.array(seq)))), _bits(rows[:, 1]))
    k = next((j for j in range(1, len(seq)) if seq[j] > max(seq[:j])), None)
    assert k is not None, f"cot_max never rises above its earlier values in {seq}"
    mid = 0.5 * (max(seq[:k]) + seq[k])
    angle = math.degrees(math.atan2(1.0, mid))
    assert max(seq[:k]) < ref.max_cot(angle) < seq[k]
    stop = Env2DAirfoil(stock["cfg"](min_angle=angle))
    stop.get_state()
    for j, a in enumerate(acts[:k], 1):
        _, _, terminal, _ = stop.step(a)
        print(f"step {j}: terminal {terminal} end_reason {stop.end_reason} smallest angle {row(current(stop))[1]:.4f} (min_angle {angle:.4f})")
        assert terminal == (j == k) and stop.end_reason == (32 if j == k else 0)


@pytest.mark.parametrize("engine", [dict(gpu_topology=False), dict(gpu_smoothing=False)])
def test_the_host_topology_engine_feeds_the_same_launch(stock, engine):
    """The uploaded host arrays instead of the device engine's (host re-triangulation with the smoothing on the GPU, and
    everything on the host): the one launch reports the loop reference's bits on the environment's meshes there too."""
    from meshdqn_amd.vec_env import VecEnv2DAirfoil
    acts = stock["acts"]
    env = VecEnv2DAirfoil(stock["cfg"](quality_weight=0.5, min_quality=0.05), 4, base_env=stock["base"], nthreads=2, **engine)
    assert env.quality.on and not env.gpu_topology
    env.get_state()
    m0 = ref.mesh(env._x0s[0], env._cells0s[0], env.nv0s[0], env.nt0s[0])
    assert _bits(env.q_ref)[0] == _bits([m0[0]])[0] and np.array_equal(_bits(env.mesh_quality), _bits([m0[:2]] * 4))
    for k in range(2):
        _, rew, done, info = env.step(acts[k])
        assert not (info["reason"] & 32).any() and (info["code"] == 0).sum() >= 3
        for b in np.flatnonzero(~done):
            m = ref.mesh(env.coords[b], env.cells[b], env.nv[b], env.nt[b])
            assert _bits(info["q_min"])[b] == _bits([m[0]])[0] and info["quality_cell"][b] == m[2]
            assert _bits(info["min_angle"])[b] == _bits(np.degrees(np.arctan2(1.0, [m[1]])))[0]
