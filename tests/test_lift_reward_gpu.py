"""GPU: the lift part of the env step's reward / accuracy stop and the `reason` output, through the C ABI on seeded random
data (`mdq_env_result_forces`, `mdq_env_finish` with the appended descriptor fields) against the plain-loop restatement
tests/lift_reward_ref.py - the kernels are not their own yardstick - and end to end through `VecEnv2DAirfoil`: `step()` (host
formula, meshdqn_amd/reward.py) against `rollout_device(actions=...)` (kernel).

Tolerances: rewards within 1e-12 - the values are O(1) and the only operations that are not correctly rounded are one
`log`, two `exp` and two `sqrt`, each within a few ulp (2.2e-16) on either side; everything else - done, code, steps, nv_out,
reason - exactly (the generator keeps every relative error 1e-9 away from its threshold)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import lift_reward_ref as ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PAR = ref.PAR
f64, i32, u8 = torch.float64, torch.int32, torch.uint8
GUARD_F, GUARD_I, GUARD_B = -777.25, -77777, 0xA5


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _outputs(B):
    """reward / done / reason with two guard words behind them, code / steps in-out, err, nv_out - filled with sentinels."""
    return dict(rew=torch.full((B + 2,), GUARD_F, dtype=f64, device="cuda"), done=torch.full((B + 8,), GUARD_B, dtype=u8, device="cuda"),
                reason=torch.full((B + 2,), GUARD_I, dtype=i32, device="cuda"), err=torch.zeros(1, dtype=i32, device="cuda"),
                nvo=torch.full((B,), GUARD_I, dtype=i32, device="cuda"))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _result(c, a, lift, auto_reset, entry="forces", lifts=True, reason=True):
    """One launch of mdq_env_result (entry "plain") or mdq_env_result_forces on case `c` with airfoil a's ground truth for
    every environment; returns the outputs on the host (guard words included)."""
    from meshdqn_amd import _lib
    lib = _lib.load()
    B, N, S = c["B"], c["N"], c["S"]
    o = _outputs(B)
    t = dict(drags=_dev(c["drags"]), gt=_dev(c["gt_drag"][a]), nv=_dev(c["nv"]), rstat=_dev(c["rstat"]), tstat=_dev(c["tstat"]),
             nsel=_dev(c["nsel"]), code=_dev(c["code"]), steps=_dev(c["steps"]), lifts=_dev(c["lifts"]), gl=_dev(c["gt_lift"][a]))
    head = (B, N, S, t["drags"].data_ptr(), t["gt"].data_ptr(), t["nv"].data_ptr(), int(c["nv0"][a]), t["rstat"].data_ptr(),
            t["tstat"].data_ptr(), t["nsel"].data_ptr(), t["code"].data_ptr(), t["steps"].data_ptr(), PAR["threshold"],
            PAR["time_reward"], PAR["goal_vertices"], PAR["timesteps"], PAR["negative_reward"], int(auto_reset), o["rew"].data_ptr(),
            o["done"].data_ptr(), o["err"].data_ptr(), o["nvo"].data_ptr())
    if entry == "plain":
        rc = lib.mdq_env_result(*head, _lib.stream_ptr())
    else:
        w, T, F = lift
        rc = lib.mdq_env_result_forces(*head, _ptr(t["lifts"] if lifts else None), _ptr(t["gl"] if lifts else None), w, T, F,
                                       _ptr(o["reason"] if reason else None), _lib.stream_ptr())
    msg = lib.mdq_last_error() if rc != 0 else b""
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in o.items()}
    out.update(code=t["code"].cpu(), steps=t["steps"].cpu(), rc=rc, msg=msg)
    return out


def _expect(c, a_of_env, lift, auto_reset, lifts=True):
    """The loop reference for case `c`: rewards, dones, reasons, final codes, steps_out."""
    code = ref.final_codes(c["code"], c["rstat"], c["tstat"], c["nsel"], c["N"])
    rew, done, reason, st = ref.batch(c["drags"], c["gt_drag"][a_of_env], c["nv"], c["nv0"][a_of_env], code, c["steps"], PAR,
                                      c["lifts"] if lifts else None, c["gt_lift"][a_of_env] if lifts else None,
                                      lift if lifts else None)
    steps = np.where(done & bool(auto_reset), 0, st).astype(np.int32)
    return rew, done, reason, code, steps


def _guards_untouched(o, B):
    assert (o["rew"][B:] == GUARD_F).all() and (o["done"][B:] == GUARD_B).all() and (o["reason"][B:] == GUARD_I).all()


@pytest.mark.parametrize("B", [1, 129, 130])
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("F", [0.0, 0.05])
def test_env_result_forces_against_the_loop_reference(lib_built, B, S, F):
    """B = 1, 129, 130: one block of the 128-thread kernel, and two with the second nearly empty.  F = 0.05 lies above the
    small ground-truth lifts of the generator (0.002 .. 0.022)."""
    lift = (0.5, 1e-3, F)
    seen, worst = 0, 0.0
    for auto_reset in (0, 1):
        for special in ([None] + list(range(6)) if B < 8 else [None]):
            c = ref.random_case(1000 * B + 10 * S + auto_reset, B, S, T=lift[1], F=F, special=special)
            assert F == 0.0 or S == 1 or ((np.abs(c["gt_lift"]) < F).any() and (np.abs(c["gt_lift"]) > F).any())
            o = _result(c, 0, lift, auto_reset)
            assert o["rc"] == 0
            rew, done, reason, code, steps = _expect(c, np.zeros(B, np.int64), lift, auto_reset)
            worst = max(worst, float(np.abs(o["rew"][:B].numpy() - rew).max()))
            print(f"B={B} S={S} F={F} auto_reset={auto_reset} special={special}: largest reward error so far {worst:.3e}")
            assert np.abs(o["rew"][:B].numpy() - rew).max() <= 1e-12
            assert np.array_equal(o["done"][:B].numpy().astype(bool), done) and np.array_equal(o["reason"][:B].numpy(), reason)
            assert np.array_equal(o["code"].numpy(), code) and np.array_equal(o["steps"].numpy(), steps)
            assert np.array_equal(o["nvo"].numpy(), c["nv"]) and int(o["err"][0]) == int((c["tstat"] != 0).any())
            _guards_untouched(o, B)
            seen |= int(np.bitwise_or.reduce(reason))
            if B >= 8:       # every code, a failing rstat, nsel < N, the step limit, both sides of both thresholds: in this batch
                assert set(c["code"]) == {0, 1, 2} and (c["rstat"] != 0).any() and (c["nsel"] < c["N"]).any()
                assert int(np.bitwise_or.reduce(reason)) == 31 and (reason == 0).any()
    assert seen & 24 == 24 and (B < 8 or seen == 31)        # (one environment: a failed step and the step limit at least)


@pytest.mark.parametrize("B,S", [(1, 5), (129, 1), (130, 5)])
def test_null_lifts_is_env_result_and_zero_weight_infinite_threshold_is_null(lib_built, B, S):
    for auto_reset in (0, 1):
        c = ref.random_case(50 + B + S + auto_reset, B, S, special=4 if B < 8 else None)
        plain = _result(c, 0, None, auto_reset, entry="plain")
        null = _result(c, 0, (7.0, 3.0, 9.0), auto_reset, lifts=False)        # (the three numbers are not read)
        noreason = _result(c, 0, (7.0, 3.0, 9.0), auto_reset, lifts=False, reason=False)
        zero = _result(c, 0, (0.0, math.inf, 0.0), auto_reset)
        assert plain["rc"] == null["rc"] == noreason["rc"] == zero["rc"] == 0
        for k in ("rew", "done", "code", "steps", "nvo", "err"):
            assert torch.equal(plain[k], null[k]) and torch.equal(plain[k], zero[k]) and torch.equal(plain[k], noreason[k]), k
        assert torch.equal(null["reason"], zero["reason"])
        assert (plain["reason"] == GUARD_I).all() and (noreason["reason"] == GUARD_I).all()      # (no reason array: none written)
        r = null["reason"][:B]
        assert torch.equal(null["done"][:B] != 0, r != 0) and not (r & 2).any()
        rew, done, reason, code, steps = _expect(c, np.zeros(B, np.int64), None, auto_reset, lifts=False)
        assert np.array_equal(r.numpy(), reason) and np.abs(null["rew"][:B].numpy() - rew).max() <= 1e-12
        on = _result(c, 0, (1.0, 1e-3, 0.0), auto_reset)
        assert torch.equal(on["done"][:B] != 0, on["reason"][:B] != 0)


# ---------------------------------------------------------------------------------------------------------- mdq_env_finish
def _finish_inputs(seed, B, N, S, NV, NP, A, lift):
    c = ref.random_case(seed, B, S, N=N, NV=NV, T=lift[1], F=lift[2], A=A)
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *sh: torch.rand(sh, dtype=f64, generator=g)                     # noqa: E731
    ri = lambda hi, *sh: torch.randint(0, hi, sh, generator=g, dtype=i32)         # noqa: E731
    Fx = 2 + 3 * S
    rows = dict(u=rnd(B, S, NP, 2), p=rnd(B, S, NV), coords=rnd(B, NV, 2), cells=ri(NV, B, 2 * NV, 3), misc=ri(99, B, 5),
                nv=torch.from_numpy(c["nv"].copy()), ncl=ri(NV, B, N), nsel=torch.from_numpy(c["nsel"].copy()))
    src = dict(u=rnd(A, S, NP, 2), p=rnd(A, S, NV), coords=rnd(A, NV, 2), cells=ri(NV, A, 2 * NV, 3), misc=ri(99, A, 5),
               nv=torch.from_numpy(c["nv0"].copy()), ncl=ri(NV, A, N), nsel=torch.full((A,), N, dtype=i32))
    return dict(c=c, rows=rows, src=src, extra=ri(99, B, 6, 7), xinit=torch.rand((A, N, Fx), generator=g), NP=NP)


def _finish_run(inp, fused, lift, auto_reset=True, with_handover=True, with_xinit=True, lifts=True):
    """`mdq_env_finish` (fused) or the launches it replaces: mdq_copy_strided (hand-over) -> mdq_env_result_forces (once per
    airfoil, every environment keeping its own airfoil's results) -> mdq_restore_rows_masked(_src) -> mdq_state_features."""
    from meshdqn_amd import _lib
    lib = _lib.load()
    sp = _lib.stream_ptr
    c, NP = inp["c"], inp["NP"]
    B, N, S, NV, A = c["B"], c["N"], c["S"], c["NV"], c["A"]
    Fx = 2 + 3 * S
    r = {k: v.clone().cuda().contiguous() for k, v in inp["rows"].items()}
    s_ = {k: v.clone().cuda().contiguous() for k, v in inp["src"].items()}
    ex, xinit = inp["extra"].cuda(), inp["xinit"].cuda()
    t = dict(drags=_dev(c["drags"]), gt=_dev(c["gt_drag"]), lifts=_dev(c["lifts"]), gl=_dev(c["gt_lift"]), rstat=_dev(c["rstat"]),
             tstat=_dev(c["tstat"]), code_in=_dev(c["code"]), steps_in=_dev(c["steps"]), airfoil=_dev(c["airfoil"]), nv0=_dev(c["nv0"]))
    o = _outputs(B)
    code_o, steps_o = torch.full((B,), GUARD_I, dtype=i32, device="cuda"), torch.full((B,), GUARD_I, dtype=i32, device="cuda")
    x = torch.zeros((B, N, Fx), dtype=torch.float32, device="cuda")
    ho = dict(coords=torch.zeros_like(r["coords"]), u_n=torch.zeros((B, NP, 2), dtype=f64, device="cuda"),
              p_n=torch.zeros((B, NV), dtype=f64, device="cuda"), nv=torch.zeros(B, dtype=i32, device="cuda"), extra=torch.zeros_like(ex))
    keys = list(r)
    per_u, per_p = NP * 2 * 8, NV * 8
    windows = [("coords", ho["coords"], 0, NV * 16), ("u", ho["u_n"], (S - 1) * per_u, per_u), ("p", ho["p_n"], (S - 1) * per_p, per_p),
               ("nv", ho["nv"], 0, 4)]
    row_bytes = {k: r[k][0].numel() * r[k].element_size() for k in keys}
    w, T, F = lift
    if not fused:
        if with_handover:
            n = len(windows) + 1
            dst = (C.c_void_p * n)(*[h.data_ptr() for _, h, _, _ in windows], ho["extra"].data_ptr())
            sr = (C.c_void_p * n)(*[r[k].data_ptr() + off for k, _, off, _ in windows], ex.data_ptr())
            nrows = (C.c_int64 * n)(*([B] * n))
            nb = (C.c_int64 * n)(*[b_ for _, _, _, b_ in windows], ex[0].numel() * 4)
            sst = (C.c_int64 * n)(*[row_bytes[k] for k, _, _, _ in windows], ex[0].numel() * 4)
            _lib.check(lib.mdq_copy_strided(n, dst, sr, nrows, nb, sst, nb, sp()), "mdq_copy_strided")
        per = []
        for a in range(A):
            oa = _outputs(B)
            ca, sa = t["code_in"].clone(), t["steps_in"].clone()
            _lib.check(lib.mdq_env_result_forces(
                B, N, S, t["drags"].data_ptr(), t["gt"][a].data_ptr(), r["nv"].data_ptr(), int(c["nv0"][a]), t["rstat"].data_ptr(),
                t["tstat"].data_ptr(), r["nsel"].data_ptr(), ca.data_ptr(), sa.data_ptr(), PAR["threshold"], PAR["time_reward"],
                PAR["goal_vertices"], PAR["timesteps"], PAR["negative_reward"], int(auto_reset), oa["rew"].data_ptr(),
                oa["done"].data_ptr(), o["err"].data_ptr(), oa["nvo"].data_ptr(), _ptr(t["lifts"] if lifts else None),
                _ptr(t["gl"][a] if lifts else None), w, T, F, oa["reason"].data_ptr(), sp()), "mdq_env_result_forces")
            per.append(dict(oa, code=ca, steps=sa))
        af = t["airfoil"].long()
        pick = lambda k, n_=B: torch.stack([p_[k][:n_] for p_ in per])[af, torch.arange(B, device="cuda")]      # noqa: E731
        for k in ("rew", "done", "reason"):
            o[k][:B] = pick(k)
        o["nvo"], code_o, steps_o = pick("nvo"), pick("code"), pick("steps")
        if auto_reset:
            n = len(keys)
            dst = (C.c_void_p * n)(*[r[k].data_ptr() for k in keys])
            sr = (C.c_void_p * n)(*[s_[k].data_ptr() for k in keys])
            nb = (C.c_int64 * n)(*[row_bytes[k] for k in keys])
            mask = o["done"][:B].contiguous()
            if A == 1:
                _lib.check(lib.mdq_restore_rows_masked(n, dst, sr, nb, B, mask.data_ptr(), sp()), "mdq_restore_rows_masked")
            else:
                _lib.check(lib.mdq_restore_rows_masked_src(n, dst, sr, nb, nb, B, mask.data_ptr(), t["airfoil"].data_ptr(), sp()),
                           "mdq_restore_rows_masked_src")
        _lib.check(lib.mdq_state_features(B, N, S, NV, NP, r["coords"].data_ptr(), r["u"].data_ptr(), r["p"].data_ptr(),
                                          r["ncl"].data_ptr(), r["nsel"].data_ptr(), x.data_ptr(), sp()), "mdq_state_features")
        if auto_reset and with_xinit:               # the fused launch shows the cached features for reset environments
            dn = o["done"][:B].bool()
            x[dn] = xinit[af[dn]]
    else:
        d = _lib.EnvFinishDesc()
        d.B, d.N, d.S, d.NV, d.NP = B, N, S, NV, NP
        d.nv0, d.timesteps, d.auto_reset = int(c["nv0"][0]), PAR["timesteps"], int(auto_reset)
        d.threshold, d.time_reward, d.goal_vertices, d.negative_reward = (PAR["threshold"], PAR["time_reward"], PAR["goal_vertices"],
                                                                          PAR["negative_reward"])
        d.new_drags, d.gt_drag, d.nv, d.rstat = t["drags"].data_ptr(), t["gt"].data_ptr(), r["nv"].data_ptr(), t["rstat"].data_ptr()
        d.topo_status, d.nsel, d.code_in, d.code_out = t["tstat"].data_ptr(), r["nsel"].data_ptr(), t["code_in"].data_ptr(), code_o.data_ptr()
        d.steps_in, d.steps_out = t["steps_in"].data_ptr(), steps_o.data_ptr()
        d.reward, d.done, d.err_flag, d.nv_out = o["rew"].data_ptr(), o["done"].data_ptr(), o["err"].data_ptr(), o["nvo"].data_ptr()
        if lifts:
            d.new_lifts, d.gt_lift = t["lifts"].data_ptr(), t["gl"].data_ptr()
        d.lift_weight, d.lift_threshold, d.lift_floor = w, T, F
        d.reason = o["reason"].data_ptr()
        if A > 1:
            d.src_of_env, d.nv0_of = t["airfoil"].data_ptr(), t["nv0"].data_ptr()
        n = len(keys)
        for i, k in enumerate(keys):
            d.dst[i], d.src[i] = r[k].data_ptr(), (s_[k].data_ptr() if auto_reset else None)
            d.row_bytes[i] = d.src_stride[i] = row_bytes[k]
        if with_handover:
            for k, dst, off, nb in windows:
                i = keys.index(k)
                d.handover_dst[i], d.handover_off[i], d.handover_bytes[i] = dst.data_ptr(), off, nb
            d.dst[n], d.src[n], d.row_bytes[n] = ex.data_ptr(), None, ex[0].numel() * 4
            d.handover_dst[n], d.handover_off[n], d.handover_bytes[n] = ho["extra"].data_ptr(), 0, ex[0].numel() * 4
            n += 1
        d.n_rows = n
        d.coords, d.u, d.p, d.n_closest = r["coords"].data_ptr(), r["u"].data_ptr(), r["p"].data_ptr(), r["ncl"].data_ptr()
        d.x_init = xinit.data_ptr() if with_xinit else None
        d.x = x.data_ptr()
        arrive = torch.zeros(B, dtype=i32, device="cuda")
        d.arrive = arrive.data_ptr()
        _lib.check(lib.mdq_env_finish(C.byref(d), sp()), "mdq_env_finish")
        assert int(arrive.abs().sum()) == 0           # the arrival counters are left at zero for the next launch
    torch.cuda.synchronize()
    return dict(rew=o["rew"].cpu(), done=o["done"].cpu(), reason=o["reason"].cpu(), err=o["err"].cpu(), nvo=o["nvo"].cpu(),
                code=code_o.cpu(), steps=steps_o.cpu(), x=x.cpu(), **{f"row_{k}": v.cpu() for k, v in r.items()},
                **{f"ho_{k}": v.cpu() for k, v in ho.items()})


# (B, N, S, NV, NP): the first resets 4.8 KiB per environment and hands 1.8 KiB over - one workgroup per environment; the
# second 35 KiB and 12 KiB - three workgroups per environment (one per 16 KiB), which meet at the arrival counter
FINISH_SHAPES = [(9, 7, 2, 33, 101), (37, 24, 5, 96, 300)]


@pytest.mark.parametrize("shape", FINISH_SHAPES)
@pytest.mark.parametrize("A", [1, 2])
@pytest.mark.parametrize("auto_reset", [True, False])
def test_env_finish_with_lifts_equals_the_launches_it_replaces(lib_built, shape, A, auto_reset):
    B, N, S, NV, NP = shape
    lift = (0.5, 1e-3, 0.05)
    inp = _finish_inputs(7 * B + A, B, N, S, NV, NP, A, lift)
    a = _finish_run(inp, False, lift, auto_reset=auto_reset)
    b = _finish_run(inp, True, lift, auto_reset=auto_reset)
    for k in a:
        assert torch.equal(a[k], b[k]), k          # bit for bit: rewards, flags, reasons, every restored / handed-over row
    _guards_untouched(b, B)
    c = inp["c"]
    rew, done, reason, code, steps = _expect(c, c["airfoil"], lift, auto_reset)
    assert np.abs(b["rew"][:B].numpy() - rew).max() <= 1e-12 and np.array_equal(b["reason"][:B].numpy(), reason)
    assert np.array_equal(b["done"][:B].numpy().astype(bool), done) and np.array_equal(b["steps"].numpy(), steps)
    assert np.array_equal(b["code"].numpy(), code)
    assert (reason == 2).any() and (reason == 0).any() and ((reason & 1).any() or B < 37)     # lift-only stops among them
    if auto_reset:                      # ... which reset their environment in place like any other stop
        for e in np.flatnonzero(reason == 2):
            for k in inp["rows"]:
                assert torch.equal(b[f"row_{k}"][e], inp["src"][k][c["airfoil"][e]]), (e, k)
            assert torch.equal(b["x"][e], inp["xinit"][c["airfoil"][e]])
    # the zero-initialised tail is the drag-only step (and still reports its reasons)
    z = _finish_run(inp, True, (0.0, 0.0, 0.0), auto_reset=auto_reset, lifts=False)
    rew0, done0, reason0, _, _ = _expect(c, c["airfoil"], None, auto_reset, lifts=False)
    assert np.array_equal(z["reason"][:B].numpy(), reason0) and np.array_equal(z["done"][:B].numpy().astype(bool), done0)
    assert np.abs(z["rew"][:B].numpy() - rew0).max() <= 1e-12


def test_lift_only_stop_resets_its_environment_and_leaves_its_neighbours(lib_built):
    B, N, S, NV, NP = FINISH_SHAPES[1]
    lift = (1.0, 1e-3, 0.0)
    inp = _finish_inputs(3, B, N, S, NV, NP, 1, lift)
    c = inp["c"]
    gd, gl = c["gt_drag"][0], c["gt_lift"][0]
    for e in (2, 3, 4):                 # three plain steps well inside both thresholds, far from the vertex goal and step limit
        c["drags"][e], c["lifts"][e] = gd * (1.0 + 1e-4), gl * (1.0 - 1e-4)
        c["code"][e] = c["rstat"][e] = c["tstat"][e] = 0
        c["nsel"][e], c["nv"][e], c["steps"][e] = N, NV, 3
        inp["rows"]["nv"][e], inp["rows"]["nsel"][e] = NV, N
    c["lifts"][3, S - 1] = gl[S - 1] * (1.0 + 1.5e-3)          # ... and one lift of environment 3 outside
    o = _finish_run(inp, True, lift, auto_reset=True)
    assert o["reason"][2:5].tolist() == [0, 2, 0] and o["done"][2:5].tolist() == [0, 1, 0]
    assert o["steps"][2:5].tolist() == [4, 0, 4] and o["code"][2:5].tolist() == [0, 0, 0]
    rew = _expect(c, c["airfoil"], lift, 1)[0]
    assert np.abs(o["rew"][:B].numpy() - rew).max() <= 1e-12 and rew[3] < rew[2] - 0.3
    for k in inp["rows"]:
        assert torch.equal(o[f"row_{k}"][3], inp["src"][k][0]), k                   # the cached initial rows
        for e in (2, 4):
            assert torch.equal(o[f"row_{k}"][e], inp["rows"][k][e]), (k, e)           # untouched
    assert torch.equal(o["x"][3], inp["xinit"][0])
    assert torch.equal(o["ho_coords"][3], inp["rows"]["coords"][3])                 # (handed over before the reset)
    plain = _finish_run(inp, True, lift, auto_reset=True, lifts=False)
    assert plain["reason"][2:5].tolist() == [0, 0, 0] and plain["steps"][3] == 4
    assert torch.equal(plain["x"][[2, 4]], o["x"][[2, 4]]) and not torch.equal(plain["x"][3], inp["xinit"][0])


BAD_LIFTS = [("only_new_lifts", None), ("only_gt_lift", None), ("w", -0.5), ("w", math.inf), ("w", math.nan), ("T", 0.0),
             ("T", -1e-3), ("T", math.nan), ("F", -1.0), ("F", math.inf), ("F", math.nan)]


@pytest.mark.parametrize("what,value", BAD_LIFTS)
def test_refusals_before_any_launch(lib_built, what, value):
    """Both entry points: non-zero, a message that names the argument, and no output written."""
    from meshdqn_amd import _lib
    lib = _lib.load()
    B, N, S, NV, NP = FINISH_SHAPES[0]
    lift = dict(w=1.0, T=1e-3, F=0.0)
    if what in lift:
        lift[what] = value
    word = dict(only_new_lifts="go together", only_gt_lift="go together", w="lift_weight", T="lift_threshold", F="lift_floor")[what]
    c = ref.random_case(5, B, S, N=N, NV=NV)
    o = _outputs(B)
    t = dict(drags=_dev(c["drags"]), gt=_dev(c["gt_drag"][0]), nv=_dev(c["nv"]), rstat=_dev(c["rstat"]), tstat=_dev(c["tstat"]),
             nsel=_dev(c["nsel"]), code=_dev(c["code"]), steps=_dev(c["steps"]), lifts=_dev(c["lifts"]), gl=_dev(c["gt_lift"][0]))
    nl = None if what == "only_gt_lift" else t["lifts"].data_ptr()
    gl = None if what == "only_new_lifts" else t["gl"].data_ptr()
    steps_o, code_o = torch.full((B,), GUARD_I, dtype=i32, device="cuda"), torch.full((B,), GUARD_I, dtype=i32, device="cuda")
    x = torch.full((B, N, 2 + 3 * S), -5.0, dtype=torch.float32, device="cuda")
    rc = lib.mdq_env_result_forces(B, N, S, t["drags"].data_ptr(), t["gt"].data_ptr(), t["nv"].data_ptr(), NV, t["rstat"].data_ptr(),
                                   t["tstat"].data_ptr(), t["nsel"].data_ptr(), t["code"].data_ptr(), t["steps"].data_ptr(),
                                   PAR["threshold"], PAR["time_reward"], PAR["goal_vertices"], PAR["timesteps"], PAR["negative_reward"],
                                   1, o["rew"].data_ptr(), o["done"].data_ptr(), o["err"].data_ptr(), o["nvo"].data_ptr(), nl, gl,
                                   lift["w"], lift["T"], lift["F"], o["reason"].data_ptr(), _lib.stream_ptr())
    assert rc != 0 and b"mdq_env_result_forces" in lib.mdq_last_error() and word.encode() in lib.mdq_last_error()
    inp = _finish_inputs(5, B, N, S, NV, NP, 1, (1.0, 1e-3, 0.0))
    r = {k: v.clone().cuda() for k, v in inp["rows"].items()}
    d = _lib.EnvFinishDesc()
    d.B, d.N, d.S, d.NV, d.NP, d.n_rows = B, N, S, NV, NP, 0
    d.nv0, d.timesteps, d.auto_reset = NV, PAR["timesteps"], 0
    d.threshold, d.time_reward, d.goal_vertices, d.negative_reward = 1e-3, 0.005, 0.95, -1.0
    d.new_drags, d.gt_drag, d.nv, d.rstat = t["drags"].data_ptr(), t["gt"].data_ptr(), r["nv"].data_ptr(), t["rstat"].data_ptr()
    d.topo_status, d.nsel, d.code_in, d.code_out = t["tstat"].data_ptr(), r["nsel"].data_ptr(), t["code"].data_ptr(), code_o.data_ptr()
    d.steps_in, d.steps_out = t["steps"].data_ptr(), steps_o.data_ptr()
    d.reward, d.done, d.err_flag, d.nv_out = o["rew"].data_ptr(), o["done"].data_ptr(), o["err"].data_ptr(), o["nvo"].data_ptr()
    d.coords, d.u, d.p, d.n_closest, d.x = r["coords"].data_ptr(), r["u"].data_ptr(), r["p"].data_ptr(), r["ncl"].data_ptr(), x.data_ptr()
    d.new_lifts, d.gt_lift, d.reason = nl, gl, o["reason"].data_ptr()
    d.lift_weight, d.lift_threshold, d.lift_floor = lift["w"], lift["T"], lift["F"]
    rc = lib.mdq_env_finish(C.byref(d), _lib.stream_ptr())
    assert rc != 0 and b"mdq_env_finish" in lib.mdq_last_error() and word.encode() in lib.mdq_last_error()
    torch.cuda.synchronize()
    assert (o["rew"] == GUARD_F).all() and (o["done"] == GUARD_B).all() and (o["reason"] == GUARD_I).all()
    assert (o["nvo"] == GUARD_I).all() and int(o["err"][0]) == 0 and (steps_o == GUARD_I).all() and (code_o == GUARD_I).all()
    assert (x == -5.0).all() and torch.equal(t["code"].cpu(), torch.from_numpy(c["code"])) and torch.equal(t["steps"].cpu(), torch.from_numpy(c["steps"]))
    # ... and the same descriptor is accepted once the argument is put right (T = +inf included)
    d.new_lifts, d.gt_lift = t["lifts"].data_ptr(), t["gl"].data_ptr()
    d.lift_weight, d.lift_threshold, d.lift_floor = 1.0, math.inf, 0.0
    _lib.check(lib.mdq_env_finish(C.byref(d), _lib.stream_ptr()), "mdq_env_finish")
    torch.cuda.synchronize()
    assert not (o["reason"][:B] & 2).any() and torch.equal(o["done"][:B] != 0, o["reason"][:B] != 0)


# ---------------------------------------------------------------------------------------------------------- end to end
def _snapshot_cfg(tmp, **agent):
    """ys930 at the stock values on the ORACLE's ground truth (the snapshot-reload branch), as tests/test_stock_gpu.py builds it."""
    ep = json.load(open(os.path.join(GOLDEN, "oracle_stock_ys930.json")))
    z = np.load(os.path.join(GOLDEN, "oracle_stock_ys930.npz"))
    snap = os.path.join(str(tmp), "snapshots")
    os.makedirs(snap, exist_ok=True)
    u, p = z["u"], z["p"]
    n2 = u.shape[1] // 2
    np.save(os.path.join(snap, "save_velocities.npy"), np.stack([u[:, :n2], u[:, n2:]], axis=2).reshape(len(u), -1))
    np.save(os.path.join(snap, "save_pressures.npy"), p)
    ap = dict(ep["agent_params"])
    ap.update(gt_drag=z["gt_drag"].copy(), gt_lift=z["gt_lift"].copy(), gt_time=np.array([5.0]), plot_dir=str(tmp), **agent)
    cfg = dict(flow_config=dict(flow_params=dict(mu=1e-3, rho=1.0, inflow="constant"),
                                geometry_params=dict(mesh=os.path.join(GOLDEN, "ys930.npz")),
                                solver_params=dict(dt=0.001, solver_type="lu", smooth=True)), agent_params=ap)
    names = ["random_1370", "random_1371", "random_1372", "far_field"]
    acts = np.full((5, 4), 180, np.int64)
    for b, n in enumerate(names):
        s = ep["episodes"][n]["steps"][:5]
        acts[:len(s), b] = [g["action"] for g in s]
    return cfg, acts


def _both_paths(cfg, acts):
    from meshdqn_amd.env import Env2DAirfoil
    from meshdqn_amd.vec_env import VecEnv2DAirfoil
    base = Env2DAirfoil(cfg)
    K, B = acts.shape
    host = VecEnv2DAirfoil(cfg, B, base_env=base, nthreads=2)
    host.get_state()
    hs = dict(rewards=np.zeros((K, B)), dones=np.zeros((K, B), bool), reasons=np.zeros((K, B), np.int32), drags=[], nv=[], codes=[])
    for k in range(K):
        _, rew, done, info = host.step(acts[k])
        hs["rewards"][k], hs["dones"][k], hs["reasons"][k] = rew, done, info["reason"]
        hs["drags"].append(info["new_drags"])
        hs["nv"].append(info["nv"])
        hs["codes"].append(info["code"].copy())
    dev = VecEnv2DAirfoil(cfg, B, base_env=base, nthreads=2)
    dev.get_state()
    out = dev.rollout_device(None, K, actions=acts)
    assert np.array_equal(out["codes"], np.array(hs["codes"]))
    return host, hs, out


def test_step_and_device_rollout_agree_with_and_without_the_keys(lib_built, tmp_path):
    """B = 4 on ys930, 5 scripted steps (the heads of the stock episodes): `step()` evaluates reward.py on the host,
    `rollout_device` the kernel, on the same device forces."""
    from meshdqn_amd import reward
    cfg, acts = _snapshot_cfg(tmp_path / "on", lift_weight=1.0, lift_threshold=1e-3, lift_floor=1e-3)
    host, hs, out = _both_paths(cfg, acts)
    assert host.lift.on and (host.lift.weight, host.lift.threshold, host.lift.floor) == (1.0, 1e-3, 1e-3)
    print("lift on:  |reward(step) - reward(rollout)| max", np.abs(hs["rewards"] - out["rewards"]).max(), "reasons", out["reasons"].tolist())
    assert np.abs(hs["rewards"] - out["rewards"]).max() <= 1e-12
    assert np.array_equal(hs["dones"], out["dones"]) and np.array_equal(hs["reasons"], out["reasons"])
    assert np.array_equal(out["dones"], out["reasons"] != 0) and (out["reasons"] & 2).any()
    cfg0, _ = _snapshot_cfg(tmp_path / "off")
    host0, hs0, out0 = _both_paths(cfg0, acts)
    assert not host0.lift.on
    print("lift off: |reward(step) - reward(rollout)| max", np.abs(hs0["rewards"] - out0["rewards"]).max(), "reasons", out0["reasons"].tolist())
    assert not (out0["reasons"] & 2).any() and not (hs0["reasons"] & 2).any()
    assert np.abs(hs0["rewards"] - out0["rewards"]).max() <= 1e-12
    assert np.array_equal(hs0["dones"], out0["dones"]) and np.array_equal(hs0["reasons"], out0["reasons"])
    # the drag-only path, bit for bit: the host rewards are today's numpy expressions on the step's drags ...
    gt, thr = host0.gt_drag, host0.threshold
    for k in range(len(acts)):
        d, nv = hs0["drags"][k], hs0["nv"][k]
        want = 2 * np.exp(-(-2 * np.log(0.5) / thr) * np.linalg.norm(np.abs(gt - d) / np.abs(gt), axis=1)) - 1 + (host0.NV - nv) * host0.TIME_REWARD
        ok = hs0["codes"][k] == 0
        assert ok.sum() >= 3 and hs0["rewards"][k][ok].tobytes() == want[ok].tobytes()
    # ... and where the lift is switched on, an episode whose drags are inside stops on it alone, with less reward for that
    # step than the drag alone gives it (both runs have followed the same meshes up to there)
    assert (out["reasons"] == reward.REASON_LIFT).any()
    b = int(np.flatnonzero((out["reasons"] == reward.REASON_LIFT).any(axis=0))[0])
    k = int(np.argmax(out["reasons"][:, b] == reward.REASON_LIFT))
    assert not out["dones"][:k, b].any() and not out0["dones"][:k + 1, b].any()
    assert out["rewards"][k, b] < out0["rewards"][k, b]
