"""CPU: the mesh-quality part of the host reward / terminal formula (`meshdqn_amd/reward.py`: QualitySpec, REASON_QUALITY)
against the plain-loop restatement `tests/quality_ref.py`, against today's call (bit for bit when off or neutral), and the
restated metric itself on the ys930 fixture (the first two rows of the table in HISTORY "Mesh quality").

Tolerance of the rewards: 1e-12, as tests/test_lift_reward_gpu.py argues it - the values are O(1) and the only operations
that are not correctly rounded are one `log`, two `exp` and two `sqrt`, each within a few ulp (2.2e-16); the quality part
adds one division, one product and two sums, all correctly rounded.  Flags and reasons exactly (the generators keep every
quantity 1e-9, relative, away from its threshold)."""
import math
import os

import numpy as np
import pytest

import lift_reward_ref as lref
import quality_ref as ref
from meshdqn_amd import reward
from meshdqn_amd.reward import LiftSpec, QualitySpec

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PAR = ref.PAR


def _call(spec, c, lifts, qspec=None, quality=None, q_ref=None):
    a = c["airfoil"]
    code = ref.final_codes(c["code"], c["rstat"], c["tstat"], c["nsel"], c["N"])
    kw = {} if qspec is None else dict(qspec=qspec, quality=quality, q_ref=q_ref)
    return reward.rewards(spec, c["gt_drag"][a], c["drags"], c["nv"], c["nv0"][a], code, c["steps"] + 1, PAR["threshold"],
                          PAR["time_reward"], PAR["goal_vertices"], PAR["timesteps"], PAR["negative_reward"],
                          c["gt_lift"][a] if lifts else None, c["lifts"] if lifts else None, **kw), code


# ---------------------------------------------------------------------------------------------------------- the spec
def test_quality_spec_from_config():
    assert not QualitySpec.from_config(dict(threshold=1e-3)).on and not reward.QUALITY_OFF.on
    s = QualitySpec.from_config(dict(quality_weight=0.5))
    assert s.on and (s.weight, s.min_quality, s.min_angle, s.max_cot) == (0.5, 0.0, 0.0, math.inf)
    s = QualitySpec.from_config(dict(min_quality=0.3))
    assert s.on and (s.weight, s.min_quality, s.min_angle, s.max_cot) == (0.0, 0.3, 0.0, math.inf)
    s = QualitySpec.from_config(dict(min_angle=12))
    assert s.on and (s.weight, s.min_quality, s.min_angle) == (0.0, 0.0, 12.0)
    assert s.max_cot == 1.0 / math.tan(math.radians(12.0)) == ref.max_cot(12.0)      # the ONE double of formula and kernel
    s = QualitySpec.from_config(dict(quality_weight=2, min_quality=0.25, min_angle=10.5))
    assert s.on and (s.weight, s.min_quality, s.min_angle) == (2.0, 0.25, 10.5)
    s = QualitySpec.from_config(dict(quality_weight=0.0, min_quality=0.0, min_angle=0.0))
    assert s.on and s.max_cot == math.inf                                           # on, but neutral
    assert reward.REASON_QUALITY == 32


@pytest.mark.parametrize("key,value", [("quality_weight", -0.1), ("quality_weight", math.inf), ("quality_weight", math.nan),
                                       ("quality_weight", "1"), ("quality_weight", True), ("min_quality", -0.1),
                                       ("min_quality", 1.0), ("min_quality", math.nan), ("min_quality", None),
                                       ("min_angle", -1.0), ("min_angle", 60.0), ("min_angle", math.nan), ("min_angle", [12])])
def test_bad_values_are_refused_with_the_keys_name(key, value):
    with pytest.raises(ValueError, match=key):
        QualitySpec.from_config({"threshold": 1e-3, key: value})


def test_a_degenerate_initial_mesh_is_refused_with_the_airfoils_name():
    on = QualitySpec(True, 1.0, 0.0, 0.0)
    on.check_q_ref(np.array([0.4, 0.3]), names=["a.npz", "b.npz"])
    with pytest.raises(ValueError, match="b.npz"):
        on.check_q_ref(np.array([0.4, 0.0]), names=["a.npz", "b.npz"])
    with pytest.raises(ValueError, match="a.npz"):
        on.check_q_ref(np.array([math.nan, 0.2]), names=["a.npz", "b.npz"])
    reward.QUALITY_OFF.check_q_ref(np.array([0.0]))         # nothing is asked of it while the spec is off


def test_the_keys_are_batch_wide_not_per_airfoil():
    from meshdqn_amd.vec_env import check_airfoil_configs
    mk = lambda mesh, **k: dict(flow_config=dict(geometry_params=dict(mesh=mesh)), agent_params=dict(threshold=1e-3, **k))  # noqa: E731
    check_airfoil_configs([mk("a", min_angle=12.0), mk("b", min_angle=12.0)])
    for key, v0, v1 in (("min_angle", 12.0, 13.0), ("quality_weight", 0.5, 1.0), ("min_quality", 0.2, 0.3)):
        with pytest.raises(ValueError, match=key):
            check_airfoil_configs([mk("a", **{key: v0}), mk("b", **{key: v1})])
        with pytest.raises(ValueError, match=key):
            check_airfoil_configs([mk("a", **{key: v0}), mk("b")])


def test_train_flags_reach_every_config():
    import train
    args = train.parser().parse_args(["--config", "a.yaml", "--min-angle", "12", "--quality-weight", "0.5"])
    cfgs = [dict(agent_params=dict(min_angle=3.0)), dict(agent_params={})]
    train.quality_options(args, cfgs)
    for c in cfgs:
        assert c["agent_params"] == dict(min_angle=12.0, quality_weight=0.5)
    args = train.parser().parse_args(["--config", "a.yaml", "--min-quality", "0.3"])
    cfgs = [dict(agent_params=dict(min_angle=3.0))]
    train.quality_options(args, cfgs)
    assert cfgs[0]["agent_params"] == dict(min_angle=3.0, min_quality=0.3)


# ---------------------------------------------------------------------------------------------------------- the formula
def test_the_restatement_is_the_lift_restatement_while_the_quality_is_off():
    for seed, lift in ((1, None), (2, (0.5, 1e-3, 0.05))):
        c = ref.random_case(seed, 37, 5, T=1e-3, F=0.05)
        code = ref.final_codes(c["code"], c["rstat"], c["tstat"], c["nsel"], c["N"])
        args = (c["drags"], c["gt_drag"][0], c["nv"], c["nv0"][0], code, c["steps"], PAR)
        tail = (None, None, None) if lift is None else (c["lifts"], c["gt_lift"][0], lift)
        a, b = lref.batch(*args, *tail), ref.batch(*args, *tail)
        assert a[0].tobytes() == b[0].tobytes() and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("lift", [None, (0.5, 1e-3, 0.05)])
@pytest.mark.parametrize("wq,Qm,ang", [(1.0, 0.3, 12.0), (0.25, 0.0, 14.0), (0.0, 0.3, 0.0), (3.0, 0.0, 0.0)])
def test_rewards_against_the_loop_reference(S, lift, wq, Qm, ang):
    qspec = QualitySpec(True, wq, Qm, ang)
    spec = reward.OFF if lift is None else LiftSpec(True, *lift)
    seen = 0
    for seed, (B, A) in enumerate([(1, 1), (37, 1), (64, 2)]):
        c = ref.random_case(300 + seed, B, S, T=1e-3, F=0.05, A=A)
        a = c["airfoil"]
        q_ref = np.array([0.45, 0.4])[:A][a]
        quality = ref.quality_columns(seed, B, Qm=Qm if Qm else 0.3, mc=qspec.max_cot)
        (rew, done, reason), code = _call(spec, c, lift is not None, qspec, quality, q_ref)
        r0, d0, q0, _ = ref.batch(c["drags"], c["gt_drag"][a], c["nv"], c["nv0"][a], code, c["steps"], PAR,
                                  *((None, None, None) if lift is None else (c["lifts"], c["gt_lift"][a], lift)),
                                  quality, q_ref, (wq, Qm, qspec.max_cot))
        print(f"S={S} lift={lift} B={B}: largest reward error {np.abs(rew - r0).max():.3e}")
        assert np.abs(rew - r0).max() <= 1e-12
        assert np.array_equal(done, d0) and np.array_equal(reason, q0) and reason.dtype == np.int32
        assert np.array_equal(done, reason != 0)
        seen |= int(np.bitwise_or.reduce(reason))
        if B >= 8:
            stop = Qm > 0.0 or ang > 0.0
            assert (reason == 0).any() and bool((reason & 32).any()) == stop
            if stop:    # quality stops on code-0 steps only, the worst mesh among them (a stop on the quality ALONE: next test)
                assert not (reason[code != 0] & 32).any() and (code[B - 1] != 0 or reason[B - 1] & 32)
    assert seen & 32 == (32 if (Qm > 0.0 or ang > 0.0) else 0) and seen & 29 == 29


@pytest.mark.parametrize("S", [1, 5])
def test_off_and_neutral_give_the_bits_of_todays_call(S):
    neutral = QualitySpec.from_config(dict(quality_weight=0.0, min_quality=0.0, min_angle=0.0))
    for seed, (B, A) in enumerate([(1, 1), (37, 1), (64, 2)]):
        c = ref.random_case(400 + seed, B, S, T=1e-3, F=0.05, A=A)
        quality = ref.quality_columns(seed, B)
        quality[-1] = 0.3, 4.0          # (a finite quality everywhere)
        q_ref = np.array([0.45, 0.4])[:A][c["airfoil"]]
        for spec, lifts in ((reward.OFF, False), (LiftSpec(True, 0.5, 1e-3, 0.05), True)):
            (r0, d0, s0), _ = _call(spec, c, lifts)                                              # today's call
            (r1, d1, s1), _ = _call(spec, c, lifts, reward.QUALITY_OFF, None, None)              # off
            (r2, d2, s2), _ = _call(spec, c, lifts, neutral, quality, q_ref)                     # on but neutral
            assert r0.tobytes() == r1.tobytes() == r2.tobytes()
            assert np.array_equal(d0, d1) and np.array_equal(d0, d2) and np.array_equal(s0, s1) and np.array_equal(s0, s2)
    # the single environment's form keeps its three values while the quality is off, and gains the fourth when on
    g, d = c["gt_drag"][0], c["drags"][0]
    assert len(reward.accuracy_terms(reward.OFF, g, d, PAR["threshold"])) == 3
    v0 = reward.accuracy_terms(reward.OFF, g, d, PAR["threshold"])[0]
    v, acc, accl, accq = reward.accuracy_terms(reward.OFF, g, d, PAR["threshold"], qspec=neutral, quality=np.array([0.3, 4.0]),
                                               q_ref=0.45)
    assert np.float64(v).tobytes() == np.float64(v0).tobytes() and not accq and not accl


def test_the_stop_is_strict_at_the_threshold_and_takes_one_ulp():
    c = ref.random_case(11, 3, 5)
    for e in range(3):                  # three plain code-0 steps well inside the drag threshold
        c["drags"][e] = c["gt_drag"][0] * (1.0 + 1e-4)
        c["code"][e] = c["rstat"][e] = c["tstat"][e] = 0
        c["nsel"][e], c["nv"][e], c["steps"][e] = c["N"], c["NV"], 2
    Qm, ang = 0.3, 12.0
    qspec = QualitySpec(True, 1.0, Qm, ang)
    mc = qspec.max_cot
    quality = np.array([[Qm, mc], [np.nextafter(Qm, 0.0), mc], [Qm, np.nextafter(mc, math.inf)]])
    (rew, done, reason), _ = _call(reward.OFF, c, False, qspec, quality, 0.45)
    assert reason.tolist() == [0, 32, 32] and done.tolist() == [False, True, True]
    # a ratio above 1 is capped: a mesh better than the initial one earns the full quality reward, 1, and no more
    (r_hi, _, _), _ = _call(reward.OFF, c, False, qspec, np.array([[0.9, 1.0]] * 3), 0.45)
    (r_eq, _, _), _ = _call(reward.OFF, c, False, qspec, np.array([[0.45, 1.0]] * 3), 0.45)
    assert r_hi.tobytes() == r_eq.tobytes()
    # the worst mesh (0, +inf) stops under either criterion, but not under neutral parameters
    worst = np.array([[0.0, math.inf]] * 3)
    assert (_call(reward.OFF, c, False, QualitySpec(True, 0.0, 0.0, ang), worst, 0.45)[0][2] == 32).all()
    assert (_call(reward.OFF, c, False, QualitySpec(True, 0.0, Qm, 0.0), worst, 0.45)[0][2] == 32).all()
    assert (_call(reward.OFF, c, False, QualitySpec(True, 0.0, 0.0, 0.0), worst, 0.45)[0][2] == 0).all()


# ---------------------------------------------------------------------------------------------------------- the metric
def test_the_restated_metric_on_hand_built_cells():
    h = math.sqrt(3.0) / 2.0
    q, cot = ref.cell((0.0, 0.0), (1.0, 0.0), (0.5, h))
    assert abs(q - 1.0) < 4e-16 and abs(cot - 1.0 / math.sqrt(3.0)) < 4e-16            # equilateral: q = 1, 60 degrees
    q, cot = ref.cell((0.0, 0.0), (1.0, 0.0), (0.0, 1.0))
    assert abs(q - ref.K / 4.0) < 4e-16 and cot == 1.0                                   # right isosceles: 45 degrees
    assert ref.cell((0.0, 0.0), (1.0, 1.0), (2.0, 2.0)) == (0.0, math.inf)              # collinear
    assert ref.cell((1.0, 2.0), (1.0, 2.0), (1.0, 2.0)) == (0.0, math.inf)              # s = 0
    assert ref.cell((0.0, 0.0), (math.nan, 0.0), (0.0, 1.0)) == (0.0, math.inf)         # not finite: the worst cell
    assert ref.cell((0.0, 0.0), (1e200, 0.0), (0.0, 1e200)) == (0.0, math.inf)          # overflow: the worst cell
    assert ref.mesh(np.zeros((3, 2)), np.zeros((2, 3), np.int32), 3, 0) == (0.0, math.inf, -1, -1, 0)
    # order independence, ties to the lowest index, ids outside [0, nv) never loaded
    rng = np.random.default_rng(0)
    P = rng.random((40, 2))
    P[30:] = [[0.0, 0.0], [1.0, 0.0], [0.5, h]] * 3 + [[0.0, 0.0]]                       # would be perfect cells if read
    cells = np.array([rng.choice(30, 3, replace=False) for _ in range(200)], np.int32)
    cells[50] = cells[150] = cells[7]
    base = ref.mesh(P, cells, 30, 200, 0.2)
    perm = rng.permutation(200)
    got = ref.mesh(P, cells[perm], 30, 200, 0.2)
    assert got[:2] == base[:2] and got[4] == base[4] and 0 < base[4] < 200
    assert perm[got[2]] in np.flatnonzero((cells == cells[base[2]]).all(axis=1)) and base[2] == min(
        np.flatnonzero((cells == cells[base[2]]).all(axis=1)))
    cells[120] = 30, 31, 32
    assert ref.mesh(P, cells, 30, 200)[:4] == (0.0, math.inf, 120, 120)
    assert ref.mesh(P, cells, 33, 200)[:2] == base[:2] or ref.mesh(P, cells, 33, 200)[0] <= base[0]
    cells[120] = 3, -1, 5
    assert ref.mesh(P, cells, 30, 200)[:4] == (0.0, math.inf, 120, 120)


def test_the_table_rows_on_the_ys930_fixture():
    """The fixture as committed and its initial state after smooth(50) (oracle/mesh.py): the first two rows of the table in
    HISTORY "Mesh quality", to the printed digits (the rows after 8 and 44 removals need 40 s of Delaunay: recorded there)."""
    from oracle.mesh import OracleMesh
    z = np.load(os.path.join(GOLDEN, "ys930.npz"))
    coords, cells = z["coords"], z["cells"]
    q, cot = ref.mesh(coords, cells, len(coords), len(cells))[:2]
    print(f"ys930 as committed: q_min {q:.6f}, smallest angle {ref.min_angle_deg(cot):.4f} deg")
    assert f"{q:.4f}" == "0.4922" and f"{ref.min_angle_deg(cot):.2f}" == "17.59"
    sm = OracleMesh(coords, cells).smooth(50)
    q, cot, cq, cc, n_low = ref.mesh(sm.coords, cells, len(coords), len(cells), 0.5)
    print(f"ys930 after smooth(50): q_min {q:.6f} (cell {cq}), smallest angle {ref.min_angle_deg(cot):.4f} deg (cell {cc}), "
          f"{n_low} cells below q = 0.5")
    assert f"{q:.4f}" == "0.4332" and f"{ref.min_angle_deg(cot):.2f}" == "15.10" and n_low >= 1
