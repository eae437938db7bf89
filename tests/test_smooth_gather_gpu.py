"""GPU: the block steps of `mdq_smooth_fast` at the block's width against the same launch with every block at full width.

`MDQ_SMOOTH_GATHER=7` (read once per process) makes every block step gather all 14 slots of its rows, the parent's arithmetic;
by default a block none of whose rows has more than 8 slots reads four per lane half.  Two fresh child processes, one per
setting, run every case of tests/smooth_gather_cases.py once; the cases below compare their files: coordinates bitwise equal,
diagnostics equal, and within 1e-13 of the careful walk `mdq_smooth` on the same input (the existing tests see 8.9e-16).

 - structured rectangles of 1 ... 97 interior vertices (1-4 blocks, every rotation position, narrow blocks only), 1 / 2 / 3 / 50 sweeps;
 - the strip of 97 interior vertices with one hub of 12 cells - in block 0, in block 1, in the last block, at ranks 31 and
   32 - so that exactly one block takes the wide step between narrow ones (checked on the host), and hubs of exactly 8 and 9
   gather slots, the two sides of the narrow / wide boundary;
 - ys930 after 0, 20 and 42 scripted removals with one vertex displaced, 50 sweeps: repair rounds between narrow sweeps."""
import os
import subprocess
import sys

import numpy as np
import pytest

import smooth_gather_cases as sgc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runs(lib_built, tmp_path_factory):
    """(default, MDQ_SMOOTH_GATHER=7): every case, each setting in a fresh process."""
    out = []
    for name, gather in (("default", None), ("gather7", "7")):
        path = str(tmp_path_factory.mktemp("smooth_gather") / f"{name}.npz")
        env = {k: v for k, v in os.environ.items() if k != "MDQ_SMOOTH_GATHER"}
        if gather:
            env["MDQ_SMOOTH_GATHER"] = gather
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [sgc.__file__, path]
        res = subprocess.run(cmd, env=env, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        out.append(dict(np.load(path)))
    return out


def _compare(runs, group, sweeps, names, moved_min):
    new, old = runs
    nv = new[f"{group}/nv"]
    for key in ("fast", "stats", "walk"):
        assert np.array_equal(new[f"{group}/{sweeps}/{key}"], old[f"{group}/{sweeps}/{key}"], equal_nan=False), (group, sweeps, key)
    fast, walk, st, start = new[f"{group}/{sweeps}/fast"], new[f"{group}/{sweeps}/walk"], new[f"{group}/{sweeps}/stats"], new[f"{group}/start"]
    for b, name in enumerate(names):
        err = np.abs(fast[b, :nv[b]] - walk[b, :nv[b]]).max()
        moved = np.abs(fast[b, :nv[b]] - start[b, :nv[b]]).max()
        print(f"{group} {name}, {sweeps} sweeps: against the walk {err:.2e} (moved {moved:.2e}); handed back / repaired sweeps / "
              f"repair rounds / sent back: {st[b]}")
        assert err < 1e-13, (group, name, sweeps, err)
        assert moved > moved_min, (group, name, sweeps)     # (the sweeps did something)
        assert st[b, 0] == 0, (group, name, st[b])           # in the blocked solve, nothing handed back
    return st


@pytest.mark.parametrize("sweeps", sgc.RECT_SWEEPS)
def test_rectangles_narrow_blocks_only(runs, sweeps):
    _compare(runs, "rect", sweeps, [str(n) for n in sgc.RECT], 1e-4)


def test_hub_meshes_have_one_wide_block():
    """On the host, by the set-up's rule: the hub's block is the only wide one, with the intended number of slots."""
    for name, (r, a, b) in sgc.HUBS.items():
        c, t = sgc.strip_hub(r, a, b, 7 + r)
        ns = sgc.row_slots(t, len(c))
        assert len(ns) == 97 and ns[r] == sgc.HUB_SLOTS[name] and np.delete(ns, r).max() <= 6, (name, ns[r])
        assert sgc.wide_blocks(t, len(c)) == sgc.HUB_WIDE[name], name
        assert (ns[r] > 8) == bool(sgc.HUB_WIDE[name]) and (not sgc.HUB_WIDE[name] or sgc.HUB_WIDE[name] == [r // 32])


@pytest.mark.parametrize("sweeps", sgc.HUB_SWEEPS)
def test_one_wide_block_between_narrow_ones(runs, sweeps):
    st = _compare(runs, "hub", sweeps, list(sgc.HUBS), 1e-5)
    if sweeps == 3:       # clear full steps: the block steps' results are the output.  (Under 50 sweeps the strip converges to
        assert (st[:, 1:] == 0).all(), st                    # round-off after about 11: later updates fall under DOLFIN_EPS and are repaired)


def test_ys930_repair_rounds_between_narrow_sweeps(runs):
    st = _compare(runs, "ys930", 50, [f"{k} removals" for k in sgc.YS_REMOVALS], 1e-4)
    assert (st[:, 2] >= 1).all(), st                         # the displaced vertex took repair rounds


@pytest.mark.parametrize("group", ["rect", "hub", "ys930"])
def test_env_entry_point_and_diagnostics(runs, group):
    """`mdq_smooth_fast_env` (the env step's entry point) gives what `mdq_smooth_fast` gives, in both settings; the words
    handed back, the repair rounds and the sent-back sweeps are equal in both runs of every case."""
    new, old = runs
    s = {"rect": sgc.RECT_SWEEPS[-1], "hub": sgc.HUB_SWEEPS[-1], "ys930": 50}[group]
    for r in (new, old):
        assert np.array_equal(r[f"{group}/{s}/env"], r[f"{group}/{s}/fast"])
        assert np.array_equal(r[f"{group}/{s}/envstats"], r[f"{group}/{s}/stats"])
    assert np.array_equal(new[f"{group}/{s}/env"], old[f"{group}/{s}/env"])
    assert np.array_equal(new[f"{group}/{s}/envstats"], old[f"{group}/{s}/envstats"])
