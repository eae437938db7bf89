"""GPU: the set-up of `mdq_smooth_fast` with only the dependent rows of a block inverse in the serial row loop (and the
neighbour lists deduplicated in registers) against the same launch on the parent's code paths, and the block inverses
against an fp64 restatement of their recurrence.

`MDQ_SMOOTH_SETUP_PARENT=3` (read once per process) selects the parent's paths.  Two fresh child processes, one per setting,
run every case of tests/smooth_inverse_cases.py once through both entry points and read the block-inverse workspace back
after every launch; the cases below compare their files: coordinates, diagnostics and workspace bitwise equal.

The workspace is also held to `reference_inverses` (numpy, fp64).  Every term of the recurrence is non-negative, so
nothing cancels; a row step rounds at most twice, and a chain of rows is at most 32 long: a relative bound of
64 x 2^-53 per entry, derived, not chosen.  Entries above the diagonal are exactly zero.

 - rectangles of 1, 31, 32, 33 and 65 interior vertices, 1 and 3 sweeps;
 - quads40: no row has an in-block lower neighbour (empty masks: the identity is all there is);
 - strip97: every row but a block's first has one (full masks);
 - wheel8: a hub row with MAXLOW = 8 in-block lower neighbours;
 - ys930 after 0 and 42 scripted removals, one vertex displaced."""
import os
import subprocess
import sys

import numpy as np
import pytest

import smooth_inverse_cases as sic

pytestmark = pytest.mark.gpu

BOUND = 64.0 * 2.0 ** -53


@pytest.fixture(scope="module")
def runs(lib_built, tmp_path_factory):
    """(default, MDQ_SMOOTH_SETUP_PARENT=3): every case, each setting in a fresh process."""
    out = []
    for name, parent in (("default", None), ("parent", "3")):
        path = str(tmp_path_factory.mktemp("smooth_inverse") / f"{name}.npz")
        env = {k: v for k, v in os.environ.items() if k != "MDQ_SMOOTH_SETUP_PARENT"}
        if parent:
            env["MDQ_SMOOTH_SETUP_PARENT"] = parent
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [sic.__file__, path]
        res = subprocess.run(cmd, env=env, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        out.append(dict(np.load(path)))
    return out


@pytest.fixture(scope="module")
def cases():
    return {"small": sic.small_cases(), "ys930": sic.ys_cases()}


GROUPS = [("small", s) for s in sic.SMALL_SWEEPS] + [("ys930", sic.YS_SWEEPS)]


@pytest.mark.parametrize("group,sweeps", GROUPS)
def test_bitwise_equal_to_the_parent_paths(runs, cases, group, sweeps):
    """Both entry points: coordinates, diagnostics and every written block of the workspace, bit for bit."""
    new, old = runs
    assert sorted(new) == sorted(old)
    keys = [k for k in new if k.startswith(f"{group}/{sweeps}/")]
    assert len(keys) == 2 * (2 + len(cases[group]))
    for k in keys:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape, k
        assert new[k].tobytes() == old[k].tobytes(), k
    for tag in ("fast", "env"):
        st = new[f"{group}/{sweeps}/{tag}/stats"]
        assert (st[:, 0] == 0).all(), (tag, st)              # every mesh in the blocked solve: its inverses were built
    for key in ("coords", "stats"):                          # the env step's entry point gives what mdq_smooth_fast gives
        assert np.array_equal(new[f"{group}/{sweeps}/env/{key}"], new[f"{group}/{sweeps}/fast/{key}"]), key
    for name, _, _ in cases[group]:
        assert new[f"{group}/{sweeps}/env/inv/{name}"].tobytes() == new[f"{group}/{sweeps}/fast/inv/{name}"].tobytes(), name


def test_the_sweeps_did_something(runs, cases):
    new, _ = runs
    for group, sweeps in GROUPS:
        out = new[f"{group}/{sweeps}/fast/coords"]
        for b, (name, c, _) in enumerate(cases[group]):
            assert np.abs(out[b, :len(c)] - c).max() > 1e-6, (group, name)


@pytest.mark.parametrize("group,sweeps", [("small", sic.SMALL_SWEEPS[-1]), ("ys930", sic.YS_SWEEPS)])
@pytest.mark.parametrize("setting", [0, 1])
def test_inverses_against_fp64_recurrence(runs, cases, group, sweeps, setting):
    run = runs[setting]
    for name, c, t in cases[group]:
        ref = sic.reference_inverses(t, len(c))
        for tag in ("fast", "env"):
            got = sic.unpack_workspace(run[f"{group}/{sweeps}/{tag}/inv/{name}"], len(ref))
            upper = np.triu(np.ones((sic.BS, sic.BS), bool), 1)[None]
            assert (got[np.broadcast_to(upper, got.shape)] == 0.0).all(), (name, tag)
            assert ((ref > 0) == (got > 0)).all(), (name, tag)
            rel = np.abs(got - ref)[ref > 0] / ref[ref > 0]
            low = sic.lower_counts(t, len(c))
            print(f"{name} {tag} ({'parent paths' if setting else 'default'}): {len(ref)} blocks, rows with lower neighbours "
                  f"{int((low > 0).sum())} of {len(low)} (most {int(low.max())}), largest relative deviation "
                  f"{rel.max():.2e} (bound {BOUND:.2e})")
            assert rel.max() <= BOUND, (name, tag, rel.max())


def test_masks_of_the_cases(cases):
    """On the host: the cases are what they are meant to be."""
    by = {name: sic.lower_counts(t, len(c)) for g in cases.values() for name, c, t in g}
    for n in sic.RECT:
        assert len(by[f"rect{n}"]) == n
    assert len(by["quads40"]) == 40 and (by["quads40"] == 0).all()                  # empty masks, two blocks
    s = by["strip97"]
    assert len(s) == 97 and (s[np.arange(97) % 32 != 0] == 1).all() and (s[::32] == 0).all()   # full masks
    assert by["wheel8"].max() == sic.MAXLOW and by["wheel8"][-1] == sic.MAXLOW
    assert all(len(by[f"ys930-{k}"]) > 600 for k in sic.YS_REMOVALS)
