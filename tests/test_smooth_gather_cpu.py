"""CPU: the width rule of the smoothing's block steps (tests/smooth_gather_cases.py restates it for the GPU tests) on the
lab meshes, and the meshes those tests build.

A block of 32 interior ranks is narrow if none of its rows has more than 8 gather slots - neighbours that are not
lower-numbered members of the same block.  ys930 and ah93w145 have narrow blocks only (widest row: 8 slots); ys930 after 20
and 42 scripted removals has one wide block, the hub's."""
import numpy as np

import smooth_gather_cases as sgc


def test_lab_meshes_have_narrow_blocks_only(meshes):
    for name, rows in (("ys930", 694), ("ah93w145", 634)):
        coords, cells = meshes[name]
        ns = sgc.row_slots(np.asarray(cells), len(coords))
        assert len(ns) == rows and ns.max() == 8, (name, len(ns), ns.max())
        assert sgc.wide_blocks(np.asarray(cells), len(coords)) == []


def test_scripted_removals_give_one_wide_block(meshes):
    for removals, blocks, widest in ((0, [], 8), (20, [13], 11), (42, [12], 13)):
        c, t = sgc.ys930_displaced(meshes, removals)
        assert sgc.wide_blocks(t, len(c)) == blocks and sgc.row_slots(t, len(c)).max() == widest, removals


def test_hub_strips_are_valid_and_wide_where_intended():
    for name, (r, a, b) in sgc.HUBS.items():
        c, t = sgc.strip_hub(r, a, b, 7 + r)            # (asserts a valid triangulation itself)
        ns = sgc.row_slots(t, len(c))
        assert ns[r] == sgc.HUB_SLOTS[name] and np.delete(ns, r).max() <= 6
        assert sgc.wide_blocks(t, len(c)) == sgc.HUB_WIDE[name]
    for n, (ny, nx) in sgc.RECT.items():
        c, t = sgc.rectangle(ny, nx, 40 + n)
        assert len(sgc.row_slots(t, len(c))) == n and sgc.wide_blocks(t, len(c)) == []
