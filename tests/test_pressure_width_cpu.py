"""CPU: the SELL-64 width class of every mesh of `test_pressure_width_gpu.py`, computed in numpy - from the cells alone and
from the slice offsets the device gets (`sl1_off`): the class decides which instance of the pressure CG an environment runs."""
import numpy as np
import pytest

from pressure_width_cases import CASES, case_mesh, width_class, widest_row


@pytest.mark.parametrize("name", sorted(CASES))
def test_width_class(meshes, lib_built, name):
    from meshdqn_amd.topology import MeshTopology
    _, _, cls, width = CASES[name]
    coords, cells, _ = case_mesh(meshes, name)
    assert widest_row(cells, len(coords)) == width
    topo = MeshTopology(coords, cells)
    rowptr1, colidx1 = topo.patterns()["p1"][:2]
    sl_off = topo.sell_layout(rowptr1, colidx1)[0]
    widths = np.diff(sl_off) // 64
    assert len(widths) == (len(coords) + 63) // 64 and widths.max() == width, widths
    assert width_class(int(widths.max())) == cls
    assert len(coords) <= 1024                  # two rows per thread of the 512-thread kernel: the register CG is reached


def test_the_classes_covered():
    assert {c[2] for c in CASES.values()} == {"<= 10", "11-12", "13-16"}        # "> 16": no script of <= 80 removals found
