"""Host-only companion of tests/test_gpu_dense_reach.py: what the replay of the dense-tail plan's per-tile-pair reach
(tests/dense_reach.py) gives on the problems the GPU cases use.  A change of the ordering or of the tail's block pattern that
takes the empty items away from P20 fails here, instead of quietly leaving the zero-slab path of the kernels untested."""
import pytest

from tests import dense_reach as DR
from tests import factor_shapes as FS


@pytest.mark.parametrize("pid,items,want", [
    ("P20", 128, dict(all=1121, kept=1112, empty=9)),
    ("P20", 64, dict(all=1121, kept=1112, empty=9)),
    ("P10", 128, dict(all=86, kept=86, empty=0)),
    ("R128", 128, dict(all=5530, kept=5530, empty=0)),
])
def test_replayed_reach(pid, items, want):
    from scilmm_amd.factor import Symbolic
    p = FS.problem(pid)
    sym = Symbolic(p["mats"], upload=False, **p["opts"])
    got = DR.replay(sym, items)
    print(pid, items, got)
    assert {k: got[k] for k in want} == want
    assert got["kept"] <= got["all"] and got["early"] + got["late"] > 0
