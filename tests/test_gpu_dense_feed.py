"""k_dense_b's chunk boundary: the default loop (A fragments by hand-counted waits, descendant entries fetched ahead) against
the loop before it (SCILMM_TUNING=1 SCILMM_DENSE_FEED=0, read per factorization), on one deterministic handle per problem.

Both loops multiply the same operands and add the products in the same order, and a deterministic handle sums nothing with
atomics: `Factor.L()` has to come out bit for bit the same.  The problems (tests/factor_shapes.py) put the loop on its edges:
R37 a ragged single chunk per descendant and a 3-wide last front, R50 / R100 descendants of one chunk and of 64 + 36, R128
descendants of two full chunks and an 8-wide last front, P10 a padded pedigree tail under a prelude.  With 64 items per launch
an item runs over several descendants, so the descendant entries that are fetched ahead are used."""
import numpy as np
import pytest

from tests import factor_shapes as FS

pytestmark = pytest.mark.gpu

SWITCHES = ("SCILMM_TUNING", "SCILMM_DENSE", "SCILMM_DENSE_ITEMS", "SCILMM_DENSE_FEED", "SCILMM_DETERMINISTIC", "SCILMM_VERBOSE")


@pytest.mark.parametrize("items", [None, "64"], ids=["default-items", "items64"])
@pytest.mark.parametrize("pid", ["R37", "R50", "R100", "R128", "P10"])
def test_feed_loop_gives_the_bits_of_the_loop_before_it(pid, items, monkeypatch):
    from scilmm_amd.factor import Symbolic
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SCILMM_TUNING", "1")
    monkeypatch.setenv("SCILMM_DENSE", "1")
    if items:
        monkeypatch.setenv("SCILMM_DENSE_ITEMS", items)
    p = FS.problem(pid)
    sym = Symbolic(p["mats"], deterministic=True, **p["opts"])
    f = sym.factorize(p["sigma2"])
    L_new, ld_new = f.L(), f.logdet()
    sym.set_profiling(1)
    f.refactorize(p["sigma2"])
    launches = sym.timing()["n_dense_launches"]
    sym.set_profiling(0)
    assert launches > 0, "the dense-tail kernel did not run"
    assert np.array_equal(f.L().data, L_new.data), "the default loop does not repeat its own bits"
    monkeypatch.setenv("SCILMM_DENSE_FEED", "0")
    f.refactorize(p["sigma2"])
    L_old = f.L()
    assert np.array_equal(L_old.indptr, L_new.indptr) and np.array_equal(L_old.indices, L_new.indices)
    nbad = int(np.count_nonzero(L_old.data != L_new.data))
    print(pid, items, "entries", L_new.nnz, "with other bits", nbad, "dense launches", launches)
    assert nbad == 0 and np.isfinite(L_new.data).all()
    assert f.logdet() == ld_new
