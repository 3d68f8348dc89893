"""Host-only companions of tests/test_gpu_selected_inverse.py: the facts of the analysis its four problems rely on (a change
of the ordering or of the tail selection fails here instead of quietly emptying the GPU cases), and the dense reference's
own comparison on a factor assembled on the host."""
import numpy as np
import pytest
import scipy.sparse as sp

from scilmm_amd.factor import Symbolic
from tests import sinv_oracle as SO
from tests.helpers import random_spd


@pytest.mark.parametrize("pid", sorted(SO.PROBLEMS))
def test_the_problems_have_the_tails_the_gpu_cases_are_about(pid):
    p, want = SO.problem(pid), SO.PROBLEMS[pid][1]
    sym = Symbolic(p["mats"], upload=False, **p["opts"])
    info = sym.info()
    start = sym.get("sn_start").astype(np.int64)
    rowptr = sym.get("sn_rowptr").astype(np.int64)
    assert (info.n, info.nsuper, info.dense_first) == (want["n"], want["nsuper"], want["dense_first"])
    assert np.diff(start)[info.dense_first:].tolist() == want["tail"]
    # a tail front stores every later row (padded where the structure has none): what k_sinv_tail's arithmetic relies on
    for f in range(info.dense_first, info.nsuper):
        assert rowptr[f + 1] - rowptr[f] == info.n - start[f], f
    if pid == "P":
        # ... and the prelude reaches into it: some front below the tail has rows among the tail's columns
        rows = sym.get("sn_rows")
        assert any(rows[rowptr[f + 1] - 1] >= start[info.dense_first] for f in range(info.dense_first))


def _stored_csc(sym, M):
    """The entries of the dense M at every position `scilmm_export_L` reports, as CSC."""
    a = sym.arrays()
    start, rowptr, rows = a["sn_start"], a["sn_rowptr"], a["sn_rows"]
    indptr, idx = [0], []
    for s in range(len(start) - 1):
        rs = rows[rowptr[s]:rowptr[s + 1]]
        for j in range(start[s + 1] - start[s]):
            idx.append(rs[j:])
            indptr.append(indptr[-1] + rs.size - j)
    idx = np.concatenate(idx)
    cols = np.repeat(np.arange(M.shape[0]), np.diff(indptr))
    return sp.csc_matrix((M[idx, cols], idx, np.array(indptr)), shape=M.shape)


def test_the_dense_reference_compares_every_stored_position():
    A = random_spd(300, 0.03, 5)
    mats, s2 = [A, sp.identity(300, format="csr")], [0.6, 0.8]
    sym = Symbolic(mats, upload=False)
    start = sym.get("sn_start")
    layout = SO.export_layout(start, sym.get("sn_rowptr"), sym.info().nnzL_stored)
    ref = SO.DenseReference(mats, s2, sym.P())
    V = (s2[0] * A + s2[1] * mats[1]).toarray()
    assert np.abs(ref.traces() - [np.trace(np.linalg.solve(V, m.toarray())) for m in mats]).max() < 1e-11
    assert abs(ref.logdet() - np.linalg.slogdet(V)[1]) < 1e-10
    Z = _stored_csc(sym, ref.Zd)
    assert Z.nnz == layout[1] and len(start) > 3
    assert SO.compare_entries(Z, ref.Zd, layout) == 0.0
    # an entry that was cleared and never written is a stored 0.0: still compared
    offdiag = Z.indices != np.repeat(np.arange(300), np.diff(Z.indptr))
    e = int(np.argmax(np.abs(Z.data) * offdiag))
    bad = Z.copy()
    bad.data[e] = 0.0
    with pytest.raises(AssertionError, match="column front"):
        SO.compare_entries(bad, ref.Zd, layout)
    # a relative 1e-6 on one diagonal entry is over the limit (cond(V) < 1e2: the entry is within 1e-2 of its panel's
    # scale), 1e-12 is not
    d = int(Z.indptr[start[1]])
    for eps, ok in ((1e-6, False), (1e-12, True)):
        bad = Z.copy()
        bad.data[d] *= 1.0 + eps
        if ok:
            assert SO.compare_entries(bad, ref.Zd, layout) < SO.ENTRY_TOL
        else:
            with pytest.raises(AssertionError):
                SO.compare_entries(bad, ref.Zd, layout)
    # a shorter export is refused, not compared
    short = sp.csc_matrix(sp.tril(Z, -1))
    with pytest.raises(AssertionError):
        SO.compare_entries(short, ref.Zd, layout)
