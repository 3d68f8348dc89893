"""Deterministic mode, host side: the public switch (C ABI and Python), the transposed pattern index of k_spmm_row and the
pull schedule of k_fwd_pull.  No GPU needed."""
import ctypes as C

import numpy as np
import scipy.sparse as sp

from scilmm_amd import _lib
from scilmm_amd.SparseCholesky import SparseCholesky
from scilmm_amd.factor import Symbolic
from tests.helpers import small_pedigree


def _problem(n=2000):
    A, _ = small_pedigree(n, 0.01, 3)
    return A, sp.identity(A.shape[0], format="csr")


def test_switch_is_exposed_through_every_layer(monkeypatch):
    monkeypatch.delenv("SCILMM_DETERMINISTIC", raising=False)
    assert SparseCholesky(deterministic=True).deterministic is True
    assert SparseCholesky().deterministic is False
    A, I = _problem(600)
    assert Symbolic([A, I], upload=False, deterministic=True).deterministic is True
    assert Symbolic([A, I], upload=False).deterministic is False
    assert Symbolic([A, I], upload=False, deterministic=False).deterministic is False
    monkeypatch.setenv("SCILMM_DETERMINISTIC", "1")
    assert Symbolic([A, I], upload=False).deterministic is True       # the environment sets a new handle's default
    assert Symbolic([A, I], upload=False, deterministic=False).deterministic is False  # ... and the argument overrides it
    assert SparseCholesky().deterministic is True
    L = _lib.lib()
    assert L.scilmm_set_deterministic(None, 1) == _lib.ERR_ARG
    on = C.c_int32(7)
    assert L.scilmm_get_deterministic(None, C.byref(on)) == _lib.ERR_ARG
    fields = dict(_lib.Timing._fields_)
    assert "n_float_atomic_launches" in fields
    assert list(fields)[-1] == "n_float_atomic_launches"  # appended: the layout of the older fields is unchanged


def test_distributed_handle_refuses_the_mode_in_either_order(monkeypatch):
    monkeypatch.delenv("SCILMM_DETERMINISTIC", raising=False)
    A, I = _problem(600)
    L = _lib.lib()
    cb = _lib.COMM_FN(lambda *a: 0)
    stream = C.c_void_p(1)  # never dereferenced by scilmm_dist_init
    a = Symbolic([A, I], upload=False)
    assert L.scilmm_dist_init(a._h, 0, 2, stream, cb, None) == _lib.OK
    assert L.scilmm_set_deterministic(a._h, 1) == _lib.ERR_STATE
    assert b"all-reduce" in L.scilmm_symbolic_error(a._h)
    assert a.deterministic is False
    assert L.scilmm_set_deterministic(a._h, 0) == _lib.OK
    b = Symbolic([A, I], upload=False, deterministic=True)
    assert L.scilmm_dist_init(b._h, 0, 2, stream, cb, None) == _lib.ERR_STATE
    assert b"all-reduce" in L.scilmm_symbolic_error(b._h)
    assert L.scilmm_dist_init(b._h, 0, 1, None, None, None) == _lib.OK  # one rank is not distributed


def test_transposed_pattern_index_matches_scipy():
    A, I = _problem(2000)
    sym = Symbolic([A, I], upload=False)
    n = sym.n
    colptr, prow = sym.get("pat_colptr"), sym.get("pat_row")
    nnz = prow.size
    # the pattern as a CSC matrix whose data are the slot numbers (+ 1: scipy must not take slot 0 for an explicit zero)
    M = sp.csc_matrix((np.arange(1, nnz + 1, dtype=np.int64), prow, colptr), shape=(n, n))
    T = sp.tril(M, k=-1).tocsr()
    T.sort_indices()
    rowptr, rowslot, rowcol = sym.get("pat_rowptr"), sym.get("pat_rowslot"), sym.get("pat_rowcol")
    assert rowptr.dtype == np.int64 and rowslot.dtype == np.int64 and rowcol.dtype == np.int32
    assert rowptr.size == n + 1 and rowslot.size == rowcol.size == nnz - n
    assert np.array_equal(rowptr, T.indptr)
    assert np.array_equal(rowcol, T.indices)
    assert np.array_equal(rowslot, T.data - 1)
    for i in range(n):  # columns ascending inside every row
        assert np.all(np.diff(rowcol[rowptr[i]:rowptr[i + 1]]) > 0)
    # index memory of the mode, from the counts alone: 8 (n + 1) + 12 entries bytes
    assert 8 * rowptr.size + 8 * rowslot.size + 4 * rowcol.size == 8 * (n + 1) + 12 * (nnz - n)


def test_pull_schedule_consumes_every_update_pair_once_in_list_order():
    A, I = _problem(10000)  # (large enough for targets with more pairs than one segment takes)
    sym = Symbolic([A, I], upload=False)
    upd_ptr = sym.get("upd_ptr")
    nsuper, npairs = upd_ptr.size - 1, sym.get("upd_src").size
    seg_front, seg_ptr, seg_slot = sym.get("pull_seg_front"), sym.get("pull_seg_ptr"), sym.get("pull_seg_slot")
    front_seg = sym.get("pull_front_seg")
    nseg = seg_front.size
    assert seg_ptr.size == nseg + 1 and seg_slot.size == nseg and front_seg.size == nsuper + 1
    # the segments tile the pair list: every pair in exactly one segment, segments in list order
    assert seg_ptr[0] == 0 and seg_ptr[-1] == npairs and np.all(np.diff(seg_ptr) >= 0)
    covered = np.zeros(npairs, dtype=np.int64)
    for g in range(nseg):
        covered[seg_ptr[g]:seg_ptr[g + 1]] += 1
    assert np.all(covered == 1)
    # the segments of one target are consecutive, start where its pair list starts, end where it ends
    assert front_seg[0] == 0 and front_seg[-1] == nseg
    multi = 0
    for s in range(nsuper):
        g0, g1 = front_seg[s], front_seg[s + 1]
        assert g1 > g0  # (every front has a segment: L*R needs its diagonal block even without update pairs)
        assert np.all(seg_front[g0:g1] == s)
        assert seg_ptr[g0] == upd_ptr[s] and seg_ptr[g1] == upd_ptr[s + 1]
        if g1 - g0 == 1:
            assert seg_slot[g0] == -1
        else:
            multi += 1
            assert np.all(np.diff(seg_ptr[g0:g1 + 1]) > 0)
            assert np.array_equal(seg_slot[g0:g1], seg_slot[g0] + np.arange(g1 - g0))  # folded in slot = list order
    assert multi > 0  # the problem exercises the segmented form
    # per level: every segment of the level's fronts once; the fold triples name the multi-segment fronts and their slots.
    # Slots are numbered inside groups of consecutive levels: inside a group no two fronts share a slot.
    level_ptr, level_fronts = sym.get("level_ptr"), sym.get("level_fronts")
    plp, pls = sym.get("pull_level_ptr"), sym.get("pull_level_segs")
    pfp, pf = sym.get("pull_fold_ptr"), sym.get("pull_fold").reshape(-1, 3)
    grp = sym.get("pull_group_ptr")
    nlev = level_ptr.size - 1
    assert plp.size == nlev + 1 and pfp.size == nlev + 1
    assert grp[0] == 0 and grp[-1] == nlev and np.all(np.diff(grp) > 0)
    assert sorted(pls.tolist()) == list(range(nseg))
    for l in range(nlev):
        fronts = level_fronts[level_ptr[l]:level_ptr[l + 1]]
        segs = pls[plp[l]:plp[l + 1]]
        assert set(seg_front[segs].tolist()) == set(fronts.tolist())
        for s, slot0, ns in pf[pfp[l]:pfp[l + 1]]:
            assert s in fronts and ns == front_seg[s + 1] - front_seg[s] and ns > 1
            assert seg_slot[front_seg[s]] == slot0
        want = {s for s in fronts.tolist() if front_seg[s + 1] - front_seg[s] > 1}
        assert {int(t[0]) for t in pf[pfp[l]:pfp[l + 1]]} == want
    for q in range(grp.size - 1):
        used = []
        for s, slot0, ns in pf[pfp[grp[q]]:pfp[grp[q + 1]]]:
            used.extend(range(slot0, slot0 + ns))
        assert sorted(used) == list(range(len(used)))  # dense from 0, no slot twice
