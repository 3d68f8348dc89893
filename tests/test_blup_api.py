"""The BLUP surface without a device: exports, the two validators, argument checks of the C entry points, constructor errors,
and the agreement of the two dense oracles the GPU tests compare against."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from scilmm_amd import _lib
from tests import blup_oracle as O
from tests.helpers import rel_err


def test_exports():
    import scilmm_amd
    from scilmm_amd import blup
    from scilmm_amd.factor import Factor
    assert scilmm_amd.BLUP is blup.BLUP
    for name in ("rel_block_dev", "rows_block_dev"):
        assert callable(getattr(Factor, name)), name
    for name in ("effects", "reliability", "predict"):
        assert callable(getattr(blup.BLUP, name)), name
    L = _lib.lib()
    for name in ("scilmm_rel_block_dev", "scilmm_rows_block_dev"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name


def test_individuals_validation_needs_no_device():
    from scilmm_amd.blup import check_individuals
    ids = check_individuals([3, 0, 11], 12)
    assert ids.dtype == np.int32 and ids.flags.c_contiguous and ids.tolist() == [3, 0, 11]
    assert check_individuals(np.array([], dtype=np.int64), 12).shape == (0,)
    assert check_individuals(np.arange(12, dtype=np.uint8), 12).dtype == np.int32
    with pytest.raises(TypeError):
        check_individuals([0.0, 1.0], 12)
    with pytest.raises(TypeError):
        check_individuals(np.array([True, False]), 12)
    with pytest.raises(ValueError):
        check_individuals([[0, 1]], 12)                              # 2-D
    with pytest.raises(ValueError):
        check_individuals([0, 12], 12)                               # past the end
    with pytest.raises(ValueError):
        check_individuals([-1, 3], 12)
    with pytest.raises(ValueError):
        check_individuals([4, 7, 4], 12)                             # repeated
    with pytest.raises(ValueError):
        check_individuals(np.array([2 ** 32 + 1], dtype=np.int64), 12)   # (would wrap to 1 as int32)


def test_rows_validation_needs_no_device():
    from scilmm_amd.blup import check_rows
    rows = sp.coo_matrix(([0.5, 0.25, 0.25, 1.0], ([0, 0, 0, 2], [7, 2, 2, 11])), shape=(3, 12))
    (indptr, indices, data), self_rel = check_rows(rows, [1.0, 1.0, 1.5], 12)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float64
    assert indptr.tolist() == [0, 2, 2, 3] and indices.tolist() == [2, 7, 11] and data.tolist() == [0.5, 0.5, 1.0]
    assert self_rel.dtype == np.float64 and self_rel.tolist() == [1.0, 1.0, 1.5]
    unsorted = sp.csr_matrix((np.array([1.0, 2.0]), np.array([5, 1]), np.array([0, 2])), shape=(1, 12))
    (_, indices, data), _ = check_rows(unsorted, [1.0], 12)
    assert indices.tolist() == [1, 5] and data.tolist() == [2.0, 1.0]
    assert unsorted.indices.tolist() == [5, 1]                       # the caller's matrix is left alone
    (indptr, _, _), self_rel = check_rows(sp.csr_matrix((0, 12)), [], 12)
    assert indptr.tolist() == [0] and self_rel.shape == (0,)
    with pytest.raises(TypeError):
        check_rows(np.zeros((3, 12)), [1, 1, 1], 12)
    with pytest.raises(ValueError):
        check_rows(rows, [1, 1, 1], 13)                              # wrong n
    with pytest.raises(ValueError):
        check_rows(rows, [1, 1], 12)                                 # one self_rel per row
    with pytest.raises(ValueError):
        check_rows(rows, [[1, 1, 1]], 12)


def test_entry_points_check_their_arguments_first():
    """Dummy non-null pointers: the argument checks come before any dereference."""
    L = _lib.lib()
    one = C.c_void_p(8)
    for r, q in ((0, 2), (129, 2), (-1, 2), (4, 0), (4, 33)):
        assert L.scilmm_rel_block_dev(one, one, one, r, one, q, one) == _lib.ERR_ARG, (r, q)
        assert L.scilmm_rows_block_dev(one, one, one, one, r, one, q, one) == _lib.ERR_ARG, (r, q)
    for null in (0, 1, 2, 4, 6):
        args = [one, one, one, 4, one, 2, one]
        args[null] = None
        assert L.scilmm_rel_block_dev(*args) == _lib.ERR_ARG, null
    for null in (0, 1, 2, 3, 5, 7):
        args = [one, one, one, one, 4, one, 2, one]
        args[null] = None
        assert L.scilmm_rows_block_dev(*args) == _lib.ERR_ARG, null


def test_constructor_validates_and_has_no_cpu_form(gpu_available):
    from scilmm_amd import BLUP, ScilmmError, SparseCholesky
    n = 40
    A = (sp.random(n, n, density=0.1, random_state=1, format="csr") + 10 * sp.identity(n, format="csr")).tocsr()
    A = (A + A.T).tocsr()
    A.sort_indices()
    I = sp.identity(n, format="csr")
    Cv, y = np.ones((n, 1)), np.arange(n, dtype=float)
    chol = SparseCholesky()
    for block in (0, 129, 1.5):
        with pytest.raises(ValueError):
            BLUP(chol, [A, I], [0.5, 0.5], Cv, y, block=block)
    with pytest.raises(ValueError):
        BLUP(chol, [A, I], [0.5, 0.5], np.ones((n, 32)), y)      # [w(C) | w(y)] has at most 32 columns
    with pytest.raises(ValueError):
        BLUP(chol, [A, I], [0.5, 0.5], Cv, y[:-1])               # one row of the covariates per entry of y
    with pytest.raises(ScilmmError):
        BLUP(lambda V: None, [A, I], [0.5, 0.5], Cv, y)           # not the device engine
    if not gpu_available:
        with pytest.raises(ScilmmError):
            BLUP(chol, [A, I], [0.5, 0.5], Cv, y)


def test_the_two_dense_oracles_agree():
    """Henderson's mixed-model equations and the dense P_V form are independent definitions of beta, u and PEV: they must
    agree on G1 to 1e-12 (measured 2e-15), at a round sigma2 and at the golden's estimate."""
    A, Cv, y, s2_hat = O.golden_g1()
    n = A.shape[0]
    for s2 in ((0.4, 0.6), tuple(s2_hat)):
        beta_h, u_h, pev_h = O.henderson(A, Cv, y, s2[0], s2[1])
        pv = O.DensePV([A, sp.identity(n, format="csr")], s2, Cv, y)
        u_p, pev_p = pv.columns(0)
        errs = rel_err(beta_h, pv.beta), rel_err(u_h, u_p), rel_err(pev_h, pev_p)
        print("sigma2", s2, "beta, u, pev rel.err", errs)
        assert max(errs) < 1e-12
        assert pev_p.min() > 0 and np.all(pev_p < s2[0] * A.diagonal())
