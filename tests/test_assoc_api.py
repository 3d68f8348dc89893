"""The association scan's surface without a device: exports, genotype validation, argument checks of the C entry points."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from scilmm_amd import _lib


def test_exports():
    import scilmm_amd
    from scilmm_amd import assoc
    from scilmm_amd.factor import Factor
    assert scilmm_amd.AssociationScan is assoc.AssociationScan
    for name in ("solve_L", "solve_Lt", "apply_P", "apply_Pt", "solve_L_dev", "solve_Lt_dev"):
        assert callable(getattr(Factor, name)), name
    L = _lib.lib()
    for name in ("scilmm_solve_L", "scilmm_solve_Lt", "scilmm_solve_L_dev", "scilmm_solve_Lt_dev", "scilmm_scan_block_dev"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert 112 <= assoc.DEFAULT_BLOCK <= assoc.RPMAX == 128


def test_genotype_validation_needs_no_device():
    from scilmm_amd.assoc import check_genotypes
    G = np.zeros((5, 12), dtype=np.int8)
    assert check_genotypes(G, 12) is G
    assert check_genotypes(G[1:3], 12).shape == (2, 12)          # a block of whole rows stays C-contiguous
    with pytest.raises(TypeError):
        check_genotypes(G.astype(np.float64), 12)
    with pytest.raises(TypeError):
        check_genotypes(G.astype(np.int16), 12)
    with pytest.raises(TypeError):
        check_genotypes(G.tolist(), 12)
    with pytest.raises(ValueError):
        check_genotypes(G[0], 12)                                 # 1-D
    with pytest.raises(ValueError):
        check_genotypes(G, 13)                                    # wrong n
    with pytest.raises(ValueError):
        check_genotypes(np.asfortranarray(G), 12)
    with pytest.raises(ValueError):
        check_genotypes(G[:, ::2], 6)                             # strided columns


def test_genotype_memmap_is_accepted(tmp_path):
    from scilmm_amd.assoc import check_genotypes
    path = tmp_path / "g.i8"
    np.arange(60, dtype=np.int8).tofile(path)
    mm = np.memmap(path, dtype=np.int8, mode="r", shape=(5, 12))
    assert check_genotypes(mm, 12) is mm


def test_entry_points_check_their_arguments_first():
    """Dummy non-null pointers: the argument checks come before any dereference."""
    L = _lib.lib()
    one = C.c_void_p(8)
    for r, q in ((0, 2), (129, 2), (-1, 2), (4, 0), (4, 33)):
        assert L.scilmm_scan_block_dev(one, one, 64, r, one, q, one) == _lib.ERR_ARG, (r, q)
    for args in ((None, one, 64, 4, one, 2, one), (one, None, 64, 4, one, 2, one), (one, one, 64, 4, None, 2, one),
                 (one, one, 64, 4, one, 2, None)):
        assert L.scilmm_scan_block_dev(*args) == _lib.ERR_ARG
    for fn in (L.scilmm_solve_L, L.scilmm_solve_Lt, L.scilmm_solve_L_dev, L.scilmm_solve_Lt_dev):
        assert fn(one, one, 0, one) == _lib.ERR_ARG
        assert fn(one, one, -3, one) == _lib.ERR_ARG
        assert fn(None, one, 1, one) == _lib.ERR_ARG
        assert fn(one, None, 1, one) == _lib.ERR_ARG
        assert fn(one, one, 1, None) == _lib.ERR_ARG


def test_constructor_validates_and_has_no_cpu_form(gpu_available):
    from scilmm_amd import AssociationScan, ScilmmError, SparseCholesky
    n = 40
    A = (sp.random(n, n, density=0.1, random_state=1, format="csr") + 10 * sp.identity(n, format="csr")).tocsr()
    A = (A + A.T).tocsr()
    A.sort_indices()
    I = sp.identity(n, format="csr")
    Cv, y = np.ones((n, 1)), np.arange(n, dtype=float)
    chol = SparseCholesky()
    for block in (0, 129, 1.5):
        with pytest.raises(ValueError):
            AssociationScan(chol, [A, I], [0.5, 0.5], Cv, y, block=block)
    with pytest.raises(ValueError):
        AssociationScan(chol, [A, I], [0.5, 0.5], np.ones((n, 32)), y)      # [w(C) | w(y)] has at most 32 columns
    with pytest.raises(ScilmmError):
        AssociationScan(lambda V: None, [A, I], [0.5, 0.5], Cv, y)           # not the device engine
    if not gpu_available:
        with pytest.raises(ScilmmError):
            AssociationScan(chol, [A, I], [0.5, 0.5], Cv, y)
