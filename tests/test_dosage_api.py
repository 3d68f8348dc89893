"""The dosage path's surface without a device: exports, the uint16 fixed point (encode / decode), the validation of a dosage
matrix, and the argument checks of the two C entry points, which come before anything of the handle is read."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from scilmm_amd import _lib


def test_exports():
    import scilmm_amd
    from scilmm_amd import dosage
    from scilmm_amd.assoc import AssociationScan
    from scilmm_amd.factor import Factor
    from scilmm_amd.sets import VariantSetTest
    assert scilmm_amd.dosage is dosage
    assert (dosage.DOSAGE_ONE, dosage.DOSAGE_MISSING) == (16384, 65535)
    for name in ("encode", "decode", "check_dosages"):
        assert callable(getattr(dosage, name)), name
    assert callable(AssociationScan.scan_dosages) and callable(VariantSetTest.test_dosages)
    for name in ("scan_block_dosage_dev", "scan_block_dosage_gram_dev"):
        assert callable(getattr(Factor, name)), name
    L = _lib.lib()
    for name in ("scilmm_scan_block_dosage_dev", "scilmm_scan_block_dosage_gram_dev"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert (_lib.DOSAGE_U16, _lib.DOSAGE_F32) == (0, 1)


def test_encode_decode():
    from scilmm_amd.dosage import decode, encode
    calls = np.array([[0, 1, 2], [2, 2, 0]])
    codes = encode(calls)
    assert codes.dtype == np.uint16 and np.array_equal(codes, calls * 16384)
    back = decode(codes)
    assert back.dtype == np.float64 and np.array_equal(back, calls)                 # hard calls come back exactly
    rng = np.random.default_rng(0)
    for dt in (np.float64, np.float32):
        d = rng.uniform(0.0, 2.0, (7, 33)).astype(dt)
        d[0, :3] = [0.0, 2.0, 1.0]
        err = np.abs(decode(encode(d)) - d.astype(np.float64)).max()
        assert err <= 2.0 ** -15, err                                                # half a code
    d = np.array([0.25, np.nan, 1.5])
    codes = encode(d)
    assert np.array_equal(codes, [4096, 65535, 24576])
    assert np.array_equal(decode(codes), d, equal_nan=True)
    assert np.all(np.isnan(decode(np.array([32769, 40000, 65534, 65535], dtype=np.uint16))))   # every code above 32768
    assert decode(np.array([32768], dtype=np.uint16))[0] == 2.0
    for bad in (-1e-3, 2.0 + 1e-3, np.inf, -np.inf):
        with pytest.raises(ValueError):
            encode(np.array([0.5, bad]))
    assert encode(np.empty((0, 5))).shape == (0, 5)
    with pytest.raises(TypeError):
        decode(np.array([1.0]))


def test_check_dosages(tmp_path):
    from scilmm_amd.dosage import check_dosages
    for dt in (np.uint16, np.float32):
        D = np.zeros((5, 12), dtype=dt)
        assert check_dosages(D, 12) is D                             # nothing is copied
        assert check_dosages(D, None) is D
        assert check_dosages(D[1:3], 12).shape == (2, 12)            # a block of whole rows stays C-contiguous
        with pytest.raises(ValueError):
            check_dosages(D[0], 12)                                  # 1-D
        with pytest.raises(ValueError):
            check_dosages(D, 13)                                     # wrong N
        with pytest.raises(ValueError):
            check_dosages(np.asfortranarray(D), 12)
        with pytest.raises(ValueError):
            check_dosages(D[:, ::2], 6)                              # strided columns
    D = np.zeros((5, 12))
    with pytest.raises(TypeError, match="float32.*encode"):
        check_dosages(D, 12)                                         # float64: says what to do
    for dt in (np.int8, np.int16, np.float16, np.uint8):
        with pytest.raises(TypeError):
            check_dosages(D.astype(dt), 12)
    with pytest.raises(TypeError):
        check_dosages(D.astype(np.float32).tolist(), 12)
    for dt in (np.uint16, np.float32):
        path = tmp_path / ("d.%s" % np.dtype(dt).name)
        np.arange(60).astype(dt).tofile(path)
        mm = np.memmap(path, dtype=dt, mode="r", shape=(5, 12))
        assert check_dosages(mm, 12) is mm


def test_genotype_path_still_refuses_dosages():
    from scilmm_amd.assoc import check_genotypes
    for dt in (np.uint16, np.float32):
        with pytest.raises(TypeError):
            check_genotypes(np.zeros((5, 12), dtype=dt), 12)


def test_entry_points_check_their_arguments_first():
    """Dummy non-null pointers (8 is aligned to both element sizes): the argument checks come before any dereference."""
    L = _lib.lib()
    one, odd, two = C.c_void_p(8), C.c_void_p(9), C.c_void_p(10)
    f, g = L.scilmm_scan_block_dosage_dev, L.scilmm_scan_block_dosage_gram_dev
    U16, F32, ARG = _lib.DOSAGE_U16, _lib.DOSAGE_F32, _lib.ERR_ARG

    def both(fac, dos, dtype, ld, N, smp, r, dQ, q, st):
        return f(fac, dos, dtype, ld, N, smp, r, dQ, q, st), g(fac, dos, dtype, ld, N, smp, r, dQ, q, st, one)

    for dtype in (U16, F32):
        for r, q in ((0, 2), (129, 2), (-1, 2), (4, 0), (4, 33), (4, -1)):
            assert both(one, one, dtype, 64, 64, one, r, one, q, one) == (ARG, ARG), (r, q)
        for N in (0, -1):
            assert both(one, one, dtype, 64, N, one, 4, one, 2, one) == (ARG, ARG)         # n_samples < 1
        assert both(one, one, dtype, 63, 64, one, 4, one, 2, one) == (ARG, ARG)            # pitch shorter than a row
        assert both(None, one, dtype, 64, 64, one, 4, one, 2, one) == (ARG, ARG)           # each null pointer
        assert both(one, None, dtype, 64, 64, one, 4, one, 2, one) == (ARG, ARG)
        assert both(one, one, dtype, 64, 64, one, 4, None, 2, one) == (ARG, ARG)
        assert both(one, one, dtype, 64, 64, one, 4, one, 2, None) == (ARG, ARG)
        assert g(one, one, dtype, 64, 64, one, 4, one, 2, one, None) == ARG                # a null d_gram
        assert both(one, odd, dtype, 64, 64, one, 4, one, 2, one) == (ARG, ARG)            # a base off its element size
    assert both(one, two, F32, 64, 64, one, 4, one, 2, one) == (ARG, ARG)                  # 2-byte aligned is not enough for float
    for dtype in (2, 3, -1, 16, 1 << 30):
        assert both(one, one, dtype, 64, 64, one, 4, one, 2, one) == (ARG, ARG), dtype     # an unknown element type


def test_scan_dosages_is_unreachable_without_a_gpu(gpu_available):
    from scilmm_amd import AssociationScan, ScilmmError, SparseCholesky, VariantSetTest
    n = 40
    A = (sp.random(n, n, density=0.1, random_state=1, format="csr") + 10 * sp.identity(n, format="csr")).tocsr()
    A = (A + A.T).tocsr()
    A.sort_indices()
    I = sp.identity(n, format="csr")
    Cv, y = np.ones((n, 1)), np.arange(n, dtype=float)
    for cls in (AssociationScan, VariantSetTest):
        with pytest.raises(ScilmmError):
            cls(lambda V: None, [A, I], [0.5, 0.5], Cv, y)               # not the device engine
        if not gpu_available:
            with pytest.raises(ScilmmError):
                cls(SparseCholesky(), [A, I], [0.5, 0.5], Cv, y)         # no object, so no scan_dosages to call
