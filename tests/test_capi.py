"""CPU tests of the C-ABI boundary: the library loads, exports every symbol include/scilmm_hip.h declares, and
fails loudly (no CPU fallback) when a numeric call is made without a GPU."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from scilmm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "scilmm_hip.h")).read()
    declared = set(re.findall(r"\b(scilmm_[a-z_A-Z0-9]+)\s*\(", header))
    L = _lib.lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(_lib.SYMBOLS)
    assert b"gfx950" in L.scilmm_version()


def test_numeric_calls_fail_loudly_without_gpu(gpu_available):
    if gpu_available:
        pytest.skip("a GPU is present")
    from scilmm_amd.factor import Symbolic
    A = sp.identity(4, format="csr") * 2.0
    with pytest.raises(_lib.ScilmmError):
        Symbolic([A])  # values_upload needs the device
    sym = Symbolic([A], upload=False)
    with pytest.raises(_lib.ScilmmError):
        sym.factorize([1.0])


def test_drop_in_surface_names():
    import scilmm_amd
    for name in ["SparseCholesky", "REML", "HE", "run_estimates", "run_estimates_from_paths", "bolt_gradient_estimation",
                 "estimate_var_comps", "compute_hess", "compute_varcomp_stderr", "matrices_weighted_sum"]:
        assert hasattr(scilmm_amd, name)
    from scilmm_amd.Estimation.LMM import LMM, SparseCholesky  # noqa: F401  (reference SciLMM.py:7)


def test_bad_arguments_are_rejected():
    from scilmm_amd.factor import Symbolic
    with pytest.raises(ValueError):
        Symbolic([sp.identity(3, format="csr"), sp.identity(4, format="csr")], upload=False)
    with pytest.raises(ValueError):
        Symbolic([sp.identity(3, format="csr")], perm=np.arange(4), upload=False)
    # the assembly maps may only be released once the values are in HBM (the device plan reads them)
    from scilmm_amd._lib import ScilmmError
    sym = Symbolic([sp.identity(3, format="csr")], upload=False)
    with pytest.raises(ScilmmError):
        sym.release_host_maps()


def test_round4_entry_points_validate_and_never_fall_back(gpu_available):
    """The entry points added in round 4 reject bad arguments on the host and -- without a GPU -- fail with the device error
    instead of computing anything on the CPU: `scilmm_csr_spmm_dev`, `scilmm_dominance_values_device`, the value-less
    `PatternCSR` analysis, `scilmm_timing.n_late_split`."""
    import ctypes as C
    from scilmm_amd.factor import PatternCSR, Symbolic
    L = _lib.lib()
    vp = C.c_void_p
    one = vp(8)   # (a non-null dummy: the argument checks come before any dereference)
    assert L.scilmm_csr_spmm_dev(-1, one, one, one, one, 1, vp(16), None) == _lib.ERR_ARG
    assert L.scilmm_csr_spmm_dev(4, one, one, one, one, 0, vp(16), None) == _lib.ERR_ARG      # r <= 0
    assert L.scilmm_csr_spmm_dev(4, one, one, one, one, 3, one, None) == _lib.ERR_ARG         # X and Y alias
    assert L.scilmm_csr_spmm_dev(4, None, one, one, one, 3, vp(16), None) == _lib.ERR_ARG
    assert L.scilmm_csr_spmm_dev(0, one, None, None, one, 3, vp(16), None) == _lib.OK         # empty matrix: nothing to do
    # a value-less pattern analyses like the matrix it came from
    A = (sp.random(60, 60, density=0.1, random_state=3, format="csr") + sp.identity(60, format="csr")).tocsr()
    A = (A + A.T).tocsr()
    A.sort_indices()
    P = PatternCSR(A.indptr, A.indices, 60)
    I = sp.identity(60, format="csr")
    sp_sym, sa_sym = Symbolic([P, I], upload=False), Symbolic([A, I], upload=False)
    assert np.array_equal(sp_sym.P(), sa_sym.P()) and sp_sym.info().nnzL == sa_sym.info().nnzL
    with pytest.raises(ValueError):
        PatternCSR(A.indptr[:-1], A.indices, 60)
    par = np.full((60, 2), -1, dtype=np.int32)
    for bad in ((0, 0), (0, 5), (-1, 0), (1, 0)):   # k_dst == k_src, out of range, the diagonal-only identity as a target
        assert L.scilmm_dominance_values_device(sp_sym._h, bad[0], bad[1], 60, _lib.ptr(par)) == _lib.ERR_ARG
    assert L.scilmm_dominance_values_device(sp_sym._h, 0, 0, 59, _lib.ptr(par)) == _lib.ERR_ARG
    assert "n_late_split" in dict(_lib.Timing._fields_)
    if not gpu_available:
        sym3 = Symbolic([P, P, I], upload=False)
        with pytest.raises(_lib.ScilmmError, match="HIP|device"):
            sym3.dominance_values_from(1, 0, par)            # needs the device: no CPU form exists
        with pytest.raises(_lib.ScilmmError, match="HIP|device"):
            sym3.ibd_values_from_pedigree(0, par)


def test_entry_points_reject_bad_arguments_before_any_device_state():
    """Every numeric entry point with a null or out-of-range argument, on a handle that has no device state (and a factor
    whose symbolic handle is null): the code comes from the argument checks alone, so it is the same with and without a
    GPU, and nothing is dereferenced.  The table was written from the checks as they stood before the entry points were
    reduced to checks + one call; `one` is a non-null dummy that a correct check order never reads."""
    import ctypes as C
    from scilmm_amd.factor import Symbolic
    L = _lib.lib()
    vp = C.c_void_p
    ARG, OK = _lib.ERR_ARG, _lib.OK
    n = 6
    A = (sp.diags([np.full(n - 1, 0.25), np.full(n, 2.0), np.full(n - 1, 0.25)], [-1, 0, 1])).tocsr()
    sym = Symbolic([A, sp.identity(n, format="csr")], upload=False)   # K = 2: matrix 1 is diagonal-only
    h = sym._h
    one = vp(8)
    hollow = C.create_string_buffer(256)            # a scilmm_factor with sym == NULL
    fac = C.cast(hollow, vp)
    dbl, i64 = C.c_double(0.0), C.c_int64(0)
    par = np.full((n, 2), -1, dtype=np.int32)
    late = par.copy()
    late[1, 0] = 3                                  # a parent that follows its child
    table = [
        ("values_upload", (None, 0, one), ARG), ("values_upload", (h, 0, None), ARG),
        ("values_upload", (h, -1, one), ARG), ("values_upload", (h, 2, one), ARG),
        ("values_download", (None, 0, one), ARG), ("values_download", (h, 0, one), ARG), ("values_download", (h, 0, None), ARG),
        ("factorize", (None, one, C.pointer(vp()), None), ARG), ("factorize", (h, None, C.pointer(vp()), None), ARG),
        ("factorize", (h, one, None, None), ARG),
        ("factor_create_external", (h, None, one, one, C.pointer(vp())), ARG),
        ("factor_create_external", (h, one, one, None, C.pointer(vp())), ARG), ("factor_create_external", (h, one, one, one, None), ARG),
        ("refactorize", (None, one, None), ARG), ("refactorize", (fac, one, None), ARG), ("refactorize", (fac, None, None), ARG),
        ("refactorize_async", (None, one), ARG), ("refactorize_async", (fac, one), ARG),
        ("factor_wait", (None, None), ARG), ("factor_wait", (fac, None), ARG),
        ("logdet", (None, C.byref(dbl)), ARG), ("logdet", (fac, C.byref(dbl)), ARG), ("logdet", (fac, None), ARG),
        ("export_L", (None, None, None, None, C.byref(i64)), ARG), ("export_L", (fac, None, None, None, C.byref(i64)), ARG),
        ("export_L", (fac, None, None, None, None), ARG),
        ("selected_inverse", (None,), ARG), ("selected_inverse", (fac,), ARG),
        ("inverse_traces", (None, one), ARG), ("inverse_traces", (fac, one), ARG), ("inverse_traces", (fac, None), ARG),
        ("he_moments", (None, 0, 1, C.byref(dbl), C.byref(dbl)), ARG), ("he_moments", (h, 0, 1, None, C.byref(dbl)), ARG),
        ("he_moments", (h, 0, 1, C.byref(dbl), None), ARG),
        ("ibd_values_device", (None, 0, n, _lib.ptr(par)), ARG), ("ibd_values_device", (h, 0, n, None), ARG),
        ("ibd_values_device", (h, -1, n, _lib.ptr(par)), ARG), ("ibd_values_device", (h, 2, n, _lib.ptr(par)), ARG),
        ("ibd_values_device", (h, 1, n, _lib.ptr(par)), ARG),        # the diagonal-only matrix
        ("ibd_values_device", (h, 0, n + 1, _lib.ptr(par)), ARG), ("ibd_values_device", (h, 0, n, _lib.ptr(late)), ARG),
        ("dominance_values_device", (None, 0, 1, n, _lib.ptr(par)), ARG), ("dominance_values_device", (h, 0, 1, n, None), ARG),
        ("dominance_values_device", (h, 0, 1, n, _lib.ptr(par)), ARG),   # the diagonal-only matrix as the source
        ("dominance_values_device", (h, 0, 2, n, _lib.ptr(par)), ARG), ("dominance_values_device", (h, 0, 0, n, _lib.ptr(par)), ARG),
        ("sync", (None,), ARG), ("sync", (h,), ARG), ("last_timing", (None, C.pointer(_lib.Timing())), ARG),
        ("last_timing", (h, C.pointer(_lib.Timing())), ARG), ("last_timing", (h, None), ARG),
        ("scan_timing", (None, C.byref(dbl)), ARG), ("scan_timing", (h, C.byref(dbl)), ARG),
        ("dist_set_work", (None, one), ARG), ("dist_set_work", (h, None), ARG),
        ("set_front_precision", (None, 32), ARG), ("set_front_precision", (h, 16), ARG), ("set_profiling", (None, 1), ARG),
        ("scan_block_dev", (None, one, n, 1, one, 1, one), ARG), ("scan_block_dev", (fac, one, n, 1, one, 1, one), ARG),
        ("scan_block_dev", (one, None, n, 1, one, 1, one), ARG), ("scan_block_dev", (one, one, n, 0, one, 1, one), ARG),
        ("scan_block_dev", (one, one, n, 129, one, 1, one), ARG), ("scan_block_dev", (one, one, n, 1, None, 1, one), ARG),
        ("scan_block_dev", (one, one, n, 1, one, 0, one), ARG), ("scan_block_dev", (one, one, n, 1, one, 1, None), ARG),
        ("rel_block_dev", (None, one, one, 1, one, 1, one), ARG), ("rel_block_dev", (fac, one, one, 1, one, 1, one), ARG),
        ("rel_block_dev", (one, None, one, 1, one, 1, one), ARG), ("rel_block_dev", (one, one, None, 1, one, 1, one), ARG),
        ("rel_block_dev", (one, one, one, 0, one, 1, one), ARG), ("rel_block_dev", (one, one, one, 129, one, 1, one), ARG),
        ("rel_block_dev", (one, one, one, 1, None, 1, one), ARG), ("rel_block_dev", (one, one, one, 1, one, 0, one), ARG),
        ("rel_block_dev", (one, one, one, 1, one, 1, None), ARG),
        ("rows_block_dev", (None, one, one, one, 1, one, 1, one), ARG), ("rows_block_dev", (fac, one, one, one, 1, one, 1, one), ARG),
        ("rows_block_dev", (one, None, one, one, 1, one, 1, one), ARG), ("rows_block_dev", (one, one, None, one, 1, one, 1, one), ARG),
        ("rows_block_dev", (one, one, one, None, 1, one, 1, one), ARG), ("rows_block_dev", (one, one, one, one, 0, one, 1, one), ARG),
        ("rows_block_dev", (one, one, one, one, 129, one, 1, one), ARG), ("rows_block_dev", (one, one, one, one, 1, None, 1, one), ARG),
        ("rows_block_dev", (one, one, one, one, 1, one, 0, one), ARG), ("rows_block_dev", (one, one, one, one, 1, one, 1, None), ARG),
    ]
    # the products (handle, k, block, r, out) and the sweeps (factor, block, r, out): null handle / block / out, r <= 0
    for name in ("spmm", "spmm_dev", "quadforms", "quadforms_dev"):
        table += [(name, (None, 0, one, 1, one), ARG), (name, (h, 0, None, 1, one), ARG), (name, (h, 0, one, 1, None), ARG),
                  (name, (h, 0, one, 0, one), ARG), (name, (h, 0, one, -3, one), ARG)]
    # (the half-solves and the blocks look at the factor last: `one` stands for it where another argument is bad)
    for name in ("solve", "lmul", "solve_dev", "lmul_dev", "solve_L", "solve_Lt", "solve_L_dev", "solve_Lt_dev"):
        f = one if "_L" in name else fac
        table += [(name, (None, one, 1, one), ARG), (name, (fac, one, 1, one), ARG), (name, (f, None, 1, one), ARG),
                  (name, (f, one, 1, None), ARG), (name, (f, one, 0, one), ARG)]
    got = [(name, i, getattr(L, "scilmm_" + name)(*args)) for i, (name, args, _) in enumerate(table)]
    assert got == [(name, i, want) for i, (name, _, want) in enumerate(table)]
    L.scilmm_factor_free(None)                      # (a null factor: nothing to do)
    assert OK == L.scilmm_get_deterministic(h, C.pointer(C.c_int32()))   # the handle is still usable and still has no device state
    assert L.scilmm_sync(h) == ARG
