"""Python handles over the C-ABI (include/scilmm_hip.h): ``Symbolic`` (pattern analysis + device-resident
A_k values) and ``Factor`` (numeric factor with the reference's factor protocol).

Factor protocol mirrored from what the reference touches on an sksparse Factor
(reference scilmm/SparseCholesky.py:30,32,40,50,52,93,100; scilmm/Estimation/LMM.py:28,30,38,48-50,87,94):
``factor(b)``, ``factor.L()``, ``factor.P()``, ``factor.logdet()`` -- plus ``factor.lmul(R)``, the fused
form of ``factor.L().dot(R)[argsort(P)]`` that never materialises L on the host, and the four pieces of ``factor(b)`` the
sksparse protocol also offers: ``solve_L``, ``solve_Lt``, ``apply_P``, ``apply_Pt`` (what ``scilmm_amd.assoc`` is built on).
"""
import ctypes as C
import os

import numpy as np
import scipy.sparse as sp

from . import _lib
from ._lib import check, lib, ptr

_ORDERINGS = {"amd": 0, "natural": 1, "given": 2, "nesdis": 3, "best": 4}


class PatternCSR(object):
    """A CSR sparsity pattern WITHOUT values (canonical: rows ascending, both halves stored): what ``Symbolic`` needs of a
    matrix whose values are then computed on the device (``ibd_values_from_pedigree``, ``dominance_values_from``) -- at
    BASELINE configs[4]'s 3M pedigree that is 21.6 GB of values per matrix that never exist on the host."""

    has_sorted_indices = True
    data = None

    def __init__(self, indptr, indices, n):
        self.indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        self.indices = np.ascontiguousarray(indices, dtype=np.int32)
        self.shape = (int(n), int(n))
        if self.indptr.shape != (n + 1,) or int(self.indptr[-1]) != self.indices.size:
            raise ValueError("indptr / indices do not describe an n x n CSR pattern")
        self.nnz = int(self.indices.size)


def _as_csr(m):
    if isinstance(m, PatternCSR):
        return m
    m = sp.csr_matrix(m)
    if not m.has_sorted_indices:
        m = m.sorted_indices()
    return m


class Symbolic(object):
    """Symbolic analysis of the pattern of V = sum_k s2_k mats[k]; built once, reused for every sigma2."""

    def __init__(self, mats, perm=None, ordering="amd", upload=True, deterministic=None, **opts):
        """deterministic: True / False selects or clears the bitwise-reproducible mode of the handle (factorization, solves,
        L*R, SpMM in a fixed summation order: ``scilmm_set_deterministic``); None follows SCILMM_DETERMINISTIC."""
        mats = [_as_csr(m) for m in mats]
        self.n = n = mats[0].shape[0]
        for m in mats:
            if m.shape != (n, n):
                raise ValueError("all matrices must be square and of equal shape")
        self.K = K = len(mats)
        self._indptr = [np.ascontiguousarray(m.indptr, dtype=np.int64) for m in mats]
        self._indices = [np.ascontiguousarray(m.indices, dtype=np.int32) for m in mats]
        self._data = [None if m.data is None else np.ascontiguousarray(m.data, dtype=np.float64) for m in mats]
        self._values_epoch = 0  # bumped whenever the resident values of a matrix change (Factor.holds)
        if perm is not None:
            ordering = "given"
            perm = np.ascontiguousarray(perm, dtype=np.int32)
            if perm.shape != (n,):
                raise ValueError("perm must have length n")
        cache = opts.pop("cache", None) or os.environ.get("SCILMM_SYMBOLIC_CACHE")
        o = _lib.Options.default(_ORDERINGS[ordering], **opts)
        a = (C.c_void_p * K)(*[x.ctypes.data for x in self._indptr])
        b = (C.c_void_p * K)(*[x.ctypes.data for x in self._indices])
        h = C.c_void_p()
        self.from_cache = False
        path = key = None
        if cache:
            # image of the analysis keyed by everything it depends on: patterns, permutation, ordering, options
            # (scilmm_symbolic_save / _load: once per pattern and node instead of once per process)
            key = self._analysis_key(n, perm, ordering, opts)
            path = os.path.join(cache, "scilmm_symbolic_%016x.bin" % key)
            if lib().scilmm_symbolic_load(os.fsencode(path), C.c_uint64(key), C.byref(h)) == _lib.OK:
                self.from_cache = True
        if not self.from_cache:
            st = lib().scilmm_symbolic_create(n, K, a, b, None if perm is None else ptr(perm), C.byref(o), 1, C.byref(h))
            self._h = h
            check(st, h)
            if path is not None:
                os.makedirs(cache, exist_ok=True)
                lib().scilmm_symbolic_save(h, os.fsencode(path), C.c_uint64(key))  # best effort: a failed write is not an error
        self._h = h
        self._uploaded = False
        self.front_bits = 64
        if deterministic is not None:
            check(lib().scilmm_set_deterministic(h, 1 if deterministic else 0), h)
        if upload:
            self.upload_values()

    # every environment variable that changes what the host analysis computes (read_analysis_switches in csrc/symbolic.cpp,
    # its only reader of the environment; tests/test_symbolic.py compares the two lists): part of the cache key
    _ANALYSIS_ENV = ("SCILMM_TUNING", "SCILMM_TAIL_WIDE", "SCILMM_TAIL_ELIG", "SCILMM_TAIL_DELAY")
    # bumped whenever the analysis changes what it produces for the same input (the library's magic number guards the FORMAT of
    # the image, this constant and scilmm_version() its CONTENT)
    _ANALYSIS_REVISION = 4

    def _analysis_key(self, n, perm, ordering, opts):
        """64-bit key of everything the analysis depends on: patterns, permutation, ordering, options, the environment
        variables it reads, the library version and the analysis revision.  xxhash when it is installed (0.5 s per 4 GB of
        pattern), hashlib.blake2b otherwise (standard library: no dependency is needed for the cache to work)."""
        try:
            import xxhash
            hx = xxhash.xxh64()
            digest = hx.intdigest
        except ImportError:
            import hashlib
            hx = hashlib.blake2b(digest_size=8)
            digest = lambda: int.from_bytes(hx.digest(), "little")
        hx.update(np.array([n, self.K, _ORDERINGS[ordering], self._ANALYSIS_REVISION], dtype=np.int64).tobytes())
        hx.update(lib().scilmm_version())
        hx.update(repr(sorted(opts.items())).encode())
        hx.update(repr(sorted((k, v) for k, v in os.environ.items() if k in self._ANALYSIS_ENV)).encode())
        if perm is not None:
            hx.update(perm.tobytes())
        for ip, ix in zip(self._indptr, self._indices):
            hx.update(memoryview(ip).cast("B"))
            hx.update(memoryview(ix).cast("B"))
        return digest()

    def upload_values(self, skip=()):
        self._values_epoch += 1
        for k in range(self.K):
            if k not in skip and self._data[k] is not None:  # (None: a PatternCSR -- its values are built on the device)
                check(lib().scilmm_values_upload(self._h, k, ptr(self._data[k])), self._h)
        self._uploaded = True

    def ibd_values_from_pedigree(self, k, parents):
        """Compute matrix k's values -- the IBD (numerator relationship) matrix of the pedigree ``parents`` ((n, 2), -1 =
        unknown, individuals in the matrices' row order, parents before children) -- ON THE DEVICE, straight into its
        HBM-resident value slots: they never cross PCIe (``scilmm_ibd_values_device``).  The analysed pattern of matrix k
        must be the pedigree's common-ancestor pattern (``scilmm_amd.ibd.ibd_pattern_from_parents``)."""
        par = np.ascontiguousarray(parents, dtype=np.int32)
        if par.shape != (self.n, 2):
            raise ValueError("parents must be an (n, 2) table")
        self._values_epoch += 1
        check(lib().scilmm_ibd_values_device(self._h, k, self.n, ptr(par)), self._h)

    def dominance_values_from(self, k_dst, k_src, parents):
        """Compute matrix ``k_dst``'s values -- the dominance relationship matrix of the pedigree ``parents`` on the analysed
        pattern (reference scilmm/Matrices/Dominance.py:12-43) -- ON THE DEVICE from matrix ``k_src``'s resident IBD values,
        straight into its value slots (``scilmm_dominance_values_device``)."""
        par = np.ascontiguousarray(parents, dtype=np.int32)
        if par.shape != (self.n, 2):
            raise ValueError("parents must be an (n, 2) table")
        self._values_epoch += 1
        check(lib().scilmm_dominance_values_device(self._h, k_dst, k_src, self.n, ptr(par)), self._h)

    def values_slots(self, k):
        """Matrix k's device-resident values in pattern-slot order (tests, diagnostics)."""
        diag_only = self._indices[k].size == self.n and np.array_equal(self._indices[k], np.arange(self.n))
        out = np.empty(self.n if diag_only else self.info().nnz_pattern)
        check(lib().scilmm_values_download(self._h, k, ptr(out)), self._h)
        return out

    def release_host_maps(self):
        """Free the host copies of the value-assembly maps and of the uploaded values (a process that only evaluates does not
        need them: 13 + 7 GB at the 1M config); ``set_values`` is no longer available afterwards."""
        check(lib().scilmm_symbolic_release_host_maps(self._h), self._h)
        self._data = [None] * self.K

    def set_values(self, k, data):
        """Replace the values of matrix k (same pattern)."""
        data = np.ascontiguousarray(data, dtype=np.float64)
        if self._data[k] is not None:
            if data.shape != self._data[k].shape:
                raise ValueError("value array does not match the analysed pattern")
            self._data[k] = data
        self._values_epoch += 1
        check(lib().scilmm_values_upload(self._h, k, ptr(data)), self._h)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                lib().scilmm_symbolic_free(h)
            except Exception:  # interpreter shutdown: the module's globals are already gone, the process frees everything
                pass
            self._h = None

    def info(self):
        info = _lib.Info()
        check(lib().scilmm_symbolic_info(self._h, C.byref(info)), self._h)
        return info

    def get(self, name):
        return _lib.symbolic_get(self._h, name)

    def arrays(self):
        names = ["perm", "sn_start", "sn_rowptr", "sn_rows", "sn_loff", "upd_ptr", "upd_src", "upd_p0", "upd_p1",
                 "asm_dst", "diag_dst"]
        return {k: self.get(k) for k in names}

    def P(self):
        return self.get("perm").astype(np.int64)

    def factorize(self, sigma2):
        return Factor(self, sigma2)

    def quadforms(self, k, U):
        """out[c] = sum_i (A_k U)_ic U_ic  (compute_gradients, SparseCholesky.py:65)."""
        U = np.ascontiguousarray(np.asarray(U, dtype=np.float64).reshape(self.n, -1))
        out = np.empty(U.shape[1])
        check(lib().scilmm_quadforms(self._h, k, ptr(U), U.shape[1], ptr(out)), self._h)
        return out

    def he_moments(self, k1, k2):
        """(sum(A_k1 o A_k2), diag(A_k1) . diag(A_k2)) from the device-resident values (HE, SparseCholesky.py:223-231)."""
        fro, dg = C.c_double(0.0), C.c_double(0.0)
        check(lib().scilmm_he_moments(self._h, k1, k2, C.byref(fro), C.byref(dg)), self._h)
        return fro.value, dg.value

    def spmm(self, k, X):
        X = np.asarray(X, dtype=np.float64)
        X2 = np.ascontiguousarray(X.reshape(self.n, -1))
        Y = np.empty_like(X2)
        check(lib().scilmm_spmm(self._h, k, ptr(X2), X2.shape[1], ptr(Y)), self._h)
        return Y.reshape(X.shape)

    def set_front_precision(self, bits):
        """32: dense-tail products on the fp32 matrix pipe, sums in fp64 (BASELINE configs[4]); 64: all fp64 (default).
        With 32 the factor has a ~1e-7 relative backward error; ``Factor.__call__`` then refines its solves."""
        check(lib().scilmm_set_front_precision(self._h, int(bits)), self._h)
        self.front_bits = int(bits)

    @property
    def deterministic(self):
        """True when every sum of an evaluation on this handle runs in a fixed order (``scilmm_set_deterministic``)."""
        on = C.c_int32(0)
        check(lib().scilmm_get_deterministic(self._h, C.byref(on)), self._h)
        return bool(on.value)

    def set_profiling(self, on=True):
        """True / 1: HIP-event brackets per kernel class; 2: also queue the look-ahead launches on one stream (clean
        per-launch durations of the dominant kernel; a measurement mode)."""
        check(lib().scilmm_set_profiling(self._h, 2 if on == 2 else int(bool(on))), self._h)

    def sync(self):
        check(lib().scilmm_sync(self._h), self._h)

    def spmm_dev(self, k, dX_ptr, r, dY_ptr):
        """Y = A_k X with device pointers ([n][r] blocks), asynchronous on the engine's stream."""
        check(lib().scilmm_spmm_dev(self._h, k, dX_ptr, r, dY_ptr), self._h)

    def quadforms_dev(self, k, dU_ptr, r, dout_ptr):
        check(lib().scilmm_quadforms_dev(self._h, k, dU_ptr, r, dout_ptr), self._h)

    def _timing(self, name, count):
        """The ``count`` intervals of ``scilmm_<name>_timing`` in ms: a float where there is one, a tuple otherwise."""
        ms = (C.c_double * count)()
        check(getattr(lib(), "scilmm_%s_timing" % name)(self._h, ms), self._h)
        return float(ms[0]) if count == 1 else tuple(float(v) for v in ms)

    def scan_timing(self):
        """(moments + dequantise, forward sweep, statistics) of the last scan block in ms, after ``sync()``."""
        return self._timing("scan", 3)

    def gxe_timing(self):
        """(``k_scan_expand``, ``k_scan_cross`` + its fold) of the last scan block in ms, after ``sync()``: parts of the first
        and the third interval of ``scan_timing``; zeros after a block that was no gxe block."""
        return self._timing("gxe", 2)

    def panel_timing(self):
        """(``k_scan_panel``, ``k_panel_fold``) of the last ``Factor.scan_panel_dev`` in ms, after ``sync()``."""
        return self._timing("panel", 2)

    def spa_timing(self):
        """``k_scan_spa`` of the last ``Factor.scan_spa*_dev`` in ms, after ``sync()``."""
        return self._timing("spa", 1)

    def sets_finish_timing(self):
        """``k_sets_finish`` of the last ``Factor.sets_finish_dev`` in ms, after ``sync()``."""
        return self._timing("sets_finish", 1)

    def sets_finish_wide_timing(self):
        """(prep + form, reduction, eigenvalues, tails) of the last ``Factor.sets_finish_wide_dev`` in ms, after ``sync()``."""
        return self._timing("sets_finish_wide", 4)

    def sets_finish_panel_timing(self):
        """(``k_sets_spectra``, ``k_sets_panel_tail``) of the last ``Factor.sets_finish_panel_dev`` in ms, after ``sync()``."""
        return self._timing("sets_finish_panel", 2)

    def sets_finish_masks_timing(self):
        """``k_sets_finish_masks`` of the last ``Factor.sets_finish_masks_dev`` in ms, after ``sync()``."""
        return self._timing("sets_finish_masks", 1)

    def sets_spa_timing(self):
        """``k_sets_spa`` of the last ``Factor.sets_spa*_dev`` in ms, after ``sync()``."""
        return self._timing("sets_spa", 1)

    def sets_spa_wide_timing(self):
        """(the last ``Factor.sets_collapse*_dev``, markers + pairs and the burden kernel of the last ``Factor.sets_spa_wide_dev``)
        in ms, after ``sync()``."""
        return self._timing("sets_spa_wide", 3)

    def timing(self):
        t = _lib.Timing()
        check(lib().scilmm_last_timing(self._h, C.byref(t)), self._h)
        return {f: getattr(t, f) for f, _ in _lib.Timing._fields_}


class Factor(object):
    """Numeric factor L L^T = V[P][:,P] living in HBM."""

    def __init__(self, symbolic, sigma2):
        self.sym = symbolic
        self.n = symbolic.n
        s2 = np.ascontiguousarray(sigma2, dtype=np.float64)
        if s2.shape != (symbolic.K,):
            raise ValueError("sigma2 must have one entry per matrix")
        h = C.c_void_p()
        bad = C.c_int32(-1)
        st = lib().scilmm_factorize(symbolic._h, ptr(s2), C.byref(h), C.byref(bad))
        self._h = h
        self._s2, self._epoch, self._pending = None, -1, None
        check(st, symbolic._h, bad.value)
        self._s2, self._epoch = s2.copy(), symbolic._values_epoch

    @classmethod
    def from_handle(cls, symbolic, handle):
        """A Factor object around an existing ``scilmm_factor*`` (caller-owned storage: ``scilmm_factor_create_external``,
        the multi-GPU engine); nothing is factorized yet."""
        f = cls.__new__(cls)
        f.sym, f.n, f._h = symbolic, symbolic.n, handle
        f._s2, f._epoch, f._pending = None, -1, None
        return f

    def holds(self, sigma2):
        """True when this object IS the factor of sum_k sigma2[k] A_k for the values now resident (so that a caller -- the
        reference factorizes once more at the optimum, SparseCholesky.py:182 -- need not repeat a factorization it has)."""
        return (self._s2 is not None and self._epoch == self.sym._values_epoch
                and np.array_equal(self._s2, np.asarray(sigma2, dtype=np.float64)))

    def refactorize(self, sigma2):
        s2 = np.ascontiguousarray(sigma2, dtype=np.float64)
        bad = C.c_int32(-1)
        self._s2, self._pending = None, None  # (a recorded async request is superseded: its sigma2 must never be adopted later)
        check(lib().scilmm_refactorize(self._h, ptr(s2), C.byref(bad)), self.sym._h, bad.value)
        self._s2, self._epoch = s2.copy(), self.sym._values_epoch
        return self

    def refactorize_async(self, sigma2):
        """Queue the refactorization and return; ``wait()`` (or any use of the factor) completes it."""
        s2 = np.ascontiguousarray(sigma2, dtype=np.float64)
        self._s2, self._pending = None, None
        check(lib().scilmm_refactorize_async(self._h, ptr(s2)), self.sym._h)
        self._pending = (s2.copy(), self.sym._values_epoch)
        return self

    def wait(self):
        bad = C.c_int32(-1)
        pending, self._pending = getattr(self, "_pending", None), None  # cleared whatever happens: a failed factorization
        check(lib().scilmm_factor_wait(self._h, C.byref(bad)), self.sym._h, bad.value)  # (raises) leaves no sigma2 behind
        if pending is not None:
            self._s2, self._epoch = pending
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                lib().scilmm_factor_free(h)
            except Exception:  # (interpreter shutdown, as above)
                pass
            self._h = None

    def _rhs(self, fn, b):
        b = np.asarray(b, dtype=np.float64)
        if b.shape[0] != self.n:
            raise ValueError("right-hand side has %d rows, expected %d" % (b.shape[0], self.n))
        B = np.ascontiguousarray(b.reshape(self.n, -1))
        X = np.empty_like(B)
        check(fn(self._h, ptr(B), B.shape[1], ptr(X)), self.sym._h)
        return X.reshape(b.shape)

    REFINE_STEPS = 2  # iterative-refinement sweeps of a solve on a factor with fp32 fronts

    def __call__(self, b):
        """factor(b) = V^{-1} b for b of shape (n,) or (n, r).  On a factor with fp32 fronts (set_front_precision(32))
        the solve is refined against the exact V = sum_k s2_k A_k (fp64 SpMM on the device): each sweep gains ~7 digits."""
        if getattr(self, "_pending", None) is not None:
            self.wait()
        x = self._rhs(lib().scilmm_solve, b)
        if getattr(self.sym, "front_bits", 64) == 32 and getattr(self, "_s2", None) is not None:
            b = np.asarray(b, dtype=np.float64)
            for _ in range(self.REFINE_STEPS):
                r = b.copy()
                for k in range(self.sym.K):
                    r -= self._s2[k] * self.sym.spmm(k, x)
                x = x + self._rhs(lib().scilmm_solve, r)
        return x

    def lmul(self, R):
        """(factor.L() @ R)[argsort(factor.P())] without exporting L (simulate_vector, SparseCholesky.py:50-51)."""
        return self._rhs(lib().scilmm_lmul, R)

    def solve_dev(self, dB_ptr, r, dX_ptr):
        """Device-pointer solve (row-major n x r, original row order); enqueues without synchronising."""
        check(lib().scilmm_solve_dev(self._h, dB_ptr, r, dX_ptr), self.sym._h)

    def lmul_dev(self, dR_ptr, r, dZ_ptr):
        check(lib().scilmm_lmul_dev(self._h, dR_ptr, r, dZ_ptr), self.sym._h)

    # ---- the halves of factor(b) (sksparse: solve_L / solve_Lt with use_LDLt_decomposition=False, apply_P, apply_Pt):
    #      f(b) == f.apply_Pt(f.solve_Lt(f.solve_L(f.apply_P(b)))), bit for bit on a deterministic handle

    def solve_L(self, b):
        """x with L x = b, for b of shape (n,) or (n, r) whose rows are in the factor's PERMUTED order (``apply_P(b)``); no
        permutation is applied.  Refused (``ScilmmError``) on a distributed factor, with fp32 fronts, and after
        ``inverse_traces`` until the next ``refactorize``."""
        if getattr(self, "_pending", None) is not None:
            self.wait()
        return self._rhs(lib().scilmm_solve_L, b)

    def solve_Lt(self, b):
        """x with L^T x = b (rows in permuted order in, permuted order out); refusals as for ``solve_L``."""
        if getattr(self, "_pending", None) is not None:
            self.wait()
        return self._rhs(lib().scilmm_solve_Lt, b)

    def _rows(self, b):
        b = np.asarray(b)
        if b.ndim not in (1, 2) or b.shape[0] != self.n:
            raise ValueError("expected %d rows" % self.n)
        return b

    def apply_P(self, b):
        """b[P]: rows from the original order into the factor's permuted order."""
        return self._rows(b)[self.P()]

    def apply_Pt(self, b):
        """The inverse of ``apply_P``: out[P] = b."""
        b = self._rows(b)
        out = np.empty_like(b)
        out[self.P()] = b
        return out

    def solve_L_dev(self, dB_ptr, r, dX_ptr):
        """Device-pointer ``solve_L`` (row-major n x r, PERMUTED row order); enqueues without synchronising."""
        check(lib().scilmm_solve_L_dev(self._h, dB_ptr, r, dX_ptr), self.sym._h)

    def solve_Lt_dev(self, dB_ptr, r, dX_ptr):
        check(lib().scilmm_solve_Lt_dev(self._h, dB_ptr, r, dX_ptr), self.sym._h)

    def scan_block_dev(self, dG_ptr, ld, r, dQ_ptr, q, dstats_ptr):
        """One block of the marker scan (``scilmm_scan_block_dev``; ``scilmm_amd.assoc.AssociationScan`` is the interface)."""
        check(lib().scilmm_scan_block_dev(self._h, dG_ptr, ld, r, dQ_ptr, q, dstats_ptr), self.sym._h)

    def scan_block_bed_dev(self, dbed_ptr, ld, n_samples, dsample_ptr, flags, r, dQ_ptr, q, dstats_ptr):
        """One block of the marker scan from packed PLINK rows (``scilmm_scan_block_bed_dev``; ``dsample_ptr`` None = identity
        map; ``AssociationScan.scan_bed`` is the interface)."""
        check(lib().scilmm_scan_block_bed_dev(self._h, dbed_ptr, ld, n_samples, dsample_ptr, flags, r, dQ_ptr, q, dstats_ptr),
              self.sym._h)

    def scan_block_gram_dev(self, dG_ptr, ld, r, dQ_ptr, q, dstats_ptr, dgram_ptr):
        """``scan_block_dev`` with the r x r Gram matrix of the whitened markers as a second output
        (``scilmm_scan_block_gram_dev``; ``scilmm_amd.sets.VariantSetTest`` is the interface)."""
        check(lib().scilmm_scan_block_gram_dev(self._h, dG_ptr, ld, r, dQ_ptr, q, dstats_ptr, dgram_ptr), self.sym._h)

    def scan_block_bed_gram_dev(self, dbed_ptr, ld, n_samples, dsample_ptr, flags, r, dQ_ptr, q, dstats_ptr, dgram_ptr):
        """``scan_block_bed_dev`` with the Gram matrix as a second output (``scilmm_scan_block_bed_gram_dev``)."""
        check(lib().scilmm_scan_block_bed_gram_dev(self._h, dbed_ptr, ld, n_samples, dsample_ptr, flags, r, dQ_ptr, q, dstats_ptr,
                                                   dgram_ptr), self.sym._h)

    def scan_block_dosage_dev(self, ddos_ptr, dtype, ld, n_samples, dsample_ptr, r, dQ_ptr, q, dstats_ptr):
        """One block of the marker scan from dosage rows (``scilmm_scan_block_dosage_dev``; ``dtype``: ``_lib.DOSAGE_U16`` or
        ``_lib.DOSAGE_F32``, ``ld`` in elements, ``dsample_ptr`` None = identity map; ``AssociationScan.scan_dosages`` is the
        interface)."""
        check(lib().scilmm_scan_block_dosage_dev(self._h, ddos_ptr, dtype, ld, n_samples, dsample_ptr, r, dQ_ptr, q, dstats_ptr),
              self.sym._h)

    def scan_block_dosage_gram_dev(self, ddos_ptr, dtype, ld, n_samples, dsample_ptr, r, dQ_ptr, q, dstats_ptr, dgram_ptr):
        """``scan_block_dosage_dev`` with the Gram matrix as a second output (``scilmm_scan_block_dosage_gram_dev``)."""
        check(lib().scilmm_scan_block_dosage_gram_dev(self._h, ddos_ptr, dtype, ld, n_samples, dsample_ptr, r, dQ_ptr, q,
                                                      dstats_ptr, dgram_ptr), self.sym._h)

    def scan_block_gxe_dev(self, dG_ptr, ld, r, dE_ptr, m, dQ_ptr, q, dstats_ptr):
        """``scan_block_dev`` for ``r`` markers with ``m`` environment columns each (``scilmm_scan_block_gxe_dev``; ``dE_ptr``:
        n x m float64 in the permuted order of ``Q``; ``scilmm_amd.gxe.InteractionScan`` is the interface)."""
        check(lib().scilmm_scan_block_gxe_dev(self._h, dG_ptr, ld, r, dE_ptr, m, dQ_ptr, q, dstats_ptr), self.sym._h)

    def scan_block_bed_gxe_dev(self, dbed_ptr, ld, n_samples, dsample_ptr, flags, r, dE_ptr, m, dQ_ptr, q, dstats_ptr):
        """``scan_block_bed_dev`` with ``m`` environment columns (``scilmm_scan_block_bed_gxe_dev``)."""
        check(lib().scilmm_scan_block_bed_gxe_dev(self._h, dbed_ptr, ld, n_samples, dsample_ptr, flags, r, dE_ptr, m, dQ_ptr, q,
                                                  dstats_ptr), self.sym._h)

    def scan_block_dosage_gxe_dev(self, ddos_ptr, dtype, ld, n_samples, dsample_ptr, r, dE_ptr, m, dQ_ptr, q, dstats_ptr):
        """``scan_block_dosage_dev`` with ``m`` environment columns (``scilmm_scan_block_dosage_gxe_dev``)."""
        check(lib().scilmm_scan_block_dosage_gxe_dev(self._h, ddos_ptr, dtype, ld, n_samples, dsample_ptr, r, dE_ptr, m, dQ_ptr, q,
                                                     dstats_ptr), self.sym._h)

    def scan_panel_dev(self, r, dY_ptr, ld_y, t, dxty_ptr, ld_out):
        """``xty[j][k] = x_j . y_k`` (r x t, leading dimension ``ld_out``) for the ``r`` whitened columns the last scan block on
        this handle left behind and the ``t`` columns of the device panel ``dY_ptr`` (n x ``ld_y`` float64 in the permuted order
        of ``Q``, 16-byte aligned, ``ld_y`` a multiple of 16); enqueues without synchronising (``scilmm_scan_panel_dev``;
        ``scilmm_amd.panel.TraitPanel`` is the interface).  ``ScilmmError`` when no block was left behind or ``r`` is not its."""
        check(lib().scilmm_scan_panel_dev(self._h, r, dY_ptr, ld_y, t, dxty_ptr, ld_out), self.sym._h)

    def scan_block_keep_dev(self, r, ddst_ptr, ld_dst, col0):
        """Copy the ``r`` whitened columns the last scan block on this handle left behind (n x rp, rp = ``r`` rounded up to 16, the
        padding zero) into columns ``col0 .. col0 + rp - 1`` of the device store ``ddst_ptr`` (n x ``ld_dst`` float64, 16-byte
        aligned, ``ld_dst`` and ``col0`` multiples of 16), where ``scan_panel_dev`` reads them as its panel; enqueues without
        synchronising and leaves the block where it is (``scilmm_scan_block_keep_dev``; ``scilmm_amd.sets.VariantSetTest`` with
        ``max_markers`` is the interface).  ``ScilmmError`` when no block was left behind or ``r`` is not its."""
        check(lib().scilmm_scan_block_keep_dev(self._h, r, ddst_ptr, ld_dst, col0), self.sym._h)

    def scan_spa_dev(self, dG_ptr, ld, r, dstats_ptr, dR_ptr, du_ptr, dmu_ptr, dC_ptr, c, dMinv_ptr, cutoff, dspa_ptr):
        """The saddlepoint p-values of the ``r`` markers of the plain block queued before it (``scilmm_scan_spa_dev``: 7 x r
        numbers to ``dspa_ptr``; ``scilmm_amd.glmm.BinaryScan`` is the interface); enqueues without synchronising."""
        check(lib().scilmm_scan_spa_dev(self._h, dG_ptr, ld, r, dstats_ptr, dR_ptr, du_ptr, dmu_ptr, dC_ptr, c, dMinv_ptr, cutoff,
                                        dspa_ptr), self.sym._h)

    def sets_finish_dev(self, r, q, dstats_ptr, dgram_ptr, dR_ptr, du_ptr, c, n_sets, set_start, weight_mode, dweights_ptr, method, rho,
                        dout_ptr, ld_out, dlam_ptr):
        """Everything after a Gram block, one workgroup per set (``scilmm_sets_finish_dev``): ``set_start`` (host int32,
        ``n_sets + 1`` offsets into the block's columns) and ``rho`` (host float64, possibly empty: no SKAT-O) are read before the
        call returns; ``n_sets`` rows of ``10 + len(rho)`` doubles go to ``dout_ptr``; enqueues without synchronising
        (``scilmm_amd.sets.VariantSetTest`` with ``finish="device"`` is the interface)."""
        set_start = np.ascontiguousarray(set_start, dtype=np.int32)
        rho = np.ascontiguousarray(rho, dtype=np.float64)
        check(lib().scilmm_sets_finish_dev(self._h, r, q, dstats_ptr, dgram_ptr, dR_ptr, du_ptr, c, n_sets, ptr(set_start), weight_mode,
                                           dweights_ptr, method, ptr(rho), rho.size, dout_ptr, ld_out, dlam_ptr), self.sym._h)

    def sets_finish_wide_dev(self, k, block, q, dstats_ptr, dgram_ptr, dcross_ptr, ld_cross, dR_ptr, du_ptr, c, weight_mode, dweights_ptr,
                             method, rho, dout_ptr, dlam_ptr):
        """Everything after the sub-blocks of ONE set of ``k`` <= 4096 markers (``scilmm_sets_finish_wide_dev``): the sub-blocks'
        statistics at a stride of ``(q + 4) block`` doubles, their Gram blocks at a stride of ``block^2``, the rows of cross
        products (``None`` for a set of one sub-block); ``rho`` (host float64, possibly empty: no SKAT-O) is read before the call
        returns; one row of ``10 + len(rho)`` doubles goes to ``dout_ptr``; enqueues without synchronising
        (``scilmm_amd.sets.VariantSetTest`` with ``finish="wide"`` is the interface)."""
        rho = np.ascontiguousarray(rho, dtype=np.float64)
        check(lib().scilmm_sets_finish_wide_dev(self._h, k, block, q, dstats_ptr, dgram_ptr, dcross_ptr, ld_cross, dR_ptr, du_ptr, c,
                                                weight_mode, dweights_ptr, method, ptr(rho), rho.size, dout_ptr, dlam_ptr), self.sym._h)

    def sets_finish_panel_dev(self, r, q, dstats_ptr, dgram_ptr, dR_ptr, c, n_sets, set_start, weight_mode, dweights_ptr, method, rho,
                              dxty_ptr, ld_xty, t, dtscale_ptr, dhead_ptr, dout_ptr):
        """Everything after a Gram block and its ``scan_panel_dev``, for the block's sets against the ``t`` traits of the panel
        (``scilmm_sets_finish_panel_dev``): a set's spectra once, then a tail per trait from the scores ``dxty_ptr`` (r x ``t``,
        ``ld_xty`` apart).  ``set_start`` and ``rho`` as for ``sets_finish_dev``; ``dtscale_ptr``: ``t`` positive scales on the
        device, or None (all 1).  ``n_sets`` rows of 4 doubles (n_used, w'Kw, flags, 0) go to ``dhead_ptr`` and ``n_sets * t`` rows
        of 8 (1'(w o s), burden_chi2, skat_q, skat_p, skato_p, skato_pmin, skato_rho, flags; row = set * t + trait) to
        ``dout_ptr``; enqueues without synchronising (``scilmm_amd.set_panel.SetTraitPanel`` is the interface).  The traits of a tail
        workgroup are chosen by the engine; the environment variable ``SCILMM_SETS_PANEL_GROUP`` (1 .. 32), read per call, takes
        its place -- the numbers do not depend on it."""
        set_start = np.ascontiguousarray(set_start, dtype=np.int32)
        rho = np.ascontiguousarray(rho, dtype=np.float64)
        check(lib().scilmm_sets_finish_panel_dev(self._h, r, q, dstats_ptr, dgram_ptr, dR_ptr, c, n_sets, ptr(set_start), weight_mode,
                                                 dweights_ptr, method, ptr(rho), rho.size, dxty_ptr, ld_xty, t, dtscale_ptr, dhead_ptr,
                                                 dout_ptr), self.sym._h)

    def sets_finish_masks_dev(self, r, q, dstats_ptr, dgram_ptr, dR_ptr, du_ptr, c, n_sets, set_start, weight_mode, dweights_ptr, method,
                              rho, dann_ptr, n_ann, maf_cut, acat_mac, dout_ptr, ld_out):
        """Everything after a Gram block for the block's sets under ``n_ann`` annotation masks crossed with the MAF cutoffs
        ``maf_cut``, one workgroup per (set, annotation, cutoff) (``scilmm_sets_finish_masks_dev``).  ``set_start`` and ``rho`` as
        for ``sets_finish_dev``; ``dann_ptr``: ``r`` uint32 words on the device, bit a = the column is in annotation a;
        ``maf_cut`` (host float64, 1 .. 8 values in (0, 0.5]) is read before the call returns; ``acat_mac``: ACAT-V's pooling
        bound.  ``n_sets * n_ann * len(maf_cut)`` rows of ``12 + len(rho)`` doubles go to ``dout_ptr`` (row = (set n_ann + a)
        n_cut + f: the row of ``sets_finish_dev``, then acatv_p and n_pooled); enqueues without synchronising
        (``scilmm_amd.set_masks.MaskedSetTest`` is the interface)."""
        set_start = np.ascontiguousarray(set_start, dtype=np.int32)
        rho = np.ascontiguousarray(rho, dtype=np.float64)
        maf_cut = np.ascontiguousarray(maf_cut, dtype=np.float64)
        check(lib().scilmm_sets_finish_masks_dev(self._h, r, q, dstats_ptr, dgram_ptr, dR_ptr, du_ptr, c, n_sets, ptr(set_start),
                                                 weight_mode, dweights_ptr, method, ptr(rho), rho.size, dann_ptr, n_ann, ptr(maf_cut),
                                                 maf_cut.size, float(acat_mac), dout_ptr, ld_out), self.sym._h)

    def sets_finish_scaled_dev(self, r, q, dstats_ptr, dgram_ptr, dR_ptr, du_ptr, c, n_sets, set_start, weight_mode, dweights_ptr, method,
                               rho, dout_ptr, ld_out, dlam_ptr, dvscale_ptr):
        """``sets_finish_dev`` with the columns' variance scales ``dvscale_ptr`` (``r`` doubles, what ``sets_spa*_dev`` wrote) in
        the weights of ``A`` alone (``scilmm_sets_finish_scaled_dev``; ``scilmm_amd.glmm.BinarySetTest`` is the interface)."""
        set_start = np.ascontiguousarray(set_start, dtype=np.int32)
        rho = np.ascontiguousarray(rho, dtype=np.float64)
        check(lib().scilmm_sets_finish_scaled_dev(self._h, r, q, dstats_ptr, dgram_ptr, dR_ptr, du_ptr, c, n_sets, ptr(set_start),
                                                  weight_mode, dweights_ptr, method, ptr(rho), rho.size, dout_ptr, ld_out, dlam_ptr,
                                                  dvscale_ptr), self.sym._h)

    def _sets_spa(self, entry, head, r, dstats_ptr, dgram_ptr, dR_ptr, du_ptr, dmu_ptr, dC_ptr, c, dMinv_ptr, cutoff, dspa_ptr, n_sets,
                  set_start, weight_mode, dweights_ptr, dbspa_ptr, dvscale_ptr):
        set_start = np.ascontiguousarray(set_start, dtype=np.int32)
        check(entry(self._h, *(tuple(head) + (r, dstats_ptr, dgram_ptr, dR_ptr, du_ptr, dmu_ptr, dC_ptr, c, dMinv_ptr, cutoff, dspa_ptr,
                                             n_sets, ptr(set_start), weight_mode, dweights_ptr, dbspa_ptr, dvscale_ptr))), self.sym._h)

    def sets_spa_dev(self, dG_ptr, ld, r, *tail):
        """The sets' variance scales and burden saddlepoint rows behind a Gram block and its ``scan_spa_dev``
        (``scilmm_sets_spa_dev``).  ``tail``: ``dstats, dgram, dR, du, dmu, dC, c, dMinv, cutoff, dspa, n_sets, set_start`` (host
        int32 offsets), ``weight_mode, dweights, dbspa`` (``n_sets`` x 13 doubles out), ``dvscale`` (``r`` doubles out); enqueues
        without synchronising (``scilmm_amd.glmm.BinarySetTest`` is the interface)."""
        self._sets_spa(lib().scilmm_sets_spa_dev, (dG_ptr, ld), r, *tail)

    def sets_spa_bed_dev(self, dbed_ptr, ld, n_samples, dsample_ptr, flags, r, *tail):
        """``sets_spa_dev`` behind a block of packed PLINK rows (``scilmm_sets_spa_bed_dev``)."""
        self._sets_spa(lib().scilmm_sets_spa_bed_dev, (dbed_ptr, ld, n_samples, dsample_ptr, flags), r, *tail)

    def sets_spa_dosage_dev(self, ddos_ptr, dtype, ld, n_samples, dsample_ptr, r, *tail):
        """``sets_spa_dev`` behind a block of dosage rows (``scilmm_sets_spa_dosage_dev``)."""
        self._sets_spa(lib().scilmm_sets_spa_dosage_dev, (ddos_ptr, dtype, ld, n_samples, dsample_ptr), r, *tail)

    def sets_spa_timing(self):
        """``k_sets_spa`` of the last ``sets_spa*_dev`` on the handle in ms, after ``sync()`` (``Symbolic.sets_spa_timing``)."""
        return self.sym.sets_spa_timing()

    def sets_collapse_dev(self, dG_ptr, ld, r, dstats_ptr, weight_mode, dweights_ptr, first, dgB_ptr):
        """The collapsed genotype of a wide set grown by the kept markers of the sub-block queued before it
        (``scilmm_sets_collapse_dev``): ``dstats_ptr`` the sub-block's statistics, ``dweights_ptr`` its ``r`` weights (mode 2),
        ``first`` whether the row starts from zero, ``dgB_ptr`` n doubles; enqueues without synchronising
        (``scilmm_amd.glmm.BinaryWideSetTest`` is the interface)."""
        check(lib().scilmm_sets_collapse_dev(self._h, dG_ptr, ld, r, dstats_ptr, weight_mode, dweights_ptr, int(bool(first)), dgB_ptr),
              self.sym._h)

    def sets_collapse_bed_dev(self, dbed_ptr, ld, n_samples, dsample_ptr, flags, r, dstats_ptr, weight_mode, dweights_ptr, first, dgB_ptr):
        """``sets_collapse_dev`` behind a sub-block of packed PLINK rows (``scilmm_sets_collapse_bed_dev``)."""
        check(lib().scilmm_sets_collapse_bed_dev(self._h, dbed_ptr, ld, n_samples, dsample_ptr, flags, r, dstats_ptr, weight_mode,
                                                 dweights_ptr, int(bool(first)), dgB_ptr), self.sym._h)

    def sets_collapse_dosage_dev(self, ddos_ptr, dtype, ld, n_samples, dsample_ptr, r, dstats_ptr, weight_mode, dweights_ptr, first,
                                 dgB_ptr):
        """``sets_collapse_dev`` behind a sub-block of dosage rows (``scilmm_sets_collapse_dosage_dev``)."""
        check(lib().scilmm_sets_collapse_dosage_dev(self._h, ddos_ptr, dtype, ld, n_samples, dsample_ptr, r, dstats_ptr, weight_mode,
                                                    dweights_ptr, int(bool(first)), dgB_ptr), self.sym._h)

    def sets_spa_wide_dev(self, k, block, q, dstats_ptr, dgram_ptr, dcross_ptr, ld_cross, dR_ptr, du_ptr, dmu_ptr, dC_ptr, c, dMinv_ptr,
                          cutoff, dspa_ptr, weight_mode, dweights_ptr, dgB_ptr, dbspa_ptr, dvscale_ptr):
        """The variance scales (``k`` doubles to ``dvscale_ptr``) and the burden saddlepoint row (13 doubles to ``dbspa_ptr``) of ONE
        set of ``k`` <= 4096 markers behind its last sub-block (``scilmm_sets_spa_wide_dev``): the slices of
        ``sets_finish_wide_dev``, the markers' saddlepoint rows at a stride of ``7 block`` and the collapsed row ``dgB_ptr``;
        enqueues without synchronising."""
        check(lib().scilmm_sets_spa_wide_dev(self._h, k, block, q, dstats_ptr, dgram_ptr, dcross_ptr, ld_cross, dR_ptr, du_ptr, dmu_ptr,
                                             dC_ptr, c, dMinv_ptr, cutoff, dspa_ptr, weight_mode, dweights_ptr, dgB_ptr, dbspa_ptr,
                                             dvscale_ptr), self.sym._h)

    def sets_finish_wide_scaled_dev(self, k, block, q, dstats_ptr, dgram_ptr, dcross_ptr, ld_cross, dR_ptr, du_ptr, c, weight_mode,
                                    dweights_ptr, method, rho, dout_ptr, dlam_ptr, dvscale_ptr):
        """``sets_finish_wide_dev`` with the markers' variance scales ``dvscale_ptr`` (``k`` doubles, what ``sets_spa_wide_dev``
        wrote) in the weights of ``A`` alone (``scilmm_sets_finish_wide_scaled_dev``)."""
        rho = np.ascontiguousarray(rho, dtype=np.float64)
        check(lib().scilmm_sets_finish_wide_scaled_dev(self._h, k, block, q, dstats_ptr, dgram_ptr, dcross_ptr, ld_cross, dR_ptr, du_ptr,
                                                       c, weight_mode, dweights_ptr, method, ptr(rho), rho.size, dout_ptr, dlam_ptr,
                                                       dvscale_ptr), self.sym._h)

    def sets_spa_wide_timing(self):
        """``Symbolic.sets_spa_wide_timing`` of the handle."""
        return self.sym.sets_spa_wide_timing()

    def scan_spa_bed_dev(self, dbed_ptr, ld, n_samples, dsample_ptr, flags, r, dstats_ptr, dR_ptr, du_ptr, dmu_ptr, dC_ptr, c,
                         dMinv_ptr, cutoff, dspa_ptr):
        """``scan_spa_dev`` behind a block of packed PLINK rows (``scilmm_scan_spa_bed_dev``)."""
        check(lib().scilmm_scan_spa_bed_dev(self._h, dbed_ptr, ld, n_samples, dsample_ptr, flags, r, dstats_ptr, dR_ptr, du_ptr, dmu_ptr,
                                            dC_ptr, c, dMinv_ptr, cutoff, dspa_ptr), self.sym._h)

    def scan_spa_dosage_dev(self, ddos_ptr, dtype, ld, n_samples, dsample_ptr, r, dstats_ptr, dR_ptr, du_ptr, dmu_ptr, dC_ptr, c,
                            dMinv_ptr, cutoff, dspa_ptr):
        """``scan_spa_dev`` behind a block of dosage rows (``scilmm_scan_spa_dosage_dev``)."""
        check(lib().scilmm_scan_spa_dosage_dev(self._h, ddos_ptr, dtype, ld, n_samples, dsample_ptr, r, dstats_ptr, dR_ptr, du_ptr,
                                               dmu_ptr, dC_ptr, c, dMinv_ptr, cutoff, dspa_ptr), self.sym._h)

    def rel_block_dev(self, weights, ids, dQ_ptr, q, dstats_ptr):
        """One block of BLUP statistics for columns ``ids`` of ``sum_k weights[k] A_k`` (``scilmm_rel_block_dev``; host
        ``weights`` and ``ids``, device ``Q`` and statistics; ``scilmm_amd.blup.BLUP`` is the interface)."""
        w = np.ascontiguousarray(weights, dtype=np.float64)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        if w.shape != (self.sym.K,) or ids.ndim != 1:
            raise ValueError("weights must have one entry per matrix, ids must be 1-D")
        check(lib().scilmm_rel_block_dev(self._h, ptr(w), ptr(ids), ids.size, dQ_ptr, q, dstats_ptr), self.sym._h)

    def rows_block_dev(self, dindptr_ptr, dindices_ptr, ddata_ptr, r, dQ_ptr, q, dstats_ptr):
        """The same for ``r`` caller rows in CSR on the device (``scilmm_rows_block_dev``): int64 ``indptr``, int32
        ``indices`` in the matrices' row order, float64 ``data``."""
        check(lib().scilmm_rows_block_dev(self._h, dindptr_ptr, dindices_ptr, ddata_ptr, r, dQ_ptr, q, dstats_ptr), self.sym._h)

    def inverse_traces(self):
        """tr(V^-1 A_k) for every matrix of the analysis, exactly: the selected inverse on the supernodal factor (Takahashi
        recursion on the device, in place) followed by one pass over each A_k's pattern.  CONSUMES the factor: it must be
        refactorized before the next solve.  On a deterministic handle the inverse is summed in a fixed order (no
        floating-point atomics): the same factor gives the same bits, entries and traces."""
        self.selected_inverse()
        out = np.empty(self.sym.K)
        check(lib().scilmm_inverse_traces(self._h, ptr(out)), self.sym._h)
        return out

    def selected_inverse(self):
        """The selected inverse alone (``scilmm_selected_inverse``): every stored entry of the factor is replaced, in place, by
        the entry of ``(V[P][:, P])^-1`` at its position.  CONSUMES the factor like ``inverse_traces``, which is this call
        followed by the traces; ``inverse_pattern_dev`` / ``inverse_on_pattern`` read the entries on V's pattern."""
        if getattr(self, "_pending", None) is not None:
            self.wait()
        check(lib().scilmm_selected_inverse(self._h), self.sym._h)  # (a refusal leaves the factor, and its sigma2, as they were)
        self._s2, self._pending = None, None  # (the panels hold entries of the inverse from here on)
        return self

    def inverse_pattern_dev(self, ddiag_ptr, doff_ptr, alpha=1.0, ds_ptr=None, beta=0.0, dT_ptr=None, c=0):
        """``M = alpha diag(s) V^-1 diag(s) + beta T T'`` on V's pattern from an inverted factor (``scilmm_inverse_pattern_dev``):
        ``ddiag_ptr`` n doubles in the matrices' row order, ``doff_ptr`` one double per pattern slot (``Symbolic.get`` of
        ``pat_colptr`` / ``pat_row``), either None to skip it; ``ds_ptr`` (n, None = ones) and ``dT_ptr`` (n x c row-major,
        c <= 32) in the matrices' row order.  Device pointers; enqueues without synchronising; the factor stays inverted."""
        check(lib().scilmm_inverse_pattern_dev(self._h, float(alpha), ds_ptr, float(beta), dT_ptr, int(c), ddiag_ptr, doff_ptr),
              self.sym._h)

    def pattern_csr(self, off, diag=None):
        """The symmetric SciPy CSR, in the matrices' row order, of one value per pattern slot (``off``, the slot order of
        ``inverse_pattern_dev``); ``diag`` (row order) replaces the diagonal slots' values when given.  Needs the host copy of
        the pattern (``ScilmmError`` after ``release_host_maps``)."""
        sym, n = self.sym, self.n
        colptr, rows, P = sym.get("pat_colptr"), sym.get("pat_row"), self.P()
        if rows.size != colptr[-1]:
            raise _lib.ScilmmError("the host copy of the pattern was released (release_host_maps): no CSR can be built")
        off = np.asarray(off, dtype=np.float64)
        if off.shape != rows.shape:
            raise ValueError("one value per pattern slot is expected")
        i, j = P[np.repeat(np.arange(n), np.diff(colptr))], P[rows]
        lower = i != j
        d = off[colptr[:-1]] if diag is None else np.asarray(diag, dtype=np.float64)[P]
        M = sp.coo_matrix((np.concatenate([off[lower], off[lower], d]),
                           (np.concatenate([i[lower], j[lower], P]), np.concatenate([j[lower], i[lower], P]))), shape=(n, n)).tocsr()
        M.sort_indices()
        return M

    def inverse_on_pattern(self):
        """``(diag, M)``: the diagonal of ``V^-1`` (row order of the matrices) and the symmetric SciPy CSR of ``V^-1`` on V's
        pattern, both read off this factor after ``selected_inverse`` / ``inverse_traces`` (tests, and callers who want the
        entries; device buffers through torch)."""
        import torch
        vp = C.c_void_p
        dd = torch.empty((self.n,), dtype=torch.float64, device="cuda")
        do = torch.empty((max(1, int(self.sym.info().nnz_pattern)),), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        self.inverse_pattern_dev(vp(dd.data_ptr()), vp(do.data_ptr()))
        self.sym.sync()
        diag, off = dd.cpu().numpy(), do.cpu().numpy()[:int(self.sym.info().nnz_pattern)]
        return diag, self.pattern_csr(off, diag)

    def logdet(self):
        out = C.c_double(0.0)
        check(lib().scilmm_logdet(self._h, C.byref(out)), self.sym._h)
        return out.value

    def P(self):
        return self.sym.P()

    def L(self):
        nnz = C.c_int64(0)
        check(lib().scilmm_export_L(self._h, None, None, None, C.byref(nnz)), self.sym._h)
        colptr = np.empty(self.n + 1, np.int64)
        rowidx = np.empty(nnz.value, np.int32)
        vals = np.empty(nnz.value, np.float64)
        check(lib().scilmm_export_L(self._h, ptr(colptr), ptr(rowidx), ptr(vals), C.byref(nnz)), self.sym._h)
        return sp.csc_matrix((vals, rowidx, colptr), shape=(self.n, self.n))
