"""Marker association scan with the variance components held fixed (EMMAX / P3D form) on the resident factor.

With ``w(b) = L^-1 P b`` (``L L^T = V[P][:, P]``), GLS of ``y`` on ``[C, g]`` under ``V`` is OLS of ``w(y)`` on
``[w(C), w(g)]``::

    g' V^-1 g = |w(g)|^2        g' V^-1 y = w(g)' w(y)        C' V^-1 g = w(C)' w(g)

so a marker costs the forward half of a solve and a column reduction.  ``AssociationScan`` whitens ``[C | y]`` once
(``Factor.solve_L_dev``) and then streams blocks of int8 markers through ``scilmm_scan_block_dev``: moments, dequantise +
centre + permute, one forward sweep, column statistics -- the n x r block never leaves HBM and only ``(q + 4)`` numbers per
marker come back.  The reference stops at the Wald tests of its covariates (scilmm/Estimation/LMM.py:129-133); the p-value
convention here is the same F(1, n - 1).

    scan = AssociationScan(cholesky_func, mats, sigma2, covariates, y)
    out = scan(genotypes)          # m x n int8, marker-major; dict of length-m arrays
    out = scan.scan_bed("cohort", sample_index=idx)   # PLINK 1 .bed / .bim / .fam, 2-bit genotypes decoded on the device
    out = scan.scan_dosages(ds, sample_index=idx)     # imputed dosages: m x N uint16 codes or float32 (scilmm_amd.dosage)
    gxe = scan.interaction(env)    # marker x environment interaction on the same factor and whitening (scilmm_amd.gxe)
    panel = scan.traits(Y)         # many traits, or scan.null_panel(...): simulated null phenotypes (scilmm_amd.panel)

There is no CPU form: without a GPU or the built library the constructor raises ``ScilmmError``.
"""
import ctypes as C
import time

import numpy as np
import scipy.linalg as la
import scipy.stats as stats

from . import _lib
from .markers import BedRows, DosageRows, Int8Rows, as_run

RPMAX = 128   # markers per device block at most (csrc/plan_types.h)
QMAX = 32     # columns of [w(C) | w(y)] at most (csrc/scan.hip.h)
# Width of a device block when the caller does not choose: one full chain window (112) or the sweeps' RPMAX (128),
# whichever gives more markers per second in profiles/assoc_scan_100k.json (tools/assoc_timing.py).
DEFAULT_BLOCK = 128
_CHUNK_BYTES = 64 << 20   # genotypes on the device at a time (whole blocks)


def check_genotypes(genotypes, n):
    """The genotype matrix as the device path takes it: m x n int8, marker-major, C-contiguous (``np.memmap`` included),
    columns in the row order of ``mats``.  TypeError for another dtype, ValueError for another shape or layout; nothing is
    converted or copied here."""
    g = genotypes
    if not isinstance(g, np.ndarray):
        raise TypeError("genotypes must be a NumPy int8 array (np.memmap included), got %s" % type(g).__name__)
    if g.dtype != np.int8:
        raise TypeError("genotypes must be int8 allele counts (negative = missing), got %s" % g.dtype)
    if g.ndim != 2:
        raise ValueError("genotypes must be 2-D, markers x individuals; got %d-D" % g.ndim)
    if g.shape[1] != n:
        raise ValueError("genotypes have %d columns, the model has %d individuals" % (g.shape[1], n))
    if not g.flags.c_contiguous:
        raise ValueError("genotypes must be C-contiguous (marker-major)")
    return g


class WhitenedModel(object):
    """What the marker scan and the BLUP share: the resident factor of ``(mats, sigma2)``, obtained or re-used through
    ``_final_factor``, and ``Q = L^-1 P [C | y]`` whitened once and kept in HBM, with ``R'R = w(C)'w(C)`` and
    ``u = R^-T w(C)'w(y)`` on the host.  An object is tied to that factor and refuses to run (``_check_factor``) once the
    factor has been refactorized at other values."""

    def __init__(self, cholesky_func, mats, sigma2, covariates, y, block=None):
        from .SparseCholesky import SparseCholesky, _device_buffers, _final_factor
        who = type(self).__name__
        if block is None:
            block = DEFAULT_BLOCK
        if not (isinstance(block, (int, np.integer)) and 1 <= block <= RPMAX):
            raise ValueError("block must be an integer in 1..%d" % RPMAX)
        covariates = np.asarray(covariates, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64).ravel()
        if covariates.ndim != 2 or covariates.shape[0] != y.size:
            raise ValueError("covariates must be n x c with one row per entry of y")
        c = covariates.shape[1]
        if not 1 <= c + 1 <= QMAX:
            raise ValueError("at most %d covariates" % (QMAX - 1))
        if not isinstance(cholesky_func, SparseCholesky):
            raise _lib.ScilmmError("%s needs the device engine (a scilmm_amd.SparseCholesky): there is no CPU form" % who)
        _lib.lib()
        torch = _device_buffers()
        if torch is None:
            raise _lib.ScilmmError("%s needs a GPU that torch can reach (device buffers): there is no CPU form" % who)
        self.torch, self.block, self.c, self.q = torch, int(block), c, c + 1
        self.factor = fac = _final_factor(cholesky_func, mats, np.asarray(sigma2, dtype=np.float64))
        self.sym = sym = fac.sym
        self.n = n = sym.n
        if y.size != n:
            raise ValueError("y has %d entries, the matrices %d rows" % (y.size, n))
        self._s2 = np.array(sigma2, dtype=np.float64)
        self.covariates = covariates
        # Q = L^-1 P [C | y]: one forward sweep, kept in HBM in the permuted order the scan kernels read
        perm = torch.from_numpy(fac.P()).cuda()
        dB = torch.from_numpy(np.ascontiguousarray(np.hstack([covariates, y[:, None]]))).cuda()[perm].contiguous()
        self.dQ = torch.empty_like(dB)
        torch.cuda.synchronize()
        fac.solve_L_dev(C.c_void_p(dB.data_ptr()), self.q, C.c_void_p(self.dQ.data_ptr()))
        sym.sync()
        G = (self.dQ.T @ self.dQ).cpu().numpy()              # [w(C) | w(y)]' [w(C) | w(y)]: (c + 1) x (c + 1)
        self.R = la.cholesky(G[:c, :c], lower=False)         # R' R = w(C)' w(C)
        self.u = la.solve_triangular(self.R, G[:c, c], trans='T', lower=False)   # R^-T w(C)' w(y)

    def _check_factor(self):
        if not self.factor.holds(self._s2):
            raise _lib.ScilmmError("the resident factor no longer holds the sigma2 this object was whitened with: build a new "
                                   "%s" % type(self).__name__)

    def _stats_buffer(self, nrows, m, blk=None):
        """Device buffer for the ``nrows`` statistics of ``m`` columns: a row of ``nrows * blk`` numbers per block of ``blk``
        columns (default: ``block``)."""
        blk = self.block if blk is None else blk
        return self.torch.empty(((m + blk - 1) // blk, nrows * blk), dtype=self.torch.float64, device="cuda")

    def _run_blocks(self, dS, out, enqueue, blk=None, after=None):
        """Fills ``out`` (nrows x m, m columns staged on the device) through ``dS``: ``enqueue(k0, rb, stats_ptr)`` queues the
        block of columns k0 .. k0 + rb - 1 (``blk`` columns per block, default ``block``), ``after(k0, rb)``, if given, what
        follows it on the block it leaves behind (``scilmm_amd.panel``); every block is queued, then one wait and one
        device-to-host copy."""
        (nrows, m), blk = out.shape, self.block if blk is None else blk
        for b, k0 in enumerate(range(0, m, blk)):
            enqueue(k0, min(blk, m - k0), C.c_void_p(dS.data_ptr() + 8 * b * nrows * blk))
            if after is not None:
                after(k0, min(blk, m - k0))
        self.sym.sync()
        hS = dS.cpu().numpy()
        for b, k0 in enumerate(range(0, m, blk)):
            rb = min(blk, m - k0)
            out[:, k0:k0 + rb] = hS[b, :nrows * rb].reshape(nrows, rb)


class AssociationScan(WhitenedModel):
    """Tests many candidate fixed effects next to ``covariates`` under V = sum_k sigma2[k] mats[k].

    ``cholesky_func``: a ``SparseCholesky``; ``mats``: every matrix of V (the identity included), as ``_final_factor`` takes
    them; ``sigma2``: one coefficient per matrix; ``covariates``: n x c (an intercept column is the caller's); ``y``: n.
    ``block``: markers per device block, 1..128.  The resident factor of ``(mats, sigma2)`` is obtained or re-used; a scan
    object is tied to it and refuses to run once the factor has been refactorized at other values (build a new one)."""

    def __init__(self, cholesky_func, mats, sigma2, covariates, y, block=None):
        super(AssociationScan, self).__init__(cholesky_func, mats, sigma2, covariates, y, block)
        self._f = stats.f(1, self.n - 1)

    def _stats(self, src, rows, chunk_bytes, nrows=None, blk=None, env=None, follow=None, rows_max=None):
        """nrows x m statistics (default: the scan's q + 4) of the markers ``rows`` (a slice or an index array) of the marker
        source ``src`` (``scilmm_amd.markers``), ``blk`` markers per device block (default ``block``), in chunks of whole
        blocks of at most ``chunk_bytes`` host bytes: a chunk is brought to the device, its blocks are queued, one wait.  The
        buffers are allocated once, for the largest chunk.  ``env``: the source's third twin (``scilmm_amd.gxe``).  ``follow``:
        a per-block follow-up (``scilmm_amd.panel``) -- ``stage(rows)`` once, ``block(k0, rb)`` behind every block of a chunk,
        ``chunk(j0, mc, dS, nrows, blk)`` when the chunk has been waited for; ``rows_max``: markers per chunk at most (whole
        blocks, at least one: what the follow-up keeps per chunk is bounded too)."""
        nrows = self.q + 4 if nrows is None else nrows
        blk = self.block if blk is None else blk
        run = isinstance(rows, slice)
        m = rows.stop - rows.start if run else rows.size
        out = np.empty((nrows, m))
        if m == 0:
            return out
        per = max(blk, min(m, max(1, chunk_bytes // src.row_bytes)) // blk * blk)
        if rows_max is not None:
            per = min(per, max(blk, rows_max // blk * blk))
        dS = self._stats_buffer(nrows, min(per, m), blk)
        src.stage(min(per, m))
        if follow is not None:
            follow.stage(min(per, m))
        enqueue = src.enqueue if env is None else (lambda k0, rb, pS: src.enqueue(k0, rb, pS, env=env))
        for j0 in range(0, m, per):
            mc = min(per, m - j0)
            src.load(slice(rows.start + j0, rows.start + j0 + mc) if run else rows[j0:j0 + mc])
            self._run_blocks(dS, out[:, j0:j0 + mc], enqueue, blk, None if follow is None else follow.block)
            if follow is not None:
                follow.chunk(j0, mc, dS, nrows, blk)
        return out

    def __call__(self, genotypes):
        """``genotypes``: m x n int8, marker-major, C-contiguous (0 / 1 / 2 allele counts, negative = missing; missing values
        are mean-imputed).  Returns a dict of length-m arrays ``beta``, ``se``, ``chi2``, ``p``, ``n_obs``, ``mean``; a
        marker without an observed value or without variation gets NaN in the first four."""
        g = check_genotypes(genotypes, self.n)
        self._check_factor()
        return self._finish(self._stats(Int8Rows(self, g), slice(0, g.shape[0]), _CHUNK_BYTES))

    def _finish(self, S):
        """The host algebra on the (q + 4) x m statistics of either block entry point: the dict ``__call__`` returns."""
        m, c = S.shape[1], self.c
        n_obs, mean, css, gg = S[0], S[1].copy(), S[2], S[3]
        z = la.solve_triangular(self.R, S[4:4 + c], trans='T', lower=False) if m else np.empty((c, 0))
        with np.errstate(divide="ignore", invalid="ignore"):
            a = gg - np.sum(z * z, axis=0)
            b = S[4 + c] - self.u.dot(z)
            bad = (n_obs == 0) | (css == 0)
            a = np.where(bad, np.nan, a)
            beta, se, chi2 = b / a, 1.0 / np.sqrt(a), b * b / a
        mean[n_obs == 0] = np.nan
        return {"beta": beta, "se": se, "chi2": chi2, "p": self._f.sf(chi2), "n_obs": n_obs.astype(np.int64), "mean": mean}

    def interaction(self, env, require_main_effects=True):
        """The marker x environment interaction scan next to this one: an ``InteractionScan`` (``scilmm_amd.gxe``) on this
        scan's factor and whitening, for the n x m environment columns ``env``."""
        from .gxe import InteractionScan
        return InteractionScan(self, env, require_main_effects)

    def traits(self, Y, scale="fixed"):
        """A panel of T traits next to this scan: a ``TraitPanel`` (``scilmm_amd.panel``) on this scan's factor and whitening.
        ``Y``: n x T float64, finite, 1 <= T <= 4096, rows in the order of ``mats``; ``scale``: "fixed" (V as given) or "profile"
        (the variance ratios shared, the scale profiled per trait: EMMAX).  ``panel(genotypes)`` tests every marker against
        every trait for one forward sweep per block."""
        from .panel import TraitPanel
        return TraitPanel.from_traits(self, Y, scale)

    def null_panel(self, n_rep=1000, seed=0):
        """A panel of ``n_rep`` (1..4096) null phenotypes simulated under this scan's model, ``N(C beta, V)``: in whitened space
        ``z ~ N(0, I)`` drawn on the device from ``torch.Generator(device="cuda").manual_seed(seed)`` and projected off the
        whitened covariates -- no solve.  The same seed, device and torch version give the same panel bits.
        ``null(genotypes, reduce="max")`` gives the per-replicate maximum chi2 for ``panel_thresholds``."""
        from .panel import TraitPanel
        return TraitPanel.null(self, n_rep, seed)

    def scan_bed(self, bed, sample_index=None, markers=None, count="A1", chunk_bytes=None):
        """The scan of ``__call__`` on the markers of a PLINK 1 fileset, decoded on the device: the packed rows are uploaded
        as they lie in the file, in chunks of whole blocks (``chunk_bytes``, default ``_CHUNK_BYTES``), and every block runs
        through ``scilmm_scan_block_bed_dev``.  ``bed``: a ``scilmm_amd.bed.BedFile`` or a path; ``sample_index``: n integers,
        the file's sample of every individual in the row order of ``mats``, -1 = not genotyped (``BedFile.sample_index``), or
        None when the file holds exactly the n individuals in that order; ``markers``: None, a slice or a 1-D integer array;
        ``count``: the counted allele, "A1" or "A2".  Returns what ``__call__`` returns for the unpacked, gathered markers
        (``bed.read(markers, sample_index, count)``), bit for bit in deterministic mode."""
        from .bed import marker_indices
        src = self._bed_source(bed, sample_index, count)
        rows = marker_indices(markers, src.m)
        if chunk_bytes is None:
            chunk_bytes = _CHUNK_BYTES
        self._check_factor()
        S = self._stats(src, as_run(rows), int(chunk_bytes))
        if rows.size:
            self.bed_seconds = (src.t_read, src.t_copy, time.perf_counter() - src.t0)
        return self._finish(S)

    def _bed_source(self, bed, sample_index, count):
        """What ``scan_bed`` and ``VariantSetTest.test_bed`` check first, before any launch: ``bed`` as a ``BedFile``, the
        counted allele, the sample map or the refusal of a file of another size without one.  Returns the ``BedRows``."""
        from .bed import BedFile, count_flag
        if not isinstance(bed, BedFile):
            bed = BedFile(bed)
        flag = count_flag(count)
        if sample_index is None:
            if bed.n_samples != self.n:
                raise ValueError("the file has %d samples, the model %d individuals: give a sample_index"
                                 % (bed.n_samples, self.n))
            idx = None
        else:
            idx = bed.check_sample_index(sample_index, self.n)
        return BedRows(self, bed, idx, flag)

    def _dosage_source(self, dosages, sample_index):
        """The checks ``scan_dosages`` and ``VariantSetTest.test_dosages`` share, before any launch.  Returns the
        ``DosageRows``."""
        from .bed import check_sample_index
        from .dosage import check_dosages
        d = check_dosages(dosages, self.n if sample_index is None else None)
        idx = None
        if sample_index is not None:
            if d.shape[1] < 1:
                raise ValueError("dosages without samples")
            idx = check_sample_index(sample_index, d.shape[1], self.n, source="dosage matrix")
        return DosageRows(self, d, _lib.DOSAGE_U16 if d.dtype == np.uint16 else _lib.DOSAGE_F32, idx)

    def scan_dosages(self, dosages, sample_index=None, chunk_bytes=None):
        """The scan of ``__call__`` on imputed dosages: ``dosages`` is m x N, marker-major, C-contiguous (``np.memmap``
        included), uint16 codes (16384 = one allele, above 32768 = missing: ``scilmm_amd.dosage.encode``) or float32 values
        (non-finite = missing; any finite value is taken as it is, so a quantitative candidate covariate goes the same way).
        ``sample_index``: n integers, the column of every individual in the row order of ``mats``, -1 = not genotyped, or None
        when the columns are exactly the n individuals in that order.  Chunks of whole blocks (``chunk_bytes``, default
        ``_CHUNK_BYTES``) go through a pinned buffer to the device and every block through ``scilmm_scan_block_dosage_dev``.
        Returns the dict of ``__call__``; for uint16 codes of hard calls, bit for bit what ``__call__`` returns for the int8
        markers in deterministic mode."""
        src = self._dosage_source(dosages, sample_index)
        if chunk_bytes is None:
            chunk_bytes = _CHUNK_BYTES
        if int(chunk_bytes) < 1:
            raise ValueError("chunk_bytes must be positive")
        self._check_factor()
        return self._finish(self._stats(src, slice(0, src.m), int(chunk_bytes)))
