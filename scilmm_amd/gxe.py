"""Marker x environment interaction scan (G x E) on the resident factor, next to an ``AssociationScan``.

Does the allele's effect differ by sex, treatment, herd, age or diet?  Per marker, GLS of ``y`` on
``[C, g~, g~ o e_1 .. g~ o e_m]`` under ``V`` (``g~``: the centred marker, missing = 0; ``o``: the entry-wise product), where
the interaction columns differ from marker to marker and so cannot be covariates of the scan.  The scan's whitening identity
holds term by term: with ``x_a = w(g~ o e_a)``, ``x_0 = w(g~)``, the test is OLS on the whitened columns -- a marker costs
``d = 1 + m`` columns of the forward sweep the scan already runs and one symmetric ``d x d`` system on the host::

    Z = R^-T w(C)'X (c x d)      M = X'X - Z'Z      b = X'w(y) - Z'u      beta = M^-1 b      cov = M^-1

``scilmm_scan_block_gxe_dev`` and its ``.bed`` / dosage twins build the ``d r`` columns of a block on the device
(``k_scan_expand`` after the form's own fill) and hand back ``|x_a|^2``, ``Q'x_a`` and the cross products ``x_a'x_b``
(``k_scan_cross``): ``3 + (q + 1) d + d (d - 1) / 2`` numbers per marker.

    gxe = scan.interaction(env)             # env: n x m (or n), 1 <= m <= 3, its columns among the scan's covariates
    out = gxe(genotypes)                    # as AssociationScan.__call__; also gxe.scan_bed(...), gxe.scan_dosages(...)
    out["chi2_int"], out["p_int"]           # the m interaction terms together; "chi2_joint": all d terms of the marker

The interaction scan shares the scan's factor, ``dQ``, ``R`` and ``u``: no second whitening, no second factor.  There is no
CPU form.
"""
import numpy as np
import scipy.linalg as la
import scipy.stats as stats

from . import _lib, assoc
from .markers import Int8Rows, as_run, vp

MMAX = 3          # environment columns at most (csrc/scan.hip.h GXE_MMAX)
RCOND_MIN = 1e-10  # a marker whose unit-diagonal M has a smaller reciprocal condition number is not estimable


def stat_rows(q, d):
    """Rows of the statistics of ``scilmm_scan_block_gxe_dev``: 3 moments, (q + 1) quantities of d terms, d (d - 1) / 2 pairs."""
    return 3 + (q + 1) * d + d * (d - 1) // 2


def check_env(env, n, covariates, block, require_main_effects=True):
    """The environment columns as the device path takes them: n x m float64, C-contiguous (a vector is n x 1), 1 <= m <= 3,
    finite; ``block`` (the scan's columns per device block) holds at least the d = 1 + m columns of one marker; and, unless
    ``require_main_effects`` is False, every column lies in the column span of ``covariates`` (least-squares residual at most
    1e-8 |e|): an interaction without its main effect in the null model tests the wrong thing, and the centring of the
    interaction columns rests on it.  ValueError otherwise; nothing of a device is touched."""
    E = np.asarray(env, dtype=np.float64)
    if E.ndim == 1:
        E = E[:, None]
    if E.ndim != 2 or E.shape[0] != n:
        raise ValueError("env must be n x m with one row per individual (n = %d); got shape %s" % (n, np.shape(env)))
    m = E.shape[1]
    if not 1 <= m <= MMAX:
        raise ValueError("env must have 1..%d columns, got %d" % (MMAX, m))
    if not np.all(np.isfinite(E)):
        raise ValueError("env must be finite (a NaN or an infinity in it)")
    if block < 1 + m:
        raise ValueError("block = %d is narrower than the %d columns of one marker (1 + %d environment columns)" % (block, 1 + m, m))
    if require_main_effects:
        Cv = np.asarray(covariates, dtype=np.float64)
        res = E - Cv.dot(la.lstsq(Cv, E)[0])
        for a in range(m):
            if np.linalg.norm(res[:, a]) > 1e-8 * np.linalg.norm(E[:, a]):
                raise ValueError("env column %d is not in the column span of the scan's covariates: put the main effect into the "
                                 "null model (or pass require_main_effects=False)" % a)
    return np.ascontiguousarray(E)


def interaction_stats(S, d, R, u, n):
    """The host algebra on the ``stat_rows(q, d)`` x M statistics of the gxe entry points (layout: include/scilmm_hip.h),
    with the scan's ``R`` (R'R = w(C)'w(C), c x c) and ``u`` (R^-T w(C)'w(y)); q = c + 1, ``n`` individuals.  Returns the dict
    of ``InteractionScan.__call__``.  Pure NumPy: no device."""
    S = np.asarray(S, dtype=np.float64)
    M, c, m = S.shape[1], R.shape[0], d - 1
    q = c + 1
    if S.shape[0] != stat_rows(q, d):
        raise ValueError("statistics of %d rows, expected %d for q = %d, d = %d" % (S.shape[0], stat_rows(q, d), q, d))
    n_obs, mean, css = S[0], S[1].copy(), S[2]
    T = S[3:3 + (q + 1) * d].reshape(q + 1, d, M)            # T[k, a]: quantity k of term a
    Z = la.solve_triangular(R, T[1:1 + c].reshape(c, d * M), trans='T', lower=False).reshape(c, d, M) if M else np.empty((c, d, 0))
    XtX = np.empty((M, d, d))
    k = 3 + (q + 1) * d
    for a in range(d):
        XtX[:, a, a] = T[0, a]
        for b in range(a + 1, d):
            XtX[:, a, b] = XtX[:, b, a] = S[k]
            k += 1
    Mm = XtX - np.einsum("kam,kbm->mab", Z, Z)
    bv = (T[q] - np.einsum("k,kam->am", u, Z)).T             # M x d
    dg = np.einsum("maa->ma", Mm)
    bad = (n_obs == 0) | (css == 0) | ~np.all(dg > 0, axis=1)
    sc = 1.0 / np.sqrt(np.where(bad[:, None], 1.0, dg))
    Ms = np.where(bad[:, None, None], np.eye(d), Mm * sc[:, :, None] * sc[:, None, :])
    ev = np.linalg.eigvalsh(Ms)                               # ascending
    bad |= ~(ev[:, 0] >= RCOND_MIN * ev[:, -1])
    Ms[bad] = np.eye(d)
    cov = np.linalg.inv(Ms) * sc[:, :, None] * sc[:, None, :]
    beta = np.einsum("mab,mb->ma", cov, bv)
    chi2_joint = np.einsum("ma,ma->m", bv, beta)
    bI = beta[:, 1:]
    chi2_int = np.einsum("ma,ma->m", bI, np.linalg.solve(cov[:, 1:, 1:], bI[:, :, None])[:, :, 0])
    se = np.sqrt(np.einsum("maa->ma", cov))
    for v in (beta, se, cov, chi2_int, chi2_joint):
        v[bad] = np.nan
    mean[n_obs == 0] = np.nan
    return {"beta": beta, "se": se, "cov": cov,
            "chi2_int": chi2_int, "p_int": stats.f(m, n - 1).sf(chi2_int / m),
            "chi2_joint": chi2_joint, "p_joint": stats.f(d, n - 1).sf(chi2_joint / d),
            "n_obs": n_obs.astype(np.int64), "mean": mean}


class InteractionScan(object):
    """``scan.interaction(env)``: tests every marker with ``d = 1 + m`` terms, its own and its products with the ``m``
    columns of ``env``, next to the covariates of ``scan`` (an ``AssociationScan``, whose factor, whitened ``Q``, ``R`` and
    ``u`` it shares; it refuses to run when the scan does).  ``env``: n x m float64 (a vector is n x 1), 1 <= m <= 3, finite,
    every column in the span of the scan's covariates unless ``require_main_effects=False``.  A device block holds
    ``scan.block // d`` markers."""

    def __init__(self, scan, env, require_main_effects=True):
        if not isinstance(scan, assoc.AssociationScan):
            raise _lib.ScilmmError("InteractionScan needs an AssociationScan on the device engine: there is no CPU form")
        E = check_env(env, scan.n, scan.covariates, scan.block, require_main_effects)
        scan._check_factor()
        self.scan, self.n = scan, scan.n
        self.m, self.d = E.shape[1], 1 + E.shape[1]
        self.block = scan.block // self.d                     # markers per device block
        self.nrows = stat_rows(scan.q, self.d)
        torch = scan.torch
        perm = torch.from_numpy(scan.factor.P()).cuda()
        self.dE = torch.from_numpy(E).cuda()[perm].contiguous()    # the permuted order of dQ
        torch.cuda.synchronize()

    def _stats(self, src, rows, chunk_bytes):
        self.scan._check_factor()
        return self.scan._stats(src, rows, chunk_bytes, self.nrows, self.block, (vp(self.dE.data_ptr()), self.m))

    def _finish(self, S):
        return interaction_stats(S, self.d, self.scan.R, self.scan.u, self.n)

    def __call__(self, genotypes):
        """``genotypes`` as for ``AssociationScan.__call__``.  Returns a dict: ``beta``, ``se`` (M x d: the marker's own term,
        then the m interaction terms), ``cov`` (M x d x d), ``chi2_int`` / ``p_int`` (the m interaction terms together:
        beta_I' cov_II^-1 beta_I), ``chi2_joint`` / ``p_joint`` (all d terms: b'beta), ``n_obs``, ``mean``.  The p-values are
        F(k, n - 1).sf(chi2 / k), the scan's convention at k = 1.  A marker without an observed value, without variation,
        or whose d columns are collinear given the covariates (unit-diagonal M with a non-positive diagonal entry or a
        reciprocal condition number below 1e-10: a marker that varies in one level of a binary environment only) gets NaN in
        everything but ``n_obs`` and ``mean``."""
        g = assoc.check_genotypes(genotypes, self.n)
        return self._finish(self._stats(Int8Rows(self.scan, g), slice(0, g.shape[0]), assoc._CHUNK_BYTES))

    def scan_bed(self, bed, sample_index=None, markers=None, count="A1", chunk_bytes=None):
        """``__call__`` on the markers of a PLINK 1 fileset, decoded on the device (``scilmm_scan_block_bed_gxe_dev``); the
        arguments of ``AssociationScan.scan_bed``.  Bit for bit what ``__call__`` returns for the unpacked, gathered markers
        in deterministic mode."""
        from .bed import marker_indices
        src = self.scan._bed_source(bed, sample_index, count)
        rows = marker_indices(markers, src.m)
        return self._finish(self._stats(src, as_run(rows), int(assoc._CHUNK_BYTES if chunk_bytes is None else chunk_bytes)))

    def scan_dosages(self, dosages, sample_index=None, chunk_bytes=None):
        """``__call__`` on imputed dosages (``scilmm_scan_block_dosage_gxe_dev``); the arguments of
        ``AssociationScan.scan_dosages``."""
        src = self.scan._dosage_source(dosages, sample_index)
        chunk_bytes = int(assoc._CHUNK_BYTES if chunk_bytes is None else chunk_bytes)
        if chunk_bytes < 1:
            raise ValueError("chunk_bytes must be positive")
        return self._finish(self._stats(src, slice(0, src.m), chunk_bytes))
