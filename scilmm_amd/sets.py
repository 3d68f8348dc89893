"""Variant-set tests (burden, SKAT in its family form famSKAT) with the variance components held fixed, on the resident factor.

For a set S of markers both tests need the score vector ``s = G~_S' P y`` and its null covariance ``K = G~_S' P G~_S``,
``P = V^-1 - V^-1 C (C' V^-1 C)^-1 C' V^-1``.  With the whitening ``w(b) = L^-1 P b`` of ``scilmm_amd.assoc`` and
``X = w(G~)``, ``Z = R^-T w(C)' X``::

    s = X' w(y) - Z' u          (the scan's numerator b, marker by marker)
    K = X' X - Z' Z

``X'X`` is the one thing the marker scan does not produce: ``scilmm_scan_block_gram_dev`` forms it from the forward
solution where it lies, on the fp64 matrix pipe, and hands back r x r numbers next to the scan's statistics.  Everything
after that is host algebra on at most 128 x 128 matrices.

    tester = VariantSetTest(cholesky_func, mats, sigma2, covariates, y)
    out = tester(genotypes, sets)                      # sets: a sequence of 1-D integer arrays of marker rows
    out = tester.test_bed("cohort", sets, sample_index=idx)
    out = tester.test_dosages(ds, sets, sample_index=idx)     # imputed dosages, uint16 codes or float32

Burden: ``beta = w's / w'Kw``, ``se = (w'Kw)^-1/2``, ``chi2 = (w's)^2 / w'Kw``, p from F(1, n - 1) as the scan's.  SKAT:
``Q = sum_j w_j^2 s_j^2``, null distribution ``sum_i lam_i chi2_1`` with ``lam`` the eigenvalues of ``diag(w) K diag(w)``
(Chen, Meigs, Dupuis 2013), tail probability by the saddlepoint approximation of Kuonen (1999) or by the modified Liu
moment matching of the SKAT package.  Davies' method and SKAT-O are not here: ``return_kernel=True`` hands out
``(s, K, w)`` per set for a caller who wants them.  There is no CPU form.
"""
import ctypes as C

import numpy as np
import scipy.linalg as la
import scipy.optimize as opt
import scipy.stats as stats

from .assoc import AssociationScan, check_genotypes
from .markers import Int8Rows

LAMBDA_FLOOR = 1e-10      # eigenvalues below this fraction of the largest are dropped from the mixture
SADDLE_SEAM = 0.05        # |q - mean| below this many standard deviations: the saddlepoint formula is singular, Liu instead
METHODS = ("saddlepoint", "liu")
KEYS = ("n_used", "burden_beta", "burden_se", "burden_chi2", "burden_p", "skat_q", "skat_p")


def _lam(lam):
    lam = np.asarray(lam, dtype=np.float64).ravel()
    return lam[lam > 0]


def mixture_sf_liu(q, lam):
    """P(sum_i lam_i chi2_1 > q) by the modified Liu moment matching (mean, variance, and kurtosis -- skewness as well where
    the two can be matched together), as the SKAT package does it.  Exact for equal ``lam``."""
    lam = _lam(lam)
    q = float(q)
    if np.isnan(q) or lam.size == 0:
        return np.nan
    c1, c2, c3, c4 = (float(np.sum(lam ** k)) for k in (1, 2, 3, 4))
    s1, s2 = c3 / c2 ** 1.5, c4 / (c2 * c2)
    # (equal lam give s1^2 == s2 in exact arithmetic: a difference of rounding size is not a skewness to match)
    if s1 * s1 > s2 * (1.0 + 1e-12):
        a = 1.0 / (s1 - np.sqrt(s1 * s1 - s2))
        d = s1 * a ** 3 - a * a
        l = a * a - 2.0 * d
    else:
        l = 1.0 / s2
        a = np.sqrt(l)
        d = 0.0
    x = (q - c1) / np.sqrt(2.0 * c2) * (np.sqrt(2.0) * a) + (l + d)
    if x <= 0:
        return 1.0
    return float(stats.chi2.sf(x, l) if d == 0.0 else stats.ncx2.sf(x, l, d))


def _lugannani_rice(q, lam):
    """The saddlepoint formula proper, for 0 < q away from the mean."""
    mu = float(lam.sum())
    hi = 0.5 / float(lam.max())                   # K is finite on t < hi

    def k1(t):
        return float(np.sum(lam / (1.0 - 2.0 * lam * t))) - q

    if q > mu:
        # K'(hi (1 - e)) >= lam_max / e: twice q at e = lam_max / (2 q)
        a, b = 0.0, hi * (1.0 - min(0.5, float(lam.max()) / (2.0 * q)))
    else:
        a, b = -hi, 0.0
        while k1(a) > 0:
            a *= 2.0
    t = opt.brentq(k1, a, b, xtol=1e-15 * hi, rtol=8.9e-16, maxiter=500)
    den = 1.0 - 2.0 * lam * t
    K0 = -0.5 * float(np.sum(np.log(den)))
    K2 = 2.0 * float(np.sum((lam / den) ** 2))
    w = np.sign(t) * np.sqrt(2.0 * (t * q - K0))
    v = t * np.sqrt(K2)
    return float(stats.norm.sf(w + np.log(v / w) / w))


def mixture_sf_saddlepoint(q, lam):
    """P(sum_i lam_i chi2_1 > q) by the Lugannani-Rice saddlepoint formula (Kuonen 1999): with the cumulant generating
    function ``K(t) = -1/2 sum log(1 - 2 lam_i t)`` and ``K'(t^) = q``, ``w = sign(t^) sqrt(2 (t^ q - K(t^)))``,
    ``v = t^ sqrt(K''(t^))``, the tail is ``1 - Phi(w + log(v / w) / w)``.  Within ``SADDLE_SEAM`` standard deviations of the
    mean, where ``t^ -> 0`` and the formula is 0 / 0, the moment-matching form answers instead: ``mixture_sf_liu(q)`` times a
    factor that goes linearly from saddlepoint / Liu at one end of that interval to saddlepoint / Liu at the other, so the
    function is continuous at both ends and decreasing across them (the two approximations differ by a per cent or so
    there; a bare switch would step UP by that much at the upper end)."""
    lam = _lam(lam)
    q = float(q)
    if np.isnan(q) or lam.size == 0:
        return np.nan
    if q <= 0:
        return 1.0
    mu, sd = float(lam.sum()), float(np.sqrt(2.0 * np.sum(lam * lam)))
    if abs(q - mu) >= SADDLE_SEAM * sd:
        return _lugannani_rice(q, lam)
    lo, hi = mu - SADDLE_SEAM * sd, mu + SADDLE_SEAM * sd     # (lo > 0: sd <= sqrt(2) mu)
    c_lo = _lugannani_rice(lo, lam) / mixture_sf_liu(lo, lam)
    c_hi = _lugannani_rice(hi, lam) / mixture_sf_liu(hi, lam)
    return mixture_sf_liu(q, lam) * (c_lo + (c_hi - c_lo) * (q - lo) / (hi - lo))


_MIXTURE = {"saddlepoint": mixture_sf_saddlepoint, "liu": mixture_sf_liu}


def check_sets(sets, m, block):
    """``sets`` as a list of int64 index arrays into ``0 .. m-1``: each 1-D, integer, 1 .. ``block`` distinct markers."""
    if isinstance(sets, np.ndarray) and sets.dtype != object and sets.ndim != 2:
        raise ValueError("sets must be a sequence of 1-D integer arrays, one per set")
    out = []
    for i, s in enumerate(sets):
        idx = np.asarray(s)
        if idx.ndim != 1 or idx.size == 0 or idx.dtype.kind not in "iu":
            raise ValueError("set %d must be a non-empty 1-D integer array" % i)
        idx = idx.astype(np.int64)
        if idx.min() < 0 or idx.max() >= m:
            raise ValueError("set %d holds a marker index outside 0 .. %d" % (i, m - 1))
        if np.unique(idx).size != idx.size:
            raise ValueError("set %d holds a marker twice" % i)
        if idx.size > block:
            raise ValueError("set %d has %d markers, more than one device block of %d: sets wider than a block are not "
                             "supported" % (i, idx.size, block))
        out.append(idx)
    return out


def check_weights(weights, sets):
    """``weights`` as "beta", None, or a list of float64 arrays aligned with ``sets`` (finite, one weight per marker)."""
    if weights is None or (isinstance(weights, str) and weights == "beta"):
        return weights
    if isinstance(weights, str):
        raise ValueError('weights must be "beta", None or a sequence of arrays aligned with sets, got %r' % (weights,))
    weights = list(weights)
    if len(weights) != len(sets):
        raise ValueError("%d weight arrays for %d sets" % (len(weights), len(sets)))
    out = []
    for i, (w, s) in enumerate(zip(weights, sets)):
        w = np.asarray(w, dtype=np.float64)
        if w.shape != s.shape or not np.all(np.isfinite(w)):
            raise ValueError("the weights of set %d must be %d finite numbers" % (i, s.size))
        out.append(w)
    return out


def check_method(method):
    if method not in METHODS:
        raise ValueError("method must be one of %s, got %r" % (", ".join(METHODS), method))
    return _MIXTURE[method]


def pack_sets(sizes, block):
    """Greedy packing, in the order given, of sets of ``sizes`` markers into device blocks of at most ``block`` markers: a
    list of lists of set numbers, one list per block.  A set never straddles two blocks."""
    blocks, used = [], 0
    for i, k in enumerate(sizes):
        k = int(k)
        if not 1 <= k <= block:
            raise ValueError("set %d has %d markers: a set holds 1 .. %d (one device block)" % (i, k, block))
        if not blocks or used + k > block:
            blocks.append([])
            used = 0
        blocks[-1].append(i)
        used += k
    return blocks


class VariantSetTest(AssociationScan):
    """Burden and SKAT tests of marker sets next to ``covariates`` under V = sum_k sigma2[k] mats[k].  The constructor is
    ``AssociationScan``'s; ``block`` bounds the markers of a set as well as of a device block."""

    def __call__(self, genotypes, sets, weights="beta", method="saddlepoint", return_kernel=False):
        """``genotypes``: m x n int8 as ``AssociationScan`` takes them; ``sets``: a sequence of 1-D integer arrays, the marker
        rows of each set (1 .. ``block`` distinct rows; a marker may belong to several sets); ``weights``: "beta" =
        Beta(1, 25) density at the marker's minor allele frequency, None = ones, or a sequence of arrays aligned with
        ``sets``; ``method``: "saddlepoint" or "liu" for ``skat_p``.  Returns a dict of length-``len(sets)`` arrays ``n_used``,
        ``burden_beta``, ``burden_se``, ``burden_chi2``, ``burden_p``, ``skat_q``, ``skat_p``; with ``return_kernel`` also
        ``kernel``, a list of ``(s, K, w)`` per set.  A marker without an observed value or without variation is dropped
        from its set (``n_used`` counts the rest); a set with nothing left gets NaN."""
        return self._run(Int8Rows(self, check_genotypes(genotypes, self.n)), sets, weights, method, return_kernel)

    def test_bed(self, bed, sets, sample_index=None, count="A1", chunk_bytes=None, weights="beta", method="saddlepoint",
                 return_kernel=False):
        """``__call__`` on the markers of a PLINK 1 fileset, decoded on the device (``scilmm_scan_block_bed_gram_dev``):
        ``sets`` index the file's markers; ``bed``, ``sample_index`` and ``count`` as for ``AssociationScan.scan_bed``.  A
        block's packed rows are uploaded as they lie in the file, so ``chunk_bytes`` has nothing to bound and is accepted
        for symmetry only.  Returns the bits of ``__call__`` on ``bed.read(None, sample_index, count)`` in deterministic
        mode."""
        src = self._bed_source(bed, sample_index, count)
        if chunk_bytes is not None and int(chunk_bytes) < 1:
            raise ValueError("chunk_bytes must be positive")
        return self._run(src, sets, weights, method, return_kernel)

    def test_dosages(self, dosages, sets, sample_index=None, weights="beta", method="saddlepoint", return_kernel=False):
        """``__call__`` on imputed dosages (``scilmm_scan_block_dosage_gram_dev``): ``sets`` index the rows of ``dosages``;
        ``dosages`` and ``sample_index`` as for ``AssociationScan.scan_dosages``.  The "beta" weights take half the mean
        dosage for the allele frequency.  For uint16 codes of hard calls it returns the bits of ``__call__`` on the int8
        markers in deterministic mode."""
        return self._run(self._dosage_source(dosages, sample_index), sets, weights, method, return_kernel)

    def _block(self, src):
        """rows -> ((q + 4) x r statistics, r x r Gram matrix) of one block of the marker source ``src``, on the host: the rows
        are brought to the device, one call of the form's Gram entry point, one wait, two device-to-host copies."""
        torch, q, blk = self.torch, self.q, self.block
        src.stage(blk)
        dS = torch.empty(((q + 4) * blk,), dtype=torch.float64, device="cuda")
        dK = torch.empty((blk * blk,), dtype=torch.float64, device="cuda")

        def run(rows):
            rb = rows.size
            src.load(rows)
            src.enqueue(0, rb, C.c_void_p(dS.data_ptr()), C.c_void_p(dK.data_ptr()))
            self.sym.sync()
            return dS[:(q + 4) * rb].cpu().numpy().reshape(q + 4, rb), dK[:rb * rb].cpu().numpy().reshape(rb, rb)
        return run

    def _run(self, src, sets, weights, method, return_kernel):
        """The checks of the sets (before any launch), then block by block: gather the block's marker rows, one device call, the
        statistics and the Gram matrix (``_block``), the host algebra set by set."""
        sets = check_sets(sets, src.m, self.block)
        weights, sf = check_weights(weights, sets), check_method(method)
        self._check_factor()
        block = self._block(src) if sets else None
        ns = len(sets)
        out = {k: np.full(ns, np.nan) for k in KEYS}
        out["n_used"] = np.zeros(ns, dtype=np.int64)
        kernel = [None] * ns
        for members in pack_sets([s.size for s in sets], self.block):
            S, G = block(np.concatenate([sets[i] for i in members]))
            a = 0
            for i in members:
                b = a + sets[i].size
                w = weights if weights is None or isinstance(weights, str) else weights[i]
                kernel[i] = self._one_set(out, i, S[:, a:b], G[a:b, a:b], w, sf)
                a = b
        if return_kernel:
            out["kernel"] = kernel
        return out

    def _one_set(self, out, i, S, G, weights, sf):
        """The host algebra of set ``i`` on its columns of the statistics and its sub-block of X'X; returns (s, K, w)."""
        c = self.c
        n_obs, mean, css = S[0], S[1], S[2]
        keep = ~((n_obs == 0) | (css == 0))
        z = la.solve_triangular(self.R, S[4:4 + c], trans='T', lower=False)[:, keep]
        s = S[4 + c][keep] - self.u.dot(z)
        K = G[np.ix_(keep, keep)] - z.T.dot(z)
        K = 0.5 * (K + K.T)
        if weights is None:
            w = np.ones(s.size)
        elif isinstance(weights, str):
            maf = np.minimum(0.5 * mean[keep], 1.0 - 0.5 * mean[keep])
            w = stats.beta.pdf(maf, 1, 25)
        else:
            w = weights[keep]
        out["n_used"][i] = k = int(keep.sum())
        if k:
            ws, wKw = float(w.dot(s)), float(w.dot(K.dot(w)))
            with np.errstate(divide="ignore", invalid="ignore"):
                out["burden_beta"][i] = ws / wKw
                out["burden_se"][i] = 1.0 / np.sqrt(wKw)
                out["burden_chi2"][i] = chi2 = ws * ws / wKw
            out["burden_p"][i] = self._f.sf(chi2)
            out["skat_q"][i] = qs = float(np.sum(w * w * s * s))
            lam = la.eigvalsh(w[:, None] * K * w[None, :])
            if lam.size and lam.max() > 0:
                out["skat_p"][i] = sf(qs, lam[lam > LAMBDA_FLOOR * lam.max()])
        return s, K, w
