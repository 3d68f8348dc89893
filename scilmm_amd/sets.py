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
moment matching of the SKAT package.  Davies' method is not here: ``return_kernel=True`` hands out ``(s, K, w)`` per set
for a caller who wants it.  There is no CPU form.

SKAT-O (Lee, Wu, Lin 2012; ``skato=True``): with ``t = w o s`` and ``A = diag(w) K diag(w)``, the statistic of the grid value
``rho`` is ``Q_rho = (1 - rho) t't + rho (1't)^2``, its null law the mixture with the eigenvalues of ``A R_rho``,
``R_rho = (1 - rho) I + rho 11'``; the test statistic is the smallest of their p-values, and its own p-value is a
one-dimensional integral over the component of the score along ``A 1`` (``skato_pvalue``, which needs ``(t, A)`` alone;
DESIGN.md section 19).

``finish="host"`` does everything after the Gram block in NumPy / SciPy, set by set.  ``finish="device"`` queues
``scilmm_sets_finish_dev`` behind the block instead: one workgroup per set does the projection, a Jacobi
eigendecomposition, the tails and the SKAT-O quadrature in LDS, and one copy of a few doubles per set comes back (``burden_p``
alone stays on the host).  The two agree to the accuracy of the tails (1e-6 relative), not bit for bit.

``max_markers=k`` lets a set hold up to k <= 4096 markers instead of one block's: such a set runs as sub-blocks whose forward
solutions are kept on the device (``scilmm_scan_block_keep_dev``) and whose cross products ``X_b' X_a`` come from
``scilmm_scan_panel_dev``; ``assemble_wide`` puts the k x k ``X'X`` together and the host algebra above takes over (DESIGN.md
section 21).  ``finish="wide"`` is ``finish="device"`` for the sets of one block, and for a wider set it leaves the pieces on the
device and queues ``scilmm_sets_finish_wide_dev`` behind the last sub-block: one tridiagonal reduction of ``A`` gives every
spectrum SKAT-O needs, and one row of numbers comes back.
"""
import ctypes as C

import numpy as np
import scipy.integrate as integ
import scipy.linalg as la
import scipy.optimize as opt
import scipy.special as special
import scipy.stats as stats

from .assoc import AssociationScan, check_genotypes
from .markers import Int8Rows

LAMBDA_FLOOR = 1e-10      # eigenvalues below this fraction of the largest are dropped from the mixture
SADDLE_SEAM = 0.05        # |q - mean| below this many standard deviations: the saddlepoint formula is singular, Liu instead
METHODS = ("saddlepoint", "liu")
KEYS = ("n_used", "burden_beta", "burden_se", "burden_chi2", "burden_p", "skat_q", "skat_p")
SKATO_KEYS = ("skato_p", "skato_pmin", "skato_rho", "skato_p_rho")
RHO_DEFAULT = (0.0, 0.01, 0.04, 0.09, 0.16, 0.25, 0.5, 1.0)
RHO_MAX, RHO_CAP = 16, 0.999      # grid values at most; a value above RHO_CAP is computed as RHO_CAP (R_rho stays definite)
Z_END = 40.0              # the SKAT-O integral stops here: 2 Phi(-40) is zero in double precision
FINISHES = ("host", "device")
FINISH_VALUES = FINISHES + ("wide",)     # what VariantSetTest takes: "wide" is the device finish that also takes a set wider than a block
WEIGHT_BETA, WEIGHT_ONES, WEIGHT_GIVEN = 0, 1, 2       # weight modes of scilmm_sets_finish_dev
FINISH_HEAD = 10          # doubles of a set's row before its per-rho p-values
WIDE_MAX = 4096           # markers of a set at most, with max_markers
PANEL_COLUMNS = 4096      # columns of a scan_panel_dev call at most: what the kept sub-blocks of a wide set may add up to


def _lam(lam):
    lam = np.asarray(lam, dtype=np.float64).ravel()
    return lam[lam > 0]


def liu_params(lam):
    """The modified Liu matching of ``sum_i lam_i chi2_1`` (``lam`` positive): ``(c1, c2, a, d, l)`` with ``c_k = sum lam^k`` (mean
    ``c1``, variance ``2 c2``), and the matched non-central chi-square's scale ``a``, non-centrality ``d`` and degrees of freedom
    ``l``."""
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
    return c1, c2, a, d, l


def mixture_sf_liu(q, lam):
    """P(sum_i lam_i chi2_1 > q) by the modified Liu moment matching (mean, variance, and kurtosis -- skewness as well where
    the two can be matched together), as the SKAT package does it.  Exact for equal ``lam``."""
    lam = _lam(lam)
    q = float(q)
    if np.isnan(q) or lam.size == 0:
        return np.nan
    c1, c2, a, d, l = liu_params(lam)
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


def check_rho(rho):
    """The SKAT-O grid as a float64 array: None = ``RHO_DEFAULT``, else 1 .. 16 values in [0, 1]."""
    rho = np.asarray(RHO_DEFAULT if rho is None else rho, dtype=np.float64).ravel()
    if not 1 <= rho.size <= RHO_MAX:
        raise ValueError("rho must hold 1 .. %d values, got %d" % (RHO_MAX, rho.size))
    if not np.all((rho >= 0.0) & (rho <= 1.0)):           # (a NaN fails both comparisons)
        raise ValueError("every rho must lie in [0, 1]")
    return rho


def _floor(lam, scale=0.0):
    """The eigenvalues above ``LAMBDA_FLOOR`` times the largest; none where the largest is not above ``scale``."""
    lam = np.asarray(lam, dtype=np.float64)
    if not lam.size or not lam.max() > scale:
        return lam[:0]
    return lam[lam > LAMBDA_FLOOR * lam.max()]


def skato_lines(T, lams, rho, tau):
    """The lines whose lower envelope is SKAT-O's ``delta(x) = min_rho (q_min(rho) - tau(rho) x) / (1 - rho)``: intercepts and
    slopes, with ``q_min(rho)`` the ``1 - T`` quantile of the modified Liu matching of the spectrum ``lams[rho]``."""
    al, be = np.empty(rho.size), np.empty(rho.size)
    for j, (r, lam) in enumerate(zip(rho, lams)):
        c1, c2, _, _, l = liu_params(lam)
        qmin = (stats.chi2.isf(T, l) - l) / np.sqrt(2.0 * l) * np.sqrt(2.0 * c2) + c1
        al[j], be[j] = qmin / (1.0 - r), tau[j] / (1.0 - r)
    return al, be


def skato_breaks(al, be, level):
    """``(z0, breaks)``: ``z0`` where the envelope of the lines ``al - be x`` (x = z^2) comes down to ``level`` (0 where it starts
    below), and the sorted ends of the pieces of [0, min(z0, Z_END)] between the pairwise intersections of the lines."""
    x0 = float(np.min((al - level) / be))
    if not x0 > 0.0:
        return 0.0, np.zeros(1)
    z0 = float(np.sqrt(x0))
    end = min(z0, Z_END)
    pts = [0.0, end]
    for i in range(al.size):
        for j in range(i + 1, al.size):
            if be[i] != be[j]:
                x = (al[i] - al[j]) / (be[i] - be[j])
                if x > 0.0 and np.sqrt(x) < end:
                    pts.append(float(np.sqrt(x)))
    return z0, np.unique(pts)


def skato_spectra(A, rho):
    """What ``skato_pvalue`` takes from ``A`` alone (r x r, symmetric; ``rho`` checked): ``(lams, lamB)``, the spectra above the
    floor of ``L_rho' A L_rho`` per grid value (capped at ``RHO_CAP``) and of ``B = A - a a' / s11`` (empty where the remainder term
    does not exist).  A caller with many score vectors against one ``A`` computes it once (``scilmm_amd.set_panel``)."""
    r = A.shape[0]
    lams, one = [], np.ones((r, r))
    for x in np.minimum(rho, RHO_CAP):
        if r == 1:
            lam = _floor(A.ravel())
        else:
            L = la.cholesky((1.0 - x) * np.eye(r) + x * one, lower=True)
            M = L.T.dot(A).dot(L)
            lam = _floor(la.eigvalsh(0.5 * (M + M.T)))
        lams.append(lam)
    tr = float(np.trace(A))
    a = A.sum(axis=1)
    s11 = float(a.sum())
    lamB = np.empty(0)
    if r > 1 and s11 > LAMBDA_FLOOR * tr:
        B = A - np.outer(a, a) / s11
        B = 0.5 * (B + B.T)
        lamB = _floor(la.eigvalsh(B), LAMBDA_FLOOR * tr)
    return lams, lamB


def skato_pvalue(t, A, rho=RHO_DEFAULT, method="saddlepoint", spectra=None):
    """SKAT-O from ``t = w o s`` and ``A = diag(w) K diag(w)`` (r x r, positive semidefinite): ``(p, pmin, rho_at_min, p_rho)``.

    Per grid value: ``Q_rho = (1 - rho) t't + rho (1't)^2`` against the mixture with the eigenvalues of ``L_rho' A L_rho``
    (``L_rho L_rho' = R_rho``; those below ``LAMBDA_FLOOR`` times the largest dropped) by ``method``; ``pmin = T`` is the smallest
    ``p_rho`` and ``rho_at_min`` the first grid value that attains it.  With ``a = A 1``, ``s11 = 1'A1`` and
    ``B = A - a a' / s11``, the part of ``Q_rho`` beside the component along ``a`` has mean ``sum lam_B``, variance
    ``2 sum lam_B^2 + 4 a'Ba / s11`` and ``df = (sum lam_B^2)^2 / sum lam_B^4``; ``tau(rho) = rho s11 + (1 - rho) a'a / s11``
    multiplies the chi2_1 of that component, and

        p = int_0^inf S_df((delta(z^2) - mu) / sigma sqrt(2 df) + df) 2 phi(z) dz,

    in survival form (the package's ``1 - int F`` cancels to nothing below 1e-12), integrated piece by piece between the kinks
    of ``delta`` and up to ``z0``, where the argument reaches 0 and the rest is ``2 Phi(-z0)``; then ``p <- min(p, n_rho T)``.
    A value of ``rho`` above 0.999 is computed as 0.999.  One marker, ``s11 <= LAMBDA_FLOOR trace(A)`` or no eigenvalue of ``B``
    above ``LAMBDA_FLOOR trace(A)`` (rank one: what is left of ``B`` is rounding): every ``p_rho`` is the same up to rounding,
    ``p = T`` and ``rho_at_min`` is the first grid value.  ``spectra``: None, or ``skato_spectra(A, rho)`` of the same ``A`` and
    ``rho``, computed once for many ``t``."""
    t = np.asarray(t, dtype=np.float64).ravel()
    A = np.asarray(A, dtype=np.float64).reshape(t.size, t.size)
    rho, sf = check_rho(rho), check_method(method)
    r, nr = t.size, rho.size
    rc = np.minimum(rho, RHO_CAP)
    tt, t1 = float(t.dot(t)), float(t.sum())
    p_rho = np.full(nr, np.nan)
    lams, lamB = skato_spectra(A, rho) if spectra is None else spectra
    for j, x in enumerate(rc):
        q, lam = tt if r == 1 else (1.0 - x) * tt + x * t1 * t1, lams[j]   # ((1 - rho) q + rho q is not q bit for bit)
        if lam.size:
            p_rho[j] = sf(q, lam)
    if np.any(np.isnan(p_rho)):
        return np.nan, np.nan, np.nan, p_rho
    j0 = int(np.argmin(p_rho))
    T = float(p_rho[j0])
    a = A.sum(axis=1)
    s11 = float(a.sum())
    if not lamB.size:                  # every p_rho is the same up to rounding: the first grid value stands for the minimiser
        return T, T, float(rho[0]), p_rho
    if T == 0.0:                       # (T has underflowed: so has p, and the quantile of 0 is infinite)
        return T, T, float(rho[j0]), p_rho
    B = A - np.outer(a, a) / s11
    B = 0.5 * (B + B.T)
    l2 = float(np.sum(lamB ** 2))
    mu, var, df = float(lamB.sum()), 2.0 * l2 + 4.0 * max(float(a.dot(B).dot(a)), 0.0) / s11, l2 * l2 / float(np.sum(lamB ** 4))
    sd = np.sqrt(var)
    al, be = skato_lines(T, lams, rc, rc * s11 + (1.0 - rc) * float(a.dot(a)) / s11)
    z0, pts = skato_breaks(al, be, mu - sd * np.sqrt(0.5 * df))

    p = 2.0 * float(stats.norm.sf(z0))
    k1, k2 = np.sqrt(2.0 * df) / sd, np.sqrt(2.0 / np.pi)
    for lo, hi in zip(pts[:-1], pts[1:]):
        # between two break points one line is the lowest: the one that is at the middle.  z = hi - (hi - lo) v^2 puts the
        # square-root singularity that S_df has at z0 for df = 1 (at, or close behind, the piece's upper end) out of quad's way
        mid = 0.5 * (lo + hi)
        j = int(np.argmin(al - be * (mid * mid)))
        a_j, b_j, h = float(al[j]), float(be[j]), hi - lo

        def f(v):
            z = hi - h * v * v
            return special.chdtrc(df, (a_j - b_j * z * z - mu) * k1 + df) * k2 * np.exp(-0.5 * z * z) * 2.0 * h * v

        p += integ.quad(f, 0.0, 1.0, epsabs=0.0, epsrel=1e-12, limit=200)[0]
    return min(p, nr * T), T, float(rho[j0]), p_rho


def check_max_markers(max_markers, block):
    """``max_markers`` as an int with ``block <= max_markers <= WIDE_MAX``."""
    if isinstance(max_markers, bool) or not isinstance(max_markers, (int, np.integer)):
        raise ValueError("max_markers must be None or an integer, got %r" % (max_markers,))
    if not block <= max_markers <= WIDE_MAX:
        raise ValueError("max_markers must lie in block .. %d = %d .. %d, got %d" % (WIDE_MAX, block, WIDE_MAX, max_markers))
    return int(max_markers)


def check_sets(sets, m, block, max_markers=None):
    """``sets`` as a list of int64 index arrays into ``0 .. m-1``: each 1-D, integer, 1 .. ``block`` distinct markers.  With
    ``max_markers`` (``block .. 4096``) a set holds up to that many, and the kept sub-blocks of the widest set must fit the
    panel call: ``(B - 1) bp <= 4096`` with ``bp`` = ``block`` rounded up to 16 and ``B`` its number of sub-blocks."""
    if isinstance(sets, np.ndarray) and sets.dtype != object and sets.ndim != 2:
        raise ValueError("sets must be a sequence of 1-D integer arrays, one per set")
    if max_markers is not None:
        max_markers = check_max_markers(max_markers, block)
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
        if max_markers is None and idx.size > block:
            raise ValueError("set %d has %d markers, more than one device block of %d: sets wider than a block are not "
                             "supported" % (i, idx.size, block))
        if max_markers is not None and idx.size > max_markers:
            raise ValueError("set %d has %d markers, more than max_markers = %d" % (i, idx.size, max_markers))
        out.append(idx)
    if max_markers is not None and out:
        i = int(np.argmax([s.size for s in out]))
        bp, B = (block + 15) // 16 * 16, -(-out[i].size // block)
        if (B - 1) * bp > PANEL_COLUMNS:
            raise ValueError("set %d has %d markers: the %d sub-blocks of %d before its last one keep %d columns, %d each, more than "
                             "the %d columns of a panel call" % (i, out[i].size, B - 1, block, (B - 1) * bp, bp, PANEL_COLUMNS))
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


def plan_sets(sizes, block):
    """The device work for sets of ``sizes`` markers where some may be wider than ``block`` (``max_markers``): a list of lists of
    set numbers in the order they run.  The sets of at most ``block`` markers are packed by ``pack_sets`` as if the wider ones
    were not in the list -- the blocks of a call on them alone -- and a block runs where its first set stands; a wider set is a
    list of its own, in its position."""
    narrow = [i for i, k in enumerate(sizes) if int(k) <= block]
    work = [[narrow[j] for j in b] for b in pack_sets([sizes[i] for i in narrow], block)]
    work += [[i] for i, k in enumerate(sizes) if int(k) > block]
    return sorted(work, key=lambda members: members[0])


def assemble_wide(stats_blocks, gram_blocks, cross_blocks, bp):
    """``((c + 5) x k statistics, k x k X'X)`` of one set of k markers run as B sub-blocks: ``stats_blocks[b]`` ((c + 5) x r_b) and
    ``gram_blocks[b]`` (r_b x r_b) are what sub-block b's Gram call returned, ``cross_blocks[b - 1]`` (r_b x b ``bp``, b = 1 .. B - 1)
    is ``X_b' [X_0 .. X_(b-1)]`` as ``scan_panel_dev`` formed it against the kept sub-blocks, each of them ``bp`` columns wide of
    which the first ``block`` = r_0 are markers and the rest padding.  Every sub-block but the last holds ``block`` markers.  A
    cross block is computed once and written twice, as it stands and transposed: the matrix is symmetric bit for bit where
    the Gram blocks are."""
    B = len(stats_blocks)
    block = stats_blocks[0].shape[1]
    if B < 1 or len(gram_blocks) != B or len(cross_blocks) != B - 1 or block > bp:
        raise ValueError("%d sub-blocks need %d Gram blocks and %d cross blocks, and bp >= %d" % (B, B, B - 1, block))
    if any(S.shape[1] != block for S in stats_blocks[:-1]) or not 1 <= stats_blocks[-1].shape[1] <= block:
        raise ValueError("every sub-block but the last holds %d markers, the last 1 .. %d" % (block, block))
    S = np.concatenate(stats_blocks, axis=1)
    k = S.shape[1]
    G = np.empty((k, k))
    for b in range(B):
        r0, rb = b * block, stats_blocks[b].shape[1]
        G[r0:r0 + rb, r0:r0 + rb] = np.asarray(gram_blocks[b]).reshape(rb, rb)
        if b:
            X = np.asarray(cross_blocks[b - 1]).reshape(rb, b, bp)[:, :, :block].reshape(rb, r0)
            G[r0:r0 + rb, :r0] = X
            G[:r0, r0:r0 + rb] = X.T
    return S, G


def set_kernel(S, G, R, u, weights):
    """``(s, K, w, keep)`` of one set from its columns ``S`` of a block's statistics ((c + 5) x r) and its sub-block ``G`` of X'X,
    with the model's ``R`` and ``u``: the markers with an observed value and with variation are kept, ``z = R^-T S[4:4+c]``,
    ``s = S[4+c] - u'z``, ``K = G - z'z`` symmetrised; ``weights``: "beta", None or one weight per marker of the set."""
    c = R.shape[0]
    n_obs, mean, css = S[0], S[1], S[2]
    keep = ~((n_obs == 0) | (css == 0))
    z = la.solve_triangular(R, S[4:4 + c], trans='T', lower=False)[:, keep]
    s = S[4 + c][keep] - u.dot(z)
    K = G[np.ix_(keep, keep)] - z.T.dot(z)
    K = 0.5 * (K + K.T)
    if weights is None:
        w = np.ones(s.size)
    elif isinstance(weights, str):
        maf = np.minimum(0.5 * mean[keep], 1.0 - 0.5 * mean[keep])
        w = stats.beta.pdf(maf, 1, 25)
    else:
        w = weights[keep]
    return s, K, w, keep


class VariantSetTest(AssociationScan):
    """Burden and SKAT tests of marker sets next to ``covariates`` under V = sum_k sigma2[k] mats[k].  The constructor is
    ``AssociationScan``'s; ``block`` bounds the markers of a set as well as of a device block."""

    def __call__(self, genotypes, sets, weights="beta", method="saddlepoint", return_kernel=False, skato=False, rho=None,
                 finish="host", max_markers=None):
        """``genotypes``: m x n int8 as ``AssociationScan`` takes them; ``sets``: a sequence of 1-D integer arrays, the marker
        rows of each set (1 .. ``block`` distinct rows; a marker may belong to several sets); ``weights``: "beta" =
        Beta(1, 25) density at the marker's minor allele frequency, None = ones, or a sequence of arrays aligned with
        ``sets``; ``method``: "saddlepoint" or "liu" for ``skat_p``.  Returns a dict of length-``len(sets)`` arrays ``n_used``,
        ``burden_beta``, ``burden_se``, ``burden_chi2``, ``burden_p``, ``skat_q``, ``skat_p``; with ``return_kernel`` also
        ``kernel``, a list of ``(s, K, w)`` per set.  A marker without an observed value or without variation is dropped
        from its set (``n_used`` counts the rest); a set with nothing left gets NaN.

        ``skato=True`` adds SKAT-O over the grid ``rho`` (None = ``RHO_DEFAULT``; 1 .. 16 values in [0, 1]): ``skato_p``,
        ``skato_pmin`` (the smallest per-rho p-value), ``skato_rho`` (the first grid value that attains it) and ``skato_p_rho``
        (n_sets x n_rho), the per-rho tails by ``method``.  ``finish="device"`` does everything after the Gram block on the
        device (``scilmm_sets_finish_dev``) and brings back the sets' numbers alone; it excludes ``return_kernel``, and its
        p-values agree with the host's to 1e-6 relative, not bit for bit.  With the three at their defaults the call is what it
        was: the same keys, the same bits.

        ``max_markers`` (None, or an integer in ``block`` .. 4096) lifts the bound on a set from ``block`` to that many
        markers.  The sets of at most ``block`` markers are packed and run as without it -- the blocks of a call on them alone,
        the same bits.  A wider set runs on its own, in its position in the list, as ``ceil(k / block)`` sub-blocks of its markers
        in the order given: every sub-block is an ordinary Gram block, its forward solution is kept on the device
        (``scilmm_scan_block_keep_dev``), and the sub-blocks behind it form their cross products against what is kept
        (``scilmm_scan_panel_dev``), so ``K`` is the whole k x k matrix, symmetric bit for bit, and everything after it -- the
        weights, burden, SKAT, ``skato``, ``return_kernel`` -- is what a narrow set gets.  With bp = ``block`` rounded up to 16 and
        B the sub-blocks of the widest set, ``(B - 1) bp`` may not exceed 4096, the columns of a panel call.  The kept
        solutions are ONE device allocation of n x (B - 1) bp doubles for the widest set of the call, dropped on return: 597 MB
        at n = 83 320 and 1 024 markers, 5.9 GB at a cohort of 1M (both at ``block`` = 128).  The host algebra grows as k^3: expect
        it to take longer than the device work of a wide set, SKAT-O above all.  ``finish="device"``
        excludes a set wider than ``block``: the device finish holds one block in LDS.

        ``finish="wide"`` is the device finish for every width: a set of at most ``block`` markers runs exactly as under
        ``finish="device"`` (the same packing, the same bits); a wider one (with ``max_markers``) runs sub-block by sub-block
        as above, but its statistics, Gram blocks and cross products stay on the device, ``scilmm_sets_finish_wide_dev`` is
        queued behind the last sub-block, and one row of numbers comes back.  It excludes ``return_kernel`` and agrees with the
        host finish as ``finish="device"`` does."""
        return self._run(Int8Rows(self, check_genotypes(genotypes, self.n)), sets, weights, method, return_kernel, skato, rho, finish,
                         max_markers=max_markers)

    def test_bed(self, bed, sets, sample_index=None, count="A1", chunk_bytes=None, weights="beta", method="saddlepoint",
                 return_kernel=False, skato=False, rho=None, finish="host", max_markers=None):
        """``__call__`` on the markers of a PLINK 1 fileset, decoded on the device (``scilmm_scan_block_bed_gram_dev``):
        ``sets`` index the file's markers; ``bed``, ``sample_index`` and ``count`` as for ``AssociationScan.scan_bed``.  A
        block's packed rows are uploaded as they lie in the file, so ``chunk_bytes`` has nothing to bound and is accepted
        for symmetry only.  Returns the bits of ``__call__`` on ``bed.read(None, sample_index, count)`` in deterministic
        mode.  ``skato``, ``rho``, ``finish``, ``max_markers``: as for ``__call__``."""
        src = self._bed_source(bed, sample_index, count)
        if chunk_bytes is not None and int(chunk_bytes) < 1:
            raise ValueError("chunk_bytes must be positive")
        return self._run(src, sets, weights, method, return_kernel, skato, rho, finish, max_markers=max_markers)

    def test_dosages(self, dosages, sets, sample_index=None, weights="beta", method="saddlepoint", return_kernel=False, skato=False,
                     rho=None, finish="host", max_markers=None):
        """``__call__`` on imputed dosages (``scilmm_scan_block_dosage_gram_dev``): ``sets`` index the rows of ``dosages``;
        ``dosages`` and ``sample_index`` as for ``AssociationScan.scan_dosages``.  The "beta" weights take half the mean
        dosage for the allele frequency.  For uint16 codes of hard calls it returns the bits of ``__call__`` on the int8
        markers in deterministic mode.  ``skato``, ``rho``, ``finish``, ``max_markers``: as for ``__call__``."""
        return self._run(self._dosage_source(dosages, sample_index), sets, weights, method, return_kernel, skato, rho, finish,
                         max_markers=max_markers)

    def set_traits(self, Y, scale="fixed"):
        """The variant-set tests of this tester against a panel of T quantitative traits under the same V: a ``SetTraitPanel``
        (``scilmm_amd.set_panel``) on this tester's factor and whitening.  ``Y``: n x T float64, finite, 1 <= T <= 4096, rows in
        the order of ``mats``; ``scale``: "fixed" or "profile", as for ``traits`` (which stays the MARKER panel of the scan).
        ``panel(genotypes, sets, ...)`` tests every set against every trait for one sweep, one Gram pass and one
        eigendecomposition per set, whatever T is."""
        from .set_panel import SetTraitPanel
        return SetTraitPanel(self, Y, scale)

    def masks(self, annotations, max_maf=(0.01, 0.001, 0.0001), acat_mac=10):
        """The variant-set tests of this tester under functional annotation masks crossed with MAF cutoffs, with ACAT-V per cell
        and the ACAT-O combination per set: a ``MaskedSetTest`` (``scilmm_amd.set_masks``) on this tester's factor and whitening.
        ``annotations``: m x A booleans (rows as ``sets`` index the marker source), or a sequence aligned with ``sets`` of k_i x A
        booleans, 1 <= A <= 32; ``max_maf``: 1 .. 8 cutoffs in (0, 0.5]; ``acat_mac``: ACAT-V pools the markers whose minor allele
        count is at most this.  ``masked(genotypes, sets, ...)`` tests every (set, annotation, cutoff) cell for one sweep and one
        Gram pass per block of sets."""
        from .set_masks import MaskedSetTest
        return MaskedSetTest(self, annotations, max_maf, acat_mac)

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

    def _block_wide(self, src, bmax, staged):
        """rows (more than ``block`` of them) -> ((q + 4) x k statistics, k x k X'X) of one set of up to ``bmax`` sub-blocks, on the
        host.  Sub-block b holds rows ``[b block, (b + 1) block)`` in the order given and is run as any block is: its rows are
        brought to the device and the form's Gram entry point gives its statistics and its diagonal block of X'X.  Behind it,
        on the stream, ``scan_panel_dev`` forms its cross block against the ``b bp`` columns kept so far (b > 0) and
        ``scan_block_keep_dev`` puts its forward solution behind them (b < B - 1); one wait per sub-block, then the copies of
        what it returned.  ``assemble_wide`` puts the pieces together.  The store is ONE allocation, n x (``bmax`` - 1) bp
        doubles (bp = ``block`` rounded up to 16), shared by the wide sets of a call and dropped with this closure."""
        torch, q, blk = self.torch, self.q, self.block
        bp = (blk + 15) // 16 * 16
        ld = (bmax - 1) * bp
        if not staged:
            src.stage(blk)
        vp = C.c_void_p
        dS = torch.empty(((q + 4) * blk,), dtype=torch.float64, device="cuda")
        dK = torch.empty((blk * blk,), dtype=torch.float64, device="cuda")
        dX = torch.empty((blk * ld,), dtype=torch.float64, device="cuda")
        store = torch.empty((self.n * ld,), dtype=torch.float64, device="cuda")

        def run(rows):
            B = -(-rows.size // blk)
            Ss, Gs, Xs = [], [], []
            for b in range(B):
                sub = rows[b * blk:(b + 1) * blk]
                rb, t = sub.size, b * bp
                src.load(sub)
                src.enqueue(0, rb, vp(dS.data_ptr()), vp(dK.data_ptr()))
                if b > 0:
                    self.factor.scan_panel_dev(rb, vp(store.data_ptr()), ld, t, vp(dX.data_ptr()), t)
                if b < B - 1:
                    self.factor.scan_block_keep_dev(rb, vp(store.data_ptr()), ld, t)
                self.sym.sync()
                Ss.append(dS[:(q + 4) * rb].cpu().numpy().reshape(q + 4, rb))
                Gs.append(dK[:rb * rb].cpu().numpy().reshape(rb, rb))
                if b > 0:
                    Xs.append(dX[:rb * t].cpu().numpy().reshape(rb, t))
            return assemble_wide(Ss, Gs, Xs, bp)
        return run

    def _block_wide_device(self, src, bmax, staged, mode, method, rho):
        """(rows, weights) -> the row of ``scilmm_sets_finish_wide_dev`` (10 + n_rho doubles) of one set of more than ``block`` rows
        and up to ``bmax`` sub-blocks, on the host.  The sub-blocks run as in ``_block_wide`` -- one wait each: the next one's rows
        take the place of this one's -- but nothing of them is copied back: every Gram call writes its own slice of the
        statistics and of the diagonal blocks, the panel call writes the sub-block's rows of the cross store.  The finish is
        queued behind the last sub-block; one more wait, one copy of the row."""
        torch, q, blk = self.torch, self.q, self.block
        bp = (blk + 15) // 16 * 16
        ld = (bmax - 1) * bp
        if not staged:
            src.stage(blk)
        vp = C.c_void_p
        dS = torch.empty((bmax * (q + 4) * blk,), dtype=torch.float64, device="cuda")
        dK = torch.empty((bmax * blk * blk,), dtype=torch.float64, device="cuda")
        dX = torch.empty((bmax * blk * ld,), dtype=torch.float64, device="cuda")
        store = torch.empty((self.n * ld,), dtype=torch.float64, device="cuda")
        dR = torch.from_numpy(np.ascontiguousarray(self.R)).cuda()
        du = torch.from_numpy(np.ascontiguousarray(self.u)).cuda()
        dW = torch.empty((bmax * blk,), dtype=torch.float64, device="cuda")
        dO = torch.empty((FINISH_HEAD + rho.size,), dtype=torch.float64, device="cuda")
        meth = METHODS.index(method)

        def run(rows, w):
            k = rows.size
            B = -(-k // blk)
            if w is not None:
                dW[:k].copy_(torch.from_numpy(w))
            for b in range(B):
                sub = rows[b * blk:(b + 1) * blk]
                rb, t = sub.size, b * bp
                src.load(sub)
                src.enqueue(0, rb, vp(dS.data_ptr() + 8 * b * (q + 4) * blk), vp(dK.data_ptr() + 8 * b * blk * blk))
                if b > 0:
                    self.factor.scan_panel_dev(rb, vp(store.data_ptr()), ld, t, vp(dX.data_ptr() + 8 * b * blk * ld), ld)
                if b < B - 1:
                    self.factor.scan_block_keep_dev(rb, vp(store.data_ptr()), ld, t)
                self.sym.sync()
            self.factor.sets_finish_wide_dev(k, blk, q, vp(dS.data_ptr()), vp(dK.data_ptr()), vp(dX.data_ptr()), ld, vp(dR.data_ptr()),
                                             vp(du.data_ptr()), self.c, mode, vp(dW.data_ptr()) if w is not None else None, meth, rho,
                                             vp(dO.data_ptr()), None)
            self.sym.sync()
            return dO.cpu().numpy().reshape(1, FINISH_HEAD + rho.size)
        return run

    def _block_device(self, src, mode, method, rho):
        """(rows, offsets, weights) -> the block's per-set rows of ``scilmm_sets_finish_dev`` (n_sets x (10 + n_rho)), on the host:
        the rows and the weights are brought to the device, the form's Gram entry point and the finish are queued one behind the
        other, one wait, one device-to-host copy of the sets' rows."""
        torch, q, blk = self.torch, self.q, self.block
        src.stage(blk)
        vp = C.c_void_p
        dS = torch.empty(((q + 4) * blk,), dtype=torch.float64, device="cuda")
        dK = torch.empty((blk * blk,), dtype=torch.float64, device="cuda")
        dR = torch.from_numpy(np.ascontiguousarray(self.R)).cuda()
        du = torch.from_numpy(np.ascontiguousarray(self.u)).cuda()
        dW = torch.empty((blk,), dtype=torch.float64, device="cuda")
        ld = FINISH_HEAD + rho.size
        dO = torch.empty((blk * ld,), dtype=torch.float64, device="cuda")
        meth = METHODS.index(method)

        def run(rows, start, w):
            rb, ns = rows.size, start.size - 1
            src.load(rows)
            if w is not None:
                dW[:rb].copy_(torch.from_numpy(w))
            src.enqueue(0, rb, vp(dS.data_ptr()), vp(dK.data_ptr()))
            self.factor.sets_finish_dev(rb, q, vp(dS.data_ptr()), vp(dK.data_ptr()), vp(dR.data_ptr()), vp(du.data_ptr()), self.c, ns,
                                        start, mode, vp(dW.data_ptr()) if w is not None else None, meth, rho, vp(dO.data_ptr()), ld, None)
            self.sym.sync()
            return dO[:ns * ld].cpu().numpy().reshape(ns, ld)
        return run

    def _run(self, src, sets, weights, method, return_kernel, skato=False, rho=None, finish="host", max_markers=None):
        """The checks of the sets (before any launch), then block by block: gather the block's marker rows, one device call, the
        statistics and the Gram matrix (``_block``), the host algebra set by set -- or, with ``finish="device"``, the finish
        queued behind the block and the sets' rows alone brought back (``_block_device``).  With ``max_markers`` a set wider than
        a block runs on its own, sub-block by sub-block (``_block_wide``), and meets the same host algebra -- or, with
        ``finish="wide"``, the wide finish on the device (``_block_wide_device``)."""
        sets = check_sets(sets, src.m, self.block, max_markers)
        weights, sf = check_weights(weights, sets), check_method(method)
        if finish not in FINISH_VALUES:
            raise ValueError("finish must be one of %s, got %r" % (", ".join(FINISH_VALUES), finish))
        if finish != "host" and return_kernel:
            raise ValueError('return_kernel=True needs finish="host": the device finish does not bring K back')
        sizes = [s.size for s in sets]
        widest = max(sizes + [0])
        if finish == "device" and widest > self.block:
            raise ValueError('a set of %d markers needs finish="host" or finish="wide": the device finish holds one block of at most '
                             '%d markers in LDS' % (widest, self.block))
        rho = check_rho(rho) if skato else None
        self._check_factor()
        ns = len(sets)
        out = {k: np.full(ns, np.nan) for k in KEYS}
        out["n_used"] = np.zeros(ns, dtype=np.int64)
        if skato:
            out.update({k: np.full(ns, np.nan) for k in SKATO_KEYS[:3]})
            out["skato_p_rho"] = np.full((ns, rho.size), np.nan)
        packed = pack_sets(sizes, self.block) if widest <= self.block else plan_sets(sizes, self.block)
        if finish != "host":
            given = not (weights is None or isinstance(weights, str))
            mode = WEIGHT_GIVEN if given else WEIGHT_ONES if weights is None else WEIGHT_BETA
            grid = rho if skato else np.empty(0)
            narrow = any(s.size <= self.block for s in sets)
            block = self._block_device(src, mode, method, grid) if narrow else None
            wide = self._block_wide_device(src, -(-widest // self.block), narrow, mode, method, grid) if widest > self.block else None
            for members in packed:
                if sets[members[0]].size > self.block:           # (finish="wide": a wide set is a list of its own)
                    O = wide(sets[members[0]], np.ascontiguousarray(weights[members[0]]) if given else None)
                else:
                    start = np.concatenate([[0], np.cumsum([sets[i].size for i in members])]).astype(np.int32)
                    w = np.ascontiguousarray(np.concatenate([weights[i] for i in members])) if given else None
                    O = block(np.concatenate([sets[i] for i in members]), start, w)
                out["n_used"][members] = O[:, 0].astype(np.int64)
                for col, k in ((1, "burden_beta"), (2, "burden_se"), (3, "burden_chi2"), (4, "skat_q"), (5, "skat_p")):
                    out[k][members] = O[:, col]
                if skato:
                    for col, k in ((6, "skato_p"), (7, "skato_pmin"), (8, "skato_rho")):
                        out[k][members] = O[:, col]
                    out["skato_p_rho"][members] = O[:, FINISH_HEAD:]
            used = out["n_used"] > 0
            out["burden_p"][used] = self._f.sf(out["burden_chi2"][used])     # (one vectorised call over the sets)
            return out
        narrow = any(s.size <= self.block for s in sets)
        block = self._block(src) if narrow else None
        wide = self._block_wide(src, -(-widest // self.block), narrow) if widest > self.block else None
        kernel = [None] * ns
        for members in packed:
            if sets[members[0]].size > self.block:
                i = members[0]
                S, G = wide(sets[i])
                w = weights if weights is None or isinstance(weights, str) else weights[i]
                kernel[i] = self._one_set(out, i, S, G, w, sf, rho, method)
                continue
            S, G = block(np.concatenate([sets[i] for i in members]))
            a = 0
            for i in members:
                b = a + sets[i].size
                w = weights if weights is None or isinstance(weights, str) else weights[i]
                kernel[i] = self._one_set(out, i, S[:, a:b], G[a:b, a:b], w, sf, rho, method)
                a = b
        if return_kernel:
            out["kernel"] = kernel
        return out

    def _one_set(self, out, i, S, G, weights, sf, rho=None, method="saddlepoint"):
        """The host algebra of set ``i`` on its columns of the statistics and its sub-block of X'X; returns (s, K, w)."""
        s, K, w, keep = set_kernel(S, G, self.R, self.u, weights)
        out["n_used"][i] = k = int(keep.sum())
        if k:
            ws, wKw = float(w.dot(s)), float(w.dot(K.dot(w)))
            with np.errstate(divide="ignore", invalid="ignore"):
                out["burden_beta"][i] = ws / wKw
                out["burden_se"][i] = 1.0 / np.sqrt(wKw)
                out["burden_chi2"][i] = chi2 = ws * ws / wKw
            out["burden_p"][i] = self._f.sf(chi2)
            out["skat_q"][i] = qs = float(np.sum(w * w * s * s))
            A = w[:, None] * K * w[None, :]
            lam = la.eigvalsh(A)
            if lam.size and lam.max() > 0:
                out["skat_p"][i] = sf(qs, lam[lam > LAMBDA_FLOOR * lam.max()])
                if rho is not None:
                    out["skato_p"][i], out["skato_pmin"][i], out["skato_rho"][i], out["skato_p_rho"][i] = skato_pvalue(w * s, A, rho, method)
        return s, K, w
