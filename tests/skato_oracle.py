"""SKAT-O written from the formulas of the SKAT package (Lee, Wu, Lin 2012; SKAT_Optimal_Param, SKAT_Optimal_Each_Q,
SKAT_Optimal_PValue), on the n x r matrix ``Z1`` with ``Z1'Z1 = diag(w) K diag(w)`` -- not on the r x r matrix that
``scilmm_amd.sets.skato_pvalue`` reduces everything to, and sharing no code with that module: the mixture tails (modified Liu,
Lugannani-Rice with its seam), the quantiles and the integral are written again here.

Where this departs from the package, on purpose (the issue behind the feature asks for it):
  * the package halves Q and Z1'Z1 together; the common factor cancels everywhere and is left out;
  * eigenvalues below 1e-10 of the largest are dropped (the package: below 1e-5 of the mean of the positive ones);
  * the last integral is taken in survival form, over z with x = z^2, piece by piece between the kinks of the minimum and up to
    the point where the integrand becomes 2 phi(z) (the package integrates 1 - F over x in [0, 40] without break points).
"""
import numpy as np
import scipy.integrate
import scipy.linalg
import scipy.optimize
import scipy.stats as st

FLOOR = 1e-10
SEAM = 0.05
RHO = (0.0, 0.01, 0.04, 0.09, 0.16, 0.25, 0.5, 1.0)


def z1_from_model(Vinv, Cv, Gt, w):
    """``Z1 = P^1/2 G~' diag(w)`` (n x r) from the dense ``inv(V)``, the covariates, the centred markers (r x n) and the weights:
    ``P = V^-1 - V^-1 C (C'V^-1 C)^-1 C'V^-1``, its square root by ``eigh``.  Returns ``(Z1, P)``."""
    ViC = Vinv @ Cv
    P = Vinv - ViC @ np.linalg.solve(Cv.T @ ViC, ViC.T)
    P = 0.5 * (P + P.T)
    ev, U = np.linalg.eigh(P)
    half = (U * np.sqrt(np.maximum(ev, 0.0))) @ U.T
    return half @ Gt.T * np.asarray(w)[None, :], P


def z1_from_gram(A):
    """An r x r ``Z1`` with ``Z1'Z1 = A`` for a positive semidefinite ``A`` (the symmetric square root)."""
    ev, U = np.linalg.eigh(0.5 * (A + A.T))
    return (U * np.sqrt(np.maximum(ev, 0.0))) @ U.T


def _liu(lam):
    c = [np.sum(lam ** k) for k in (1, 2, 3, 4)]
    s1, s2 = c[2] / c[1] ** 1.5, c[3] / c[1] ** 2
    if s1 * s1 > s2 * (1.0 + 1e-12):
        a = 1.0 / (s1 - np.sqrt(s1 * s1 - s2))
        d = s1 * a ** 3 - a * a
        l = a * a - 2.0 * d
    else:
        l, d = 1.0 / s2, 0.0
        a = np.sqrt(l)
    return c[0], np.sqrt(2.0 * c[1]), a, d, l


def sf_liu(q, lam):
    mu, sd, a, d, l = _liu(lam)
    x = (q - mu) / sd * np.sqrt(2.0) * a + l + d
    if x <= 0:
        return 1.0
    return float(st.chi2.sf(x, l) if d == 0.0 else st.ncx2.sf(x, l, d))


def _lr(q, lam):
    """Lugannani-Rice at q != mean: the saddlepoint by bisection-safe root finding on (-inf, 1 / (2 max lam))."""
    top = 0.5 / lam.max()
    k1 = lambda t: np.sum(lam / (1.0 - 2.0 * lam * t)) - q
    if q > lam.sum():
        lo, hi = 0.0, top * (1.0 - 1e-16)
        e = 0.5
        while k1(top * (1.0 - e)) < 0:
            e *= 0.5
        hi = top * (1.0 - e)
    else:
        lo, hi = -top, 0.0
        while k1(lo) > 0:
            lo *= 2.0
    t = scipy.optimize.brentq(k1, lo, hi, xtol=1e-300, rtol=8.9e-16, maxiter=1000)
    den = 1.0 - 2.0 * lam * t
    K0, K2 = -0.5 * np.sum(np.log(den)), 2.0 * np.sum((lam / den) ** 2)
    w, v = np.sign(t) * np.sqrt(2.0 * (t * q - K0)), t * np.sqrt(K2)
    return float(st.norm.sf(w + np.log(v / w) / w))


def in_seam(q, lam):
    return abs(q - lam.sum()) < SEAM * np.sqrt(2.0 * np.sum(lam * lam))


def sf_saddle(q, lam):
    if q <= 0:
        return 1.0
    mu, sd = lam.sum(), np.sqrt(2.0 * np.sum(lam * lam))
    if not in_seam(q, lam):
        return _lr(q, lam)
    lo, hi = mu - SEAM * sd, mu + SEAM * sd
    c_lo, c_hi = _lr(lo, lam) / sf_liu(lo, lam), _lr(hi, lam) / sf_liu(hi, lam)
    return sf_liu(q, lam) * (c_lo + (c_hi - c_lo) * (q - lo) / (hi - lo))


def _lambda(M, scale=0.0):
    lam = scipy.linalg.eigvalsh(0.5 * (M + M.T))
    if not lam.size or not lam.max() > scale:
        return lam[:0]
    return lam[lam > FLOOR * lam.max()]


def skato(Z1, t, rho=RHO, method="saddlepoint"):
    """A dict: ``p``, ``pmin``, ``rho`` (the first minimiser), ``p_rho``, and what the tests want to know about the case:
    ``seam`` (per rho: Q_rho lies inside the saddlepoint seam), ``q_rho``, ``lam_rho``, ``degenerate``."""
    sf = {"saddlepoint": sf_saddle, "liu": sf_liu}[method]
    Z1, t = np.asarray(Z1, dtype=np.float64), np.asarray(t, dtype=np.float64)
    n, r = Z1.shape
    rho = np.asarray(rho, dtype=np.float64)
    rc = np.minimum(rho, 0.999)
    out = dict(p=np.nan, pmin=np.nan, rho=np.nan, p_rho=np.full(rho.size, np.nan), seam=np.zeros(rho.size, bool), q_rho=[], lam_rho=[],
               degenerate=False)
    for j, x in enumerate(rc):
        q = (1.0 - x) * np.sum(t * t) + x * np.sum(t) ** 2 if r > 1 else float(t[0] * t[0])
        Rr = (1.0 - x) * np.eye(r) + x * np.ones((r, r))
        Lc = np.linalg.cholesky(Rr).T                       # upper, Lc'Lc = R_rho (the package's chol)
        Z2 = Z1 @ Lc.T
        lam = _lambda(Z2.T @ Z2)
        out["q_rho"].append(q)
        out["lam_rho"].append(lam)
        if lam.size:
            out["p_rho"][j] = sf(q, lam)
            out["seam"][j] = in_seam(q, lam)
    if np.any(np.isnan(out["p_rho"])):
        return out
    j0 = int(np.argmin(out["p_rho"]))
    T = out["pmin"] = float(out["p_rho"][j0])
    out["rho"] = float(rho[j0])
    # SKAT_Optimal_Param
    zm = Z1.mean(axis=1)
    zz = float(np.sum(zm * zm))
    tr = float(np.sum(Z1 * Z1))
    lamB = np.empty(0)
    if r > 1 and r * r * zz > FLOOR * tr:
        cof1 = (zm @ Z1) / zz
        item1 = np.outer(zm, cof1)
        item2 = Z1 - item1
        W2 = item2.T @ item2
        lamB = _lambda(W2, FLOOR * tr)
    if not lamB.size or T == 0.0:                           # (T = 0: it has underflowed, and so has p)
        out["p"], out["degenerate"] = T, True
        if not lamB.size:                                   # every p_rho is the same up to rounding: the first grid value
            out["rho"] = float(rho[0])
        return out
    mu = float(lamB.sum())
    var = 2.0 * float(np.sum(lamB ** 2)) + 4.0 * float(np.sum((item1.T @ item1) * W2))
    df = float(np.sum(lamB ** 2)) ** 2 / float(np.sum(lamB ** 4))
    tau = r * r * rc * zz + (1.0 - rc) * float(np.sum(cof1 ** 2)) * zz
    # SKAT_Optimal_Each_Q: the 1 - T quantile of every Q_rho by the modified Liu matching
    qmin = np.empty(rho.size)
    for j, lam in enumerate(out["lam_rho"]):
        m1, sd1, _, _, l = _liu(lam)
        qmin[j] = (st.chi2.isf(T, l) - l) / np.sqrt(2.0 * l) * sd1 + m1
    al, be = qmin / (1.0 - rc), tau / (1.0 - rc)
    sd = np.sqrt(var)

    def arg(z):
        return (np.min(al - be * z * z) - mu) / sd * np.sqrt(2.0 * df) + df

    def f(z):
        return st.chi2.sf(arg(z), df) * 2.0 * st.norm.pdf(z)

    if arg(0.0) <= 0.0:
        p = 1.0
    else:
        # the integrand is 2 phi(z) from z0 on, where the argument has come down to 0
        hi = 1.0
        while arg(hi) > 0.0:
            hi *= 2.0
        z0 = scipy.optimize.brentq(arg, 0.0, hi, xtol=1e-300, rtol=8.9e-16)
        end = min(z0, 40.0)
        pts = {0.0, end}
        for i in range(rho.size):
            for j in range(i + 1, rho.size):
                if be[i] != be[j]:
                    x = (al[i] - al[j]) / (be[i] - be[j])
                    if x > 0 and np.sqrt(x) < end:
                        pts.add(float(np.sqrt(x)))
        pts = sorted(pts)
        p = 2.0 * float(st.norm.sf(z0))
        for lo, up in zip(pts[:-1], pts[1:]):
            p += scipy.integrate.quad(f, lo, up, epsabs=0.0, epsrel=1e-12, limit=200)[0]
    out["p"] = min(p, rho.size * T)
    return out
