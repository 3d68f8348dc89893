"""Host algebra of the variant-set tests for binary traits (``scilmm_amd.glmm.BinarySetTest``): the inverse
that turns a saddlepoint ``log p`` into a normal deviate, and the tests on the rescaled covariance.  Pure NumPy / SciPy: nothing
of a device is touched here.

With the score ``s``, its covariance ``K`` and the weights ``w`` of a set's kept markers (``sets.set_kernel``) and a variance
scale per marker, ``t = w o s`` is unchanged and ``A~ = diag(w o scale) K diag(w o scale)`` takes the place of
``diag(w) K diag(w)``: burden ``chi2 = (1't)^2 / 1'A~1`` against chi2_1, SKAT ``Q = t't`` against the spectrum of ``A~``, SKAT-O
as ``sets.skato_pvalue`` on ``(t, A~)``.  The scales themselves -- ``rho_j`` from the markers' saddlepoint p-values and the burden
floor ``phi`` -- are the device's (``scilmm_sets_spa*_dev``); ``normal_deviate`` is the host form of the one step of theirs that
is not plain arithmetic.
"""
import numpy as np
import scipy.linalg as la
import scipy.special as special

from . import sets as S

BSPA_ROWLEN = 13            # log_p_B | a_w | s_B | zeta_hi | zeta_lo | iters | flag | a_B | b_B | v~_B | V_Q | phi | n_adj (csrc/setspa.hip.h)
FLAG_SCALED = 16            # bit 4 of a finish row's flags: a kept column's scale is not 1
BINARY_KEYS = ("burden_chi2_norm", "burden_spa_log_p", "burden_spa_flag", "burden_scale", "n_adjusted")


def log_erfc(v):
    """``log erfc(v / sqrt 2)`` for v >= 0: the logarithm of the two-sided normal tail, finite far beyond where the tail underflows."""
    v = np.asarray(v, dtype=np.float64)
    y = v * np.sqrt(0.5)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(y < 0.5, np.log1p(-special.erf(y)), np.log(special.erfcx(y)) - 0.5 * v * v)


def normal_deviate(log_p, max_iter=100):
    """``v >= 0`` with ``log erfc(v / sqrt 2) = log_p`` (the two-sided normal deviate of ``p``), element by element; NaN where
    ``log_p`` is NaN or not below 0, infinite for ``-inf``.  Newton inside a bracket from its upper end ``sqrt(-2 log_p)`` -- the
    function is decreasing and concave, so the steps come down to the root from above -- as the device takes it."""
    lp = np.atleast_1d(np.asarray(log_p, dtype=np.float64))
    out = np.full(lp.shape, np.nan)
    out[lp == -np.inf] = np.inf
    ok = (lp < 0) & np.isfinite(lp)
    t = lp[ok]
    lo, hi = np.zeros(t.size), np.sqrt(-2.0 * t)
    v = hi.copy()
    for _ in range(max_iter):
        f = log_erfc(v) - t
        lo, hi = np.where(f > 0, v, lo), np.where(f > 0, hi, v)
        vn = v + f * special.erfcx(v * np.sqrt(0.5)) * np.sqrt(0.5 * np.pi)
        vn = np.where((vn > lo) & (vn < hi), vn, 0.5 * (lo + hi))
        done = np.abs(vn - v) <= 1e-15 * vn
        v = vn
        if np.all(done):
            break
    out[ok] = v
    return out.reshape(np.shape(log_p))


def scaled_tests(s, K, w, vscale, method="saddlepoint", rho=None):
    """The tests of one set on ``(t, A~)``: a dict of ``burden_beta = 1't / 1'A~1``, ``burden_se = (1'A~1)^-1/2``,
    ``burden_chi2 = (1't)^2 / 1'A~1``, ``skat_q = t't``, ``skat_p`` (NaN where ``A~`` has no positive eigenvalue) and, with a grid
    ``rho``, ``skato`` = ``sets.skato_pvalue(t, A~, rho, method)``."""
    s, w, vscale = (np.asarray(v, dtype=np.float64).ravel() for v in (s, w, vscale))
    K = np.asarray(K, dtype=np.float64).reshape(s.size, s.size)
    sf = S.check_method(method)
    t, ws = w * s, w * vscale
    A = ws[:, None] * K * ws[None, :]
    t1, s11 = float(t.sum()), float(A.sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        out = {"burden_beta": t1 / s11, "burden_se": 1.0 / np.sqrt(s11), "burden_chi2": t1 * t1 / s11}
    out["skat_q"] = q = float(t.dot(t))
    out["skat_p"], out["skato"] = np.nan, None
    lam = la.eigvalsh(A)
    if lam.size and lam.max() > 0:
        out["skat_p"] = sf(q, lam[lam > S.LAMBDA_FLOOR * lam.max()])
        if rho is not None:
            out["skato"] = S.skato_pvalue(t, A, rho, method)
    return out
