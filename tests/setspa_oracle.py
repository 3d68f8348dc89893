"""Dense NumPy / SciPy oracle of the variant-set tests for binary traits (scilmm_amd.glmm.BinarySetTest), steps 1 - 5 of DESIGN.md
section 20 written as the section states them: the dense ``P``, the markers' and the burden's saddlepoint p-values through
``spa_oracle.spa`` (brentq roots), the two-sided normal deviate of a ``log p`` from SciPy's inverse where ``p`` is representable
and from a bracketed root on ``log erfc`` (via ``log_ndtr``) where it is not, and the tests on ``(t, A~)`` through
``tests/skato_oracle.py``.  Nothing here uses the library."""
import numpy as np
import scipy.linalg as la
import scipy.optimize as opt
import scipy.special as sc
import scipy.stats as stats

from tests import skato_oracle as KO
from tests import spa_oracle as SO


def deviate(log_p):
    """v >= 0 with log erfc(v / sqrt 2) = log(2 Phi(-v)) = log_p, for log_p < 0."""
    if log_p > -600.0:
        return float(-sc.ndtri(0.5 * np.exp(log_p)))
    f = lambda v: np.log(2.0) + sc.log_ndtr(-v) - log_p
    return float(opt.brentq(f, 0.0, np.sqrt(-2.0 * log_p) + 1.0, xtol=1e-300, rtol=8.9e-16, maxiter=1000))


def chi2_of(flag, log_p):
    """x = v^2 of a saddlepoint result, or None where step 1 gives none."""
    if flag != 1 or not log_p < 0:
        return None
    v = deviate(log_p)
    x = v * v
    return x if np.isfinite(x) and x > 0 else None


class Cohort(object):
    """The dense parts every set of one null point shares: ``P`` of ``V = W^-1 + sum tau_k A_k``, the centred markers, the
    covariate adjustment of step 1 of the saddlepoint call, and (per cutoff, cached) the markers' saddlepoint results."""

    def __init__(self, A_list, tau, C, mu, working_y, G):
        A = [np.asarray(a.toarray() if hasattr(a, "toarray") else a, dtype=float) for a in A_list]
        self.mu, self.C, self.y = mu, C, working_y
        self.w = mu * (1 - mu)
        Vi = la.inv(np.diag(1 / self.w) + sum(tk * a for tk, a in zip(tau, A)))
        ViC = Vi @ C
        P = Vi - ViC @ la.solve(C.T @ ViC, ViC.T)
        self.P = 0.5 * (P + P.T)
        self.Gt, self.n_obs, self.mean = SO.centred(G)
        self.keep = (self.n_obs > 0) & (np.abs(self.Gt).max(axis=1) > 0)
        self.PG = self.P @ self.Gt.T
        self.b = working_y @ self.PG
        self.a = np.sum(self.Gt.T * self.PG, axis=0)
        self._markers = {}

    def adjust(self, g):
        """g^ = g~ - C (C'WC)^-1 C'W g~."""
        C, w = self.C, self.w
        return g - C @ la.solve((C.T * w) @ C, (C.T * w) @ g)

    def spa(self, g, a, b, cutoff):
        """Steps 1 - 3 of the saddlepoint call for the centred row g with score b and variance a: dict of flag, log_p, a_w, s."""
        out = dict(flag=0, log_p=np.nan, a_w=np.nan, s=np.nan, zs=np.nan)
        if not a > 0:
            return out
        out["zs"] = zs = b / np.sqrt(a)
        if not abs(zs) > cutoff:
            return out
        gh = self.adjust(g)
        a_w = float((gh * gh) @ self.w)
        s = b * np.sqrt(a_w / a)
        r = SO.spa(gh, self.mu, s, zs)
        out.update(flag=r["flag"], log_p=r["log_p"], a_w=a_w, s=s)
        return out

    def markers(self, cutoff):
        """Per marker the saddlepoint result behind its plain block (flag 0 for a dropped marker), computed once per cutoff."""
        if cutoff not in self._markers:
            rows = []
            for j in range(self.Gt.shape[0]):
                rows.append(self.spa(self.Gt[j], self.a[j], self.b[j], cutoff) if self.keep[j]
                            else dict(flag=0, log_p=np.nan, a_w=np.nan, s=np.nan, zs=np.nan))
            self._markers[cutoff] = rows
        return self._markers[cutoff]


def weights_of(co, rows, weights):
    if weights is None:
        return np.ones(rows.size)
    if isinstance(weights, str):
        maf = np.minimum(0.5 * co.mean[rows], 1.0 - 0.5 * co.mean[rows])
        return stats.beta.pdf(maf, 1, 25)
    return np.asarray(weights, dtype=float)


def tests_on(t, A, rho=KO.RHO, method="saddlepoint"):
    """Step 5 on (t, A~): burden_chi2 / beta / se, skat_q, skat_p and SKAT-O from the Z1 oracle."""
    t1, s11 = t.sum(), A.sum()
    out = dict(burden_chi2=t1 * t1 / s11, burden_beta=t1 / s11, burden_se=1 / np.sqrt(s11), skat_q=float(t @ t))
    out["burden_p"] = float(stats.chi2.sf(out["burden_chi2"], 1))
    sf = {"saddlepoint": KO.sf_saddle, "liu": KO.sf_liu}[method]
    lam = KO._lambda(A)
    out["skat_p"] = sf(out["skat_q"], lam) if lam.size else np.nan
    o = KO.skato(KO.z1_from_gram(A), t, rho, method)
    out.update(skato_p=o["p"], skato_pmin=o["pmin"], skato_rho=o["rho"], skato_p_rho=o["p_rho"])
    return out


def set_test(co, rows, weights="beta", cutoff=2.0, rho=KO.RHO, method="saddlepoint"):
    """Steps 1 - 5 for the set of marker rows ``rows`` (``weights``: "beta", None or one per row).  A dict with what
    ``BinarySetTest`` returns for the set and what the device's 13 numbers hold, plus ``vscale`` (kept markers, rho_j sqrt(phi)),
    ``zs`` (kept markers), ``zs_B``, ``x_B`` and ``kept``."""
    rows = np.asarray(rows, dtype=np.int64)
    w_all = weights_of(co, rows, weights)
    keep = co.keep[rows]
    kept, w = rows[keep], w_all[keep]
    out = dict(n_used=int(keep.sum()), kept=kept, flag=0, n_adj=0)
    if not kept.size:
        return out
    s = co.b[kept]
    K = co.Gt[kept] @ co.PG[:, kept]
    K = 0.5 * (K + K.T)
    a = np.diag(K)
    mk = co.markers(cutoff)
    # 1. the markers' variance scales
    rho_j = np.ones(kept.size)
    with np.errstate(invalid="ignore", divide="ignore"):
        zs = s / np.sqrt(a)
    for i, j in enumerate(kept):
        x = chi2_of(mk[j]["flag"], mk[j]["log_p"])
        if x is not None and a[i] > 0:
            rho_j[i] = np.sqrt(zs[i] ** 2 / x)
    out["n_adj"] = int(np.sum(rho_j != 1.0))
    # 2. - 3. the adjusted kernel and the burden's saddlepoint call
    t = w * s
    b_B, a_B = float(w @ s), float(w @ K @ w)
    r = co.spa(w @ co.Gt[kept], a_B, b_B, cutoff)
    x_B = chi2_of(r["flag"], r["log_p"])
    v_B = b_B * b_B / x_B if x_B is not None else None
    # 4. the burden floor
    wr = w * rho_j
    V_Q = float(wr @ K @ wr)
    phi = v_B / V_Q if v_B is not None and v_B > V_Q and V_Q > 0 else 1.0
    vscale = rho_j * np.sqrt(phi)
    ws = w * vscale
    A = ws[:, None] * K * ws[None, :]
    out.update(s=s, K=K, w=w, t=t, A=A, zs=zs, zs_B=r["zs"], vscale=vscale, a_B=a_B, b_B=b_B, V_Q=V_Q, phi=phi, x_B=x_B, v_B=v_B,
               flag=r["flag"], log_p=r["log_p"], a_w=r["a_w"], s_B=r["s"], burden_chi2_norm=b_B * b_B / a_B)
    # 5. the tests
    out.update(tests_on(t, A, rho, method))
    return out
