"""Dense NumPy / SciPy oracle of the binary-trait path (scilmm_amd.glmm): the PQL fit of the logistic mixed model with dense
``inv(V)``, the un-whitened score statistics, and the saddlepoint p-value with ``scipy.optimize.brentq`` roots.  Nothing here
uses the library; the formulas are written as DESIGN.md section 18 states them, not as the kernel evaluates them."""
import numpy as np
import scipy.linalg as la
import scipy.optimize as opt
import scipy.special as sc
import scipy.stats as stats

MONO, ALLMISS, MISS30 = 3, 5, 9      # rows of markers(): monomorphic, all missing, 30 % missing
ASSOC = (12, 40, 77)                 # rows that phenotype() gives an effect


def markers(n, m, seed):
    """m x n int8 markers with minor allele frequencies from 0.005 to 0.3 and the three edge cases."""
    rng = np.random.default_rng(seed)
    maf = np.exp(rng.uniform(np.log(0.005), np.log(0.3), m))
    G = rng.binomial(2, maf[:, None], size=(m, n)).astype(np.int8)
    for j in range(m):                               # (a rare marker that happened not to vary gets two carriers)
        if j != MONO and G[j].max() == G[j].min():
            G[j, rng.choice(n, 2, replace=False)] = 1
    G[MONO] = 0
    G[ALLMISS] = -1
    G[MISS30, rng.random(n) < 0.3] = -1
    for j in ASSOC:
        G[j] = rng.binomial(2, 0.2, n)
    return G


def phenotype(A, C, G, prevalence, tau, seed, effect=1.2):
    """0/1 phenotypes of about the given prevalence: logit = intercept + covariates + a random effect N(0, tau A) + the markers ASSOC."""
    rng = np.random.default_rng(seed)
    n = C.shape[0]
    u = np.linalg.cholesky(A.toarray() + 1e-10 * np.eye(n)) @ rng.standard_normal(n) * np.sqrt(tau)
    eta = u + 0.3 * (C[:, 1:] @ rng.standard_normal(C.shape[1] - 1)) if C.shape[1] > 1 else u.copy()
    for j in ASSOC:
        g = G[j].astype(float)
        eta = eta + effect * (g - g.mean())
    off = opt.brentq(lambda o: sc.expit(eta + o).mean() - prevalence, -30, 30)
    return (rng.random(n) < sc.expit(eta + off)).astype(float)


def logistic(C, y, tol=1e-12, max_iter=100):
    """Covariate-only logistic regression by IRLS."""
    alpha = np.zeros(C.shape[1])
    for _ in range(max_iter):
        mu = sc.expit(C @ alpha)
        w = mu * (1 - mu)
        new = la.solve((C.T * w) @ C, C.T @ (w * (C @ alpha) + y - mu), assume_a="pos")
        done = np.abs(new - alpha).max() <= tol * max(1.0, np.abs(new).max())
        alpha = new
        if done:
            break
    return alpha


def fit(A_list, C, y, tau0=None, tol=1e-8, max_iter=100):
    """PQL as GMMAT's glmmkin runs it for a binomial family with dispersion 1, dense."""
    A = [np.asarray(a.toarray() if hasattr(a, "toarray") else a, dtype=float) for a in A_list]
    K1, n = len(A), y.size
    tau = np.full(K1, 0.5) if tau0 is None else np.array(tau0, dtype=float)
    alpha, b = logistic(C, y), np.zeros(n)
    converged, it = False, 0
    for it in range(1, max_iter + 1):
        eta = C @ alpha + b
        mu = sc.expit(eta)
        w = mu * (1 - mu)
        yt = eta + (y - mu) / w

        def parts(t):
            Vi = la.inv(np.diag(1 / w) + sum(tk * a for tk, a in zip(t, A)))
            ViC = Vi @ C
            return Vi, ViC, la.inv(C.T @ ViC)

        Vi, ViC, M = parts(tau)
        P = Vi - ViC @ M @ ViC.T
        Py = P @ yt
        free = np.flatnonzero(tau > 0)
        new = tau.copy()
        if free.size:
            APy = [A[k] @ Py for k in free]
            score = np.array([Py @ v - np.sum(P * A[k]) for k, v in zip(free, APy)])
            AI = np.array([[u @ (P @ v) for v in APy] for u in APy])
            step, t = la.solve(AI, score), 1.0
            for _ in range(64):
                if np.all(tau[free] + t * step >= 0):
                    break
                t *= 0.5
            else:
                t = 0.0
            new[free] = tau[free] + t * step
        new[(new < tol) & (tau < tol)] = 0.0
        X = la.solve(np.diag(1 / w) + sum(tk * a for tk, a in zip(new, A)), np.column_stack([C, yt]), assume_a="pos")
        alpha_new = la.solve(C.T @ X[:, :-1], C.T @ X[:, -1], assume_a="pos")
        r = X[:, -1] - X[:, :-1] @ alpha_new
        b = sum(tk * (a @ r) for tk, a in zip(new, A))
        crit = max(np.max(np.abs(alpha_new - alpha) / (np.abs(alpha_new) + np.abs(alpha) + tol)),
                   np.max(np.abs(new - tau) / (new + tau + tol)))
        alpha, tau = alpha_new, new
        if crit < tol:
            converged = True
            break
    eta = C @ alpha + b
    mu = sc.expit(eta)
    w = mu * (1 - mu)
    return dict(tau=tau, alpha=alpha, b=b, eta=eta, mu=mu, weights=w, working_y=eta + (y - mu) / w, n_iter=it, converged=converged,
                boundary=bool(np.any(tau == 0)))


def centred(G):
    """(g~ rows as float64 with the missing mean-imputed, n_obs, mean) of int8 markers or of float dosages (NaN = missing)."""
    G = np.asarray(G)
    miss = (G < 0) if G.dtype.kind in "iu" else ~np.isfinite(G)
    Gf = np.where(miss, 0.0, G.astype(float))
    n_obs = (~miss).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = Gf.sum(axis=1) / n_obs
    Gt = np.where(miss, 0.0, Gf - np.where(n_obs > 0, mean, 0.0)[:, None])
    return Gt, n_obs, mean


def score(A_list, tau, C, mu, working_y, G):
    """The un-whitened score statistics at a fitted null: per marker a = g~'P g~, b = g~'P y~ (P of V = W^-1 + sum tau_k A_k), the
    covariate-adjusted rows g^ = g~ - C (C'WC)^-1 C'W g~ and a_w = sum w g^^2; NaN in a, b for a marker without an observed value or
    without variation."""
    A = [np.asarray(a.toarray() if hasattr(a, "toarray") else a, dtype=float) for a in A_list]
    w = mu * (1 - mu)
    Vi = la.inv(np.diag(1 / w) + sum(tk * a for tk, a in zip(tau, A)))
    ViC = Vi @ C
    P = Vi - ViC @ la.solve(C.T @ ViC, ViC.T)
    Gt, n_obs, mean = centred(G)
    bad = (n_obs == 0) | (np.abs(Gt).max(axis=1) == 0)
    PG = P @ Gt.T
    a = np.where(bad, np.nan, np.sum(Gt.T * PG, axis=0))
    b = np.where(bad, np.nan, working_y @ PG)
    Gh = Gt - (la.solve((C.T * w) @ C, (C.T * w) @ Gt.T).T @ C.T)
    return dict(a=a, b=b, a_w=(Gh * Gh) @ w, gh=Gh, n_obs=n_obs, mean=mean, bad=bad)


def cgf(gh, mu, t):
    """K(t), K'(t), K''(t) of T = sum gh_i (y_i - mu_i), y_i ~ Bernoulli(mu_i) independent."""
    m1 = gh @ mu
    x = gh * t
    K = np.sum(np.logaddexp(np.log1p(-mu), np.log(mu) + x)) - t * m1
    p = sc.expit(sc.logit(mu) + x)
    return K, gh @ p - m1, (gh * gh) @ (p * (1 - p))


def root_brentq(gh, mu, q):
    """zeta with K'(zeta) = q (brentq, xtol 1e-14), None when q lies outside the support of T."""
    m1 = gh @ mu
    lim = (np.sum(gh[gh > 0]) if q > 0 else np.sum(gh[gh < 0])) - m1
    if not abs(q) < abs(lim):
        return None
    f = lambda t: cgf(gh, mu, t)[1] - q
    hi = np.sign(q) * 1e-3
    while f(hi) * np.sign(q) < 0:
        hi *= 2.0
        if abs(hi) > 1e12:
            return None
    return opt.brentq(f, 0.0, hi, xtol=1e-14, rtol=4 * np.finfo(float).eps, maxiter=500)


def root_newton(gh, mu, q, tol=1e-13, max_iter=64):
    """The same root by safeguarded Newton from 0 (the kernel's iteration): (zeta, iterations) or (None, iterations)."""
    sg = 1.0 if q > 0 else -1.0
    lo, hi, y = 0.0, np.inf, 0.0
    for it in range(1, max_iter + 1):
        _, k1, k2 = cgf(gh, mu, sg * y)
        f = sg * k1 - abs(q)
        if f < 0:
            lo = y
        else:
            hi = y
        with np.errstate(divide="ignore", invalid="ignore"):
            yn = y - f / k2
        if not (lo < yn < hi):
            yn = 0.5 * (lo + hi)
        if not np.isfinite(yn):
            return None, it
        dy, y = abs(yn - y), yn
        if dy <= tol * max(1.0, y):
            return sg * y, it
    return None, max_iter


def spa(gh, mu, s, zs=None):
    """The two-sided saddlepoint p-value of the score s: dict of log_p, flag (1: both roots and both tail arguments fine; 2: the
    normal value log(2 Phi(-|zs|)) instead), zeta_hi, zeta_lo."""
    tails, zeta = [], []
    for q in (abs(s), -abs(s)):
        z = root_brentq(gh, mu, q)
        zeta.append(np.nan if z is None else z)
        if z is None:
            continue
        K, K1, K2 = cgf(gh, mu, z)
        with np.errstate(divide="ignore", invalid="ignore"):
            om = np.sqrt(2 * (z * K1 - K))
            v = om + np.log(abs(z) * np.sqrt(K2) / om) / om
        if np.isfinite(v) and v > 0:
            tails.append(stats.norm.logsf(v))
    if len(tails) == 2:
        return dict(log_p=float(np.logaddexp(*tails)), flag=1, zeta_hi=zeta[0], zeta_lo=zeta[1])
    lp = np.nan if zs is None else float(np.log(2.0) + stats.norm.logsf(abs(zs)))
    return dict(log_p=lp, flag=2, zeta_hi=zeta[0], zeta_lo=zeta[1])


def scan(A_list, null, C, G, cutoff=0.0):
    """What BinaryScan returns, dense: beta, se, chi2, log_p, spa_flag, n_obs, a_w, s, zs per marker."""
    sc_ = score(A_list, null["tau"], C, null["mu"], null["working_y"], G)
    a, b = sc_["a"], sc_["b"]
    m = a.size
    with np.errstate(invalid="ignore", divide="ignore"):
        zs = b / np.sqrt(a)
        s = b * np.sqrt(sc_["a_w"] / a)
    flag, log_p = np.zeros(m, dtype=np.int64), np.full(m, np.nan)
    for j in range(m):
        if sc_["bad"][j] or not a[j] > 0 or not abs(zs[j]) > cutoff:
            continue
        r = spa(sc_["gh"][j], null["mu"], s[j], zs[j])
        flag[j], log_p[j] = r["flag"], r["log_p"]
    return dict(beta=b / a, se=1 / np.sqrt(a), chi2=b * b / a, log_p=log_p, spa_flag=flag, n_obs=sc_["n_obs"], a_w=sc_["a_w"], s=s, zs=zs,
                a=a, b=b, bad=sc_["bad"])
