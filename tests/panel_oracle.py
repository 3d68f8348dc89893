"""The un-whitened oracle of the phenotype panels (tests/test_panel_api.py, tests/test_gpu_panel.py): per trait and marker, GLS
of y_t on [C, g~] with the dense inv(V) -- the formula of tests/test_gpu_assoc.py::_oracle for T traits; it shares nothing with
the code under test.  For scale="profile" V is scaled by s_t = y_t' P_V y_t / (n - c) with the explicit dense P_V."""
import numpy as np

MONO, ALLMISS, FULL, ENDS = 0, 1, 2, 3   # the overwritten markers


def markers(n, m, seed):
    """binomial(2, MAF), MAF uniform 0.05-0.5, 2 % missing (-1); four markers overwritten with the edge cases."""
    rng = np.random.default_rng(seed)
    maf = rng.uniform(0.05, 0.5, m)
    G = rng.binomial(2, maf[:, None], size=(m, n)).astype(np.int8)
    G[rng.random((m, n)) < 0.02] = -1
    G[MONO] = 1                                   # monomorphic
    G[ALLMISS] = -1                               # nothing observed
    G[FULL] = rng.binomial(2, 0.3, n)             # no missing value
    G[ENDS] = rng.binomial(2, 0.3, n)
    G[ENDS, 0] = G[ENDS, -1] = -1                 # missing at the first and the last individual only
    return np.ascontiguousarray(G)


def centred(G):
    obs = G >= 0
    n_obs = obs.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(obs, G, 0).sum(axis=1) / n_obs
    Gt = np.where(obs, G - np.where(n_obs > 0, mean, 0.0)[:, None], 0.0)
    return n_obs, mean, Gt


def traits(n, Cv, T, seed):
    """T phenotypes with different covariate effects and noise levels."""
    rng = np.random.default_rng(seed)
    return Cv @ rng.standard_normal((Cv.shape[1], T)) + rng.standard_normal((n, T)) * rng.uniform(0.5, 2.0, T)


def gls(Vi, Cv, Y, G, scale):
    """beta, se, chi2 (m x T) of the last coefficient of GLS of y_t on [C, g~] under V (scale="fixed") or under s_t V
    (scale="profile"), marker by marker and trait by trait; n_obs, mean (m); s_t (T)."""
    n, c = Cv.shape
    T, m = Y.shape[1], len(G)
    n_obs, mean, Gt = centred(G)
    ViC = Vi @ Cv
    PV = Vi - ViC @ np.linalg.solve(Cv.T @ ViC, ViC.T)
    s = np.einsum("it,ij,jt->t", Y, PV, Y) / (n - c) if scale == "profile" else np.ones(T)
    ViG, ViY = Vi @ Gt.T, Vi @ Y
    beta, se = np.full((m, T), np.nan), np.full((m, T), np.nan)
    for j in range(m):
        if n_obs[j] == 0 or not Gt[j].any():
            continue
        X = np.hstack([Cv, Gt[j][:, None]])
        XtViX = X.T @ np.hstack([ViC, ViG[:, j][:, None]])
        XtViY = X.T @ ViY
        Mt = XtViX[None] / s[:, None, None]                   # inv(s_t V) = Vi / s_t: one (c + 1) x (c + 1) system per trait
        beta[j] = np.linalg.solve(Mt, (XtViY / s).T[:, :, None])[:, -1, 0]
        se[j] = np.sqrt(np.linalg.inv(Mt)[:, -1, -1])
    return dict(beta=beta, se=se, chi2=(beta / se) ** 2, n_obs=n_obs, mean=mean, scale=s)
