"""What tests/test_gxe_api.py and tests/test_gpu_gxe.py share: seeded markers with the edge cases of a marker x environment
scan, environment columns, and the UN-WHITENED oracle -- per-marker GLS of y on [C, g~, g~ o e_1 ..] with a dense inv(V),
which shares nothing with the code under test."""
import numpy as np
import scipy.stats as stats

from tests.helpers import rel_err

TOL = 1e-9                                          # the suite's tolerance for derived statistics (tests/test_gpu_assoc.py)
MONO, ALLMISS, FULL, ENDS, LEVEL = 0, 1, 2, 3, 4    # the overwritten markers
DEGENERATE = (MONO, ALLMISS, LEVEL)
KEYS = ("beta", "se", "cov", "chi2_int", "chi2_joint")


def environment(n, m, seed):
    """n x m: a binary first column (both levels present), standard normal ones after it."""
    rng = np.random.default_rng(seed)
    E = rng.standard_normal((n, m))
    E[:, 0] = rng.permutation(np.arange(n) % 2)
    return E


def markers(n, M, seed, e0):
    """binomial(2, MAF), MAF uniform 0.05-0.5, 2 % missing (-1); five markers overwritten with the edge cases.  LEVEL varies
    only where the binary ``e0`` is 1 and has no missing value: g~ o e0 is then a combination of g~, 1 and e0."""
    rng = np.random.default_rng(seed)
    maf = rng.uniform(0.05, 0.5, M)
    G = rng.binomial(2, maf[:, None], size=(M, n)).astype(np.int8)
    G[rng.random((M, n)) < 0.02] = -1
    G[MONO] = 1                                   # monomorphic
    G[ALLMISS] = -1                               # nothing observed
    G[FULL] = rng.binomial(2, 0.3, n)             # no missing value
    G[ENDS] = rng.binomial(2, 0.3, n)
    G[ENDS, 0] = G[ENDS, -1] = -1                 # missing at the first and the last individual only
    G[LEVEL] = np.where(e0 == 1, rng.binomial(2, 0.3, n), 1)
    return np.ascontiguousarray(G)


def centred(G):
    """n_obs, mean over the observed (NaN without any), g~ = g - mean with missing = 0; int8 or float (non-finite = missing)."""
    obs = G >= 0 if G.dtype.kind == "i" else np.isfinite(G)
    n_obs = obs.sum(axis=1)
    G0 = np.where(obs, G, 0).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = G0.sum(axis=1) / n_obs
    Gt = np.where(obs, G0 - np.where(n_obs > 0, mean, 0.0)[:, None], 0.0)
    return n_obs, mean, Gt


def oracle(Vi, Cv, y, E, G, skip=DEGENERATE):
    """beta (M x d), se, cov (M x d x d) of the marker's d = 1 + m coefficients in GLS of y on [C, g~, g~ o e_1 ..] under V,
    the Wald chi2 of the m interaction coefficients and of all d; NaN for the markers ``skip``."""
    M, c, d = len(G), Cv.shape[1], 1 + E.shape[1]
    n_obs, mean, Gt = centred(G)
    ViC, Viy = Vi @ Cv, Vi @ y
    out = dict(beta=np.full((M, d), np.nan), se=np.full((M, d), np.nan), cov=np.full((M, d, d), np.nan),
               chi2_int=np.full(M, np.nan), chi2_joint=np.full(M, np.nan), n_obs=n_obs, mean=mean)
    for j in range(M):
        if j in skip:
            continue
        Xg = np.column_stack([Gt[j]] + [Gt[j] * E[:, a] for a in range(d - 1)])
        X = np.hstack([Cv, Xg])
        XtViX = X.T @ np.hstack([ViC, Vi @ Xg])
        coef = np.linalg.solve(XtViX, X.T @ Viy)
        cov = np.linalg.inv(XtViX)[c:, c:]
        b = coef[c:]
        out["beta"][j], out["cov"][j], out["se"][j] = b, cov, np.sqrt(np.diag(cov))
        out["chi2_joint"][j] = b @ np.linalg.solve(cov, b)
        out["chi2_int"][j] = b[1:] @ np.linalg.solve(cov[1:, 1:], b[1:])
    return out


def compare(out, ref, n, bad=DEGENERATE):
    """``out`` (the dict of InteractionScan) against the oracle: NaN exactly at ``bad``, the rest at TOL; exact p-values,
    n_obs and (1e-15) mean."""
    M, d = ref["beta"].shape
    isbad = np.zeros(M, bool)
    isbad[list(bad)] = True
    for k in KEYS:
        assert out[k].shape == ref[k].shape, k
        err = rel_err(out[k][~isbad], ref[k][~isbad])
        print(k, "rel.err", err)
        assert err < TOL, (k, err)
        nan = np.isnan(out[k]).reshape(M, -1)
        assert np.array_equal(nan.all(axis=1), isbad) and np.array_equal(nan.any(axis=1), isbad), k
    for k, df in (("int", d - 1), ("joint", d)):
        assert np.array_equal(out["p_" + k], stats.f(df, n - 1).sf(out["chi2_" + k] / df), equal_nan=True), k
        assert np.array_equal(np.isnan(out["p_" + k]), isbad), k
    assert out["n_obs"].dtype.kind == "i" and np.array_equal(out["n_obs"], ref["n_obs"])
    ok = ref["n_obs"] > 0
    assert np.abs(out["mean"][ok] - ref["mean"][ok]).max() <= 1e-15 and np.all(np.isnan(out["mean"][~ok]))
