"""SKAT-O on the host path (scilmm_amd.sets.skato_pvalue) against tests/skato_oracle.py, which works on the n x r matrix Z1 with
the SKAT package's formulas and shares no code with the module; the degenerate rules, the grid's checks, the Bonferroni bound,
the calibration under the null, and the argument checks of scilmm_sets_finish_dev that need no device.

Measured on the CPU when this was written: skato_pvalue against the oracle over r = 2, 5, 17, 40, 128, null and planted t, both
methods: p, pmin and every p_rho within 1.4e-12 relative (bound 1e-9), p from 0.9 down to 1e-123, the case held to T < 1e-30 at
T = 1.3e-41 (r = 17, saddlepoint); the Kolmogorov-Smirnov distance of 1000 null p-values from the uniform law: 0.036
(bound 0.06; the 1 % critical value at N = 1000 is 0.0515), P(p < 0.05) = 0.048."""
import ctypes as C
import inspect

import numpy as np
import pytest

from scilmm_amd import _lib
from scilmm_amd import sets as S
from tests import skato_oracle as O

TOL = 1e-9
SIZES = (2, 5, 17, 40, 128)


def _case(r, planted, seed=1):
    """(Z1, t): a random n x r Z1 with uneven column scales, t = Z1'eps (null) plus `planted` standard deviations per marker."""
    rng = np.random.default_rng([seed, r, planted])
    n = r + 22
    Z = rng.standard_normal((n, r)) * rng.uniform(0.2, 2.0, r)
    t = Z.T @ rng.standard_normal(n)
    if planted:
        t = t + planted * np.sqrt(np.sum(Z * Z, axis=0)) * rng.choice([-1.0, 1.0], r)
    return Z, t


def _dev(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))


@pytest.mark.parametrize("method", S.METHODS)
@pytest.mark.parametrize("r", SIZES)
def test_skato_pvalue_matches_the_z1_oracle(r, method):
    smallest = 1.0
    for planted in (0, 1, 6):
        Z, t = _case(r, planted)
        p, pmin, rho, p_rho = S.skato_pvalue(t, Z.T @ Z, method=method)
        ref = O.skato(Z, t, method=method)
        assert not ref["degenerate"] and ref["p"] > 0
        d = max(_dev(p, ref["p"]), _dev(pmin, ref["pmin"]), _dev(p_rho, ref["p_rho"]))
        print("r", r, method, "planted", planted, "p", p, "T", pmin, "rho", rho, "rel.dev", d)
        assert d < TOL and rho == ref["rho"]
        assert p <= len(S.RHO_DEFAULT) * pmin and pmin == p_rho.min() and pmin <= p <= 1.0
        smallest = min(smallest, pmin)
    if r == 17:
        assert smallest < 1e-30                         # the survival form of the integral holds far below 1e-16


def test_degenerate_sets():
    rng = np.random.default_rng(5)
    # one marker: skat_p exactly, whatever the grid
    A, t = np.array([[2.5]]), np.array([3.1])
    for method in S.METHODS:
        p, pmin, rho, p_rho = S.skato_pvalue(t, A, method=method)
        ref = S.check_method(method)(float(t[0] * t[0]), A.ravel())
        assert p == ref and pmin == ref and rho == 0.0 and np.all(p_rho == ref)
    # rank one: A = b b', t along b; and A 1 = 0 (s11 = 0), t in the range of A
    b = rng.standard_normal(9)
    Q, _ = np.linalg.qr(np.hstack([np.ones((8, 1)), rng.standard_normal((8, 7))]))
    A0 = (Q[:, 1:] * rng.uniform(0.5, 2.0, 7)) @ Q[:, 1:].T
    A0 = 0.5 * (A0 + A0.T)
    for name, A, t in (("rank one", np.outer(b, b), 2.1 * b), ("s11 = 0", A0, A0 @ rng.standard_normal(8))):
        p, pmin, rho, p_rho = S.skato_pvalue(t, A)
        ref = O.skato(O.z1_from_gram(A), t)
        print(name, p, pmin, p_rho, ref["p"])
        assert ref["degenerate"] and p == pmin == p_rho.min() and rho == 0.0 == ref["rho"]
        assert np.max(np.abs(p_rho / p - 1.0)) < 1e-6       # every p_rho is the same up to rounding
        assert _dev(p, ref["p"]) < 1e-6                      # (rounding-sized eigenvalues around the floor: not the 1e-9 of the rest)
    # nothing to test with: NaN
    p, pmin, rho, p_rho = S.skato_pvalue(np.zeros(3), np.zeros((3, 3)))
    assert np.isnan(p) and np.isnan(pmin) and np.isnan(rho) and np.all(np.isnan(p_rho))


def test_the_grid():
    Z, t = _case(5, 1)
    A = Z.T @ Z
    for bad in ([], np.linspace(0, 1, 17), [0.0, 1.5], [-0.1], [0.0, np.nan]):
        with pytest.raises(ValueError, match="rho"):
            S.skato_pvalue(t, A, rho=bad)
        with pytest.raises(ValueError, match="rho"):
            S.check_rho(bad)
    assert S.check_rho(None).tolist() == list(S.RHO_DEFAULT) and len(S.RHO_DEFAULT) == 8
    assert S.check_rho(np.linspace(0, 1, 16)).size == 16
    # 1 is computed as 0.999, and reported as 1
    a, b = S.skato_pvalue(t, A, rho=[0.3, 1.0]), S.skato_pvalue(t, A, rho=[0.3, 0.999])
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[3], b[3])
    assert S.skato_pvalue(t, A, rho=[1.0])[2] == 1.0
    for method in S.METHODS:
        sf = S.check_method(method)
        lam = np.linalg.eigvalsh(A)
        # rho = [0] is SKAT
        p, pmin, rho, p_rho = S.skato_pvalue(t, A, rho=[0.0], method=method)
        skat = sf(float(t @ t), lam[lam > S.LAMBDA_FLOOR * lam.max()])
        assert abs(pmin / skat - 1.0) < 1e-12 and rho == 0.0 and p_rho.shape == (1,) and p <= pmin
        # rho = [1] is the burden end of the family: Q = 0.001 t't + 0.999 (1't)^2 against the eigenvalues of A R_0.999,
        # taken here from the unsymmetric product
        p, pmin, rho, p_rho = S.skato_pvalue(t, A, rho=[1.0], method=method)
        R = 0.001 * np.eye(5) + 0.999 * np.ones((5, 5))
        lam = np.sort(np.linalg.eigvals(A @ R).real)
        burden = sf(0.001 * float(t @ t) + 0.999 * float(t.sum()) ** 2, lam[lam > S.LAMBDA_FLOOR * lam.max()])
        assert abs(pmin / burden - 1.0) < 1e-9 and rho == 1.0 and p <= pmin


def test_liu_params_is_the_matching_of_mixture_sf_liu():
    import scipy.stats as stats
    lam = np.array([3.0, 1.0, 0.5, 0.25])
    c1, c2, a, d, l = S.liu_params(lam)
    # (for positive lam, c3^2 <= c2 c4 by Cauchy-Schwarz: the skewness cannot be matched as well, and d = 0)
    assert c1 == lam.sum() and c2 == np.sum(lam ** 2) and d == 0.0 and l == c2 * c2 / np.sum(lam ** 4) and a == np.sqrt(l)
    q = 9.0
    x = (q - c1) / np.sqrt(2.0 * c2) * (np.sqrt(2.0) * a) + (l + d)
    assert S.mixture_sf_liu(q, lam) == float(stats.chi2.sf(x, l))
    c1, c2, a, d, l = S.liu_params(np.full(6, 0.7))
    assert d == 0.0 and abs(l - 6.0) < 1e-12


def test_calibration_under_the_null():
    """1000 null draws t = Z1'eps for one fixed A (r = 5): the p-values are uniform to the accuracy of the approximation."""
    rng = np.random.default_rng(2012)
    Z = rng.standard_normal((60, 5)) * np.array([1.0, 0.4, 2.0, 0.8, 1.3]) + 0.3 * rng.standard_normal((60, 1))
    A = Z.T @ Z
    N = 1000
    p = np.sort([S.skato_pvalue(Z.T @ rng.standard_normal(60), A)[0] for _ in range(N)])
    ks = max(np.max(np.arange(1, N + 1) / N - p), np.max(p - np.arange(N) / N))
    print("KS distance", ks, "P(p < 0.05)", np.mean(p < 0.05), "P(p < 0.01)", np.mean(p < 0.01))
    assert ks < 0.06


def _fake_tester():
    import scipy.stats as stats
    t = object.__new__(S.VariantSetTest)
    t.c, t.n = 2, 40
    t.R, t.u, t._f = np.array([[2.0, 0.3], [0.0, 1.5]]), np.array([0.2, -0.1]), stats.f(1, 39)
    return t


def test_defaults_keep_the_keys_and_the_new_keywords_add_theirs():
    for f in (S.VariantSetTest.__call__, S.VariantSetTest.test_bed, S.VariantSetTest.test_dosages):
        par = inspect.signature(f).parameters
        assert par["skato"].default is False and par["rho"].default is None and par["finish"].default == "host", f.__name__
    # the host algebra of one set on made-up statistics: first as it always was, then with the grid
    rng = np.random.default_rng(0)
    t, r = _fake_tester(), 4
    X = rng.standard_normal((30, r))
    Sx = np.vstack([np.full(r, 30.0), np.full(r, 0.2), np.ones(r), np.sum(X * X, axis=0), 0.1 * rng.standard_normal((3, r))])
    G = X.T @ X
    out = {k: np.full(1, np.nan) for k in S.KEYS}
    out["n_used"] = np.zeros(1, dtype=np.int64)
    t._one_set(out, 0, Sx, G, "beta", S.mixture_sf_saddlepoint)
    assert sorted(out) == sorted(("n_used", "burden_beta", "burden_se", "burden_chi2", "burden_p", "skat_q", "skat_p"))
    assert out["n_used"][0] == r and 0 < out["skat_p"][0] <= 1
    more = {k: np.full(1, np.nan) for k in S.KEYS + S.SKATO_KEYS[:3]}
    more["n_used"], more["skato_p_rho"] = np.zeros(1, dtype=np.int64), np.full((1, 8), np.nan)
    t._one_set(more, 0, Sx, G, "beta", S.mixture_sf_saddlepoint, S.check_rho(None), "saddlepoint")
    for k in S.KEYS:
        assert np.array_equal(more[k], out[k]), k           # the old numbers: the same bits
    assert 0 < more["skato_pmin"][0] <= more["skato_p"][0] <= 1 and more["skato_rho"][0] in S.RHO_DEFAULT
    assert abs(more["skato_p_rho"][0, 0] / out["skat_p"][0] - 1.0) < 1e-9


def test_run_rejects_its_new_arguments_before_any_device_call():
    t = object.__new__(S.VariantSetTest)
    t.n, t.block = 12, 4
    G = np.random.default_rng(0).integers(0, 3, (6, 12)).astype(np.int8)
    sets = [[0, 1], [5]]
    with pytest.raises(ValueError, match="finish"):
        t(G, sets, finish="gpu")
    with pytest.raises(ValueError, match="return_kernel"):
        t(G, sets, finish="device", return_kernel=True)
    for bad in ([], [2.0], [np.nan], np.linspace(0, 1, 17)):
        with pytest.raises(ValueError, match="rho"):
            t(G, sets, skato=True, rho=bad)


def test_finish_entry_point_checks_its_arguments_first():
    """Dummy non-null device pointers: every argument error is found before anything of the handle or the device is read."""
    from scilmm_amd.factor import Factor
    L = _lib.lib()
    assert "scilmm_sets_finish_dev" in _lib.SYMBOLS and hasattr(L, "scilmm_sets_finish_dev") and callable(Factor.sets_finish_dev)
    one = C.c_void_p(8)
    start = np.array([0, 2, 5], dtype=np.int32)
    rho = np.array([0.0, 0.5, 1.0])
    good = dict(fac=one, r=5, q=3, stats=one, gram=one, R=one, u=one, c=2, n_sets=2, start=_lib.ptr(start), mode=0, w=None, method=0,
                rho=_lib.ptr(rho), n_rho=3, out=one, ld=13, lam=None)

    def call(**kw):
        a = dict(good, **kw)
        return L.scilmm_sets_finish_dev(*[a[k] for k in good])

    bad_start = [np.array(v, dtype=np.int32) for v in ([1, 2, 5], [0, 2, 6], [0, 2, 2], [0, 3, 2])]
    bad_rho = [np.array(v) for v in ([0.0, 1.5, 1.0], [0.0, -0.1, 1.0], [0.0, np.nan, 1.0])]
    cases = [dict(fac=None), dict(stats=None), dict(gram=None), dict(R=None), dict(u=None), dict(start=None), dict(out=None),
             dict(rho=None), dict(r=0), dict(r=129), dict(c=0, q=1), dict(c=32, q=33), dict(q=4), dict(n_sets=0), dict(n_sets=6),
             dict(n_rho=-1), dict(n_rho=17), dict(ld=12), dict(mode=3), dict(mode=-1), dict(mode=2, w=None), dict(method=2)]
    cases += [dict(start=_lib.ptr(v)) for v in bad_start] + [dict(rho=_lib.ptr(v)) for v in bad_rho]
    for kw in cases:
        assert call(**kw) == _lib.ERR_ARG, kw
