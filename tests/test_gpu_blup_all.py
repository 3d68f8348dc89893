"""Whole-cohort BLUP from the selected inverse (``BLUP.reliability_all``, ``.prediction_error_covariance``, ``.leave_one_out``)
against the column path of the same object and against the dense oracles of tests/blup_oracle.py (Henderson's mixed-model
equations, the dense P_V form), which share nothing with the identities under test; leave-one-out against refits written here
from dense NumPy.

Tolerance: the project's 1e-9 relative max-norm (tests.helpers.rel_err), the bar of tests/test_gpu_blup.py.  Every comparison
prints its measured error."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import blup_oracle as O
from tests.helpers import random_spd, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-9
S2 = (0.4, 0.6)
S2_K3 = (0.3, 0.1, 0.6)

_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _CACHE.clear()


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _g1():
    def make():
        A, Cv, y, _ = O.golden_g1()
        n = A.shape[0]
        w = np.random.default_rng(21).uniform(0.5, 2.0, n)
        return dict(A=A, D=O.golden_dominance(A.shape), I=sp.identity(n, format="csr"), W=sp.diags(1.0 / w).tocsr(), C=Cv, y=y, n=n)
    return _once("g1", make)


def _spd():
    def make():
        A = random_spd(300, 0.05, 3)
        n = A.shape[0]
        rng = np.random.default_rng(11)
        Cv = np.hstack([np.ones((n, 1)), rng.standard_normal((n, 3))])
        y = Cv @ np.array([0.5, -0.2, 0.1, 0.3]) + rng.standard_normal(n)
        return dict(A=A, I=sp.identity(n, format="csr"), C=Cv, y=y, n=n)
    return _once("spd", make)


def _pv(name, p, mats, s2):
    return _once(("pv", name, mats, s2), lambda: O.DensePV([p[m] for m in mats], s2, p["C"], p["y"]))


def _blup(p, mats, s2, chol=None, **kw):
    from scilmm_amd import BLUP, SparseCholesky
    chol = chol or SparseCholesky(**kw)
    return BLUP(chol, [p[m] for m in mats], s2, p["C"], p["y"]), chol


def _close(what, got, ref, tol=TOL):
    e = rel_err(got, ref)
    print(what, "rel.err", e)
    assert e < tol, what


def _check(out, u, pev, what):
    _close(what + " u", out["u"], u)
    _close(what + " pev", out["pev"], pev)
    assert np.all(out["reliability"] >= 0) and np.all(out["reliability"] < 1), what


@pytest.mark.parametrize("name", ["g1", "spd"])
def test_total_against_the_column_path_and_the_dense_projection(name):
    p = _g1() if name == "g1" else _spd()
    u, pev = _pv(name, p, "AI", S2).columns("total")
    blup, _ = _blup(p, "AI", S2)
    cols = blup.reliability("total")                              # one sweep column per individual: the path before
    out = blup.reliability_all("total")
    _check(out, u, pev, name + " vs DensePV:")
    _check(out, cols["u"], cols["pev"], name + " vs reliability():")
    _close("self_rel", out["self_rel"], cols["self_rel"], 1e-15)
    _close("reliability", out["reliability"], cols["reliability"])
    assert sorted(out) == sorted(cols)


def test_one_relationship_matrix_k0_against_hendersons_equations():
    p = _g1()
    beta, u, pev = _once("hend", lambda: O.henderson(p["A"], p["C"], p["y"], S2[0], S2[1]))
    blup, _ = _blup(p, "AI", S2)
    out = blup.reliability_all(0)
    _close("beta", blup.beta, beta)
    _check(out, u, pev, "k = 0 vs Henderson:")
    assert np.array_equal(out["self_rel"], p["A"].diagonal())
    _close("reliability", out["reliability"], 1.0 - pev / (S2[0] * p["A"].diagonal()))
    tot = blup.reliability_all("total")                           # the cached pass: the same numbers, other scaling of self_rel
    assert np.array_equal(tot["pev"], out["pev"]) and np.array_equal(tot["u"], out["u"])
    _close("total self_rel", tot["self_rel"], S2[0] * out["self_rel"], 1e-15)


def test_three_components_total_and_the_refusal_of_a_single_one():
    p = _g1()
    pv = _pv("g1", p, "ADI", S2_K3)
    blup, _ = _blup(p, "ADI", S2_K3)
    out = blup.reliability_all("total")
    _check(out, *pv.columns("total"), "K = 3 total:")
    _close("self_rel", out["self_rel"], np.diag(pv.covariance("total")))
    for k in (0, 1):
        with pytest.raises(ValueError, match=r"reliability\(%d\)" % k):
            blup.reliability_all(k)
    ids = np.arange(0, p["n"], 37)
    _check(blup.reliability(0, ids), pv.columns(0)[0][ids], pv.columns(0)[1][ids], "K = 3, k = 0 on the column path afterwards:")


def test_weighted_residuals():
    """The last matrix diag(1 / w), w in [0.5, 2]: e_i differs from individual to individual."""
    p = _g1()
    pv = _pv("g1", p, "AW", S2)
    blup, _ = _blup(p, "AW", S2)
    _check(blup.reliability_all("total"), *pv.columns("total"), "record weights:")
    loo = blup.leave_one_out()
    _close("leverage", loo["leverage"], np.diag(pv.P))
    _close("residual", loo["residual"], pv.Py / np.diag(pv.P))


@pytest.mark.parametrize("case", ["g1-AI", "g1-ADI", "spd-AI"])
def test_prediction_error_covariance_on_the_pattern(case):
    name, mats = case.split("-")
    p = _g1() if name == "g1" else _spd()
    s2 = S2 if len(mats) == 2 else S2_K3
    pv = _pv(name, p, mats, s2)
    G = pv.covariance("total")
    ref = G - G @ pv.P @ G
    blup, _ = _blup(p, mats, s2)
    M = blup.prediction_error_covariance()
    assert sp.isspmatrix_csr(M) and M.shape == ref.shape and abs(M - M.T).max() == 0.0
    stored = sum(abs(p[m]) for m in mats).tocsr()                 # V's pattern
    stored.sort_indices()
    assert np.array_equal(M.indptr, stored.indptr) and np.array_equal(M.indices, stored.indices)
    rows = np.repeat(np.arange(p["n"]), np.diff(M.indptr))
    _close(case + " PEV / PEC on the pattern", M.data, ref[rows, M.indices])
    off = rows != M.indices
    e = np.abs(M.data[off] - ref[rows[off], M.indices[off]]).max() / np.abs(ref[rows[off], M.indices[off]]).max()
    print(case, "off-diagonal alone rel.err", e, "pairs", int(off.sum()) // 2)
    assert e < TOL
    _close("diagonal == reliability_all", M.diagonal(), blup.reliability_all("total")["pev"], 1e-15)
    i, j = rows[off][0], M.indices[off][0]                        # the error variance of a difference of two relatives
    d = np.zeros(p["n"])
    d[i], d[j] = 1.0, -1.0
    _close("difference of two relatives", M[i, i] + M[j, j] - 2 * M[i, j], d @ ref @ d)


def test_leave_one_out_against_refits():
    p = _spd()
    n, Cv, y = p["n"], p["C"], p["y"]
    blup, _ = _blup(p, "AI", S2)
    loo = blup.leave_one_out()
    assert sorted(loo) == ["leverage", "prediction", "residual", "studentized", "variance"]
    V = S2[0] * p["A"].toarray() + S2[1] * np.eye(n)
    ids = [0, 1, 57, 128, 199, 255, 256, 299]
    res, var = [], []
    for i in ids:                                                 # delete the row and the column, refit GLS, predict
        m = np.arange(n) != i
        Vi = np.linalg.inv(V[np.ix_(m, m)])
        CtViC = Cv[m].T @ Vi @ Cv[m]
        b = np.linalg.solve(CtViC, Cv[m].T @ Vi @ y[m])
        w = Vi @ V[m, i]
        res.append(y[i] - (Cv[i] @ b + w @ (y[m] - Cv[m] @ b)))
        d = Cv[i] - Cv[m].T @ w
        var.append(V[i, i] - V[m, i] @ w + d @ np.linalg.solve(CtViC, d))
    _close("leave-one-out residual", loo["residual"][ids], res)
    _close("leave-one-out variance", loo["variance"][ids], var)
    _close("prediction", loo["prediction"][ids], y[ids] - np.array(res))
    _close("studentized", loo["studentized"][ids], np.array(res) / np.sqrt(var))
    _close("studentized^2 variance == residual^2", loo["studentized"] ** 2 * loo["variance"], loo["residual"] ** 2, 1e-14)
    assert np.array_equal(loo["prediction"], y - loo["residual"])
    pv = _pv("spd", p, "AI", S2)
    _close("leverage", loo["leverage"], np.diag(pv.P))
    assert np.all(loo["leverage"] > 0) and np.all(loo["variance"] > 0)


@pytest.mark.parametrize("call", ["reliability_all", "prediction_error_covariance", "leave_one_out"])
def test_factor_restored_afterwards(call):
    from scilmm_amd import AssociationScan
    p = _g1()
    pv = _pv("g1", p, "AI", S2)
    blup, chol = _blup(p, "AI", S2)
    getattr(blup, call)()
    blup._check_factor()                                          # the factor holds this object's sigma2 again
    ids = np.arange(5, p["n"], 41)
    out = blup.reliability(0, ids)
    u, pev = pv.columns(0)
    _check(out, u[ids], pev[ids], "reliability(0) after %s:" % call)
    _close("effects after", blup.effects(0), u)
    scan = AssociationScan(chol, [p["A"], p["I"]], S2, p["C"], p["y"])
    assert scan.factor is blup.factor
    g = np.random.default_rng(2).integers(0, 3, (7, p["n"])).astype(np.int8)
    res = scan(g)
    assert all(np.all(np.isfinite(v)) for v in res.values())
    fresh = AssociationScan(type(chol)(), [p["A"], p["I"]], S2, p["C"], p["y"])(g)     # a factor that was never inverted
    for k in res:
        _close("scan " + k, res[k], fresh[k])


def test_deterministic_handle_restores_the_factor_bit_for_bit():
    import ctypes as C
    import torch
    p = _g1()
    blup, _ = _blup(p, "AI", S2, deterministic=True)
    f, sym, n = blup.factor, blup.sym, p["n"]
    dB = torch.from_numpy(np.random.default_rng(4).standard_normal((n, 7))).cuda()

    def solve():
        dX = torch.empty_like(dB)
        torch.cuda.synchronize()
        f.solve_dev(C.c_void_p(dB.data_ptr()), 7, C.c_void_p(dX.data_ptr()))
        sym.sync()
        return dX.cpu().numpy()

    before, L0 = solve(), f.L()
    a = blup.reliability_all("total")
    after, L1 = solve(), f.L()
    assert np.array_equal(before, after)
    assert np.array_equal(L0.data, L1.data) and np.array_equal(L0.indices, L1.indices)
    assert sym.timing()["n_float_atomic_launches"] == 0
    _check(a, *_pv("g1", p, "AI", S2).columns("total"), "deterministic:")
