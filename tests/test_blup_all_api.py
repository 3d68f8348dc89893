"""The whole-cohort BLUP surface without a device: exports, argument checks of ``reliability_all`` /
``prediction_error_covariance`` / ``leave_one_out`` and of ``scilmm_inverse_pattern_dev``, and a pure-NumPy check of the three
identities the device path rests on, against ``G - G P_V G`` and brute-force leave-one-out refits on a
40 x 40 dense problem.  The identities are algebra, so they hold to rounding: 1e-11 on this problem (cond(V) < 1e2)."""
import ctypes as C
import types

import numpy as np
import pytest

from scilmm_amd import _lib
from tests.helpers import rel_err


def test_exports():
    from scilmm_amd import blup
    from scilmm_amd.factor import Factor
    for name in ("selected_inverse", "inverse_pattern_dev", "inverse_on_pattern", "pattern_csr", "inverse_traces"):
        assert callable(getattr(Factor, name)), name
    for name in ("reliability_all", "prediction_error_covariance", "leave_one_out"):
        assert callable(getattr(blup.BLUP, name)), name
    assert "scilmm_inverse_pattern_dev" in _lib.SYMBOLS and hasattr(_lib.lib(), "scilmm_inverse_pattern_dev")


def test_component_argument_needs_no_device():
    from scilmm_amd.blup import check_all_component
    assert check_all_component("total", 2) == "total" and check_all_component("total", 3) == "total"
    assert check_all_component(0, 2) == 0 and check_all_component(np.int64(0), 2) == 0
    for k, K in ((1, 2), (-1, 2), (2, 3), ("all", 2), (0.0, 2), (None, 2), (True, 2)):
        with pytest.raises(ValueError):
            check_all_component(k, K)
    for k in (0, 1):
        with pytest.raises(ValueError, match=r"reliability\(%d\)" % k) as info:
            check_all_component(k, 3)
        assert "pattern" in str(info.value)                           # the reason is named


def _stub(K, last_indices, n=4):
    """A BLUP that never saw a device: what the argument checks of the three methods read, and nothing else."""
    from scilmm_amd.blup import BLUP
    b = BLUP.__new__(BLUP)
    b.n = n
    b.sym = types.SimpleNamespace(K=K, _indices=[np.arange(n, dtype=np.int32)] * (K - 1) + [np.asarray(last_indices, dtype=np.int32)])
    return b


def test_methods_check_their_arguments_before_touching_the_factor():
    k3 = _stub(3, np.arange(4))
    with pytest.raises(ValueError, match="reliability"):
        k3.reliability_all(0)
    with pytest.raises(ValueError):
        _stub(2, np.arange(4)).reliability_all(1)
    with pytest.raises(ValueError):
        _stub(2, np.arange(4)).reliability_all("genetic")
    # a residual covariance that is not diagonal: every one of the three says so
    full = _stub(2, [0, 1, 1, 2, 3])
    for call in (lambda: full.reliability_all("total"), full.prediction_error_covariance, full.leave_one_out):
        with pytest.raises(ValueError, match="diagonal"):
            call()


def test_entry_point_checks_its_arguments_first():
    """Dummy non-null pointers: the argument checks come before any dereference."""
    L = _lib.lib()
    one = C.c_void_p(8)
    for c in (33, -1, 1 << 20):
        assert L.scilmm_inverse_pattern_dev(one, 1.0, one, 1.0, one, c, one, one) == _lib.ERR_ARG, c
    assert L.scilmm_inverse_pattern_dev(one, 1.0, one, 1.0, one, 4, None, None) == _lib.ERR_ARG
    assert L.scilmm_inverse_pattern_dev(None, 1.0, one, 1.0, one, 4, one, one) == _lib.ERR_ARG


def test_the_three_identities_on_a_dense_problem():
    """PEV / PEC / (P_V)_ii from Z, H and T as the device path forms them, against G - G P_V G; the leave-one-out residual
    and its variance against n refits with the row and the column deleted."""
    rng = np.random.default_rng(17)
    n, c = 40, 3
    X = rng.standard_normal((n, n))
    G = 0.5 * (X @ X.T / n + np.eye(n))                               # two components' sum would do as well: G is any SPD
    e = 0.6 / rng.uniform(0.5, 2.0, n)                                # record weights
    V = G + np.diag(e)
    Cv = np.hstack([np.ones((n, 1)), rng.standard_normal((n, c - 1))])
    y = Cv @ np.array([0.5, -0.2, 0.1]) + np.linalg.cholesky(V) @ rng.standard_normal(n)
    Z = np.linalg.inv(V)
    R = np.linalg.cholesky(Cv.T @ Z @ Cv).T                           # R'R = C' V^-1 C
    H = Z @ Cv @ np.linalg.inv(R)
    T = Cv @ np.linalg.inv(R) - e[:, None] * H
    PV = Z - H @ H.T
    PEC_ref = G - G @ PV @ G
    errs = {"G H = T": rel_err(T, G @ H),
            "pev": rel_err(e - e * e * np.diag(Z) + np.sum(T * T, axis=1), np.diag(PEC_ref))}
    PEC = -np.outer(e, e) * Z + T @ T.T
    off = ~np.eye(n, dtype=bool)
    errs["pec"] = np.abs(PEC - PEC_ref)[off].max() / np.abs(PEC_ref).max()
    r = PV @ y
    beta = np.linalg.solve(Cv.T @ Z @ Cv, Cv.T @ Z @ y)
    errs["u"] = rel_err(y - Cv @ beta - e * r, G @ r)
    res, var = np.empty(n), np.empty(n)
    for i in range(n):                                                # brute force: delete, refit GLS, predict
        m = np.arange(n) != i
        Vi = np.linalg.inv(V[np.ix_(m, m)])
        b = np.linalg.solve(Cv[m].T @ Vi @ Cv[m], Cv[m].T @ Vi @ y[m])
        w = Vi @ V[m, i]
        res[i] = y[i] - (Cv[i] @ b + w @ (y[m] - Cv[m] @ b))
        d = Cv[i] - Cv[m].T @ w
        var[i] = V[i, i] - V[m, i] @ w + d @ np.linalg.solve(Cv[m].T @ Vi @ Cv[m], d)
    errs["loo residual"] = rel_err(r / np.diag(PV), res)
    errs["loo variance"] = rel_err(1.0 / np.diag(PV), var)
    print(errs)
    assert max(errs.values()) < 1e-11, errs
