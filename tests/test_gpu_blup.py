"""BLUP (predicted values, prediction error variances, reliabilities) against dense oracles that share nothing with the
whitened formula under test: Henderson's mixed-model equations and the dense P_V form (tests/blup_oracle.py; they agree
with each other to 2e-15, tests/test_blup_api.py).

Tolerance: 1e-9 relative max-norm (tests.helpers.rel_err) -- the marker scan's bar for the same chain of operations (a
forward sweep, column sums, a small triangular solve).  Every comparison prints its measured error."""
import ctypes as C

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


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _g1():
    """The G1 pedigree: n = 1472 (no multiple of 256 or 128), stored columns of 2 to 209 entries."""
    def make():
        A, Cv, y, s2_hat = O.golden_g1()
        n = A.shape[0]
        return dict(A=A, D=O.golden_dominance(A.shape), I=sp.identity(n, format="csr"), C=Cv, y=y, n=n, s2_hat=tuple(s2_hat))
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


def _henderson(s2):
    p = _g1()
    return _once(("hend", s2), lambda: O.henderson(p["A"], p["C"], p["y"], s2[0], s2[1]))


def _pv_g1(s2=S2):
    p = _g1()
    return _once(("pv2", s2), lambda: O.DensePV([p["A"], p["I"]], s2, p["C"], p["y"]))


def _pv_k3():
    p = _g1()
    return _once("pv3", lambda: O.DensePV([p["A"], p["D"], p["I"]], S2_K3, p["C"], p["y"]))


def _blup(p, mats, s2, block=None, chol=None, **kw):
    from scilmm_amd import BLUP, SparseCholesky
    chol = chol or SparseCholesky(**kw)
    return BLUP(chol, [p[m] for m in mats], s2, p["C"], p["y"], block=block), chol


def _close(what, got, ref):
    e = rel_err(got, ref)
    print(what, "rel.err", e)
    assert e < TOL, what


def _check(out, u, pev, ids, what):
    _close(what + " u", out["u"], u[ids])
    _close(what + " pev", out["pev"], pev[ids])
    assert np.all(out["reliability"] >= 0) and np.all(out["reliability"] < 1), what


@pytest.mark.parametrize("which", ["round", "golden"])
def test_g1_pedigree_against_hendersons_equations(which):
    p = _g1()
    s2 = S2 if which == "round" else p["s2_hat"]
    beta, u, pev = _henderson(s2)
    n = p["n"]
    blup, chol = _blup(p, "AI", s2, block=128)
    _close("beta", blup.beta, beta)
    order = np.random.default_rng(5).permutation(n)           # eleven full blocks and one of 64
    out = blup.reliability(0, order)
    _check(out, u, pev, order, "all, block 128:")
    assert np.array_equal(out["self_rel"], p["A"].diagonal()[order])
    _close("reliability", out["reliability"], 1.0 - pev[order] / (s2[0] * p["A"].diagonal()[order]))
    sub = np.random.default_rng(6).choice(n, 100, replace=False)
    blup37, _ = _blup(p, "AI", s2, block=37, chol=chol)      # 37, 37, 26: padded widths 48 and 32
    assert blup37.factor is blup.factor
    _check(blup37.reliability(0, sub), u, pev, sub, "100-subset, block 37:")
    dflt = blup.reliability()                                 # k = 0, everybody, in row order
    _check(dflt, u, pev, np.arange(n), "default arguments:")


@pytest.mark.parametrize("k", [0, 1, "total"])
def test_three_components_against_the_dense_projection(k):
    """K = 3 with the dominance matrix: D stores 1 562 entries on the 36 026-entry pattern, most of its slots hold 0."""
    p = _g1()
    u, pev = _pv_k3().columns(k)
    blup, _ = _once("blup3", lambda: _blup(p, "ADI", S2_K3))
    _close("beta", blup.beta, _pv_k3().beta)
    ids = np.random.default_rng(7).permutation(p["n"])[:300]
    out = blup.reliability(k, ids)
    _check(out, u, pev, ids, "k = %s:" % k)
    G = _pv_k3().covariance(k)
    scale = 1.0 if k == "total" else S2_K3[k]
    _close("self_rel", scale * out["self_rel"], np.diag(G)[ids])


def test_non_pedigree_values_just_over_one_statistics_slice():
    p = _spd()
    pv = _once("pvspd", lambda: O.DensePV([p["A"], p["I"]], S2, p["C"], p["y"]))
    u, pev = pv.columns(0)
    blup, _ = _blup(p, "AI", S2)
    assert blup.c == 4 and p["n"] == 300
    _close("beta", blup.beta, pv.beta)
    _check(blup.reliability(0), u, pev, np.arange(300), "spd300:")
    _close("effects", blup.effects(0), u)


def test_edges_of_the_pattern():
    """The first permuted column is all stored column; the last stores only its diagonal and gets everything else from the
    row pass."""
    p = _g1()
    _, u, pev = _henderson(S2)
    blup, _ = _blup(p, "AI", S2)
    P, n = blup.factor.P(), p["n"]
    for ids in ([P[0]], [P[n - 1]], [P[0], P[n // 2], P[n - 1]], [P[n - 1], P[0]]):
        ids = np.array(ids)
        _check(blup.reliability(0, ids), u, pev, ids, "permuted %s:" % [int(np.flatnonzero(P == i)[0]) for i in ids])
    one, _ = _blup(p, "AI", S2, block=1, chol=None)
    ids = np.array([P[n // 3], P[n - 2], P[1]])
    _check(one.reliability(0, ids), u, pev, ids, "block 1:")


def test_effects_equal_the_block_form_and_the_oracle():
    p = _g1()
    blup, _ = _once("blup3", lambda: _blup(p, "ADI", S2_K3))
    for k in (0, 1, "total"):
        u = _pv_k3().columns(k)[0]
        eff = blup.effects(k)
        _close("effects(%s) vs oracle" % k, eff, u)
        _close("effects(%s) vs reliability" % k, eff, blup.reliability(k)["u"])


def test_predict_offspring_and_an_unrelated_individual():
    p = _g1()
    A, n = p["A"], p["n"]
    rng = np.random.default_rng(8)
    i, j = rng.integers(0, n, 40), rng.integers(0, n, 40)
    rows = sp.vstack([0.5 * (A[i] + A[j]), sp.csr_matrix((1, n))]).tocsr()       # 40 offspring, then an all-zero row
    self_rel = np.concatenate([1.0 + 0.5 * np.asarray(A[i, j]).ravel(), [1.0]])
    u, pev = _pv_g1().rows(rows, self_rel, S2[0])
    blup, _ = _blup(p, "AI", S2, block=16)
    out = blup.predict(rows, self_rel, 0)
    _close("predict u", out["u"], u)
    _close("predict pev", out["pev"], pev)
    assert np.all(out["reliability"][:-1] > 0) and np.all(out["reliability"] < 1)
    assert out["u"][-1] == 0 and out["pev"][-1] == S2[0] * 1.0 and out["reliability"][-1] == 0     # exactly
    assert np.array_equal(out["self_rel"], self_rel)


def test_deterministic_handle_repeats_its_bits_and_rows_equal_columns():
    p = _g1()
    A, n = p["A"], p["n"]
    _, u, pev = _henderson(S2)
    blup, _ = _blup(p, "AI", S2, block=128, deterministic=True)
    S = np.random.default_rng(9).permutation(n)[:150]        # a full block and one of 22
    a, b = blup.reliability(0, S), blup.reliability(0, S)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    _check(a, u, pev, S, "deterministic:")
    rows = blup.predict(A[S], A.diagonal()[S], 0)             # the same columns through the caller-rows entry point
    for k in a:
        assert np.array_equal(a[k], rows[k]), k
    e1, e2 = blup.effects(0), blup.effects(0)
    assert np.array_equal(e1, e2)
    tot = blup.reliability("total", S)
    assert np.array_equal(tot["u"], blup.reliability("total", S)["u"])
    _close("total == k 0 when there is one genetic component", tot["u"], a["u"])
    assert blup.sym.timing()["n_float_atomic_launches"] == 0


def test_state_refusals_and_argument_checks_on_a_live_handle():
    import torch
    from scilmm_amd import ScilmmError, _lib
    p = _spd()
    n = p["n"]
    first, chol = _blup(p, "AI", S2, block=16)
    first.reliability(0, np.arange(5))
    second, _ = _blup(p, "AI", (0.7, 0.3), block=16, chol=chol)
    assert second.factor is first.factor                      # refactorized, not doubled
    for call in (lambda: first.reliability(0, np.arange(5)), lambda: first.effects(0),
                 lambda: first.predict(p["A"][:2], [1.0, 1.0])):
        with pytest.raises(ScilmmError, match="sigma2"):
            call()
    with pytest.raises(ValueError):
        second.reliability(0, [1, 1])
    with pytest.raises(ValueError):
        second.reliability(0, [n])
    with pytest.raises(ValueError):
        second.reliability(2)
    # the C entry point itself: a repeated or out-of-range id is an argument error, and nothing is queued
    L, h, vp = _lib.lib(), second.factor._h, C.c_void_p
    dS = torch.zeros(((second.q + 2) * 4,), dtype=torch.float64, device="cuda")
    w = np.array([1.0, 0.0])
    for ids in ([3, 7, 3, 1], [0, 1, 2, n], [0, -1, 2, 3]):
        ids = np.array(ids, dtype=np.int32)
        rc = L.scilmm_rel_block_dev(h, w.ctypes.data_as(vp), ids.ctypes.data_as(vp), 4, vp(second.dQ.data_ptr()), second.q,
                                    vp(dS.data_ptr()))
        assert rc == _lib.ERR_ARG, ids
    second.sym.sync()
    assert not dS.cpu().numpy().any()
    out = second.reliability(0, np.arange(5))                 # the handle is as it was
    pv = O.DensePV([p["A"], p["I"]], (0.7, 0.3), p["C"], p["y"])
    _check(out, *pv.columns(0), np.arange(5), "after the refused calls:")
    # a factor consumed by the selected inverse: both block calls refuse
    second.factor.inverse_traces()
    with pytest.raises(ScilmmError):
        second.reliability(0, np.arange(5))
    with pytest.raises(ScilmmError):
        second.predict(p["A"][:2], [1.0, 1.0])
    dQ, ids = vp(second.dQ.data_ptr()), np.arange(4, dtype=np.int32)
    with pytest.raises(ScilmmError):
        second.factor.rel_block_dev(w, ids, dQ, second.q, vp(dS.data_ptr()))
    indptr = torch.zeros((5,), dtype=torch.int64, device="cuda")
    idx = torch.zeros((1,), dtype=torch.int32, device="cuda")
    val = torch.zeros((1,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(ScilmmError):
        second.factor.rows_block_dev(vp(indptr.data_ptr()), vp(idx.data_ptr()), vp(val.data_ptr()), 4, dQ, second.q,
                                     vp(dS.data_ptr()))
