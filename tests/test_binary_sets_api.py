"""Variant-set tests for binary traits without a device: the argument checks of scilmm_amd.glmm.BinarySetTest (which raise before
any device call), the host algebra of step 5 (scilmm_amd.binary_sets.scaled_tests) on a made-up (s, K, w, vscale) against
tests/setspa_oracle.py, the log p -> normal deviate inverse against SciPy, and the argument checks of the four new entry points
on dummy pointers (this last test needs the built library, not a device)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import scipy.special as sc
import scipy.stats as stats

from scilmm_amd import binary_sets as B
from scilmm_amd import glmm
from scilmm_amd import sets as S
from tests import setspa_oracle as SO


def test_normal_deviate_inverts_the_two_sided_tail():
    lp = -np.logspace(-3, 4, 71)
    v = B.normal_deviate(lp)
    assert v.shape == lp.shape and np.all(np.diff(v) > 0)
    rep = lp > -600                                                         # where p itself is representable: SciPy's inverse
    want = -sc.ndtri(0.5 * np.exp(lp[rep]))
    assert np.max(np.abs(v[rep] - want) / want) < 1e-12
    assert np.max(np.abs(np.sqrt(2.0) * sc.erfcinv(np.exp(lp[rep])) - v[rep]) / v[rep]) < 1e-10
    # beyond: log(2 Phi(-v)) through log_ndtr, which does not underflow (the sum itself rounds at an ulp of max(log 2, |log p|))
    back = np.log(2.0) + sc.log_ndtr(-v)
    assert np.all(np.abs(back - lp) < 2e-15 * np.maximum(1.0, np.abs(lp)))
    for x in lp[::10]:
        assert abs(SO.deviate(x) - B.normal_deviate(x)) < 1e-12 * SO.deviate(x)   # the oracle's own inverse
    assert float(B.normal_deviate(np.log(stats.chi2.sf(3.3 ** 2, 1)))) == pytest.approx(3.3, rel=1e-13)
    out = B.normal_deviate([0.0, 1e-3, np.nan, -np.inf, -1.0])
    assert np.all(np.isnan(out[:3])) and out[3] == np.inf and np.isfinite(out[4])


def _made_up(k, seed):
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((k + 6, k)) * rng.uniform(0.3, 1.7, k)
    K = Z.T @ Z
    ev, U = np.linalg.eigh(K)
    s = (U * np.sqrt(ev)) @ rng.standard_normal(k) * 1.6
    return s, K, rng.uniform(0.5, 2.0, k), rng.uniform(0.8, 1.3, k)


@pytest.mark.parametrize("k,method", [(1, "saddlepoint"), (2, "saddlepoint"), (7, "saddlepoint"), (7, "liu"), (17, "saddlepoint")])
def test_scaled_tests_match_the_oracle(k, method):
    s, K, w, vs = _made_up(k, 40 + k)
    rho = np.array(SO.KO.RHO)
    got = B.scaled_tests(s, K, w, vs, method, rho)
    ws = w * vs
    want = SO.tests_on(w * s, ws[:, None] * K * ws[None, :], rho, method)
    for key in ("burden_beta", "burden_se", "burden_chi2", "skat_q"):
        assert got[key] == pytest.approx(want[key], rel=1e-12), key
    assert got["skat_p"] == pytest.approx(want["skat_p"], rel=1e-6)
    p, pmin, r0, p_rho = got["skato"]
    assert p == pytest.approx(want["skato_p"], rel=1e-6) and pmin == pytest.approx(want["skato_pmin"], rel=1e-6)
    assert r0 == want["skato_rho"] and np.allclose(p_rho, want["skato_p_rho"], rtol=1e-6, atol=0)
    # t keeps w: the scales enter A alone
    plain = B.scaled_tests(s, K, w, np.ones(k), method, rho)
    assert plain["skat_q"] == got["skat_q"] and plain["burden_chi2"] != got["burden_chi2"]
    assert B.scaled_tests(s, K, w, vs, method)["skato"] is None
    # a common factor f on the scales divides the burden's chi2 by f^2: what the burden floor does
    f = 1.7
    assert B.scaled_tests(s, K, w, f * vs, method)["burden_chi2"] == pytest.approx(got["burden_chi2"] / f ** 2, rel=1e-13)


def _shell():
    t = object.__new__(glmm.BinarySetTest)
    t.n, t.block, t.c, t.cutoff = 12, 4, 1, 2.0
    return t


def test_run_rejects_its_arguments_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device side was reached")
    monkeypatch.setattr(glmm._lib, "lib", no_device)
    t = _shell()
    monkeypatch.setattr(t, "_check_factor", no_device, raising=False)
    G = np.random.default_rng(0).integers(0, 3, (6, 12)).astype(np.int8)
    sets = [[0, 1], [5]]
    for kw in (dict(sets=[[0, 6]]), dict(sets=[[0, 0]]), dict(sets=[[0, 1, 2, 3, 4]]), dict(sets=[[]]), dict(sets=[[0.5]]),
               dict(weights="gamma"), dict(weights=[np.ones(2)]), dict(weights=[np.ones(2), np.array([np.nan])]), dict(method="davies"),
               dict(skato=True, rho=[0.0, 1.5]), dict(skato=True, rho=[]), dict(finish="gpu"), dict(finish="device", return_kernel=True)):
        a = dict(dict(sets=sets), **kw)
        with pytest.raises(ValueError):
            t(G, a.pop("sets"), **a)
    with pytest.raises(ValueError):
        t(G[:, :11], sets)                                                   # markers of another cohort
    # the constructor: cutoff and covariates are checked before the model's device side is built
    n = 12
    import scipy.sparse as sp
    null = glmm.LogisticMixedModel(None, [sp.identity(n, format="csr")], np.ones((n, 1)), np.r_[np.ones(4), np.zeros(n - 4)]).null_at(
        [0.3], [-0.7], np.zeros(n))
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            null.sets(cutoff=bad)
    for bad_C in (np.ones((n, 0)), np.ones((n, 32)), np.ones((n - 1, 1)), np.ones(n)):
        with pytest.raises(ValueError):
            glmm.BinarySetTest(None, null, bad_C)


def test_the_interface_is_the_variant_set_tests():
    for name in ("__call__", "test_bed", "test_dosages"):
        assert inspect.signature(getattr(glmm.BinarySetTest, name)) == inspect.signature(getattr(S.VariantSetTest, name)), name
    assert issubclass(glmm.BinarySetTest, S.VariantSetTest) and hasattr(glmm.NullModel, "sets")
    par = inspect.signature(glmm.NullModel.sets).parameters
    assert par["block"].default is None and par["cutoff"].default == 2.0
    assert "variant-set and G x E" not in glmm.__doc__ and "G x E" in glmm.__doc__
    assert S.KEYS == ("n_used", "burden_beta", "burden_se", "burden_chi2", "burden_p", "skat_q", "skat_p")     # VariantSetTest's keys stay


def test_exports_and_entry_points_reject_bad_arguments_before_any_device_state():
    from scilmm_amd import _lib
    from scilmm_amd.factor import Factor, Symbolic
    from scilmm_amd.markers import BedRows, DosageRows, Int8Rows
    for name in ("sets_spa_dev", "sets_spa_bed_dev", "sets_spa_dosage_dev", "sets_finish_scaled_dev", "sets_spa_timing"):
        assert hasattr(Factor, name) and "scilmm_" + name in _lib.SYMBOLS
    assert hasattr(Symbolic, "sets_spa_timing") and "scilmm_sets_spa_timing" in _lib.SYMBOLS
    assert all(hasattr(k, "sets_spa") for k in (Int8Rows, BedRows, DosageRows))
    L = _lib.lib()
    vp = C.c_void_p
    ARG, one = _lib.ERR_ARG, vp(8)
    hollow = C.create_string_buffer(256)            # a scilmm_factor with sym == NULL
    fac = C.cast(hollow, vp)
    start = np.array([0, 2, 4], dtype=np.int32)
    ps = _lib.ptr(start)
    # d_stats, d_gram, d_R, d_u, d_mu, d_C, c, d_Minv, cutoff, d_spa, n_sets, set_start, weight_mode, d_weights, d_bspa, d_vscale
    good = [one, one, one, one, one, one, 1, one, 2.0, one, 2, ps, 1, None, one, one]
    bad_start = [np.array(v, dtype=np.int32) for v in ([1, 2, 4], [0, 2, 5], [0, 2, 2], [0, 3, 2])]
    forms = [(L.scilmm_sets_spa_dev, [one, 16]), (L.scilmm_sets_spa_bed_dev, [one, 4, 16, None, 0]),
             (L.scilmm_sets_spa_dosage_dev, [one, _lib.DOSAGE_F32, 16, 16, None])]
    for fn, head in forms:
        assert fn(None, *head, 4, *good) == ARG and fn(fac, *head, 4, *good) == ARG               # no handle
        assert fn(one, None, *head[1:], 4, *good) == ARG                                          # no marker rows
        for r in (0, 129, -1):
            assert fn(one, *head, r, *good) == ARG
        cases = [(i, None) for i in (0, 1, 2, 3, 4, 5, 7, 9, 11, 14, 15)]
        cases += [(6, 0), (6, 32), (8, -0.5), (8, float("nan")), (10, 0), (10, 5), (12, 3), (12, -1), (12, 2)]
        cases += [(11, _lib.ptr(v)) for v in bad_start]
        for k, bad in cases:
            args = list(good)
            args[k] = bad
            assert fn(one, *head, 4, *args) == ARG, (fn.__name__, k, bad)
    assert L.scilmm_sets_spa_bed_dev(one, one, 3, 16, None, 0, 4, *good) == ARG                   # pitch shorter than a packed row
    assert L.scilmm_sets_spa_bed_dev(one, one, 4, 16, None, 4, 4, *good) == ARG                   # an unknown flag
    assert L.scilmm_sets_spa_dosage_dev(one, one, 9, 16, 16, None, 4, *good) == ARG               # an unknown element type
    # the scaled finish: its twin's checks, and the scales
    rho = np.array([0.0, 1.0])
    fin = [4, 2, one, one, one, one, 1, 2, ps, 1, None, 0, _lib.ptr(rho), 2, one, 12, None]
    assert L.scilmm_sets_finish_scaled_dev(one, *fin, None) == ARG                                # no scales
    assert L.scilmm_sets_finish_scaled_dev(None, *fin, one) == ARG and L.scilmm_sets_finish_scaled_dev(fac, *fin, one) == ARG
    for k, bad in ((0, 0), (0, 129), (1, 3), (2, None), (3, None), (7, 0), (8, None), (9, 3), (11, 2), (13, 17), (14, None), (15, 11)):
        args = list(fin)
        args[k] = bad
        assert L.scilmm_sets_finish_scaled_dev(one, *args, one) == ARG, (k, bad)
    n = 6
    import scipy.sparse as sp
    A = (sp.diags([np.full(n - 1, 0.25), np.full(n, 2.0), np.full(n - 1, 0.25)], [-1, 0, 1])).tocsr()
    sym = Symbolic([A, sp.identity(n, format="csr")], upload=False)
    dbl = (C.c_double * 1)()
    assert L.scilmm_sets_spa_timing(None, dbl) == ARG and L.scilmm_sets_spa_timing(sym._h, dbl) == ARG   # no device state
    assert L.scilmm_sets_spa_timing(sym._h, None) == ARG
    assert L.scilmm_get_deterministic(sym._h, C.pointer(C.c_int32())) == _lib.OK                  # the handle is still usable
