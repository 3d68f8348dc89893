"""Binary traits without a device: the dense oracle (tests/spa_oracle.py) against itself -- its two root finders, the saddlepoint
equation, the fixed point of the PQL -- and the argument checks of scilmm_amd.glmm, which raise before any device call.

The cohort is a 459-individual pedigree (small_pedigree(700, 0.01, 0)) with c = 3.  The two phenotype draws are chosen so that the
oracle ALONE converges within 30 iterations, one to an interior tau >= 0.2 and one to the boundary; both conditions are asserted."""
import numpy as np
import pytest
import scipy.sparse as sp

from scilmm_amd import glmm
from tests import spa_oracle as O
from tests.helpers import small_pedigree

M = 40
_CASE = {}


def _case(kind):
    if kind not in _CASE:
        A = small_pedigree(700, 0.01, 0)[0]
        n = A.shape[0]
        rng = np.random.default_rng(11)
        C = np.hstack([np.ones((n, 1)), rng.standard_normal((n, 2))])
        G = O.markers(n, 130, 7)
        prev, seed = {"interior": (0.05, 4), "boundary": (0.10, 1)}[kind]
        y = O.phenotype(A, C, G, prev, 1.0, seed)
        fit = O.fit([A], C, y, tol=1e-9)
        _CASE[kind] = dict(A=A, n=n, C=C, G=G[:M], y=y, fit=fit)
    return _CASE[kind]


def test_oracle_cases_are_what_the_tests_need():
    f = _case("interior")["fit"]
    assert f["converged"] and f["n_iter"] <= 30 and not f["boundary"] and f["tau"][0] >= 0.2, f["tau"]
    f = _case("boundary")["fit"]
    assert f["converged"] and f["n_iter"] <= 30 and f["boundary"] and f["tau"][0] == 0.0, f["tau"]


def test_newton_and_brentq_roots_agree_and_solve_the_saddlepoint_equation():
    p = _case("interior")
    f = p["fit"]
    sc = O.scan([p["A"]], f, p["C"], p["G"])
    seen = 0
    for j in range(M):
        if sc["bad"][j]:
            continue
        gh, s = O.score([p["A"]], f["tau"], p["C"], f["mu"], f["working_y"], p["G"][j:j + 1])["gh"][0], sc["s"][j]
        for q in (abs(s), -abs(s)):
            zb = O.root_brentq(gh, f["mu"], q)
            zn, it = O.root_newton(gh, f["mu"], q)
            assert (zb is None) == (zn is None), (j, q)
            if zb is None:
                continue
            seen += 1
            assert abs(zb - zn) <= 1e-10 * max(1.0, abs(zb)), (j, q, zb, zn)
            assert it <= 64 and zn * q > 0
            for z in (zb, zn):
                _, k1, k2 = O.cgf(gh, f["mu"], z)
                assert abs(k1 - q) <= 1e-9 * np.sqrt(k2), (j, q, k1 - q)
    assert seen >= 2 * (M - 4)


def test_a_score_outside_the_support_has_no_root():
    p = _case("interior")
    f = p["fit"]
    gh = O.score([p["A"]], f["tau"], p["C"], f["mu"], f["working_y"], p["G"][:1])["gh"][0]
    top = np.sum(gh[gh > 0]) - gh @ f["mu"]
    assert O.root_brentq(gh, f["mu"], 1.01 * top) is None and O.root_newton(gh, f["mu"], 1.01 * top)[0] is None
    assert O.spa(gh, f["mu"], 1.01 * top, zs=3.0)["flag"] == 2


@pytest.mark.parametrize("kind", ["interior", "boundary"])
def test_at_the_fixed_point_the_score_is_the_plain_residual_score(kind):
    """g~' P_V y~ = g~'(y - mu^) at the end of the fit: V^-1 (y~ - C alpha) = W (y~ - eta) = y - mu."""
    p = _case(kind)
    f = p["fit"]
    sc = O.score([p["A"]], f["tau"], p["C"], f["mu"], f["working_y"], p["G"])
    Gt = O.centred(p["G"])[0]
    ok = ~sc["bad"]
    plain = Gt[ok] @ (p["y"] - f["mu"])
    gap = np.abs(sc["b"][ok] - plain).max() / np.abs(plain).max()
    print(kind, "tau", f["tau"], "iterations", f["n_iter"], "rel.gap", gap)
    assert gap < 1e-6


def test_binary_stats_host_algebra():
    rng = np.random.default_rng(0)
    c, m = 2, 5
    R = np.triu(rng.uniform(1, 2, (c, c)))
    u = rng.standard_normal(c)
    S = np.vstack([np.full(m, 50.0), rng.uniform(0, 1, m), rng.uniform(1, 2, m), rng.uniform(30, 40, m), rng.standard_normal((c, m)),
                   rng.standard_normal(m)])
    S[0, 1] = 0           # no observed value
    S[2, 2] = 0           # no variation
    SPA = np.full((glmm.SPA_ROWS, m), np.nan)
    SPA[6] = [1, 0, 0, 2, 0]
    SPA[0, 0], SPA[1, 0], SPA[1, 3], SPA[0, 3] = np.log(1e-3), 20.0, 25.0, -1.0
    out = glmm.binary_stats(S, SPA, R, u)
    assert out["spa_flag"].tolist() == [1, 0, 0, 2, 0] and out["spa_flag"].dtype.kind == "i"
    assert np.isnan(out["beta"][[1, 2]]).all() and np.isnan(out["mean"][1]) and not np.isnan(out["beta"][[0, 3, 4]]).any()
    assert out["p"][0] == pytest.approx(1e-3) and out["log_p"][0] == SPA[0, 0]
    assert np.array_equal(out["p"][[3, 4]], out["p_norm"][[3, 4]])                       # a failed attempt keeps the normal value
    assert np.allclose(out["chi2"][[0, 3, 4]], (out["beta"] / out["se"])[[0, 3, 4]] ** 2)
    assert np.isnan(out["variance_ratio"][[1, 2, 4]]).all() and out["variance_ratio"][0] > 0


def test_argument_checks_raise_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(glmm._lib, "lib", no_device)
    n = 12
    A = sp.identity(n, format="csr")
    C = np.ones((n, 1))
    y = np.r_[np.ones(4), np.zeros(n - 4)]
    LMM = glmm.LogisticMixedModel
    LMM(None, [A], C, y)                                                   # (fine: nothing of a device is needed to build it)
    for bad_y in (np.r_[2.0, y[1:]], np.r_[np.nan, y[1:]], np.zeros(n), np.ones(n), y[:, None], np.array(["a"] * n)):
        with pytest.raises(ValueError):
            LMM(None, [A], C, bad_y)
    for bad_C in (np.ones((n, 0)), np.ones((n, 32)), np.ones((n - 1, 1)), np.ones(n), np.full((n, 1), np.inf)):
        with pytest.raises(ValueError):
            LMM(None, [A], bad_C, y)
    with pytest.raises(ValueError):
        LMM(None, [], C, y)
    with pytest.raises(ValueError):
        LMM(None, [sp.identity(n + 1, format="csr")], C, y)
    model = LMM(None, [A], np.ones((n, 31)), y)                            # c = 31 is the most
    for kw in (dict(tau0=[0.5, 0.5]), dict(tau0=[-1.0]), dict(tau0=[np.nan]), dict(tol=0.0), dict(max_iter=0)):
        with pytest.raises(ValueError):
            model.fit(**kw)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            glmm.check_cutoff(bad)
    assert glmm.check_cutoff(0) == 0.0
    null = LMM(None, [A], C, y).null_at([0.3], [-0.7], np.zeros(n))
    assert null.sigma2_full.tolist() == [0.3, 1.0] and len(null.mats_full) == 2 and not null.boundary
    assert np.allclose(null.mats_full[1].diagonal(), 1 / null.weights) and np.allclose(null.mu, 1 / (1 + np.exp(0.7)))
    with pytest.raises(ValueError):
        null.scan(cutoff=-2.0)
    with pytest.raises(ValueError):
        LMM(None, [A], C, y).null_at([0.3, 0.1], [-0.7], np.zeros(n))


def test_exports_and_entry_points_reject_bad_arguments_before_any_device_state():
    """The three saddlepoint entry points with a null or out-of-range argument, on a null handle, on a factor whose symbolic handle
    is null and on a dummy that a correct check order never reads: the code comes from the argument checks alone (this one test
    needs the built library, not a device)."""
    import ctypes as C
    import scilmm_amd
    from scilmm_amd import _lib
    from scilmm_amd.factor import Factor, Symbolic
    from scilmm_amd.markers import BedRows, DosageRows, Int8Rows
    assert hasattr(scilmm_amd, "LogisticMixedModel") and hasattr(scilmm_amd, "BinaryScan") and hasattr(Symbolic, "spa_timing")
    for name in ("scan_spa_dev", "scan_spa_bed_dev", "scan_spa_dosage_dev"):
        assert hasattr(Factor, name) and "scilmm_" + name in _lib.SYMBOLS
    assert all(hasattr(k, "spa") for k in (Int8Rows, BedRows, DosageRows))
    L = _lib.lib()
    vp = C.c_void_p
    ARG = _lib.ERR_ARG
    one = vp(8)
    hollow = C.create_string_buffer(256)            # a scilmm_factor with sym == NULL
    fac = C.cast(hollow, vp)
    good = [one, one, one, one, one, 1, one, 2.0, one]          # d_stats, d_R, d_u, d_mu, d_C, c, d_Minv, cutoff, d_spa
    forms = [(L.scilmm_scan_spa_dev, [one, 16]), (L.scilmm_scan_spa_bed_dev, [one, 4, 16, None, 0]),
             (L.scilmm_scan_spa_dosage_dev, [one, _lib.DOSAGE_F32, 16, 16, None])]
    for fn, head in forms:
        assert fn(None, *head, 4, *good) == ARG and fn(fac, *head, 4, *good) == ARG               # no handle
        assert fn(one, None, *head[1:], 4, *good) == ARG                                          # no marker rows
        for r in (0, 129, -1):
            assert fn(one, *head, r, *good) == ARG
        for k, bad in [(i, None) for i in (0, 1, 2, 3, 4, 6, 8)] + [(5, 0), (5, 32), (7, -0.5), (7, float("nan"))]:
            args = list(good)
            args[k] = bad
            assert fn(one, *head, 4, *args) == ARG, (fn.__name__, k, bad)
    assert L.scilmm_scan_spa_bed_dev(one, one, 3, 16, None, 0, 4, *good) == ARG                   # pitch shorter than a packed row
    assert L.scilmm_scan_spa_bed_dev(one, one, 4, 16, None, 4, 4, *good) == ARG                   # an unknown flag
    assert L.scilmm_scan_spa_dosage_dev(one, one, 9, 16, 16, None, 4, *good) == ARG               # an unknown element type
    assert L.scilmm_scan_spa_dosage_dev(one, vp(10), _lib.DOSAGE_F32, 16, 16, None, 4, *good) == ARG   # rows not element-aligned
    assert L.scilmm_scan_spa_dosage_dev(one, one, _lib.DOSAGE_U16, 8, 16, None, 4, *good) == ARG  # pitch shorter than a row
    n = 6
    A = (sp.diags([np.full(n - 1, 0.25), np.full(n, 2.0), np.full(n - 1, 0.25)], [-1, 0, 1])).tocsr()
    sym = Symbolic([A, sp.identity(n, format="csr")], upload=False)
    dbl = (C.c_double * 1)()
    assert L.scilmm_spa_timing(None, dbl) == ARG and L.scilmm_spa_timing(sym._h, dbl) == ARG      # no device state
    assert L.scilmm_spa_timing(sym._h, None) == ARG
    assert L.scilmm_get_deterministic(sym._h, C.pointer(C.c_int32())) == _lib.OK                  # the handle is still usable
