"""The phenotype panels' surface without a device: the host algebra (``panel.panel_stats``) fed with a dense CPU whitening in
place of the device block against the un-whitened GLS oracle (tests/panel_oracle.py), the pure argument checks,
``panel_thresholds`` on a hand-made vector, the exports and the argument checks of ``scilmm_scan_panel_dev``.

Tolerance 1e-9 relative (tests.helpers.rel_err: max-norm), what the suite holds for the scan's derived statistics; the measured
error is printed (3e-14 at most on these inputs: random_spd(300, 0.05, 3), 130 markers, 2 % missing, T = 5)."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as la
import scipy.sparse as sp
import scipy.stats as stats

from scilmm_amd import _lib
from tests import panel_oracle as O
from tests.helpers import random_spd, rel_err

S2 = [0.4, 0.6]
M, T = 130, 5
TOL = 1e-9


@pytest.fixture(scope="module")
def problem():
    A = random_spd(300, 0.05, 3)
    n = A.shape[0]
    V = (S2[0] * A + S2[1] * sp.identity(n)).toarray()
    rng = np.random.default_rng(11)
    Cv = np.hstack([np.ones((n, 1)), rng.standard_normal((n, 3))])
    return dict(n=n, L=np.linalg.cholesky(V), Vi=np.linalg.inv(V), C=Cv, Y=O.traits(n, Cv, T, 5), G=O.markers(n, M, 7))


def _whitened(p, c):
    """(S, B, R, s_t) as the device path hands them to ``panel_stats``, from a dense whitening w(b) = L^-1 b (identity
    permutation): the (q + 4) x M statistics of the plain block, B = X'Y~, the scan's R, the per-trait scales."""
    w = lambda b: la.solve_triangular(p["L"], b, lower=True)
    n, Cv = p["n"], p["C"][:, :c]
    wC, wY = w(Cv), w(p["Y"])
    R = la.cholesky(wC.T @ wC, lower=False)
    Qc = la.solve_triangular(R, wC.T, trans='T', lower=False).T           # w(C) R^-1
    Yt = wY - Qc @ (Qc.T @ wY)
    n_obs, mean, Gt = O.centred(p["G"])
    X = w(Gt.T)
    S = np.zeros((c + 5, M))
    S[0], S[1], S[2], S[3] = n_obs, np.where(n_obs > 0, mean, 0.0), (Gt * Gt).sum(axis=1), (X * X).sum(axis=0)
    S[4:4 + c] = wC.T @ X
    S[4 + c] = wY[:, 0] @ X                                                # (the scan's own y: not read by the panel)
    return S, X.T @ Yt, R, (Yt * Yt).sum(axis=0) / (n - c)


@pytest.mark.parametrize("scale", ["fixed", "profile"])
@pytest.mark.parametrize("c", [1, 4])
def test_panel_stats_match_unwhitened_gls(problem, c, scale):
    from scilmm_amd.panel import panel_stats
    p = problem
    S, B, R, s_t = _whitened(p, c)
    out = panel_stats(S, B, R, p["n"], scale, s_t)
    ref = O.gls(p["Vi"], p["C"][:, :c], p["Y"], p["G"], scale)
    bad = np.zeros(M, bool)
    bad[[O.MONO, O.ALLMISS]] = True
    for k in ("beta", "se", "chi2"):
        assert out[k].shape == (M, T)
        print(k, "rel.err", rel_err(out[k][~bad], ref[k][~bad]))
        assert rel_err(out[k][~bad], ref[k][~bad]) < TOL, k
        assert np.array_equal(np.isnan(out[k]), np.repeat(bad[:, None], T, axis=1)), k   # NaN exactly on the two degenerate rows
    assert np.array_equal(out["p"], stats.f(1, p["n"] - 1).sf(out["chi2"]), equal_nan=True)
    assert out["n_obs"].dtype.kind == "i" and np.array_equal(out["n_obs"], ref["n_obs"])
    assert np.isnan(out["mean"][O.ALLMISS]) and out["mean"][O.MONO] == 1.0
    if scale == "profile":
        print("scale rel.err", rel_err(out["scale"], ref["scale"]))
        assert rel_err(out["scale"], ref["scale"]) < TOL
    else:
        assert "scale" not in out


def test_one_trait_fixed_scale_is_the_scan(problem):
    """``panel_stats`` for Y = y[:, None] against the scan's own host algebra on the same statistics."""
    from scilmm_amd.assoc import AssociationScan
    from scilmm_amd.panel import panel_stats
    p = problem
    S, B, R, _ = _whitened(p, 4)
    scan = AssociationScan.__new__(AssociationScan)            # (no device: only what _finish reads)
    w = lambda b: la.solve_triangular(p["L"], b, lower=True)
    scan.c, scan.R, scan._f = 4, R, stats.f(1, p["n"] - 1)
    scan.u = la.solve_triangular(R, w(p["C"]).T @ w(p["Y"][:, 0]), trans='T', lower=False)
    ref, out = scan._finish(S), panel_stats(S, B[:, :1], R, p["n"])
    ok = ~np.isnan(ref["beta"])
    for k in ("beta", "se", "chi2"):
        assert rel_err(out[k][ok, 0], ref[k][ok]) < 1e-12, k
        assert np.array_equal(np.isnan(out[k][:, 0]), ~ok)


def test_pure_checks_refuse():
    from scilmm_amd import panel
    n = 12
    Y = np.zeros((n, 3))
    assert panel.check_traits(Y, n).shape == (n, 3)
    assert panel.check_traits(np.arange(n * 2).reshape(n, 2), n).dtype == np.float64
    for bad in (np.zeros(n), np.zeros((n + 1, 3)), np.zeros((n, 0)), np.zeros((n, panel.TMAX + 1)), np.zeros((n, 2, 2))):
        with pytest.raises(ValueError):
            panel.check_traits(bad, n)
    for k, v in ((0, np.nan), (n - 1, np.inf)):
        Z = Y.copy()
        Z[k, 1] = v
        with pytest.raises(ValueError, match="missing"):
            panel.check_traits(Z, n)
    for bad in ("Y", None, np.array([["a"] * 3] * n), np.zeros((n, 3), dtype=complex)):
        with pytest.raises(TypeError):
            panel.check_traits(bad, n)
    assert panel.check_n_rep(1) == 1 and panel.check_n_rep(np.int64(panel.TMAX)) == panel.TMAX
    for bad in (0, -1, panel.TMAX + 1):
        with pytest.raises(ValueError):
            panel.check_n_rep(bad)
    for bad in (10.0, "10", True, None):
        with pytest.raises(TypeError):
            panel.check_n_rep(bad)
    with pytest.raises(TypeError):
        panel.check_seed(0.5)
    assert panel.check_scale("fixed") == "fixed" and panel.check_scale("profile") == "profile"
    assert panel.check_reduce(None) is None and panel.check_reduce("max") == "max"
    for bad in ("Fixed", None, 1):
        with pytest.raises(ValueError):
            panel.check_scale(bad)
    for bad in ("min", "MAX", 0):
        with pytest.raises(ValueError):
            panel.check_reduce(bad)
    with pytest.raises(ValueError):
        panel.panel_stats(np.zeros((6, 4)), np.zeros((4, 2)), np.eye(1), n, "free")
    with pytest.raises(ValueError):
        panel.panel_stats(np.zeros((6, 4)), np.zeros((4, 2)), np.eye(1), n, "profile", np.ones(3))
    with pytest.raises(ValueError):
        panel.panel_stats(np.zeros((6, 4)), np.zeros((5, 2)), np.eye(1), n)
    # a panel stands on an AssociationScan only (no panels on the interaction scan or the set tests)
    with pytest.raises(_lib.ScilmmError, match="AssociationScan"):
        panel.TraitPanel(object(), None, "fixed")


def test_panel_thresholds_on_a_hand_made_vector():
    from scilmm_amd import panel_thresholds
    mx = np.array([7.0, 1.0, 4.0, 10.0, 3.0, 9.0, 2.0, 8.0, 5.0, 6.0])      # 1 .. 10: the 0.75 quantile lies between 7 and 8
    n = 50
    thr = panel_thresholds(mx, n, alpha=0.25)
    assert thr["chi2"] == 8.0                                                # "higher": an order statistic, never interpolated
    assert thr["p"] == stats.f(1, n - 1).sf(8.0) and thr["m_eff"] == 0.25 / thr["p"]
    assert panel_thresholds(mx, n, alpha=0.05)["chi2"] == 10.0
    assert panel_thresholds(mx, n, alpha=0.9)["chi2"] == 2.0                 # position 0.9 between 1 and 2
    assert panel_thresholds(mx[:1], n)["chi2"] == 7.0
    for bad in (dict(max_chi2=[], n=n), dict(max_chi2=[1.0, np.nan], n=n), dict(max_chi2=mx, n=n, alpha=0.0),
                dict(max_chi2=mx, n=n, alpha=1.0)):
        with pytest.raises(ValueError):
            panel_thresholds(**bad)


def test_exports():
    import scilmm_amd
    from scilmm_amd.assoc import AssociationScan
    from scilmm_amd.factor import Factor, Symbolic
    for name in ("TraitPanel", "panel_stats", "panel_thresholds"):
        assert hasattr(scilmm_amd, name)
    assert hasattr(AssociationScan, "traits") and hasattr(AssociationScan, "null_panel")
    assert hasattr(Factor, "scan_panel_dev") and hasattr(Symbolic, "panel_timing")
    assert {"scilmm_scan_panel_dev", "scilmm_panel_timing"} <= set(_lib.SYMBOLS)


def test_entry_point_rejects_bad_arguments_before_any_device_state():
    """``scilmm_scan_panel_dev`` with a null or out-of-range argument, on a null handle, a factor whose symbolic handle is null
    and a dummy that a correct check order never reads: the code comes from the argument checks alone."""
    from scilmm_amd.factor import Symbolic
    L = _lib.lib()
    vp = C.c_void_p
    ARG = _lib.ERR_ARG
    one, a16 = vp(8), vp(32)                        # non-null dummies: any address, and a 16-byte aligned one
    hollow = C.create_string_buffer(256)            # a scilmm_factor with sym == NULL
    fac = C.cast(hollow, vp)
    table = [
        (None, 1, a16, 16, 1, a16, 1), (fac, 1, a16, 16, 1, a16, 1),            # no handle
        (one, 1, None, 16, 1, a16, 1), (one, 1, a16, 16, 1, None, 1),           # null d_Y, d_xty
        (one, 0, a16, 16, 1, a16, 1), (one, 129, a16, 16, 1, a16, 1), (one, -1, a16, 16, 1, a16, 1),   # r outside 1..128
        (one, 1, a16, 16, 0, a16, 1), (one, 1, a16, 4112, 4097, a16, 4097),     # t outside 1..4096
        (one, 1, a16, 16, 17, a16, 17),                                         # ld_y < t
        (one, 1, a16, 24, 1, a16, 1), (one, 1, a16, 1, 1, a16, 1),              # ld_y % 16 != 0
        (one, 1, a16, 16, 5, a16, 4),                                           # ld_out < t
        (one, 1, one, 16, 1, a16, 1),                                           # d_Y not 16-byte aligned
    ]
    got = [L.scilmm_scan_panel_dev(*args) for args in table]
    assert got == [ARG] * len(table)
    n = 6
    A = (sp.diags([np.full(n - 1, 0.25), np.full(n, 2.0), np.full(n - 1, 0.25)], [-1, 0, 1])).tocsr()
    sym = Symbolic([A, sp.identity(n, format="csr")], upload=False)
    dbl = (C.c_double * 2)()
    assert L.scilmm_panel_timing(None, dbl) == ARG and L.scilmm_panel_timing(sym._h, dbl) == ARG      # no device state
    assert L.scilmm_panel_timing(sym._h, None) == ARG
    assert L.scilmm_get_deterministic(sym._h, C.pointer(C.c_int32())) == _lib.OK                      # the handle is still usable
