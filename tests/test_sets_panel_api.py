"""The set panel's surface without a device (scilmm_amd.set_panel): exports, the argument checks of the C entry point and of the
Python layer, and the pure-NumPy host algebra ``host_set`` on a made-up (S, G, B) block against ``VariantSetTest._one_set`` trait
by trait -- the set's score row replaced by the trait's column of B and u = 0.

TOL 1e-12 relative on every number (NaN and infinities in the same places): at scale 1 ``host_set`` evaluates the expressions of
``_one_set``, and with ``skato_spectra`` handed to ``skato_pvalue`` the same spectra; only the order of LAPACK calls differs.
Under ``scale="profile"`` the reference is ``_one_set`` on the score divided by sqrt(s_t), with ``burden_beta`` and ``burden_se``
brought back to the trait's own units."""
import ctypes as C

import numpy as np
import pytest
import scipy.stats as stats

from scilmm_amd import _lib

TOL = 1e-12
RHO = np.array([0.0, 0.01, 0.04, 0.09, 0.16, 0.25, 0.5, 1.0])


def test_exports():
    import scilmm_amd
    from scilmm_amd import set_panel, sets
    from scilmm_amd.factor import Factor, Symbolic
    assert scilmm_amd.SetTraitPanel is set_panel.SetTraitPanel
    assert callable(sets.VariantSetTest.set_traits) and callable(sets.skato_spectra)
    assert callable(Factor.sets_finish_panel_dev) and callable(Symbolic.sets_finish_panel_timing)
    L = _lib.lib()
    for name in ("scilmm_sets_finish_panel_dev", "scilmm_sets_finish_panel_timing"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert set_panel.KEYS == sets.KEYS and set_panel.SKATO_KEYS == ("skato_p", "skato_pmin", "skato_rho")


def test_entry_point_checks_its_arguments_first():
    """Dummy non-null pointers: every argument error comes before any dereference of the handle or of device memory."""
    L, one = _lib.lib(), C.c_void_p(8)
    start, rho = np.array([0, 2, 5], dtype=np.int32), np.array([0.0, 0.5, 1.0])
    good = dict(fac=one, r=5, q=3, stats=one, gram=one, R=one, c=2, n_sets=2, start=_lib.ptr(start), mode=0, w=None, method=0,
                rho=_lib.ptr(rho), n_rho=3, xty=one, ld=7, t=7, tscale=None, head=one, out=one)
    bad_start = [np.array(v, dtype=np.int32) for v in ([1, 2, 5], [0, 2, 6], [0, 2, 2], [0, 3, 2])]
    bad_rho = [np.array(v) for v in ([0.0, 1.5, 1.0], [0.0, -0.1, 1.0], [0.0, np.nan, 1.0])]
    cases = [dict(fac=None), dict(stats=None), dict(gram=None), dict(R=None), dict(start=None), dict(xty=None), dict(head=None),
             dict(out=None), dict(rho=None), dict(r=0), dict(r=129), dict(c=0, q=1), dict(c=32, q=33), dict(q=4), dict(n_sets=0),
             dict(n_sets=6), dict(n_rho=-1), dict(n_rho=17), dict(mode=3), dict(mode=2, w=None), dict(method=2), dict(t=0),
             dict(t=4097, ld=4097), dict(t=-1), dict(ld=6)]
    cases += [dict(start=_lib.ptr(v)) for v in bad_start] + [dict(rho=_lib.ptr(v)) for v in bad_rho]
    # (with everything else in range the handle would be read next: `one` is no handle, so the good call itself is not made)
    for kw in cases:
        a = dict(good, **kw)
        assert L.scilmm_sets_finish_panel_dev(*[a[k] for k in good]) == _lib.ERR_ARG, kw
    assert L.scilmm_sets_finish_panel_timing(None, (C.c_double * 2)()) == _lib.ERR_ARG


def test_python_checks_raise_without_a_device():
    from scilmm_amd import ScilmmError, set_panel
    from scilmm_amd.panel import check_scale, check_traits
    from scilmm_amd.sets import check_sets
    for bad in ("device ", "wide", None, 1):
        with pytest.raises(ValueError, match="finish"):
            set_panel.check_finish(bad)
    assert set_panel.check_finish("host") == "host" and set_panel.check_finish("device") == "device"
    set_panel.check_keywords({})
    for k in ("return_kernel", "max_markers"):
        with pytest.raises(ValueError, match=k):
            set_panel.check_keywords({k: None})
    with pytest.raises(TypeError, match="reduce"):
        set_panel.check_keywords({"reduce": "max"})
    with pytest.raises(ValueError, match="more than one device block"):       # a wide set: what _run checks first
        check_sets([np.arange(9)], 20, 8)
    for bad in ([1.0, 0.0], [1.0, -2.0], [np.nan], [np.inf], [[1.0]]):
        with pytest.raises(ValueError, match="scale"):
            set_panel.check_scales(bad)
    assert set_panel.check_scales([0.5, 2.0]).tolist() == [0.5, 2.0]
    # the constructor: the tester's type and the scale before anything else; T = 0, T = 4097 and a NaN are check_traits'
    with pytest.raises(ScilmmError, match="VariantSetTest"):
        set_panel.SetTraitPanel(object(), np.zeros((3, 1)))
    with pytest.raises(ValueError, match="scale"):
        check_scale("profiled")
    for Y in (np.zeros((5, 0)), np.zeros((5, 4097)), np.array([[0.0], [np.nan], [1.0], [2.0], [3.0]])):
        with pytest.raises(ValueError):
            check_traits(Y, 5)
    out = set_panel.new_out(3, 4, True, np.array([1.0, 2.0, 3.0, 4.0]))
    assert sorted(out) == sorted(set_panel.KEYS + set_panel.SKATO_KEYS + ("scale",))
    assert out["n_used"].shape == (3,) and out["n_used"].dtype == np.int64 and out["skato_rho"].shape == (3, 4)
    assert sorted(set_panel.new_out(3, 4, False)) == sorted(set_panel.KEYS)


def _block(rng, sizes, c, T):
    """A made-up block: the (c + 5) x r statistics, a positive definite X'X that dominates z'z, R, and B = X'Y~ (r x T); one
    marker without variation and one without an observed value."""
    r = sum(sizes)
    R = np.triu(0.2 * rng.standard_normal((c, c))) + np.diag(rng.uniform(1.0, 2.0, c))
    X = rng.standard_normal((r + 40, r)) * rng.uniform(0.3, 1.7, r)
    W = 0.3 * rng.standard_normal((c, r))
    z = np.linalg.solve(R.T, W)
    G = X.T @ X + z.T @ z
    St = np.zeros((c + 5, r))
    St[0], St[1], St[2], St[3] = 203.0, rng.uniform(0.01, 0.4, r), 1.0, np.diag(G)
    St[4:4 + c] = W
    St[4 + c] = rng.standard_normal(r)                        # the tester's own score row: not a trait of the panel
    St[2, 1], St[0, sizes[0] + 2] = 0.0, 0.0
    B = X.T @ rng.standard_normal((r + 40, T))
    B[:, 1] = 0.0                                             # a trait with no score at all
    B[:, 2] += 6.0 * np.sqrt(np.diag(G))                      # a signal
    return St, 0.5 * (G + G.T), R, B


def _one_set_reference(St, G, R, B, t, weights, method, rho, scale):
    """VariantSetTest._one_set on the set with B[:, t] / sqrt(scale) for its score row and u = 0, without a device: the method
    needs R, u and the burden's null law of its object, nothing else."""
    from scilmm_amd import sets
    obj = object.__new__(sets.VariantSetTest)
    obj.R, obj.u, obj._f = R, np.zeros(R.shape[0]), stats.f(1, 202)
    S2 = St.copy()
    S2[4 + R.shape[0]] = B[:, t] / np.sqrt(scale)
    out = {k: np.full(1, np.nan) for k in sets.KEYS + sets.SKATO_KEYS[:3]}
    out["n_used"] = np.zeros(1, dtype=np.int64)
    out["skato_p_rho"] = np.full((1, len(rho)), np.nan)
    obj._one_set(out, 0, S2, G, weights, sets.check_method(method), rho, method)
    out["burden_beta"] *= np.sqrt(scale)                      # beta and se in the trait's own units
    out["burden_se"] *= np.sqrt(scale)
    return out


@pytest.mark.parametrize("method", ["saddlepoint", "liu"])
@pytest.mark.parametrize("profile", [False, True])
def test_host_algebra_matches_one_set_trait_by_trait(method, profile):
    from scilmm_amd import set_panel, sets
    rng = np.random.default_rng(24)
    sizes, c, T = [5, 1, 9, 2], 3, 4
    St, G, R, B = _block(rng, sizes, c, T)
    s_t = np.array([0.7, 1.0, 2.3, 1.9]) if profile else None
    out = set_panel.new_out(len(sizes), T, True, s_t)
    f = stats.f(1, 202)
    a, worst = 0, 0.0
    for i, m in enumerate(sizes):
        b = a + m
        w = None if i == 2 else "beta" if i < 2 else rng.uniform(0.5, 2.0, m)
        set_panel.host_set(out, i, St[:, a:b], G[a:b, a:b], B[a:b], R, w, sets.check_method(method), f, RHO, method, s_t)
        for t in range(T):
            ref = _one_set_reference(St[:, a:b], G[a:b, a:b], R, B[a:b], t, w, method, RHO, 1.0 if s_t is None else s_t[t])
            assert out["n_used"][i] == ref["n_used"][0] > 0
            for k in set_panel.KEYS[1:] + set_panel.SKATO_KEYS:
                got, want = out[k][i, t], ref[k][0]
                if not np.isfinite(want):
                    assert np.array_equal(got, want, equal_nan=True), (i, t, k)
                    continue
                e = abs(got - want) / abs(want) if want != 0 else abs(got)
                worst = max(worst, e)
                assert e < TOL, (i, t, k, got, want)
        a = b
    assert out["n_used"].tolist() == [4, 1, 8, 2]
    assert np.all(out["skat_q"][:, 1] == 0.0) and np.all(out["skat_p"][:, 1] == 1.0)       # the trait without a score
    print("host_set against _one_set, worst rel. deviation", worst)
    if profile:
        assert np.array_equal(out["scale"], s_t)


def test_precomputed_spectra_leave_skato_pvalue_alone():
    from scilmm_amd import sets
    rng = np.random.default_rng(5)
    for k in (1, 2, 7):
        Z = rng.standard_normal((k + 4, k))
        A = Z.T @ Z
        t = 1.5 * rng.standard_normal(k)
        plain = sets.skato_pvalue(t, A, RHO, "saddlepoint")
        again = sets.skato_pvalue(t, A, RHO, "saddlepoint", sets.skato_spectra(A, RHO))
        assert plain[:3] == again[:3] and np.array_equal(plain[3], again[3])


def test_an_empty_set_stays_nan():
    from scilmm_amd import set_panel, sets
    rng = np.random.default_rng(1)
    St, G, R, B = _block(rng, [3, 3], 2, 3)
    St[2, :3] = 0.0
    out = set_panel.new_out(2, 3, True)
    set_panel.host_set(out, 0, St[:, :3], G[:3, :3], B[:3], R, "beta", sets.mixture_sf_saddlepoint, stats.f(1, 202), RHO)
    assert out["n_used"][0] == 0 and all(np.all(np.isnan(out[k][0])) for k in set_panel.KEYS[1:] + set_panel.SKATO_KEYS)
