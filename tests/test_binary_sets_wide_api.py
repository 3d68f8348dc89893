"""Wide variant sets for binary traits, without a device: the argument tables of the five entry points and of
the timing call on dummy pointers; the Python refusals on an object that was never constructed; a NumPy statement of the scaled
tridiagonal route -- the model of tests/test_sets_wide_finish_api.py with ``w o scale`` in A alone -- against
``binary_sets.scaled_tests``.

Tolerances: those of tests/test_sets_wide_finish_api.py (the same model against the same host algebra): skat_q and the burden
numbers 1e-12 relative, every p-value 1e-9 relative, ``skato_rho`` exact."""
import ctypes as C

import numpy as np
import pytest

from scilmm_amd import _lib, binary_sets
from tests import test_gpu_skato as GK
from tests import test_sets_wide_finish_api as WF

vp = C.c_void_p
RHO = GK.RHO


def _hollow():
    """A scilmm_factor with sym == NULL: what is right in every other way ends here."""
    return C.create_string_buffer(256)


def test_exports():
    from scilmm_amd import BinaryWideSetTest, glmm
    from scilmm_amd.factor import Factor, Symbolic
    from scilmm_amd.markers import BedRows, DosageRows, Int8Rows
    assert issubclass(BinaryWideSetTest, glmm.BinarySetTest) and BinaryWideSetTest is glmm.BinaryWideSetTest
    for name in ("scilmm_sets_collapse_dev", "scilmm_sets_collapse_bed_dev", "scilmm_sets_collapse_dosage_dev", "scilmm_sets_spa_wide_dev",
                 "scilmm_sets_finish_wide_scaled_dev", "scilmm_sets_spa_wide_timing"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
        assert callable(getattr(Factor, name[len("scilmm_"):] if name.endswith("_dev") else "sets_spa_wide_timing"))
    assert callable(Symbolic.sets_spa_wide_timing)
    for cls in (Int8Rows, BedRows, DosageRows):
        assert callable(cls.collapse)


def test_collapse_entry_points_reject_bad_arguments_before_any_device_state():
    L, one, n = _lib.lib(), vp(8), 100
    hollow = _hollow()
    good = dict(stats=one, mode=1, w=None, first=1, gB=one)
    cases = [dict(), dict(stats=None), dict(gB=None), dict(first=2), dict(first=-1), dict(mode=3), dict(mode=-1), dict(mode=2, w=None),
             dict(mode=2, w=one), dict(first=0)]
    forms = [(L.scilmm_sets_collapse_dev, [one, n]), (L.scilmm_sets_collapse_bed_dev, [one, (n + 3) // 4, n, None, 0]),
             (L.scilmm_sets_collapse_dosage_dev, [one, _lib.DOSAGE_U16, n, n, None])]
    for fn, head in forms:
        for kw in cases:           # (the legal ones reach the handle, null here)
            a = dict(good, **kw)
            assert fn(C.cast(hollow, vp), *head, 5, *[a[k] for k in good]) == _lib.ERR_ARG, (fn.__name__, kw)
        for r in (0, -1, 129):
            assert fn(C.cast(hollow, vp), *head, r, *good.values()) == _lib.ERR_ARG
        assert fn(None, *head, 5, *good.values()) == _lib.ERR_ARG
        assert fn(C.cast(hollow, vp), None, *head[1:], 5, *good.values()) == _lib.ERR_ARG
    h = C.cast(hollow, vp)
    assert L.scilmm_sets_collapse_bed_dev(h, one, (n + 3) // 4 - 1, n, None, 0, 5, *good.values()) == _lib.ERR_ARG   # pitch shorter than a row
    assert L.scilmm_sets_collapse_bed_dev(h, one, (n + 3) // 4, n, None, 2, 5, *good.values()) == _lib.ERR_ARG      # an unknown flag
    assert L.scilmm_sets_collapse_bed_dev(h, one, (n + 3) // 4, 0, None, 0, 5, *good.values()) == _lib.ERR_ARG
    assert L.scilmm_sets_collapse_dosage_dev(h, one, 7, n, n, None, 5, *good.values()) == _lib.ERR_ARG              # an unknown element type
    assert L.scilmm_sets_collapse_dosage_dev(h, vp(9), _lib.DOSAGE_U16, n, n, None, 5, *good.values()) == _lib.ERR_ARG   # a misaligned pointer
    assert L.scilmm_sets_collapse_dosage_dev(h, one, _lib.DOSAGE_F32, n - 1, n, None, 5, *good.values()) == _lib.ERR_ARG


def test_set_saddlepoint_entry_point_rejects_bad_arguments_before_any_device_state():
    f = _lib.lib().scilmm_sets_spa_wide_dev
    one = vp(8)
    hollow = _hollow()
    good = dict(fac=C.cast(hollow, vp), k=300, block=128, q=5, stats=one, gram=one, cross=one, ld=256, R=one, u=one, mu=one, C=one, c=4,
                Minv=one, cutoff=2.0, spa=one, mode=1, w=None, gB=one, bspa=one, vscale=one)
    cases = [dict()] + [dict([(k, None)]) for k in ("fac", "stats", "gram", "R", "u", "mu", "C", "Minv", "spa", "gB", "bspa", "vscale")]
    cases += [dict(k=0), dict(k=-1), dict(k=4097), dict(block=0), dict(block=129),
              dict(k=4096, block=100, ld=4096), dict(k=3701, block=100, ld=8192),      # more kept columns than a panel call holds
              dict(ld=255), dict(ld=0), dict(cross=None), dict(k=128, cross=one), dict(k=5, block=16),
              dict(q=4), dict(q=6), dict(c=0, q=1), dict(c=32, q=33), dict(cutoff=-1.0), dict(cutoff=float("nan")), dict(mode=3), dict(mode=-1),
              dict(mode=2, w=None)]
    # what is legal reaches the handle (null here)
    cases += [dict(k=128, cross=None, ld=0), dict(k=1, block=1, cross=None, ld=0), dict(k=4096, ld=3968), dict(k=225, block=112, ld=224),
              dict(mode=2, w=one), dict(cutoff=0.0), dict(c=31, q=32)]
    for kw in cases:
        a = dict(good, **kw)
        assert f(*[a[k] for k in good]) == _lib.ERR_ARG, kw


def test_scaled_wide_finish_rejects_bad_arguments_before_any_device_state():
    f = _lib.lib().scilmm_sets_finish_wide_scaled_dev
    one = vp(8)
    hollow = _hollow()
    rho = np.array([0.0, 0.5, 1.0])
    good = dict(fac=C.cast(hollow, vp), k=300, block=128, q=5, stats=one, gram=one, cross=one, ld=256, R=one, u=one, c=4, mode=1, w=None,
                method=0, rho=_lib.ptr(rho), n_rho=3, out=one, lam=None, vscale=one)
    bad_rho = [np.array(v) for v in ([0.0, 1.5, 1.0], [0.0, -0.1, 1.0], [0.0, np.nan, 1.0])]
    cases = [dict(), dict(vscale=None), dict(fac=None), dict(stats=None), dict(gram=None), dict(R=None), dict(u=None), dict(out=None),
             dict(rho=None), dict(k=0), dict(k=4097), dict(block=0), dict(block=129), dict(k=4096, block=100, ld=4096), dict(ld=255),
             dict(cross=None), dict(k=128, cross=one), dict(q=4), dict(c=0, q=1), dict(c=32, q=33), dict(n_rho=-1), dict(n_rho=17),
             dict(mode=3), dict(mode=2, w=None), dict(method=2), dict(method=-1)]
    cases += [dict(rho=_lib.ptr(v)) for v in bad_rho]
    cases += [dict(k=128, cross=None, ld=0), dict(n_rho=0, rho=None), dict(mode=2, w=one), dict(lam=one)]     # legal: the null handle
    for kw in cases:
        a = dict(good, **kw)
        assert f(*[a[k] for k in good]) == _lib.ERR_ARG, kw


def test_timing_call_rejects_null_arguments():
    t = _lib.lib().scilmm_sets_spa_wide_timing
    ms = (C.c_double * 3)()
    hollow = _hollow()                                  # (a symbolic handle without a device)
    assert t(None, ms) == _lib.ERR_ARG and t(C.cast(hollow, vp), None) == _lib.ERR_ARG and t(C.cast(hollow, vp), ms) == _lib.ERR_ARG


def test_sets_without_max_markers_is_exactly_a_binary_set_test(monkeypatch):
    """``NullModel.sets`` picks the class by ``max_markers`` alone; the constructors are not run."""
    from scilmm_amd import glmm
    made = []
    monkeypatch.setattr(glmm.BinarySetTest, "__init__", lambda self, *a, **kw: made.append((type(self), kw)))
    null = object.__new__(glmm.NullModel)
    null._model = type("M", (), dict(cholesky_func=None, covariates=None))()
    t = null.sets(block=16, cutoff=0.5)
    assert type(t) is glmm.BinarySetTest and made[-1] == (glmm.BinarySetTest, dict(block=16, cutoff=0.5))
    monkeypatch.setattr(glmm.BinaryWideSetTest, "__init__", lambda self, *a, **kw: made.append((type(self), kw)))
    t = null.sets(block=16, cutoff=0.5, max_markers=300)
    assert type(t) is glmm.BinaryWideSetTest and made[-1] == (glmm.BinaryWideSetTest, dict(block=16, cutoff=0.5, max_markers=300))


def test_python_refusals_run_on_an_object_that_was_never_constructed():
    from scilmm_amd.glmm import BinaryWideSetTest
    n, m = 21, 40
    G = np.random.default_rng(0).integers(0, 3, (m, n)).astype(np.int8)
    t = object.__new__(BinaryWideSetTest)
    t.n, t.block, t.max_markers = n, 4, 16
    wide = [[0, 1], list(range(9))]
    calls = (lambda **kw: t(G, wide, **kw), lambda **kw: t.test_dosages(np.zeros((m, n), dtype=np.float32), wide, **kw))
    for call in calls:
        with pytest.raises(ValueError, match="finish must be one of host, device, wide, got 'lds'"):
            call(finish="lds")
        with pytest.raises(ValueError, match="return_kernel=True needs finish=\"host\""):
            call(finish="wide", return_kernel=True)
        with pytest.raises(ValueError, match="return_kernel=True needs finish=\"host\""):
            call(finish="device", return_kernel=True)
        with pytest.raises(ValueError, match="set 1 has 9 markers, more than max_markers = 8"):
            call(max_markers=8)                               # the call's value overrides the constructor's
        with pytest.raises(ValueError, match="max_markers must lie in block .. 4096"):
            call(max_markers=3)
        with pytest.raises(ValueError, match="max_markers must lie in block .. 4096"):
            call(max_markers=4097)
        with pytest.raises(ValueError, match="max_markers must be None or an integer"):
            call(max_markers=8.0)
        with pytest.raises(ValueError, match='a set of 9 markers needs finish="host" or finish="wide": the device finish holds one block'):
            call(finish="device")
        with pytest.raises(ValueError, match="method must be one of"):
            call(method="davies")
        with pytest.raises(ValueError, match="rho"):
            call(finish="wide", skato=True, rho=[0.0, 1.5])
        with pytest.raises(ValueError, match="2 weight arrays for|1 weight arrays for 2 sets"):
            call(weights=[np.ones(2)])
        with pytest.raises(ValueError, match="weights must be"):
            call(weights="gamma")
    with pytest.raises(ValueError, match="set 1 holds a marker twice"):
        t(G, [[0, 1], [2, 3, 4, 5, 6, 2]])
    with pytest.raises(ValueError, match="outside 0 .. 39"):
        t(G, [[0, 1], list(range(36, 45))])
    t.max_markers = 8
    with pytest.raises(ValueError, match="set 1 has 9 markers, more than max_markers = 8"):
        t(G, wide)
    # the kept sub-blocks of the widest set must fit a panel call: block 100 -> 112 columns each, 37 of them
    t.block, t.max_markers = 100, 4096
    with pytest.raises(ValueError, match="more than the 4096 columns of a panel call"):
        t(np.zeros((3701, n), dtype=np.int8), [list(range(3701))])
    # the constructor's own check
    for bad in (3, 4097, 2.5, True):
        with pytest.raises(ValueError, match="max_markers"):
            from scilmm_amd.sets import check_max_markers
            check_max_markers(bad, 4)


def scaled_route_row(s, K, w, vscale, rho, method):
    """The row of the scaled wide finish from the tridiagonal route: A = diag(w o scale) K diag(w o scale), t = w o s keeps w."""
    ws = w * vscale
    return WF.route_row(w * s, ws[:, None] * K * ws[None, :], rho, method)


@pytest.mark.parametrize("method", ["saddlepoint", "liu"])
def test_the_scaled_tridiagonal_route_matches_scaled_tests(method):
    rng = np.random.default_rng(23)
    worst = {}
    for m in (2, 17, 129):
        K = GK._psd(rng, m)
        ev, U = np.linalg.eigh(K)
        s = (U * np.sqrt(np.maximum(ev, 0.0))) @ rng.standard_normal(m) + (1.5 * np.sqrt(np.diag(K)) if m == 17 else 0.0)
        w, vscale = rng.uniform(0.5, 2.0, m), rng.uniform(1.0, 1.5, m)
        want = binary_sets.scaled_tests(s, K, w, vscale, method, RHO)
        got = scaled_route_row(s, K, w, vscale, RHO, method)
        for a, b, name in zip(got["burden"] + (got["skat_q"],), [want[k] for k in ("burden_beta", "burden_se", "burden_chi2", "skat_q")],
                              ("burden_beta", "burden_se", "burden_chi2", "skat_q")):
            e = abs(a - b) / abs(b)
            worst["q"] = max(worst.get("q", 0.0), e)
            assert e < WF.QTOL, (m, name, e)
        p, pmin, rho_at, p_rho = want["skato"]
        a = np.r_[got["skat_p"], got["p"], got["pmin"], got["p_rho"]]
        b = np.r_[want["skat_p"], p, pmin, p_rho]
        e = float(np.max(np.abs(a - b) / np.abs(b)))
        worst["p"] = max(worst.get("p", 0.0), e)
        assert e < WF.PTOL, (m, "p-values", e)
        assert got["rho"] == rho_at
        # the scales matter: the unscaled route gives another burden, by far more than the tolerance
        plain = WF.route_row(w * s, w[:, None] * K * w[None, :], RHO, method)
        assert abs(plain["burden"][2] - want["burden_chi2"]) > 1e-3 * want["burden_chi2"]
        # and with every scale 1 the scaled route IS the unscaled one
        ones = scaled_route_row(s, K, w, np.ones(m), RHO, method)
        assert ones["burden"] == plain["burden"] and ones["p"] == plain["p"] and np.array_equal(ones["p_rho"], plain["p_rho"])
    print("scaled route against scaled_tests (%s): worst deviations" % method, worst)
