"""The finish of a wide variant set by one tridiagonal reduction, without a device: a NumPy model of
the route -- the Householder pre-step that maps 1 to -sqrt(m) e_1, ``sytd2``, the scalings of T per grid value, the Schur
complement for the remainder B, the scalars -- against ``sets.skato_pvalue`` and ``VariantSetTest._one_set``; the argument table
of ``scilmm_sets_finish_wide_dev`` on dummy pointers; the Python refusals on an object that was never constructed.

Tolerances (NumPy model against the host path, both on the CPU): every spectrum within 1e-12 of its largest eigenvalue,
``skat_q`` and the burden numbers 1e-12 relative, every p-value 1e-9 relative; ``skato_rho`` and ``n_used`` exact.  Measured when
this was written: spectra 3.7e-15, skat_q and the burden numbers 4.4e-15, p-values 2.8e-12 (printed with -s).  The model's eigenvalues come from
``scipy.linalg.eigvalsh_tridiagonal``, the host path's from nine dense ``eigvalsh``."""
import ctypes as C

import numpy as np
import pytest
import scipy.integrate as integ
import scipy.linalg as la
import scipy.special as special
import scipy.stats as stats

from scilmm_amd import _lib
from tests import test_gpu_skato as GK

RHO = GK.RHO
LTOL, QTOL, PTOL = 1e-12, 1e-12, 1e-9


def _apply(A, v, tau):
    """A <- H A H in place for H = I - tau v v', as the device does it: p = tau A v, w = p - tau/2 (p'v) v, A -= v w' + w v'."""
    p = tau * (A @ v)
    w = p - 0.5 * tau * (p @ v) * v
    A -= np.outer(v, w) + np.outer(w, v)


def tridiagonal_route(A):
    """(d, e) of T = Q'AQ with Q e_1 = -1 / sqrt(m): the pre-step, then Householder steps without dlarfg's rescaling loop; a
    tail whose sum of squares is 0 gives tau = 0 and e_j = the leading entry."""
    A = np.array(A, dtype=np.float64)
    m = A.shape[0]
    sq = np.sqrt(float(m))
    v = np.full(m, 1.0 / (1.0 + sq))
    v[0] = 1.0
    _apply(A, v, 1.0 + 1.0 / sq)
    d, e = np.empty(m), np.empty(m - 1)
    for j in range(m - 1):
        d[j] = A[j, j]
        x = A[j + 1:, j].copy()
        alpha, ss = x[0], float(x[1:] @ x[1:])
        e[j] = alpha
        if ss == 0.0:
            continue
        beta = -np.copysign(np.sqrt(alpha * alpha + ss), alpha)
        v = x / (alpha - beta)
        v[0] = 1.0
        _apply(A[j + 1:, j + 1:], v, (beta - alpha) / beta)
        e[j] = beta
    d[m - 1] = A[m - 1, m - 1]
    return d, e


def _eig(d, e):
    return la.eigvalsh_tridiagonal(d, e)[::-1] if d.size > 1 else d.copy()


def route_spectra(d, e, rho):
    """The spectra of A, of every A R_rho and of B = A - a a' / s11 (None where the host path has none), in descending order."""
    from scilmm_amd.sets import LAMBDA_FLOOR, RHO_CAP
    m = d.size
    lam_a, lam_rho, lam_b = _eig(d, e), [], None
    for x in np.minimum(rho, RHO_CAP):
        if m == 1:
            lam_rho.append(d.copy())
            continue
        c0, c1 = 1.0 - x, 1.0 - x + x * m
        dd, ee = d * c0, e * c0
        dd[0], ee[0] = d[0] * c1, e[0] * np.sqrt(c1 * c0)
        lam_rho.append(_eig(dd, ee))
    if m > 1 and m * d[0] > LAMBDA_FLOOR * d.sum():
        db = d[1:].copy()
        db[0] -= e[0] * e[0] / d[0]
        lam_b = _eig(db, e[1:])
    return lam_a, lam_rho, lam_b


def route_row(t, A, rho, method):
    """What the device's row holds, from the route: the numbers of ``skato_pvalue`` and of ``_one_set`` with every spectrum and
    every scalar taken from (d, e); the tails, the lines and the quadrature are the host module's."""
    from scilmm_amd import sets as mod
    sf = mod.check_method(method)
    m = t.size
    d, e = tridiagonal_route(A)
    lam_a, lam_rho, lam_b = route_spectra(d, e, rho)
    s11, tr = m * d[0], float(d.sum())
    ws, tt = float(t.sum()), float(t @ t)
    out = dict(lam=lam_a, burden=(ws / s11, 1.0 / np.sqrt(s11), ws * ws / s11), skat_q=tt, skat_p=sf(tt, mod._floor(lam_a)))
    rc = np.minimum(rho, mod.RHO_CAP)
    lams = [mod._floor(l) for l in lam_rho]
    p_rho = np.array([sf(tt if m == 1 else (1.0 - x) * tt + x * ws * ws, l) for x, l in zip(rc, lams)])
    j0 = int(np.argmin(p_rho))
    T = float(p_rho[j0])
    lamB = mod._floor(lam_b, mod.LAMBDA_FLOOR * tr) if lam_b is not None else np.empty(0)
    out.update(p_rho=p_rho, pmin=T, spectra=(lam_rho, lam_b))
    if not lamB.size:
        out.update(p=T, rho=float(rho[0]))
        return out
    aa = m * (d[0] ** 2 + e[0] ** 2)
    aba = max(m * e[0] ** 2 * (d[1] - e[0] ** 2 / d[0]), 0.0)
    l2 = float(np.sum(lamB ** 2))
    mu, sd, df = float(lamB.sum()), np.sqrt(2.0 * l2 + 4.0 * aba / s11), l2 * l2 / float(np.sum(lamB ** 4))
    al, be = mod.skato_lines(T, lams, rc, rc * s11 + (1.0 - rc) * aa / s11)
    z0, pts = mod.skato_breaks(al, be, mu - sd * np.sqrt(0.5 * df))
    p = 2.0 * float(stats.norm.sf(z0))
    k1, k2 = np.sqrt(2.0 * df) / sd, np.sqrt(2.0 / np.pi)
    for lo, hi in zip(pts[:-1], pts[1:]):
        mid = 0.5 * (lo + hi)
        j = int(np.argmin(al - be * (mid * mid)))
        a_j, b_j, h = float(al[j]), float(be[j]), hi - lo
        f = lambda v: special.chdtrc(df, (a_j - b_j * (hi - h * v * v) ** 2 - mu) * k1 + df) * k2 * np.exp(-0.5 * (hi - h * v * v) ** 2) * 2.0 * h * v
        p += integ.quad(f, 0.0, 1.0, epsabs=0.0, epsrel=1e-12, limit=200)[0]
    out.update(p=min(p, rho.size * T), rho=float(rho[j0]))
    return out


def route_cases():
    """(name, K, s): random PSD matrices at m = 2, 3, 17, 129, 257, rank-deficient ones at 33 (rank 12) and 300 (rank 120), the
    identity at 17, 1 an exact eigenvector, rank one; every second one with a signal added to the score."""
    rng = np.random.default_rng(22)
    out = []

    def score(K, signal):
        ev, U = np.linalg.eigh(K)
        t = (U * np.sqrt(np.maximum(ev, 0.0))) @ rng.standard_normal(K.shape[0])
        return t + (2.0 * np.sqrt(np.diag(K)) * rng.choice([-1.0, 1.0], K.shape[0]) if signal else 0.0)

    for i, k in enumerate((2, 3, 17, 129, 257)):
        K = GK._psd(rng, k)
        out.append(("psd%d" % k, K, score(K, i % 2 == 1)))
    for k, rank in ((33, 12), (300, 120)):
        K = GK._psd(rng, k, rank=rank)
        out.append(("rank%dof%d" % (rank, k), K, score(K, k == 33)))
    out.append(("identity17", np.eye(17), 1.4 * rng.standard_normal(17)))
    K = GK._ones_eigvec(rng, 17)
    out.append(("ones_eigvec17", K, score(K, True)))
    b = rng.standard_normal(9)
    out.append(("rank_one9", np.outer(b, b), 2.1 * b))
    return out


def compare_row(got, host_row, host_lam, what, worst):
    """A route's row against the host's (layout of the device's rows) within the tolerances of this file."""
    lam_h = np.sort(host_lam[~np.isnan(host_lam)])[::-1]
    e = float(np.max(np.abs(got["lam"] - lam_h)) / lam_h[0])
    worst["lam"] = max(worst.get("lam", 0.0), e)
    assert e < LTOL, (what, "lam", e)
    for a, b, name in zip(got["burden"] + (got["skat_q"],), host_row[1:5], ("burden_beta", "burden_se", "burden_chi2", "skat_q")):
        e = abs(a - b) / abs(b)
        worst["q"] = max(worst.get("q", 0.0), e)
        assert e < QTOL, (what, name, e)
    a = np.r_[got["skat_p"], got["p"], got["pmin"], got["p_rho"]]
    b = np.r_[host_row[5], host_row[6], host_row[7], host_row[GK.HEAD:]]
    e = float(np.max(np.abs(a - b) / np.abs(b)))
    worst["p"] = max(worst.get("p", 0.0), e)
    assert e < PTOL, (what, "p-values", e, a, b)
    assert got["rho"] == host_row[8], (what, got["rho"], host_row[8])


@pytest.mark.parametrize("method", ["saddlepoint", "liu"])
def test_the_tridiagonal_route_matches_the_host_finish(method):
    from scilmm_amd import sets as mod
    rng = np.random.default_rng(7)
    R = np.triu(0.2 * rng.standard_normal((GK.CC, GK.CC))) + np.diag(rng.uniform(1.0, 2.0, GK.CC))
    u = 0.5 * rng.standard_normal(GK.CC)
    tester = object.__new__(mod.VariantSetTest)       # the host algebra alone: R, u and the F distribution are all it reads
    tester.R, tester.u, tester._f = R, u, stats.f(1, 202)
    worst = {}
    for name, K, s in route_cases():
        S, G, start = GK._made_up_block([(name, K, s, True, ())], rng, R, u)
        out = {k: np.full(1, np.nan) for k in mod.KEYS + mod.SKATO_KEYS[:3]}
        out["n_used"], out["skato_p_rho"] = np.zeros(1, dtype=np.int64), np.full((1, RHO.size), np.nan)
        s_, K_, w = tester._one_set(out, 0, S, G, None, mod.check_method(method), RHO, method)
        assert out["n_used"][0] == K.shape[0]
        A, t = w[:, None] * K_ * w[None, :], w * s_
        host = np.r_[out["n_used"][0], out["burden_beta"][0], out["burden_se"][0], out["burden_chi2"][0], out["skat_q"][0], out["skat_p"][0],
                     out["skato_p"][0], out["skato_pmin"][0], out["skato_rho"][0], 0.0, out["skato_p_rho"][0]]
        direct = mod.skato_pvalue(t, A, RHO, method)
        assert host[6] == direct[0] and host[7] == direct[1] and np.array_equal(host[GK.HEAD:], direct[3])
        got = route_row(t, A, RHO, method)
        compare_row(got, host, la.eigvalsh(A), name, worst)
        # every spectrum of the route against the dense eigvalsh of its matrix
        m = t.size
        lam_rho, lam_b = got["spectra"]
        if m > 1:
            for x, lr in zip(np.minimum(RHO, 0.999), lam_rho):
                L = la.cholesky((1.0 - x) * np.eye(m) + x * np.ones((m, m)), lower=True)
                ref = la.eigvalsh(L.T @ A @ L)[::-1]
                assert np.max(np.abs(lr - ref)) < LTOL * ref[0], (name, x)
            a = A.sum(axis=1)
            if lam_b is not None:
                ref = la.eigvalsh(A - np.outer(a, a) / a.sum())[::-1]
                assert np.max(np.abs(lam_b - ref[:m - 1])) < LTOL * np.trace(A), name
        if name == "rank_one9":                               # nothing is left of B: the degenerate rule on both sides
            assert got["p"] == got["pmin"] and got["rho"] == RHO[0] and host[6] == host[7]
    print("route against the host finish (%s): worst deviations" % method, worst)


def test_the_degenerate_rules_give_the_hosts_answers():
    """One marker, 1'A1 <= 1e-10 trace and no eigenvalue of B above 1e-10 trace: p = T and the first grid value, as the host says."""
    from scilmm_amd import sets as mod
    rng = np.random.default_rng(5)
    K = GK._no_ones(rng, 8)
    b = rng.standard_normal(9)
    for name, A, t in (("one marker", np.array([[2.5]]), np.array([1.7])), ("s11_zero8", K, K @ rng.integers(-3, 4, 8).astype(np.float64)),
                       ("rank_one9", np.outer(b, b), 2.1 * b)):
        p, pmin, rho, p_rho = mod.skato_pvalue(t, A, RHO, "saddlepoint")
        got = route_row(t, A, RHO, "saddlepoint")
        assert p == pmin and rho == RHO[0] and got["p"] == got["pmin"] and got["rho"] == RHO[0], name
        assert abs(got["pmin"] - pmin) < PTOL * pmin and np.max(np.abs(got["p_rho"] - p_rho) / p_rho) < PTOL, name


def test_exports():
    from scilmm_amd import sets
    from scilmm_amd.factor import Factor, Symbolic
    assert callable(Factor.sets_finish_wide_dev) and callable(Symbolic.sets_finish_wide_timing)
    for name in ("scilmm_sets_finish_wide_dev", "scilmm_sets_finish_wide_timing"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    assert sets.FINISHES == ("host", "device") and sets.FINISH_VALUES == ("host", "device", "wide")


def test_wide_entry_point_rejects_bad_arguments_before_any_device_state():
    """Dummy non-null pointers, a null handle and a factor whose symbolic handle is null: the code comes from the argument
    checks alone."""
    f = _lib.lib().scilmm_sets_finish_wide_dev
    vp = C.c_void_p
    one = vp(8)
    hollow = C.create_string_buffer(256)            # a scilmm_factor with sym == NULL: what is right in every other way ends here
    rho = np.array([0.0, 0.5, 1.0])
    good = dict(fac=C.cast(hollow, vp), k=300, block=128, q=5, stats=one, gram=one, cross=one, ld=256, R=one, u=one, c=4, mode=1, w=None,
                method=0, rho=_lib.ptr(rho), n_rho=3, out=one, lam=None)
    bad_rho = [np.array(v) for v in ([0.0, 1.5, 1.0], [0.0, -0.1, 1.0], [0.0, np.nan, 1.0])]
    cases = [dict(), dict(fac=None), dict(stats=None), dict(gram=None), dict(R=None), dict(u=None), dict(out=None), dict(rho=None),
             dict(k=0), dict(k=-1), dict(k=4097), dict(block=0), dict(block=129),
             dict(k=4096, block=100, ld=4096),                # 40 kept sub-blocks of 112 columns: 4480 > 4096
             dict(k=3701, block=100, ld=8192),                # 38 sub-blocks: the 37 kept ones are 4144 columns
             dict(ld=255), dict(ld=0), dict(cross=None),      # ld_cross < (B - 1) bp = 256; B = 3 without a cross store
             dict(k=128, cross=one), dict(k=5, block=16),     # B = 1 with a cross store
             dict(q=4), dict(q=6), dict(c=0, q=1), dict(c=32, q=33), dict(n_rho=-1), dict(n_rho=17), dict(mode=3), dict(mode=-1),
             dict(mode=2, w=None), dict(method=2), dict(method=-1)]
    cases += [dict(rho=_lib.ptr(v)) for v in bad_rho]
    for kw in cases:
        a = dict(good, **kw)
        assert f(*[a[k] for k in good]) == _lib.ERR_ARG, kw
    # what is legal reaches the handle (null here): B = 1 without a cross store, the widest set, a ragged last sub-block of one
    for kw in (dict(k=128, cross=None, ld=0), dict(k=1, block=1, cross=None, ld=0), dict(k=4096, ld=3968), dict(k=225, block=112, ld=224),
               dict(k=3700, block=100, ld=4032), dict(n_rho=0, rho=None), dict(mode=2, w=one), dict(lam=one)):
        a = dict(good, **kw)
        assert f(*[a[k] for k in good]) == _lib.ERR_ARG, kw
    t = _lib.lib().scilmm_sets_finish_wide_timing
    ms = (C.c_double * 4)()
    assert t(None, ms) == _lib.ERR_ARG and t(C.cast(hollow, vp), None) == _lib.ERR_ARG


def test_python_refusals_run_on_an_object_that_was_never_constructed():
    from scilmm_amd.glmm import BinarySetTest
    from scilmm_amd.sets import VariantSetTest
    n, m = 21, 40
    G = np.random.default_rng(0).integers(0, 3, (m, n)).astype(np.int8)
    t = object.__new__(VariantSetTest)
    t.n, t.block = n, 4
    wide = [[0, 1], list(range(9))]
    with pytest.raises(ValueError, match="finish must be one of host, device, wide, got 'lds'"):
        t(G, wide, max_markers=16, finish="lds")
    for call in (lambda **kw: t(G, wide, **kw), lambda **kw: t.test_dosages(np.zeros((m, n), dtype=np.float32), wide, **kw)):
        with pytest.raises(ValueError, match="return_kernel=True needs finish=\"host\""):
            call(max_markers=16, finish="wide", return_kernel=True)
        with pytest.raises(ValueError, match="more than one device block of 4"):
            call(finish="wide")                               # the new value does not lift the bound: max_markers does
        with pytest.raises(ValueError, match="set 1 has 9 markers, more than max_markers = 8"):
            call(max_markers=8, finish="wide")
    with pytest.raises(ValueError, match="rho"):
        t(G, wide, max_markers=16, finish="wide", skato=True, rho=[0.0, 1.5])
    # finish="device" still refuses a wide set, and names both ways out
    with pytest.raises(ValueError, match='a set of 9 markers needs finish="host" or finish="wide": the device finish holds one block'):
        t(G, wide, max_markers=16, finish="device")
    b = object.__new__(BinarySetTest)
    b.n, b.block = n, 4
    with pytest.raises(ValueError, match="finish must be one of host, device, got 'wide'"):
        b(G, [[0, 1]], finish="wide")
    with pytest.raises(ValueError, match="max_markers is not supported for binary traits"):
        b(G, wide, max_markers=16, finish="wide")
