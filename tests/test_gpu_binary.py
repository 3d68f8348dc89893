"""Binary traits on the device (scilmm_amd.glmm, scilmm_scan_spa*_dev) against the dense oracle (tests/spa_oracle.py).

Tolerances.  log_p: 1e-8 max(1, |log p|) per marker -- at the root s - K'(zeta) = 0, so omega depends on zeta to second order and nu
linearly: a root good to 1e-10 moves log p by less than 1e-9.  a_w and s: 1e-11 relative (max-norm, tests.helpers.rel_err): two
summation orders of n <= 2000 terms differ by at most 4.4e-13 sum|terms|.  beta, se, chi2: the suite's 1e-9.  flag and n_obs: exact.
Bit identity where the issue is the order of a sum.  The null fit: 1e-6 relative between two implementations of the same map, both
iterated to tol = 1e-9.

The scan tests run at a GIVEN null point (tau, alpha, b) -- the identities the scan rests on hold at any point, converged or not --
so that one dense inverse per case is all the oracle costs; the fit is compared on its own."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as la
import scipy.stats as stats

from scilmm_amd import glmm
from tests import spa_oracle as O
from tests.helpers import random_spd, rel_err, small_pedigree

pytestmark = pytest.mark.gpu

TOL = 1e-9
M = 130                      # markers: partial last blocks at block = 16 and 128
TAU = [0.4]
vp = C.c_void_p

_PROBLEMS = {}


def _problem(name):
    """(A, markers, the 31 covariate columns, y) per cohort, the null point and the oracle's scan per c; built once."""
    if name not in _PROBLEMS:
        if name == "pedigree":
            A = small_pedigree(2000, 0.01, 0)[0]              # n = 1502: no multiple of 16 or 256
        elif name == "spd300":
            A = random_spd(300, 0.05, 3)                      # a ragged second stride
        else:
            A = small_pedigree(2000, 0.01, 0)[0][:100][:, :100].tocsr()   # n = 100: threads with no row
            A.sort_indices()
        n = A.shape[0]
        rng = np.random.default_rng(11)
        Cv = np.hstack([np.ones((n, 1)), rng.standard_normal((n, 30))])
        G = O.markers(n, M, 7)
        y = O.phenotype(A, Cv[:, :4], G, 0.05, 0.5, 3)        # prevalence 0.05; the markers O.ASSOC carry an effect
        assert 0 < y.sum() < n
        _PROBLEMS[name] = dict(A=A, n=n, C=Cv, G=G, y=y, b=0.4 * rng.standard_normal(n), ref={})
    return _PROBLEMS[name]


def _alpha(c, mu0=0.05):
    return np.r_[np.log(mu0 / (1 - mu0)), 0.15 * np.random.default_rng(c).standard_normal(c - 1)]


def _oracle(p, c, mu0=0.05, m=M):
    """The oracle's null point (fitted probabilities about mu0) and its scan (cutoff 0) of the problem's first m markers for c
    covariates."""
    if (c, mu0, m) not in p["ref"]:
        Cc = p["C"][:, :c]
        eta = Cc @ _alpha(c, mu0) + p["b"]
        mu = 1 / (1 + np.exp(-eta))
        null = dict(tau=np.array(TAU), mu=mu, working_y=eta + (p["y"] - mu) / (mu * (1 - mu)))
        p["ref"][c, mu0, m] = (null, O.scan([p["A"]], null, Cc, p["G"][:m]))
    return p["ref"][c, mu0, m]


def _scan(p, c, block=None, cutoff=0.0, mu0=0.05, **kw):
    from scilmm_amd import LogisticMixedModel, SparseCholesky
    model = LogisticMixedModel(SparseCholesky(**kw), [p["A"]], p["C"][:, :c], p["y"])
    return model.null_at(TAU, _alpha(c, mu0), p["b"]).scan(block=block, cutoff=cutoff)


def _check_against_oracle(out, spa_rows, ref, tag):
    att = ref["spa_flag"] > 0
    assert np.array_equal(out["spa_flag"], ref["spa_flag"]), tag
    assert out["n_obs"].dtype.kind == "i" and np.array_equal(out["n_obs"], ref["n_obs"]), tag
    assert np.array_equal(np.isnan(out["beta"]), ref["bad"]), tag
    for k in ("beta", "se", "chi2"):
        print(tag, k, "rel.err", rel_err(out[k][~ref["bad"]], ref[k][~ref["bad"]]))
        assert rel_err(out[k][~ref["bad"]], ref[k][~ref["bad"]]) < TOL, (tag, k)
    for k, row in (("a_w", 1), ("s", 2)):
        print(tag, k, "rel.err", rel_err(spa_rows[row][att], ref[k][att]))
        assert rel_err(spa_rows[row][att], ref[k][att]) < 1e-11, (tag, k)
    one = ref["spa_flag"] == 1
    gap = np.abs(out["log_p"][one] - ref["log_p"][one]) / np.maximum(1.0, np.abs(ref["log_p"][one]))
    print(tag, "log_p worst gap / max(1, |log p|)", gap.max(), "flags", np.bincount(ref["spa_flag"], minlength=3),
          "iters max", np.nanmax(spa_rows[5]), "min log_p", ref["log_p"][one].min())
    assert np.all(gap < 1e-8), (tag, gap.max())
    assert np.array_equal(out["p"][one], np.exp(out["log_p"][one]))
    assert np.array_equal(out["p_norm"], stats.chi2.sf(out["chi2"], 1), equal_nan=True)
    with np.errstate(invalid="ignore"):
        assert rel_err(out["variance_ratio"][att], (ref["a"] / ref["a_w"])[att]) < TOL
    assert np.all(np.isnan(out["variance_ratio"][~att]))


@pytest.mark.parametrize("name,c,block", [("pedigree", 1, 128), ("pedigree", 4, 16), ("pedigree", 31, 1),
                                          ("spd300", 1, 1), ("spd300", 4, 128), ("spd300", 31, 16),
                                          ("sub100", 1, 16), ("sub100", 4, 1), ("sub100", 31, 128)])
def test_scan_matches_the_dense_oracle(name, c, block):
    """cutoff = 0: every non-degenerate marker takes both roots.  Every c and every block width on every cohort."""
    p = _problem(name)
    _, ref = _oracle(p, c)
    assert ref["spa_flag"][[O.MONO, O.ALLMISS]].tolist() == [0, 0] and np.all(ref["spa_flag"][list(O.ASSOC)] == 1)
    scan = _scan(p, c, block)
    out = scan(p["G"])
    _check_against_oracle(out, scan.last_spa, ref, (name, c, block))


def test_cutoff_selects_the_markers():
    p = _problem("pedigree")
    _, ref = _oracle(p, 4)
    full = _scan(p, 4, 128, cutoff=0.0, deterministic=True)
    all_rows = full(p["G"])
    scan = _scan(p, 4, 128, cutoff=2.0, deterministic=True)
    out = scan(p["G"])
    with np.errstate(invalid="ignore"):
        near = np.abs(np.abs(ref["zs"]) - 2.0) < 1e-6
        want0 = ref["bad"] | ~(np.abs(ref["zs"]) > 2.0)
    assert near.sum() <= 1
    assert np.array_equal((out["spa_flag"] == 0)[~near], want0[~near])
    assert 0 < (out["spa_flag"] == 1).sum() < M - 2
    # a marker's seven numbers do not depend on the cutoff that let it through, nor on its neighbours
    on = out["spa_flag"] > 0
    assert np.array_equal(scan.last_spa[:, on], full.last_spa[:, on])
    assert np.all(np.isnan(scan.last_spa[:6, ~on])) and np.array_equal(out["p"][~on], out["p_norm"][~on], equal_nan=True)
    assert np.array_equal(out["chi2"], all_rows["chi2"], equal_nan=True)


def _block(scan, G, r, torch):
    n = scan.n
    ld = (n + 15) // 16 * 16
    dG = torch.zeros((r, ld), dtype=torch.int8, device="cuda")
    dG[:, :n] = torch.from_numpy(np.ascontiguousarray(G[:r])).cuda()
    dS = torch.zeros(((scan.q + 4) * r,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    scan.factor.scan_block_dev(vp(dG.data_ptr()), ld, r, vp(scan.dQ.data_ptr()), scan.q, vp(dS.data_ptr()))
    return dG, ld, dS


def _spa_call(scan, dG, ld, r, dS, torch, cutoff=0.0):
    dP = torch.full((glmm.SPA_ROWS * r,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    scan.factor.scan_spa_dev(vp(dG.data_ptr()), ld, r, vp(dS.data_ptr()), vp(scan.dR.data_ptr()), vp(scan.du.data_ptr()),
                             vp(scan.dmu.data_ptr()), vp(scan.dC.data_ptr()), scan.c, vp(scan.dMinv.data_ptr()), cutoff, vp(dP.data_ptr()))
    scan.sym.sync()
    return dP.cpu().numpy().reshape(glmm.SPA_ROWS, r)


def test_entry_point_with_doctored_statistics():
    """The score of two markers replaced in d_stats: zs = 1e6 lies outside the support of T (flag 2, the normal value), zs = 40 inside
    it (flag 1, log_p finite far below where p underflows).  At the prevalence of the other tests the statistic is so skewed that 40
    standard deviations up are a tail of e^-434 only, and at fitted probabilities of 0.5 no score of this cohort reaches 40 (its
    most is sqrt n = 38.8): the null point of this test has fitted probabilities about 0.2, where the oracle's value is e^-825 --
    asserted on the oracle.  No launch of the call sums with floating-point atomics."""
    import torch
    p = _problem("pedigree")
    c, r, mu0 = 4, 19, 0.2
    null, ref = _oracle(p, c, mu0, r)
    scan = _scan(p, c, 128, mu0=mu0)
    dG, ld, dS = _block(scan, p["G"], r, torch)
    scan.sym.sync()
    S = dS.cpu().numpy().reshape(scan.q + 4, r).copy()
    z = la.solve_triangular(scan.R, S[4:4 + c], trans='T', lower=False)
    a = S[3] - np.sum(z * z, axis=0)
    j_out, j_in = 1, O.ASSOC[0]
    for j, zs in ((j_out, 1e6), (j_in, 40.0)):
        S[4 + c, j] = scan.u.dot(z[:, j]) + zs * np.sqrt(a[j])
    dS.copy_(torch.from_numpy(S.ravel()).cuda())
    gh = O.score([p["A"]], null["tau"], p["C"][:, :c], null["mu"], null["working_y"], p["G"][j_in:j_in + 1])["gh"][0]
    s40 = 40.0 * np.sqrt(ref["a_w"][j_in])
    assert s40 < np.sum(gh[gh > 0]) - gh @ null["mu"]                      # (a condition on the test's input: 40 sd is attainable)
    before = scan.sym.timing()["n_float_atomic_launches"]
    P = _spa_call(scan, dG, ld, r, dS, torch)
    assert scan.sym.timing()["n_float_atomic_launches"] == before
    assert scan.sym.spa_timing() > 0.0
    assert P[6, j_out] == 2 and P[0, j_out] == pytest.approx(np.log(2.0) + stats.norm.logsf(1e6), rel=1e-12)
    want = O.spa(gh, null["mu"], s40)
    print("zs = 40: log_p", P[0, j_in], "oracle", want["log_p"], "iters", P[5, j_in], "zeta", P[3, j_in], P[4, j_in])
    assert want["flag"] == 1 and want["log_p"] < -700                     # (a condition on the test's input, on the oracle alone)
    assert P[6, j_in] == 1 and want["flag"] == 1 and np.isfinite(P[0, j_in]) and P[0, j_in] < -700
    assert abs(P[0, j_in] - want["log_p"]) < 1e-8 * abs(want["log_p"])
    assert abs(P[3, j_in] - want["zeta_hi"]) < 1e-9 * abs(want["zeta_hi"]) and abs(P[4, j_in] - want["zeta_lo"]) < 1e-9 * abs(want["zeta_lo"])
    rest = np.setdiff1d(np.arange(r), [j_out, j_in])
    assert np.array_equal(P[6, rest], ref["spa_flag"][rest])               # the others are what the scan gives them
    gap = np.abs(P[0, rest] - ref["log_p"][rest])[ref["spa_flag"][rest] == 1]
    assert np.all(gap < 1e-8 * np.maximum(1.0, np.abs(ref["log_p"][rest][ref["spa_flag"][rest] == 1])))


def _same_bits(a, b):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_two_runs_give_the_same_bits_on_a_deterministic_handle():
    p = _problem("spd300")
    scan = _scan(p, 4, 16, deterministic=True)
    first = scan(p["G"])
    rows = scan.last_spa.copy()
    _same_bits(scan(p["G"]), first)
    assert np.array_equal(scan.last_spa, rows, equal_nan=True)
    assert scan.sym.timing()["n_float_atomic_launches"] == 0


def test_spa_call_repeats_its_bits_on_a_default_handle():
    """The same d_stats twice through the entry point on a default handle (whose sweeps may sum in another order from run to run:
    the statistics are the call's input): the call itself has no order to vary."""
    import torch
    p = _problem("spd300")
    scan = _scan(p, 4, 128)
    dG, ld, dS = _block(scan, p["G"], 128, torch)
    a = _spa_call(scan, dG, ld, 128, dS, torch)
    b = _spa_call(scan, dG, ld, 128, dS, torch)
    assert np.array_equal(a, b, equal_nan=True) and np.all(a[6, list(O.ASSOC)] == 1)


def test_bed_and_dosage_forms_give_the_bits_of_int8(tmp_path):
    from scilmm_amd import dosage
    from tests.test_bed_api import pack, write_fileset
    p = _problem("spd300")
    n = p["n"]
    scan = _scan(p, 4, 16, deterministic=True)
    G = p["G"][:37]
    ref = scan(G)
    rows = scan.last_spa.copy()
    assert (ref["spa_flag"] == 1).sum() >= 30
    path = write_fileset(tmp_path / "cohort", pack(G), n)
    _same_bits(scan.scan_bed(path), ref)
    assert np.array_equal(scan.last_spa, rows, equal_nan=True)
    codes = dosage.encode(np.where(G < 0, np.nan, G.astype(np.float64)))
    assert codes.dtype == np.uint16
    _same_bits(scan.scan_dosages(codes), ref)
    assert np.array_equal(scan.last_spa, rows, equal_nan=True)
    # a sample map: the file's samples reversed, two individuals not genotyped
    idx = np.arange(n, dtype=np.int64)[::-1].copy()
    Gm = G[:, idx].copy()
    idx[[3, 70]] = -1
    Gx = G.copy()
    Gx[:, [3, 70]] = -1
    want = scan(Gx)
    pathm = write_fileset(tmp_path / "mapped", pack(Gm), n)
    _same_bits(scan.scan_bed(pathm, sample_index=idx), want)
    _same_bits(scan.scan_dosages(dosage.encode(np.where(Gm < 0, np.nan, Gm.astype(np.float64))), sample_index=idx), want)


def test_float_dosages_against_the_oracle():
    p = _problem("spd300")
    c = 4
    null, _ = _oracle(p, c)
    rng = np.random.default_rng(5)
    D = np.clip(p["G"][:40].astype(np.float64) + rng.uniform(-0.2, 0.2, (40, p["n"])), 0.0, 2.0)
    D[p["G"][:40] < 0] = np.nan
    D = D.astype(np.float32)
    D[O.MONO] = 0.25
    ref = O.scan([p["A"]], null, p["C"][:, :c], D.astype(np.float64))
    scan = _scan(p, c, 16)
    out = scan.scan_dosages(D)
    _check_against_oracle(out, scan.last_spa, ref, ("spd300", c, "float32"))


def test_a_panel_still_runs_on_the_block_an_spa_call_followed():
    import torch
    p = _problem("spd300")
    scan = _scan(p, 4, 128, deterministic=True)
    r, T = 19, 16
    dY = torch.from_numpy(np.random.default_rng(2).standard_normal((p["n"], T))).cuda()

    def panel():
        dO = torch.zeros((r, T), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        scan.factor.scan_panel_dev(r, vp(dY.data_ptr()), T, T, vp(dO.data_ptr()), T)
        scan.sym.sync()
        return dO.cpu().numpy()

    dG, ld, dS = _block(scan, p["G"], r, torch)
    plain = panel()
    dG, ld, dS = _block(scan, p["G"], r, torch)
    P = _spa_call(scan, dG, ld, r, dS, torch)
    live = np.setdiff1d(np.arange(r), [O.MONO, O.ALLMISS])
    assert np.array_equal(panel(), plain) and np.all(plain[live] != 0.0) and np.all(P[6, live] > 0)
    # ... and through the public objects: the Gaussian panel of the working vector next to the binary scan
    out = scan.traits(scan.null.working_y[:, None])(p["G"][:r])
    ref = scan(p["G"][:r])
    ok = ~np.isnan(ref["beta"])
    assert rel_err(out["chi2"][ok, 0], ref["chi2"][ok]) < 1e-12


def test_refusals_and_argument_checks(monkeypatch):
    import torch
    from scilmm_amd import ScilmmError, _lib
    from scilmm_amd.factor import Symbolic
    p = _problem("spd300")
    scan = _scan(p, 1, 16)
    L, one, h, n = _lib.lib(), vp(8), scan.factor._h, p["n"]
    tail = lambda c=1, cut=0.0: (one, one, one, one, one, c, one, cut, one)
    for r, c in ((0, 1), (129, 1), (4, 0), (4, 32)):
        assert L.scilmm_scan_spa_dev(h, one, n, r, *tail(c)) == _lib.ERR_ARG
        assert L.scilmm_scan_spa_bed_dev(h, one, (n + 3) // 4, n, None, 0, r, *tail(c)) == _lib.ERR_ARG
        assert L.scilmm_scan_spa_dosage_dev(h, one, _lib.DOSAGE_U16, n, n, None, r, *tail(c)) == _lib.ERR_ARG
    for cut in (-1.0, float("nan")):
        assert L.scilmm_scan_spa_dev(h, one, n, 4, *tail(1, cut)) == _lib.ERR_ARG
    assert L.scilmm_scan_spa_dev(None, one, n, 4, *tail()) == _lib.ERR_ARG
    assert L.scilmm_scan_spa_dev(h, None, n, 4, *tail()) == _lib.ERR_ARG
    assert L.scilmm_scan_spa_dev(h, one, n - 1, 4, *tail()) == _lib.ERR_ARG                     # pitch shorter than a row
    assert L.scilmm_scan_spa_bed_dev(h, one, (n + 3) // 4, n, None, 2, 4, *tail()) == _lib.ERR_ARG      # an unknown flag
    assert L.scilmm_scan_spa_dosage_dev(h, one, 7, n, n, None, 4, *tail()) == _lib.ERR_ARG      # an unknown element type
    for k in range(9):                                                                          # every pointer of the common tail
        if k not in (5, 7):
            t = list(tail())
            t[k] = None
            assert L.scilmm_scan_spa_dev(h, one, n, 4, *t) == _lib.ERR_ARG, k
    ref = scan(p["G"][:20])
    # a factor consumed by the selected inverse: refused, usable again once refactorized
    dG, ld, dS = _block(scan, p["G"], 20, torch)
    scan.sym.sync()
    scan.factor.inverse_traces()
    with pytest.raises(ScilmmError):
        _spa_call(scan, dG, ld, 20, dS, torch)
    scan.factor.refactorize(scan._s2)
    _same_bits({k: v for k, v in scan(p["G"][:20]).items() if k in ("spa_flag", "n_obs")}, {k: ref[k] for k in ("spa_flag", "n_obs")})
    # fp32-product fronts
    from tests.test_gpu_halfsolve import _pedigree
    monkeypatch.setenv("SCILMM_TUNING", "1")
    monkeypatch.setenv("SCILMM_DENSE", "1")
    q = _pedigree()
    sym32 = Symbolic([q["A"], q["I"]])
    sym32.set_front_precision(32)
    f32 = sym32.factorize([0.35, 0.65])
    buf = torch.zeros((4096,), dtype=torch.float64, device="cuda")
    g8 = torch.zeros((q["A"].shape[0] + 16,), dtype=torch.int8, device="cuda")
    b = vp(buf.data_ptr())
    with pytest.raises(ScilmmError, match="fp32"):
        f32.scan_spa_dev(vp(g8.data_ptr()), q["A"].shape[0], 1, b, b, b, b, b, 1, b, 0.0, b)
    B = np.random.default_rng(0).standard_normal((q["A"].shape[0], 2))
    assert rel_err(q["V"] @ f32(B), B) < 1e-9                             # the refusal left the handle as it was


@pytest.mark.parametrize("kind,true_tau,seed", [("interior", 1.0, 5), ("boundary", 0.0, 10)])
def test_null_fit_matches_the_dense_pql(kind, true_tau, seed):
    """Prevalence 0.05, c = 3, exact traces on a deterministic handle.  The two phenotype draws are chosen so that the oracle alone
    converges within 30 iterations, to tau >= 0.2 and to the boundary."""
    from scilmm_amd import LogisticMixedModel, SparseCholesky
    p = _problem("pedigree")
    Cv = p["C"][:, :3]
    y = O.phenotype(p["A"], Cv, p["G"], 0.05, true_tau, seed)
    ref = O.fit([p["A"]], Cv, y, tol=1e-9)
    assert ref["converged"] and ref["n_iter"] <= 30                        # conditions on the test's input, on the oracle alone
    if kind == "interior":
        assert not ref["boundary"] and ref["tau"][0] >= 0.2
    else:
        assert ref["boundary"] and ref["tau"][0] == 0.0
    null = LogisticMixedModel(SparseCholesky(exact_trace=True, deterministic=True), [p["A"]], Cv, y).fit(tol=1e-9)
    print(kind, "tau", null.tau, ref["tau"], "iterations", null.n_iter, ref["n_iter"], "gaps tau %.3g alpha %.3g mu %.3g"
          % (np.abs(null.tau - ref["tau"]).max(), rel_err(null.alpha, ref["alpha"]), rel_err(null.mu, ref["mu"])))
    assert null.converged and null.n_iter == ref["n_iter"] and null.boundary == ref["boundary"]
    if kind == "interior":
        assert rel_err(null.tau, ref["tau"]) < 1e-6
    else:
        assert null.tau[0] == 0.0
    assert rel_err(null.alpha, ref["alpha"]) < 1e-6 and rel_err(null.mu, ref["mu"]) < 1e-6
    assert np.array_equal(null.sigma2_full, np.r_[null.tau, 1.0]) and len(null.mats_full) == 2
    # end to end: the scan at the fitted null, default cutoff
    out = null.scan()(p["G"][:32])
    want = O.scan([p["A"]], ref, Cv, p["G"][:32], cutoff=2.0)
    with np.errstate(invalid="ignore"):
        clear = ~(np.abs(np.abs(want["zs"]) - 2.0) < 1e-3)
    assert np.array_equal(out["spa_flag"][clear], want["spa_flag"][clear])
    ok = ~want["bad"]
    assert rel_err(out["chi2"][ok], want["chi2"][ok]) < 1e-4               # (the two nulls agree to 1e-6)
    assert np.all((out["p"][ok] > 0) & (out["p"][ok] <= 1))


def test_fit_with_the_monte_carlo_trace_runs():
    """The default SparseCholesky estimates tr(P A_k) from random vectors: the fit takes its steps on that estimate (two of them
    here; its convergence is the estimator's business) and the information comes from the factor the evaluation left resident."""
    from scilmm_amd import LogisticMixedModel, SparseCholesky
    p = _problem("spd300")
    np.random.seed(0)
    null = LogisticMixedModel(SparseCholesky(), [p["A"]], p["C"][:, :2], p["y"]).fit(max_iter=2)
    assert null.n_iter == 2 and not null.converged
    assert np.all(np.isfinite(null.tau)) and np.all(null.tau >= 0) and np.all(np.isfinite(null.alpha))
    assert np.all((null.mu > 0) & (null.mu < 1)) and null.mats_full[1].shape == (p["n"], p["n"])
