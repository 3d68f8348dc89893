"""Variant-set tests for binary traits on the device (scilmm_amd.glmm.BinarySetTest, scilmm_sets_spa*_dev,
scilmm_sets_finish_scaled_dev) against the dense oracle (tests/setspa_oracle.py), at a GIVEN null point of the cohorts of
tests/test_gpu_binary.py (pedigree n = 1502, sub100 n = 100; prevalence 0.05).

Tolerances.  flags and counts: exact.  a_B, b_B, a_w, s_B, skat_q: 1e-9 relative; burden_spa_log_p: 1e-8 max(1, |log p|); skat_p and
the SKAT-O p-values: 1e-6 relative (what tests/test_gpu_binary.py and tests/test_gpu_skato.py hold the same kinds of quantity to).
vscale, phi, burden_chi2: 1e-7 relative -- derived, not measured: with x = v^2 and log erfc(v / sqrt 2) = log p,
|dx / x| = 2 |d log p| / (v h(v)), h(v) = sqrt(2 / pi) exp(-v^2 / 2) / erfc(v / sqrt 2).  v h(v) rises from 0.571 at v = 0.5
towards v^2, while |log p| is about v^2 / 2 for a large v: at |zs| > 0.5 a log-p error of 1e-8 max(1, |log p|) moves x by at most
2e-8 / 0.571 = 3.5e-8 relative (1e-8 far out), and 1e-7 leaves a factor of about three.  Bit identity where the issue is the order
of a sum.

Worst deviations measured on an MI355X when this was written (printed by the tests with -s): a_B, b_B, a_w, s_B 4.3e-14; log_p_B
3.3e-14; vscale 1.3e-13; phi 1.3e-15; burden_chi2 8.6e-14 (1.8e-15 against x_B where the floor binds); p-values 1.2e-12; device
finish against host finish 4.4e-13."""
import ctypes as C

import numpy as np
import pytest

from scilmm_amd import binary_sets, glmm
from tests import setspa_oracle as SO
from tests import spa_oracle as O
from tests.helpers import small_pedigree

pytestmark = pytest.mark.gpu

TOL, LTOL, PTOL, VTOL = 1e-9, 1e-8, 1e-6, 1e-7
M = 130
TAU = [0.4]
RHO = np.array([0.0, 0.01, 0.04, 0.09, 0.16, 0.25, 0.5, 1.0])
vp = C.c_void_p

_PROBLEMS = {}


def _problem(name):
    """The cohorts of tests/test_gpu_binary.py::_problem, rebuilt here: (A, markers, the 31 covariate columns, y), the set list,
    and the oracle's cohorts and sets per (c, cutoff, weights); built once."""
    if name not in _PROBLEMS:
        A = small_pedigree(2000, 0.01, 0)[0]
        if name == "sub100":
            A = A[:100][:, :100].tocsr()
            A.sort_indices()
        n = A.shape[0]
        rng = np.random.default_rng(11)
        Cv = np.hstack([np.ones((n, 1)), rng.standard_normal((n, 30))])
        G = O.markers(n, M, 7)
        y = O.phenotype(A, Cv[:, :4], G, 0.05, 0.5, 3)
        assert 0 < y.sum() < n
        _PROBLEMS[name] = dict(A=A, n=n, C=Cv, G=G, y=y, b=0.4 * rng.standard_normal(n), sets=_sets(G), cohort={}, ref={})
    return _PROBLEMS[name]


def _sets(G):
    """Sizes 1, 2 and 17 (one block together), a 128-marker set (a block alone: the finish's 512-thread path), the three edge-case
    markers with two ordinary ones, the two that leave nothing, the markers with an effect, a set of the ten rarest markers, and a
    set that shares marker 20 with the first."""
    special = {O.MONO, O.ALLMISS, O.MISS30} | set(O.ASSOC)
    freq = np.where(G < 0, 0, G).sum(axis=1) / np.maximum((G >= 0).sum(axis=1), 1)
    rare = [int(j) for j in np.argsort(freq, kind="stable") if int(j) not in special][:10]
    return [np.array([20]), np.array([21, 22]), np.arange(23, 40), np.arange(128), np.array([O.MONO, O.ALLMISS, O.MISS30, 50, 51]),
            np.array([O.MONO, O.ALLMISS]), np.array(list(O.ASSOC) + [60, 61]), np.array(rare), np.array([20, 100, 101, 102])]


NOTHING, ASSOC_SET, RARE_SET = 5, 6, 7


def _alpha(c, mu0=0.05):
    return np.r_[np.log(mu0 / (1 - mu0)), 0.15 * np.random.default_rng(c).standard_normal(c - 1)]


def _given(p):
    rng = np.random.default_rng(5)
    return [rng.uniform(0.5, 2.0, s.size) for s in p["sets"]]


def _cohort(p, c):
    if c not in p["cohort"]:
        Cc = p["C"][:, :c]
        eta = Cc @ _alpha(c) + p["b"]
        mu = 1 / (1 + np.exp(-eta))
        p["cohort"][c] = SO.Cohort([p["A"]], np.array(TAU), Cc, mu, eta + (p["y"] - mu) / (mu * (1 - mu)), p["G"])
    return p["cohort"][c]


def _oracle(p, c, weights, cutoff):
    """The oracle's result per set for (c, weights: "beta" / None / "given", cutoff)."""
    key = (c, weights, cutoff)
    if key not in p["ref"]:
        co = _cohort(p, c)
        given = _given(p)
        p["ref"][key] = [SO.set_test(co, s, given[i] if weights == "given" else weights, cutoff, RHO) for i, s in enumerate(p["sets"])]
    return p["ref"][key]


def _null(p, c, **kw):
    from scilmm_amd import LogisticMixedModel, SparseCholesky
    model = LogisticMixedModel(SparseCholesky(**kw), [p["A"]], p["C"][:, :c], p["y"])
    return model.null_at(TAU, _alpha(c), p["b"])


def _tester(p, c, block=128, cutoff=2.0, **kw):
    return _null(p, c, **kw).sets(block=block, cutoff=cutoff)


def _weights(p, weights):
    return _given(p) if weights == "given" else weights


def _rel(a, b):
    return abs(a - b) / abs(b)


def _check_oracle_inputs(ref, cutoff, rich, floor):
    """Conditions on the tests' inputs, from the oracle alone: no standardised score at the cutoff (a flag cannot flip on rounding);
    `rich`: at least three sets hold an adjusted marker; `floor`: the burden floor binds in at least one set."""
    live = [r for r in ref if r["n_used"]]
    assert not rich or sum(r["n_adj"] > 0 for r in live) >= 3
    assert not floor or any(r["phi"] > 1.0 for r in live)
    for r in live:
        z = np.r_[r["zs"], r["zs_B"]]
        assert not np.any(np.abs(np.abs(z[np.isfinite(z)]) - cutoff) < 1e-6)
    assert ref[NOTHING]["n_used"] == 0


@pytest.mark.parametrize("name,c,weights,cutoff,rich,floor", [("pedigree", 4, "beta", 2.0, True, False), ("pedigree", 1, None, 0.5, True, True),
                                                              ("pedigree", 31, "given", 2.0, True, True), ("sub100", 4, "beta", 0.5, True, True),
                                                              ("sub100", 31, None, 2.0, False, False), ("sub100", 1, "given", 0.5, True, False)])
def test_host_finish_matches_the_dense_oracle(name, c, weights, cutoff, rich, floor):
    p = _problem(name)
    ref = _oracle(p, c, weights, cutoff)
    _check_oracle_inputs(ref, cutoff, rich, floor)
    tester = _tester(p, c, cutoff=cutoff)
    out = tester(p["G"], p["sets"], weights=_weights(p, weights), skato=True, rho=RHO, return_kernel=True)
    B = tester.last_bspa
    worst = {}

    def close(what, got, want, tol):
        e = _rel(got, want)
        worst[what] = max(worst.get(what, 0.0), e)
        assert e < tol, (name, c, weights, cutoff, i, what, got, want, e)

    for i, r in enumerate(ref):
        assert out["n_used"][i] == r["n_used"] and out["n_adjusted"][i] == r["n_adj"] and out["burden_spa_flag"][i] == r["flag"], i
        if not r["n_used"]:
            assert np.all(np.isnan([out[k][i] for k in ("burden_chi2", "burden_p", "skat_p", "skato_p", "burden_scale", "burden_spa_log_p")]))
            assert out["kernel"][i] is None or out["kernel"][i][0].size == 0
            continue
        close("a_B", B[i, 7], r["a_B"], TOL)
        close("b_B", B[i, 8], r["b_B"], TOL)
        close("V_Q", B[i, 10], r["V_Q"], VTOL)
        close("burden_chi2_norm", out["burden_chi2_norm"][i], r["burden_chi2_norm"], TOL)
        close("skat_q", out["skat_q"][i], r["skat_q"], TOL)
        if r["flag"]:
            close("a_w", B[i, 1], r["a_w"], TOL)
            close("s_B", B[i, 2], r["s_B"], TOL)
            gap = abs(out["burden_spa_log_p"][i] - r["log_p"]) / max(1.0, abs(r["log_p"]))
            worst["log_p"] = max(worst.get("log_p", 0.0), gap)
            assert gap < LTOL, (i, gap)
        else:
            assert np.all(np.isnan(B[i, :6]))
        s, Kt, w, vs = out["kernel"][i]
        assert np.max(np.abs(vs - r["vscale"]) / r["vscale"]) < VTOL, i
        worst["vscale"] = max(worst.get("vscale", 0.0), float(np.max(np.abs(vs - r["vscale"]) / r["vscale"])))
        Kref = r["vscale"][:, None] * r["K"] * r["vscale"][None, :]
        assert np.max(np.abs(Kt - Kref)) < VTOL * np.max(np.abs(Kref)), i
        close("phi", out["burden_scale"][i], r["phi"], VTOL)
        close("burden_chi2", out["burden_chi2"][i], r["burden_chi2"], VTOL)
        close("burden_beta", out["burden_beta"][i], r["burden_beta"], VTOL)
        close("burden_se", out["burden_se"][i], r["burden_se"], VTOL)
        if r["phi"] > 1.0:
            close("chi2 at the floor", out["burden_chi2"][i], r["x_B"], VTOL)
        close("burden_p", out["burden_p"][i], r["burden_p"], PTOL)
        for k in ("skat_p", "skato_p", "skato_pmin"):
            close(k, out[k][i], r[k], PTOL)
        assert np.max(np.abs(out["skato_p_rho"][i] - r["skato_p_rho"]) / r["skato_p_rho"]) < PTOL, i
    print(name, c, weights, cutoff, "worst deviations", worst, "phi", [round(r["phi"], 4) for r in ref if r["n_used"]],
          "n_adj", [r["n_adj"] for r in ref])


def test_the_adjustment_changes_the_answer():
    """Without the feature: the unadjusted VariantSetTest on the working vector gives another skat_p than the oracle, by far more
    than the comparison tolerance, for the set of the markers with an effect and for the rare-variant set."""
    from scilmm_amd import SparseCholesky, VariantSetTest
    p = _problem("pedigree")
    ref = _oracle(p, 1, None, 0.5)
    null = _null(p, 1)
    plain = VariantSetTest(SparseCholesky(), null.mats_full, null.sigma2_full, p["C"][:, :1], null.working_y, block=128)(p["G"], p["sets"], weights=None)
    for i in (ASSOC_SET, RARE_SET):
        assert ref[i]["n_adj"] > 0
        gap = _rel(plain["skat_p"][i], ref[i]["skat_p"])
        print("set", i, "unadjusted skat_p", plain["skat_p"][i], "oracle", ref[i]["skat_p"], "n_adj", ref[i]["n_adj"], "phi", ref[i]["phi"])
        assert gap > 10 * PTOL, (i, gap)


class _Block(object):
    """One block at the C level: the marker rows on the device, the Gram entry point and the markers' saddlepoint call run once;
    ``S``, ``G``, ``P`` are their results on the host, and ``sets_spa`` / ``finish`` run on whatever the caller uploads."""

    def __init__(self, tester, G, rows):
        import torch
        from scilmm_amd.markers import Int8Rows
        self.t, self.torch, self.rb = tester, torch, len(rows)
        rb, q = self.rb, tester.q
        self.src = Int8Rows(tester, G)
        self.src.stage(128)
        self.src.load(np.asarray(rows))
        new = lambda k: torch.full((k,), -7.25, dtype=torch.float64, device="cuda")
        self.dS, self.dK, self.dP = new((q + 4) * rb), new(rb * rb), new(glmm.SPA_ROWS * rb)
        torch.cuda.synchronize()
        self.src.enqueue(0, rb, vp(self.dS.data_ptr()), vp(self.dK.data_ptr()))
        self.src.spa(0, rb, (vp(self.dS.data_ptr()),) + self.null(tester.cutoff) + (vp(self.dP.data_ptr()),))
        tester.sym.sync()
        self.S = self.dS.cpu().numpy().reshape(q + 4, rb).copy()
        self.G = self.dK.cpu().numpy().reshape(rb, rb).copy()
        self.P = self.dP.cpu().numpy().reshape(glmm.SPA_ROWS, rb).copy()

    def null(self, cutoff):
        t = self.t
        return (vp(t.dR.data_ptr()), vp(t.du.data_ptr()), vp(t.dmu.data_ptr()), vp(t.dC.data_ptr()), t.c, vp(t.dMinv.data_ptr()), cutoff)

    def upload(self, S=None, G=None, P=None):
        for d, h in ((self.dS, S), (self.dK, G), (self.dP, P)):
            if h is not None:
                d.copy_(self.torch.from_numpy(np.ascontiguousarray(h).ravel()))
        self.torch.cuda.synchronize()

    def sets_spa(self, start, cutoff, mode=1, weights=None):
        """(n_sets x 13 rows, r scales); exactly the documented doubles are written."""
        torch, rb = self.torch, self.rb
        start = np.asarray(start, dtype=np.int32)
        ns = start.size - 1
        dB = torch.full((ns * 13 + 3,), -7.25, dtype=torch.float64, device="cuda")
        self.dV = torch.full((rb + 3,), -7.25, dtype=torch.float64, device="cuda")
        dW = torch.from_numpy(np.ascontiguousarray(weights)).cuda() if weights is not None else None
        torch.cuda.synchronize()
        self.src.sets_spa(0, rb, (vp(self.dS.data_ptr()), vp(self.dK.data_ptr())) + self.null(cutoff) +
                          (vp(self.dP.data_ptr()), ns, start, mode, vp(dW.data_ptr()) if dW is not None else None, vp(dB.data_ptr()),
                           vp(self.dV.data_ptr())))
        self.t.sym.sync()
        B, V = dB.cpu().numpy(), self.dV.cpu().numpy()
        assert np.all(B[ns * 13:] == -7.25) and np.all(V[rb:] == -7.25) and not np.any(B[:ns * 13] == -7.25)
        assert not np.any(V[:start[-1]] == -7.25) and np.all(V[start[-1]:rb] == -7.25)        # columns outside every set: not written
        return B[:ns * 13].reshape(ns, 13), V[:rb]

    def finish(self, start, scaled, mode=1, rho=RHO, dV=None):
        torch, t, rb = self.torch, self.t, self.rb
        start = np.asarray(start, dtype=np.int32)
        ns, ld = start.size - 1, 10 + len(rho)
        dO = torch.full((ns * ld,), -7.25, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        args = (rb, t.q, vp(self.dS.data_ptr()), vp(self.dK.data_ptr()), vp(t.dR.data_ptr()), vp(t.du.data_ptr()), t.c, ns, start, mode,
                None, 0, rho, vp(dO.data_ptr()), ld, None)
        if scaled:
            t.factor.sets_finish_scaled_dev(*(args + (vp(dV.data_ptr()),)))
        else:
            t.factor.sets_finish_dev(*args)
        t.sym.sync()
        return dO.cpu().numpy().reshape(ns, ld)


def test_doctored_marker_rows_at_the_c_level():
    """Per-marker saddlepoint rows written by hand: log_p = 0, +1e-3, NaN with flag 1, flag 2 and flag 0 give a scale of exactly 1;
    log_p = -800 (p underflows) gives a finite scale that agrees with the oracle's root.  The cutoff of the set call is out of
    reach, so no burden is attempted and phi = 1."""
    import torch
    from scilmm_amd.sets import set_kernel
    p = _problem("pedigree")
    tester = _tester(p, 4)
    rows = np.arange(20, 28)
    blk = _Block(tester, p["G"], rows)
    P = blk.P.copy()
    P[:, :] = np.nan
    P[6] = [1, 1, 1, 2, 0, 1, 1, 1]
    P[0] = [0.0, 1e-3, np.nan, -5.0, -5.0, -800.0, -3.0, -1e-3]
    blk.upload(P=P)
    n0 = tester.sym.timing()["n_float_atomic_launches"]
    B, V = blk.sets_spa([0, 8], cutoff=1e9)
    assert tester.sym.timing()["n_float_atomic_launches"] == n0
    assert tester.factor.sets_spa_timing() == tester.sym.sets_spa_timing() > 0.0
    assert np.all(V[:5] == 1.0) and B[0, 6] == 0 and B[0, 11] == 1.0 and B[0, 12] == 3 and np.all(np.isnan(B[0, :6])) and np.isnan(B[0, 9])
    s, K, w, keep = set_kernel(blk.S, blk.G, tester.R, tester.u, None)
    assert keep.all()
    zs = s / np.sqrt(np.diag(K))
    for j, lp in ((5, -800.0), (6, -3.0), (7, -1e-3)):
        want = abs(zs[j]) / SO.deviate(lp)
        print("log_p", lp, "scale", V[j], "oracle", want)
        assert np.isfinite(V[j]) and _rel(V[j], want) < 1e-9, (j, V[j], want)
    # V_Q and a_B from the same K: the scales enter V_Q alone
    assert _rel(B[0, 7], K.sum()) < TOL and _rel(B[0, 10], V[:8] @ K @ V[:8]) < TOL and _rel(B[0, 8], s.sum()) < TOL
    # the scaled finish on these scales: A = diag(w o scale) K diag(w o scale), t unchanged; bit 4 of the flags
    rows_s = blk.finish([0, 8], True, dV=blk.dV)
    t = binary_sets.scaled_tests(s, K, w, V[:8], "saddlepoint", RHO)
    assert int(rows_s[0, 9]) & binary_sets.FLAG_SCALED
    for col, k in ((1, "burden_beta"), (2, "burden_se"), (3, "burden_chi2"), (4, "skat_q")):
        assert _rel(rows_s[0, col], t[k]) < TOL, k
    assert _rel(rows_s[0, 5], t["skat_p"]) < PTOL and _rel(rows_s[0, 6], t["skato"][0]) < PTOL
    assert np.max(np.abs(rows_s[0, 10:] - t["skato"][3]) / t["skato"][3]) < PTOL


def test_scaled_finish_with_unit_scales_gives_the_bits_of_the_plain_finish():
    import torch
    p = _problem("pedigree")
    tester = _tester(p, 4)
    members = [p["sets"][i] for i in (0, 1, 2, 4, 5, 6)]
    start = np.concatenate([[0], np.cumsum([m.size for m in members])])
    for rows, st in ((np.concatenate(members), start), (np.arange(128), np.array([0, 128]))):
        blk = _Block(tester, p["G"], rows)
        ones = torch.ones((blk.rb,), dtype=torch.float64, device="cuda")
        for mode in (0, 1):
            plain = blk.finish(st, False, mode=mode)
            scaled = blk.finish(st, True, mode=mode, dV=ones)
            assert np.array_equal(plain, scaled, equal_nan=True)
            assert not np.any(plain[:, 9].astype(int) & binary_sets.FLAG_SCALED)
            assert not np.any(np.isnan(plain[plain[:, 0] > 0][:, :6]))


def test_a_set_gives_the_same_bits_wherever_it_lies():
    """The rare-variant set alone, last in a full block and between two others: the block's statistics, Gram matrix and marker rows
    of the set are written in from the first layout (they are the call's inputs), so the set call and the scaled finish see the same
    numbers at other columns and next to other neighbours.  Twice each: two runs give the same bits."""
    p = _problem("pedigree")
    tester = _tester(p, 1, cutoff=0.5)
    x = p["sets"][RARE_SET]
    k = x.size
    filler = np.setdiff1d(np.arange(M), x)
    layouts = {"alone": ([x], 0), "last in a full block": ([filler[:128 - k], x], 1), "between two": ([filler[:5], x, filler[5:75]], 1)}
    ref, got = None, {}
    for name, (members, at) in layouts.items():
        start = np.concatenate([[0], np.cumsum([m.size for m in members])])
        blk = _Block(tester, p["G"], np.concatenate(members))
        a, b = start[at], start[at + 1]
        if ref is None:
            ref = (blk.S[:, a:b].copy(), blk.G[a:b, a:b].copy(), blk.P[:, a:b].copy())
        blk.S[:, a:b], blk.G[a:b, a:b], blk.P[:, a:b] = ref
        blk.upload(S=blk.S, G=blk.G, P=blk.P)
        n0 = tester.sym.timing()["n_float_atomic_launches"]    # (the Gram block of a default handle has counted its own)
        B, V = blk.sets_spa(start, 0.5)
        fin = blk.finish(start, True, dV=blk.dV)
        B2, V2 = blk.sets_spa(start, 0.5)
        fin2 = blk.finish(start, True, dV=blk.dV)
        assert np.array_equal(B, B2, equal_nan=True) and np.array_equal(V, V2) and np.array_equal(fin, fin2, equal_nan=True), name
        assert tester.sym.timing()["n_float_atomic_launches"] == n0
        got[name] = (B[at], V[a:b], fin[at])
    assert got["alone"][0][6] == 1 and got["alone"][0][12] > 0            # the burden was saddlepointed, markers were adjusted
    for name in ("last in a full block", "between two"):
        for u, v in zip(got[name], got["alone"]):
            assert np.array_equal(u, v, equal_nan=True), name


def _same(a, b, keys=None):
    for k in keys or a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_two_runs_and_the_three_input_forms_give_the_same_bits(tmp_path):
    from scilmm_amd import dosage
    from tests.test_bed_api import pack, write_fileset
    p = _problem("sub100")
    tester = _tester(p, 4, cutoff=0.5, deterministic=True)
    kw = dict(skato=True, finish="device")
    first = tester(p["G"], p["sets"], **kw)
    rows = tester.last_bspa.copy()
    assert (first["burden_spa_flag"] == 1).sum() >= 3 and (first["n_adjusted"] > 0).sum() >= 3
    _same(tester(p["G"], p["sets"], **kw), first)
    assert np.array_equal(tester.last_bspa, rows, equal_nan=True)
    path = write_fileset(tmp_path / "cohort", pack(p["G"]), p["n"])
    _same(tester.test_bed(path, p["sets"], **kw), first)
    assert np.array_equal(tester.last_bspa, rows, equal_nan=True)
    codes = dosage.encode(np.where(p["G"] < 0, np.nan, p["G"].astype(np.float64)))
    assert codes.dtype == np.uint16
    _same(tester.test_dosages(codes, p["sets"], **kw), first)
    assert np.array_equal(tester.last_bspa, rows, equal_nan=True)
    assert tester.sym.timing()["n_float_atomic_launches"] == 0


@pytest.mark.parametrize("name,c,weights", [("pedigree", 4, "beta"), ("sub100", 31, "given"), ("sub100", 1, None)])
def test_device_finish_matches_host_finish_end_to_end(name, c, weights):
    p = _problem(name)
    tester = _tester(p, c, cutoff=0.5, deterministic=True)
    w = _weights(p, weights)
    host = tester(p["G"], p["sets"], weights=w, skato=True)
    dev = tester(p["G"], p["sets"], weights=w, skato=True, finish="device")
    from scilmm_amd.sets import KEYS, SKATO_KEYS
    assert sorted(dev) == sorted(host) == sorted(KEYS + SKATO_KEYS + binary_sets.BINARY_KEYS)
    _same(dev, host, ("n_used", "n_adjusted", "burden_spa_flag", "burden_spa_log_p", "burden_scale", "burden_chi2_norm", "skato_rho"))
    live = host["n_used"] > 0
    assert live.sum() == len(p["sets"]) - 1
    worst = 0.0
    for k in ("burden_beta", "burden_se", "burden_chi2", "burden_p", "skat_q", "skat_p", "skato_p", "skato_pmin", "skato_p_rho"):
        assert np.all(np.isnan(dev[k][~live])) and not np.any(np.isnan(dev[k][live])), k
        e = float(np.max(np.abs(dev[k][live] - host[k][live]) / np.abs(host[k][live])))
        worst = max(worst, e)
        assert e < PTOL, (k, e)
    print(name, c, weights, "device finish against host finish, worst rel. deviation", worst)


def test_refusals_and_argument_checks(monkeypatch):
    import torch
    from scilmm_amd import ScilmmError, _lib
    from scilmm_amd.factor import Symbolic
    p = _problem("sub100")
    tester = _tester(p, 1)
    L, one, h, n = _lib.lib(), vp(8), tester.factor._h, p["n"]
    start = np.array([0, 2, 5], dtype=np.int32)
    good = dict(stats=one, gram=one, R=one, u=one, mu=one, C=one, c=1, Minv=one, cutoff=2.0, spa=one, n_sets=2, start=_lib.ptr(start),
                mode=1, w=None, bspa=one, vscale=one)
    bad_start = [np.array(v, dtype=np.int32) for v in ([1, 2, 5], [0, 2, 6], [0, 2, 2], [0, 3, 2])]
    cases = [dict([(k, None)]) for k in ("stats", "gram", "R", "u", "mu", "C", "Minv", "spa", "start", "bspa", "vscale")]
    cases += [dict(c=0), dict(c=32), dict(cutoff=-1.0), dict(cutoff=float("nan")), dict(n_sets=0), dict(n_sets=6), dict(mode=3),
              dict(mode=2, w=None)] + [dict(start=_lib.ptr(v)) for v in bad_start]
    forms = [(L.scilmm_sets_spa_dev, [one, n]), (L.scilmm_sets_spa_bed_dev, [one, (n + 3) // 4, n, None, 0]),
             (L.scilmm_sets_spa_dosage_dev, [one, _lib.DOSAGE_U16, n, n, None])]
    for fn, head in forms:
        for kw in cases:
            a = dict(good, **kw)
            assert fn(h, *head, 5, *[a[k] for k in good]) == _lib.ERR_ARG, (fn.__name__, kw)
        for r in (0, 129):
            assert fn(h, *head, r, *good.values()) == _lib.ERR_ARG
        assert fn(None, *head, 5, *good.values()) == _lib.ERR_ARG and fn(h, None, *head[1:], 5, *good.values()) == _lib.ERR_ARG
    assert L.scilmm_sets_spa_dev(h, one, n - 1, 5, *good.values()) == _lib.ERR_ARG                  # pitch shorter than a row
    assert L.scilmm_sets_spa_bed_dev(h, one, (n + 3) // 4, n, None, 2, 5, *good.values()) == _lib.ERR_ARG   # an unknown flag
    assert L.scilmm_sets_spa_dosage_dev(h, one, 7, n, n, None, 5, *good.values()) == _lib.ERR_ARG   # an unknown element type
    rho = np.array([0.0, 0.5, 1.0])
    fgood = dict(fac=h, r=5, q=2, stats=one, gram=one, R=one, u=one, c=1, n_sets=2, start=_lib.ptr(start), mode=1, w=None, method=0,
                 rho=_lib.ptr(rho), n_rho=3, out=one, ld=13, lam=None, vscale=one)
    fcases = [dict(fac=None), dict(stats=None), dict(gram=None), dict(R=None), dict(u=None), dict(start=None), dict(out=None), dict(vscale=None),
              dict(rho=None), dict(r=0), dict(r=129), dict(c=0, q=1), dict(c=32, q=33), dict(q=4), dict(n_sets=0), dict(n_sets=6),
              dict(n_rho=-1), dict(n_rho=17), dict(ld=12), dict(mode=3), dict(mode=2, w=None), dict(method=2)]
    fcases += [dict(start=_lib.ptr(v)) for v in bad_start]
    for kw in fcases:
        a = dict(fgood, **kw)
        assert L.scilmm_sets_finish_scaled_dev(*[a[k] for k in fgood]) == _lib.ERR_ARG, kw
    # the handle is as usable as before; a factor consumed by the selected inverse is refused, and usable again once refactorized
    sets = p["sets"][:3]
    ref = tester(p["G"], sets, finish="device")
    blk = _Block(tester, p["G"], np.arange(8))
    tester.factor.inverse_traces()
    with pytest.raises(ScilmmError):
        blk.sets_spa([0, 8], 2.0)
    ones = torch.ones((8,), dtype=torch.float64, device="cuda")
    with pytest.raises(ScilmmError):
        blk.finish([0, 8], True, dV=ones)
    tester.factor.refactorize(tester._s2)
    _same(tester(p["G"], sets, finish="device"), ref, ("n_used", "n_adjusted", "burden_spa_flag"))
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
        f32.sets_spa_dev(vp(g8.data_ptr()), q["A"].shape[0], 1, b, b, b, b, b, b, 1, b, 2.0, b, 1, np.array([0, 1], dtype=np.int32), 1, None, b, b)
    with pytest.raises(ScilmmError, match="fp32"):
        f32.sets_finish_scaled_dev(5, 2, b, b, b, b, 1, 2, start, 1, None, 0, rho, b, 13, None, b)
    Bm = np.random.default_rng(0).standard_normal((q["A"].shape[0], 2))
    from tests.helpers import rel_err
    assert rel_err(q["V"] @ f32(Bm), Bm) < 1e-9                            # the refusals left the handle as it was


def test_a_distributed_handle_is_refused():
    """One rank of a world of two, never factorized (that would need the other rank): the refusal comes before any device work."""
    import torch
    from scilmm_amd import ScilmmError
    from scilmm_amd.dist import HipChainEngine
    from tests.test_gpu_halfsolve import _pedigree
    q = _pedigree()
    eng = HipChainEngine([q["A"], q["I"]], 0, 2, None, "cuda:0")
    buf = torch.zeros((4096,), dtype=torch.float64, device="cuda")
    g8 = torch.zeros((q["A"].shape[0] + 16,), dtype=torch.int8, device="cuda")
    b = vp(buf.data_ptr())
    start = np.array([0, 2, 5], dtype=np.int32)
    with pytest.raises(ScilmmError, match="distributed"):
        eng.fac.sets_spa_dev(vp(g8.data_ptr()), q["A"].shape[0], 5, b, b, b, b, b, b, 1, b, 2.0, b, 2, start, 1, None, b, b)
    with pytest.raises(ScilmmError, match="distributed"):
        eng.fac.sets_finish_scaled_dev(5, 2, b, b, b, b, 1, 2, start, 1, None, 0, np.array([0.0, 1.0]), b, 12, None, b)
    assert eng.collectives == 0
