"""VariantSetTest / scilmm_scan_block_gram_dev against the un-whitened set statistics written here with the dense inv(V) and
the explicit P = V^-1 - V^-1 C (C' V^-1 C)^-1 C' V^-1 -- which shares nothing with the code under test.

Tolerances: 1e-9 relative (max-norm, tests.helpers.rel_err) for s, K, the weights, the eigenvalues and the derived
statistics, what the suite holds for derived statistics (the two forms agree to 9e-14 on the CPU at these inputs); n_used
exact; NaN exactly where a set has nothing left; p-values bit for bit the module's own functions of the returned
statistics, and within 1e-6 relative of the same functions of the oracle's statistics.  At the C level: the statistics of the
Gram entry points bit for bit those of the plain ones, the Gram matrix bitwise symmetric, its diagonal within 1e-12 of the gg
row (another summation order), its entries within 1e-9 of X'X from Factor.solve_L, exactly r * r values written.
Reference skat_p of the two planted sets, computed on the CPU when this was written: between 1.9e-10 and 4e-3 over the three problems and both c
(the test asserts 1e-12 < p < 0.1)."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp
import scipy.stats as stats

from tests import test_bed_api as T
from tests.helpers import random_spd, rel_err, small_pedigree

pytestmark = pytest.mark.gpu

TOL = 1e-9
M = 304                      # markers: the four edge cases and 300 rare ones
MONO, ALLMISS, FULL, ENDS = 0, 1, 2, 3
S2 = [0.4, 0.6]
SIZES = (1, 2, 16, 17, 100, 28, 29, 128)
PLANTED = (3, 5)             # the sets with an effect on y
EFFECT = {"pedigree": 0.024, "spd300": 0.2, "spd203": 0.25}
KEYS = ("n_used", "burden_beta", "burden_se", "burden_chi2", "burden_p", "skat_q", "skat_p")


def _markers(n, m, seed):
    """binomial(2, MAF), MAF uniform 0.005-0.05, 2 % missing (-1); four markers overwritten with the edge cases."""
    rng = np.random.default_rng(seed)
    maf = rng.uniform(0.005, 0.05, m)
    G = rng.binomial(2, maf[:, None], size=(m, n)).astype(np.int8)
    G[rng.random((m, n)) < 0.02] = -1
    G[MONO] = 1                                   # monomorphic
    G[ALLMISS] = -1                               # nothing observed
    G[FULL] = rng.binomial(2, 0.3, n)             # no missing value
    G[ENDS] = rng.binomial(2, 0.3, n)
    G[ENDS, 0] = G[ENDS, -1] = -1                 # missing at the first and the last individual only
    return np.ascontiguousarray(G)


def _sets():
    """Sizes 1, 2, 16, 17, 100, 28, 29, 128 in that order, then the set of the two degenerate markers alone.  Set 2 holds the
    monomorphic and the all-missing marker, set 3 the two other edge markers and marker 5, which set 1 holds as well; set 7
    is drawn from all the rare markers, unsorted, so it overlaps the others."""
    sets, at = [], 4
    for k, size in enumerate(SIZES[:7]):
        head = {2: [MONO, ALLMISS], 3: [FULL, ENDS, 5]}.get(k, [])
        body = size - len(head)
        sets.append(np.array(head[:1] + list(range(at, at + body)) + head[1:], dtype=np.int64))
        at += body
    sets.append(np.random.default_rng(5).permutation(np.arange(4, M))[:128])
    sets.append(np.array([ALLMISS, MONO]))
    assert [s.size for s in sets] == list(SIZES) + [2] and at <= M
    return sets


def _centred(G):
    obs = G >= 0
    n_obs = obs.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(obs, G, 0).sum(axis=1) / n_obs
    Gt = np.where(obs, G - np.where(n_obs > 0, mean, 0.0)[:, None], 0.0)
    return n_obs, mean, Gt


_PROBLEMS = {}


def _problem(name):
    """Matrices, markers, sets, covariates and a phenotype with effects planted on the markers of two sets, built once."""
    if name not in _PROBLEMS:
        A = {"pedigree": lambda: small_pedigree(2000, 0.01, 0)[0], "spd300": lambda: random_spd(300, 0.05, 3),
             "spd203": lambda: random_spd(203, 0.05, 5)}[name]()
        n = A.shape[0]
        rng = np.random.default_rng(11)
        Cv = np.hstack([np.ones((n, 1)), rng.standard_normal((n, 3))])
        G, sets = _markers(n, M, 7), _sets()
        _, _, Gt = _centred(G)
        y = Cv @ np.array([0.5, -0.2, 0.1, 0.3]) + rng.standard_normal(n)
        for k in PLANTED:                       # effects of both signs, each worth EFFECT standard deviations of y per marker
            sd = np.sqrt(np.maximum((Gt[sets[k]] ** 2).sum(axis=1), 1.0) / n)
            y = y + (EFFECT[name] * rng.choice([-1.0, 1.0], sets[k].size) / sd) @ Gt[sets[k]]
        _PROBLEMS[name] = dict(A=A, I=sp.identity(n, format="csr"), n=n, C=Cv, y=y, G=G, sets=sets, ref={}, testers={})
    return _PROBLEMS[name]


def _oracle(p, c, sets, weights="beta", method="saddlepoint"):
    """Per set: (s, K, w) over the markers that are left, the eigenvalues and every statistic, from the un-whitened formula."""
    from scilmm_amd import sets as mod
    key = (c, weights is None, method, tuple(s.tobytes() for s in sets))
    if key in p["ref"]:
        return p["ref"][key]
    if "P" not in p or c not in p["P"]:
        Vi = np.linalg.inv((S2[0] * p["A"] + S2[1] * p["I"]).toarray())
        Cv = p["C"][:, :c]
        ViC = Vi @ Cv
        p.setdefault("P", {})[c] = Vi - ViC @ np.linalg.solve(Cv.T @ ViC, ViC.T)
    P, y, n = p["P"][c], p["y"], p["n"]
    n_obs, mean, Gt = _centred(p["G"])
    sf = {"saddlepoint": mod.mixture_sf_saddlepoint, "liu": mod.mixture_sf_liu}[method]
    ref = {k: np.full(len(sets), np.nan) for k in KEYS}
    ref["n_used"] = np.zeros(len(sets), dtype=np.int64)
    ref["kernel"], ref["lam"] = [], []
    for i, rows in enumerate(sets):
        rows = np.array([j for j in rows if n_obs[j] > 0 and Gt[j].any()], dtype=np.int64)
        X = Gt[rows]
        s, K = X @ (P @ y), X @ P @ X.T
        w = stats.beta.pdf(np.minimum(mean[rows] / 2, 1 - mean[rows] / 2), 1, 25) if weights == "beta" else np.ones(rows.size)
        ref["kernel"].append((s, K, w))
        ref["n_used"][i] = rows.size
        lam = np.linalg.eigvalsh(w[:, None] * K * w[None, :]) if rows.size else np.empty(0)
        ref["lam"].append(lam)
        if rows.size:
            ws, wKw = w @ s, w @ K @ w
            ref["burden_beta"][i], ref["burden_se"][i], ref["burden_chi2"][i] = ws / wKw, wKw ** -0.5, ws * ws / wKw
            ref["burden_p"][i] = stats.f(1, n - 1).sf(ws * ws / wKw)
            ref["skat_q"][i] = np.sum(w * w * s * s)
            ref["skat_p"][i] = sf(ref["skat_q"][i], lam[lam > 1e-10 * lam.max()])
    p["ref"][key] = ref
    return ref


def _tester(p, c, block, deterministic=False):
    """One object per (problem, c, block, mode), shared by the tests."""
    from scilmm_amd import SparseCholesky, VariantSetTest
    key = (c, block, deterministic)
    if key not in p["testers"]:
        p["testers"][key] = VariantSetTest(SparseCholesky(deterministic=deterministic), [p["A"], p["I"]], S2, p["C"][:, :c], p["y"],
                                           block=block)
    return p["testers"][key]


def _compare(out, ref, n, method="saddlepoint"):
    from scilmm_amd import sets as mod
    sf = {"saddlepoint": mod.mixture_sf_saddlepoint, "liu": mod.mixture_sf_liu}[method]
    assert out["n_used"].dtype.kind == "i" and np.array_equal(out["n_used"], ref["n_used"])
    bad = ref["n_used"] == 0
    for k in ("burden_beta", "burden_se", "burden_chi2", "skat_q"):
        print(k, "rel.err", rel_err(out[k][~bad], ref[k][~bad]))
        assert rel_err(out[k][~bad], ref[k][~bad]) < TOL, k
    for k in KEYS[1:]:
        assert np.array_equal(np.isnan(out[k]), bad), k              # NaN exactly at the sets with nothing left
    for i, ((s, K, w), (s0, K0, w0)) in enumerate(zip(out["kernel"], ref["kernel"])):
        assert s.shape == s0.shape and K.shape == K0.shape and w.shape == w0.shape, i
        if not s0.size:
            continue
        assert rel_err(s, s0) < TOL and rel_err(K, K0) < TOL and rel_err(w, w0) < TOL, (i, rel_err(s, s0), rel_err(K, K0))
        assert np.array_equal(K, K.T), i
        lam = scipy.linalg.eigvalsh(w[:, None] * K * w[None, :])       # (the module's solver: another one gives other last bits)
        assert rel_err(lam, ref["lam"][i]) < TOL, (i, rel_err(lam, ref["lam"][i]))
        # the p-values: the module's own functions of the returned statistics, bit for bit
        assert out["burden_p"][i] == stats.f(1, n - 1).sf(out["burden_chi2"][i]), i
        assert out["skat_p"][i] == sf(out["skat_q"][i], lam[lam > 1e-10 * lam.max()]), i
    for k in ("burden_p", "skat_p"):
        d = np.abs(out[k][~bad] - ref[k][~bad]) / ref[k][~bad]
        print(k, "max rel. deviation from the reference p", d.max())
        assert d.max() < 1e-6, k


def _fit(sets, block):
    return [s for s in sets if s.size <= block]


@pytest.mark.parametrize("block", [16, 112, 128])
@pytest.mark.parametrize("c", [1, 4])
@pytest.mark.parametrize("name", ["pedigree", "spd300", "spd203"])
def test_sets_match_the_unwhitened_formula(name, c, block):
    p = _problem(name)
    if name == "spd203":
        assert p["n"] % 4 != 0                    # the last MFMA k-step is ragged, and n is shorter than one slice
    tester = _tester(p, c, block)
    sets = _fit(p["sets"], block)
    if len(sets) < len(p["sets"]):
        with pytest.raises(ValueError, match="more than one device block of %d" % block):
            tester(p["G"], p["sets"])
    ref = _oracle(p, c, sets)
    for k in PLANTED:
        if p["sets"][k].size <= block:
            i = [j for j, s in enumerate(sets) if s is p["sets"][k]][0]
            print("reference skat_p of planted set", k, ref["skat_p"][i])
            assert 1e-12 < ref["skat_p"][i] < 0.1
    out = tester(p["G"], sets, return_kernel=True)
    assert sorted(out) == sorted(KEYS + ("kernel",)) and all(out[k].shape == (len(sets),) for k in KEYS)
    _compare(out, ref, p["n"])
    k2 = [j for j, s in enumerate(sets) if s is p["sets"][2]]
    if k2:
        assert out["n_used"][k2[0]] == 16 - 2     # the monomorphic and the all-missing marker are dropped from their set
    assert out["n_used"][-1] == 0                 # ... and leave nothing of the set that holds only them


def test_unit_weights_given_weights_liu_and_no_sets():
    p = _problem("spd300")
    tester, sets = _tester(p, 4, 128), p["sets"]
    ref = _oracle(p, 4, sets, weights=None, method="liu")
    out = tester(p["G"], sets, weights=None, method="liu", return_kernel=True)
    _compare(out, ref, p["n"], method="liu")
    beta = tester(p["G"], sets, return_kernel=True)
    given = []
    for s, (_, _, w) in zip(sets, beta["kernel"]):      # the beta weights handed back in, padded where markers were dropped
        full = np.ones(s.size)
        n_obs, _, Gt = _centred(p["G"][s])
        full[(n_obs > 0) & Gt.any(axis=1)] = w
        given.append(full)
    again = tester(p["G"], sets, weights=given)
    for k in KEYS:
        assert np.array_equal(again[k], beta[k], equal_nan=True), k
    assert "kernel" not in again
    empty = tester(p["G"], [])
    assert sorted(empty) == sorted(KEYS) and all(v.shape == (0,) for v in empty.values())


def _block(tester, G, torch, gram, sentinel=-7.25):
    """One block through scilmm_scan_block_gram_dev (or the plain entry point): (statistics, the whole r_max^2 Gram buffer)."""
    r, n, q = G.shape[0], G.shape[1], tester.q
    ld = (n + 15) // 16 * 16
    dG = torch.zeros((r, ld), dtype=torch.int8, device="cuda")
    dG[:, :n].copy_(torch.from_numpy(G))
    dS = torch.zeros(((q + 4) * r,), dtype=torch.float64, device="cuda")
    dK = torch.full((r * r + 64,), sentinel, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    vp = C.c_void_p
    if gram:
        tester.factor.scan_block_gram_dev(vp(dG.data_ptr()), ld, r, vp(tester.dQ.data_ptr()), q, vp(dS.data_ptr()), vp(dK.data_ptr()))
    else:
        tester.factor.scan_block_dev(vp(dG.data_ptr()), ld, r, vp(tester.dQ.data_ptr()), q, vp(dS.data_ptr()))
    tester.sym.sync()
    return dS.cpu().numpy().reshape(q + 4, r), dK.cpu().numpy()


@pytest.mark.parametrize("name", ["pedigree", "spd203"])
def test_gram_block_at_the_c_level(name):
    import torch
    p = _problem(name)
    tester = _tester(p, 4, 128, deterministic=True)
    G19 = np.ascontiguousarray(np.vstack([p["G"][:4], p["G"][40:55]]))
    _, _, Gt = _centred(G19)
    X = tester.factor.solve_L(tester.factor.apply_P(np.ascontiguousarray(Gt.T)))       # n x 19, permuted rows
    XtX = X.T @ X
    for r in (1, 17, 19):
        # r = 1: the all-zero monomorphic marker alone is useless, take a polymorphic one
        rows = [FULL] if r == 1 else list(range(r))
        S, K = _block(tester, np.ascontiguousarray(G19[rows]), torch, True)
        S0, K0 = _block(tester, np.ascontiguousarray(G19[rows]), torch, False)
        assert np.array_equal(S, S0, equal_nan=True), r                  # the statistics: the bits of the plain entry point
        assert np.all(K0 == -7.25) and np.all(K[r * r:] == -7.25) and not np.any(K[:r * r] == -7.25), r   # exactly r * r written
        K = K[:r * r].reshape(r, r)
        assert np.array_equal(K, K.T), r                                 # symmetric bit for bit
        gg = S[3]
        print(name, r, "diag vs gg", rel_err(np.diag(K), gg), "vs solve_L", rel_err(K, XtX[np.ix_(rows, rows)]))
        assert rel_err(np.diag(K), gg) < 1e-12, r
        assert rel_err(K, XtX[np.ix_(rows, rows)]) < TOL, r


def _block_bed(tester, packed, N, idx, r, torch):
    q, nb = tester.q, packed.shape[1]
    dB = torch.from_numpy(np.ascontiguousarray(packed[:r])).cuda()
    dI = None if idx is None else torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).cuda()
    dS = torch.zeros(((q + 4) * r,), dtype=torch.float64, device="cuda")
    dK = torch.zeros((r * r,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    vp = C.c_void_p
    tester.factor.scan_block_bed_gram_dev(vp(dB.data_ptr()), nb, N, None if dI is None else vp(dI.data_ptr()), 0, r,
                                          vp(tester.dQ.data_ptr()), q, vp(dS.data_ptr()), vp(dK.data_ptr()))
    tester.sym.sync()
    return dS.cpu().numpy().reshape(q + 4, r), dK.cpu().numpy()


def test_bed_block_gives_the_bits_of_the_int8_block(tmp_path):
    """scilmm_scan_block_bed_gram_dev with the identity map and with a map that reorders the individuals and drops some."""
    import torch
    p = _problem("spd203")
    n = p["n"]
    tester = _tester(p, 4, 128, deterministic=True)
    G19 = np.ascontiguousarray(p["G"][:19])
    S, K = _block_bed(tester, T.pack(G19), n, None, 19, torch)
    S0, K0 = _block(tester, G19, torch, True)
    assert np.array_equal(S, S0, equal_nan=True) and np.array_equal(K, K0[:19 * 19])
    N = n + 38
    rng = np.random.default_rng(3)
    Gf = _markers(N, 19, 21)
    idx = rng.permutation(N)[:n].astype(np.int32)
    idx[rng.choice(n, size=n // 20, replace=False)] = -1
    Gc = np.ascontiguousarray(np.where(idx >= 0, Gf[:, np.maximum(idx, 0)], -1).astype(np.int8))
    S, K = _block_bed(tester, T.pack(Gf), N, idx, 19, torch)
    S0, K0 = _block(tester, Gc, torch, True)
    assert np.array_equal(S, S0, equal_nan=True) and np.array_equal(K, K0[:19 * 19])
    assert np.array_equal(S[0], (Gc >= 0).sum(axis=1))


def test_test_bed_gives_the_bits_of_call_on_the_unpacked_markers(tmp_path):
    from scilmm_amd.bed import BedFile
    p = _problem("spd203")
    n = p["n"]
    tester, sets = _tester(p, 4, 128, deterministic=True), p["sets"]
    path = T.write_fileset(tmp_path / "id", T.pack(p["G"]), n)
    a = tester.test_bed(path, sets, return_kernel=True)
    b = tester(BedFile(path).read(), sets, return_kernel=True)
    c = tester(p["G"], sets, return_kernel=True)
    N = n + 37
    Gf = _markers(N, M, 9)
    rng = np.random.default_rng(4)
    idx = rng.permutation(N)[:n].astype(np.int32)
    idx[rng.choice(n, size=n // 20, replace=False)] = -1
    bed = BedFile(T.write_fileset(tmp_path / "map", T.pack(Gf), N))
    d = tester.test_bed(bed, sets, sample_index=idx, count="A2", weights=None, method="liu", return_kernel=True)
    e = tester(bed.read(None, idx, "A2"), sets, weights=None, method="liu", return_kernel=True)
    for x, y in ((a, b), (a, c), (d, e)):
        for k in KEYS:
            assert x[k].dtype == y[k].dtype and np.array_equal(x[k], y[k], equal_nan=True), k
        for (s, K, w), (s0, K0, w0) in zip(x["kernel"], y["kernel"]):
            assert np.array_equal(s, s0) and np.array_equal(K, K0) and np.array_equal(w, w0)


def test_deterministic_mode_repeats_its_bits_and_adds_no_atomics():
    from scilmm_amd import AssociationScan, SparseCholesky
    p = _problem("pedigree")
    sets = _fit(p["sets"], 112)
    tester = _tester(p, 4, 112, deterministic=True)
    a, b = tester(p["G"], sets, return_kernel=True), tester(p["G"], sets, return_kernel=True)
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    for (s, K, w), (s0, K0, w0) in zip(a["kernel"], b["kernel"]):
        assert np.array_equal(s, s0) and np.array_equal(K, K0) and np.array_equal(w, w0)
    assert tester.sym.timing()["n_float_atomic_launches"] == 0
    _compare(a, _oracle(p, 4, sets), p["n"])
    # default mode: the counter grows by what the same blocks of the plain scan add -- the Gram adds nothing
    from scilmm_amd.sets import pack_sets
    free = _tester(p, 4, 112)
    n0 = free.sym.timing()["n_float_atomic_launches"]
    free(p["G"], sets)
    n1 = free.sym.timing()["n_float_atomic_launches"]
    scan = AssociationScan(SparseCholesky(), [p["A"], p["I"]], S2, p["C"], p["y"], block=112)
    m0 = scan.sym.timing()["n_float_atomic_launches"]
    for members in pack_sets([s.size for s in sets], 112):
        rows = np.concatenate([sets[i] for i in members])
        assert rows.size <= 112
        scan(np.ascontiguousarray(p["G"][rows]))           # one plain block of the same width
    m1 = scan.sym.timing()["n_float_atomic_launches"]
    print("float-atomic launches: sets", n1 - n0, "plain scan", m1 - m0)
    assert n1 - n0 == m1 - m0


def test_refusals():
    from scilmm_amd import ScilmmError, SparseCholesky, VariantSetTest, _lib
    p = _problem("spd300")
    n = p["n"]
    chol = SparseCholesky()
    tester = VariantSetTest(chol, [p["A"], p["I"]], S2, p["C"][:, :1], p["y"], block=16)
    L, one, h = _lib.lib(), C.c_void_p(8), tester.factor._h
    f, g = L.scilmm_scan_block_gram_dev, L.scilmm_scan_block_bed_gram_dev
    nb = (n + 3) // 4
    assert f(h, one, n, 4, one, 2, one, None) == _lib.ERR_ARG                       # a null d_gram
    assert g(h, one, nb, n, None, 0, 4, one, 2, one, None) == _lib.ERR_ARG
    for r, q in ((0, 2), (129, 2), (4, 0), (4, 33)):                                  # the r / q bounds of the scan block
        assert f(h, one, n, r, one, q, one, one) == _lib.ERR_ARG
        assert g(h, one, nb, n, None, 0, r, one, q, one, one) == _lib.ERR_ARG
    assert f(h, one, n - 1, 4, one, 2, one, one) == _lib.ERR_ARG                    # pitch shorter than a row
    assert g(h, one, nb - 1, n, None, 0, 4, one, 2, one, one) == _lib.ERR_ARG
    assert g(h, one, nb, n, None, 2, 4, one, 2, one, one) == _lib.ERR_ARG           # an unknown flag bit
    assert g(h, one, nb + 1, n + 1, None, 0, 4, one, 2, one, one) == _lib.ERR_ARG   # identity map with N != n
    sets = _fit(p["sets"], 16)
    tester(p["G"], sets)
    other = VariantSetTest(chol, [p["A"], p["I"]], [0.7, 0.3], p["C"][:, :1], p["y"], block=16)
    assert other.factor is tester.factor
    with pytest.raises(ScilmmError, match="sigma2"):
        tester(p["G"], sets)                                # the first object's whitening belongs to the old factor
    other(p["G"], sets)
    other.factor.inverse_traces()                           # consumes the factor
    with pytest.raises(ScilmmError):
        other(p["G"], sets)
