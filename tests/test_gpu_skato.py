"""scilmm_sets_finish_dev and VariantSetTest(..., skato=True, finish="device") against the host finish of the same inputs
(scilmm_amd.sets: LAPACK eigenvalues, SciPy tails, adaptive quadrature), and the host against tests/skato_oracle.py.

Tolerances: the eigenvalues within 1e-9 of the largest one of LAPACK's; the burden numbers and skat_q 1e-9 relative (what the
suite holds derived statistics to); every p-value (skat_p, skato_p, skato_pmin, skato_p_rho) 1e-6 relative, the tolerance
tests/test_gpu_sets.py holds p-values to; skato_rho and n_used exact; exactly the documented doubles written.

At the C level the statistics and the Gram matrix are made up, so that the spectrum of every set is chosen: random positive
semidefinite matrices at the sizes 1, 2, 3, 16, 17, 63, 64, 65, 127, 128 (both parities of the round-robin pairing, every LDS
size up to the largest), rank 3 of 17, the identity (every pole of the secular equations equal: full deflation), a matrix with
1 an exact eigenvector (zero weights in the secular equations), rank one and 1'A1 = 0 (the degenerate rule), a set whose Q_0 is
the mean of its null law (inside the saddlepoint seam), a set with T < 1e-30, and a set with dropped markers at its first, a
middle and its last column.

Worst deviations measured on an MI355X when this was written (printed by the tests with -s): at the C level, device finish
against host finish, eigenvalues 3.2e-14 of the largest, burden numbers and skat_q 1.7e-15, p-values 6.5e-12 (the 1'A1 = 0 set;
2.5e-12 at 128 markers), T down to 3.8e-39; end to end 1.3e-12; the host against the Z1 oracle 1.5e-12."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg
import scipy.stats as stats

from tests import skato_oracle as O
from tests import test_bed_api as T
from tests import test_gpu_sets as GS
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

PTOL, TOL = 1e-6, 1e-9
HEAD = 10
SENT = -7.25
RHO = np.array([0.0, 0.01, 0.04, 0.09, 0.16, 0.25, 0.5, 1.0])
CC = 4                        # covariates of the made-up blocks
vp = C.c_void_p


def _psd(rng, k, rank=None):
    Z = rng.standard_normal((rank or k + 8, k)) * rng.uniform(0.3, 1.7, k)
    return Z.T @ Z


def _ones_eigvec(rng, k):
    Q, _ = np.linalg.qr(np.hstack([np.ones((k, 1)), rng.standard_normal((k, k - 1))]))
    A = (Q * rng.uniform(0.2, 3.0, k)) @ Q.T
    return 0.5 * (A + A.T)


def _no_ones(rng, k):
    """A graph Laplacian with small integer weights: positive semidefinite, and K 1 = 0 in floating point as well."""
    Wt = np.triu(rng.integers(1, 4, (k, k)).astype(np.float64), 1)
    Wt = Wt + Wt.T
    return np.diag(Wt.sum(axis=1)) - Wt


def _made_up_sets():
    """(name, K, s, exact, dropped): the covariance and the score of the kept markers; `exact`: the covariates' rows are zero for
    this set, so that K reaches the kernel bit for bit; `dropped`: positions (in the set) of markers without variation."""
    rng = np.random.default_rng(2012)
    out = []

    def null_t(K):
        ev, U = np.linalg.eigh(K)
        return (U * np.sqrt(np.maximum(ev, 0.0))) @ rng.standard_normal(K.shape[0])

    for k in (1, 2, 3, 16, 17, 63, 64, 65, 127, 128):
        K = _psd(rng, k)
        out.append(("psd%d" % k, K, null_t(K) * (1.0 + (k % 3)), False, ()))
    K = _psd(rng, 17, rank=3)
    out.append(("rank3of17", K, 1.5 * null_t(K), False, ()))
    out.append(("identity16", np.eye(16), 1.4 * rng.standard_normal(16), True, ()))
    K = _ones_eigvec(rng, 5)
    out.append(("ones_eigvec5", K, 1.3 * null_t(K), True, ()))
    K = _ones_eigvec(rng, 64)
    out.append(("ones_eigvec64", K, 1.2 * null_t(K), True, ()))
    b = rng.standard_normal(9)
    out.append(("rank_one9", np.outer(b, b), 2.1 * b, True, ()))
    K = _no_ones(rng, 8)
    # (integers: 1't and 1'K1 are exactly 0 on both sides, so the burden numbers are the same 0 / 0 and 1 / 0 on both)
    out.append(("s11_zero8", K, K @ rng.integers(-3, 4, 8).astype(np.float64), True, ()))
    K = _psd(rng, 12)
    t = null_t(K)
    out.append(("seam12", K, t * np.sqrt(np.trace(K) / (t @ t)), True, ()))          # Q_0 = t't = the mean of its null law
    K = _psd(rng, 17)
    out.append(("tiny17", K, null_t(K) + 6.0 * np.sqrt(np.diag(K)) * rng.choice([-1.0, 1.0], 17), False, ()))
    K = _psd(rng, 9)
    out.append(("dropped12", K, 1.7 * null_t(K), False, (0, 5, 11)))
    # two markers with a signal: df = 1 and some thirty pieces of the integral (test_a_set_gives_the_same_bits_...)
    rng = np.random.default_rng([77, 0])
    Z = rng.standard_normal((12, 2)) * rng.uniform(0.3, 1.7, 2)
    K = Z.T @ Z
    out.append(("kinks2", K, null_t(K) + 3.0 * np.sqrt(np.diag(K)) * rng.choice([-1.0, 1.0], 2), True, ()))
    return out


def _pieces(t, A):
    """The pieces of positive length of the SKAT-O integral of (t, A), from the host module's own parts."""
    from scilmm_amd import sets as mod
    rho, r = np.minimum(RHO, 0.999), t.size
    lams, p_rho = [], []
    for x in rho:
        L = np.linalg.cholesky((1 - x) * np.eye(r) + x * np.ones((r, r)))
        lams.append(mod._floor(scipy.linalg.eigvalsh(L.T @ A @ L)))
        p_rho.append(mod.mixture_sf_saddlepoint((1 - x) * (t @ t) + x * t.sum() ** 2, lams[-1]))
    a = A.sum(axis=1)
    s11 = a.sum()
    B = A - np.outer(a, a) / s11
    lamB = mod._floor(scipy.linalg.eigvalsh(B), 1e-10 * np.trace(A))
    l2 = np.sum(lamB ** 2)
    mu, sd, df = lamB.sum(), np.sqrt(2 * l2 + 4 * max(a @ B @ a, 0.0) / s11), l2 * l2 / np.sum(lamB ** 4)
    al, be = mod.skato_lines(min(p_rho), lams, rho, rho * s11 + (1 - rho) * (a @ a) / s11)
    return mod.skato_breaks(al, be, mu - sd * np.sqrt(0.5 * df))[1].size - 1


def _made_up_block(members, rng, R, u):
    """The (c + 5) x r statistics and the r x r Gram matrix of a block that holds the made-up sets `members` one after the other:
    with z = R^-T W the kernel finds K = G - z'z and s = S[4 + c] - u'z as they were chosen."""
    sizes = [m[1].shape[0] + len(m[4]) for m in members]
    r, c = sum(sizes), R.shape[0]
    S, G = np.zeros((c + 5, r)), 0.1 * rng.standard_normal((r, r))
    G = G + G.T                                             # (what lies between two sets is never read: anything)
    S[0], S[1], S[2] = 203.0, rng.uniform(0.01, 0.1, r), 1.0
    W = 0.3 * rng.standard_normal((c, r))
    start, a = [0], 0
    for (name, K, s, exact, dropped), size in zip(members, sizes):
        keep = np.array([j not in dropped for j in range(size)])
        cols = a + np.flatnonzero(keep)
        if exact:
            W[:, a:a + size] = 0.0
        z = scipy.linalg.solve_triangular(R, W[:, cols], trans="T", lower=False)
        G[np.ix_(cols, cols)] = K + z.T @ z
        S[4 + c, cols] = s + u @ z
        for j in np.flatnonzero(~keep):                     # no variation, or nothing observed
            S[2 if j % 2 else 0, a + j] = 0.0
        a += size
        start.append(a)
    S[3] = np.diag(G)
    S[4:4 + c] = W
    return S, 0.5 * (G + G.T), np.array(start, dtype=np.int32)


def _finish(fac, sym, torch, S, G, R, u, start, mode=1, weights=None, method=0, rho=RHO, lam=True):
    """One call of scilmm_sets_finish_dev on sentinel-filled buffers: (rows, lam); exactly the documented doubles are written."""
    q, r = S.shape[0] - 4, S.shape[1]
    ns, ld = start.size - 1, HEAD + len(rho) + 3
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    dS, dG, dR, du = dev(S), dev(G), dev(R), dev(u)
    dW = dev(weights) if weights is not None else None
    dO = torch.full((ns * ld + 5,), SENT, dtype=torch.float64, device="cuda")
    dL = torch.full((r + 5,), SENT, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    fac.sets_finish_dev(r, q, vp(dS.data_ptr()), vp(dG.data_ptr()), vp(dR.data_ptr()), vp(du.data_ptr()), q - 1, ns, start, mode,
                        vp(dW.data_ptr()) if dW is not None else None, method, rho, vp(dO.data_ptr()), ld, vp(dL.data_ptr()) if lam else None)
    sym.sync()
    O_, L_ = dO.cpu().numpy(), dL.cpu().numpy()
    rows = O_[:ns * ld].reshape(ns, ld)
    used = HEAD + len(rho)
    assert np.all(O_[ns * ld:] == SENT) and np.all(rows[:, used:] == SENT) and not np.any(rows[:, :used] == SENT)
    assert np.all(L_[r:] == SENT) and (not lam or not np.any(L_[:start[-1]] == SENT)) and (lam or np.all(L_ == SENT))
    return rows[:, :used], L_[:r]


def _host_rows(S, G, R, u, start, weights, method, rho):
    """The host finish of the same inputs, in the layout of the device's rows, and the eigenvalues in the layout of d_lam."""
    from scilmm_amd import sets as mod
    sf = mod.check_method(method)
    rows, lam_all = np.full((start.size - 1, HEAD + len(rho)), np.nan), np.full(S.shape[1], np.nan)
    for i in range(start.size - 1):
        a, b = start[i], start[i + 1]
        w_in = weights if weights is None or isinstance(weights, str) else weights[a:b]
        s, K, w, keep = mod.set_kernel(S[:, a:b], G[a:b, a:b], R, u, w_in)
        rows[i, 0], rows[i, 9] = keep.sum(), 0.0
        if not keep.any():
            continue
        ws, wKw = w @ s, w @ K @ w
        A = w[:, None] * K * w[None, :]
        lam = scipy.linalg.eigvalsh(A)
        lam_all[a + np.flatnonzero(keep)] = lam[::-1]
        with np.errstate(divide="ignore", invalid="ignore"):
            rows[i, 1:5] = ws / wKw, 1.0 / np.sqrt(wKw), ws * ws / wKw, np.sum(w * w * s * s)
        rows[i, 5] = sf(rows[i, 4], lam[lam > mod.LAMBDA_FLOOR * lam.max()])
        if len(rho):
            p, pmin, r0, p_rho = mod.skato_pvalue(w * s, A, rho, method)
            rows[i, 6:9], rows[i, HEAD:] = (p, pmin, r0), p_rho
    return rows, lam_all


def _compare_rows(dev, host, lam_d, lam_h, what, worst):
    assert np.array_equal(dev[:, 0], host[:, 0]), what                       # n_used
    live = host[:, 0] > 0
    assert np.all(np.isnan(dev[~live, 1:9])) and np.all(dev[~live, 9] == 0), what
    d, h = dev[live], host[live]
    for col, name in ((1, "burden_beta"), (2, "burden_se"), (3, "burden_chi2"), (4, "skat_q")):
        fin = np.isfinite(h[:, col])                        # (w'Kw = 0 exactly: the same NaN or infinity on both sides)
        assert np.array_equal(d[~fin, col], h[~fin, col], equal_nan=True), (what, name)
        e = float(np.max(np.abs(d[fin, col] - h[fin, col]) / np.abs(h[fin, col])))
        worst[name] = max(worst.get(name, 0.0), e)
        assert e < TOL, (what, name, e)
    cols = [5] + ([6, 7] + list(range(HEAD, dev.shape[1])) if dev.shape[1] > HEAD else [])
    e = np.abs(d[:, cols] - h[:, cols]) / np.abs(h[:, cols])
    print(what, "p-values: worst rel. deviation per set", np.max(e, axis=1))
    worst["p"] = max(worst.get("p", 0.0), float(e.max()))
    assert not np.any(np.isnan(d[:, cols])) and e.max() < PTOL, (what, e.max())
    if dev.shape[1] > HEAD:
        assert np.array_equal(d[:, 8], h[:, 8]), (what, d[:, 8], h[:, 8])    # skato_rho
        assert np.all(d[:, 6] <= (dev.shape[1] - HEAD) * d[:, 7])
    else:
        assert np.all(np.isnan(d[:, 6:9]))
    assert not np.any(d[:, 9].astype(int) & 6), (what, d[:, 9])              # no iteration ran out of steps
    if lam_d is not None:
        assert np.array_equal(np.isnan(lam_d), np.isnan(lam_h)), what
        ok = ~np.isnan(lam_h)
        e = float(np.max(np.abs(lam_d[ok] - lam_h[ok])) / np.max(lam_h[ok]))
        worst["lam"] = max(worst.get("lam", 0.0), e)
        assert e < TOL, (what, e)


_STATE = {}


def _c_level():
    """The factor handle and the made-up blocks with their host finish, built once."""
    if not _STATE:
        from scilmm_amd.sets import pack_sets
        p = GS._problem("spd203")
        assert p["n"] == 203
        tester = GS._tester(p, 4, 128, deterministic=True)
        rng = np.random.default_rng(7)
        R = np.triu(0.2 * rng.standard_normal((CC, CC))) + np.diag(rng.uniform(1.0, 2.0, CC))
        u = 0.5 * rng.standard_normal(CC)
        made = _made_up_sets()
        blocks = []
        for members in pack_sets([m[1].shape[0] + len(m[4]) for m in made], 128):
            mem = [made[i] for i in members]
            S, G, start = _made_up_block(mem, rng, R, u)
            blocks.append(dict(names=[m[0] for m in mem], S=S, G=G, start=start, host=_host_rows(S, G, R, u, start, None, "saddlepoint", RHO)))
        _STATE.update(tester=tester, R=R, u=u, made={m[0]: m for m in made}, blocks=blocks)
    return _STATE


def test_the_made_up_sets_are_what_they_claim():
    """Conditions on the tests' inputs, from the oracle alone."""
    st = _c_level()
    _, K, s, _, _ = st["made"]["seam12"]
    ref = O.skato(O.z1_from_gram(K), s)
    assert ref["seam"][0] and not ref["degenerate"]
    _, K, s, _, _ = st["made"]["tiny17"]
    ref = O.skato(O.z1_from_gram(K), s)
    print("tiny17: T", ref["pmin"], "p", ref["p"])
    assert 0 < ref["pmin"] < 1e-30 and not ref["degenerate"]
    for name in ("rank_one9", "s11_zero8"):
        _, K, s, _, _ = st["made"][name]
        assert O.skato(O.z1_from_gram(K), s)["degenerate"], name
    _, K, s, _, _ = st["made"]["rank3of17"]
    assert np.linalg.matrix_rank(K) == 3
    _, K, _, _, _ = st["made"]["ones_eigvec64"]
    assert np.max(np.abs(K @ np.ones(64) - (np.ones(64) @ K @ np.ones(64) / 64) * np.ones(64))) < 1e-12 * np.trace(K)


def test_finish_at_the_c_level_matches_the_host_finish():
    import torch
    st = _c_level()
    fac, sym = st["tester"].factor, st["tester"].sym
    worst = {}
    for b in st["blocks"]:
        rows, lam = _finish(fac, sym, torch, b["S"], b["G"], st["R"], st["u"], b["start"])
        _compare_rows(rows, b["host"][0], lam, b["host"][1], "+".join(b["names"]), worst)
        flags = dict(zip(b["names"], rows[:, 9].astype(int)))
        for name, f in flags.items():
            deg = name in ("psd1", "rank_one9", "s11_zero8")
            assert f & 8 and bool(f & 1) == deg, (name, f)
    print("worst deviations, device finish against host finish:", worst)
    # the other tail, the other weight modes, no SKAT-O, no d_lam: on the first block (sizes 1 .. 63 and a full mix)
    b = st["blocks"][0]
    S, G, start = b["S"], b["G"], b["start"]
    w = np.random.default_rng(3).uniform(0.5, 2.0, S.shape[1])
    for what, kw, hw, hm in (("liu", dict(method=1), None, "liu"), ("given weights", dict(mode=2, weights=w), w, "saddlepoint"),
                             ("beta weights", dict(mode=0), "beta", "saddlepoint")):
        rows, lam = _finish(fac, sym, torch, S, G, st["R"], st["u"], start, **kw)
        host = _host_rows(S, G, st["R"], st["u"], start, hw, hm, RHO)
        _compare_rows(rows, host[0], lam, host[1], what, worst)
    # a Q so small that every Liu tail is exactly 1: T = 1, the quantiles are 0, and no root runs out of steps
    rng = np.random.default_rng(4)
    K5 = _psd(rng, 5)
    S1, G1, start1 = _made_up_block([("small_q5", K5, 1e-3 * np.ones(5), True, ())], rng, st["R"], st["u"])
    rows, lam = _finish(fac, sym, torch, S1, G1, st["R"], st["u"], start1, method=1)
    host = _host_rows(S1, G1, st["R"], st["u"], start1, None, "liu", RHO)
    assert host[0][0, 7] == 1.0 and rows[0, 7] == 1.0
    _compare_rows(rows, host[0], lam, host[1], "every Liu tail 1", worst)
    rows, _ = _finish(fac, sym, torch, S, G, st["R"], st["u"], start, rho=np.empty(0), lam=False)
    _compare_rows(rows, b["host"][0][:, :HEAD], None, None, "no SKAT-O", worst)
    grid = np.array([0.0, 0.3, 1.0])
    rows, _ = _finish(fac, sym, torch, S, G, st["R"], st["u"], start, rho=grid)
    _compare_rows(rows, _host_rows(S, G, st["R"], st["u"], start, None, "saddlepoint", grid)[0], None, None, "three grid values", worst)


def test_a_set_gives_the_same_bits_wherever_it_lies():
    import torch
    st = _c_level()
    tester = st["tester"]
    fac, sym, made = tester.factor, tester.sym, st["made"]
    n0 = sym.timing()["n_float_atomic_launches"]
    # kinks2: more pieces of the integral than a workgroup of 256 threads has groups of 32 lanes, so the order of its sum would
    # show if it depended on the number of threads -- which the block's largest set decides: 256 alone, 512 next to a wide set
    assert _pieces(made["kinks2"][2], made["kinks2"][1]) > 8
    for which in ("tiny17", "kinks2"):
        x = made[which]
        k = x[1].shape[0]
        rng = np.random.default_rng(11)
        filler = lambda k: ("f%d" % k, _psd(rng, k), rng.standard_normal(k), False, ())
        layouts = {"alone": ([x], 0), "last in a full block": ([filler(128 - k), x], 1), "between two": ([filler(5), x, filler(70)], 1)}
        got = {}
        for name, (members, at) in layouts.items():
            S, G, start = _made_up_block(members, np.random.default_rng(1), st["R"], st["u"])
            if name == "last in a full block":
                assert start[-1] == 128
            # the set's own numbers must be the same bits in every layout: write them in from the first one
            a, b_ = start[at], start[at + 1]
            if "ref" not in got:
                got["ref"] = (S[:, a:b_].copy(), G[a:b_, a:b_].copy())
            S[:, a:b_], G[a:b_, a:b_] = got["ref"]
            rows, lam = _finish(fac, sym, torch, S, G, st["R"], st["u"], start)
            again, lam2 = _finish(fac, sym, torch, S, G, st["R"], st["u"], start)
            assert np.array_equal(rows, again, equal_nan=True) and np.array_equal(lam, lam2, equal_nan=True), name    # two runs
            got[name] = (rows[at], lam[a:b_])
            assert not int(rows[at][9]) & 1, (which, name)                  # the integral was taken
        for name in ("last in a full block", "between two"):
            assert np.array_equal(got[name][0], got["alone"][0]) and np.array_equal(got[name][1], got["alone"][1]), (which, name)
    assert sym.timing()["n_float_atomic_launches"] == n0


def _host_and_device(name, c, block):
    p = GS._problem(name)
    key = ("skato", c, block)
    if key not in p["ref"]:
        tester = GS._tester(p, c, block, deterministic=True)
        sets = GS._fit(p["sets"], block)
        p["ref"][key] = (tester, sets, tester(p["G"], sets, skato=True), tester(p["G"], sets, skato=True, finish="device"))
    return p["ref"][key]


def _compare_dicts(dev, host, what):
    from scilmm_amd.sets import KEYS, SKATO_KEYS
    assert sorted(dev) == sorted(host) == sorted(KEYS + SKATO_KEYS), what
    assert dev["n_used"].dtype == host["n_used"].dtype and np.array_equal(dev["n_used"], host["n_used"])
    live = host["n_used"] > 0
    for k in KEYS[1:] + SKATO_KEYS:
        assert dev[k].shape == host[k].shape and np.all(np.isnan(dev[k][~live])) and not np.any(np.isnan(dev[k][live])), (what, k)
    for k in ("burden_beta", "burden_se", "burden_chi2", "skat_q"):
        assert rel_err(dev[k][live], host[k][live]) < TOL, (what, k)
    worst = 0.0
    for k in ("burden_p", "skat_p", "skato_p", "skato_pmin", "skato_p_rho"):
        e = float(np.max(np.abs(dev[k][live] - host[k][live]) / np.abs(host[k][live])))
        worst = max(worst, e)
        assert e < PTOL, (what, k, e)
    assert np.array_equal(dev["skato_rho"][live], host["skato_rho"][live]), what
    print(what, "worst rel. deviation of a p-value", worst)


@pytest.mark.parametrize("block", [16, 128])
@pytest.mark.parametrize("c", [1, 4])
@pytest.mark.parametrize("name", ["spd203", "pedigree"])
def test_device_finish_matches_host_finish_end_to_end(name, c, block):
    tester, sets, host, dev = _host_and_device(name, c, block)
    _compare_dicts(dev, host, "%s c=%d block=%d" % (name, c, block))
    p = GS._problem(name)
    plain = tester(p["G"], sets)
    assert sorted(plain) == sorted(GS.KEYS)                                  # the defaults: the old keys ...
    for k in GS.KEYS:
        assert np.array_equal(plain[k], host[k], equal_nan=True), k          # ... and skato=True leaves their bits alone
    small = tester(p["G"], sets, finish="device")                            # burden and SKAT only
    assert sorted(small) == sorted(GS.KEYS)
    for k in GS.KEYS:
        assert np.array_equal(small[k], dev[k], equal_nan=True), k


@pytest.mark.parametrize("c", [1, 4])
def test_host_skato_matches_the_z1_oracle(c):
    """spd203 (n = 203): Z1 = P^1/2 G~' diag(w) from the dense inv(V) and the explicit P, then the package's formulas."""
    tester, sets, host, _ = _host_and_device("spd203", c, 128)
    p = GS._problem("spd203")
    ref = GS._oracle(p, c, sets)
    Vi = np.linalg.inv((GS.S2[0] * p["A"] + GS.S2[1] * p["I"]).toarray())
    n_obs, mean, Gt = GS._centred(p["G"])
    worst = 0.0
    for i, rows in enumerate(sets):
        rows = np.array([j for j in rows if n_obs[j] > 0 and Gt[j].any()], dtype=np.int64)
        if not rows.size:
            assert np.isnan(host["skato_p"][i])
            continue
        s, K, w = ref["kernel"][i]
        Z1, _ = O.z1_from_model(Vi, p["C"][:, :c], Gt[rows], w)
        assert rel_err(Z1.T @ Z1, w[:, None] * K * w[None, :]) < 1e-9
        o = O.skato(Z1, w * s)
        got = np.r_[host["skato_p"][i], host["skato_pmin"][i], host["skato_p_rho"][i]]
        want = np.r_[o["p"], o["pmin"], o["p_rho"]]
        e = float(np.max(np.abs(got - want) / want))
        worst = max(worst, e)
        assert e < PTOL and host["skato_rho"][i] == o["rho"], (i, e)
    print("host against the Z1 oracle, worst rel. deviation", worst)


def test_bed_and_dosages_give_the_bits_of_the_int8_call(tmp_path):
    p = GS._problem("spd203")
    tester, sets, _, dev = _host_and_device("spd203", 4, 128)
    from scilmm_amd.sets import KEYS, SKATO_KEYS
    path = T.write_fileset(tmp_path / "id", T.pack(p["G"]), p["n"])
    bed = tester.test_bed(path, sets, skato=True, finish="device")
    codes = np.where(p["G"] >= 0, p["G"].astype(np.int64) * 16384, 65535).astype(np.uint16)
    dos = tester.test_dosages(codes, sets, skato=True, finish="device")
    for other in (bed, dos):
        for k in KEYS + SKATO_KEYS:
            assert np.array_equal(other[k], dev[k], equal_nan=True), k


def test_argument_errors_and_refusals(monkeypatch):
    import torch
    from scilmm_amd import ScilmmError, _lib
    from scilmm_amd.factor import Symbolic
    st = _c_level()
    tester = st["tester"]
    fac, sym = tester.factor, tester.sym
    L, h, one = _lib.lib(), fac._h, vp(8)
    start, rho = np.array([0, 2, 5], dtype=np.int32), np.array([0.0, 0.5, 1.0])
    good = dict(fac=h, r=5, q=3, stats=one, gram=one, R=one, u=one, c=2, n_sets=2, start=_lib.ptr(start), mode=0, w=None, method=0,
                rho=_lib.ptr(rho), n_rho=3, out=one, ld=13, lam=None)
    bad_start = [np.array(v, dtype=np.int32) for v in ([1, 2, 5], [0, 2, 6], [0, 2, 2], [0, 3, 2])]
    bad_rho = [np.array(v) for v in ([0.0, 1.5, 1.0], [0.0, -0.1, 1.0], [0.0, np.nan, 1.0])]
    cases = [dict(fac=None), dict(stats=None), dict(gram=None), dict(R=None), dict(u=None), dict(start=None), dict(out=None),
             dict(rho=None), dict(r=0), dict(r=129), dict(c=0, q=1), dict(c=32, q=33), dict(q=4), dict(n_sets=0), dict(n_sets=6),
             dict(n_rho=-1), dict(n_rho=17), dict(ld=12), dict(mode=3), dict(mode=2, w=None), dict(method=2)]
    cases += [dict(start=_lib.ptr(v)) for v in bad_start] + [dict(rho=_lib.ptr(v)) for v in bad_rho]
    for kw in cases:
        a = dict(good, **kw)
        assert L.scilmm_sets_finish_dev(*[a[k] for k in good]) == _lib.ERR_ARG, kw
    # the handle is as usable as before
    b = st["blocks"][0]
    rows, _ = _finish(fac, sym, torch, b["S"], b["G"], st["R"], st["u"], b["start"])
    _compare_rows(rows, b["host"][0], None, None, "after the argument errors", {})
    p = GS._problem("spd203")
    with pytest.raises(ValueError, match="return_kernel"):
        tester(p["G"], p["sets"], finish="device", return_kernel=True)
    # fp32-product fronts: refused as a scan block is, the handle left as it was
    from tests.test_gpu_halfsolve import _pedigree
    monkeypatch.setenv("SCILMM_TUNING", "1")
    monkeypatch.setenv("SCILMM_DENSE", "1")
    q = _pedigree()
    sym32 = Symbolic([q["A"], q["I"]])
    sym32.set_front_precision(32)
    f32 = sym32.factorize([0.35, 0.65])
    buf = torch.zeros((4096,), dtype=torch.float64, device="cuda")
    bp = vp(buf.data_ptr())
    with pytest.raises(ScilmmError, match="fp32"):
        f32.sets_finish_dev(5, 3, bp, bp, bp, bp, 2, 2, start, 1, None, 0, rho, bp, 13, None)
    B = np.random.default_rng(0).standard_normal((q["A"].shape[0], 2))
    assert rel_err(q["V"] @ f32(B), B) < 1e-9


def test_a_distributed_handle_is_refused():
    """One rank of a world of two, never factorized (that would need the other rank): the refusal comes before any device work."""
    import torch
    from scilmm_amd import ScilmmError
    from scilmm_amd.dist import HipChainEngine
    from tests.test_gpu_halfsolve import _pedigree
    q = _pedigree()
    eng = HipChainEngine([q["A"], q["I"]], 0, 2, None, "cuda:0")
    buf = torch.zeros((4096,), dtype=torch.float64, device="cuda")
    bp = vp(buf.data_ptr())
    with pytest.raises(ScilmmError, match="distributed"):
        eng.fac.sets_finish_dev(5, 3, bp, bp, bp, bp, 2, 2, np.array([0, 2, 5], dtype=np.int32), 1, None, 0, np.array([0.0, 1.0]), bp, 12, None)
    assert eng.collectives == 0
