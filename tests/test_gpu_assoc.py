"""AssociationScan against a per-marker GLS written here with the dense inv(V) -- the un-whitened formula, which shares
nothing with the code under test -- and against the project's own estimate_fixed_effects.

Tolerances: 1e-9 relative (max-norm over the markers, tests.helpers.rel_err) for the derived statistics, what the suite holds
for nll; n_obs exact; mean within 1e-15.  The two formulas agree to 3e-15 on the CPU at these inputs."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.stats as stats

from tests.helpers import random_spd, rel_err, small_pedigree

pytestmark = pytest.mark.gpu

TOL = 1e-9
M = 130                      # markers: partial last blocks at every block width below
MONO, ALLMISS, FULL, ENDS = 0, 1, 2, 3   # the overwritten markers
S2 = [0.4, 0.6]


def _markers(n, m, seed):
    """binomial(2, MAF), MAF uniform 0.05-0.5, 2 % missing (-1); four markers overwritten with the edge cases."""
    rng = np.random.default_rng(seed)
    maf = rng.uniform(0.05, 0.5, m)
    G = rng.binomial(2, maf[:, None], size=(m, n)).astype(np.int8)
    G[rng.random((m, n)) < 0.02] = -1
    G[MONO] = 1                                   # monomorphic
    G[ALLMISS] = -1                               # nothing observed
    G[FULL] = rng.binomial(2, 0.3, n)             # no missing value
    G[ENDS] = rng.binomial(2, 0.3, n)
    G[ENDS, 0] = G[ENDS, -1] = -1                 # missing at the first and the last individual only
    return np.ascontiguousarray(G)


def _centred(G):
    obs = G >= 0
    n_obs = obs.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(obs, G, 0).sum(axis=1) / n_obs
    Gt = np.where(obs, G - np.where(n_obs > 0, mean, 0.0)[:, None], 0.0)
    return n_obs, mean, Gt


_PROBLEMS = {}


def _problem(name):
    """(A, I, markers, covariates, y) and the dense inverses per sigma2, built once."""
    if name not in _PROBLEMS:
        A = small_pedigree(2000, 0.01, 0)[0] if name == "pedigree" else random_spd(300, 0.05, 3)
        n = A.shape[0]
        rng = np.random.default_rng(11)
        Cv = np.hstack([np.ones((n, 1)), rng.standard_normal((n, 3))])
        y = Cv @ np.array([0.5, -0.2, 0.1, 0.3]) + rng.standard_normal(n)
        _PROBLEMS[name] = dict(A=A, I=sp.identity(n, format="csr"), n=n, C=Cv, y=y, G=_markers(n, M, 7), G2=_markers(n, 37, 8), vi={})
    return _PROBLEMS[name]


def _oracle(p, s2, c, G):
    """beta, se, chi2 of the last coefficient of GLS of y on [C, g~] under V, marker by marker."""
    key = tuple(s2)
    if key not in p["vi"]:
        p["vi"][key] = np.linalg.inv((s2[0] * p["A"] + s2[1] * p["I"]).toarray())
    Vi, Cv, y = p["vi"][key], p["C"][:, :c], p["y"]
    n_obs, mean, Gt = _centred(G)
    ViG = Vi @ Gt.T
    ViC, Viy = Vi @ Cv, Vi @ y
    beta, se = np.full(len(G), np.nan), np.full(len(G), np.nan)
    for j in range(len(G)):
        if n_obs[j] == 0 or not Gt[j].any():
            continue
        X = np.hstack([Cv, Gt[j][:, None]])
        ViX = np.hstack([ViC, ViG[:, j][:, None]])
        XtViX = X.T @ ViX
        beta[j] = np.linalg.solve(XtViX, X.T @ Viy)[-1]
        se[j] = np.sqrt(np.linalg.inv(XtViX)[-1, -1])
    return dict(beta=beta, se=se, chi2=(beta / se) ** 2, n_obs=n_obs, mean=mean)


def _compare(out, ref, n):
    bad = np.zeros(len(ref["beta"]), bool)
    bad[[MONO, ALLMISS]] = True
    for k in ("beta", "se", "chi2"):
        print(k, "rel.err", rel_err(out[k][~bad], ref[k][~bad]))
        assert rel_err(out[k][~bad], ref[k][~bad]) < TOL, k
        assert np.array_equal(np.isnan(out[k]), bad), k     # NaN exactly at the two degenerate markers
    assert np.array_equal(np.isnan(out["p"]), bad)
    assert np.array_equal(out["p"], stats.f(1, n - 1).sf(out["chi2"]), equal_nan=True)
    assert out["n_obs"].dtype.kind == "i" and np.array_equal(out["n_obs"], ref["n_obs"])
    ok = ref["n_obs"] > 0
    assert np.abs(out["mean"][ok] - ref["mean"][ok]).max() <= 1e-15 and np.all(np.isnan(out["mean"][~ok]))


def _scan(p, c, block=None, s2=S2, chol=None, **kw):
    from scilmm_amd import AssociationScan, SparseCholesky
    chol = chol or SparseCholesky(**kw)
    return AssociationScan(chol, [p["A"], p["I"]], s2, p["C"][:, :c], p["y"], block=block), chol


@pytest.mark.parametrize("block", [16, 112, 128])
@pytest.mark.parametrize("c", [1, 4])
@pytest.mark.parametrize("name", ["pedigree", "spd300"])
def test_scan_matches_dense_gls(name, c, block):
    p = _problem(name)
    scan, _ = _scan(p, c, block)
    _compare(scan(p["G"]), _oracle(p, S2, c, p["G"]), p["n"])


def test_default_block_and_the_projects_own_fixed_effects():
    """block=None, and a second oracle through the public path: the last coefficient of estimate_fixed_effects(factor, y,
    [C, g~]) is the marker's beta."""
    from scilmm_amd import assoc, estimate_fixed_effects
    p = _problem("pedigree")
    scan, _ = _scan(p, 4)
    assert scan.block == assoc.DEFAULT_BLOCK and 112 <= scan.block <= 128
    out = scan(p["G"])
    _compare(out, _oracle(p, S2, 4, p["G"]), p["n"])
    _, _, Gt = _centred(p["G"])
    for j in (FULL, ENDS, M - 1):
        fe = estimate_fixed_effects(scan.factor, p["y"], np.hstack([p["C"], Gt[j][:, None]]))[3]
        assert abs(fe[-1] - out["beta"][j]) <= TOL * abs(fe[-1]), j


def test_deterministic_scan_repeats_its_bits():
    p = _problem("pedigree")
    scan, _ = _scan(p, 4, 112, deterministic=True)
    a, b = scan(p["G"]), scan(p["G"])
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert scan.sym.timing()["n_float_atomic_launches"] == 0
    _compare(a, _oracle(p, S2, 4, p["G"]), p["n"])


def test_more_than_one_chunk_gives_the_bits_of_one_chunk(monkeypatch):
    """The int8 scan in several chunks (``assoc._CHUNK_BYTES`` is read at call time) against the one chunk of the default: one
    block per chunk (eight full chunks and one of 2 markers), then two blocks per chunk (four full chunks and one of 2)."""
    from scilmm_amd import assoc
    p = _problem("pedigree")
    scan, _ = _scan(p, 4, 16, deterministic=True)
    ref = scan(p["G"])
    for chunk_bytes in (1, 32 * ((p["n"] + 15) // 16 * 16)):
        monkeypatch.setattr(assoc, "_CHUNK_BYTES", chunk_bytes)
        out = scan(p["G"])
        for k in ref:
            assert np.array_equal(out[k], ref[k], equal_nan=True), (chunk_bytes, k)


def test_repeated_use_and_a_second_sigma2():
    """One object, two marker sets; then a second object after the factor moved to another sigma2: nothing is carried over."""
    from scilmm_amd import ScilmmError
    p = _problem("pedigree")
    scan, chol = _scan(p, 4, 112)
    _compare(scan(p["G"]), _oracle(p, S2, 4, p["G"]), p["n"])
    _compare(scan(p["G2"]), _oracle(p, S2, 4, p["G2"]), p["n"])
    assert all(v.shape == (0,) for v in scan(p["G"][:0]).values())
    other = [0.7, 0.3]
    scan2, _ = _scan(p, 4, 112, s2=other, chol=chol)
    assert scan2.factor is scan.factor                   # the resident factor was refactorized, not doubled
    _compare(scan2(p["G"]), _oracle(p, other, 4, p["G"]), p["n"])
    with pytest.raises(ScilmmError, match="sigma2"):
        scan(p["G"])                                       # the first object's whitening belongs to the old factor


def _block_stats(scan, G, ld, offset, torch):
    """scilmm_scan_block_dev on a device copy of G whose rows are `ld` bytes apart and start `offset` bytes into a buffer."""
    r, n, q = G.shape[0], G.shape[1], scan.q
    buf = torch.full((offset + r * ld + 64,), 1, dtype=torch.int8, device="cuda")   # (an observed value between the rows: a
    for j in range(r):                                                                # kernel that counted it would miscount)
        buf[offset + j * ld: offset + j * ld + n] = torch.from_numpy(G[j]).cuda()
    dS = torch.zeros(((q + 4) * r,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    scan.factor.scan_block_dev(C.c_void_p(buf.data_ptr() + offset), ld, r, C.c_void_p(scan.dQ.data_ptr()), q, C.c_void_p(dS.data_ptr()))
    scan.sym.sync()
    return dS.cpu().numpy().reshape(q + 4, r)


def test_any_row_pitch_and_alignment_gives_the_same_bits():
    """The kernels read aligned 16-byte pieces whatever the pitch and the base address of the genotype rows."""
    import torch
    p = _problem("pedigree")
    n = p["n"]
    assert n % 16 != 0
    scan, _ = _scan(p, 4, 128, deterministic=True)
    G = p["G"][:19]
    ref = _block_stats(scan, G, (n + 15) // 16 * 16, 0, torch)
    for ld, offset in ((n, 0), (n, 3), (n + 5, 13)):
        assert np.array_equal(_block_stats(scan, G, ld, offset, torch), ref), (ld, offset)
    n_obs, mean, _ = _centred(G)
    assert np.array_equal(ref[0], n_obs) and np.array_equal(ref[2] == 0, np.arange(19) < 2)


def test_refusals_and_argument_checks():
    from scilmm_amd import ScilmmError, _lib
    p = _problem("spd300")
    scan, chol = _scan(p, 1, 16)
    L, one, h = _lib.lib(), C.c_void_p(8), scan.factor._h
    for r, q in ((0, 2), (129, 2), (4, 0), (4, 33)):
        assert L.scilmm_scan_block_dev(h, one, p["n"], r, one, q, one) == _lib.ERR_ARG
    assert L.scilmm_scan_block_dev(h, one, p["n"] - 1, 4, one, 2, one) == _lib.ERR_ARG     # pitch shorter than a row
    scan.factor.inverse_traces()                      # consumes the factor
    with pytest.raises(ScilmmError):
        scan(p["G"])
