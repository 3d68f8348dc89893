"""AssociationScan.scan_bed / scilmm_scan_block_bed_dev against the int8 path on the unpacked markers, bit for bit.

The tolerance of the comparisons with the int8 path is ZERO, and it is derived, not measured: the moments are integer sums
that go through the same two expressions (mean = sum / cnt, css = sq - sum * mean), W holds (double)g - mean of the same
integers, and everything behind W is the same launches; in deterministic mode those repeat their bits.  One case in the
default mode is held against the dense per-marker GLS of tests/test_gpu_assoc.py (re-stated here) at that file's 1e-9.
Files are written by the packer of tests/test_bed_api.py, padding bits set to ones."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.stats as stats

from tests import test_bed_api as T
from tests.helpers import random_spd, rel_err, small_pedigree

pytestmark = pytest.mark.gpu

TOL = 1e-9
M = 130                      # markers: a partial last block at widths 16 and 128
MONO, ALLMISS, FULL, ENDS = 0, 1, 2, 3
S2 = [0.4, 0.6]
KEYS = ("beta", "se", "chi2", "p", "n_obs", "mean")


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


_PROBLEMS = {}


def _problem(name):
    if name not in _PROBLEMS:
        A = small_pedigree(2000, 0.01, 0)[0] if name == "pedigree" else random_spd(301, 0.05, 3)
        n = A.shape[0]
        rng = np.random.default_rng(11)
        Cv = np.hstack([np.ones((n, 1)), rng.standard_normal((n, 3))])
        y = Cv @ np.array([0.5, -0.2, 0.1, 0.3]) + rng.standard_normal(n)
        G = _markers(n, M, 7)
        _PROBLEMS[name] = dict(A=A, I=sp.identity(n, format="csr"), n=n, C=Cv, y=y, G=G,
                               G3=np.ascontiguousarray(np.vstack([G, _markers(n, 137, 8)])), scans={}, ref={})
    return _PROBLEMS[name]


def _scan(p, block, deterministic=True):
    """One scan object per (problem, block, mode), shared by the tests."""
    from scilmm_amd import AssociationScan, SparseCholesky
    key = (block, deterministic)
    if key not in p["scans"]:
        p["scans"][key] = AssociationScan(SparseCholesky(deterministic=deterministic), [p["A"], p["I"]], S2, p["C"], p["y"],
                                          block=block)
    return p["scans"][key]


def _same(a, b):
    assert sorted(a) == sorted(b) == sorted(KEYS)
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("block", [16, 128])
@pytest.mark.parametrize("name", ["spd301", "pedigree"])
def test_identity_map_gives_the_bits_of_the_int8_path(tmp_path, name, block):
    """267 markers: three chunks of one block at width 128 (128 + 128 + 11), seventeen at width 16, the last one partial."""
    p = _problem(name)
    n = p["n"]
    if name == "spd301":
        assert (n % 4, n % 16, n % 64) == (1, 13, 45)
    G = p["G3"]
    path = T.write_fileset(tmp_path / "id", T.pack(G), n)
    scan = _scan(p, block)
    nb = (n + 3) // 4
    out = scan.scan_bed(path, chunk_bytes=block * nb)
    assert -(-len(G) // block) >= 3 and len(G) % block
    ref = scan(G)
    _same(out, ref)
    assert np.array_equal(np.isnan(out["beta"][:4]), [True, True, False, False])
    assert np.array_equal(out["n_obs"], (G >= 0).sum(axis=1))
    _same(scan.scan_bed(path), ref)                                   # one chunk
    assert scan.sym.timing()["n_float_atomic_launches"] == 0
    # markers as a slice and as an index array; none at all
    from scilmm_amd.bed import BedFile
    bed = BedFile(path)
    _same(scan.scan_bed(bed, markers=slice(5, 200, 3)), scan(np.ascontiguousarray(G[5:200:3])))
    pick = np.array([266, 0, 1, 130, 7, 7])
    _same(scan.scan_bed(bed, markers=pick, chunk_bytes=1), scan(np.ascontiguousarray(G[pick])))
    empty = scan.scan_bed(bed, markers=slice(0, 0))
    assert sorted(empty) == sorted(KEYS) and all(v.shape == (0,) for v in empty.values())


def _oracle(p, G):
    """beta, se, chi2 of the last coefficient of GLS of y on [C, g~] under V, marker by marker (tests/test_gpu_assoc.py)."""
    Vi = np.linalg.inv((S2[0] * p["A"] + S2[1] * p["I"]).toarray())
    Cv, y = p["C"], p["y"]
    obs = G >= 0
    n_obs = obs.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(obs, G, 0).sum(axis=1) / n_obs
    Gt = np.where(obs, G - np.where(n_obs > 0, mean, 0.0)[:, None], 0.0)
    ViG, ViC, Viy = Vi @ Gt.T, Vi @ Cv, Vi @ y
    beta, se = np.full(len(G), np.nan), np.full(len(G), np.nan)
    for j in range(len(G)):
        if n_obs[j] == 0 or not Gt[j].any():
            continue
        X = np.hstack([Cv, Gt[j][:, None]])
        XtViX = X.T @ np.hstack([ViC, ViG[:, j][:, None]])
        beta[j] = np.linalg.solve(XtViX, X.T @ Viy)[-1]
        se[j] = np.sqrt(np.linalg.inv(XtViX)[-1, -1])
    return dict(beta=beta, se=se, chi2=(beta / se) ** 2, n_obs=n_obs, mean=mean)


def test_default_mode_matches_dense_gls(tmp_path):
    p = _problem("pedigree")
    n, G = p["n"], p["G"]
    scan = _scan(p, None, deterministic=False)
    out = scan.scan_bed(T.write_fileset(tmp_path / "gls", T.pack(G), n))
    ref = _oracle(p, G)
    bad = np.zeros(M, bool)
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


def _mapped(n, N, seed):
    """A file of N shuffled samples for a cohort of n: 5 % of the cohort absent, two individuals on one sample."""
    rng = np.random.default_rng(seed)
    idx = rng.permutation(N)[:n].astype(np.int32)
    absent = rng.choice(n, size=max(1, n // 20), replace=False)
    idx[absent] = -1
    here = np.flatnonzero(idx >= 0)
    idx[here[1]] = idx[here[0]]                    # two individuals share a sample
    return idx, here


def _gather(Gf, idx, N):
    ok = (idx >= 0) & (idx < N)
    return np.ascontiguousarray(np.where(ok, Gf[:, np.where(ok, idx, 0)], -1).astype(np.int8))


def _block_bed(scan, dB_ptr, ld, N, idx, flags, r, torch):
    q = scan.q
    dI = None if idx is None else torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).cuda()
    dS = torch.zeros(((q + 4) * r,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    scan.factor.scan_block_bed_dev(C.c_void_p(dB_ptr), ld, N, None if dI is None else C.c_void_p(dI.data_ptr()), flags, r,
                                   C.c_void_p(scan.dQ.data_ptr()), q, C.c_void_p(dS.data_ptr()))
    scan.sym.sync()
    return dS.cpu().numpy().reshape(q + 4, r)


def _block_int8(scan, G, torch):
    r, n, q = G.shape[0], G.shape[1], scan.q
    ld = (n + 15) // 16 * 16
    dG = torch.zeros((r, ld), dtype=torch.int8, device="cuda")
    dG[:, :n].copy_(torch.from_numpy(G))
    dS = torch.zeros(((q + 4) * r,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    scan.factor.scan_block_dev(C.c_void_p(dG.data_ptr()), ld, r, C.c_void_p(scan.dQ.data_ptr()), q, C.c_void_p(dS.data_ptr()))
    scan.sym.sync()
    return dS.cpu().numpy().reshape(q + 4, r)


@pytest.mark.parametrize("extra", [37, 38, 39])
@pytest.mark.parametrize("name", ["spd301", "pedigree"])
def test_sample_map_gives_the_bits_of_the_gathered_int8_markers(tmp_path, name, extra):
    import torch
    p = _problem(name)
    n = p["n"]
    N = n + extra
    Gf = _markers(N, M, 20 + extra)
    idx, here = _mapped(n, N, extra)
    assert (idx < 0).sum() >= n // 20 and len(set(idx[idx >= 0])) == (idx >= 0).sum() - 1
    packed = T.pack(Gf)
    path = T.write_fileset(tmp_path / "map", packed, N)
    scan = _scan(p, 128)
    Gc = _gather(Gf, idx, N)
    ref = scan(Gc)
    _same(scan.scan_bed(path, sample_index=idx, chunk_bytes=1), ref)
    assert np.array_equal(ref["n_obs"], (Gc >= 0).sum(axis=1))
    _same(scan.scan_bed(path, sample_index=idx.astype(np.int64), count="A2"), scan(np.where(Gc >= 0, 2 - Gc, -1).astype(np.int8)))
    _same(_scan(p, 16).scan_bed(path, sample_index=idx, markers=slice(0, 40)), _scan(p, 16)(Gc[:40]))
    # samples past the file's last one, which scan_bed refuses on the host: through the C entry point they are missing
    far = idx.copy()
    far[here[2]], far[here[3]] = N, 2 ** 31 - 1
    nb = packed.shape[1]
    dB = torch.from_numpy(packed[:19].copy()).cuda()
    got = _block_bed(scan, dB.data_ptr(), nb, N, far, 0, 19, torch)
    want = _block_int8(scan, _gather(Gf[:19], far, N), torch)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(got[0], (_gather(Gf[:19], far, N) >= 0).sum(axis=1))
    assert not np.array_equal(got[0], (Gc[:19] >= 0).sum(axis=1))


def test_any_row_pitch_and_alignment_gives_the_same_bits():
    """Aligned 16-byte pieces whatever the pitch and the base address; the bytes between and around the rows are 0x00, four
    observed samples with two copies of A1 each: a kernel that counted them would miscount."""
    import torch
    p = _problem("pedigree")
    n = p["n"]
    scan = _scan(p, 128)
    G = p["G"][:19]
    packed = T.pack(G)
    nb = packed.shape[1]
    res = []
    for ld, offset in ((nb, 0), (nb, 3), (nb + 5, 13), ((nb + 15) // 16 * 16, 0)):
        host = np.zeros(offset + 19 * ld + 64, dtype=np.uint8)
        for j in range(19):
            host[offset + j * ld: offset + j * ld + nb] = packed[j]
        buf = torch.from_numpy(host).cuda()
        res.append(_block_bed(scan, buf.data_ptr() + offset, ld, n, None, 0, 19, torch))
    for s in res[1:]:
        assert np.array_equal(s, res[0], equal_nan=True)
    assert np.array_equal(res[0][0], (G >= 0).sum(axis=1))
    assert np.array_equal(res[0], _block_int8(scan, G, torch), equal_nan=True)


@pytest.mark.parametrize("name", ["spd301", "pedigree"])
def test_count_a2(tmp_path, name):
    p = _problem(name)
    G = p["G"]
    scan = _scan(p, 128)
    out = scan.scan_bed(T.write_fileset(tmp_path / "a2", T.pack(G), p["n"]), count="A2")
    _same(out, scan(np.where(G >= 0, 2 - G, -1).astype(np.int8)))
    with pytest.raises(ValueError):
        scan.scan_bed(str(tmp_path / "a2"), count="a2")


def test_argument_checks_and_refusals(tmp_path):
    from scilmm_amd import AssociationScan, ScilmmError, SparseCholesky, _lib
    p = _problem("spd301")
    n = p["n"]
    scan = AssociationScan(SparseCholesky(), [p["A"], p["I"]], S2, p["C"][:, :1], p["y"], block=16)
    L, one, h, f = _lib.lib(), C.c_void_p(8), scan.factor._h, _lib.lib().scilmm_scan_block_bed_dev
    nb = (n + 3) // 4
    assert f(h, None, nb, n, None, 0, 4, one, 2, one) == _lib.ERR_ARG                      # a null d_bed
    assert f(None, one, nb, n, None, 0, 4, one, 2, one) == _lib.ERR_ARG
    assert f(h, one, nb, n, None, 0, 4, None, 2, one) == _lib.ERR_ARG
    assert f(h, one, nb, n, None, 0, 4, one, 2, None) == _lib.ERR_ARG
    for r, q in ((0, 2), (129, 2), (4, 0), (4, 33)):
        assert f(h, one, nb, n, None, 0, r, one, q, one) == _lib.ERR_ARG
    for N in (0, -1):
        assert f(h, one, nb, N, one, 0, 4, one, 2, one) == _lib.ERR_ARG                    # n_samples < 1
    assert f(h, one, nb - 1, n, None, 0, 4, one, 2, one) == _lib.ERR_ARG                   # pitch shorter than a row
    assert f(h, one, nb, 4 * nb + 1, one, 0, 4, one, 2, one) == _lib.ERR_ARG               # ... of 4 nb + 1 samples (nb + 1 bytes)
    for flags in (2, 3, 4, -1, 1 << 30):
        assert f(h, one, nb, n, None, flags, 4, one, 2, one) == _lib.ERR_ARG               # unknown flag bits
    for N in (n - 1, n + 1):
        assert f(h, one, nb + 1, N, None, 0, 4, one, 2, one) == _lib.ERR_ARG               # identity map with N != n
    G = p["G"]
    path = T.write_fileset(tmp_path / "arg", T.pack(G), n)
    big = T.write_fileset(tmp_path / "big", T.pack(_markers(n + 2, 5, 1)), n + 2)
    ident = np.arange(n)
    for bad in (ident[:-1], np.r_[ident, 0], np.where(ident == 5, n, ident), np.where(ident == 5, -2, ident), ident[None, :],
                ident.astype(float)):
        with pytest.raises(ValueError):
            scan.scan_bed(path, sample_index=bad)
    with pytest.raises(ValueError, match="sample_index"):
        scan.scan_bed(big)                                 # sample_index=None with N != n
    assert np.array_equal(scan.scan_bed(big, sample_index=ident)["n_obs"][2], n)
    scan.factor.inverse_traces()                           # consumes the factor
    with pytest.raises(ScilmmError):
        scan.scan_bed(path)
