"""InteractionScan (marker x environment) against the un-whitened oracle of tests/gxe_oracle.py -- per-marker GLS of y on
[C, g~, g~ o e_1 ..] with the dense inv(V) -- and the layout of scilmm_scan_block_gxe_dev row by row against column dot
products of an explicit half-solve.

The two problems of tests/test_gpu_assoc.py: n = 300 is two slices of the statistics with a ragged second one; the pedigree's
n is no multiple of 16 and fills all SCAN_FOLD runs of the fold.  block in {16, 112, 128} with m in {1, 2, 3} gives block
widths d r of 16, 15, 16, 112, 111, 112, 128, 126, 128 (full, ragged, no multiple of 16; r <= 32 and r > 32: both shapes of
k_scan_cross) and 130 markers leave a partial last block at every one of them.

Tolerances: 1e-9 relative (max-norm over the markers, tests.helpers.rel_err) for the derived statistics, the suite's; the
host algebra on a dense CPU whitening agrees with the oracle to 3e-15 at n = 300 (tests/test_gxe_api.py).  The raw sums of
the entry point against dot products of the same forward solution taken in another order: 1e-12 relative (max-norm over the
row's markers) for |x_a|^2 and the cross rows; 1e-12 |q_k| |x_a| entry by entry for Q'x_a -- two orders of a sum of n terms
differ by at most 2 n 2^-53 sum |terms| = 4.4e-13 sum |terms| at n = 2000, and sum |terms| <= |q_k| |x_a|.  n_obs exact; mean
within 1e-15."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from tests import gxe_oracle as O
from tests import test_bed_api as T
from tests.helpers import random_spd, rel_err, small_pedigree

pytestmark = pytest.mark.gpu

M = 130                      # markers: partial last blocks at every block width
S2 = [0.4, 0.6]
vp = C.c_void_p

_PROBLEMS = {}


def _problem(name):
    """(A, I, markers, environment, covariates, y), the dense inv(V) and the oracles, built once per module."""
    if name not in _PROBLEMS:
        A = small_pedigree(2000, 0.01, 0)[0] if name == "pedigree" else random_spd(300, 0.05, 3)
        n = A.shape[0]
        I = sp.identity(n, format="csr")
        rng = np.random.default_rng(11)
        E = O.environment(n, 3, 5)
        extra = rng.standard_normal((n, 3))
        y = 0.5 + extra @ np.array([-0.2, 0.1, 0.3]) + E @ np.array([0.3, -0.1, 0.2]) + rng.standard_normal(n)
        _PROBLEMS[name] = dict(A=A, I=I, n=n, E=E, extra=extra, y=y, G=O.markers(n, M, 7, E[:, 0]), refs={},
                               Vi=np.linalg.inv((S2[0] * A + S2[1] * I).toarray()))
    return _PROBLEMS[name]


def _covariates(p, m, extra):
    """Intercept, optionally three more covariates, and the m environment columns: c = 1 + m or 4 + m."""
    return np.hstack([np.ones((p["n"], 1))] + ([p["extra"]] if extra else []) + [p["E"][:, :m]])


def _ref(p, m, extra):
    if (m, extra) not in p["refs"]:
        p["refs"][m, extra] = O.oracle(p["Vi"], _covariates(p, m, extra), p["y"], p["E"][:, :m], p["G"])
    return p["refs"][m, extra]


def _gxe(p, m, extra, block=None, s2=S2, chol=None, **kw):
    from scilmm_amd import AssociationScan, SparseCholesky
    chol = chol or SparseCholesky(**kw)
    scan = AssociationScan(chol, [p["A"], p["I"]], s2, _covariates(p, m, extra), p["y"], block=block)
    return scan.interaction(p["E"][:, :m]), scan, chol


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("block", [16, 112, 128])
@pytest.mark.parametrize("extra", [False, True])
@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("name", ["pedigree", "spd300"])
def test_int8_matches_dense_gls(name, m, extra, block):
    p = _problem(name)
    gxe, scan, _ = _gxe(p, m, extra, block)
    assert gxe.block == block // (1 + m) and gxe.scan is scan and scan.c == (4 if extra else 1) + m
    O.compare(gxe(p["G"]), _ref(p, m, extra), p["n"])


def test_default_block_and_no_markers():
    p = _problem("spd300")
    gxe, scan, _ = _gxe(p, 2, True)
    assert gxe.block == scan.block // 3
    O.compare(gxe(p["G"]), _ref(p, 2, True), p["n"])
    out = gxe(p["G"][:0])
    assert out["beta"].shape == (0, 3) and out["cov"].shape == (0, 3, 3) and out["p_int"].shape == (0,)


@pytest.mark.parametrize("name,m,block", [("pedigree", 2, 112), ("spd300", 3, 128), ("spd300", 1, 16)])
def test_bed_and_dosages_give_the_bits_of_the_int8_path(tmp_path, name, m, block):
    """The fills write the same W and the expansion does not know the form: in deterministic mode every key has the bits of
    the int8 path.  The fileset holds the same markers with its samples shuffled; float32 dosages of the same hard calls go
    to the oracle."""
    p = _problem(name)
    n, G = p["n"], p["G"]
    gxe, _, _ = _gxe(p, m, True, block, deterministic=True)
    ref = gxe(G)
    O.compare(ref, _ref(p, m, True), n)
    order = np.random.default_rng(3).permutation(n)              # the file's sample s is individual order[s]
    idx = np.argsort(order).astype(np.int32)
    path = T.write_fileset(tmp_path / "cohort", T.pack(G[:, order]), n)
    _same(gxe.scan_bed(path, sample_index=idx), ref)
    _same(gxe.scan_bed(path, sample_index=idx, chunk_bytes=1), ref)                  # a block per chunk
    _same(gxe.scan_bed(path, sample_index=idx, markers=np.array([7, 3, 120])), gxe(G[[7, 3, 120]]))   # (the bits depend on r)
    codes = np.ascontiguousarray(np.where(G >= 0, G.astype(np.int32) * 16384, 65535).astype(np.uint16))
    _same(gxe.scan_dosages(codes), ref)
    _same(gxe.scan_dosages(np.ascontiguousarray(codes[:, order]), sample_index=idx), ref)
    f32 = np.ascontiguousarray(np.where(G >= 0, G, np.nan).astype(np.float32))
    O.compare(gxe.scan_dosages(f32), _ref(p, m, True), n)


def test_raw_entry_point_layout_row_by_row():
    """One block at m = 2, r = 19 on the pedigree: every row of d_stats against the forward solution of the explicitly built
    d r columns (Factor.solve_L_dev) -- |x_a|^2, Q'x_a and the cross rows as column dot products."""
    import torch
    p = _problem("pedigree")
    n, m, r = p["n"], 2, 19
    d = 1 + m
    gxe, scan, _ = _gxe(p, m, True, 128, deterministic=True)
    q, G = scan.q, p["G"][:r]
    assert gxe.nrows == 3 + (q + 1) * d + d * (d - 1) // 2
    ld = (n + 15) // 16 * 16
    dG = torch.zeros((r, ld), dtype=torch.int8, device="cuda")
    dG[:, :n].copy_(torch.from_numpy(G))
    dS = torch.full((gxe.nrows * r + 8,), -7.0, dtype=torch.float64, device="cuda")     # (a guard behind the statistics)
    torch.cuda.synchronize()
    scan.factor.scan_block_gxe_dev(vp(dG.data_ptr()), ld, r, vp(gxe.dE.data_ptr()), m, vp(scan.dQ.data_ptr()), q, vp(dS.data_ptr()))
    scan.sym.sync()
    hS = dS.cpu().numpy()
    assert np.all(hS[gxe.nrows * r:] == -7.0)
    S = hS[:gxe.nrows * r].reshape(gxe.nrows, r)
    n_obs, mean, Gt = O.centred(G)
    assert np.array_equal(S[0], n_obs) and np.array_equal(S[2] == 0, np.arange(r) < 2)
    assert np.abs(S[1][n_obs > 0] - mean[n_obs > 0]).max() <= 1e-15
    # the d r columns, column a r + c = term a of marker c, through the half-solve the scan whitened [C | y] with
    E = p["E"][:, :m]
    cols = np.hstack([Gt.T] + [Gt.T * E[:, a:a + 1] for a in range(m)])
    perm = torch.from_numpy(scan.factor.P()).cuda()
    dB = torch.from_numpy(np.ascontiguousarray(cols)).cuda()[perm].contiguous()
    dX = torch.empty_like(dB)
    torch.cuda.synchronize()
    scan.factor.solve_L_dev(vp(dB.data_ptr()), d * r, vp(dX.data_ptr()))
    scan.sym.sync()
    X = dX.cpu().numpy().reshape(n, d, r)
    Q = scan.dQ.cpu().numpy()
    for a in range(d):
        assert rel_err(S[3 + a], (X[:, a] * X[:, a]).sum(axis=0)) < 1e-12, a
        for k in range(q):
            bound = 1e-12 * np.linalg.norm(Q[:, k]) * np.linalg.norm(X[:, a], axis=0)
            assert np.all(np.abs(S[3 + (k + 1) * d + a] - Q[:, k] @ X[:, a]) <= bound), (a, k)
    row = 3 + (q + 1) * d
    for a in range(d):
        for b in range(a + 1, d):
            assert rel_err(S[row], (X[:, a] * X[:, b]).sum(axis=0)) < 1e-12, (a, b)
            row += 1
    assert row == gxe.nrows
    # timing: the two kernels are parts of the first and the third interval
    t, g = scan.sym.scan_timing(), scan.sym.gxe_timing()
    assert 0 < g[0] <= t[0] and 0 < g[1] <= t[2]


def test_deterministic_scan_repeats_its_bits():
    p = _problem("pedigree")
    for m, block in ((1, 128), (3, 112)):
        gxe, scan, _ = _gxe(p, m, True, block, deterministic=True)
        a, b = gxe(p["G"]), gxe(p["G"])
        _same(a, b)
        assert scan.sym.timing()["n_float_atomic_launches"] == 0
        O.compare(a, _ref(p, m, True), p["n"])


def test_refusals_and_argument_checks():
    from scilmm_amd import ScilmmError, _lib
    p = _problem("spd300")
    gxe, scan, chol = _gxe(p, 2, False, 128)
    L, one, h, n = _lib.lib(), vp(8), scan.factor._h, p["n"]
    for r, m in ((4, 0), (4, 4), (65, 1), (43, 2), (33, 3)):
        assert L.scilmm_scan_block_gxe_dev(h, one, n, r, one, m, one, scan.q, one) == _lib.ERR_ARG, (r, m)
        assert L.scilmm_scan_block_bed_gxe_dev(h, one, (n + 3) // 4, n, None, 0, r, one, m, one, scan.q, one) == _lib.ERR_ARG, (r, m)
        assert L.scilmm_scan_block_dosage_gxe_dev(h, one, _lib.DOSAGE_F32, n, n, None, r, one, m, one, scan.q, one) == _lib.ERR_ARG, (r, m)
    assert L.scilmm_scan_block_gxe_dev(h, one, n, 4, None, 2, one, scan.q, one) == _lib.ERR_ARG      # a null d_E
    assert L.scilmm_scan_block_gxe_dev(h, one, n - 1, 4, one, 2, one, scan.q, one) == _lib.ERR_ARG   # pitch shorter than a row
    O.compare(gxe(p["G"]), _ref(p, 2, False), n)
    # the factor moves to another sigma2: the scan's whitening, which the interaction scan shares, is stale
    gxe2, scan2, _ = _gxe(p, 2, False, 128, s2=[0.7, 0.3], chol=chol)
    assert scan2.factor is scan.factor
    with pytest.raises(ScilmmError, match="sigma2"):
        gxe(p["G"])
    with pytest.raises(ScilmmError, match="sigma2"):
        scan.interaction(p["E"][:, :2])
    assert np.isfinite(gxe2(p["G"])["chi2_int"][O.FULL])
    scan2.factor.inverse_traces()                      # consumes the factor
    with pytest.raises(ScilmmError):
        gxe2(p["G"])
