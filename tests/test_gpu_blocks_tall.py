"""The block calls on a resident factor at cohort sizes where their folds hold runs of several slices and their capped grids
wrap: the marker scan in its three input forms, G x E, the Gram block, the panel, the keep, the BLUP blocks and
scilmm_csr_spmm_dev, on the three family cohorts of tests/tall_cohorts.py (T8K n = 8199, T65K n = 65 577, B64 n = 16 448;
tests/test_tall_cohorts.py asserts without a GPU which loop of which kernel each of them reaches).

References: the un-whitened per-marker GLS of tests/test_gpu_assoc.py (and of tests/gxe_oracle.py) with the block-wise
sparse inverse of V in place of the dense one -- nothing is densified --, and X_ref = solve_L(apply_P(.)) through the public
half-solve, every reduction of it taken in np.longdouble.

Tolerances, the project's: 1e-9 for beta, se and chi2 (test_gpu_assoc.TOL; the two GLS formulas agree to 4e-13 on the CPU at
these cohorts, tests/test_tall_cohorts.py); 1e-12 max-norm for the Gram, panel, keep and cross products and the raw rows of
the statistics (test_gpu_panel; fp64 sums of 65 577 terms are good to 1e-15, tests/test_tall_cohorts.py); 1e-13 for
DeviceCSR.dot (test_gpu_reml); n_obs exact; mean within 1e-15; css within 4 u sum(g^2) of the exact value in Python integers
(u = 2^-53: the kernel's three sums are exact integers, so only one division, one product and one subtraction round).

Every comparison prints its measured error.  Measured (MI355X):
  scan vs GLS      T8K  c = 1: beta 6.2e-14, se 3.1e-14, chi2 3.6e-14; c = 4: 4.9e-14, 3.1e-14, 3.8e-14 (block 16 and 128 alike)
                   T65K c = 4: beta 1.1e-14, se 1.3e-15, chi2 2.3e-14
  raw int8 block   T8K  mean 5.5e-17, css 0.58 u sum(g^2), |x|^2 6.0e-16, Q'x 5.5e-16
                   T65K mean 4.4e-17, css 0.60 u sum(g^2) (gathered: 0.53), |x|^2 6.1e-16, Q'x 1.8e-15
  input forms      .bed and uint16 bit-identical to int8 under either map; float32 identical but for css (5.5e-15 from it)
  Gram             r = 19: 1.6e-15 vs X_ref'X_ref, diagonal vs |x|^2 1.6e-15; r = 128: 2.6e-15, 2.8e-15
  panel            T8K 0 .. 1.8e-15; T65K 1.7e-15 .. 1.8e-15
  keep             0 (a copy) in all four cases
  G x E vs GLS     m = 1: beta 7.5e-14, se 4.9e-14, cov 8.2e-14, chi2_int 1.9e-14, chi2_joint 2.6e-14; m = 3: 7.3e-14, 4.9e-14,
                   8.3e-14, 2.0e-14, 2.1e-14; |x_a|^2 2.0e-16 .. 6.0e-16, cross rows 1.6e-16 .. 3.3e-16
  BLUP blocks      65 requests, 2016 row-part slots, all at or past 256 * REL_GRID; |x|^2 3.9e-16, Q'x 4.5e-16 (both handles)
  DeviceCSR.dot    0 (rows of at most eight entries, summed in storage order as scipy does)
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

from tests import gxe_oracle as XO
from tests import tall_cohorts as TC
from tests import test_gpu_assoc as GA
from tests.helpers import rel_err
from tests.test_bed_api import pack

pytestmark = pytest.mark.gpu

TOL = GA.TOL                 # derived statistics
PROD = 1e-12                 # products of the forward solution, max-norm
CANARY = 7.25
U = 2.0 ** -53
TMAXT = 130                  # traits of the widest panel: across the 128-column panel boundary
DEGENERATE = (GA.MONO, GA.ALLMISS)
vp = C.c_void_p

_KEPT = {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_cohorts():
    yield
    _KEPT.clear()
    TC.release()


def _once(key, make):
    if key not in _KEPT:
        _KEPT[key] = make()
    return _KEPT[key]


def _chol(cid, det=False):
    """One SparseCholesky per cohort and mode: its analysis and its resident factor serve every case of the module."""
    from scilmm_amd import SparseCholesky
    return _once(("chol", cid, det), lambda: SparseCholesky(deterministic=det))


def _scan(cid, c=4, block=128, det=False, covariates=None):
    from scilmm_amd import AssociationScan
    p = TC.cohort(cid)
    Cv = p["C"][:, :c] if covariates is None else covariates
    return AssociationScan(_chol(cid, det), [p["A"], p["I"]], TC.S2, Cv, p["y"], block=block)


def _xref(scan, key, cols):
    """X_ref = solve_L(apply_P(cols)) on the scan's factor, as np.longdouble; kept per key.  (A half-solve uses the work
    buffers: it comes before the block whose left-behind X a case reads.)"""
    fac = scan.factor
    return _once(("xref", id(fac)) + key, lambda: fac.solve_L(fac.apply_P(np.ascontiguousarray(cols))).astype(np.longdouble))


def _xref_markers(scan, cid):
    """X_ref of the cohort's 130 markers, n x 130."""
    return _xref(scan, (cid, "G"), GA._centred(TC.markers(TC.cohort(cid)))[2].T)


def _dot(Xa, Xb):
    """Xa' Xb in np.longdouble (einsum: numpy's matmul has no fast path for it)."""
    return np.einsum("ni,nj->ij", Xa, Xb).astype(np.float64)


def _oracle(cid, c):
    p = TC.cohort(cid)
    TC.inverse(p)
    return _once(("gls", cid, c), lambda: GA._oracle(p, TC.S2, c, TC.markers(p)))


def _ld(n):
    return (n + 15) // 16 * 16


def _rows_int8(G, torch):
    dG = torch.zeros((G.shape[0], _ld(G.shape[1])), dtype=torch.int8, device="cuda")
    dG[:, :G.shape[1]].copy_(torch.from_numpy(np.ascontiguousarray(G)))
    return dG


def _block(scan, G, torch, gram=False, sentinel=-CANARY):
    """One int8 block through scilmm_scan_block_dev (or _gram_dev), waited for: statistics (q + 4) x r (and the whole Gram
    buffer, r * r values and 64 of the sentinel behind them)."""
    r, n, q = G.shape[0], G.shape[1], scan.q
    dG = _rows_int8(G, torch)
    dS = torch.zeros(((q + 4) * r,), dtype=torch.float64, device="cuda")
    dK = torch.full((r * r + 64,), sentinel, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    if gram:
        scan.factor.scan_block_gram_dev(vp(dG.data_ptr()), _ld(n), r, vp(scan.dQ.data_ptr()), q, vp(dS.data_ptr()), vp(dK.data_ptr()))
    else:
        scan.factor.scan_block_dev(vp(dG.data_ptr()), _ld(n), r, vp(scan.dQ.data_ptr()), q, vp(dS.data_ptr()))
    scan.sym.sync()
    S = dS.cpu().numpy().reshape(q + 4, r)
    return (S, dK.cpu().numpy()) if gram else S


def _check_moments(S, G, what):
    """Rows 0..2 of a block's statistics against the integer sums of the int8 markers G."""
    worst_mean, worst_css = 0.0, 0.0
    for j, (cnt, s, sq) in enumerate(TC.exact_moments(G)):
        assert S[0][j] == cnt, (what, j)
        if cnt == 0:
            assert S[1][j] == 0.0 and S[2][j] == 0.0, (what, j)          # (the raw rows; the scan turns the mean into NaN)
            continue
        em = abs(Fraction(float(S[1][j])) - Fraction(s, cnt))
        exact = Fraction(sq) - Fraction(s * s, cnt)
        ec = abs(Fraction(float(S[2][j])) - exact)
        assert em <= Fraction(1e-15), (what, j)
        assert ec <= 4 * Fraction(U) * sq, (what, j)
        assert (S[2][j] == 0.0) == (exact == 0), (what, j)
        worst_mean, worst_css = max(worst_mean, float(em)), max(worst_css, float(ec / (Fraction(U) * sq)))
    print(what, "mean abs.err %.2e" % worst_mean, "css err / (u sum g^2) %.3f" % worst_css)


def _check_rows_3(S, scan, X, what):
    """Rows 3.. of a plain block (|x_c|^2, Q'x_c) against the longdouble reductions of X_ref."""
    Q = scan.dQ.cpu().numpy().astype(np.longdouble)
    e_gg, e_qx = rel_err(S[3], (X * X).sum(axis=0).astype(np.float64)), rel_err(S[4:], _dot(Q, X))
    print(what, "|x|^2 rel.err %.2e" % e_gg, "Q'x rel.err %.2e" % e_qx)
    assert e_gg < PROD and e_qx < PROD, what


# ---- 1. the scan at T8K

@pytest.mark.parametrize("block", [16, 128])
@pytest.mark.parametrize("c", [1, 4])
def test_scan_at_t8k_matches_the_blockwise_gls(c, block):
    p = TC.cohort("T8K")
    out = _scan("T8K", c, block)(TC.markers(p))
    print("T8K c", c, "block", block)
    GA._compare(out, _oracle("T8K", c), p["n"])


def test_raw_block_at_t8k_against_the_half_solve():
    """19 markers, the four edge markers among them: 33 slices in runs of 5, 5, 5, 5, 5, 5, 3, 0 and three trips of the moments."""
    import torch
    p = TC.cohort("T8K")
    scan = _scan("T8K", 4, 128)
    X = _xref_markers(scan, "T8K")[:, :19]
    G = TC.markers(p)[:19]
    S = _block(scan, G, torch)
    _check_moments(S, G, "T8K int8")
    _check_rows_3(S, scan, X, "T8K r 19")
    assert np.all(S[3:, :2] == 0.0)                           # the monomorphic and the all-missing marker: zero columns


# ---- 2. the scan at T65K, and the three input forms

def test_scan_at_t65k_matches_the_blockwise_gls():
    p = TC.cohort("T65K")
    out = _scan("T65K", 4, 128)(TC.markers(p))
    print("T65K c 4 block 128")
    GA._compare(out, _oracle("T65K", 4), p["n"])


def _block_bed(scan, packed, N, idx, r, torch):
    dB = torch.from_numpy(np.ascontiguousarray(packed[:r])).cuda()
    dI = None if idx is None else torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).cuda()
    dS = torch.zeros(((scan.q + 4) * r,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    scan.factor.scan_block_bed_dev(vp(dB.data_ptr()), packed.shape[1], N, None if dI is None else vp(dI.data_ptr()), 0, r,
                                   vp(scan.dQ.data_ptr()), scan.q, vp(dS.data_ptr()))
    scan.sym.sync()
    return dS.cpu().numpy().reshape(scan.q + 4, r)


def _block_dosage(scan, rows, N, idx, r, torch):
    from scilmm_amd import _lib
    kind = _lib.DOSAGE_U16 if rows.dtype == np.uint16 else _lib.DOSAGE_F32
    dD = torch.from_numpy(np.ascontiguousarray(rows[:r]).view(np.uint8)).cuda()
    dI = None if idx is None else torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).cuda()
    dS = torch.zeros(((scan.q + 4) * r,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    scan.factor.scan_block_dosage_dev(vp(dD.data_ptr()), kind, rows.shape[1], N, None if dI is None else vp(dI.data_ptr()), r,
                                      vp(scan.dQ.data_ptr()), scan.q, vp(dS.data_ptr()))
    scan.sym.sync()
    return dS.cpu().numpy().reshape(scan.q + 4, r)


def _codes(G):
    return np.ascontiguousarray(np.where(G >= 0, G.astype(np.int32) * 16384, 65535).astype(np.uint16))


def _floats(G):
    return np.ascontiguousarray(np.where(G >= 0, G, np.nan).astype(np.float32))


def test_input_forms_at_t65k_give_the_bits_of_the_int8_block():
    """One raw block of 19 markers as .bed, uint16 and float32 dosages: with the identity map (the piece loops of the moments
    kernels in 5, 9 and 17 trips), then with a sample map that reorders the individuals and drops some (33 rounds of eight
    individuals in flight).  The int8 block itself against the integer moments and the half-solve."""
    import torch
    p = TC.cohort("T65K")
    n = p["n"]
    scan = _scan("T65K", 4, 128, det=True)
    X = _xref_markers(scan, "T65K")[:, :19]
    G = TC.markers(p)[:19]
    want = _block(scan, G, torch)
    _check_moments(want, G, "T65K int8")
    _check_rows_3(want, scan, X, "T65K r 19")
    N = n + 38
    Gf = GA._markers(N, 19, 21)
    rng = np.random.default_rng(3)
    idx = rng.permutation(N)[:n].astype(np.int32)
    idx[rng.choice(n, size=n // 20, replace=False)] = -1
    idx[-1] = N - 1                                            # the file's last sample at the last individual
    Gc = np.ascontiguousarray(np.where(idx >= 0, Gf[:, np.maximum(idx, 0)], -1).astype(np.int8))
    mapped = _block(scan, Gc, torch)
    _check_moments(mapped, Gc, "T65K int8, gathered")
    assert not np.array_equal(mapped[0], want[0])
    rest = [0, 1] + list(range(3, len(want)))                 # (float32: css is a two-pass fp64 sum, not the integers')
    for what, rows, full, Nf, ix in (("identity", G, want, n, None), ("mapped", Gf, mapped, N, idx)):
        S = _block_bed(scan, pack(rows), Nf, ix, 19, torch)
        assert np.array_equal(S, full, equal_nan=True), (".bed", what)
        S = _block_dosage(scan, _codes(rows), Nf, ix, 19, torch)
        assert np.array_equal(S, full, equal_nan=True), ("uint16", what)
        S = _block_dosage(scan, _floats(rows), Nf, ix, 19, torch)
        assert np.array_equal(S[rest], full[rest], equal_nan=True), ("float32", what)
        assert np.array_equal(S[2] == 0, full[2] == 0), ("float32", what)
        ok = full[2] != 0
        print("T65K float32", what, "css rel.diff to the integers' %.2e" % rel_err(S[2][ok], full[2][ok]))
    assert scan.sym.timing()["n_float_atomic_launches"] == 0


# ---- 3. the Gram block at T8K

@pytest.mark.parametrize("r", [19, 128])
def test_gram_at_t8k(r):
    """17 slices of 512 rows in runs of 5, 5, 5, 2.  r = 19: the first markers, the two zero columns among them; r = 128:
    markers 2 .. 129."""
    import torch
    p = TC.cohort("T8K")
    scan = _scan("T8K", 4, 128)
    lo = 0 if r == 19 else 2
    X = _xref_markers(scan, "T8K")[:, lo:lo + r]
    G = TC.markers(p)[lo:lo + r]
    S, K = _block(scan, G, torch, gram=True)
    S0 = _block(scan, G, torch)
    assert np.array_equal(S[:3], S0[:3])
    assert np.all(K[r * r:] == -CANARY) and not np.any(K[:r * r] == -CANARY)      # exactly r * r written
    K = K[:r * r].reshape(r, r)
    assert np.array_equal(K, K.T)                                                 # symmetric bit for bit
    ref = _once(("xtx", "T8K", id(scan.factor), r), lambda: _dot(X, X))
    print("T8K Gram r", r, "vs X_ref'X_ref %.2e" % rel_err(K, ref), "diagonal vs |x|^2 %.2e" % rel_err(np.diag(K), S[3]))
    assert rel_err(K, ref) < PROD
    assert rel_err(np.diag(K), S[3]) < 1e-12
    _check_rows_3(S, scan, X, "T8K Gram block r %d" % r)


# ---- 4. the panel at T8K and T65K

def _panel_problem(cid, scan):
    """Markers 2 .. 129 (all of them vary: the block of r = 1 is no zero column), 130 standard normal trait columns in the
    permuted order, and X_ref' Y."""
    def make():
        n = TC.cohort(cid)["n"]
        X = _xref_markers(scan, cid)[:, 2:]
        Yp = np.random.default_rng(3).standard_normal((n, TMAXT))
        return dict(Yp=Yp, ref=_dot(X, Yp.astype(np.longdouble)))
    return _once(("panel", cid, id(scan.factor)), make)


@pytest.mark.parametrize("t", [1, TMAXT])
@pytest.mark.parametrize("r", [1, 128])
@pytest.mark.parametrize("cid", ["T8K", "T65K"])
def test_panel_across_runs_of_slices(cid, r, t):
    """scilmm_scan_panel_dev behind one int8 block: five slices of 2048 rows in runs of 2, 2, 1, 0 at T8K, 33 in runs of 9, 9,
    9, 6 at T65K.  ld_out = t + 3 with a canary in the spare columns and in row r; NaN in Y's padding columns."""
    import torch
    p = TC.cohort(cid)
    n = p["n"]
    scan = _scan(cid, 1, 128)
    prob = _panel_problem(cid, scan)
    G = TC.markers(p)[2:2 + r]
    ld_y, ld_out = (t + 15) // 16 * 16, t + 3
    dG = _rows_int8(G, torch)
    dY = torch.full((n, ld_y), float("nan"), dtype=torch.float64, device="cuda")
    dY[:, :t] = torch.from_numpy(np.ascontiguousarray(prob["Yp"][:, :t])).cuda()
    dO = torch.full((r + 1, ld_out), CANARY, dtype=torch.float64, device="cuda")
    dS = torch.zeros(((scan.q + 4) * r,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    fac = scan.factor
    fac.scan_block_dev(vp(dG.data_ptr()), _ld(n), r, vp(scan.dQ.data_ptr()), scan.q, vp(dS.data_ptr()))
    fac.scan_panel_dev(r, vp(dY.data_ptr()), ld_y, t, vp(dO.data_ptr()), ld_out)
    scan.sym.sync()
    out, stat = dO.cpu().numpy(), dS.cpu().numpy().reshape(scan.q + 4, r)
    assert np.array_equal(stat[0], (G >= 0).sum(axis=1))
    ref = prob["ref"][:r, :t]
    assert np.all(np.isfinite(out))
    print(cid, "panel r", r, "t", t, "rel.err %.2e" % rel_err(out[:r, :t], ref))
    assert rel_err(out[:r, :t], ref) < PROD and np.abs(ref).min() > 0.0
    assert np.all(out[:r, t:] == CANARY) and np.all(out[r] == CANARY)


# ---- 5. the keep at T65K

@pytest.mark.parametrize("col0", [0, 32])
@pytest.mark.parametrize("r", [19, 128])
def test_keep_at_t65k_strides_over_its_grid(r, col0):
    """2050 chunks of 32 rows on 2048 workgroups, the last chunk of 9 rows.  The store has one spare row and 16 spare columns
    behind the block's."""
    import torch
    p = TC.cohort("T65K")
    n = p["n"]
    scan = _scan("T65K", 1, 128)
    lo = 0 if r == 19 else 2
    X = _xref_markers(scan, "T65K")[:, lo:lo + r].astype(np.float64)
    G = TC.markers(p)[lo:lo + r]
    rp = (r + 15) // 16 * 16
    ld = col0 + rp + 16
    dG = _rows_int8(G, torch)
    dS = torch.zeros(((scan.q + 4) * r,), dtype=torch.float64, device="cuda")
    store = torch.full((n + 1, ld), CANARY, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    fac = scan.factor
    fac.scan_block_dev(vp(dG.data_ptr()), _ld(n), r, vp(scan.dQ.data_ptr()), scan.q, vp(dS.data_ptr()))
    fac.scan_block_keep_dev(r, vp(store.data_ptr()), ld, col0)
    scan.sym.sync()
    got = store.cpu().numpy()
    print("T65K keep r", r, "col0", col0, "kept columns vs X_ref %.2e" % rel_err(got[:n, col0:col0 + r], X),
          "rows from 65536 on %.2e" % rel_err(got[65536:n, col0:col0 + r], X[65536:]))
    assert rel_err(got[:n, col0:col0 + r], X) < PROD
    assert rel_err(got[65536:n, col0:col0 + r], X[65536:]) < PROD          # the two chunks of the second trip, by themselves
    assert np.all(got[:n, col0 + r:col0 + rp] == 0.0)
    assert np.all(got[:n, :col0] == CANARY) and np.all(got[:n, col0 + rp:] == CANARY)
    assert np.all(got[n] == CANARY)


# ---- 6. G x E at T8K

def _gxe_problem(m):
    """Covariates [1, e_1 .. e_m] (the main effects in the null model), the oracle with the block-wise inverse."""
    def make():
        p = TC.cohort("T8K")
        E = XO.environment(p["n"], 3, 5)[:, :m]
        Cv = np.hstack([np.ones((p["n"], 1)), E])
        return dict(E=E, C=Cv, ref=XO.oracle(TC.inverse(p), Cv, p["y"], E, TC.markers(p), skip=DEGENERATE))
    return _once(("gxe", m), make)


@pytest.mark.parametrize("m,per_block", [(1, 64), (3, 32)])
def test_gxe_at_t8k(m, per_block):
    """m = 1: 64 markers per block, k_scan_cross<2, 64>; m = 3: 32 markers, k_scan_cross<4, 32>.  The whole scan against the
    oracle, then the |x_a|^2 and the cross-product rows of one full raw block against the half-solve of its d r columns."""
    import torch
    p = TC.cohort("T8K")
    n, d = p["n"], 1 + m
    g = _gxe_problem(m)
    scan = _scan("T8K", block=128, covariates=g["C"])
    gxe = scan.interaction(g["E"])
    assert gxe.block == per_block
    XO.compare(gxe(TC.markers(p)), g["ref"], n, bad=DEGENERATE)
    r, q = per_block, scan.q
    G = TC.markers(p)[2:2 + r]
    Gt = GA._centred(G)[2]
    cols = np.hstack([Gt.T] + [Gt.T * g["E"][:, a:a + 1] for a in range(m)])
    X = _xref(scan, ("gxe", m), cols).reshape(n, d, r)
    dG = _rows_int8(G, torch)
    dS = torch.full((gxe.nrows * r + 8,), -CANARY, dtype=torch.float64, device="cuda")       # (a guard behind the statistics)
    torch.cuda.synchronize()
    scan.factor.scan_block_gxe_dev(vp(dG.data_ptr()), _ld(n), r, vp(gxe.dE.data_ptr()), m, vp(scan.dQ.data_ptr()), q, vp(dS.data_ptr()))
    scan.sym.sync()
    hS = dS.cpu().numpy()
    assert np.all(hS[gxe.nrows * r:] == -CANARY)
    S = hS[:gxe.nrows * r].reshape(gxe.nrows, r)
    _check_moments(S, G, "T8K gxe m %d" % m)
    for a in range(d):
        e = rel_err(S[3 + a], (X[:, a] * X[:, a]).sum(axis=0).astype(np.float64))
        print("m", m, "|x_%d|^2 rel.err %.2e" % (a, e))
        assert e < PROD, a
    row = 3 + (q + 1) * d
    for a in range(d):
        for b in range(a + 1, d):
            e = rel_err(S[row], (X[:, a] * X[:, b]).sum(axis=0).astype(np.float64))
            print("m", m, "x_%d'x_%d rel.err %.2e" % (a, b, e))
            assert e < PROD, (a, b)
            row += 1
    assert row == gxe.nrows


# ---- 7. the BLUP blocks at B64

def _pattern_slots(p, P, ids):
    """The permuted lower-triangle CSC pattern of A + I rebuilt in scipy (diagonal first in a column, rows ascending): the
    slots of the ROW parts of the requested individuals, entries (p_c, j < p_c), which only the streaming pass reaches."""
    B = (p["A"] + p["I"]).tocsr()[P][:, P]
    L = sp.tril(B, format="csc")
    L.sort_indices()
    iperm = np.empty(p["n"], dtype=np.int64)
    iperm[P] = np.arange(p["n"])
    col = np.repeat(np.arange(p["n"]), np.diff(L.indptr))
    hit = np.isin(L.indices, iperm[ids]) & (L.indices != col)
    return L.nnz, np.flatnonzero(hit)


@pytest.mark.parametrize("det", [False, True])
def test_blup_blocks_at_b64_reach_the_strided_slots(det):
    """K = 2 (A and the identity), G = 0.7 A + 0.3 I.  Requested: the 64 individuals that are last in P() and the first and the
    last individual of the original order.  On the deterministic handle the same columns through scilmm_rows_block_dev give the
    same bits, and no launch sums with floating-point atomics."""
    import torch
    p = TC.cohort("B64")
    n = p["n"]
    scan = _scan("B64", 4, 128, det=det)
    fac, q = scan.factor, scan.q
    P = fac.P()
    ids = np.array(list(dict.fromkeys([int(i) for i in P[-64:]] + [0, n - 1])), dtype=np.int32)
    r = ids.size
    nnz, slots = _pattern_slots(p, P, ids)
    K = TC.kernel_constants()
    assert nnz == 257 * 64 * 65 // 2 and slots.size > 0 and slots.max() >= 256 * K["REL_GRID"], (nnz, slots.max())
    print("B64 det", det, "requests", r, "row-part slots", slots.size, "of them at or past 256 * REL_GRID:",
          int((slots >= 256 * K["REL_GRID"]).sum()))
    w = np.array([0.7, 0.3])
    Gm = (w[0] * p["A"] + w[1] * p["I"]).tocsr()
    X = _xref(scan, ("rel", det), Gm[:, ids].toarray())
    before = scan.sym.timing()["n_float_atomic_launches"]
    dS = torch.full(((q + 2) * r + 8,), -CANARY, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    fac.rel_block_dev(w, ids, vp(scan.dQ.data_ptr()), q, vp(dS.data_ptr()))
    scan.sym.sync()
    hS = dS.cpu().numpy()
    assert np.all(hS[(q + 2) * r:] == -CANARY)
    S = hS[:(q + 2) * r].reshape(q + 2, r)
    assert np.array_equal(S[0], Gm.diagonal()[ids])
    Q = scan.dQ.cpu().numpy().astype(np.longdouble)
    e_gg, e_qx = rel_err(S[1], (X * X).sum(axis=0).astype(np.float64)), rel_err(S[2:], _dot(Q, X))
    print("B64 det", det, "|x|^2 rel.err %.2e" % e_gg, "Q'x rel.err %.2e" % e_qx)
    assert e_gg < PROD and e_qx < PROD
    if det:
        rows = Gm[ids].tocsr()
        rows.sort_indices()
        d_ptr = torch.from_numpy(rows.indptr.astype(np.int64)).cuda()
        d_idx = torch.from_numpy(rows.indices.astype(np.int32)).cuda()
        d_val = torch.from_numpy(rows.data.astype(np.float64)).cuda()
        dR = torch.full(((q + 2) * r,), -CANARY, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        fac.rows_block_dev(vp(d_ptr.data_ptr()), vp(d_idx.data_ptr()), vp(d_val.data_ptr()), r, vp(scan.dQ.data_ptr()), q, vp(dR.data_ptr()))
        scan.sym.sync()
        R = dR.cpu().numpy().reshape(q + 2, r)
        assert np.all(R[0] == 0.0) and np.array_equal(R[1:], S[1:])
        assert scan.sym.timing()["n_float_atomic_launches"] == before == 0


# ---- 8. DeviceCSR.dot at T65K

@pytest.mark.parametrize("r", [1, 130])
def test_device_csr_dot_at_t65k_strides_over_its_rows(r):
    """65 577 rows on 65 536 waves: the last 41 rows are second trips."""
    import torch
    from scilmm_amd import _lib
    p = TC.cohort("T65K")
    A = p["A"]
    dA = _once("dcsr", lambda: _lib.DeviceCSR(A, torch))
    X = np.random.default_rng(3).standard_normal((p["n"], r))
    Y = dA.dot(torch.from_numpy(X).cuda()).cpu().numpy()
    ref = A @ X
    print("T65K DeviceCSR.dot r", r, "rel.err %.2e" % rel_err(Y, ref), "rows from 65536 on %.2e" % rel_err(Y[65536:], ref[65536:]))
    assert rel_err(Y, ref) < 1e-13 and rel_err(Y[65536:], ref[65536:]) < 1e-13


# ---- 9. the deterministic handle at T8K

def test_deterministic_handle_at_t8k_repeats_its_bits():
    import torch
    p = TC.cohort("T8K")
    n = p["n"]
    scan = _scan("T8K", 4, 128, det=True)
    G = TC.markers(p)
    a, b = scan(G), scan(G)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    GA._compare(a, _oracle("T8K", 4), n)
    Yp = np.random.default_rng(3).standard_normal((n, TMAXT))
    dY = torch.zeros((n, 144), dtype=torch.float64, device="cuda")
    dY[:, :TMAXT] = torch.from_numpy(Yp).cuda()
    runs = []
    for _ in range(2):
        dO = torch.zeros((128, TMAXT), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        S, K = _block(scan, G[2:], torch, gram=True)
        scan.factor.scan_panel_dev(128, vp(dY.data_ptr()), 144, TMAXT, vp(dO.data_ptr()), TMAXT)
        scan.sym.sync()
        runs.append((S, K, dO.cpu().numpy()))
    for x, y in zip(*runs):
        assert np.array_equal(x, y) and np.all(np.isfinite(x))
    assert scan.sym.timing()["n_float_atomic_launches"] == 0
