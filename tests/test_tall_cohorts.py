"""Host-only companion of tests/test_gpu_blocks_tall.py: the facts about its three cohorts that put the GPU cases on the
edges of the block kernels, asserted from the constants in csrc/ (`tall_cohorts.kernel_constants`) and the run rule of the
fold kernels (`tall_cohorts.fold_runs`) -- a later change of a slice, a fold width or a grid cap fails here by name -- and
what the GPU tolerances rest on, on the CPU:

  * the whitened GLS (the scan's host algebra on a block-wise Cholesky whitening in numpy) against the un-whitened oracle of
    tests/test_gpu_assoc.py with the block-wise inverse.  Bound 1e-11, two decades inside the 1e-9 the GPU cases hold;
    measured (max-norm over the 128 non-degenerate markers, c = 4): T8K beta 6.4e-14, se 4.5e-14, chi2 3.0e-14; T65K beta
    4.2e-13, se 2.4e-13, chi2 2.7e-13 (tests/test_gpu_assoc.py states 3e-15 at n <= 1502).
  * a plain fp64 X'Y against the np.longdouble product at n = 65 577, standard normal inputs: bound 1e-12 (what the GPU cases
    hold for Gram, panel, keep and cross products); measured 1.0e-15."""
import numpy as np
import pytest
import scipy.linalg as la

from tests import tall_cohorts as TC
from tests import test_gpu_assoc as GA
from tests.helpers import rel_err


@pytest.fixture(scope="module", autouse=True)
def _release_the_cohorts():
    yield
    TC.release()


K = TC.kernel_constants()


def _ceil(a, b):
    return (a + b - 1) // b


def test_the_library_is_built_with_the_slices_of_the_headers():
    assert K["MAKE_GRAM_SLICE"] == K["GRAM_SLICE"] and K["MAKE_PANEL_SLICE"] == K["PANEL_SLICE"]


def test_the_cohorts_are_what_they_say():
    for cid, (nblocks, nnz) in (("T8K", (227 * 8 + 7, 227 * 204 + 91 + 36)), ("B64", (257, 257 * 64 * 64))):
        # (T8K: 227 cycles of 1..8 = 36 individuals and 204 entries each, then 1..6 and a family of 8 truncated to 6)
        p = TC.cohort(cid)
        A, n = p["A"], p["n"]
        assert A.shape == (n, n) and A.has_sorted_indices and len(p["blocks"]) == nblocks and A.nnz == nnz
        assert sum(len(b) for b in p["blocks"]) == n
        assert np.all(np.diff(A.indptr) == np.repeat([len(b) for b in p["blocks"]], [len(b) for b in p["blocks"]]))
        assert (abs(A - A.T)).nnz == 0 and np.all(A.diagonal() == 1.0)
        V = (TC.S2[0] * A + TC.S2[1] * p["I"]).tocsr()
        R = (V @ TC.inverse(p) - p["I"]).tocsr()
        assert abs(R).max() < 1e-14                                  # the block-wise inverse is the inverse
    assert TC.COHORTS["T8K"]["n"] == 4 * 2048 + 7 and TC.COHORTS["T8K"]["n"] % 16 == 7 and TC.COHORTS["T8K"]["n"] % 4 == 3
    assert TC.COHORTS["T65K"]["n"] == 65536 + 41 and TC.COHORTS["B64"]["n"] == 257 * 64
    assert TC.family_sizes(40, (1, 2, 3)).tolist() == [1, 2, 3] * 6 + [1, 2, 1]     # cycled, the last block truncated


@pytest.mark.parametrize("kernel,slice_,fold,runs", [
    ("k_scan_fold", "SCAN_SLICE", "SCAN_FOLD", [5, 5, 5, 5, 5, 5, 3, 0]),
    ("k_gram_fold", "GRAM_SLICE", "GRAM_FOLD", [5, 5, 5, 2]),
    ("k_panel_fold", "PANEL_SLICE", "PANEL_FOLD", [2, 2, 1, 0]),
])
def test_t8k_gives_every_fold_a_full_a_ragged_and_an_empty_run(kernel, slice_, fold, runs):
    """(17 Gram slices in four runs of five leave k_gram_fold no empty run at T8K: 5, 5, 5, 2.  Its empty run is the one case
    the small cohorts of the suite do reach -- three slices at n = 1502, the fourth run starts past them.)"""
    n = TC.COHORTS["T8K"]["n"]
    nslice = _ceil(n, K[slice_])
    got = TC.run_lengths(nslice, K[fold])
    assert got == runs, (kernel, nslice, got)
    assert sum(got) == nslice
    full = max(got)
    assert full >= 2 and any(0 < g < full for g in got), kernel       # a run of two or more slices and a shorter one
    if kernel == "k_gram_fold":
        assert TC.run_lengths(_ceil(1502, K[slice_]), K[fold]) == [1, 1, 1, 0]
    else:
        assert 0 in got, kernel                                        # ... and a run that starts past the last slice
    for (s0, s1), g in zip(TC.fold_runs(nslice, K[fold]), got):
        assert s1 <= nslice and (s1 - s0 == g or (g == 0 and s0 >= s1))


def test_the_smaller_cohorts_of_the_suite_never_leave_single_slice_runs():
    """Why the tall cohorts are needed: at n = 1502 every run of every fold is 0 or 1 slice long."""
    for slice_, fold in (("SCAN_SLICE", "SCAN_FOLD"), ("GRAM_SLICE", "GRAM_FOLD"), ("PANEL_SLICE", "PANEL_FOLD")):
        assert max(TC.run_lengths(_ceil(1502, K[slice_]), K[fold])) == 1
    assert max(TC.run_lengths(_ceil(4103, K["PANEL_SLICE"]), K["PANEL_FOLD"])) == 1


def test_t65k_folds():
    """Not what T65K is for, but what its folds see: 257 scan slices (seven runs of 33 and one of 26), 129 Gram slices, 33
    panel slices."""
    n = TC.COHORTS["T65K"]["n"]
    assert TC.run_lengths(_ceil(n, K["SCAN_SLICE"]), K["SCAN_FOLD"]) == [33] * 7 + [26]
    assert TC.run_lengths(_ceil(n, K["GRAM_SLICE"]), K["GRAM_FOLD"]) == [33, 33, 33, 30]
    assert TC.run_lengths(_ceil(n, K["PANEL_SLICE"]), K["PANEL_FOLD"]) == [9, 9, 9, 6]


def test_moments_take_several_trips():
    """k_scan_moments: 256 threads, one 16-byte piece each per trip; the piece count allows for 15 bytes of misalignment.
    The siblings: k_bed_moments (identity: 16-byte pieces of 64 samples; mapped: BED_FLIGHT individuals per thread and trip),
    k_dos_moments (identity: DOS_PIECES pieces per thread and trip, 8 or 4 elements a piece; mapped: DOS_FLIGHT)."""
    n8, n65 = TC.COHORTS["T8K"]["n"], TC.COHORTS["T65K"]["n"]
    assert _ceil(15 + n8, 16) > 256 and _ceil(_ceil(n8, 16), 256) == 3
    assert _ceil(_ceil(n65, 16), 256) == 17
    assert _ceil(_ceil(_ceil(n65, 4), 16), 256) == 5                       # .bed, identity map
    assert _ceil(n65, K["BED_FLIGHT"] * 256) == 33                         # .bed, sample map
    assert _ceil(_ceil(n65, 8), K["DOS_PIECES"] * 256) == 9                # uint16 dosages, identity map
    assert _ceil(_ceil(n65, 4), K["DOS_PIECES"] * 256) == 17               # float32 dosages, identity map
    assert _ceil(n65, K["DOS_FLIGHT"] * 256) == 33                         # dosages, sample map
    # n = 1502 does all of this in one trip
    assert _ceil(15 + 1502, 16) <= 256 and 1502 <= K["BED_FLIGHT"] * 256 and 1502 <= K["DOS_FLIGHT"] * 256


def test_t65k_wraps_the_capped_grids():
    n = TC.COHORTS["T65K"]["n"]
    chunks = _ceil(n, K["KEEP_ROWS"])
    assert chunks > K["KEEP_GRID"] and (chunks, K["KEEP_GRID"]) == (2050, 2048)      # two workgroups take a second chunk
    assert n - (chunks - 1) * K["KEEP_ROWS"] == 9                                   # ... the last of them a ragged one
    assert n > 4 * K["SPMM_GRID"] and K["SPMM_GRID"] == 256 * 64                    # a wave per row, four waves a workgroup
    assert 1502 <= K["KEEP_ROWS"] * K["KEEP_GRID"] and 1502 <= 4 * K["SPMM_GRID"]


def test_b64_wraps_the_row_pass_of_k_rel_gather():
    p = TC.cohort("B64")
    slots = sum(len(b) * (len(b) + 1) // 2 for b in p["blocks"])
    assert slots == 257 * 64 * 65 // 2 == 534560 and slots > 256 * K["REL_GRID"]
    assert (p["A"].nnz + p["n"]) // 2 == slots                        # the lower triangle of A, diagonal included


def _whitened_gls(p, c, G):
    """The scan's algebra (scilmm_amd.assoc: R'R = w(C)'w(C), u = R^-T w(C)'w(y), a = |x|^2 - |z|^2, b = w(y)'x - u'z) on a
    block-wise Cholesky whitening in numpy."""
    Li = TC.block_whitener(p["blocks"], *TC.S2)
    wC, wy = Li @ p["C"][:, :c], Li @ p["y"]
    _, _, Gt = GA._centred(G)
    X = Li @ Gt.T
    R = la.cholesky(wC.T @ wC, lower=False)
    u = la.solve_triangular(R, wC.T @ wy, trans="T", lower=False)
    z = la.solve_triangular(R, wC.T @ X, trans="T", lower=False)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = (X * X).sum(axis=0) - (z * z).sum(axis=0)
        b = wy @ X - u @ z
        return dict(beta=b / a, se=1.0 / np.sqrt(a), chi2=b * b / a)


@pytest.mark.parametrize("cid", ["T8K", "T65K"])
def test_whitened_and_unwhitened_gls_agree(cid):
    p = TC.cohort(cid)
    TC.inverse(p)
    G = TC.markers(p)
    ref = GA._oracle(p, TC.S2, 4, G)
    out = _whitened_gls(p, 4, G)
    ok = np.ones(TC.M, bool)
    ok[[GA.MONO, GA.ALLMISS]] = False
    assert np.array_equal(np.isnan(ref["beta"]), ~ok)
    for k in ("beta", "se", "chi2"):
        print(cid, k, "whitened vs un-whitened", rel_err(out[k][ok], ref[k][ok]))
        assert rel_err(out[k][ok], ref[k][ok]) < 1e-11, k


def test_fp64_products_at_65k_are_good_to_1e_12():
    n = TC.COHORTS["T65K"]["n"]
    rng = np.random.default_rng(5)
    X, Y = rng.standard_normal((n, 8)), rng.standard_normal((n, 9))
    ref = np.einsum("ni,nj->ij", X.astype(np.longdouble), Y.astype(np.longdouble))
    err = rel_err((X.T @ Y), ref.astype(np.float64))
    exact = float(np.abs(X.T @ Y - ref).max() / np.abs(ref).max())
    print("fp64 X'Y vs longdouble at n = %d: %.2e (%.2e before rounding the reference)" % (n, err, exact))
    assert err < 1e-12 and exact < 1e-12
