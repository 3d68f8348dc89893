"""The variant-set tests' surface without a device: exports, the checks of sets / weights / method, the greedy packing, the
test_bed argument paths that fail before any device call, and the two mixture tail functions.

Mixture functions, as measured on the CPU with this implementation (Brent root; inside the seam of 0.05 standard deviations
around the mean the saddlepoint function is Liu's, scaled to meet the saddlepoint values at the seam's two ends):
  equal lam (an exact scaled chi2_r), r = 1, 5, 20, 128, q / lam = r + {-0.5, 0, 1, 3, 10, 30} sqrt(2 r) where positive, and
  q = 30 lam at r = 1, at lam = 1, 3.7e-4 and 2.5e6: mixture_sf_liu against chi2.sf <= 8.6e-14 relative (bound 1e-10), p down
  to 1.6e-63; mixture_sf_saddlepoint within 0.0452 in log10 p (worst r = 1, q = 30 lam; bound 0.06), within 0.0081 for r >= 5
  (worst at the mean of r = 5; 0.003 away from it).
  unequal lam, r = 2, 7, 33, fixed-seed simulation of 2e6 draws: saddlepoint at the simulated 0.9 and 0.99 quantiles within
  5.6 % relative of 0.1 and 0.01 (bound 10 %; the simulation's own standard error at 0.01 is 0.7 %)."""
import ctypes as C

import numpy as np
import pytest
import scipy.stats as stats

from scilmm_amd import _lib


def test_exports():
    import scilmm_amd
    from scilmm_amd import sets
    from scilmm_amd.assoc import AssociationScan
    from scilmm_amd.factor import Factor
    assert scilmm_amd.VariantSetTest is sets.VariantSetTest and issubclass(sets.VariantSetTest, AssociationScan)
    for name in ("scan_block_gram_dev", "scan_block_bed_gram_dev"):
        assert callable(getattr(Factor, name)), name
    L = _lib.lib()
    for name in ("scilmm_scan_block_gram_dev", "scilmm_scan_block_bed_gram_dev"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert callable(sets.mixture_sf_saddlepoint) and callable(sets.mixture_sf_liu)


def test_entry_points_check_their_arguments_first():
    """Dummy non-null pointers: the argument checks come before any dereference; a null d_gram is an argument error."""
    L = _lib.lib()
    one = C.c_void_p(8)
    f, g = L.scilmm_scan_block_gram_dev, L.scilmm_scan_block_bed_gram_dev
    assert f(one, one, 64, 4, one, 2, one, None) == _lib.ERR_ARG
    assert g(one, one, 16, 64, None, 0, 4, one, 2, one, None) == _lib.ERR_ARG
    for r, q in ((0, 2), (129, 2), (-1, 2), (4, 0), (4, 33)):
        assert f(one, one, 64, r, one, q, one, one) == _lib.ERR_ARG, (r, q)
        assert g(one, one, 16, 64, one, 0, r, one, q, one, one) == _lib.ERR_ARG, (r, q)
    for args in ((None, one, 64, 4, one, 2, one, one), (one, None, 64, 4, one, 2, one, one), (one, one, 64, 4, None, 2, one, one),
                 (one, one, 64, 4, one, 2, None, one)):
        assert f(*args) == _lib.ERR_ARG
    for args in ((None, one, 16, 64, one, 0, 4, one, 2, one, one), (one, None, 16, 64, one, 0, 4, one, 2, one, one),
                 (one, one, 16, 64, one, 0, 4, None, 2, one, one), (one, one, 16, 64, one, 0, 4, one, 2, None, one),
                 (one, one, 16, 0, one, 0, 4, one, 2, one, one), (one, one, 15, 64, one, 0, 4, one, 2, one, one),
                 (one, one, 16, 64, one, 2, 4, one, 2, one, one)):
        assert g(*args) == _lib.ERR_ARG


def test_check_sets():
    from scilmm_amd.sets import check_sets
    out = check_sets([[3], np.array([0, 9, 4]), np.arange(8, dtype=np.int32)], 10, 8)
    assert [s.tolist() for s in out] == [[3], [0, 9, 4], list(range(8))] and all(s.dtype == np.int64 for s in out)
    assert check_sets([], 10, 8) == []
    with pytest.raises(ValueError, match="twice"):
        check_sets([[1, 2, 1]], 10, 8)
    for bad in ([[10]], [[-1]], [[0, 11]]):
        with pytest.raises(ValueError, match="outside"):
            check_sets(bad, 10, 8)
    with pytest.raises(ValueError, match="more than one device block of 8"):
        check_sets([[0, 1], list(range(9))], 10, 8)
    for bad in ([[]], [[0.0, 1.0]], [[[0, 1]]], [3], np.arange(4)):
        with pytest.raises(ValueError):
            check_sets(bad, 10, 8)


def test_check_weights_and_method():
    from scilmm_amd.sets import check_method, check_weights, mixture_sf_liu, mixture_sf_saddlepoint
    sets = [np.array([0, 1]), np.array([2])]
    assert check_weights("beta", sets) == "beta" and check_weights(None, sets) is None
    w = check_weights([[1, 2], [0.5]], sets)
    assert [x.tolist() for x in w] == [[1.0, 2.0], [0.5]] and all(x.dtype == np.float64 for x in w)
    for bad in ("flat", [[1, 2]], [[1, 2], [1, 2]], [[1, np.nan], [1]], [[1, np.inf], [1]]):
        with pytest.raises(ValueError):
            check_weights(bad, sets)
    assert check_method("saddlepoint") is mixture_sf_saddlepoint and check_method("liu") is mixture_sf_liu
    for bad in ("davies", None, "Liu"):
        with pytest.raises(ValueError, match="method"):
            check_method(bad)


def test_greedy_packing():
    from scilmm_amd.sets import pack_sets
    sizes = [1, 2, 16, 17, 100, 28, 29, 128]
    assert pack_sets(sizes, 128) == [[0, 1, 2, 3], [4, 5], [6], [7]]          # 100 + 28 fill a block exactly; 29 opens the next
    assert pack_sets(sizes[:4], 17) == [[0, 1], [2], [3]]
    assert pack_sets([4, 4, 4], 8) == [[0, 1], [2]]
    assert pack_sets([8, 1, 8], 8) == [[0], [1], [2]]                           # in the order given: no look-ahead
    assert pack_sets([], 8) == []
    for sizes, block in (([9], 8), ([1, 0], 8), ([129], 128)):
        with pytest.raises(ValueError):
            pack_sets(sizes, block)
    rng = np.random.default_rng(0)
    for block in (16, 112, 128):
        sizes = rng.integers(1, block + 1, 200).tolist()
        blocks = pack_sets(sizes, block)
        assert [i for b in blocks for i in b] == list(range(200))                 # every set once, in order
        tot = [sum(sizes[i] for i in b) for b in blocks]
        assert max(tot) <= block
        assert all(tot[k] + sizes[blocks[k + 1][0]] > block for k in range(len(blocks) - 1))   # a block closes only when full


CASES = [(r, x) for r in (1, 5, 20, 128) for x in (-0.5, 0.0, 1.0, 3.0, 10.0, 30.0)] + [(1, None)]


def _q_over_lam(r, x):
    return 30.0 if x is None else r + x * np.sqrt(2.0 * r)


@pytest.mark.parametrize("lam0", [1.0, 3.7e-4, 2.5e6])
def test_equal_lambda_is_an_exact_scaled_chi2(lam0):
    from scilmm_amd.sets import mixture_sf_liu, mixture_sf_saddlepoint
    worst_liu, worst_sp, worst_sp5, pmin = 0.0, 0.0, 0.0, 1.0
    for r, x in CASES:
        t = _q_over_lam(r, x)
        if t <= 0:
            continue
        lam, q = np.full(r, lam0), t * lam0
        ref = stats.chi2.sf(t, r)
        pmin = min(pmin, ref)
        liu, sp = mixture_sf_liu(q, lam), mixture_sf_saddlepoint(q, lam)
        assert ref > 0 and np.isfinite(liu) and np.isfinite(sp) and sp > 0, (r, x)
        worst_liu = max(worst_liu, abs(liu - ref) / ref)
        d = abs(np.log10(sp) - np.log10(ref))
        worst_sp = max(worst_sp, d)
        if r >= 5:
            worst_sp5 = max(worst_sp5, d)
    print("liu rel.err", worst_liu, "saddlepoint |dlog10 p|", worst_sp, "(r >= 5:", worst_sp5, ") smallest p", pmin)
    assert pmin < 1e-30
    assert worst_liu < 1e-10
    assert worst_sp < 0.06


def _unequal(r):
    return np.random.default_rng(100 + r).uniform(0.05, 1.0, r) ** 2 * (1.0 + 4.0 * (np.arange(r) == 0))


@pytest.mark.parametrize("r", [1, 2, 7, 33, 128])
def test_both_decrease_in_q_across_the_mean(r):
    """A grid of 0.01 standard deviations across the seam at mean +- 0.05 sd, a coarser one out to the tails.  Inside the
    seam the saddlepoint function is Liu's times a factor interpolated between the seam's ends, which is what makes it
    continuous there: a bare switch steps up by 1.2 % at the upper end for r = 2 (measured), more than p falls in 0.01 sd."""
    from scilmm_amd.sets import mixture_sf_liu, mixture_sf_saddlepoint
    for lam in (np.ones(r), _unequal(r)):
        mu, sd = lam.sum(), np.sqrt(2 * np.sum(lam ** 2))
        x = np.unique(np.r_[np.linspace(-0.2, 0.2, 41), np.linspace(-3, 12, 61)])
        q = mu + x * sd
        q = q[q > 0]
        for f in (mixture_sf_saddlepoint, mixture_sf_liu):
            p = np.array([f(v, lam) for v in q])
            assert np.all((p > 0) & (p <= 1)), f.__name__
            d, sat = np.diff(p), p[:-1] > 1.0 - 1e-9          # (far below the mean 1 - p is lost in the rounding of p: flat there)
            assert np.all(d <= 0) and np.all(d[~sat] < 0), (f.__name__, r, q[:-1][~sat][d[~sat] >= 0])
    assert mixture_sf_saddlepoint(0.0, lam) == 1.0 and mixture_sf_saddlepoint(-1.0, lam) == 1.0
    assert np.isnan(mixture_sf_saddlepoint(np.nan, lam)) and np.isnan(mixture_sf_liu(np.nan, lam))


@pytest.mark.parametrize("r", [2, 7, 33])
def test_saddlepoint_against_simulation(r):
    from scilmm_amd.sets import mixture_sf_saddlepoint
    lam = _unequal(r)
    rng = np.random.default_rng(r)
    draws = np.zeros(2_000_000)
    for l in lam:
        draws += l * rng.chisquare(1, draws.size)
    for tail in (0.1, 0.01):
        q = np.quantile(draws, 1.0 - tail)
        p = mixture_sf_saddlepoint(q, lam)
        print("r", r, "tail", tail, "saddlepoint", p, "rel.dev", abs(p - tail) / tail)
        assert abs(p - tail) / tail < 0.10


def test_test_bed_argument_paths_before_any_device_call(tmp_path):
    """The checks of test_bed run on an object that was never constructed: none of them may touch the device."""
    from tests import test_bed_api as T
    from scilmm_amd.sets import VariantSetTest
    n, m = 21, 6
    G = np.random.default_rng(0).integers(0, 3, (m, n)).astype(np.int8)
    path = T.write_fileset(tmp_path / "s", T.pack(G), n)
    t = object.__new__(VariantSetTest)
    t.n, t.block = n, 4
    sets = [[0, 1], [5]]
    with pytest.raises(ValueError):
        t.test_bed(path, sets, count="a1")
    with pytest.raises(ValueError, match="sample_index"):
        t.test_bed(path, sets, sample_index=np.arange(n - 1))
    with pytest.raises(ValueError, match="sample_index"):
        t.test_bed(path, sets, sample_index=np.where(np.arange(n) == 3, n, np.arange(n)))
    t.n = n + 1
    with pytest.raises(ValueError, match="give a sample_index"):
        t.test_bed(path, sets)
    t.n = n
    with pytest.raises(ValueError, match="outside"):
        t.test_bed(path, [[0, m]])
    with pytest.raises(ValueError, match="twice"):
        t.test_bed(path, [[2, 2]])
    with pytest.raises(ValueError, match="more than one device block of 4"):
        t.test_bed(path, [[0, 1, 2, 3, 4]])
    with pytest.raises(ValueError, match="method"):
        t.test_bed(path, sets, method="davies")
    with pytest.raises(ValueError):
        t.test_bed(path, sets, weights=[[1.0, 1.0]])
    with pytest.raises(ValueError, match="chunk_bytes"):
        t.test_bed(path, sets, chunk_bytes=0)
    with pytest.raises(TypeError):
        t(G.astype(np.float64), sets)
    with pytest.raises(ValueError, match="outside"):
        t(G, [[m]])
