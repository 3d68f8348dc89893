"""The masked set test's surface without a device (scilmm_amd.set_masks): exports, ``acat`` against its closed form, the host
``acatv`` and its pooling rule, cell membership, the packing of annotation words, the argument checks of the C entry point and of
the Python layer, and ``VariantSetTest`` left as it was.

Tolerances.  ``acat`` of one p is p up to the rounding of tan and atan on a well-conditioned argument (1e-13 relative asked).  A
symmetric pair p, 1 - p cancels to T = 0 up to the rounding of 1 - p itself (half an ulp of 1, 1.1e-16), which the tangent's
slope pi / sin^2(p pi) carries into T / 2 and atan / pi into the result: |acat - 0.5| <= 1.1e-16 / (2 sin^2(p pi)) plus a few
ulps of the terms' own rounding; 2e-16 / sin^2(p pi) + 1e-15 asked.  Across the branch at p = 1e-15 the two forms 1 / (p pi)
and 1 / tan(p pi) differ by (p pi)^2 / 3 ~ 3e-30 relative and the two arguments by one ulp: 1e-10 relative asked."""
import ctypes as C
import inspect

import numpy as np
import pytest
import scipy.special as special
import scipy.stats as stats

from scilmm_amd import _lib

RHO = np.array([0.0, 0.5, 1.0])


def test_exports():
    import scilmm_amd
    from scilmm_amd import set_masks, sets
    from scilmm_amd.factor import Factor, Symbolic
    assert scilmm_amd.MaskedSetTest is set_masks.MaskedSetTest and scilmm_amd.acat is set_masks.acat
    assert callable(sets.VariantSetTest.masks) and callable(set_masks.acatv)
    assert callable(Factor.sets_finish_masks_dev) and callable(Symbolic.sets_finish_masks_timing)
    L = _lib.lib()
    for name in ("scilmm_sets_finish_masks_dev", "scilmm_sets_finish_masks_timing"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert set_masks.CELL_KEYS == sets.KEYS + ("acatv_p", "n_pooled")


def test_acat_against_the_closed_form():
    from scilmm_amd.set_masks import acat
    for p in (1e-300, 1e-40, 1e-17, 1e-15, 1e-12, 1e-6, 0.01, 0.3, 0.4999, 0.5, 0.7, 0.99):
        assert abs(acat([p]) - p) <= 1e-13 * p, p                           # a single p returns itself
    assert acat(np.array([0.2])).shape == ()
    for p in (1e-3, 0.05, 0.2, 0.4, 0.5):
        assert abs(acat([p, 1.0 - p]) - 0.5) < 2e-16 / np.sin(p * np.pi) ** 2 + 1e-15, p     # symmetric pairs
    # the closed form on moderate p-values, with and without weights, along either axis
    rng = np.random.default_rng(0)
    P, W = rng.uniform(0.01, 0.95, (4, 6)), rng.uniform(0.1, 2.0, (4, 6))
    closed = lambda p, w, ax: 0.5 - np.arctan(np.sum(w * np.tan((0.5 - p) * np.pi), axis=ax) / np.sum(w, axis=ax)) / np.pi
    assert np.allclose(acat(P), closed(P, np.ones_like(P), -1), rtol=1e-12, atol=0)
    assert np.allclose(acat(P, W, axis=0), closed(P, W, 0), rtol=1e-12, atol=0)
    assert np.allclose(acat(P, W[0], axis=1), closed(P, W[:1], 1), rtol=1e-12, atol=0)
    # the small-p branch is continuous at 1e-15, alone and next to another term
    lo, hi = np.nextafter(1e-15, 0.0), 1e-15
    for rest in ([], [0.3], [0.3, 0.9]):
        a, b = acat([lo] + rest), acat([hi] + rest)
        assert a > 0 and abs(a - b) <= 1e-10 * b, (rest, a, b)
    # ... and the large-T branch at 1e15 (T = 1 / (p pi) crosses it at p = 3.2e-16)
    for p in (3.1e-16, 3.3e-16):
        assert abs(acat([p]) - p) <= 1e-13 * p
    assert acat([0.0]) == 0.0 and acat([0.0, 0.5, 0.99]) == 0.0             # p = 0 gives 0
    assert acat([1.0]) > 0.99                                               # capped at 1 - 1e-15: finite
    # NaN and weight 0 are skipped; nothing left: NaN
    assert acat([0.2, np.nan, 0.4]) == acat([0.2, 0.4]) and acat([0.2, 0.4], [1.0, 0.0]) == acat([0.2])
    assert np.isnan(acat([np.nan, np.nan])) and np.isnan(acat([])) and np.isnan(acat([0.3], [0.0]))
    got = acat(np.array([[0.1, np.nan], [np.nan, np.nan]]), axis=1)
    assert abs(got[0] - 0.1) < 1e-14 and np.isnan(got[1])
    for bad in ([-0.1], [1.5]):
        with pytest.raises(ValueError, match="p-value"):
            acat(bad)
    for bad in ([-1.0], [np.inf], [np.nan]):
        with pytest.raises(ValueError, match="weights"):
            acat([0.5], bad)


def _cell(rng, k):
    Z = rng.standard_normal((k + 6, k)) * rng.uniform(0.3, 1.7, k)
    K = Z.T @ Z
    return rng.uniform(1.0, 3.0, k) * np.sqrt(np.diag(K)), K, rng.uniform(0.5, 2.0, k)


def test_host_acatv_and_its_pooling_rule():
    from scilmm_amd.set_masks import acat, acatv
    rng = np.random.default_rng(1)
    s, K, w = _cell(rng, 6)
    n_obs = np.full(6, 80.0)
    maf = np.array([0.0625, 0.2, 0.01, 0.3, 0.05, 0.0626])                  # mac = 10 exactly | 32 | 1.6 | 48 | 8 | 10.016
    om = w * w * maf * (1 - maf)
    marg = special.erfc(np.sqrt(0.5 * s * s / np.diag(K)))
    # nothing pooled: the Cauchy combination of the marginal tests
    p, n_pooled = acatv(s, K, w, maf, n_obs, 0.0)
    assert n_pooled == 0 and p == acat(marg, om)
    # mac <= acat_mac is pooled (the boundary included): markers 0, 2, 4 become one burden term with the mean of their weights
    p, n_pooled = acatv(s, K, w, maf, n_obs, 10.0)
    pool = np.array([0, 2, 4])
    wp = w[pool]
    pb = special.erfc(np.sqrt(0.5 * (wp @ s[pool]) ** 2 / (wp @ K[np.ix_(pool, pool)] @ wp)))
    own = np.array([1, 3, 5])
    want = acat(np.r_[marg[own], pb], np.r_[om[own], om[pool].mean()])
    assert n_pooled == 3 and abs(p - want) <= 1e-14 * want
    # everything pooled: the burden term alone
    p, n_pooled = acatv(s, K, w, maf, n_obs, 1e6)
    pb = special.erfc(np.sqrt(0.5 * (w @ s) ** 2 / (w @ K @ w)))
    assert n_pooled == 6 and abs(p - pb) <= 1e-13 * pb
    # a pool whose quadratic form is not positive is left out, and still counted
    K0 = K.copy()
    K0[np.ix_(pool, pool)] = 0.0
    p, n_pooled = acatv(s, K0, w, maf, n_obs, 10.0)
    assert n_pooled == 3 and p == acat(marg[own], om[own])
    # K_jj = 0 and w_j = 0 leave a marker out; without a term: NaN
    K1, w1 = K.copy(), w.copy()
    K1[1, 1], w1[3] = 0.0, 0.0
    p, n_pooled = acatv(s, K1, w1, maf, n_obs, 0.0)
    keep = np.array([0, 2, 4, 5])
    assert n_pooled == 0 and p == acat(marg[keep], om[keep])
    assert np.isnan(acatv(s[:1], np.zeros((1, 1)), w[:1], maf[:1], n_obs[:1], 0.0)[0])
    assert acatv(s[:1], np.zeros((1, 1)), w[:1], maf[:1], n_obs[:1], 1e6) [1] == 1
    # a strong marker: the 1 / (p pi) branch, and the p-value of one term is the term's
    s9 = s.copy()
    s9[1] = 9.0 * np.sqrt(K[1, 1])
    p, _ = acatv(s9, K, w, maf, n_obs, 0.0)
    assert special.erfc(9.0 / np.sqrt(2.0)) < 1e-15 and 0 < p < 1e-17


def test_cell_membership():
    from scilmm_amd.set_masks import cell_members, maf_of, pack_words
    St = np.zeros((8, 7))
    St[0], St[2] = 100.0, 1.0
    St[1] = [0.02, 0.2, 1.98, 0.01, np.nextafter(0.02, 1.0), 0.02, 0.02]
    St[0, 5], St[2, 6] = 0.0, 0.0                                           # nothing observed | no variation
    ann = np.ones((7, 2), dtype=bool)
    ann[1, 1] = ann[2, 1] = False
    words = pack_words(ann)
    assert maf_of(0.02) == 0.01 and maf_of(1.98) == 1.0 - 0.99
    # maf == cut is in, one ulp above is out; the dropped markers are in no cell
    assert cell_members(St, words, 0, 0.01).tolist() == [True, False, False, True, False, False, False]
    assert cell_members(St, words, 0, 0.5).tolist() == [True, True, True, True, True, False, False]
    assert cell_members(St, words, 0, 1.0 - 0.99).tolist() == [True, False, True, True, True, False, False]
    assert cell_members(St, words, 1, 0.5).tolist() == [True, False, False, True, True, False, False]


def test_packing_of_annotation_words():
    from scilmm_amd import set_masks as M
    B = np.zeros((3, 32), dtype=bool)
    B[0, 0] = B[1, 31] = B[2, 5] = B[2, 31] = True
    w = M.pack_words(B)
    assert w.dtype == np.uint32 and w.tolist() == [1, 2 ** 31, 2 ** 31 + 32]
    assert M.pack_words(np.ones((2, 3), dtype=bool)).tolist() == [7, 7]
    rng = np.random.default_rng(2)
    ann = rng.random((20, 3)) < 0.5
    sets = [np.array([3, 1, 7]), np.array([19]), np.array([7, 0])]
    form, a = M.check_annotations(ann)
    glob = M.set_words(form, a, sets, 20)
    form2, per = M.check_annotations([ann[s] for s in sets])
    assert form == "global" and form2 == "per_set"
    assert all(np.array_equal(x, y) and x.dtype == np.uint32 for x, y in zip(glob, M.set_words(form2, per, sets, 20)))
    assert glob[0].tolist() == [int(sum(int(ann[j, b]) << b for b in range(3))) for j in (3, 1, 7)]
    with pytest.raises(ValueError, match="rows"):
        M.set_words(form, a, sets, 21)
    with pytest.raises(ValueError, match="annotation arrays"):
        M.set_words(form2, per[:2], sets, 20)
    with pytest.raises(ValueError, match="rows"):
        M.set_words(form2, [per[0], per[1], per[2][:1]], sets, 20)


class _Src(object):
    m = 20


def _hollow(cls):
    """A tester without a device: what the checks and the host algebra read of it."""
    t = object.__new__(cls)
    t.block, t.R, t.u, t._f = 8, np.triu(np.ones((2, 2))) + np.eye(2), np.array([0.3, -0.2]), stats.f(1, 99)
    return t


def test_refusals_and_argument_errors():
    from scilmm_amd import MaskedSetTest, glmm, set_masks as M, sets
    from scilmm_amd.set_panel import SetTraitPanel
    tester = _hollow(sets.VariantSetTest)
    ann = np.ones((20, 2), dtype=bool)
    masked = tester.masks(ann, max_maf=(0.5, 0.01), acat_mac=10)
    assert isinstance(masked, MaskedSetTest) and (masked.A, masked.F, masked.acat_mac) == (2, 2, 10.0) and masked.cut.tolist() == [0.5, 0.01]
    some = [np.arange(3)]
    run = lambda **kw: masked._run(_Src(), some, kw.pop("weights", "beta"), kw.pop("method", "saddlepoint"), kw.pop("skato", False),
                                   kw.pop("rho", None), kw.pop("finish", "device"), kw.pop("combine", M.COMBINE_DEFAULT),
                                   kw.pop("return_kernel", False))
    with pytest.raises(ValueError, match="wide"):
        run(finish="wide")
    with pytest.raises(ValueError, match="finish"):
        run(finish="gpu")
    with pytest.raises(ValueError, match="return_kernel"):
        run(return_kernel=True)
    with pytest.raises(ValueError, match="skato=True"):
        run(combine=("burden", "skato"))
    for bad in ((), ("burden", "burden"), ("davies",)):
        with pytest.raises(ValueError, match="combine"):
            run(combine=bad)
    with pytest.raises(ValueError, match="more than one device block"):
        masked._run(_Src(), [np.arange(9)], "beta", "saddlepoint", False, None, "device", M.COMBINE_DEFAULT, False)
    with pytest.raises(ValueError, match="rows"):
        tester.masks(np.ones((19, 2), dtype=bool))._run(_Src(), some, "beta", "saddlepoint", False, None, "device", M.COMBINE_DEFAULT, False)
    # the keywords of VariantSetTest that masks do not take, on every entry; an unknown one is a TypeError
    for call in (masked, masked.test_bed, masked.test_dosages):
        with pytest.raises(ValueError, match="max_markers"):
            call(None, some, max_markers=256)
        with pytest.raises(ValueError, match="set_traits"):
            call(None, some, set_traits=np.zeros((5, 2)))
        with pytest.raises(TypeError, match="reduce"):
            call(None, some, reduce="max")
    with pytest.raises(ValueError, match="set_traits"):
        masked.set_traits(np.zeros((5, 2)))
    # a binary-trait tester and a set panel have no masks
    for cls in (glmm.BinarySetTest, glmm.BinaryWideSetTest):
        with pytest.raises(ValueError, match="binary"):
            _hollow(cls).masks(ann)
    with pytest.raises(ValueError, match="set_traits"):
        MaskedSetTest(object.__new__(SetTraitPanel), ann)
    assert not hasattr(SetTraitPanel, "masks")
    # annotations, max_maf, acat_mac
    for bad in (np.ones((20, 0), dtype=bool), np.ones((20, 33), dtype=bool), np.ones((20, 2)), np.ones(20, dtype=bool), None, "lof",
                [], [np.ones((3, 2), dtype=bool), np.ones((3, 3), dtype=bool)], [np.ones((3, 2), dtype=np.int8)]):
        with pytest.raises(ValueError, match="annotation"):
            tester.masks(bad)
    assert tester.masks(np.ones((20, 32), dtype=bool)).A == 32
    for bad in ((), np.full(9, 0.1), (0.0,), (0.6,), (0.1, -0.1), (np.nan,)):
        with pytest.raises(ValueError, match="max_maf"):
            tester.masks(ann, max_maf=bad)
    assert tester.masks(ann, max_maf=0.5).F == 1 and tester.masks(ann, max_maf=np.full(8, 0.1)).F == 8
    for bad in (-1, np.inf, np.nan, "10", None, True):
        with pytest.raises(ValueError, match="acat_mac"):
            tester.masks(ann, acat_mac=bad)
    assert tester.masks(ann, acat_mac=0).acat_mac == 0.0


def masks_arg_cases():
    """(good, cases) of scilmm_sets_finish_masks_dev with dummy non-null pointers: every case is an argument error.  Shared with
    tests/test_gpu_sets_masks.py, which puts a real handle in."""
    one = C.c_void_p(8)
    start, rho, cut = np.array([0, 2, 5], dtype=np.int32), np.array([0.0, 0.5, 1.0]), np.array([0.5, 0.01])
    good = dict(fac=one, r=5, q=3, stats=one, gram=one, R=one, u=one, c=2, n_sets=2, start=_lib.ptr(start), mode=0, w=None, method=0,
                rho=_lib.ptr(rho), n_rho=3, ann=one, n_ann=3, cut=_lib.ptr(cut), n_cut=2, mac=10.0, out=one, ld=15)
    bad_start = [np.array(v, dtype=np.int32) for v in ([1, 2, 5], [0, 2, 6], [0, 2, 2], [0, 3, 2])]
    bad_rho = [np.array(v) for v in ([0.0, 1.5, 1.0], [0.0, -0.1, 1.0], [0.0, np.nan, 1.0])]
    bad_cut = [np.array(v) for v in ([0.5, 0.0], [0.5, 0.6], [-0.1, 0.1], [np.nan, 0.1])]
    cases = [dict(fac=None), dict(stats=None), dict(gram=None), dict(R=None), dict(u=None), dict(start=None), dict(out=None),
             dict(rho=None), dict(r=0), dict(r=129), dict(c=0, q=1), dict(c=32, q=33), dict(q=4), dict(n_sets=0), dict(n_sets=6),
             dict(n_rho=-1), dict(n_rho=17), dict(ld=14), dict(ld=13), dict(mode=3), dict(mode=2, w=None), dict(method=2),
             dict(ann=None), dict(cut=None), dict(n_ann=0), dict(n_ann=33), dict(n_cut=0), dict(n_cut=9), dict(mac=-1.0),
             dict(mac=np.inf), dict(mac=np.nan)]
    cases += [dict(start=_lib.ptr(v)) for v in bad_start] + [dict(rho=_lib.ptr(v)) for v in bad_rho] + [dict(cut=_lib.ptr(v)) for v in bad_cut]
    return good, cases, (start, rho, cut, bad_start, bad_rho, bad_cut)          # (the arrays are kept alive by the caller)


def test_entry_point_checks_its_arguments_first():
    """Dummy non-null pointers: every argument error comes before any dereference of the handle or of device memory."""
    L = _lib.lib()
    good, cases, alive = masks_arg_cases()
    # (with everything else in range the handle would be read next: the dummy is no handle, so the good call itself is not made)
    for kw in cases:
        a = dict(good, **kw)
        assert L.scilmm_sets_finish_masks_dev(*[a[k] for k in good]) == _lib.ERR_ARG, kw
    assert L.scilmm_sets_finish_masks_timing(None, (C.c_double * 1)()) == _lib.ERR_ARG
    assert alive


def _block(rng, sizes, c):
    r = sum(sizes)
    R = np.triu(0.2 * rng.standard_normal((c, c))) + np.diag(rng.uniform(1.0, 2.0, c))
    X = rng.standard_normal((r + 40, r)) * rng.uniform(0.3, 1.7, r)
    W = 0.3 * rng.standard_normal((c, r))
    z = np.linalg.solve(R.T, W)
    G = X.T @ X + z.T @ z
    St = np.zeros((c + 5, r))
    St[0], St[1], St[2], St[3] = 203.0, rng.uniform(0.01, 0.4, r), 1.0, np.diag(G)
    St[4:4 + c] = W
    St[4 + c] = 2.0 * rng.standard_normal(r)
    St[2, 1] = 0.0
    return St, 0.5 * (G + G.T), R


def test_host_cells_are_one_set_on_the_cells_columns_and_the_tester_is_what_it_was():
    from scilmm_amd import set_masks as M, sets
    # VariantSetTest without .masks: its surface is what it was
    assert list(inspect.signature(sets.VariantSetTest.__call__).parameters) == [
        "self", "genotypes", "sets", "weights", "method", "return_kernel", "skato", "rho", "finish", "max_markers"]
    assert sets.KEYS == ("n_used", "burden_beta", "burden_se", "burden_chi2", "burden_p", "skat_q", "skat_p")
    assert sets.FINISH_VALUES == ("host", "device", "wide")
    rng = np.random.default_rng(25)
    St, G, R = _block(rng, [9], 2)
    tester = _hollow(sets.VariantSetTest)
    tester.R, tester.u = R, np.array([0.3, -0.2])
    sf = sets.check_method("saddlepoint")
    plain = {k: np.full(1, np.nan) for k in sets.KEYS + sets.SKATO_KEYS[:3]}
    plain["n_used"], plain["skato_p_rho"] = np.zeros(1, dtype=np.int64), np.full((1, 3), np.nan)
    tester._one_set(plain, 0, St, G, "beta", sf, RHO, "saddlepoint")
    assert plain["n_used"][0] == 8
    # one all-true annotation and the cutoff 0.5: the cell is the set, and every shared number is the bits of _one_set
    ann = rng.random((9, 3)) < 0.5
    ann[:, 1] = True
    cuts = (0.5, 0.1, 0.004)
    masked = tester.masks([ann], max_maf=cuts, acat_mac=10)
    out = M.new_out(1, 3, 3, RHO)
    kernel = masked._host_set(out, 0, St, G, M.pack_words(ann), "beta", sf, RHO, "saddlepoint")
    for k in sets.KEYS + sets.SKATO_KEYS:
        assert np.array_equal(out[k][0, 1, 0], plain[k][0]), k
    # every cell: _one_set on the cell's columns, and acatv of its kernel
    maf = M.maf_of(St[1])
    for a in range(3):
        for f, cut in enumerate(cuts):
            cols = np.flatnonzero((St[2] != 0) & ann[:, a] & (maf <= cut))
            assert out["n_used"][0, a, f] == cols.size
            if not cols.size:
                assert kernel[a * 3 + f] is None and out["n_pooled"][0, a, f] == 0
                assert all(np.all(np.isnan(out[k][0, a, f])) for k in M.CELL_KEYS[1:-1] + sets.SKATO_KEYS)
                continue
            one = {k: np.full(1, np.nan) for k in sets.KEYS + sets.SKATO_KEYS[:3]}
            one["n_used"], one["skato_p_rho"] = np.zeros(1, dtype=np.int64), np.full((1, 3), np.nan)
            s, K, w = tester._one_set(one, 0, St[:, cols], G[np.ix_(cols, cols)], "beta", sf, RHO, "saddlepoint")
            for k in sets.KEYS + sets.SKATO_KEYS:
                assert np.array_equal(out[k][0, a, f], one[k][0], equal_nan=True), (a, f, k)
            p, n_pooled = M.acatv(s, K, w, maf[cols], St[0, cols], 10.0)
            assert out["acatv_p"][0, a, f] == p and out["n_pooled"][0, a, f] == n_pooled
            assert np.array_equal(kernel[a * 3 + f][1], K)
    assert out["n_used"][0, 2, 2] == 0 or out["n_used"].min() == 0              # (the smallest cutoff empties a cell)
    # acato_p: the equal-weight combination over the non-empty cells, identical cells counted as often as they occur
    M.combine_cells(out, ("burden", "skat", "acatv"))
    live = out["n_used"][0] > 0
    want = M.acat(np.concatenate([out[k][0][live] for k in ("burden_p", "skat_p", "acatv_p")]))
    assert out["cells_used"][0] == live.sum() and abs(out["acato_p"][0] - want) <= 1e-13 * want
    M.combine_cells(out, ("skato",))
    assert abs(out["acato_p"][0] - M.acat(out["skato_p"][0][live])) <= 1e-13 * out["acato_p"][0]
