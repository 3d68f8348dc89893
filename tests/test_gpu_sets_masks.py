"""scilmm_sets_finish_masks_dev and VariantSetTest.masks: every (set, annotation, cutoff) cell against the finish of the cell's
markers alone, ACAT-V against the host ``acatv``, and the Python surface end to end on the 203-individual cohort of
tests/test_gpu_skato.py (its handle, its made-up blocks and its helpers).

What is asked.  At the C level the first 10 + n_rho doubles of a cell's row are the BITS of scilmm_sets_finish_dev on a block
that holds only the cell's kept columns: the same routines on the same numbers (test_a_set_gives_the_same_bits_wherever_it_lies
of test_gpu_skato.py establishes that the finish does not depend on the thread count or the LDS cap).  ``n_pooled`` is exact;
``acatv_p`` agrees with the host to PTOL = 1e-6 on inputs where, from the host side alone, every term's p is at most 0.9 and the
cell's p at most 0.5: there erfc, tan and atan are good to a few ulps on both sides and nothing amplifies them.  End to end the
burden numbers and skat_q agree to TOL = 1e-9 and p-values to PTOL with a call of the tester on the cells' members (a Gram entry
may depend on the column's place in its block, so not bit for bit), n_used, skato_rho and n_pooled exactly.

Worst deviations measured on an MI355X when this was written (printed by the tests with -s): every cell's first 10 + n_rho
doubles the bits of the finish of its markers alone (cells of 0, 1 .. 18, 21 .. 43, 63 .. 78, 127 and 128 markers); acatv_p at the
C level, device against host, 1.3e-14; end to end in deterministic mode the cells against the tester on their members 0 on
every number (the Gram entries did not depend on the column's place); device finish against host finish under masks: burden
numbers and skat_q 3.3e-14, p-values 6.8e-13 (skato_p_rho), acatv_p 8.5e-15, acato_p 9.0e-14."""
import numpy as np
import pytest
import scipy.special as special

from tests import test_bed_api as T
from tests import test_gpu_sets as GS
from tests.test_gpu_skato import HEAD, PTOL, RHO, SENT, TOL, _c_level, _finish, _made_up_block, vp
from tests.test_sets_masks_api import masks_arg_cases

pytestmark = pytest.mark.gpu

CUTS = np.array([0.04, 0.09, 0.5])
NA = 3
MAC = 10.0


def _masks(fac, sym, torch, S, G, R, u, start, words, cuts=CUTS, n_ann=NA, mac=MAC, mode=1, weights=None, method=0, rho=RHO):
    """One call of scilmm_sets_finish_masks_dev on a sentinel-filled buffer: the rows (n_sets, n_ann, n_cut, 12 + n_rho); exactly
    the documented doubles are written."""
    q, r = S.shape[0] - 4, S.shape[1]
    ns, F, used = start.size - 1, len(cuts), HEAD + len(rho) + 2
    ld = used + 3
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    dS, dG, dR, du = dev(S), dev(G), dev(R), dev(u)
    dW = dev(weights) if weights is not None else None
    dA = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).cuda()
    dO = torch.full((ns * n_ann * F * ld + 5,), SENT, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    fac.sets_finish_masks_dev(r, q, vp(dS.data_ptr()), vp(dG.data_ptr()), vp(dR.data_ptr()), vp(du.data_ptr()), q - 1, ns, start, mode,
                              vp(dW.data_ptr()) if dW is not None else None, method, rho, vp(dA.data_ptr()), n_ann, cuts, mac,
                              vp(dO.data_ptr()), ld)
    sym.sync()
    O_ = dO.cpu().numpy()
    rows = O_[:ns * n_ann * F * ld].reshape(ns, n_ann, F, ld)
    assert np.all(O_[ns * n_ann * F * ld:] == SENT) and np.all(rows[..., used:] == SENT) and not np.any(rows[..., :used] == SENT)
    return rows[..., :used]


def _split(S, rng):
    """A copy of a made-up block's statistics with a `mean` row that the cutoffs split (maf 0.01 .. 0.15: mac 4 .. 61 at 203
    individuals), and annotation words: bit 0 half the markers, bit 1 all of them, bit 2 one in seven."""
    S = S.copy()
    r = S.shape[1]
    S[1] = rng.uniform(0.02, 0.3, r)
    ann = np.stack([rng.random(r) < 0.5, np.ones(r, dtype=bool), rng.random(r) < 0.15], axis=1)
    from scilmm_amd.set_masks import pack_words
    return S, pack_words(ann)


def _cells(S, start, words, cuts=CUTS, n_ann=NA):
    """(set, a, f, the cell's columns of the block), from the host side."""
    from scilmm_amd.set_masks import cell_members
    for i in range(start.size - 1):
        a0, b0 = start[i], start[i + 1]
        for a in range(n_ann):
            for f, cut in enumerate(cuts):
                yield i, a, f, a0 + np.flatnonzero(cell_members(S[:, a0:b0], words[a0:b0], a, cut))


def _check_empty(row, n_rho):
    assert row[0] == 0 and row[9] == 0 and row[HEAD + n_rho + 1] == 0
    assert np.all(np.isnan(row[1:9])) and np.all(np.isnan(row[HEAD:HEAD + n_rho + 1]))


def test_a_cell_gives_the_bits_of_the_finish_of_its_markers_alone():
    import torch
    st = _c_level()
    fac, sym = st["tester"].factor, st["tester"].sym
    n0 = sym.timing()["n_float_atomic_launches"]
    rng = np.random.default_rng(25)
    sizes, n_rho = [], len(RHO)
    for bi, b in enumerate(st["blocks"]):
        S, words = _split(b["S"], rng)
        G, start = b["G"], b["start"]
        modes = ((1, None),) + (((0, None), (2, rng.uniform(0.5, 2.0, S.shape[1]))) if bi == 0 else ())
        for mode, w in modes:
            rows = _masks(fac, sym, torch, S, G, st["R"], st["u"], start, words, mode=mode, weights=w)
            again = _masks(fac, sym, torch, S, G, st["R"], st["u"], start, words, mode=mode, weights=w)
            assert np.array_equal(rows, again, equal_nan=True), b["names"]                    # two runs
            for i, a, f, cols in _cells(S, start, words):
                row = rows[i, a, f]
                sizes.append(cols.size)
                if not cols.size:
                    _check_empty(row, n_rho)
                    continue
                ref, _ = _finish(fac, sym, torch, S[:, cols], G[np.ix_(cols, cols)], st["R"], st["u"],
                                 np.array([0, cols.size], dtype=np.int32), mode=mode, weights=None if w is None else w[cols], lam=False)
                assert np.array_equal(row[:HEAD + n_rho], ref[0], equal_nan=True), (b["names"][i], a, f, mode, row, ref[0])
                assert row[0] == cols.size and 0 <= row[HEAD + n_rho + 1] <= cols.size
            # the cell that keeps everything is the set itself
            full, _ = _finish(fac, sym, torch, S, G, st["R"], st["u"], start, mode=mode, weights=w, lam=False)
            assert np.array_equal(rows[:, 1, 2, :HEAD + n_rho], full, equal_nan=True), b["names"]
    # no SKAT-O: 12 doubles a row
    b = st["blocks"][0]
    S, words = _split(b["S"], rng)
    rows = _masks(fac, sym, torch, S, b["G"], st["R"], st["u"], b["start"], words, rho=np.empty(0))
    plain, _ = _finish(fac, sym, torch, S, b["G"], st["R"], st["u"], b["start"], rho=np.empty(0), lam=False)
    assert rows.shape[-1] == 12 and np.array_equal(rows[:, 1, 2, :HEAD], plain, equal_nan=True)
    print("cell sizes covered:", sorted(set(sizes)))
    assert {0, 1, 128} <= set(sizes) and 127 in sizes                        # an empty cell, one marker, a full block
    assert sym.timing()["n_float_atomic_launches"] == n0


def _terms(s, K, w, maf, n_obs, mac):
    """The terms of ACAT-V (p, weight) and the pool's size, written out once more from the contract."""
    macs, om = 2.0 * n_obs * maf, w * w * maf * (1.0 - maf)
    pool = macs <= mac
    out = [(special.erfc(np.sqrt(0.5 * s[j] ** 2 / K[j, j])), om[j]) for j in np.flatnonzero(~pool) if K[j, j] > 0 and om[j] > 0]
    if pool.any():
        q = w[pool] @ K[np.ix_(pool, pool)] @ w[pool]
        if q > 0 and om[pool].mean() > 0:
            out.append((special.erfc(np.sqrt(0.5 * (w[pool] @ s[pool]) ** 2 / q)), om[pool].mean()))
    return out, int(pool.sum())


def _signal_blocks(st):
    """Made-up blocks whose every marker carries a signal of one sign, s_j = z_j sqrt(K_jj) with z_j in [1, 3]: every marginal p is
    at most erfc(1 / sqrt 2) = 0.32, and so is a pool's (by Cauchy-Schwarz its z is at least 1 as well, whatever the positive
    weights), hence the cell's."""
    rng = np.random.default_rng(31)

    def member(k, dropped=()):
        Z = rng.standard_normal((k + 8, k)) * rng.uniform(0.3, 1.7, k)
        K = Z.T @ Z
        return ("sig%d" % k, K, rng.uniform(1.0, 3.0, k) * np.sqrt(np.diag(K)), False, dropped)
    return [_made_up_block([member(1), member(2), member(7), member(33), member(64), member(9, (0, 5, 11))], rng, st["R"], st["u"]),
            _made_up_block([member(128)], rng, st["R"], st["u"])]


def test_acatv_at_the_c_level_matches_the_host():
    import torch
    from scilmm_amd import sets as mod
    from scilmm_amd.set_masks import acat, acatv, maf_of
    st = _c_level()
    fac, sym = st["tester"].factor, st["tester"].sym
    rng = np.random.default_rng(32)
    worst, n_rho, pooled_seen = 0.0, len(RHO), set()
    for S, G, start in _signal_blocks(st):
        S, words = _split(S, rng)
        wg = rng.uniform(0.5, 2.0, S.shape[1])
        for mode, w, hw in ((1, None, None), (0, None, "beta"), (2, wg, wg)):
            rows = _masks(fac, sym, torch, S, G, st["R"], st["u"], start, words, mode=mode, weights=w)
            for i, a, f, cols in _cells(S, start, words):
                if not cols.size:
                    continue
                s, K, wk, keep = mod.set_kernel(S[:, cols], G[np.ix_(cols, cols)], st["R"], st["u"], hw if mode != 2 else hw[cols])
                assert keep.all()
                maf, n_obs = maf_of(S[1, cols]), S[0, cols]
                terms, n_pooled = _terms(s, K, wk, maf, n_obs, MAC)
                p, n_pooled2 = acatv(s, K, wk, maf, n_obs, MAC)
                # the condition on the inputs, from the host side alone
                assert terms and all(t[0] <= 0.9 for t in terms) and p <= 0.5, (i, a, f, terms, p)
                assert abs(acat([t[0] for t in terms], [t[1] for t in terms]) - p) <= 1e-12 * p
                assert n_pooled == n_pooled2 and rows[i, a, f, HEAD + n_rho + 1] == n_pooled, (i, a, f)
                e = abs(rows[i, a, f, HEAD + n_rho] - p) / p
                worst = max(worst, e)
                pooled_seen.add(0 if n_pooled == 0 else 2 if n_pooled == cols.size else 1)
                assert e < PTOL, (i, a, f, mode, rows[i, a, f, HEAD + n_rho], p)
    assert {0, 1} <= pooled_seen                                             # cells without a pool, and a pool next to single markers
    # the branches, hand-built: a term with p < 1e-15 (1 / (p pi), and T > 1e15 behind it); an empty pool; everything pooled
    rng = np.random.default_rng(33)
    Z = rng.standard_normal((14, 6))
    K = Z.T @ Z
    s = rng.uniform(1.0, 2.0, 6) * np.sqrt(np.diag(K))
    s[2] = 9.0 * np.sqrt(K[2, 2])
    S, G, start = _made_up_block([("strong6", K, s, True, ())], rng, st["R"], st["u"])
    S[1] = [0.2, 0.01, 0.3, 0.02, 0.25, 0.1]
    words = np.full(6, 7, dtype=np.uint32)
    assert special.erfc(9.0 / np.sqrt(2.0)) < 1e-15
    for mac, want_pooled in ((MAC, 2), (0.0, 0), (1e6, 6)):
        rows = _masks(fac, sym, torch, S, G, st["R"], st["u"], start, words, mac=mac)
        sk, Kk, wk, _ = mod.set_kernel(S, G, st["R"], st["u"], None)
        p, n_pooled = acatv(sk, Kk, wk, maf_of(S[1]), S[0], mac)
        got = rows[0, 0, 2]
        assert n_pooled == want_pooled == got[HEAD + n_rho + 1]
        assert 0 < p < 1e-17                                                # (the strong marker leads, pooled or not)
        e = abs(got[HEAD + n_rho] - p) / p
        worst = max(worst, e)
        assert e < PTOL, (mac, got[HEAD + n_rho], p)
    # a cell without a term: K_jj = 0 for its one marker (an exact zero: the covariates' rows are zero for the set)
    S1, G1, start1 = _made_up_block([("zero1", np.zeros((1, 1)), np.zeros(1), True, ())], rng, st["R"], st["u"])
    rows = _masks(fac, sym, torch, S1, G1, st["R"], st["u"], start1, np.full(1, 7, dtype=np.uint32), mac=0.0)
    assert rows[0, 0, 2, 0] == 1 and np.isnan(rows[0, 0, 2, HEAD + n_rho]) and rows[0, 0, 2, HEAD + n_rho + 1] == 0
    print("acatv_p, device against host, worst rel. deviation", worst)


_E2E = {}


def _e2e():
    """The spd203 problem under three nested annotations and three cutoffs that split its markers, run once."""
    if not _E2E:
        st = _c_level()
        p = GS._problem("spd203")
        tester, G = st["tester"], p["G"]
        sets = GS._fit(p["sets"], 128)
        rng = np.random.default_rng(41)
        u = rng.random(G.shape[0])
        ann = np.stack([u < 0.3, u < 0.6, np.ones(G.shape[0], dtype=bool)], axis=1)
        cuts = (0.5, 0.0301, 0.0151)
        n_obs, mean, Gt = GS._centred(G)
        from scilmm_amd.set_masks import maf_of
        with np.errstate(invalid="ignore"):
            maf = maf_of(mean)
        kept = (n_obs > 0) & Gt.any(axis=1)
        assert not np.any(np.abs(maf[kept][:, None] - np.array(cuts)[None, :]) < 1e-9)       # no marker at a cutoff
        masked = tester.masks(ann, max_maf=cuts, acat_mac=10)
        dev = masked(G, sets, skato=True)
        members = {}
        for i, rows in enumerate(sets):
            for a in range(3):
                for f, cut in enumerate(cuts):
                    members[i, a, f] = np.array([j for j in rows if kept[j] and ann[j, a] and maf[j] <= cut], dtype=np.int64)
        _E2E.update(tester=tester, G=G, sets=sets, ann=ann, cuts=cuts, masked=masked, dev=dev, members=members, p=p)
    return _E2E


def _close(got, want, tol, what):
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), what
    e = float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin]))) if fin.any() else 0.0
    assert e < tol, (what, e)
    return e


def test_cells_match_the_tester_on_their_members_end_to_end():
    from scilmm_amd import sets as mod
    from scilmm_amd.set_masks import acat
    e = _e2e()
    dev, members, tester = e["dev"], e["members"], e["tester"]
    ns, nr = len(e["sets"]), len(mod.RHO_DEFAULT)
    for k in ("burden_beta", "skat_p", "acatv_p", "skato_pmin"):
        assert dev[k].shape == (ns, 3, 3), k
    assert dev["skato_p_rho"].shape == (ns, 3, 3, nr) and dev["acato_p"].shape == (ns,) and dev["cells_used"].shape == (ns,)
    assert dev["n_used"].dtype == np.int64 and dev["n_pooled"].dtype == np.int64 and dev["cells_used"].dtype == np.int64
    live = [key for key, mem in members.items() if mem.size]
    sizes = np.array([[[members[i, a, f].size for f in range(3)] for a in range(3)] for i in range(ns)])
    assert np.array_equal(dev["n_used"], sizes) and 0 in sizes and sizes.max() > 64
    assert np.array_equal(dev["cells_used"], (sizes > 0).reshape(ns, -1).sum(axis=1))
    # ONE call of the tester on every non-empty cell's members as a set of its own
    ref = tester(e["G"], [members[key] for key in live], skato=True, finish="device")
    at = tuple(np.array(v) for v in zip(*live))
    worst = {}
    for k in ("burden_beta", "burden_se", "burden_chi2", "skat_q"):
        worst[k] = _close(dev[k][at], ref[k], TOL, k)
    for k in ("burden_p", "skat_p", "skato_p", "skato_pmin", "skato_p_rho"):
        worst[k] = _close(dev[k][at], ref[k], PTOL, k)
    assert np.array_equal(dev["n_used"][at], ref["n_used"]) and np.array_equal(dev["skato_rho"][at], ref["skato_rho"])
    print("cells against the tester on their members, worst rel. deviations", worst)
    dead = sizes == 0
    for k in ("burden_beta", "burden_se", "burden_chi2", "burden_p", "skat_q", "skat_p", "acatv_p", "skato_p", "skato_pmin", "skato_rho"):
        assert np.all(np.isnan(dev[k][dead])), k
    assert np.all(dev["n_pooled"][dead] == 0) and np.all(dev["n_pooled"] <= dev["n_used"])
    # acato_p: the equal-weight combination of the cells' p-values, NaN skipped
    P = np.stack([dev[k] for k in ("burden_p", "skat_p", "acatv_p")], axis=1).reshape(ns, -1)
    assert np.array_equal(dev["acato_p"], acat(P, axis=1), equal_nan=True)
    with_o = e["masked"](e["G"], e["sets"], skato=True, combine=("skato",))
    assert np.array_equal(with_o["acato_p"], acat(dev["skato_p"].reshape(ns, -1), axis=1), equal_nan=True)
    for k in dev:
        if k != "acato_p":
            assert np.array_equal(with_o[k], dev[k], equal_nan=True), k        # two runs: the same bits


def test_one_all_true_annotation_is_the_tester_bit_for_bit():
    from scilmm_amd import sets as mod
    e = _e2e()
    tester, G, sets = e["tester"], e["G"], e["sets"]
    for kw in (dict(skato=True), dict(), dict(weights=None, method="liu", skato=True, rho=(0.0, 0.3, 1.0))):
        plain = tester(G, sets, finish="device", **kw)
        one = tester.masks(np.ones((G.shape[0], 1), dtype=bool), max_maf=(0.5,))(G, sets, **kw)
        assert sorted(set(one) - set(plain)) == ["acato_p", "acatv_p", "cells_used", "n_pooled"]
        for k in plain:
            assert one[k].shape == plain[k].shape[:1] + (1, 1) + plain[k].shape[1:], k
            assert np.array_equal(one[k][:, 0, 0], plain[k], equal_nan=True), k
    assert sorted(plain) == sorted(mod.KEYS + mod.SKATO_KEYS)


def test_device_cells_match_the_host_finish_and_both_annotation_forms_agree():
    e = _e2e()
    masked, G, sets, dev = e["masked"], e["G"], e["sets"], e["dev"]
    # burden, SKAT and ACAT-V on every set; SKAT-O (whose host form integrates adaptively) on the sets of up to 16 markers
    host = masked(G, sets, finish="host", return_kernel=True)
    small = [i for i, s in enumerate(sets) if s.size <= 16]
    host_o = masked(G, [sets[i] for i in small], finish="host", skato=True, combine=("burden", "skat", "acatv", "skato"))
    dev_o = masked(G, [sets[i] for i in small], skato=True, combine=("burden", "skat", "acatv", "skato"))
    worst = {}
    for h, d, keys in ((host, dev, ()), (host_o, dev_o, ("skato_p", "skato_pmin", "skato_p_rho"))):
        assert np.array_equal(d["n_used"], h["n_used"]) and np.array_equal(d["n_pooled"], h["n_pooled"])
        assert np.array_equal(d["cells_used"], h["cells_used"])
        for k in ("burden_beta", "burden_se", "burden_chi2", "skat_q"):
            worst[k] = max(worst.get(k, 0.0), _close(d[k], h[k], TOL, k))
        for k in ("burden_p", "skat_p", "acatv_p", "acato_p") + keys:
            worst[k] = max(worst.get(k, 0.0), _close(d[k], h[k], PTOL, k))
        if keys:
            assert np.array_equal(d["skato_rho"], h["skato_rho"], equal_nan=True)
    print("device finish against host finish under masks, worst rel. deviations", worst)
    assert len(host["kernel"]) == len(sets) and all(len(k) == 9 for k in host["kernel"])
    for i in range(len(sets)):
        for c in range(9):
            cell = host["kernel"][i][c]
            assert (cell is None) == (dev["n_used"][i, c // 3, c % 3] == 0)
            assert cell is None or cell[1].shape == (cell[0].size,) * 2
    # the per-set form of the annotations: the same bits
    per = e["tester"].masks([e["ann"][s] for s in sets], max_maf=e["cuts"], acat_mac=10)(G, sets, skato=True)
    for k in dev:
        assert np.array_equal(per[k], dev[k], equal_nan=True), k


def test_bed_and_dosages_give_the_bits_of_the_int8_call(tmp_path):
    e = _e2e()
    masked, G, sets, dev, p = e["masked"], e["G"], e["sets"], e["dev"], e["p"]
    path = T.write_fileset(tmp_path / "id", T.pack(G), p["n"])
    bed = masked.test_bed(path, sets, skato=True)
    codes = np.where(G >= 0, G.astype(np.int64) * 16384, 65535).astype(np.uint16)
    dos = masked.test_dosages(codes, sets, skato=True)
    for other in (bed, dos):
        assert sorted(other) == sorted(dev)
        for k in dev:
            assert np.array_equal(other[k], dev[k], equal_nan=True), k


def test_argument_errors_leave_the_handle_usable():
    import torch
    from scilmm_amd import _lib
    st = _c_level()
    fac, sym = st["tester"].factor, st["tester"].sym
    L = _lib.lib()
    good, cases, alive = masks_arg_cases()
    good["fac"] = fac._h
    for kw in cases:
        a = dict(good, **kw)
        assert L.scilmm_sets_finish_masks_dev(*[a[k] for k in good]) == _lib.ERR_ARG, kw
    assert alive
    b = st["blocks"][0]
    words = np.full(b["S"].shape[1], 1, dtype=np.uint32)
    rows = _masks(fac, sym, torch, b["S"], b["G"], st["R"], st["u"], b["start"], words, cuts=np.array([0.5]), n_ann=1)
    full, _ = _finish(fac, sym, torch, b["S"], b["G"], st["R"], st["u"], b["start"], lam=False)
    assert np.array_equal(rows[:, 0, 0, :HEAD + len(RHO)], full, equal_nan=True)
    assert sym.sets_finish_masks_timing() > 0.0


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
        eng.fac.sets_finish_masks_dev(5, 3, bp, bp, bp, bp, 2, 2, np.array([0, 2, 5], dtype=np.int32), 1, None, 0, np.array([0.0, 1.0]), bp,
                                      2, np.array([0.5, 0.01]), 10.0, bp, 14)
    assert eng.collectives == 0
