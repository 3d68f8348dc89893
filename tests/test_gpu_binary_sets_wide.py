"""Wide variant sets for binary traits on the device (scilmm_amd.glmm.BinaryWideSetTest, scilmm_sets_collapse*_dev,
scilmm_sets_spa_wide_dev, scilmm_sets_finish_wide_scaled_dev) against the dense oracle
(tests/setspa_oracle.py::set_test, which takes any number of rows), at the GIVEN null point and on the cohorts of
tests/test_gpu_binary_sets.py (pedigree n = 1502, sub100 n = 100; prevalence 0.05; M = 130 markers), whose helpers are imported.

Tolerances: those of tests/test_gpu_binary_sets.py, where they are derived.  Flags and counts: exact.  a_B, b_B, a_w, s_B, skat_q:
1e-9 relative; burden_spa_log_p: 1e-8 max(1, |log p|); p-values: 1e-6 relative; vscale, phi, V_Q, burden_chi2: 1e-7 relative.  The
collapsed row: 1e-12 of its largest entry against NumPy (at most 128 terms of one sign pattern each, rounded once per fma), and bit
identity across the cuts and the input forms, where the issue is the order of a sum.  The pair sums a_B and V_Q of a narrow set fed
through the wide entry points are NOT the bits of scilmm_sets_spa_dev's: k_sets_spa deals the pairs to its threads at a stride of
256, k_swide_pairs sums row by row; they are held to the tolerances above.

At the C level every buffer an entry point reads a part of is NaN-filled before the sub-blocks write into it: the rest of a ragged
slice, the padding columns of the cross store, the collapsed row before its first collapse.  A stray read shows as a NaN.

The conditions on the inputs are asserted from the oracle alone (`_check_conditions`).  One of them is stated for another set than
it was first written down for: "ASSOC + the non-ASSOC markers at positions 60 .. 90" is read here as positions 60 .. 89 of the
non-special markers by frequency, for which the oracle gives phi = 1.0235 at (pedigree, c = 4, None, 2.0), not 1.017; no reading
of the positions that was tried gives 1.017, and the set serves its purpose (a second set at the burden floor) with either.

Worst deviations measured on an MI355X when this was written (printed by the tests with -s): against the oracle a_B, b_B, a_w,
s_B, skat_q 1.5e-14 (burden_chi2_norm 3.2e-14); log_p_B 5.2e-13; vscale 1.9e-13; phi, burden_chi2 2.1e-13; p-values 1.8e-12;
finish="wide" against the host finish 3.2e-12; the collapsed row against NumPy 1.2e-15 of its largest entry; a narrow set through
the wide entry points against scilmm_sets_spa_dev 2.7e-16 (a_B, V_Q, phi; every other number the same bits)."""
import ctypes as C

import numpy as np
import pytest

from scilmm_amd import binary_sets, glmm
from tests import setspa_oracle as SO
from tests import spa_oracle as O
from tests import test_gpu_binary_sets as BS

pytestmark = pytest.mark.gpu

TOL, LTOL, PTOL, VTOL = BS.TOL, BS.LTOL, BS.PTOL, BS.VTOL
RHO, M, vp = BS.RHO, BS.M, C.c_void_p
CANARY = -7.25


def _freq_order(p):
    """The non-special markers from the rarest to the most common."""
    G = p["G"]
    special = {O.MONO, O.ALLMISS, O.MISS30} | set(O.ASSOC)
    freq = np.where(G < 0, 0, G).sum(axis=1) / np.maximum((G >= 0).sum(axis=1), 1)
    return [int(j) for j in np.argsort(freq, kind="stable") if int(j) not in special]


def _sets16(p, common=False):
    """The sets of block 16, all wider than a block: (label, rows); `common`: the 40 most common non-special markers as well."""
    order = _freq_order(p)
    return _SETS16(order) + ([("common40", np.array(order[-40:]))] if common else [])


def _SETS16(order):
    return [("23..39", np.arange(23, 40)), ("20..52", np.arange(20, 53)), ("60..109", np.arange(60, 110)), ("all130", np.arange(130)),
            ("special+40..69", np.array([O.MONO, O.ALLMISS, O.MISS30] + list(range(40, 70)))),
            ("assoc+rare30", np.array(list(O.ASSOC) + order[:30])), ("assoc+mid30", np.array(list(O.ASSOC) + order[60:90]))]


def _given(rows):
    return np.random.default_rng(5 + rows.size).uniform(0.5, 2.0, rows.size)


def _oracle(p, c, weights, cutoff, label, rows):
    refs = p.setdefault("ref_wide", {})
    key = (c, weights, cutoff, label)
    if key not in refs:
        refs[key] = SO.set_test(BS._cohort(p, c), rows, _given(rows) if weights == "given" else weights, cutoff, RHO)
    return refs[key]


def _wtester(p, c, block, cutoff, max_markers=256, **kw):
    return BS._null(p, c, **kw).sets(block=block, cutoff=cutoff, max_markers=max_markers)


def _near(x, want, tol):
    return abs(x - want) < tol


def _check_conditions(name, c, weights, cutoff, refs):
    """Conditions on the tests' inputs, from the oracle alone (`refs`: label -> the oracle's result)."""
    for r in refs.values():
        if r["n_used"]:
            z = np.r_[r["zs"], r["zs_B"]]
            assert not np.any(np.abs(np.abs(z[np.isfinite(z)]) - cutoff) < 1e-6)     # (a flag cannot flip on rounding)
    key = (name, c, weights, cutoff)
    if key == ("pedigree", 1, None, 0.5):
        assert _near(refs["assoc+rare30"]["phi"], 1.079, 1e-3)
        assert refs["20..52"]["flag"] != 0 and _near(abs(refs["20..52"]["zs_B"]), 2.008, 1e-3)
        assert refs["23..39"]["flag"] == 0 and _near(abs(refs["23..39"]["zs_B"]), 0.13, 1e-2)
    if key == ("pedigree", 4, None, 2.0):
        assert _near(refs["assoc+rare30"]["phi"], 1.085, 1e-3) and refs["assoc+rare30"]["flag"] == 1
        # (positions 60 .. 89 of the list of non-special markers by frequency: the oracle gives 1.0235 for them)
        assert _near(refs["assoc+mid30"]["phi"], 1.0235, 1e-3) and refs["assoc+mid30"]["flag"] == 1
    if key == ("pedigree", 31, "beta", 0.5):
        r = refs["all130"]
        assert (r["n_used"], r["n_adj"], r["flag"]) == (128, 78, 1)
    if key == ("pedigree", 4, "beta", 2.0):       # the rho path alone: no burden is attempted, a few markers are adjusted
        assert all(r["flag"] == 0 for r in refs.values())
        assert all(2 <= r["n_adj"] <= 7 for k, r in refs.items() if k != "special+40..69") and refs["special+40..69"]["n_adj"] == 1
    if key == ("sub100", 1, None, 0.5):
        assert _near(refs["common40"]["phi"], 1.014, 1e-3)


def _against_oracle(out, B, i, r, what, worst):
    def close(k, got, want, tol):
        e = abs(got - want) / abs(want)
        worst[k] = max(worst.get(k, 0.0), e)
        assert e < tol, (what, k, got, want, e)

    assert out["n_used"][i] == r["n_used"] and out["n_adjusted"][i] == r["n_adj"] and out["burden_spa_flag"][i] == r["flag"], what
    if not r["n_used"]:
        assert np.all(np.isnan([out[k][i] for k in ("burden_chi2", "burden_p", "skat_p", "skato_p", "burden_scale", "burden_spa_log_p")]))
        assert out["kernel"][i][0].size == 0
        return
    close("a_B", B[i, 7], r["a_B"], TOL)
    close("b_B", B[i, 8], r["b_B"], TOL)
    close("V_Q", B[i, 10], r["V_Q"], VTOL)
    close("burden_chi2_norm", out["burden_chi2_norm"][i], r["burden_chi2_norm"], TOL)
    close("skat_q", out["skat_q"][i], r["skat_q"], TOL)
    if r["flag"]:
        close("a_w", B[i, 1], r["a_w"], TOL)
        close("s_B", B[i, 2], r["s_B"], TOL)
        gap = abs(out["burden_spa_log_p"][i] - r["log_p"]) / max(1.0, abs(r["log_p"]))
        worst["log_p"] = max(worst.get("log_p", 0.0), gap)
        assert gap < LTOL, (what, gap)
    else:
        assert np.all(np.isnan(B[i, :6]))
    s, Kt, w, vs = out["kernel"][i]
    e = float(np.max(np.abs(vs - r["vscale"]) / r["vscale"]))
    worst["vscale"] = max(worst.get("vscale", 0.0), e)
    assert e < VTOL, (what, "vscale", e)
    Kref = r["vscale"][:, None] * r["K"] * r["vscale"][None, :]
    assert np.max(np.abs(Kt - Kref)) < VTOL * np.max(np.abs(Kref)), what
    close("phi", out["burden_scale"][i], r["phi"], VTOL)
    for k in ("burden_chi2", "burden_beta", "burden_se"):
        close(k, out[k][i], r[k], VTOL)
    if r["phi"] > 1.0:
        close("chi2 at the floor", out["burden_chi2"][i], r["x_B"], VTOL)
    for k in ("burden_p", "skat_p", "skato_p", "skato_pmin"):
        close(k, out[k][i], r[k], PTOL)
    e = float(np.max(np.abs(out["skato_p_rho"][i] - r["skato_p_rho"]) / r["skato_p_rho"]))
    worst["skato_p_rho"] = max(worst.get("skato_p_rho", 0.0), e)
    assert e < PTOL, (what, "skato_p_rho", e)


def _wide_against_host(dev, host, what, worst):
    from scilmm_amd.sets import KEYS, SKATO_KEYS
    assert sorted(dev) == sorted(host) == sorted(KEYS + SKATO_KEYS + binary_sets.BINARY_KEYS)
    BS._same(dev, host, ("n_used", "n_adjusted", "burden_spa_flag", "burden_spa_log_p", "burden_scale", "burden_chi2_norm", "skato_rho"))
    live = host["n_used"] > 0
    for k in ("burden_beta", "burden_se", "burden_chi2", "burden_p", "skat_q", "skat_p", "skato_p", "skato_pmin", "skato_p_rho"):
        assert np.all(np.isnan(dev[k][~live])) and not np.any(np.isnan(dev[k][live])), (what, k)
        if live.any():
            e = float(np.max(np.abs(dev[k][live] - host[k][live]) / np.abs(host[k][live])))
            worst[k] = max(worst.get(k, 0.0), e)
            assert e < PTOL, (what, k, e)


# (name, c, weights, cutoff, the other block sizes as well)
CONFIGS = [("pedigree", 1, None, 0.5, True), ("pedigree", 4, None, 2.0, False), ("pedigree", 31, "beta", 0.5, True),
           ("pedigree", 4, "beta", 2.0, False), ("sub100", 1, None, 0.5, False), ("sub100", 4, "given", 0.5, False)]


@pytest.mark.parametrize("name,c,weights,cutoff,blocks", CONFIGS)
def test_host_finish_matches_the_dense_oracle_and_the_wide_finish_the_host_finish(name, c, weights, cutoff, blocks):
    p = BS._problem(name)
    runs = [(16, _sets16(p, common=name == "sub100"))]
    if blocks:
        runs += [(128, [("all129", np.arange(129)), ("all130", np.arange(130))]), (112, [("all130", np.arange(130))]),
                 (1, [("nothing", np.array([O.MONO, O.ALLMISS]))])]
    refs = {label: _oracle(p, c, weights, cutoff, label, rows) for _, sets in runs for label, rows in sets}
    _check_conditions(name, c, weights, cutoff, refs)
    assert not blocks or refs["nothing"]["n_used"] == 0
    worst, worst_wide = {}, {}
    for block, sets in runs:
        tester = _wtester(p, c, block, cutoff, deterministic=True)
        assert type(tester) is glmm.BinaryWideSetTest and tester.block == block
        rows = [s for _, s in sets]
        wts = [_given(s) for s in rows] if weights == "given" else weights
        host = tester(p["G"], rows, weights=wts, skato=True, rho=RHO, return_kernel=True)
        Bh = tester.last_bspa.copy()
        for i, (label, _) in enumerate(sets):
            _against_oracle(host, Bh, i, refs[label], (name, c, weights, cutoff, block, label), worst)
        dev = tester(p["G"], rows, weights=wts, skato=True, rho=RHO, finish="wide")
        assert np.array_equal(tester.last_bspa, Bh, equal_nan=True)
        del host["kernel"]
        _wide_against_host(dev, host, (name, c, weights, cutoff, block), worst_wide)
        assert tester.sym.timing()["n_float_atomic_launches"] == 0
    print(name, c, weights, cutoff, "host finish against the oracle", worst, "wide finish against host finish", worst_wide,
          "phi", {k: round(r["phi"], 4) for k, r in refs.items() if r["n_used"]}, "n_adj", {k: r["n_adj"] for k, r in refs.items()})


class _Pieces(object):
    """One wide set at the C level: its rows run as sub-blocks of ``blk`` through the source's Gram entry point, saddlepoint call
    and collapse, the panel and the keep, into NaN-filled buffers; ``gB`` is the collapsed row after the last collapse.
    ``spa_wide`` and ``finish`` run on what the sub-blocks left (or what ``upload_spa`` wrote over it)."""

    def __init__(self, tester, src, rows, blk, mode=1, w=None, stage=True, follow=True):
        import torch
        self.t, self.torch, self.rows, self.blk, self.mode = tester, torch, np.asarray(rows), blk, mode
        q, n, k = tester.q, tester.n, len(rows)
        self.k, self.B, self.bp = k, -(-k // blk), (blk + 15) // 16 * 16
        B, bp = self.B, self.bp
        self.ld = ld = (B - 1) * bp
        nans = lambda m: torch.full((max(m, 1),), float("nan"), dtype=torch.float64, device="cuda")
        self.dS, self.dK, self.dP = nans(B * (q + 4) * blk), nans(B * blk * blk), nans(B * glmm.SPA_ROWS * blk)
        self.dX, self.store, self.dg = nans(k * ld), nans(n * ld), nans(n)
        self.dW = torch.from_numpy(np.ascontiguousarray(w)).cuda() if w is not None else None
        if stage:
            src.stage(128)
        torch.cuda.synchronize()
        at = lambda d, off: vp(d.data_ptr() + 8 * off)
        for b in range(B):
            sub = self.rows[b * blk:(b + 1) * blk]
            rb, t = sub.size, b * bp
            pS = at(self.dS, b * (q + 4) * blk)
            src.load(sub)
            src.enqueue(0, rb, pS, at(self.dK, b * blk * blk))
            if follow:
                src.spa(0, rb, (pS,) + self.null(tester.cutoff) + (at(self.dP, b * glmm.SPA_ROWS * blk),))
            src.collapse(0, rb, (pS, mode, at(self.dW, b * blk) if w is not None else None, b == 0, vp(self.dg.data_ptr())))
            if follow and b > 0:
                tester.factor.scan_panel_dev(rb, vp(self.store.data_ptr()), ld, t, at(self.dX, b * blk * ld), ld)
            if follow and b < B - 1:
                tester.factor.scan_block_keep_dev(rb, vp(self.store.data_ptr()), ld, t)
            tester.sym.sync()
        self.gB = self.dg.cpu().numpy().copy()

    def null(self, cutoff):
        t = self.t
        return (vp(t.dR.data_ptr()), vp(t.du.data_ptr()), vp(t.dmu.data_ptr()), vp(t.dC.data_ptr()), t.c, vp(t.dMinv.data_ptr()), cutoff)

    def _wide(self):
        return (self.k, self.blk, self.t.q, vp(self.dS.data_ptr()), vp(self.dK.data_ptr()), vp(self.dX.data_ptr()) if self.B > 1 else None,
                self.ld)

    def host(self):
        """((q + 4) x k statistics, k x k X'X, 7 x k saddlepoint rows) put together on the host."""
        from scilmm_amd.sets import assemble_wide
        q, blk, ld, k = self.t.q, self.blk, self.ld, self.k
        hS, hK, hX, hP = (d.cpu().numpy() for d in (self.dS, self.dK, self.dX, self.dP))
        rbs = [min(blk, k - b * blk) for b in range(self.B)]
        Ss = [hS[b * (q + 4) * blk:][:(q + 4) * rb].reshape(q + 4, rb) for b, rb in enumerate(rbs)]
        Gs = [hK[b * blk * blk:][:rb * rb].reshape(rb, rb) for b, rb in enumerate(rbs)]
        Xs = [hX[b * blk * ld:][:rb * ld].reshape(rb, ld)[:, :b * self.bp] for b, rb in enumerate(rbs) if b > 0]
        P = np.concatenate([hP[b * 7 * blk:][:7 * rb].reshape(7, rb) for b, rb in enumerate(rbs)], axis=1)
        return assemble_wide(Ss, Gs, Xs, self.bp) + (P,)

    def upload_spa(self, P):
        """7 x k saddlepoint rows cut into the sub-blocks' slices, NaN elsewhere."""
        blk, h = self.blk, np.full(self.dP.numel(), np.nan)
        for b in range(self.B):
            rb = min(blk, self.k - b * blk)
            h[b * 7 * blk:b * 7 * blk + 7 * rb] = P[:, b * blk:b * blk + rb].ravel()
        self.dP.copy_(self.torch.from_numpy(h))
        self.torch.cuda.synchronize()

    def spa_wide(self, cutoff):
        """(13 numbers, k scales, the row the call left behind); exactly the documented doubles are written."""
        torch, k, n = self.torch, self.k, self.t.n
        dB = torch.full((13 + 3,), CANARY, dtype=torch.float64, device="cuda")
        self.dV = torch.full((k + 3,), CANARY, dtype=torch.float64, device="cuda")
        dg = torch.cat([self.dg, torch.full((3,), CANARY, dtype=torch.float64, device="cuda")])
        torch.cuda.synchronize()
        self.t.factor.sets_spa_wide_dev(*(self._wide() + self.null(cutoff) + (vp(self.dP.data_ptr()), self.mode,
                                                                              vp(self.dW.data_ptr()) if self.dW is not None else None,
                                                                              vp(dg.data_ptr()), vp(dB.data_ptr()), vp(self.dV.data_ptr()))))
        self.t.sym.sync()
        B, V, g = dB.cpu().numpy(), self.dV.cpu().numpy(), dg.cpu().numpy()
        assert np.all(B[13:] == CANARY) and np.all(V[k:] == CANARY) and np.all(g[n:] == CANARY)
        assert not np.any(B[:13] == CANARY) and not np.any(V[:k] == CANARY) and not np.any(np.isnan(V[:k]))
        return B[:13], V[:k], g[:n]

    def finish(self, dV=None, rho=RHO, method=0):
        torch, t = self.torch, self.t
        n = 10 + len(rho)
        dO = torch.full((n + 3,), CANARY, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        args = self._wide() + (vp(t.dR.data_ptr()), vp(t.du.data_ptr()), t.c, self.mode, vp(self.dW.data_ptr()) if self.dW is not None else None,
                               method, rho, vp(dO.data_ptr()), None)
        if dV is None:
            t.factor.sets_finish_wide_dev(*args)
        else:
            t.factor.sets_finish_wide_scaled_dev(*(args + (vp(dV.data_ptr()),)))
        t.sym.sync()
        O_ = dO.cpu().numpy()
        assert np.all(O_[n:] == CANARY) and not np.any(O_[:n] == CANARY)
        return O_[:n]


def _forms(tester, p, tmp_path):
    """The three marker sources of the same hard calls."""
    from scilmm_amd import dosage
    from scilmm_amd.markers import Int8Rows
    from tests.test_bed_api import pack, write_fileset
    path = write_fileset(tmp_path / "cohort", pack(p["G"]), p["n"])
    codes = dosage.encode(np.where(p["G"] < 0, np.nan, p["G"].astype(np.float64)))
    assert codes.dtype == np.uint16
    return {"int8": Int8Rows(tester, p["G"]), "bed": tester._bed_source(path, None, "A1"), "dosage": tester._dosage_source(codes, None)}


def test_the_collapsed_row_at_the_c_level(tmp_path):
    """d_gB after the collapses, before the set saddlepoint: against NumPy's sum_j w_j g~_j, and the same bits for sub-blocks of 1,
    16 and 128 and from int8, .bed and hard-call dosage rows, for the three weight modes.  The set holds the monomorphic and the
    all-missing marker (dropped: sub-block 3 and 5 of the cut into single markers keep nothing) and the one with 30 % missing."""
    import scipy.stats as stats
    p = BS._problem("pedigree")
    tester = _wtester(p, 4, 128, 2.0)
    rows = np.arange(130)
    Gt, n_obs, mean = O.centred(p["G"])
    keep = (n_obs > 0) & (np.abs(Gt).max(axis=1) > 0)
    assert not keep[O.MONO] and not keep[O.ALLMISS] and keep.sum() == 128
    forms = _forms(tester, p, tmp_path)
    given = _given(rows)
    n0 = tester.sym.timing()["n_float_atomic_launches"]
    for mode, w, wref in ((1, None, np.ones(130)), (0, None, stats.beta.pdf(np.minimum(0.5 * mean, 1 - 0.5 * mean), 1, 25)), (2, given, given)):
        want = (wref[keep][:, None] * Gt[keep]).sum(axis=0)
        first = None
        for form, src in forms.items():
            for blk in ((1, 16, 128) if form == "int8" else (16,)):
                # (the Gram blocks of a default handle count their atomic launches: the collapse is timed alone below)
                got = _Pieces(tester, src, rows, blk, mode, w, follow=False).gB
                assert not np.any(np.isnan(got))
                e = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
                assert e < 1e-12, (mode, form, blk, e)
                if first is None:
                    first = got
                    print("collapsed row, mode", mode, "against NumPy:", e, "of the largest entry", np.max(np.abs(want)))
                assert np.array_equal(got, first), (mode, form, blk)
    # the collapse alone: a sub-block with nothing kept leaves the row as it is, or zero if it is the first; no atomics
    import torch
    src = forms["int8"]
    dS = torch.full(((tester.q + 4) * 2,), float("nan"), dtype=torch.float64, device="cuda")
    dK = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
    dg = torch.full((p["n"] + 3,), CANARY, dtype=torch.float64, device="cuda")
    src.load(np.array([O.MONO, O.ALLMISS]))
    src.enqueue(0, 2, vp(dS.data_ptr()), vp(dK.data_ptr()))
    tester.sym.sync()
    n0 = tester.sym.timing()["n_float_atomic_launches"]
    src.collapse(0, 2, (vp(dS.data_ptr()), 1, None, False, vp(dg.data_ptr())))
    tester.sym.sync()
    assert np.all(dg.cpu().numpy() == CANARY)
    src.collapse(0, 2, (vp(dS.data_ptr()), 1, None, True, vp(dg.data_ptr())))
    tester.sym.sync()
    g = dg.cpu().numpy()
    assert np.all(g[:p["n"]] == 0.0) and np.all(g[p["n"]:] == CANARY)
    assert tester.sym.timing()["n_float_atomic_launches"] == n0
    ms = tester.factor.sets_spa_wide_timing()
    assert ms == tester.sym.sets_spa_wide_timing() and ms[0] > 0.0


def test_a_narrow_set_through_the_wide_entry_points_matches_sets_spa_dev():
    """B = 1: the block's statistics, Gram matrix and saddlepoint rows ARE the slices.  The 13 numbers and the scales agree with
    scilmm_sets_spa_dev's within the tolerances of this file; a_B and V_Q fold in another order, so they are not bit-identical
    (the collapsed row is: one fma chain)."""
    from scilmm_amd.markers import Int8Rows
    p = BS._problem("pedigree")
    tester = _wtester(p, 1, 128, 0.5)
    worst, attempted, adjusted = {}, 0, 0
    for i in (2, 3, 4, 5, 6, 7):
        rows = p["sets"][i]
        blk = BS._Block(tester, p["G"], rows)
        Bn, Vn = blk.sets_spa([0, rows.size], 0.5)
        pc = _Pieces(tester, Int8Rows(tester, p["G"]), rows, 128)
        assert pc.B == 1
        Bw, Vw, ghat = pc.spa_wide(0.5)
        assert Bw[6] == Bn[0, 6] and Bw[12] == Bn[0, 12] and np.isnan(Bw[5]) == np.isnan(Bn[0, 5]), i
        attempted += Bw[6] != 0
        adjusted += Bw[12] > 0
        if i == BS.NOTHING:
            assert np.all(np.isnan(np.delete(Bw, [6, 12]))) and Bw[6] == 0 and Bw[12] == 0 and np.all(Vw == 1.0)
            continue
        for col, tol in ((0, LTOL), (1, TOL), (2, TOL), (3, VTOL), (4, VTOL), (7, TOL), (8, TOL), (9, VTOL), (10, VTOL), (11, VTOL)):
            a, b = Bw[col], Bn[0, col]
            if np.isnan(b):
                assert np.isnan(a), (i, col)
                continue
            e = abs(a - b) / (max(1.0, abs(b)) if col == 0 else abs(b))
            worst[col] = max(worst.get(col, 0.0), e)
            assert e < tol, (i, col, a, b, e)
        assert Bw[8] == Bn[0, 8] or abs(Bw[8] - Bn[0, 8]) < TOL * abs(Bn[0, 8])
        e = float(np.max(np.abs(Vw - Vn[:rows.size]) / Vn[:rows.size]))
        worst["vscale"] = max(worst.get("vscale", 0.0), e)
        assert e < VTOL, (i, e)
        assert np.array_equal(Vw == 1.0, Vn[:rows.size] == 1.0), i
        # not attempted: the collapsed row is left as it was
        assert Bw[6] != 0 or np.array_equal(ghat, pc.gB)
    assert attempted >= 2 and adjusted >= 3
    print("narrow set through the wide entry points against scilmm_sets_spa_dev: worst deviations by column", worst)


def test_scaled_wide_finish_unit_scales_give_the_bits_and_other_scales_the_host_numbers():
    import torch
    from scilmm_amd.markers import Int8Rows
    from scilmm_amd.sets import set_kernel
    p = BS._problem("pedigree")
    tester = _wtester(p, 4, 128, 2.0)
    src = Int8Rows(tester, p["G"])
    rng = np.random.default_rng(3)
    for rows, blk, mode, w in ((np.arange(130), 16, 0, None), (np.arange(130), 112, 1, None), (np.arange(23, 40), 16, 2, _given(np.arange(23, 40))),
                               (np.array([O.MONO, O.ALLMISS]), 1, 1, None)):
        pc = _Pieces(tester, src, rows, blk, mode, w)
        k = rows.size
        plain = pc.finish()
        ones = torch.ones((k,), dtype=torch.float64, device="cuda")
        assert np.array_equal(plain, pc.finish(dV=ones), equal_nan=True), (blk, mode)
        if k == 2:
            assert plain[0] == 0 and plain[9] == 0 and np.all(np.isnan(plain[1:9]))
            continue
        assert not int(plain[9]) & binary_sets.FLAG_SCALED and not np.any(np.isnan(plain[:9]))
        # scales in [1, 1.5]; a dropped marker's scale is not looked at for the flag
        S, G, _ = pc.host()
        wi = None if mode == 1 else "beta" if mode == 0 else w
        s, K, wk, keep = set_kernel(S, G, tester.R, tester.u, wi)
        V = rng.uniform(1.0, 1.5, k)
        got = pc.finish(dV=torch.from_numpy(V).cuda())
        t = binary_sets.scaled_tests(s, K, wk, V[keep], "saddlepoint", RHO)
        assert int(got[9]) & binary_sets.FLAG_SCALED and got[0] == keep.sum()
        for col, key in ((1, "burden_beta"), (2, "burden_se"), (3, "burden_chi2"), (4, "skat_q")):
            assert abs(got[col] - t[key]) < TOL * abs(t[key]), (blk, key)
        assert got[4] == plain[4]                                  # t keeps w
        assert abs(got[5] - t["skat_p"]) < PTOL * t["skat_p"] and abs(got[6] - t["skato"][0]) < PTOL * t["skato"][0]
        assert np.max(np.abs(got[10:] - t["skato"][3]) / t["skato"][3]) < PTOL
        only_dropped = np.where(keep, 1.0, 1.25)
        if not keep.all():
            assert np.array_equal(pc.finish(dV=torch.from_numpy(only_dropped).cuda()), plain, equal_nan=True)
    ms = tester.sym.sets_finish_wide_timing()
    assert all(v >= 0.0 for v in ms) and ms[0] > 0.0


def test_doctored_marker_rows_at_the_c_level():
    """Per-marker saddlepoint rows written by hand into the slices of three sub-blocks: log_p = 0, +1e-3, NaN with flag 1, flag 2 and
    flag 0 give a scale of exactly 1; log_p = -800 (p underflows) gives a finite scale that agrees with the oracle's root.  The
    cutoff of the set call is out of reach, so no burden is attempted and phi = 1."""
    from scilmm_amd.markers import Int8Rows
    from scilmm_amd.sets import set_kernel
    p = BS._problem("pedigree")
    tester = _wtester(p, 4, 128, 2.0)
    rows = np.arange(20, 28)
    pc = _Pieces(tester, Int8Rows(tester, p["G"]), rows, 3)
    assert pc.B == 3
    P = np.full((7, 8), np.nan)
    P[6] = [1, 1, 1, 2, 0, 1, 1, 1]
    P[0] = [0.0, 1e-3, np.nan, -5.0, -5.0, -800.0, -3.0, -1e-3]
    pc.upload_spa(P)
    n0 = tester.sym.timing()["n_float_atomic_launches"]
    B, V, g = pc.spa_wide(1e9)
    assert tester.sym.timing()["n_float_atomic_launches"] == n0
    ms = tester.factor.sets_spa_wide_timing()
    assert ms[1] > 0.0 and ms[2] > 0.0
    assert np.all(V[:5] == 1.0) and B[6] == 0 and B[11] == 1.0 and B[12] == 3 and np.all(np.isnan(B[:6])) and np.isnan(B[9])
    assert np.array_equal(g, pc.gB)
    S, G, _ = pc.host()
    s, K, w, keep = set_kernel(S, G, tester.R, tester.u, None)
    assert keep.all()
    zs = s / np.sqrt(np.diag(K))
    for j, lp in ((5, -800.0), (6, -3.0), (7, -1e-3)):
        want = abs(zs[j]) / SO.deviate(lp)
        print("log_p", lp, "scale", V[j], "oracle", want)
        assert np.isfinite(V[j]) and abs(V[j] - want) < 1e-9 * want, (j, V[j], want)
    assert abs(B[7] - K.sum()) < TOL * K.sum() and abs(B[10] - V @ K @ V) < TOL * (V @ K @ V) and abs(B[8] - s.sum()) < TOL * abs(s.sum())
    got = pc.finish(dV=pc.dV)
    t = binary_sets.scaled_tests(s, K, w, V, "saddlepoint", RHO)
    assert int(got[9]) & binary_sets.FLAG_SCALED
    for col, key in ((1, "burden_beta"), (2, "burden_se"), (3, "burden_chi2"), (4, "skat_q")):
        assert abs(got[col] - t[key]) < TOL * abs(t[key]), key
    assert abs(got[5] - t["skat_p"]) < PTOL * t["skat_p"] and abs(got[6] - t["skato"][0]) < PTOL * t["skato"][0]


def test_a_narrow_set_between_two_wide_ones_carries_the_bits_of_a_call_on_it_alone():
    p = BS._problem("pedigree")
    null = BS._null(p, 1, deterministic=True)
    wide = null.sets(block=16, cutoff=0.5, max_markers=64)
    plain = null.sets(block=16, cutoff=0.5)
    assert type(plain) is glmm.BinarySetTest
    narrow = [np.arange(23, 33), np.array([O.ASSOC[0], 60, 61])]
    sets = [np.arange(20, 53), narrow[0], np.arange(60, 110), narrow[1]]
    for finish, alone_finish in (("host", "host"), ("wide", "device")):
        out = wide(p["G"], sets, weights=None, skato=True, rho=RHO, finish=finish)
        rows = wide.last_bspa.copy()
        alone = plain(p["G"], narrow, weights=None, skato=True, rho=RHO, finish=alone_finish)
        assert sorted(out) == sorted(alone)
        for k in alone:
            assert np.array_equal(out[k][[1, 3]], alone[k], equal_nan=True), (finish, k)
        assert np.array_equal(rows[[1, 3]], plain.last_bspa, equal_nan=True)
        assert out["n_used"][0] == 33 and out["n_used"][2] == 50 and not np.any(np.isnan(out["skato_p"]))
    # a per-call max_markers overrides the constructor's, before any launch
    with pytest.raises(ValueError, match="more than max_markers = 32"):
        wide(p["G"], sets, max_markers=32)
    with pytest.raises(ValueError, match='needs finish="host" or finish="wide"'):
        wide(p["G"], sets, finish="device")


def test_two_runs_and_the_three_input_forms_give_the_same_bits(tmp_path):
    from scilmm_amd import dosage
    from tests.test_bed_api import pack, write_fileset
    p = BS._problem("sub100")
    tester = _wtester(p, 4, 16, 0.5, deterministic=True)
    sets = [s for _, s in _sets16(p, common=True)] + [np.arange(23, 33)]
    path = write_fileset(tmp_path / "cohort", pack(p["G"]), p["n"])
    codes = dosage.encode(np.where(p["G"] < 0, np.nan, p["G"].astype(np.float64)))
    assert codes.dtype == np.uint16
    for kw in (dict(skato=True, finish="wide"), dict(finish="host")):
        first = tester(p["G"], sets, **kw)
        rows = tester.last_bspa.copy()
        assert (first["burden_spa_flag"] == 1).sum() >= 3 and (first["n_adjusted"] > 0).sum() >= 3
        for again in (tester(p["G"], sets, **kw), tester.test_bed(path, sets, **kw), tester.test_dosages(codes, sets, **kw)):
            BS._same(again, first)
            assert np.array_equal(tester.last_bspa, rows, equal_nan=True)
    assert tester.sym.timing()["n_float_atomic_launches"] == 0


def test_refusals_fp32_fronts_and_a_distributed_handle(monkeypatch):
    import torch
    from scilmm_amd import ScilmmError, _lib
    from scilmm_amd.dist import HipChainEngine
    from scilmm_amd.factor import Symbolic
    from tests.helpers import rel_err
    from tests.test_gpu_halfsolve import _pedigree
    q = _pedigree()
    n = q["A"].shape[0]
    buf = torch.zeros((4096,), dtype=torch.float64, device="cuda")
    g8 = torch.zeros((n + 16,), dtype=torch.int8, device="cuda")
    b, g = vp(buf.data_ptr()), vp(g8.data_ptr())
    rho = np.array([0.0, 1.0])

    def calls(fac):
        return [lambda: fac.sets_collapse_dev(g, n, 1, b, 1, None, True, b),
                lambda: fac.sets_collapse_bed_dev(g, (n + 3) // 4, n, None, 0, 1, b, 1, None, True, b),
                lambda: fac.sets_collapse_dosage_dev(g, _lib.DOSAGE_U16, n, n, None, 1, b, 1, None, True, b),
                lambda: fac.sets_spa_wide_dev(5, 128, 2, b, b, None, 0, b, b, b, b, 1, b, 2.0, b, 1, None, b, b, b),
                lambda: fac.sets_finish_wide_scaled_dev(5, 128, 2, b, b, None, 0, b, b, 1, 1, None, 0, rho, b, None, b)]

    # one rank of a world of two, never factorized: the refusal comes before any device work
    eng = HipChainEngine([q["A"], q["I"]], 0, 2, None, "cuda:0")
    for call in calls(eng.fac):
        with pytest.raises(ScilmmError, match="distributed"):
            call()
    assert eng.collectives == 0
    # fp32-product fronts
    monkeypatch.setenv("SCILMM_TUNING", "1")
    monkeypatch.setenv("SCILMM_DENSE", "1")
    sym32 = Symbolic([q["A"], q["I"]])
    sym32.set_front_precision(32)
    f32 = sym32.factorize([0.35, 0.65])
    for call in calls(f32):
        with pytest.raises(ScilmmError, match="fp32"):
            call()
    Bm = np.random.default_rng(0).standard_normal((n, 2))
    assert rel_err(q["V"] @ f32(Bm), Bm) < 1e-9                            # the refusals left the handle as it was
