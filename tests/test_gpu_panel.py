"""Phenotype panels on the device (scilmm_amd.panel, scilmm_scan_panel_dev) against the dense un-whitened GLS oracle
(tests/panel_oracle.py), against the scan itself, and the kernel alone against the public half-solve.

Tolerances: 1e-9 relative (max-norm, tests.helpers.rel_err) against the dense oracle, what the suite holds for the scan; 1e-12
between the panel of one trait and the scan and between X'Y and the half-solve reference (another summation order only; what
tests/test_gpu_sets.py holds between the Gram diagonal and |x|^2); bit identity where the issue is the order of a sum."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.stats as stats

from tests import panel_oracle as O
from tests.helpers import random_spd, rel_err, small_pedigree

pytestmark = pytest.mark.gpu

TOL = 1e-9
M = 130                      # markers: partial last blocks at every block width below
TMAXT = 130                  # traits of the widest panel: across the 128-column panel boundary
S2 = [0.4, 0.6]
PANEL_SLICE = 2048           # csrc/panel.hip.h
vp = C.c_void_p

_PROBLEMS = {}


def _problem(name):
    """(A, I, markers, covariates, y, traits) and the oracle's results per (c, scale), built once."""
    if name not in _PROBLEMS:
        A = small_pedigree(2000, 0.01, 0)[0] if name == "pedigree" else random_spd(300, 0.05, 3)
        n = A.shape[0]
        rng = np.random.default_rng(11)
        Cv = np.hstack([np.ones((n, 1)), rng.standard_normal((n, 3))])
        y = Cv @ np.array([0.5, -0.2, 0.1, 0.3]) + rng.standard_normal(n)
        _PROBLEMS[name] = dict(A=A, I=sp.identity(n, format="csr"), n=n, C=Cv, y=y, G=O.markers(n, M, 7), Y=O.traits(n, Cv, TMAXT, 5),
                               ref={})
    return _PROBLEMS[name]


def _oracle(p, c, scale):
    if (c, scale) not in p["ref"]:
        if "vi" not in p:
            p["vi"] = np.linalg.inv((S2[0] * p["A"] + S2[1] * p["I"]).toarray())
        p["ref"][c, scale] = O.gls(p["vi"], p["C"][:, :c], p["Y"], p["G"], scale)
    return p["ref"][c, scale]


def _scan(p, c, block=None, **kw):
    from scilmm_amd import AssociationScan, SparseCholesky
    return AssociationScan(SparseCholesky(**kw), [p["A"], p["I"]], S2, p["C"][:, :c], p["y"], block=block)


def _same_bits(a, b, keys=None):
    for k in (keys or a):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("block", [16, 112, 128])
@pytest.mark.parametrize("c", [1, 4])
@pytest.mark.parametrize("name", ["pedigree", "spd300"])
def test_panel_matches_dense_gls(name, c, block):
    """T = 1 (a single column), 17 (a partial 16-tile) and 130 (across the 128-column panel boundary), both scales, on one scan
    per case: the oracle's columns 0 .. T - 1."""
    p = _problem(name)
    scan = _scan(p, c, block)
    bad = np.zeros(M, bool)
    bad[[O.MONO, O.ALLMISS]] = True
    for scale in ("fixed", "profile"):
        ref = _oracle(p, c, scale)
        for T in (1, 17, TMAXT):
            out = scan.traits(p["Y"][:, :T], scale=scale)(p["G"])
            for k in ("beta", "se", "chi2"):
                assert out[k].shape == (M, T)
                print(name, c, block, scale, T, k, "rel.err", rel_err(out[k][~bad], ref[k][~bad, :T]))
                assert rel_err(out[k][~bad], ref[k][~bad, :T]) < TOL, (scale, T, k)
                assert np.array_equal(np.isnan(out[k]), np.repeat(bad[:, None], T, axis=1)), (scale, T, k)   # NaN on the two degenerate rows only
            assert np.array_equal(out["p"], stats.f(1, p["n"] - 1).sf(out["chi2"]), equal_nan=True)
            assert out["n_obs"].dtype.kind == "i" and np.array_equal(out["n_obs"], ref["n_obs"])
            if scale == "profile":
                assert rel_err(out["scale"], ref["scale"][:T]) < TOL


@pytest.mark.parametrize("name", ["pedigree", "spd300"])
def test_one_trait_is_the_scan(name):
    p = _problem(name)
    scan = _scan(p, 4, 112)
    ref = scan(p["G"])
    out = scan.traits(p["y"][:, None])(p["G"])
    ok = ~np.isnan(ref["beta"])
    for k in ("beta", "se", "chi2"):
        print(name, k, "rel.diff", rel_err(out[k][ok, 0], ref[k][ok]))
        assert rel_err(out[k][ok, 0], ref[k][ok]) < 1e-12, k
        assert np.array_equal(np.isnan(out[k][:, 0]), ~ok), k
    _same_bits(out, ref, ("n_obs", "mean"))


def test_a_traits_bits_do_not_depend_on_its_panel():
    """Deterministic mode: one trait alone (T = 1) and at positions 0, 77 and 129 of a 130-column panel; two runs; no launch
    that sums with floating-point atomics over the whole panel scan."""
    p = _problem("pedigree")
    scan = _scan(p, 4, 112, deterministic=True)
    y = p["Y"][:, 5]
    alone = scan.traits(y[:, None], scale="profile")(p["G"])
    for pos in (0, 77, 129):
        Y = p["Y"].copy()
        Y[:, pos] = y
        panel = scan.traits(Y, scale="profile")
        out, again = panel(p["G"]), panel(p["G"])
        _same_bits(out, again)
        for k in ("beta", "se", "chi2", "p"):
            assert np.array_equal(out[k][:, pos], alone[k][:, 0], equal_nan=True), (pos, k)
        assert out["scale"][pos] == alone["scale"][0]
        _same_bits(out, alone, ("n_obs", "mean"))
    assert scan.sym.timing()["n_float_atomic_launches"] == 0


def _block(scan, dG, ld, r, torch):
    dS = torch.zeros(((scan.q + 4) * r,), dtype=torch.float64, device="cuda")
    scan.factor.scan_block_dev(vp(dG.data_ptr()), ld, r, vp(scan.dQ.data_ptr()), scan.q, vp(dS.data_ptr()))
    return dS


def _slices_problem():
    """Three row slices with a ragged end: n = 2 PANEL_SLICE + 7 (n mod 4 = 3, n mod 16 != 0); 128 markers that all vary (the
    four edge cases dropped: the block of r = 1 is no zero column)."""
    if "slices" not in _PROBLEMS:
        n = 2 * PANEL_SLICE + 7
        A = random_spd(n, 0.0005, 9)
        rng = np.random.default_rng(3)
        _PROBLEMS["slices"] = dict(A=A, I=sp.identity(n, format="csr"), n=n, C=np.ones((n, 1)), y=rng.standard_normal(n),
                                   G=O.markers(n, 132, 4)[4:], Yp=rng.standard_normal((n, TMAXT)))
    return _PROBLEMS["slices"]


def test_kernel_across_slices_against_the_half_solve():
    """scilmm_scan_panel_dev behind one int8 block of r markers against X_ref' Yp, X_ref = solve_L(apply_P(G~')) through the
    public half-solve: nothing of the new code is in the reference.  ld_out = t + 3 with a canary in the spare columns and in
    row r; NaN in Y's padding columns."""
    import torch
    p = _slices_problem()
    n = p["n"]
    assert n % 4 == 3 and n % 16 != 0 and (n + PANEL_SLICE - 1) // PANEL_SLICE == 3
    scan = _scan(p, 1, 128)
    fac = scan.factor
    ld = (n + 15) // 16 * 16
    dG = torch.zeros((128, ld), dtype=torch.int8, device="cuda")
    dG[:, :n].copy_(torch.from_numpy(p["G"]))
    _, _, Gt = O.centred(p["G"])
    Xref = fac.solve_L(fac.apply_P(np.ascontiguousarray(Gt.T)))                   # n x 128
    for r in (1, 19, 128):
        for t in (1, TMAXT):
            ld_y, ld_out = (t + 15) // 16 * 16, t + 3
            dY = torch.full((n, ld_y), float("nan"), dtype=torch.float64, device="cuda")
            dY[:, :t] = torch.from_numpy(p["Yp"][:, :t]).cuda()
            dO = torch.full((r + 1, ld_out), 7.25, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            dS = _block(scan, dG, ld, r, torch)                 # (kept until the stream has been waited for)
            fac.scan_panel_dev(r, vp(dY.data_ptr()), ld_y, t, vp(dO.data_ptr()), ld_out)
            scan.sym.sync()
            out, stat = dO.cpu().numpy(), dS.cpu().numpy().reshape(scan.q + 4, r)
            assert np.array_equal(stat[0], O.centred(p["G"][:r])[0])      # (the block itself ran as ever)
            ref = Xref[:, :r].T @ p["Yp"][:, :t]
            assert np.all(np.isfinite(out))
            print("r", r, "t", t, "rel.err", rel_err(out[:r, :t], ref))
            assert rel_err(out[:r, :t], ref) < 1e-12 and np.abs(ref).min() > 0.0, (r, t)
            assert np.all(out[:r, t:] == 7.25) and np.all(out[r] == 7.25), (r, t)
            assert all(ms >= 0.0 for ms in scan.sym.panel_timing())


def test_the_block_left_behind_is_tracked():
    import torch
    from scilmm_amd import ScilmmError
    p = _problem("spd300")
    n = p["n"]
    scan = _scan(p, 1, 128, deterministic=True)          # (the last assertion compares the bits of two sweeps)
    fac = scan.factor
    ld = (n + 15) // 16 * 16
    dG = torch.zeros((19, ld), dtype=torch.int8, device="cuda")
    dG[:, :n].copy_(torch.from_numpy(p["G"][4:23]))
    dY = torch.ones((n, 16), dtype=torch.float64, device="cuda")
    dO = torch.zeros((19, 1), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    panel = lambda r: fac.scan_panel_dev(r, vp(dY.data_ptr()), 16, 1, vp(dO.data_ptr()), 1)
    with pytest.raises(ScilmmError, match="no scan block"):
        panel(19)                                        # nothing has run yet
    dS = _block(scan, dG, ld, 19, torch)
    with pytest.raises(ScilmmError, match="19 columns"):
        panel(18)                                        # another r than the block's
    panel(19)
    panel(19)                                            # (a panel writes nothing of the work buffers: the block is still there)
    scan.sym.sync()
    first = dO.cpu().numpy().copy()
    fac.solve_L(np.zeros(n))                             # overwrites the work buffers
    with pytest.raises(ScilmmError, match="no scan block"):
        panel(19)
    dS = _block(scan, dG, ld, 19, torch)                 # a fresh block: the handle is as usable as ever
    dO.zero_()
    panel(19)
    scan.sym.sync()
    assert np.array_equal(dO.cpu().numpy(), first) and np.all(first != 0.0) and dS is not None
    fac.refactorize(S2)                                  # the block in X belongs to the factor that was replaced
    with pytest.raises(ScilmmError, match="no scan block"):
        panel(19)


def test_bed_and_dosage_forms_give_the_bits_of_int8(tmp_path):
    from scilmm_amd import dosage
    from tests.test_bed_api import pack, write_fileset
    p = _problem("spd300")
    n = p["n"]
    scan = _scan(p, 4, 16, deterministic=True)
    panel = scan.traits(p["Y"][:, :17], scale="profile")
    G = p["G"][:37]
    ref = panel(G)
    path = write_fileset(tmp_path / "cohort", pack(G), n)
    _same_bits(panel.scan_bed(path), ref)
    codes = dosage.encode(np.where(G < 0, np.nan, G.astype(np.float64)))
    assert codes.dtype == np.uint16
    _same_bits(panel.scan_dosages(codes), ref)
    mx = panel(G, reduce="max")
    _same_bits(panel.scan_bed(path, reduce="max"), mx)
    _same_bits(panel.scan_dosages(codes, reduce="max"), mx)


def test_reduce_max_is_the_column_maximum(monkeypatch):
    """One chunk, then chunks of two blocks (``panel._PANEL_BYTES`` is read at call time): the running maximum and its marker."""
    from scilmm_amd import panel as panel_mod
    p = _problem("spd300")
    scan = _scan(p, 4, 16)
    for scale in ("fixed", "profile"):
        panel = scan.traits(p["Y"], scale=scale)
        full = panel(p["G"])
        want, where = np.nanmax(full["chi2"], axis=0), np.nanargmax(full["chi2"], axis=0)
        for rows in (None, 32):
            if rows:
                monkeypatch.setattr(panel_mod, "_PANEL_BYTES", 8 * TMAXT * rows)
            mx = panel(p["G"], reduce="max")
            assert set(mx) == {"max_chi2", "argmax", "n_tested"}
            assert mx["max_chi2"].shape == (TMAXT,) and mx["argmax"].shape == (TMAXT,) and mx["argmax"].dtype == np.int64
            print(scale, rows, "rel.diff", rel_err(mx["max_chi2"], want))
            assert rel_err(mx["max_chi2"], want) < 1e-12
            assert np.array_equal(mx["argmax"], where)
            assert mx["n_tested"] == M - 2
        monkeypatch.undo()
    with pytest.raises(ValueError):
        panel(p["G"], reduce="min")


def test_null_panel():
    """The same seed gives the same bits, another seed other values; with one non-degenerate marker the statistic is exactly
    chi2(1) under scale="fixed": the mean of 4096 draws (32 column panels) lies in 1 +- 0.11 = five standard errors (sqrt(2) / 64
    each)."""
    from scilmm_amd import panel_thresholds
    p = _problem("spd300")
    scan = _scan(p, 4, 16)
    G = p["G"][:23]
    a = scan.null_panel(n_rep=50, seed=3)(G, reduce="max")
    b = scan.null_panel(n_rep=50, seed=3)(G, reduce="max")
    c = scan.null_panel(n_rep=50, seed=4)(G, reduce="max")
    _same_bits(a, b)
    assert not np.any(a["max_chi2"] == c["max_chi2"])
    assert a["n_tested"] == 21
    thr = panel_thresholds(a["max_chi2"], scan.n, alpha=0.1)
    assert thr["chi2"] in a["max_chi2"] and thr["m_eff"] == 0.1 / thr["p"]
    one = scan.null_panel(n_rep=4096, seed=0)(p["G"][[O.MONO, O.FULL]], reduce="max")
    assert one["n_tested"] == 1 and np.all(one["argmax"] == 1)
    print("mean of 4096 null chi2(1):", one["max_chi2"].mean())
    assert abs(one["max_chi2"].mean() - 1.0) < 0.11
    with pytest.raises(ValueError):
        scan.null_panel(n_rep=4097)
