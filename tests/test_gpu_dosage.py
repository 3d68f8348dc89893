"""AssociationScan.scan_dosages / VariantSetTest.test_dosages / scilmm_scan_block_dosage_dev.

Hard calls against the int8 path at ZERO tolerance, derived and not measured.  uint16: the moments are integer sums of
g * 16384, scaled by powers of two (exact) and put through the two expressions of the int8 kernel (mean = sum / cnt,
css = sq - sum * mean), W holds (double)code * 2^-14 - mean = (double)g - mean, and everything behind W is the same launches,
which repeat their bits in deterministic mode.  float32: the fp64 sum of small integers is exact in any order, the mean is
the same quotient and W the same doubles; only css is rounded otherwise, and it is not returned (the rule min == max makes it
exactly 0 for the monomorphic marker).
Fractional dosages against a per-marker GLS written here with the dense inv(V) (the un-whitened formula of
tests/test_gpu_assoc.py, restated for real-valued markers) at that file's 1e-9 relative (max-norm, tests.helpers.rel_err);
n_obs exact; mean within 1e-15 relative of the exactly rounded sum (math.fsum) over n_obs -- the device sum is a tree of
depth <= 19 over positive terms whose top levels carry the error: about 1e-16.  Variant sets against the un-whitened burden /
SKAT statistics of tests/test_gpu_sets.py, restated, at that file's tolerances.
Problems, covariates, sigma2, hard-call markers and scan objects are those of tests/test_gpu_bed.py (shared, built once)."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.linalg
import scipy.stats as stats

from tests import test_gpu_bed as B
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-9
S2 = B.S2
KEYS = B.KEYS
M = 130                                              # fractional markers: a partial second block at width 128
CONST, EMPTY, FULL, ENDS, NARROW = 0, 1, 2, 3, 4     # the overwritten rows
SET_KEYS = ("n_used", "burden_beta", "burden_se", "burden_chi2", "burden_p", "skat_q", "skat_p")


def _codes(G):
    """Hard calls as uint16 codes: g * 16384, -1 -> 65535."""
    return np.ascontiguousarray(np.where(G >= 0, G.astype(np.int32) * 16384, 65535).astype(np.uint16))


def _floats(G):
    return np.ascontiguousarray(np.where(G >= 0, G, np.nan).astype(np.float32))


def _fractional(N, m, seed):
    """Dosages around binomial calls: call + (Beta(2, 2) - 1/2) / 2 clipped to [0, 2], MAF uniform 0.05-0.5, 2 % missing (NaN);
    five rows overwritten with the edge cases.  float64."""
    rng = np.random.default_rng(seed)
    maf = rng.uniform(0.05, 0.5, m)
    D = rng.binomial(2, maf[:, None], size=(m, N)) + 0.5 * (rng.beta(2.0, 2.0, size=(m, N)) - 0.5)
    D = np.clip(D, 0.0, 2.0)
    D[rng.random((m, N)) < 0.02] = np.nan
    D[CONST] = 0.7                                             # constant and fractional
    D[EMPTY] = np.nan                                          # nothing observed
    D[FULL] = np.clip(rng.binomial(2, 0.3, N) + 0.5 * (rng.beta(2.0, 2.0, N) - 0.5), 0.0, 2.0)   # no missing value
    D[ENDS] = D[FULL][::-1]
    D[ENDS, 0] = D[ENDS, -1] = np.nan                          # missing at the first and the last sample only
    D[NARROW] = 1.9 + rng.uniform(-0.01, 0.01, N)              # mean >> sd
    return D


def _forms(D):
    """dtype name -> (what goes to the device, what the oracle sees: the values the device decodes, in float64)."""
    from scilmm_amd.dosage import decode, encode
    codes, f32 = encode(D), np.ascontiguousarray(D.astype(np.float32))
    return {"u16": (codes, decode(codes)), "f32": (f32, f32.astype(np.float64))}


def _centred(D):
    """n_obs, mean (exactly rounded sum / n_obs), the centred markers with 0 for the missing, and the markers without an
    observed value or without variation (smallest observed value == largest)."""
    obs = np.isfinite(D)
    n_obs = obs.sum(axis=1)
    mean = np.array([math.fsum(row[o]) / k if k else np.nan for row, o, k in zip(D, obs, n_obs)])
    Dt = np.where(obs, D - np.where(n_obs > 0, mean, 0.0)[:, None], 0.0)
    flat = np.array([k == 0 or row[o].min() == row[o].max() for row, o, k in zip(D, obs, n_obs)])
    return n_obs, mean, Dt, flat


def _vi(p):
    if "vi" not in p:
        p["vi"] = np.linalg.inv((S2[0] * p["A"] + S2[1] * p["I"]).toarray())
    return p["vi"]


def _gls(p, D):
    """beta, se, chi2 of the last coefficient of GLS of y on [C, d~] under V, marker by marker."""
    Vi, Cv, y = _vi(p), p["C"], p["y"]
    n_obs, mean, Dt, flat = _centred(D)
    ViD, ViC, Viy = Vi @ Dt.T, Vi @ Cv, Vi @ y
    beta, se = np.full(len(D), np.nan), np.full(len(D), np.nan)
    for j in range(len(D)):
        if flat[j]:
            continue
        X = np.hstack([Cv, Dt[j][:, None]])
        XtViX = X.T @ np.hstack([ViC, ViD[:, j][:, None]])
        beta[j] = np.linalg.solve(XtViX, X.T @ Viy)[-1]
        se[j] = np.sqrt(np.linalg.inv(XtViX)[-1, -1])
    return dict(beta=beta, se=se, chi2=(beta / se) ** 2, n_obs=n_obs, mean=mean, flat=flat)


def _compare(out, ref, n):
    bad = ref["flat"]
    for k in ("beta", "se", "chi2"):
        print(k, "rel.err", rel_err(out[k][~bad], ref[k][~bad]))
        assert rel_err(out[k][~bad], ref[k][~bad]) < TOL, k
        assert np.array_equal(np.isnan(out[k]), bad), k            # NaN exactly at the degenerate markers
    assert np.array_equal(np.isnan(out["p"]), bad)
    assert np.array_equal(out["p"], stats.f(1, n - 1).sf(out["chi2"]), equal_nan=True)
    assert out["n_obs"].dtype.kind == "i" and np.array_equal(out["n_obs"], ref["n_obs"])
    ok = ref["n_obs"] > 0
    dm = np.abs(out["mean"][ok] - ref["mean"][ok]) / np.abs(ref["mean"][ok])
    print("mean rel.err", dm.max())
    assert dm.max() <= 1e-15 and np.all(np.isnan(out["mean"][~ok]))


def _frac(p):
    """The problem's fractional dosages in both forms, and their GLS reference, built once."""
    if "dos" not in p:
        p["dos"] = _forms(_fractional(p["n"], M, 31))
        p["dos_ref"] = {}
    return p["dos"]


def _frac_ref(p, form):
    _frac(p)
    if form not in p["dos_ref"]:
        p["dos_ref"][form] = _gls(p, p["dos"][form][1])
    return p["dos_ref"][form]


@pytest.mark.parametrize("block", [16, 128])
@pytest.mark.parametrize("name", ["spd301", "pedigree"])
def test_u16_hard_calls_give_the_bits_of_the_int8_path(name, block):
    """267 markers: three chunks of one block at width 128 (128 + 128 + 11), seventeen at width 16, the last one partial."""
    p = B._problem(name)
    n, G = p["n"], p["G3"]
    if name == "spd301":
        assert n % 8 == 5                                             # rows of pitch n start at every alignment
    codes = _codes(G)
    scan = B._scan(p, block)
    assert -(-len(G) // block) >= 3 and len(G) % block
    ref = scan(G)
    out = scan.scan_dosages(codes, chunk_bytes=block * n * 2)
    B._same(out, ref)
    assert np.array_equal(np.isnan(out["beta"][:4]), [True, True, False, False])
    assert np.array_equal(out["n_obs"], (G >= 0).sum(axis=1))
    B._same(scan.scan_dosages(codes), ref)                            # one chunk
    B._same(scan.scan_dosages(codes, chunk_bytes=1), ref)             # the smallest chunk is still one block
    assert scan.sym.timing()["n_float_atomic_launches"] == 0
    empty = scan.scan_dosages(codes[:0])
    assert sorted(empty) == sorted(KEYS) and all(v.shape == (0,) for v in empty.values())
    with pytest.raises(TypeError):
        scan(codes)                                                   # __call__ keeps refusing anything but int8


@pytest.mark.parametrize("block", [16, 128])
@pytest.mark.parametrize("name", ["spd301", "pedigree"])
def test_f32_hard_calls_give_the_bits_of_the_int8_path(name, block):
    p = B._problem(name)
    n, G = p["n"], p["G3"]
    scan = B._scan(p, block)
    ref = scan(G)
    out = scan.scan_dosages(_floats(G), chunk_bytes=block * n * 4)
    B._same(out, ref)
    assert np.array_equal(np.isnan(out["beta"][:4]), [True, True, False, False])      # min == max: the monomorphic marker
    B._same(scan.scan_dosages(_floats(G)), ref)
    inf = _floats(G)
    inf[np.isnan(inf)] = np.tile([np.inf, -np.inf], inf.size)[:np.isnan(inf).sum()]    # any non-finite value is missing
    B._same(scan.scan_dosages(inf), ref)
    assert scan.sym.timing()["n_float_atomic_launches"] == 0


def _block(scan, host, dtype, offset, ld, N, idx, r, torch, gram=False):
    """One block through the C entry point: `host` is a whole buffer of elements, the rows start `offset` elements into it
    and lie `ld` elements apart.  Returns the statistics (and the Gram matrix)."""
    from scilmm_amd import _lib
    q = scan.q
    kind = _lib.DOSAGE_U16 if dtype == np.uint16 else _lib.DOSAGE_F32
    raw = torch.from_numpy(host.view(np.uint8)).cuda()
    dI = None if idx is None else torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).cuda()
    dS = torch.zeros(((q + 4) * r,), dtype=torch.float64, device="cuda")
    dK = torch.zeros((r * r,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    vp = C.c_void_p
    args = (vp(raw.data_ptr() + offset * host.dtype.itemsize), kind, ld, N, None if dI is None else vp(dI.data_ptr()), r,
            vp(scan.dQ.data_ptr()), q, vp(dS.data_ptr()))
    if gram:
        scan.factor.scan_block_dosage_gram_dev(*(args + (vp(dK.data_ptr()),)))
    else:
        scan.factor.scan_block_dosage_dev(*args)
    scan.sym.sync()
    S = dS.cpu().numpy().reshape(q + 4, r)
    return (S, dK.cpu().numpy().reshape(r, r)) if gram else S


def _pitched(rows, ld, offset, fill):
    """`rows` laid out `ld` elements apart, `offset` elements into a buffer whose every other element is `fill` (an observed
    value: a kernel that counted an element between or around the rows would miscount)."""
    r, N = rows.shape
    host = np.full(offset + r * ld + 64, fill, dtype=rows.dtype)
    for j in range(r):
        host[offset + j * ld: offset + j * ld + N] = rows[j]
    return host


@pytest.mark.parametrize("name", ["spd301", "pedigree"])
def test_any_row_pitch_and_alignment_gives_the_same_bits(name):
    """Aligned 16-byte pieces whatever the pitch and the base address; ld = n + 3 and odd offsets put the rows at every
    element alignment inside a piece."""
    import torch
    p = B._problem(name)
    n = p["n"]
    scan = B._scan(p, 128)
    G = p["G"][:19]
    want = B._block_int8(scan, G, torch)
    assert np.array_equal(want[2] == 0, np.arange(19) < 2)
    for rows, fill, per in ((_codes(G), 16384, 8), (_floats(G), 1.0, 4)):
        pad = (n + per - 1) // per * per
        for ld, offset in ((pad, 0), (n, 0), (n, 3), (n + 3, 0), (n + 3, 1), (n + 5, per - 1)):
            S = _block(scan, _pitched(rows, ld, offset, fill), rows.dtype, offset, ld, n, None, 19, torch)
            rest = [0, 1] + list(range(3, len(S)))          # (css: rounded otherwise from floats; what matters is where it is 0)
            assert np.array_equal(S[rest], want[rest], equal_nan=True), (rows.dtype, ld, offset)
            assert np.array_equal(S[2] == 0, want[2] == 0), (rows.dtype, ld, offset)
    # uint16: css as well, bit for bit
    S = _block(scan, _pitched(_codes(G), n + 3, 1, 16384), np.uint16, 1, n + 3, n, None, 19, torch)
    assert np.array_equal(S, want, equal_nan=True)


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("form", ["u16", "f32"])
@pytest.mark.parametrize("name", ["spd301", "pedigree"])
def test_fractional_dosages_match_dense_gls(name, form, deterministic):
    p = B._problem(name)
    n = p["n"]
    dev, seen = _frac(p)[form]
    ref = _frac_ref(p, form)
    assert np.array_equal(np.flatnonzero(ref["flat"]), [CONST, EMPTY])
    assert ref["n_obs"][FULL] == n and ref["n_obs"][ENDS] == n - 2 and np.isnan(seen[ENDS, [0, -1]]).all()
    assert abs(ref["mean"][NARROW] - 1.9) < 1e-3 and np.nanstd(seen[NARROW]) < 0.01
    scan = B._scan(p, 128, deterministic)
    out = scan.scan_dosages(dev)
    _compare(out, ref, n)
    if deterministic:
        B._same(scan.scan_dosages(dev, chunk_bytes=1), out)          # the same bits block by block, and twice
        assert scan.sym.timing()["n_float_atomic_launches"] == 0
        _compare(B._scan(p, 16).scan_dosages(dev[:40]), {k: v[:40] for k, v in ref.items()}, n)


def _mapped(n, N, seed):
    """N samples in shuffled order for a cohort of n, about 3 % of the cohort absent."""
    rng = np.random.default_rng(seed)
    idx = rng.permutation(N)[:n].astype(np.int32)
    idx[rng.choice(n, size=max(1, (3 * n) // 100), replace=False)] = -1
    return idx


def _gather(Df, idx, missing):
    ok = (idx >= 0) & (idx < Df.shape[1])
    return np.ascontiguousarray(np.where(ok, Df[:, np.where(ok, idx, 0)], missing).astype(Df.dtype))


@pytest.mark.parametrize("name", ["spd301", "pedigree"])
def test_sample_map(name):
    import torch
    p = B._problem(name)
    n = p["n"]
    N = n + 37
    idx = _mapped(n, N, 5)
    assert (idx < 0).sum() >= 1 and (idx >= n).any()
    forms = _forms(_fractional(N, M, 41))
    scan = B._scan(p, 128)
    # uint16: integer sums, so the bits of the host-gathered matrix through the identity form
    codes = forms["u16"][0]
    gathered = _gather(codes, idx, 65535)
    ref = scan.scan_dosages(gathered)
    out = scan.scan_dosages(codes, sample_index=idx, chunk_bytes=1)
    B._same(out, ref)
    assert np.array_equal(out["n_obs"], (gathered <= 32768).sum(axis=1))
    B._same(scan.scan_dosages(codes, sample_index=idx.astype(np.int64)), ref)
    B._same(B._scan(p, 16).scan_dosages(codes[:40], sample_index=idx), B._scan(p, 16).scan_dosages(gathered[:40]))
    # float32: another summation order than the identity form's, so against the oracle; the same call repeats its bits
    f32, seen = forms["f32"]
    out = scan.scan_dosages(f32, sample_index=idx)
    _compare(out, _gls(p, _gather(seen, idx, np.nan)), n)
    B._same(scan.scan_dosages(f32, sample_index=idx), out)
    assert scan.sym.timing()["n_float_atomic_launches"] == 0
    # samples past the last one, which scan_dosages refuses on the host: through the C entry point they are missing
    here = np.flatnonzero(idx >= 0)
    far = idx.copy()
    far[here[2]], far[here[3]], far[here[4]] = N, 2 ** 31 - 1, -5
    for rows, missing in ((codes[:19], 65535), (f32[:19], np.nan)):
        got = _block(scan, rows.reshape(-1).copy(), rows.dtype, 0, N, N, far, 19, torch)
        g19 = _gather(rows, far, missing)
        want = _block(scan, _pitched(g19, n, 0, missing), rows.dtype, 0, n, n, None, 19, torch)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[0], np.isfinite(_forms_value(g19)).sum(axis=1))
        if rows.dtype == np.uint16:
            assert np.array_equal(got, want, equal_nan=True)
        else:
            live = want[2] != 0
            assert rel_err(got[1:, live], want[1:, live]) < TOL and np.array_equal(got[2] == 0, want[2] == 0)
    # refused before any launch
    ident = np.where(idx < 0, 0, idx)
    for bad in (ident[:-1], np.r_[ident, 0], np.where(np.arange(n) == 5, N, ident), np.where(np.arange(n) == 5, -2, ident),
                ident[None, :], ident.astype(float)):
        with pytest.raises(ValueError):
            scan.scan_dosages(codes, sample_index=bad)
    with pytest.raises(ValueError):
        scan.scan_dosages(codes)                                      # N != n without a map


def _forms_value(rows):
    from scilmm_amd.dosage import decode
    return decode(rows) if rows.dtype == np.uint16 else rows.astype(np.float64)


def test_stale_factor_and_consumed_factor_refuse():
    from scilmm_amd import AssociationScan, ScilmmError, SparseCholesky
    p = B._problem("spd301")
    codes = _codes(p["G"])
    chol = SparseCholesky(deterministic=True)
    scan = AssociationScan(chol, [p["A"], p["I"]], S2, p["C"], p["y"], block=16)
    B._same(scan.scan_dosages(codes), scan(p["G"]))
    other = AssociationScan(chol, [p["A"], p["I"]], [0.7, 0.3], p["C"], p["y"], block=16)
    assert other.factor is scan.factor                     # the resident factor was refactorized, not doubled
    with pytest.raises(ScilmmError, match="sigma2"):
        scan.scan_dosages(codes)                           # the first object's whitening belongs to the old factor
    with pytest.raises(ScilmmError, match="sigma2"):
        scan.scan_dosages(_floats(p["G"]))
    other.scan_dosages(codes)
    other.factor.inverse_traces()                          # consumes the factor
    with pytest.raises(ScilmmError):
        other.scan_dosages(codes)


# ---- variant sets


def _tester(p, deterministic):
    from scilmm_amd import SparseCholesky, VariantSetTest
    key = ("sets", deterministic)
    if key not in p["scans"]:
        p["scans"][key] = VariantSetTest(SparseCholesky(deterministic=deterministic), [p["A"], p["I"]], S2, p["C"], p["y"], block=128)
    return p["scans"][key]


def _sets(flat, empty):
    """Sizes 1, 5 and 128, and a set of five that holds the constant (or monomorphic) and the empty marker."""
    sets = [np.array([7]), np.arange(10, 15), np.arange(2, 130), np.array([flat, 20, 21, empty, 22])]
    assert [s.size for s in sets] == [1, 5, 128, 5]
    return sets


def _same_sets(x, y):
    for k in SET_KEYS:
        assert x[k].dtype == y[k].dtype and np.array_equal(x[k], y[k], equal_nan=True), k
    for (s, K, w), (s0, K0, w0) in zip(x["kernel"], y["kernel"]):
        assert np.array_equal(s, s0) and np.array_equal(K, K0) and np.array_equal(w, w0)


@pytest.mark.parametrize("name", ["spd301", "pedigree"])
def test_sets_of_u16_hard_calls_give_the_bits_of_the_int8_sets(name):
    p = B._problem(name)
    G = p["G"]
    tester, sets = _tester(p, True), _sets(B.MONO, B.ALLMISS)
    ref = tester(G, sets, return_kernel=True)
    out = tester.test_dosages(_codes(G), sets, return_kernel=True)
    assert sorted(out) == sorted(SET_KEYS + ("kernel",))
    _same_sets(out, ref)
    assert np.array_equal(out["n_used"], [1, 5, 128, 3])
    _same_sets(tester.test_dosages(_codes(G), sets, weights=None, method="liu", return_kernel=True),
               tester(G, sets, weights=None, method="liu", return_kernel=True))
    assert "kernel" not in tester.test_dosages(_codes(G), sets)
    none = tester.test_dosages(_codes(G), [])
    assert sorted(none) == sorted(SET_KEYS) and all(v.shape == (0,) for v in none.values())
    assert tester.sym.timing()["n_float_atomic_launches"] == 0


def _set_oracle(p, D, sets):
    """Per set: (s, K, w) over the markers that are left, the eigenvalues and every statistic, from the un-whitened formula
    with the explicit P = V^-1 - V^-1 C (C' V^-1 C)^-1 C' V^-1 (tests/test_gpu_sets.py)."""
    from scilmm_amd import sets as mod
    if "P" not in p:
        Vi, Cv = _vi(p), p["C"]
        ViC = Vi @ Cv
        p["P"] = Vi - ViC @ np.linalg.solve(Cv.T @ ViC, ViC.T)
    P, y, n = p["P"], p["y"], p["n"]
    _, mean, Dt, flat = _centred(D)
    ref = {k: np.full(len(sets), np.nan) for k in SET_KEYS}
    ref["n_used"] = np.zeros(len(sets), dtype=np.int64)
    ref["kernel"], ref["lam"] = [], []
    for i, rows in enumerate(sets):
        rows = np.array([j for j in rows if not flat[j]], dtype=np.int64)
        X = Dt[rows]
        s, K = X @ (P @ y), X @ P @ X.T
        w = stats.beta.pdf(np.minimum(mean[rows] / 2, 1 - mean[rows] / 2), 1, 25)
        ref["kernel"].append((s, K, w))
        ref["n_used"][i] = rows.size
        lam = np.linalg.eigvalsh(w[:, None] * K * w[None, :])
        ref["lam"].append(lam)
        ws, wKw = w @ s, w @ K @ w
        ref["burden_beta"][i], ref["burden_se"][i], ref["burden_chi2"][i] = ws / wKw, wKw ** -0.5, ws * ws / wKw
        ref["burden_p"][i] = stats.f(1, n - 1).sf(ws * ws / wKw)
        ref["skat_q"][i] = np.sum(w * w * s * s)
        ref["skat_p"][i] = mod.mixture_sf_saddlepoint(ref["skat_q"][i], lam[lam > 1e-10 * lam.max()])
    return ref


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("form", ["u16", "f32"])
@pytest.mark.parametrize("name", ["spd301", "pedigree"])
def test_sets_of_fractional_dosages_match_the_unwhitened_formula(name, form, deterministic):
    from scilmm_amd import sets as mod
    p = B._problem(name)
    n = p["n"]
    dev, seen = _frac(p)[form]
    sets = _sets(CONST, EMPTY)
    key = ("set_ref", form)
    if key not in p["ref"]:
        p["ref"][key] = _set_oracle(p, seen, sets)
    ref = p["ref"][key]
    out = _tester(p, deterministic).test_dosages(dev, sets, return_kernel=True)
    assert out["n_used"].dtype.kind == "i" and np.array_equal(out["n_used"], ref["n_used"])
    assert np.array_equal(out["n_used"], [1, 5, 128, 3])               # the constant and the empty marker are dropped
    for k in ("burden_beta", "burden_se", "burden_chi2", "skat_q"):
        print(k, "rel.err", rel_err(out[k], ref[k]))
        assert rel_err(out[k], ref[k]) < TOL, k
    for i, ((s, K, w), (s0, K0, w0)) in enumerate(zip(out["kernel"], ref["kernel"])):
        assert s.shape == s0.shape and K.shape == K0.shape and w.shape == w0.shape, i
        assert rel_err(s, s0) < TOL and rel_err(K, K0) < TOL and rel_err(w, w0) < TOL, (i, rel_err(s, s0), rel_err(K, K0))
        assert np.array_equal(K, K.T), i
        lam = scipy.linalg.eigvalsh(w[:, None] * K * w[None, :])
        assert rel_err(lam, ref["lam"][i]) < TOL, (i, rel_err(lam, ref["lam"][i]))
        assert out["burden_p"][i] == stats.f(1, n - 1).sf(out["burden_chi2"][i]), i
        assert out["skat_p"][i] == mod.mixture_sf_saddlepoint(out["skat_q"][i], lam[lam > 1e-10 * lam.max()]), i
    for k in ("burden_p", "skat_p"):
        d = np.abs(out[k] - ref[k]) / ref[k]
        print(k, "max rel. deviation from the reference p", d.max())
        assert d.max() < 1e-6, k


def test_gram_entry_point_with_a_map_and_its_refusals():
    """The Gram form at the C level: the statistics are the bits of the plain form, the matrix is symmetric bit for bit;
    argument errors on a live handle."""
    import torch
    from scilmm_amd import _lib
    p = B._problem("spd301")
    n = p["n"]
    N = n + 37
    idx = _mapped(n, N, 6)
    tester = _tester(p, True)
    for form, (dev, _) in _forms(_fractional(N, 19, 43)).items():
        S, K = _block(tester, dev.reshape(-1).copy(), dev.dtype, 0, N, N, idx, 19, torch, gram=True)
        S0 = _block(tester, dev.reshape(-1).copy(), dev.dtype, 0, N, N, idx, 19, torch)
        assert np.array_equal(S, S0, equal_nan=True), form
        assert np.array_equal(K, K.T) and rel_err(np.diag(K), S[3]) < 1e-12, form
    L, one, h = _lib.lib(), C.c_void_p(8), tester.factor._h
    f, g = L.scilmm_scan_block_dosage_dev, L.scilmm_scan_block_dosage_gram_dev
    for dtype in (_lib.DOSAGE_U16, _lib.DOSAGE_F32):
        assert g(h, one, dtype, n, n, None, 4, one, 2, one, None) == _lib.ERR_ARG                 # a null d_gram
        for Ns in (n - 1, n + 1):
            assert f(h, one, dtype, n + 1, Ns, None, 4, one, 2, one) == _lib.ERR_ARG              # identity map with N != n
            assert g(h, one, dtype, n + 1, Ns, None, 4, one, 2, one, one) == _lib.ERR_ARG
        assert f(h, one, dtype, n - 1, n, None, 4, one, 2, one) == _lib.ERR_ARG                   # pitch shorter than a row
        assert f(h, C.c_void_p(9), dtype, n, n, None, 4, one, 2, one) == _lib.ERR_ARG             # a misaligned base
    assert f(h, one, 2, n, n, None, 4, one, 2, one) == _lib.ERR_ARG                               # an unknown element type
