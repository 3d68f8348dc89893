"""scilmm_sets_finish_wide_dev and VariantSetTest(..., finish="wide") against the host finish of the same inputs and, for the
sets of one block, against scilmm_sets_finish_dev.

Tolerances are those of tests/test_gpu_skato.py, whose helpers compare the rows: the eigenvalues within 1e-9 of the largest one
of LAPACK's; the burden numbers and skat_q 1e-9 relative; every p-value 1e-6 relative; skato_rho and n_used exact; no flag for an
iteration that ran out of steps.  At the C level the statistics and the Gram matrix are made up and cut by the test into the
slices and the cross store the entry point reads; whatever the entry point must not read -- the padding columns of the cross
store, the rest of a ragged slice -- is NaN, so that a stray read shows in the result.  No set is wider than 300 markers: m = 2
(no step behind the pre-step) and m = 3 (one step) are the smallest shapes at which the reduction can go wrong, 129 .. 300 take
more than one workgroup of every kernel and every ragged edge of the row tiles (8 rows) and of the waves (64 columns).

Worst deviations measured on an MI355X when this was written (printed by the tests with -s), device against host: eigenvalues
4.2e-15 of the largest, burden numbers and skat_q 4.6e-15, p-values 6.5e-12 at the C level (the 1'A1 = 0 set; 4.1e-12 over
several sub-blocks) and 2.7e-12 end to end; the wide against the narrow device finish 2.4e-12."""
import ctypes as C

import numpy as np
import pytest

from tests import test_bed_api as T
from tests import test_gpu_sets as GS
from tests import test_gpu_skato as GK
from tests.test_gpu_dosage import _codes
from tests.test_sets_wide_api import wide_sets

pytestmark = pytest.mark.gpu

HEAD, RHO, SENT, vp = GK.HEAD, GK.RHO, GK.SENT, C.c_void_p
CANARY = -7.25e30


def _cut(S, G, block, pad=np.nan, extra=0):
    """The (c + 5) x k statistics and the k x k matrix X'X cut into what the sub-blocks leave behind: the slices of the
    statistics and of the diagonal blocks, and the cross store (row i: the b bp columns of the kept sub-blocks before its own),
    everything else filled with `pad`; ld_cross = (B - 1) bp + extra."""
    k, rows = S.shape[1], S.shape[0]
    B, bp = -(-k // block), (block + 15) // 16 * 16
    ld = (B - 1) * bp + extra
    st, gr = np.full(B * rows * block, pad), np.full(B * block * block, pad)
    cr = np.full((k, max(ld, 1)), pad)
    for b in range(B):
        r0 = b * block
        rb = min(block, k - r0)
        st[b * rows * block:b * rows * block + rows * rb] = S[:, r0:r0 + rb].ravel()
        gr[b * block * block:b * block * block + rb * rb] = G[r0:r0 + rb, r0:r0 + rb].ravel()
        for a in range(b):
            cr[r0:r0 + rb, a * bp:a * bp + block] = G[r0:r0 + rb, a * block:(a + 1) * block]
    return st, gr, (cr if B > 1 else None), ld


def _wide(fac, sym, torch, S, G, R, u, block, mode=1, weights=None, method=0, rho=RHO, lam=True, pad=np.nan, extra=0):
    """One call of scilmm_sets_finish_wide_dev on sentinel-filled outputs: (row, lam); exactly the documented doubles are written."""
    q, k = S.shape[0] - 4, S.shape[1]
    st, gr, cr, ld = _cut(S, G, block, pad, extra)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    dS, dG, dR, du = dev(st), dev(gr), dev(R), dev(u)
    dX = dev(cr) if cr is not None else None
    dW = dev(weights) if weights is not None else None
    n = HEAD + len(rho)
    dO = torch.full((n + 5,), SENT, dtype=torch.float64, device="cuda")
    dL = torch.full((k + 5,), SENT, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    fac.sets_finish_wide_dev(k, block, q, vp(dS.data_ptr()), vp(dG.data_ptr()), vp(dX.data_ptr()) if dX is not None else None, ld,
                             vp(dR.data_ptr()), vp(du.data_ptr()), q - 1, mode, vp(dW.data_ptr()) if dW is not None else None, method, rho,
                             vp(dO.data_ptr()), vp(dL.data_ptr()) if lam else None)
    sym.sync()
    O_, L_ = dO.cpu().numpy(), dL.cpu().numpy()
    assert np.all(O_[n:] == SENT) and not np.any(O_[:n] == SENT)
    assert np.all(L_[k:] == SENT) and (np.all(L_ == SENT) if not lam else not np.any(L_[:k] == SENT))
    return O_[:n].reshape(1, n), L_[:k]


def _host(S, G, R, u, weights, method, rho):
    """The host finish of one set that spans the whole block, and its eigenvalues in the layout of the wide d_lam: descending,
    then NaN."""
    k = S.shape[1]
    rows, lam = GK._host_rows(S, G, R, u, np.array([0, k], dtype=np.int32), weights, method, rho)
    vals = np.sort(lam[~np.isnan(lam)])[::-1]
    out = np.full(k, np.nan)
    out[:vals.size] = vals
    return rows, out


_GOOD = []


def _compare(row, host, lam, lam_h, what, worst):
    """GK._compare_rows; where a burden number of the host is not finite (1'A1 = 0 exactly) the helper wants a row beside it
    that is: the first row that passed stands there once more."""
    if not np.all(np.isfinite(host[:, 1:5])) and _GOOD:
        g = _GOOD[0]
        row, host = np.vstack([g[0], row]), np.vstack([g[1], host])
        if lam is not None:
            lam, lam_h = np.r_[g[2], lam], np.r_[g[3], lam_h]
    GK._compare_rows(row, host, lam, lam_h, what, worst)
    if not _GOOD and lam is not None:
        _GOOD.append((row, host, lam, lam_h))


def _one(name, K, s, exact=False, dropped=()):
    return (name, K, s, exact, dropped)


def _block_of(member, st, seed=1):
    return GK._made_up_block([member], np.random.default_rng(seed), st["R"], st["u"])


def test_one_sub_block_matches_the_host_finish_and_the_narrow_device_finish():
    import torch
    st = GK._c_level()
    fac, sym = st["tester"].factor, st["tester"].sym
    n0 = sym.timing()["n_float_atomic_launches"]
    worst, against_narrow = {}, {}
    for name, member in st["made"].items():
        S, G, start = _block_of(member, st)
        k = S.shape[1]
        host, lam_h = _host(S, G, st["R"], st["u"], None, "saddlepoint", RHO)
        row, lam = _wide(fac, sym, torch, S, G, st["R"], st["u"], 128)
        _compare(row, host, lam, lam_h, name, worst)
        narrow, lam_n = GK._finish(fac, sym, torch, S, G, st["R"], st["u"], start)
        vals = np.sort(lam_n[~np.isnan(lam_n)])[::-1]
        lam_n = np.r_[vals, np.full(k - vals.size, np.nan)]
        _compare(row, narrow, lam, lam_n, name + " (narrow)", against_narrow)
        assert row[0, 9] == narrow[0, 9], (name, row[0, 9], narrow[0, 9])       # the same flags: degenerate, SKAT-O
        deg = name in ("psd1", "rank_one9", "s11_zero8")
        assert int(row[0, 9]) & 8 and bool(int(row[0, 9]) & 1) == deg, (name, row[0, 9])
        # the same set as sub-blocks of 16 and of 1 (k sub-blocks of one marker, where the panel limit allows it)
        for block in (16, 1):
            if k > block and (-(-k // block) - 1) * 16 <= 4096:
                again, lam2 = _wide(fac, sym, torch, S, G, st["R"], st["u"], block)
                _compare(again, host, lam2, lam_h, "%s block %d" % (name, block), worst)
    print("worst deviations, wide finish against host finish:", worst, "against the narrow device finish:", against_narrow)
    # the other tail, the other weight modes, no SKAT-O, no d_lam, another grid: on a set of 65 with three dropped markers
    rng = np.random.default_rng(31)
    K = GK._psd(rng, 62)
    ev, U = np.linalg.eigh(K)
    member = _one("psd62of65", K, (U * np.sqrt(ev)) @ rng.standard_normal(62), False, (0, 31, 64))
    S, G, _ = _block_of(member, st)
    w = rng.uniform(0.5, 2.0, 65)
    for what, kw, hw, hm in (("liu", dict(method=1), None, "liu"), ("given weights", dict(mode=2, weights=w), w, "saddlepoint"),
                             ("beta weights", dict(mode=0), "beta", "saddlepoint")):
        for block in (128, 16):
            row, lam = _wide(fac, sym, torch, S, G, st["R"], st["u"], block, **kw)
            host, lam_h = _host(S, G, st["R"], st["u"], hw, hm, RHO)
            assert row[0, 0] == 62
            _compare(row, host, lam, lam_h, "%s block %d" % (what, block), worst)
    host, _ = _host(S, G, st["R"], st["u"], None, "saddlepoint", RHO)
    row, _ = _wide(fac, sym, torch, S, G, st["R"], st["u"], 16, rho=np.empty(0), lam=False)
    _compare(row, host[:, :HEAD], None, None, "no SKAT-O", worst)
    grid = np.array([0.0, 0.3, 1.0])
    row, _ = _wide(fac, sym, torch, S, G, st["R"], st["u"], 16, rho=grid)
    _compare(row, _host(S, G, st["R"], st["u"], None, "saddlepoint", grid)[0], None, None, "three grid values", worst)
    assert sym.timing()["n_float_atomic_launches"] == n0


def _wide_members():
    """(name, K, s, exact, dropped, block): positive semidefinite K at k = 33 and 50 (block 16), 129, 257 and 300 (block 128; the
    last of rank 120 with two identical columns), 225 at block 112 (two whole sub-blocks and a ragged third of one marker),
    dropped markers in different sub-blocks, one marker left, nothing left."""
    rng = np.random.default_rng(2022)

    def null_t(K, signal=0.0):
        ev, U = np.linalg.eigh(K)
        return (U * np.sqrt(np.maximum(ev, 0.0))) @ rng.standard_normal(K.shape[0]) + signal * np.sqrt(np.diag(K))

    out = []
    for k, block in ((33, 16), (50, 16), (129, 128), (257, 128), (225, 112)):
        K = GK._psd(rng, k)
        out.append(_one("psd%d" % k, K, null_t(K, 0.3 * (k % 2)), False, ()) + (block,))
    Z = rng.standard_normal((120, 300)) * rng.uniform(0.3, 1.7, 300)
    Z[:, 211] = Z[:, 7]                                         # two identical columns, in different sub-blocks
    K = Z.T @ Z
    out.append(_one("rank120of300", K, null_t(K), False, ()) + (128,))
    K = GK._psd(rng, 46)
    out.append(_one("dropped50", K, null_t(K, 0.2), False, (0, 15, 16, 49)) + (16,))
    K = GK._psd(rng, 137)
    out.append(_one("dropped140", K, null_t(K), False, (5, 127, 139)) + (128,))
    out.append(_one("one_left20", np.array([[1.7]]), np.array([2.2]), False, tuple(j for j in range(20) if j != 17)) + (16,))
    out.append(_one("none_left20", np.zeros((0, 0)), np.zeros(0), False, tuple(range(20))) + (16,))
    return out


def test_several_sub_blocks_match_the_host_finish():
    import torch
    st = GK._c_level()
    fac, sym = st["tester"].factor, st["tester"].sym
    worst, rows = {}, {}
    for member in _wide_members():
        name, block = member[0], member[5]
        S, G, _ = _block_of(member[:5], st)
        k = S.shape[1]
        assert k > block
        host, lam_h = _host(S, G, st["R"], st["u"], None, "saddlepoint", RHO)
        row, lam = _wide(fac, sym, torch, S, G, st["R"], st["u"], block)
        rows[name] = (S, G, block, row, lam)
        assert row[0, 0] == k - len(member[4])
        if name == "none_left20":
            assert np.all(np.isnan(lam)) and np.all(np.isnan(row[0, 1:9])) and row[0, 9] == 0 and np.all(np.isnan(row[0, HEAD:]))
            continue
        _compare(row, host, lam, lam_h, name, worst)
        assert bool(int(row[0, 9]) & 1) == (name == "one_left20"), (name, row[0, 9])
    print("worst deviations, wide finish on several sub-blocks against host finish:", worst)
    # the padding columns of the cross store and the rest of the ragged slices hold something finite instead of NaN, and the rows
    # of the store are further apart: not a bit changes
    for name in ("psd225", "psd33"):
        S, G, block, row, lam = rows[name]
        again, lam2 = _wide(fac, sym, torch, S, G, st["R"], st["u"], block, pad=CANARY, extra=48)
        assert np.array_equal(again, row) and np.array_equal(lam2, lam), name
    # the work space is the handle's: a set gives the same bits behind a wider one and behind a narrower one
    for name in ("psd33", "psd257", "dropped50", "rank120of300", "psd33"):
        S, G, block, row, lam = rows[name]
        again, lam2 = _wide(fac, sym, torch, S, G, st["R"], st["u"], block)
        assert np.array_equal(again, row, equal_nan=True) and np.array_equal(lam2, lam, equal_nan=True), name
    ms = sym.sets_finish_wide_timing()
    assert len(ms) == 4 and all(v > 0.0 for v in ms)


_E2E = {}


def _end_to_end(name, c, block):
    key = (name, c, block)
    if key not in _E2E:
        p = GS._problem(name)
        tester = GS._tester(p, c, block, deterministic=True)
        sets = [s for s in wide_sets(block) if s.size != 32]
        mm = max(s.size for s in sets)
        _E2E[key] = (tester, sets, mm, tester(p["G"], sets, skato=True, max_markers=mm),
                     tester(p["G"], sets, skato=True, max_markers=mm, finish="wide"))
    return _E2E[key]


@pytest.mark.parametrize("block", [16, 128])
@pytest.mark.parametrize("c", [1, 4])
@pytest.mark.parametrize("name", ["spd203", "pedigree"])
def test_wide_finish_matches_host_finish_end_to_end(name, c, block):
    tester, sets, mm, host, wide = _end_to_end(name, c, block)
    assert [s.size for s in sets] == ([17, 33, 50] if block == 16 else [129, 257])
    GK._compare_dicts(wide, host, "%s c=%d block=%d" % (name, c, block))


def test_narrow_sets_between_wide_ones_forms_repeats_and_no_skato(tmp_path):
    from scilmm_amd.sets import KEYS, SKATO_KEYS
    p = GS._problem("spd203")
    n = p["n"]
    tester, wides, mm, _, wide = _end_to_end("spd203", 4, 16)
    n0 = tester.sym.timing()["n_float_atomic_launches"]
    narrow = [np.array([5, 40, 41, 42]), np.array([7, 8])]
    sets = [wides[0], narrow[0], wides[1], narrow[1], wides[2]]
    a = tester(p["G"], sets, skato=True, max_markers=mm, finish="wide")
    alone = tester(p["G"], narrow, skato=True, finish="device")
    for k in KEYS + SKATO_KEYS:
        assert np.array_equal(a[k][[1, 3]], alone[k], equal_nan=True), k                 # the bits of finish="device"
        assert np.array_equal(a[k][[0, 2, 4]], wide[k], equal_nan=True), k               # a wide set: the same bits wherever it stands
    b = tester(p["G"], sets, skato=True, max_markers=mm, finish="wide")
    bed = tester.test_bed(T.write_fileset(tmp_path / "wf", T.pack(p["G"]), n), sets, skato=True, max_markers=mm, finish="wide")
    dos = tester.test_dosages(_codes(p["G"]), sets, skato=True, max_markers=mm, finish="wide")
    for other in (b, bed, dos):
        for k in KEYS + SKATO_KEYS:
            assert other[k].dtype == a[k].dtype and np.array_equal(other[k], a[k], equal_nan=True), k
    small = tester(p["G"], sets, max_markers=mm, finish="wide")                          # burden and SKAT alone
    assert sorted(small) == sorted(KEYS)
    for k in KEYS:
        assert np.array_equal(small[k], a[k], equal_nan=True), k
    # alone, and behind another wide set of a different width: the work space is reused and nothing stale is read
    for i in (0, 2):
        one = tester(p["G"], [wides[i]], skato=True, max_markers=mm, finish="wide")
        two = tester(p["G"], [wides[2 - i], wides[i]], skato=True, max_markers=mm, finish="wide")
        for k in KEYS + SKATO_KEYS:
            assert np.array_equal(one[k][0], wide[k][i], equal_nan=True) and np.array_equal(two[k][1], wide[k][i], equal_nan=True), (i, k)
    # given weights reach the wide finish marker by marker
    w = [np.random.default_rng(3).uniform(0.5, 2.0, s.size) for s in sets]
    GK._compare_dicts(tester(p["G"], sets, weights=w, skato=True, max_markers=mm, finish="wide"),
                      tester(p["G"], sets, weights=w, skato=True, max_markers=mm), "given weights")
    assert tester.sym.timing()["n_float_atomic_launches"] == n0


def test_refusals_and_state_errors(monkeypatch):
    import torch
    from scilmm_amd import ScilmmError, _lib
    from scilmm_amd.dist import HipChainEngine
    from scilmm_amd.factor import Symbolic
    from tests.helpers import rel_err
    st = GK._c_level()
    tester = st["tester"]
    fac, sym = tester.factor, tester.sym
    p = GS._problem("spd203")
    wide = [np.arange(4, 37)]
    t16 = GS._tester(p, 4, 16, deterministic=True)
    with pytest.raises(ValueError, match="return_kernel"):
        t16(p["G"], wide, max_markers=64, finish="wide", return_kernel=True)
    with pytest.raises(ValueError, match="holds one block"):
        t16(p["G"], wide, max_markers=64, finish="device")
    with pytest.raises(ValueError, match="more than max_markers = 32"):
        t16(p["G"], wide, max_markers=32, finish="wide")
    with pytest.raises(ValueError, match="finish must be one of host, device, wide"):
        t16(p["G"], wide, max_markers=64, finish="lds")
    # argument errors on a live handle leave it as usable as before
    L, one = _lib.lib(), vp(8)
    rho = np.array([0.0, 0.5, 1.0])
    good = dict(fac=fac._h, k=40, block=16, q=3, stats=one, gram=one, cross=one, ld=32, R=one, u=one, c=2, mode=1, w=None, method=0,
                rho=_lib.ptr(rho), n_rho=3, out=one, lam=None)
    for kw in (dict(k=0), dict(k=4097), dict(block=129), dict(ld=31), dict(cross=None), dict(k=16), dict(q=4), dict(n_rho=17),
               dict(rho=_lib.ptr(np.array([0.0, 1.5, 1.0]))), dict(mode=2), dict(method=2), dict(out=None)):
        a = dict(good, **kw)
        assert L.scilmm_sets_finish_wide_dev(*[a[k] for k in good]) == _lib.ERR_ARG, kw
    member = st["made"]["psd17"]
    S, G, _ = _block_of(member, st)
    row, lam = _wide(fac, sym, torch, S, G, st["R"], st["u"], 16)
    host, lam_h = _host(S, G, st["R"], st["u"], None, "saddlepoint", RHO)
    _compare(row, host, lam, lam_h, "after the argument errors", {})
    # fp32-product fronts and a distributed handle: refused as the narrow finish refuses them, the handle left as it was
    from tests.test_gpu_halfsolve import _pedigree
    buf = torch.zeros((4096,), dtype=torch.float64, device="cuda")
    bp = vp(buf.data_ptr())
    q = _pedigree()
    eng = HipChainEngine([q["A"], q["I"]], 0, 2, None, "cuda:0")
    with pytest.raises(ScilmmError, match="distributed"):
        eng.fac.sets_finish_wide_dev(20, 16, 3, bp, bp, bp, 16, bp, bp, 2, 1, None, 0, rho, bp, None)
    assert eng.collectives == 0
    monkeypatch.setenv("SCILMM_TUNING", "1")
    monkeypatch.setenv("SCILMM_DENSE", "1")
    sym32 = Symbolic([q["A"], q["I"]])
    sym32.set_front_precision(32)
    f32 = sym32.factorize([0.35, 0.65])
    with pytest.raises(ScilmmError, match="fp32"):
        f32.sets_finish_wide_dev(20, 16, 3, bp, bp, bp, 16, bp, bp, 2, 1, None, 0, rho, bp, None)
    B = np.random.default_rng(0).standard_normal((q["A"].shape[0], 2))
    assert rel_err(q["V"] @ f32(B), B) < 1e-9
