"""scilmm_sets_finish_panel_dev and VariantSetTest.set_traits against scilmm_sets_finish_dev run trait by trait on the same block
(the set's score row replaced by the trait's column of X'Y~, u = 0), against the panel's own host finish, and against the
un-whitened oracle of tests/test_gpu_sets.py with the trait for its phenotype.

Tolerances, those of tests/test_gpu_skato.py: the burden numbers and skat_q 1e-9 relative; every p-value (skat_p, skato_p,
skato_pmin, burden_p) 1e-6 relative; skato_rho, n_used and the flag word exact; exactly the documented doubles written.  Bits:
a (set, trait) pair gives the same bits whatever T is, wherever the trait's column and the set lie, whatever the group size.

At the C level the blocks hold the made-up sets of tests/test_gpu_skato.py (sizes 1 .. 128, rank-deficient, identity, 1 an
eigenvector, 1'A1 = 0, the saddlepoint seam, T < 1e-30, dropped markers, many pieces of the integral) and the traits are the
set's own score, zeros, two draws from the null and the score plus a 6-sd signal; then 67 traits with a group size of 8 (nine
groups, the last one of three).

Worst deviations measured on an MI355X when this was written (printed by the tests with -s): at the C level, panel finish against
scalar finish, T = 5: 0 on every number (a wave's butterfly over a set of at most 128 markers adds in the order of the
workgroup's tree); with scales burden_beta 1.6e-15; T = 67 in groups of 8: skat_q 3.0e-16, p-values 5.9e-14.  End to end: column 0
against the scalar device finish 4.4e-14, against the panel's host finish 5.7e-13; the other columns against the host finish and
the oracle 8.8e-12; scale="profile" against its host finish 4.3e-13."""
import ctypes as C

import numpy as np
import pytest

from tests import test_bed_api as T
from tests import test_gpu_sets as GS
from tests import test_gpu_skato as GK
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

PTOL, TOL = GK.PTOL, GK.TOL
SENT = GK.SENT
RHO = GK.RHO
HEAD, ROW = 4, 8
GROUP = "SCILMM_SETS_PANEL_GROUP"
vp = C.c_void_p


def _traits(members, rng, T_):
    """B = X'Y~ (r x T_) for a block of made-up sets: per set its own score | zeros | two draws from the null | the score plus a
    6-sd signal | further draws from the null, each with its own scale.  The rows of dropped markers hold anything."""
    parts = []
    for name, K, s, exact, dropped in members:
        k, m = K.shape[0], K.shape[0] + len(dropped)
        ev, U = np.linalg.eigh(K)
        half = U * np.sqrt(np.maximum(ev, 0.0))
        Bk = half @ rng.standard_normal((k, T_)) * rng.uniform(0.5, 2.0, T_)
        Bk[:, 0], Bk[:, 1] = s, 0.0
        Bk[:, 4] = s + 6.0 * np.sqrt(np.diag(K)) * rng.choice([-1.0, 1.0], k)
        full = 0.5 * np.ones((m, T_))
        full[[j for j in range(m) if j not in dropped]] = Bk
        parts.append(full)
    return np.vstack(parts)


_STATE = {}


def _c_level():
    """The handle of tests/test_gpu_skato.py and its made-up sets, packed into blocks with u = 0, and 67 traits per block."""
    if not _STATE:
        from scilmm_amd.sets import pack_sets
        st = GK._c_level()
        rng = np.random.default_rng(24)
        made = list(st["made"].values())
        blocks = []
        for members in pack_sets([m[1].shape[0] + len(m[4]) for m in made], 128):
            mem = [made[i] for i in members]
            S, G, start = GK._made_up_block(mem, rng, st["R"], np.zeros(GK.CC))
            blocks.append(dict(names=[m[0] for m in mem], members=mem, S=S, G=G, start=start, B=_traits(mem, rng, 67)))
        _STATE.update(tester=st["tester"], R=st["R"], made=st["made"], blocks=blocks)
    return _STATE


def _panel_finish(fac, sym, torch, S, G, R, start, B, tscale=None, mode=1, weights=None, method=0, rho=RHO):
    """One call of scilmm_sets_finish_panel_dev on sentinel-filled buffers, the scores at a leading dimension of T + 3:
    (head, rows); exactly the documented doubles are written."""
    q, r = S.shape[0] - 4, S.shape[1]
    ns, T_ = start.size - 1, B.shape[1]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    Bp = np.full((r, T_ + 3), np.nan)
    Bp[:, :T_] = B
    dS, dG, dR, dB = dev(S), dev(G), dev(R), dev(Bp)
    dW = dev(weights) if weights is not None else None
    dT = dev(tscale) if tscale is not None else None
    dH = torch.full((ns * HEAD + 5,), SENT, dtype=torch.float64, device="cuda")
    dO = torch.full((ns * T_ * ROW + 5,), SENT, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    fac.sets_finish_panel_dev(r, q, vp(dS.data_ptr()), vp(dG.data_ptr()), vp(dR.data_ptr()), q - 1, ns, start, mode,
                              vp(dW.data_ptr()) if dW is not None else None, method, rho, vp(dB.data_ptr()), T_ + 3, T_,
                              vp(dT.data_ptr()) if dT is not None else None, vp(dH.data_ptr()), vp(dO.data_ptr()))
    sym.sync()
    H, O_ = dH.cpu().numpy(), dO.cpu().numpy()
    assert np.all(H[ns * HEAD:] == SENT) and np.all(O_[ns * T_ * ROW:] == SENT)
    assert not np.any(H[:ns * HEAD] == SENT) and not np.any(O_[:ns * T_ * ROW] == SENT)
    return H[:ns * HEAD].reshape(ns, HEAD), O_[:ns * T_ * ROW].reshape(ns, T_, ROW)


def _scalar_rows(fac, sym, torch, S, G, R, start, b, **kw):
    """scilmm_sets_finish_dev on the block with the score row b and u = 0: n_sets rows of 10 + n_rho doubles."""
    S2 = S.copy()
    S2[S.shape[0] - 1] = b
    return GK._finish(fac, sym, torch, S2, G, R, np.zeros(R.shape[0]), start, lam=False, **kw)[0]


def _dev(got, want):
    """Relative deviation where the reference is finite and not 0; elsewhere the same NaN, the same infinity up to its sign (w'Kw
    = 0 exactly: the sign of a 1't of rounding size is not the test's), the same 0."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want) & (want != 0)
    assert np.array_equal(np.abs(got[~fin]), np.abs(want[~fin]), equal_nan=True), (got[~fin], want[~fin])
    return float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin]))) if fin.any() else 0.0


def _compare_block(head, rows, ref, what, worst, skato=True):
    """head, rows: the panel's; ref[t]: the scalar finish's rows of trait t."""
    for t, r_ in enumerate(ref):
        assert np.array_equal(head[:, 0], r_[:, 0]), (what, t)                      # n_used
        live = r_[:, 0] > 0
        assert np.all(np.isnan(rows[~live, t, :7])) and np.all(rows[~live, t, 7] == 0), (what, t)
        assert np.all(np.isnan(head[~live, 1])) and np.all(head[~live, 2:] == 0), what
        h, d, x = head[live], rows[live, t], r_[live]
        with np.errstate(divide="ignore", invalid="ignore"):
            mine = {"burden_beta": d[:, 0] / h[:, 1], "burden_se": 1.0 / np.sqrt(h[:, 1]), "burden_chi2": d[:, 1], "skat_q": d[:, 2]}
        for col, name in ((1, "burden_beta"), (2, "burden_se"), (3, "burden_chi2"), (4, "skat_q")):
            e = _dev(mine[name], x[:, col])
            worst[name] = max(worst.get(name, 0.0), e)
            assert e < TOL, (what, t, name, e)
        pc = [(3, 5)] + ([(4, 6), (5, 7)] if skato else [])
        for mc, sc in pc:
            assert not np.any(np.isnan(d[:, mc])), (what, t, mc)
            e = _dev(d[:, mc], x[:, sc])
            worst["p"] = max(worst.get("p", 0.0), e)
            assert e < PTOL, (what, t, mc, e)
        if skato:
            assert np.array_equal(d[:, 6], x[:, 8]), (what, t, d[:, 6], x[:, 8])      # skato_rho
            assert np.all(d[:, 4] <= len(RHO) * d[:, 5])
        else:
            assert np.all(np.isnan(d[:, 4:7]))
        assert np.array_equal(d[:, 7], x[:, 9]), (what, t, d[:, 7], x[:, 9])          # the flag word
        assert not np.any(d[:, 7].astype(int) & 6) and np.all((h[:, 2].astype(int) & ~d[:, 7].astype(int)) == 0), (what, t)
        assert np.all(h[:, 3] == 0)


def test_panel_finish_at_the_c_level_matches_the_scalar_finish():
    import torch
    st = _c_level()
    fac, sym = st["tester"].factor, st["tester"].sym
    worst = {}
    for b in st["blocks"]:
        S, G, start, B = b["S"], b["G"], b["start"], b["B"][:, :5]
        head, rows = _panel_finish(fac, sym, torch, S, G, st["R"], start, B)
        ref = [_scalar_rows(fac, sym, torch, S, G, st["R"], start, B[:, t]) for t in range(5)]
        _compare_block(head, rows, ref, "+".join(b["names"]), worst)
        flags = dict(zip(b["names"], rows[:, 0, 7].astype(int)))
        for name, f in flags.items():
            assert f & 8 and bool(f & 1) == (name in ("psd1", "rank_one9", "s11_zero8")), (name, f)
        assert np.all(rows[:, 1, 2] == 0.0) and np.all(rows[head[:, 0] > 0, 1, 3] == 1.0)      # the trait without a score: Q = 0, p = 1
    print("worst deviations, panel finish against scalar finish, T = 5:", worst)
    # the other tail, the other weight modes, no SKAT-O, another grid, scales: on the first block
    b = st["blocks"][0]
    S, G, start, B = b["S"], b["G"], b["start"], b["B"][:, :5]
    w = np.random.default_rng(3).uniform(0.5, 2.0, S.shape[1])
    for what, kw in (("liu", dict(method=1)), ("given weights", dict(mode=2, weights=w)), ("beta weights", dict(mode=0)),
                     ("three grid values", dict(rho=np.array([0.0, 0.3, 1.0])))):
        head, rows = _panel_finish(fac, sym, torch, S, G, st["R"], start, B, **kw)
        ref = [_scalar_rows(fac, sym, torch, S, G, st["R"], start, B[:, t], **kw) for t in range(5)]
        _compare_block(head, rows, ref, what, worst)
    head, rows = _panel_finish(fac, sym, torch, S, G, st["R"], start, B, rho=np.empty(0))
    ref = [_scalar_rows(fac, sym, torch, S, G, st["R"], start, B[:, t], rho=np.empty(0)) for t in range(5)]
    _compare_block(head, rows, ref, "no SKAT-O", worst, skato=False)
    # scales: the scalar finish of the score divided by sqrt(scale); 1'(w o s) stays unscaled
    sc = np.array([0.37, 1.0, 2.5, 1.0, 11.0])
    head1, rows1 = _panel_finish(fac, sym, torch, S, G, st["R"], start, B)
    head, rows = _panel_finish(fac, sym, torch, S, G, st["R"], start, B, tscale=sc)
    assert np.array_equal(head, head1, equal_nan=True) and np.array_equal(rows[:, :, 0], rows1[:, :, 0], equal_nan=True)
    assert np.array_equal(rows[:, [1, 3]], rows1[:, [1, 3]], equal_nan=True)                   # a scale of 1.0 changes no bit
    ref = [_scalar_rows(fac, sym, torch, S, G, st["R"], start, B[:, t] / np.sqrt(sc[t])) for t in range(5)]
    scaled = rows.copy()
    scaled[:, :, 0] /= np.sqrt(sc)
    _compare_block(head, scaled, ref, "scales", worst)
    print("worst deviations with the variants:", worst)


def test_sixty_seven_traits_in_groups_of_eight(monkeypatch):
    import torch
    st = _c_level()
    fac, sym = st["tester"].factor, st["tester"].sym
    monkeypatch.setenv(GROUP, "8")
    worst = {}
    for b in st["blocks"]:
        S, G, start, B = b["S"], b["G"], b["start"], b["B"]
        head, rows = _panel_finish(fac, sym, torch, S, G, st["R"], start, B)
        ref = [_scalar_rows(fac, sym, torch, S, G, st["R"], start, B[:, t]) for t in range(B.shape[1])]
        _compare_block(head, rows, ref, "+".join(b["names"]), worst)
    print("worst deviations, panel finish against scalar finish, T = 67 in groups of 8:", worst)


def test_a_pair_gives_the_same_bits_wherever_it_lies(monkeypatch):
    import torch
    st = _c_level()
    tester = st["tester"]
    fac, sym, made = tester.factor, tester.sym, st["made"]
    n0 = sym.timing()["n_float_atomic_launches"]
    # a trait alone and as column 41 of 67; group sizes 1, 8, 32 and the engine's own choice
    b = st["blocks"][0]
    S, G, start, B = b["S"], b["G"], b["start"], b["B"]
    head67, rows67 = _panel_finish(fac, sym, torch, S, G, st["R"], start, B)
    again = _panel_finish(fac, sym, torch, S, G, st["R"], start, B)
    assert np.array_equal(head67, again[0], equal_nan=True) and np.array_equal(rows67, again[1], equal_nan=True)     # two runs
    head1, rows1 = _panel_finish(fac, sym, torch, S, G, st["R"], start, B[:, 41:42])
    assert np.array_equal(head1, head67, equal_nan=True) and np.array_equal(rows1[:, 0], rows67[:, 41], equal_nan=True)
    for g in ("1", "8", "32"):
        monkeypatch.setenv(GROUP, g)
        head, rows = _panel_finish(fac, sym, torch, S, G, st["R"], start, B)
        assert np.array_equal(head, head67, equal_nan=True) and np.array_equal(rows, rows67, equal_nan=True), g
    monkeypatch.delenv(GROUP)
    # a set alone in a block and behind others (256 threads of k_sets_spectra alone, 512 next to a wide set)
    for which in ("tiny17", "kinks2"):
        x = made[which]
        k = x[1].shape[0]
        rng = np.random.default_rng(11)
        filler = lambda k: ("f%d" % k, GK._psd(rng, k), rng.standard_normal(k), False, ())
        layouts = {"alone": ([x], 0), "last in a full block": ([filler(128 - k), x], 1), "between two": ([filler(5), x, filler(70)], 1)}
        Bx = _traits([x], np.random.default_rng(2), 5)
        got = {}
        for name, (members, at) in layouts.items():
            S, G, start = GK._made_up_block(members, np.random.default_rng(1), st["R"], np.zeros(GK.CC))
            a, b_ = start[at], start[at + 1]
            if "ref" not in got:
                got["ref"] = (S[:, a:b_].copy(), G[a:b_, a:b_].copy())
            S[:, a:b_], G[a:b_, a:b_] = got["ref"]
            B = np.random.default_rng(4).standard_normal((S.shape[1], 5))
            B[a:b_] = Bx
            head, rows = _panel_finish(fac, sym, torch, S, G, st["R"], start, B)
            got[name] = (head[at], rows[at])
            assert not int(rows[at][0, 7]) & 1, (which, name)                            # the integral was taken
        for name in ("last in a full block", "between two"):
            assert np.array_equal(got[name][0], got["alone"][0]) and np.array_equal(got[name][1], got["alone"][1]), (which, name)
    assert sym.timing()["n_float_atomic_launches"] == n0


_E2E = {}


def _end_to_end():
    """The pedigree problem of tests/test_gpu_sets.py with four phenotypes: its own and three others with effects on other sets."""
    if not _E2E:
        p = GS._problem("pedigree")
        tester, sets, _, scalar = GK._host_and_device("pedigree", 4, 128)
        GS._oracle(p, 4, sets)                                     # (leaves the projection P with the problem: the copies below share it)
        rng = np.random.default_rng(41)
        _, _, Gt = GS._centred(p["G"])
        Y = np.empty((p["n"], 4))
        Y[:, 0] = p["y"]
        for t in range(1, 4):
            y = p["C"] @ rng.standard_normal(4) + (0.5 + t) * rng.standard_normal(p["n"])
            if t < 3:                                              # (the last one is a pure null phenotype)
                k = (1, 4)[t - 1]
                sd = np.sqrt(np.maximum((Gt[sets[k]] ** 2).sum(axis=1), 1.0) / p["n"])
                y = y + (0.05 * rng.choice([-1.0, 1.0], sets[k].size) / sd) @ Gt[sets[k]]
            Y[:, t] = y
        panel = tester.set_traits(Y)
        _E2E.update(p=p, tester=tester, sets=sets, scalar=scalar, Y=Y, panel=panel, dev=panel(p["G"], sets, skato=True))
    return _E2E


def _compare_columns(got, want, live, what, skato):
    from scilmm_amd.set_panel import SKATO_KEYS
    for k in ("burden_beta", "burden_se", "burden_chi2", "skat_q"):
        assert rel_err(got[k][live], want[k][live]) < TOL, (what, k, rel_err(got[k][live], want[k][live]))
    worst = 0.0
    for k in ("burden_p", "skat_p") + (SKATO_KEYS[:2] if skato else ()):
        e = float(np.max(np.abs(got[k][live] - want[k][live]) / np.abs(want[k][live])))
        worst = max(worst, e)
        assert e < PTOL, (what, k, e)
    if skato:
        assert np.array_equal(got["skato_rho"][live], want["skato_rho"][live]), what
    print(what, "worst rel. deviation of a p-value", worst)


def test_end_to_end_against_the_scalar_tester_the_host_finish_and_the_oracle():
    from scilmm_amd.set_panel import KEYS, SKATO_KEYS
    e = _end_to_end()
    p, sets, dev, scalar, tester = e["p"], e["sets"], e["dev"], e["scalar"], e["tester"]
    ns = len(sets)
    assert sorted(dev) == sorted(KEYS + SKATO_KEYS) and dev["n_used"].shape == (ns,) and dev["n_used"].dtype == np.int64
    assert all(dev[k].shape == (ns, 4) for k in KEYS[1:] + SKATO_KEYS)
    assert np.array_equal(dev["n_used"], scalar["n_used"])
    live = dev["n_used"] > 0
    assert not live[-1] and all(np.all(np.isnan(dev[k][~live])) and not np.any(np.isnan(dev[k][live])) for k in KEYS[1:] + SKATO_KEYS)
    # column 0: the tester's own phenotype, against tester(..., skato=True, finish="device") and the panel's host finish
    col0 = {k: dev[k][:, 0] for k in KEYS[1:] + SKATO_KEYS}
    _compare_columns(col0, scalar, live, "column 0 against the scalar device finish", True)
    one = tester.set_traits(e["Y"][:, :1])
    host0 = one(p["G"], sets, skato=True, finish="host")
    assert np.array_equal(host0["n_used"], dev["n_used"]) and sorted(host0) == sorted(dev)
    _compare_columns(col0, {k: host0[k][:, 0] for k in col0}, live, "column 0 against the panel's host finish", True)
    dev0 = one(p["G"], sets, skato=True)
    for k in col0:
        assert np.array_equal(dev0[k][:, 0], col0[k], equal_nan=True), k               # T = 1 and column 0 of T = 4: the same bits
    # every column against the host finish (burden and SKAT) and against the un-whitened oracle with that phenotype
    host = e["panel"](p["G"], sets, finish="host")
    plain = e["panel"](p["G"], sets)
    assert sorted(plain) == sorted(KEYS)
    for t in range(4):
        for k in KEYS[1:]:
            assert np.array_equal(plain[k][:, t], dev[k][:, t], equal_nan=True), (k, t)   # skato=True leaves their bits alone
        got = {k: dev[k][:, t] for k in KEYS[1:]}
        _compare_columns(got, {k: host[k][:, t] for k in got}, live, "column %d against the host finish" % t, False)
        ref = GS._oracle(dict(p, y=e["Y"][:, t], ref={}), 4, sets)
        assert np.array_equal(dev["n_used"], ref["n_used"])
        _compare_columns(got, ref, live, "column %d against the oracle" % t, False)


def test_profile_is_the_fixed_result_rescaled():
    import scipy.stats as stats
    from scilmm_amd import sets as mod
    e = _end_to_end()
    p, sets, dev, tester = e["p"], e["sets"], e["dev"], e["tester"]
    prof = tester.set_traits(e["Y"], scale="profile")
    out = prof(p["G"], sets, skato=True)
    s_t = out["scale"]
    assert s_t.shape == (4,) and np.array_equal(s_t, tester.traits(e["Y"], scale="profile").s_t) and np.all(s_t > 0)
    live = dev["n_used"] > 0
    assert np.array_equal(out["burden_beta"], dev["burden_beta"], equal_nan=True)
    assert rel_err(out["burden_se"][live], (dev["burden_se"] * np.sqrt(s_t))[live]) < TOL
    assert rel_err(out["burden_chi2"][live], (dev["burden_chi2"] / s_t)[live]) < TOL
    assert rel_err(out["skat_q"][live], (dev["skat_q"] / s_t)[live]) < TOL
    assert np.array_equal(out["burden_p"][live], stats.f(1, p["n"] - 1).sf(out["burden_chi2"][live]))
    host = prof(p["G"], sets, finish="host")
    assert np.array_equal(host["scale"], s_t)
    for t in range(4):
        got = {k: out[k][:, t] for k in mod.KEYS[1:]}
        _compare_columns(got, {k: host[k][:, t] for k in got}, live, "profile, column %d against the host finish" % t, False)
    assert np.all(out["skato_p"][live] <= 8 * out["skato_pmin"][live]) and not np.any(np.isnan(out["skato_p"][live]))


def test_bed_and_dosages_give_the_bits_of_the_int8_call_and_runs_repeat(tmp_path):
    from scilmm_amd.set_panel import KEYS, SKATO_KEYS
    p = GS._problem("spd203")
    tester = GS._tester(p, 4, 128, deterministic=True)
    sets = p["sets"]
    rng = np.random.default_rng(9)
    Y = np.column_stack([p["y"], p["C"] @ rng.standard_normal(4) + rng.standard_normal(p["n"]), rng.standard_normal(p["n"])])
    panel = tester.set_traits(Y)
    dev = panel(p["G"], sets, skato=True)
    again = tester.set_traits(Y)(p["G"], sets, skato=True)
    path = T.write_fileset(tmp_path / "id", T.pack(p["G"]), p["n"])
    bed = panel.test_bed(path, sets, skato=True)
    codes = np.where(p["G"] >= 0, p["G"].astype(np.int64) * 16384, 65535).astype(np.uint16)
    dos = panel.test_dosages(codes, sets, skato=True)
    for other in (again, bed, dos):
        for k in KEYS + SKATO_KEYS:
            assert np.array_equal(other[k], dev[k], equal_nan=True), k
    assert tester.sym.timing()["n_float_atomic_launches"] == 0


def test_refusals(monkeypatch):
    import torch
    from scilmm_amd import ScilmmError, _lib
    from scilmm_amd.factor import Symbolic
    e = _end_to_end()
    p, tester, panel, sets = e["p"], e["tester"], e["panel"], e["sets"]
    small = GS._tester(p, 4, 16, deterministic=True).set_traits(e["Y"][:, :2])
    with pytest.raises(ValueError, match="more than one device block of 16"):
        small(p["G"], p["sets"])
    for kw in (dict(return_kernel=True), dict(max_markers=256)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            panel(p["G"], sets, **kw)
    with pytest.raises(TypeError, match="reduce"):
        panel(p["G"], sets, reduce="max")
    with pytest.raises(ValueError, match="finish"):
        panel(p["G"], sets, finish="wide")
    n = p["n"]
    for Y in (np.zeros((n, 0)), np.zeros((n, 4097))):
        with pytest.raises(ValueError, match="1..4096"):
            tester.set_traits(Y)
    bad = e["Y"].copy()
    bad[7, 2] = np.nan
    with pytest.raises(ValueError, match="finite"):
        tester.set_traits(bad)
    with pytest.raises(ValueError, match="scale"):
        tester.set_traits(e["Y"], scale="profiled")
    assert type(tester.traits(e["Y"])).__name__ == "TraitPanel"                      # AssociationScan.traits stays what it is
    # the C level: the handle's own refusals.  A factor consumed by the selected inverse:
    q = GS._problem("spd203")
    sym = Symbolic([q["A"], q["I"]])
    f = sym.factorize(GS.S2)
    f.selected_inverse()
    buf = torch.zeros((4096,), dtype=torch.float64, device="cuda")
    bp = vp(buf.data_ptr())
    start, rho = np.array([0, 2, 5], dtype=np.int32), np.array([0.0, 0.5, 1.0])
    with pytest.raises(ScilmmError, match="not valid"):
        f.sets_finish_panel_dev(5, 3, bp, bp, bp, 2, 2, start, 1, None, 0, rho, bp, 4, 4, None, bp, bp)
    # t = 0, t = 4097 and a scale the host can read that is not positive (pinned memory): argument errors, the handle stays usable
    fac = tester.factor
    L = _lib.lib()
    args = lambda t, ld, ts: (fac._h, 5, 3, bp, bp, bp, 2, 2, _lib.ptr(start), 1, None, 0, _lib.ptr(rho), 3, bp, ld, t, ts, bp, bp)
    assert L.scilmm_sets_finish_panel_dev(*args(0, 4, None)) == _lib.ERR_ARG
    assert L.scilmm_sets_finish_panel_dev(*args(4097, 4097, None)) == _lib.ERR_ARG
    pinned = torch.tensor([1.0, 0.0, 2.0, 1.0], dtype=torch.float64).pin_memory()
    assert L.scilmm_sets_finish_panel_dev(*args(4, 4, vp(pinned.data_ptr()))) == _lib.ERR_ARG
    pinned[1] = float("nan")
    assert L.scilmm_sets_finish_panel_dev(*args(4, 4, vp(pinned.data_ptr()))) == _lib.ERR_ARG
    again = panel(p["G"], sets, skato=True)
    for k in e["dev"]:
        assert np.array_equal(again[k], e["dev"][k], equal_nan=True), k
