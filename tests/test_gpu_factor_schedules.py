"""The factorization's dense-tail kernels at ragged fronts, and every schedule switch of csrc/dev.h that no other module sets:
each case factorizes one problem of tests/factor_shapes.py on a handle created under the case's environment and passes
`_check_factor` of tests/test_gpu_parity.py (L entry by entry, log-det, solves and L*R against the oracle at 1e-10), and
each case shows from the plan's own report (SCILMM_VERBOSE) and from `timing()` that it ran what it names.

  DENSE_CASES    k_dense_b on R37 / R50 / R100 / R128: odd widths, single ragged chunks, 64 + 36, full chunks; K segments over
                 several descendants (SCILMM_DENSE_ITEMS=64, SCILMM_DENSE_FILL=0) and the taper's split of them
  FP32_CASES     k_dense_h (fp32 shadow) and k_dense32 (SCILMM_SHADOW=0) on R37 and P10
  PANEL_CASES    k_trsm<true>, and the slab counts k_reduce / k_potrf / k_trsm fold (split-K off, many slabs, fewest slabs)
  OUTSIDE_CASES  k_outside in 1 / 3 / one-per-panel launches, without the groups of identical tail rows, on the chain's priority
  STREAM_CASES   1 and 3 side streams; on deterministic handles 1, 2 and 3 streams give the same bits

tests/test_factor_shapes.py holds the facts of the host analysis without a GPU and checks that every switch `read_tuning()`
reads occurs in one of these tables (or in test_gpu_parity's) or is exempted with a reason.  The oracle's factor is built once per
problem (on host threads, side by side, before the first case) and its solves are kept: every case of a problem asks for the same ones."""
import concurrent.futures
import hashlib
import re

import numpy as np
import pytest

from tests import factor_shapes as FS
from tests.test_gpu_parity import TOL, _check_factor
from tests.test_gpu_selected_inverse import _stderr_text

pytestmark = pytest.mark.gpu

DENSE = {"SCILMM_DENSE": "1"}
ITEMS64 = dict(DENSE, SCILMM_DENSE_ITEMS="64")
TAPER = dict(ITEMS64, SCILMM_DENSE_TAPER="1")
NOFILL = dict(DENSE, SCILMM_DENSE_FILL="0")
DENSE_CASES = ([(pid, env) for pid in ("R37", "R50", "R100", "R128") for env in (DENSE, ITEMS64, TAPER, NOFILL)] +
               [(pid, dict(DENSE, **extra)) for pid in ("R37", "R128")
                for extra in ({"SCILMM_NO_LOOKAHEAD": "1"}, {"SCILMM_LOOK_DEPTH": "4"})] +
               [("R37", dict(DENSE, SCILMM_NO_MFMA="1"))])
FP32_CASES = [(pid, env) for pid in ("R37", "P10") for env in (DENSE, dict(DENSE, SCILMM_SHADOW="0"))]
MANY_SLABS = {"SCILMM_MIN_ITEM": "1", "SCILMM_MAX_ITEM": "1", "SCILMM_TARGET_ITEMS": "100000"}
FEW_SLABS = {"SCILMM_TARGET_ITEMS": "1"}
PANEL_CASES = [(pid, env) for pid in ("P10", "R128")
               for env in ({"SCILMM_TRSM_LITE": "0"}, {"SCILMM_NO_SPLITK": "1"}, MANY_SLABS, FEW_SLABS)]
OUTSIDE = {"SCILMM_OUTSIDE": "1"}
OUTSIDE_CASES = [(pid, dict(OUTSIDE, **extra)) for pid in ("P10", "P20")
                 for extra in ({"SCILMM_OUTSIDE_CHUNKS": "1"}, {"SCILMM_OUTSIDE_CHUNKS": "3"}, {"SCILMM_OUTSIDE_CHUNKS": "32"},
                               {"SCILMM_OUTSIDE_MERGE": "0"}, {"SCILMM_OUTSIDE_PRIO": "1"},
                               {"SCILMM_DENSE": "1", "SCILMM_OUTSIDE_CHUNKS": "32"})]
STREAM_CASES = [("P10", dict(base, SCILMM_SIDE_STREAMS=k)) for k in ("1", "3") for base in ({}, dict(DENSE, **OUTSIDE))]
TABLES = {"DENSE_CASES": DENSE_CASES, "FP32_CASES": FP32_CASES, "PANEL_CASES": PANEL_CASES, "OUTSIDE_CASES": OUTSIDE_CASES,
          "STREAM_CASES": STREAM_CASES}


def switches_in_tables():
    """Every switch a case of this module sets (tests/test_factor_shapes.py: the coverage check)."""
    return {k for cases in TABLES.values() for _, env in cases for k in env}


# the switches of other modules' cases that a leftover value of would change what a case here runs
_CLEARED = switches_in_tables() | {"SCILMM_TUNING", "SCILMM_DETERMINISTIC", "SCILMM_VERBOSE", "SCILMM_NO_CHAIN", "SCILMM_CELL_LIMIT",
                                   "SCILMM_HOST_CELLS", "SCILMM_RESERVE_CUS"}

REPORTS = {
    "dense": re.compile(r"dense tail: fronts (\d+)\.\.(\d+) \((\d+) wide\), (\d+) early \+ (\d+) late implicit items"),
    "groups": re.compile(r"k_outside: (\d+) descendants in (\d+) groups of identical tail rows; (\d+) of (\d+) block pairs"),
    "chunks": re.compile(r"k_outside: (\d+) block-pair items of prelude fronts below level (\d+) \(tail starts at column (\d+)\), (\d+) chunks"),
    "prio": re.compile(r"k_outside: on a stream of (the chain's|the look-ahead streams') priority"),
    "early": re.compile(r"early launches: (\d+) explicit items, (\d+) partial slabs on (\d+) tiles, (\d+) \.\. (\d+) per tile, "
                        r"(\d+) tiles with an odd count, (\d+) with an even one"),
    "late": re.compile(r"late launches: (\d+) explicit items, (\d+) partial slabs on (\d+) tiles, (\d+) \.\. (\d+) per tile, "
                       r"(\d+) tiles with an odd count, (\d+) with an even one"),
    "kernels": re.compile(r"split-K (on|off), panel solve (\S+), (\d+) side streams"),
}
FP32_KERNEL = re.compile(r"fp32 fronts: (k_dense_h|k_dense32)\b")
_SLAB_FIELDS = ("items", "slabs", "tiles", "lo", "hi", "odd", "even")

_HANDLES = {}   # (problem, environment, deterministic) -> handle and the plan's report
_ORACLES = {}   # problem -> future of its _MemoOracle


def _ints(m, names):
    return dict(zip(names, map(int, m.groups())))


def _parse(text):
    rep = {}
    for key, rx in REPORTS.items():
        m = rx.search(text)
        if not m:
            continue
        if key in ("early", "late"):
            rep[key] = _ints(m, _SLAB_FIELDS)
        elif key == "dense":
            rep[key] = _ints(m, ("first", "last", "width", "early", "late"))
        elif key == "groups":
            rep[key] = _ints(m, ("descendants", "groups", "pairs_kept", "pairs"))
        elif key == "chunks":
            rep[key] = _ints(m, ("items", "level", "column", "chunks"))
        elif key == "prio":
            rep[key] = m.group(1)
        else:
            rep[key] = dict(splitk=m.group(1), trsm=m.group(2), nside=int(m.group(3)))
    return rep


class _MemoOracle(object):
    """The oracle's factor of one problem; its solves, products and export are computed once per argument."""

    def __init__(self, V, perm):
        from oracle import oracle as O
        self._o = O.OracleFactor(V, perm)
        self._memo = {}

    def _once(self, what, fn, B):
        B = np.ascontiguousarray(B, dtype=np.float64)
        key = (what, B.shape, hashlib.blake2b(B.tobytes(), digest_size=16).digest())
        if key not in self._memo:
            self._memo[key] = fn(B)
        return self._memo[key]

    def __call__(self, B):
        return self._once("solve", self._o, B)

    def lmul(self, R):
        return self._once("lmul", self._o.lmul, R)

    def L(self):
        if "L" not in self._memo:
            self._memo["L"] = self._o.L()
        return self._memo["L"]

    def P(self):
        return self._o.P()

    def logdet(self):
        return self._o.logdet()


@pytest.fixture(scope="module", autouse=True)
def _problems():
    """The oracle factorizations of the six problems, side by side on host threads (the C oracle is serial and releases the
    GIL); releases everything with the module."""
    from oracle import oracle as O
    from scilmm_amd.factor import Symbolic
    O.lib()
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=len(FS.PROBLEMS))
    for pid in ("R128", "R37", "P10", "P20", "R50", "R100"):   # longest first
        p = FS.problem(pid)
        perm = Symbolic(p["mats"], upload=False, **p["opts"]).P()
        V = sum(s * m for s, m in zip(p["sigma2"], p["mats"])).tocsr()
        _ORACLES[pid] = pool.submit(_MemoOracle, V, perm)
    for fut in _ORACLES.values():
        fut.result()
    yield
    pool.shutdown(wait=True, cancel_futures=True)
    _ORACLES.clear()
    _HANDLES.clear()
    FS.release()


def _oracle(pid):
    return _ORACLES[pid].result()


def _set_env(monkeypatch, env, verbose=False):
    for k in _CLEARED:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SCILMM_TUNING", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if verbose:
        monkeypatch.setenv("SCILMM_VERBOSE", "1")


def _handle(monkeypatch, pid, env, deterministic=None):
    """One Symbolic per (problem, environment), created under that environment -- most switches are read when the device plan
    is built, with the upload of the values -- with the plan's report.  Leaves the case's environment set."""
    from scilmm_amd.factor import Symbolic
    key = (pid, tuple(sorted(env.items())), deterministic)
    if key not in _HANDLES:
        p = FS.problem(pid)
        text = []
        _set_env(monkeypatch, env, verbose=True)
        with _stderr_text(text):
            sym = Symbolic(p["mats"], deterministic=deterministic, **p["opts"])
        rep = _parse(text[0])
        assert "kernels" in rep and "dense" in rep and "early" in rep and "late" in rep, text[0]
        _HANDLES[key] = dict(sym=sym, report=rep, text=text[0])
    _set_env(monkeypatch, env)
    return _HANDLES[key]


def _ids(cases):
    return ["%s-%s" % (pid, ",".join("%s=%s" % (k.replace("SCILMM_", ""), v) for k, v in sorted(env.items())) or "default")
            for pid, env in cases]


def _dense_launches(sym, f, sigma2):
    """Launches of the dense-tail kernel in one factorization (`timing()` counts them in a profiled one)."""
    sym.set_profiling(1)
    try:
        f.refactorize(sigma2)
        return sym.timing()["n_dense_launches"]
    finally:
        sym.set_profiling(0)


def _check(pid, h):
    """`_check_factor` on the case's handle; returns the factor and the dense-tail launches of a factorization."""
    p = FS.problem(pid)
    f = _check_factor(p["mats"], p["sigma2"], h["sym"], rs=(5, 103), oracle=_oracle(pid))
    return f, _dense_launches(h["sym"], f, p["sigma2"])


# ---- dense-tail shapes

def _replayed_early_items(sym, env):
    if env.get("SCILMM_NO_LOOKAHEAD") == "1":
        return 0                                                          # every descendant is late
    return FS.replay_early_items(FS.tail_pairs(sym), int(env.get("SCILMM_DENSE_ITEMS", 128)), int(env.get("SCILMM_DENSE_FILL", 256)),
                                 env.get("SCILMM_DENSE_TAPER") == "1", int(env.get("SCILMM_LOOK_DEPTH", FS.LOOK_DEPTH)))[0]


@pytest.mark.parametrize("pid,env", DENSE_CASES, ids=_ids(DENSE_CASES))
def test_dense_tail_shapes(pid, env, monkeypatch):
    """k_dense_b on fronts that are not 128 wide.  The plan's early item count equals the replay of its K-segment rule
    (tests/factor_shapes.py; test_factor_shapes.py holds what the replay gives per setting); with 64 items per launch R37 and
    R128 have items over several descendants (`next_chunk` crosses a descendant boundary inside the software pipeline); the
    scalar case has no dense path (k_dense_b has no scalar form) and runs the same fronts through k_update2<false> and
    k_trsm<false>."""
    h = _handle(monkeypatch, pid, env)
    sym, rep = h["sym"], h["report"]
    f, nd = _check(pid, h)
    print(pid, env, rep["dense"], "dense launches", nd)
    if env.get("SCILMM_NO_MFMA") == "1":
        assert nd == 0 and rep["dense"]["early"] == 0 and rep["kernels"]["trsm"] == "k_trsm<false>"
        return
    assert nd > 0 and rep["kernels"]["trsm"] == "k_trsm_lite"
    assert rep["dense"]["early"] == _replayed_early_items(sym, env), (rep["dense"], env)
    if env.get("SCILMM_NO_LOOKAHEAD") == "1":
        assert rep["dense"]["early"] == 0 and rep["dense"]["late"] > 0
    if pid in ("R37", "R128") and env.get("SCILMM_DENSE_ITEMS") == "64":
        assert rep["dense"]["early"] < FS.single_descendant_early_items(sym)   # items over two or more descendants


@pytest.mark.parametrize("pid", ["R37", "R128"])
def test_taper_splits_the_last_segments(pid, monkeypatch):
    """SCILMM_DENSE_TAPER=1 cuts the last two K segments of an early launch in two and in four: strictly more early items than
    the same plan without it wherever a segment is two or more descendants long (on R50 and R100 none is: the taper cases
    there have the item counts of the plain ones, which `test_dense_tail_shapes` holds to the replay)."""
    plain = _handle(monkeypatch, pid, ITEMS64)["report"]["dense"]["early"]
    taper = _handle(monkeypatch, pid, TAPER)["report"]["dense"]["early"]
    print(pid, "early items: 64 per launch", plain, "with the taper", taper)
    assert taper > plain


# ---- fp32-product fronts

@pytest.mark.parametrize("pid,env", FP32_CASES, ids=_ids(FP32_CASES))
def test_fp32_fronts_shadow_and_staged(pid, env, monkeypatch):
    """Front precision 32 through the fp32 shadow (k_dense_h) and with SCILMM_SHADOW=0 (k_dense32; read per call), at the bounds
    of test_gpu_parity.test_fp32_fronts_with_fp64_sums_and_refinement: factor within 1e-5 of the fp64 oracle and not equal to
    it, log-det 1e-7, refined solves 1e-10, and the fp64 factor back after a return to 64 bits.
    Measured errL (MI355X): R37 k_dense_h 3.3e-10, k_dense32 1.0e-10 (log-det 4.9e-13, 1.6e-13); P10 k_dense_h 1.1e-8,
    k_dense32 3.4e-9 (log-det 3.6e-10, 2.1e-11).  R37's updates are small beside its diagonal n I, so its fp32 rounding shows
    less; both kernels stay three orders of magnitude inside the bound on both shapes."""
    from tests.helpers import rel_err
    h = _handle(monkeypatch, pid, env)
    sym = h["sym"]
    p, o = FS.problem(pid), _oracle(pid)
    s2 = p["sigma2"]
    V = sum(s * m for s, m in zip(s2, p["mats"])).tocsr()
    n = V.shape[0]
    Lo = o.L()
    scale = np.abs(Lo.data).max()
    f = sym.factorize(s2)
    assert np.array_equal(f.P(), o.P())
    ld64, L64 = f.logdet(), f.L()
    assert np.abs((L64 - Lo).tocsr().data).max() / scale < TOL           # the fp64 path is untouched
    assert abs(ld64 - o.logdet()) < TOL * abs(o.logdet())
    sym.set_front_precision(32)
    try:
        text = []
        monkeypatch.setenv("SCILMM_VERBOSE", "1")
        with _stderr_text(text):
            f.refactorize(s2)
        monkeypatch.delenv("SCILMM_VERBOSE")
        m = FP32_KERNEL.search(text[0])
        assert m and m.group(1) == ("k_dense32" if env.get("SCILMM_SHADOW") == "0" else "k_dense_h"), text[0]
        errL = np.abs((f.L() - Lo).tocsr().data).max() / scale
        errld = abs(f.logdet() - o.logdet()) / abs(o.logdet())
        print("%s %s: errL %.3e (limit 1e-5), log-det %.3e (limit 1e-7)" % (pid, m.group(1), errL, errld))
        assert 0.0 < errL < 1e-5, errL
        assert errld < 1e-7, errld
        B = np.random.default_rng(3).standard_normal((n, 5))
        X = f(B)
        assert rel_err(X, o(B)) < TOL                                     # refined solve
        assert rel_err(V @ X, B) < 1e-11
        assert _dense_launches(sym, f, s2) > 0
    finally:
        sym.set_front_precision(64)
    f.refactorize(s2)
    assert abs(f.logdet() - ld64) < 1e-12 * abs(ld64)
    assert np.abs(f.L().data - L64.data).max() < 1e-12 * scale


# ---- panel solve and slab folds

@pytest.mark.parametrize("pid,env", PANEL_CASES, ids=_ids(PANEL_CASES))
def test_panel_solve_and_slab_folds(pid, env, monkeypatch):
    """k_trsm<true> in place of k_trsm_lite, and the partial-slab counts that k_reduce (early launches) and k_potrf / k_trsm
    (late launches) fold: none (split-K off), up to 64 per tile (items of one cost unit), the fewest the cut allows."""
    h = _handle(monkeypatch, pid, env)
    rep = h["report"]
    base = _handle(monkeypatch, pid, {})["report"]
    _set_env(monkeypatch, env)
    _check(pid, h)
    print(pid, env, rep["kernels"], "early", rep["early"], "late", rep["late"], "| default: early", base["early"], "late", base["late"])
    assert base["kernels"] == dict(splitk="on", trsm="k_trsm_lite", nside=2)
    assert base["early"]["slabs"] > 0
    if "SCILMM_TRSM_LITE" in env:
        assert rep["kernels"]["trsm"] == "k_trsm<true>" and rep["early"] == base["early"] and rep["late"] == base["late"]
    elif "SCILMM_NO_SPLITK" in env:
        assert rep["kernels"]["splitk"] == "off"
        assert rep["early"]["slabs"] == 0 and rep["late"]["slabs"] == 0   # one item per tile and launch subtracts in place
        assert rep["early"]["items"] < base["early"]["items"] and rep["late"]["items"] <= base["late"]["items"]
    elif env == MANY_SLABS:
        assert rep["early"]["items"] > base["early"]["items"] and rep["early"]["hi"] > base["early"]["hi"]
        assert rep["late"]["slabs"] > base["late"]["slabs"]               # k_potrf and k_trsm fold slabs on load
    else:
        assert rep["early"]["items"] < base["early"]["items"] and rep["early"]["hi"] <= base["early"]["hi"]


@pytest.mark.parametrize("pid", ["P10", "R128"])
def test_odd_and_even_slab_counts_both_occur(pid, monkeypatch):
    """k_reduce folds the early slabs of a tile two at a time plus a remainder: the many-slab and the fewest-slab plans of a
    problem together hold tiles with an odd and tiles with an even count (MI355X, tiles odd / even, smallest .. largest count:
    P10 42 / 46, 2 .. 33 and 0 / 1, 2 .. 2; R128 324 / 342, 2 .. 37 and 66 / 187, 2 .. 3)."""
    reps = [_handle(monkeypatch, pid, env)["report"]["early"] for env in (MANY_SLABS, FEW_SLABS)]
    print(pid, "early (odd, even, lo, hi):", [(r["odd"], r["even"], r["lo"], r["hi"]) for r in reps])
    assert sum(r["odd"] for r in reps) > 0 and sum(r["even"] for r in reps) > 0
    assert max(r["hi"] for r in reps) >= 3                               # the two-way loop runs and leaves a remainder


# ---- k_outside

@pytest.mark.parametrize("pid,env", OUTSIDE_CASES, ids=_ids(OUTSIDE_CASES))
def test_outside_chunks_groups_and_priority(pid, env, monkeypatch):
    """k_outside: as many launches as asked for, capped by the number of distinct first panels; without the merge every
    descendant is its own group, with it the members of a group are summed in registers before the one atomic scatter."""
    h = _handle(monkeypatch, pid, env)
    sym, rep = h["sym"], h["report"]
    f, nd = _check(pid, h)
    facts = FS.outside_groups(sym)
    print(pid, env, rep["groups"], rep["chunks"], rep["prio"], "first panels", facts["first_panels"])
    assert (nd > 0) == ("SCILMM_DENSE" in env)
    assert rep["groups"]["descendants"] == facts["descendants"]
    if env.get("SCILMM_OUTSIDE_MERGE") == "0":
        assert rep["groups"]["groups"] == rep["groups"]["descendants"]
    else:
        assert rep["groups"]["groups"] == facts["groups"] < rep["groups"]["descendants"]
        assert rep["chunks"]["items"] == facts["pairs"]
    if "SCILMM_OUTSIDE_CHUNKS" in env:
        assert rep["chunks"]["chunks"] == min(int(env["SCILMM_OUTSIDE_CHUNKS"]), facts["first_panels"])
    assert rep["prio"] == ("the chain's" if env.get("SCILMM_OUTSIDE_PRIO") == "1" else "the look-ahead streams'")
    # equal to rounding between runs (atomics), as test_gpu_parity.test_outside_kernel_repeatable_to_rounding states it
    s2 = FS.problem(pid)["sigma2"]
    ld1, L1 = f.logdet(), f.L()
    before = sym.timing()["n_float_atomic_launches"]
    f.refactorize([0.7, 0.2])
    # (k_outside is the factorization's only kernel that sums with atomics: one launch per chunk)
    assert sym.timing()["n_float_atomic_launches"] - before == rep["chunks"]["chunks"] > 0
    f.refactorize(s2)
    ld2, L2 = f.logdet(), f.L()
    assert abs(ld1 - ld2) < 1e-12 * abs(ld1)
    assert np.array_equal(L1.indices, L2.indices) and np.abs(L1.data - L2.data).max() < 1e-12 * np.abs(L1.data).max()


# ---- side streams

@pytest.mark.parametrize("pid,env", STREAM_CASES, ids=_ids(STREAM_CASES))
def test_side_streams(pid, env, monkeypatch):
    h = _handle(monkeypatch, pid, env)
    assert h["report"]["kernels"]["nside"] == int(env["SCILMM_SIDE_STREAMS"])
    f, nd = _check(pid, h)
    assert (nd > 0) == ("SCILMM_DENSE" in env)


def test_side_streams_do_not_move_a_bit_on_deterministic_handles(monkeypatch):
    """Deterministic handles sum in a fixed slab order and use no atomics; SCILMM_SIDE_STREAMS only moves the early launches
    between streams, so 1, 2 and 3 streams give the same bits.  A difference is a missing dependency between streams."""
    p = FS.problem("P10")
    got = {}
    for k in ("1", "2", "3"):
        h = _handle(monkeypatch, "P10", {"SCILMM_SIDE_STREAMS": k}, deterministic=True)
        assert h["sym"].deterministic and h["report"]["kernels"]["nside"] == int(k)
        f = h["sym"].factorize(p["sigma2"])
        assert h["sym"].timing()["n_float_atomic_launches"] == 0
        got[k] = (f.logdet(), f.L().data.copy())
    o = _oracle("P10")
    assert abs(got["2"][0] - o.logdet()) < TOL * abs(o.logdet())
    for k in ("1", "3"):
        assert got[k][0] == got["2"][0], (k, got[k][0], got["2"][0])
        assert np.array_equal(got[k][1], got["2"][1]), (k, np.abs(got[k][1] - got["2"][1]).max())
