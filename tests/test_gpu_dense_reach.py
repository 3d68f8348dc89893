"""The dense-tail plan's per-tile-pair reach: an item's K range is trimmed to the first and last descendant whose true rows reach
the item's 256 rows, and an item that no descendant of its segment reaches is still emitted, empty, and stores zeros to its
partial slabs (csrc/plan.hip emit_dense_items; k_dense_b, k_dense_h, k_dense32 in csrc/kernels.hip.h).

  P20, P10   pedigree tails (padded block pattern) with SCILMM_DENSE=1, at the default item count and with 64 items per launch:
             `_check_factor` of tests/test_gpu_parity.py (L entry by entry, log-det, solves and L*R against the oracle at 1e-10).
             The plan's report has to show what tests/dense_reach.py replays from the host analysis; on P20 that is 1112 of 1121
             products and 9 empty items at both item counts (tests/test_dense_reach_replay.py holds the figures without a GPU),
             so the zero-slab path runs.
  R128       a dense matrix: every descendant reaches every tile pair, the report shows kept == all, and L is bit for bit the L
             of the loop before the feed change (SCILMM_DENSE_FEED=0) -- the trim touches nothing.
  P20, fp32  front precision 32 through the shadow (k_dense_h) and with SCILMM_SHADOW=0 (k_dense32), at the fp32 bounds of
             tests/test_gpu_factor_schedules.py: factor within 1e-5 of the fp64 oracle and not equal to it, log-det 1e-7, refined
             solves 1e-10.
"""
import re

import numpy as np
import pytest

from tests import dense_reach as DR
from tests import factor_shapes as FS
from tests.test_gpu_parity import TOL, _check_factor
from tests.test_gpu_selected_inverse import _stderr_text

pytestmark = pytest.mark.gpu

SWITCHES = ("SCILMM_TUNING", "SCILMM_DENSE", "SCILMM_DENSE_ITEMS", "SCILMM_DENSE_FEED", "SCILMM_DENSE_FILL", "SCILMM_DENSE_TAPER",
            "SCILMM_SHADOW", "SCILMM_DETERMINISTIC", "SCILMM_VERBOSE", "SCILMM_NO_MFMA", "SCILMM_NO_LOOKAHEAD", "SCILMM_LOOK_DEPTH")
REACH = re.compile(r"dense tail: per-pair reach keeps (\d+) of (\d+) \(tile pair, descendant\) products, (\d+) empty items")
ITEMS = re.compile(r"dense tail: fronts (\d+)\.\.(\d+) \((\d+) wide\), (\d+) early \+ (\d+) late implicit items")
FP32_KERNEL = re.compile(r"fp32 fronts: (k_dense_h|k_dense32)\b")

_ORACLES = {}
_HANDLES = {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _ORACLES.clear()
    _HANDLES.clear()


def _oracle(pid):
    """The oracle's factor of the problem under the engine's permutation, built once."""
    if pid not in _ORACLES:
        from oracle import oracle as O
        from scilmm_amd.factor import Symbolic
        p = FS.problem(pid)
        perm = Symbolic(p["mats"], upload=False, **p["opts"]).P()
        V = sum(s * m for s, m in zip(p["sigma2"], p["mats"])).tocsr()
        _ORACLES[pid] = O.OracleFactor(V, perm)
    return _ORACLES[pid]


def _handle(monkeypatch, pid, items, deterministic=None):
    """One handle per (problem, items per launch), created under SCILMM_DENSE=1, with the plan's report; leaves that
    environment set."""
    from scilmm_amd.factor import Symbolic
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SCILMM_TUNING", "1")
    monkeypatch.setenv("SCILMM_DENSE", "1")
    if items:
        monkeypatch.setenv("SCILMM_DENSE_ITEMS", str(items))
    key = (pid, items, deterministic)
    if key not in _HANDLES:
        p = FS.problem(pid)
        text = []
        monkeypatch.setenv("SCILMM_VERBOSE", "1")
        with _stderr_text(text):
            sym = Symbolic(p["mats"], deterministic=deterministic, **p["opts"])
        monkeypatch.delenv("SCILMM_VERBOSE")
        m, mi = REACH.search(text[0]), ITEMS.search(text[0])
        assert m and mi, text[0]
        kept, total, empty = map(int, m.groups())
        _HANDLES[key] = dict(sym=sym, kept=kept, all=total, empty=empty, early=int(mi.group(4)), late=int(mi.group(5)))
    return _HANDLES[key]


@pytest.mark.parametrize("items", [None, 64], ids=["default-items", "items64"])
@pytest.mark.parametrize("pid", ["P20", "P10"])
def test_trimmed_and_empty_items_give_the_oracles_factor(pid, items, monkeypatch):
    h = _handle(monkeypatch, pid, items)
    want = DR.replay(h["sym"], items or 128)
    got = {k: h[k] for k in ("all", "kept", "empty", "early", "late")}
    print(pid, items, "plan", got, "replay", want)
    assert got == want
    if pid == "P20":
        assert h["kept"] < h["all"] and h["empty"] >= 1          # the zero-slab path runs
    p = FS.problem(pid)
    _check_factor(p["mats"], p["sigma2"], h["sym"], rs=(5, 103), oracle=_oracle(pid))


def test_dense_matrix_keeps_every_product_and_the_bits(monkeypatch):
    h = _handle(monkeypatch, "R128", None, deterministic=True)
    assert h["kept"] == h["all"] > 0 and h["empty"] == 0
    p = FS.problem("R128")
    f = h["sym"].factorize(p["sigma2"])
    L_new = f.L()
    monkeypatch.setenv("SCILMM_DENSE_FEED", "0")
    f.refactorize(p["sigma2"])
    assert np.array_equal(f.L().data, L_new.data)


@pytest.mark.parametrize("shadow", ["1", "0"], ids=["k_dense_h", "k_dense32"])
def test_fp32_fronts_on_trimmed_and_empty_items(shadow, monkeypatch):
    from tests.helpers import rel_err
    h = _handle(monkeypatch, "P20", None)
    assert h["empty"] >= 1
    sym, p, o = h["sym"], FS.problem("P20"), _oracle("P20")
    s2 = p["sigma2"]
    V = sum(s * m for s, m in zip(s2, p["mats"])).tocsr()
    Lo = o.L()
    scale = np.abs(Lo.data).max()
    f = sym.factorize(s2)
    monkeypatch.setenv("SCILMM_SHADOW", shadow)
    sym.set_front_precision(32)
    try:
        text = []
        monkeypatch.setenv("SCILMM_VERBOSE", "1")
        with _stderr_text(text):
            f.refactorize(s2)
        monkeypatch.delenv("SCILMM_VERBOSE")
        m = FP32_KERNEL.search(text[0])
        assert m and m.group(1) == ("k_dense32" if shadow == "0" else "k_dense_h"), text[0]
        errL = np.abs((f.L() - Lo).tocsr().data).max() / scale
        errld = abs(f.logdet() - o.logdet()) / abs(o.logdet())
        print("P20 %s: errL %.3e (limit 1e-5), log-det %.3e (limit 1e-7)" % (m.group(1), errL, errld))
        assert 0.0 < errL < 1e-5, errL
        assert errld < 1e-7, errld
        B = np.random.default_rng(3).standard_normal((V.shape[0], 5))
        X = f(B)
        assert rel_err(X, o(B)) < TOL                                 # refined solve
        assert rel_err(V @ X, B) < 1e-11
    finally:
        sym.set_front_precision(64)
