"""The selected inverse in DETERMINISTIC mode: on a handle created with `deterministic=True` every stored entry of Z comes
from a sum whose order the plan fixes (`k_sinv_tail<true>` + `k_sinv_tail_fold`, `k_sinv_cc_ordered` + `k_sinv_cc_fold`), so

  * the entries and the traces meet the dense LAPACK inverse (tests/sinv_oracle.py) at the default mode's 1e-9,
  * a second inversion of the same matrix gives the same BITS, entries and traces,
  * turning the dispatch order of the ordered launches round (SCILMM_SINV_REVERSE) does not move a bit,
  * no launch of the handle summed with floating-point atomics (`n_float_atomic_launches == 0`),

on the problems A, B, C and P of tests/test_gpu_selected_inverse.py, with the segment length of the diagonal-block kernel
forced (SCILMM_SINV_CC_TILES) and in the scalar / gather forms.  Bits are compared inside ONE switch set only: another
segment length is another order of summation.  A default handle keeps the atomic kernels and counts them."""
import contextlib
import os
import re
import sys
import tempfile

import numpy as np
import pytest

from tests import sinv_oracle as SO

pytestmark = pytest.mark.gpu

SWITCHES = ("SCILMM_TUNING", "SCILMM_SINV_GENERIC", "SCILMM_NO_MFMA", "SCILMM_DENSE", "SCILMM_DETERMINISTIC",
            "SCILMM_SINV_CC_TILES", "SCILMM_SINV_REVERSE")
MODES = {"default": {},
         "tiles1": {"SCILMM_TUNING": "1", "SCILMM_SINV_CC_TILES": "1"},   # every front with two tiles of R is folded (default: 2)
         "tiles3": {"SCILMM_TUNING": "1", "SCILMM_SINV_CC_TILES": "3"},   # B: 36 tiles per early front, later ones ragged
         "generic": {"SCILMM_TUNING": "1", "SCILMM_SINV_GENERIC": "1"},   # the gather kernel for the tail too
         "nomfma": {"SCILMM_TUNING": "1", "SCILMM_NO_MFMA": "1"}}          # scalar kernels (fixed when the device plan is built)
REPORT = re.compile(r"selected inverse: (\d+) tail fronts, (\d+) items, (\d+) of them over more than one front, pre-tail tiles (\d+)")
ORDERED = re.compile(r"selected inverse, order-fixed: tail row tiles (\d+) direct, (\d+) folded from (\d+) slots \((\d+) bytes\); "
                     r"cc segments of up to (\d+) tiles: (\d+) direct, (\d+) folded \((\d+) bytes\)")

_HANDLES = {}   # (problem, mode, deterministic) -> handle, analysis arrays, the plan's report
_REFS = {}      # (problem, sigma2) -> DenseReference
_BITS = {}      # (problem, mode) -> (Z.data, traces) of the first inversion at the problem's sigma2


@pytest.fixture(scope="module", autouse=True)
def _release_the_problems():
    """The handles, the dense references and the dense matrices (a few GB on the host) go with the module."""
    yield
    _HANDLES.clear()
    _REFS.clear()
    _BITS.clear()
    SO._BUILT.clear()


def _set_mode(monkeypatch, mode, reverse=False):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    if reverse:
        monkeypatch.setenv("SCILMM_TUNING", "1")
        monkeypatch.setenv("SCILMM_SINV_REVERSE", "1")


def _handle(pid, mode, deterministic=True):
    """One Symbolic per (problem, switch set), created under the set's environment (the caller has set it)."""
    from scilmm_amd.factor import Symbolic
    key = (pid, mode, deterministic)
    if key not in _HANDLES:
        p = SO.problem(pid)
        sym = Symbolic(p["mats"], deterministic=deterministic, **p["opts"])
        assert sym.deterministic is deterministic
        _HANDLES[key] = dict(sym=sym, mats=p["mats"], report=None, ordered=None, text=None,
                             layout=SO.export_layout(sym.get("sn_start"), sym.get("sn_rowptr"), sym.info().nnzL_stored))
    return _HANDLES[key]


def _ref(pid, h, sigma2):
    key = (pid, tuple(float(s) for s in sigma2))
    if key not in _REFS:
        _REFS[key] = SO.DenseReference(h["mats"], sigma2, h["sym"].P())
    assert np.array_equal(_REFS[key].perm, h["sym"].P())   # (the analysis does not depend on the mode)
    return _REFS[key]


@contextlib.contextmanager
def _stderr_text(out):
    """The library's own stderr lines of the block, appended to the list `out`."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as fh:
        os.dup2(fh.fileno(), 2)
        try:
            yield
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            fh.seek(0)
            out.append(fh.read().decode(errors="replace"))


def _invert(h, f):
    """`f.inverse_traces()`; the handle's first inversion builds the plan, whose report is kept."""
    if h["report"] is not None:
        return f.inverse_traces()
    text = []
    had = os.environ.get("SCILMM_VERBOSE")
    os.environ["SCILMM_VERBOSE"] = "1"
    try:
        with _stderr_text(text):
            tr = f.inverse_traces()
    finally:
        if had is None:
            del os.environ["SCILMM_VERBOSE"]
        else:
            os.environ["SCILMM_VERBOSE"] = had
    m = REPORT.search(text[0])
    assert m, text[0]
    h["text"] = text[0]
    h["report"] = dict(zip(("tail_fronts", "items", "multi", "pre_tiles"), map(int, m.groups())))
    m = ORDERED.search(text[0])
    if m:
        h["ordered"] = dict(zip(("tail_direct", "tail_folded", "tail_slots", "tail_bytes", "T", "cc_direct", "cc_folded", "cc_bytes"),
                                map(int, m.groups())))
    return tr


def _inverted(pid, mode, monkeypatch, reverse=False):
    """Gate the factor at the problem's sigma2, invert: (handle, Z as exported, traces, reference)."""
    _set_mode(monkeypatch, mode, reverse)
    h = _handle(pid, mode)
    s2 = SO.problem(pid)["sigma2"]
    ref = _ref(pid, h, s2)
    f = h["sym"].factorize(s2)
    SO.check_factor(f, ref, h["layout"], what="%s/%s" % (pid, mode))
    tr = _invert(h, f)
    return h, f, f.L(), np.array(tr), ref


def _oracle_repeat_and_counter(pid, mode, monkeypatch):
    """The conditions of every switch set: oracle tolerances, the handle repeats itself bit for bit, no float atomics."""
    what = "%s/%s" % (pid, mode)
    h, f, Z, tr, ref = _inverted(pid, mode, monkeypatch)
    e = SO.compare_entries(Z, ref.Zd, h["layout"], what=what)
    t = SO.compare_traces(tr, ref, what=what)
    print("%s: entries %.3e of the panel scale, traces %.3e (limits %.0e, %.0e); order-fixed plan %s"
          % (what, e, t, SO.ENTRY_TOL, SO.TRACE_TOL, h["ordered"]))
    assert h["ordered"] is not None, h["text"]
    _BITS.setdefault((pid, mode), (Z.data.copy(), tr.copy()))
    s2 = SO.problem(pid)["sigma2"]
    f.refactorize(s2)
    tr2 = np.array(_invert(h, f))
    Z2 = f.L()
    assert np.array_equal(Z.data, Z2.data) and np.array_equal(Z.indices, Z2.indices), what
    assert np.array_equal(tr, tr2), (what, tr, tr2)
    assert np.array_equal(_BITS[(pid, mode)][0], Z2.data) and np.array_equal(_BITS[(pid, mode)][1], tr2), what
    assert h["sym"].timing()["n_float_atomic_launches"] == 0, what
    return h


@pytest.mark.parametrize("pid", ["A", "B", "C", "P"])
def test_entries_traces_same_bits_and_no_float_atomics(pid, monkeypatch):
    """The test that shows the feature: before the ordered kernels the counter was above 0 after an inversion."""
    _oracle_repeat_and_counter(pid, "default", monkeypatch)


@pytest.mark.parametrize("pid", ["A", "B", "P"])
def test_reversed_dispatch_order_gives_the_same_bits(pid, monkeypatch):
    """Workgroup b takes item grid - 1 - b in the ordered tail and cc kernels: what arrives first is turned round, every
    sum's order is tied to the item and stays -- "order-fixed", not "happened to arrive in the same order"."""
    if (pid, "default") not in _BITS:
        _oracle_repeat_and_counter(pid, "default", monkeypatch)
    h, f, Z, tr, ref = _inverted(pid, "default", monkeypatch, reverse=True)
    SO.compare_entries(Z, ref.Zd, h["layout"], what=pid + "/reversed")
    assert np.array_equal(_BITS[(pid, "default")][0], Z.data), pid
    assert np.array_equal(_BITS[(pid, "default")][1], tr), (pid, tr)
    assert h["sym"].timing()["n_float_atomic_launches"] == 0


@pytest.mark.parametrize("pid,mode", [("A", "tiles1"), ("P", "tiles1"), ("B", "tiles3")])
def test_forced_segment_lengths(pid, mode, monkeypatch):
    """T = 1: every front with more than one tile of R goes through slots and the fold; T = 3 on B: 36 (35 further down)
    tiles per early front, so the last segment of a front is ragged.  (Bits are not compared with another T's.)"""
    h = _oracle_repeat_and_counter(pid, mode, monkeypatch)
    assert h["ordered"]["T"] == int(MODES[mode]["SCILMM_SINV_CC_TILES"]) and h["ordered"]["cc_folded"] > 0, h["ordered"]


@pytest.mark.parametrize("pid,mode", [("A", "nomfma"), ("P", "nomfma"), ("B", "generic")])
def test_scalar_and_gather_forms(pid, mode, monkeypatch):
    """SCILMM_NO_MFMA: `k_sinv_cc_ordered<false>` behind the gather kernel; SCILMM_SINV_GENERIC: the matrix-core form of it
    on column-major Y for the tail fronts as well (no tail kernel: `k_sinv_w` stores each tile once)."""
    _oracle_repeat_and_counter(pid, mode, monkeypatch)


def test_the_report_of_the_ordered_plan(monkeypatch):
    """The second report line of a deterministic handle: each of the four paths is taken on at least one of A, B, P; the
    tail's row tiles are the analysis' (256 rows of R each, fronts with a later front), and with their slots they account
    for every item of the first line."""
    _set_mode(monkeypatch, "default")
    rep = {}
    for pid in "ABP":
        h = _handle(pid, "default")
        if h["report"] is None:
            _invert(h, h["sym"].factorize(SO.problem(pid)["sigma2"]))
        assert h["ordered"] is not None, h["text"]
        o, r = h["ordered"], h["report"]
        rep[pid] = o
        start = np.asarray(h["sym"].get("sn_start"), dtype=np.int64)
        n, df = int(start[-1]), h["sym"].info().dense_first
        u = n - start[df + 1:-1]                       # rows of R of every tail front but the last
        tiles = int(((u[u > 0] + 255) // 256).sum())
        assert o["tail_direct"] + o["tail_folded"] == tiles, (pid, o, tiles)
        assert o["tail_direct"] + o["tail_slots"] == r["items"], (pid, o, r)
        assert o["tail_bytes"] % (256 * 16 * 8) == 0 and o["cc_bytes"] % (128 * 128 * 8) == 0   # whole slots
        assert (o["tail_bytes"] > 0) == (o["tail_folded"] > 0) and (o["cc_bytes"] > 0) == (o["cc_folded"] > 0)
    print(rep)
    for key in ("tail_direct", "tail_folded", "cc_direct", "cc_folded"):
        assert any(rep[pid][key] > 0 for pid in "ABP"), (key, rep)


def test_a_default_handle_keeps_the_atomic_kernels(monkeypatch):
    _set_mode(monkeypatch, "default")
    h = _handle("A", "default", deterministic=False)
    s2 = SO.problem("A")["sigma2"]
    f = h["sym"].factorize(s2)
    before = h["sym"].timing()["n_float_atomic_launches"]
    tr = _invert(h, f)
    SO.compare_traces(tr, _ref("A", h, s2), what="A/default handle")
    assert h["sym"].timing()["n_float_atomic_launches"] > before   # k_sinv_tail and k_sinv_cc, atomic forms
    assert h["ordered"] is None and "order-fixed" not in h["text"], h["text"]
