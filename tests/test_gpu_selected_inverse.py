"""The selected inverse where it has a DENSE TAIL: every stored entry of Z and every trace against the dense LAPACK
inverse (tests/sinv_oracle.py), on the problems whose host analysis reaches `k_sinv_tail`, `k_sinv_zero`, the transposed-Y
branches of `k_sinv_y` / `k_sinv_cc`, the tail branch of `sinv_offset` and the item planner of `ensure_sinv_plan`:

  A  dense SPD n = 1101, natural order: 9 tail fronts (last 77 wide), two B chunks per front, the ragged one 13 deep, one
     later front per item;
  B  dense n = 4500, max_width = 32: 141 fronts (last 20), items over several later fronts, every chunk shorter than the LDS
     buffer, a last row tile of fewer than 256 rows;
  C  dense n = 6500, max_width = 96: 68 fronts (last 68 = 64 + 4), items over several fronts of two chunks each;
  P  pedigree n = 4780, K = 2: 651 prelude fronts under a padded tail of 128 / 128 / 128 / 62 columns.

(tests/test_selected_inverse_shapes.py holds these facts without a GPU; `test_the_problems_reach_the_tail_kernels` reads the
plan's own report.)  Entries: 1e-9 of the front panel's largest reference entry; traces: 1e-9 relative; the factor on the
same handle passes the L / log-det / solve checks of test_gpu_parity at 1e-10 before every inversion.  Deterministic mode
and fp32 fronts leave the selected inverse alone and are not covered here."""
import contextlib
import os
import re
import sys
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp

from tests import sinv_oracle as SO

pytestmark = pytest.mark.gpu

MODES = {"default": {},
         "generic": {"SCILMM_TUNING": "1", "SCILMM_SINV_GENERIC": "1"},   # the gather kernel for the tail too
         "nomfma": {"SCILMM_TUNING": "1", "SCILMM_NO_MFMA": "1"}}          # scalar kernels (fixed when the device plan is built)
CASES = [("A", "default"), ("B", "default"), ("C", "default"), ("P", "default"),
         ("A", "generic"), ("B", "generic"), ("P", "generic"), ("A", "nomfma"), ("P", "nomfma")]
REPORT = re.compile(r"selected inverse: (\d+) tail fronts, (\d+) items, (\d+) of them over more than one front, pre-tail tiles (\d+)")

_HANDLES = {}   # (problem, mode) -> handle, analysis arrays, the plan's report
_REFS = {}      # (problem, sigma2) -> DenseReference


@pytest.fixture(scope="module", autouse=True)
def _release_the_problems():
    """The handles, the dense references and the dense matrices (a few GB on the host) go with the module."""
    yield
    _HANDLES.clear()
    _REFS.clear()
    SO._BUILT.clear()


def _set_mode(monkeypatch, mode):
    for k in ("SCILMM_TUNING", "SCILMM_SINV_GENERIC", "SCILMM_NO_MFMA", "SCILMM_DENSE", "SCILMM_DETERMINISTIC"):
        monkeypatch.delenv(k, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)


def _handle(pid, mode, mats=None, opts=None):
    """One Symbolic per (problem, mode), created under the mode's environment (the caller has set it)."""
    from scilmm_amd.factor import Symbolic
    key = (pid, mode)
    if key not in _HANDLES:
        p = SO.problem(pid) if mats is None else dict(mats=mats, opts=opts)
        sym = Symbolic(p["mats"], **p["opts"])
        _HANDLES[key] = dict(sym=sym, mats=p["mats"], dense_first=sym.info().dense_first, report=None,
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
    h["report"] = dict(zip(("tail_fronts", "items", "multi", "pre_tiles"), map(int, m.groups())))
    return tr


def _gate(h, f, ref, what):
    return SO.check_factor(f, ref, h["layout"], what=what)


def _check_inverse(h, f, ref, tr, what):
    e = SO.compare_entries(f.L(), ref.Zd, h["layout"], what=what)
    t = SO.compare_traces(tr, ref, what=what)
    ms = h["sym"].timing()
    print("%s: entries %.3e of the panel scale, traces %.3e (limits %.0e, %.0e); device: factorization %.1f ms, inversion %.1f ms"
          % (what, e, t, SO.ENTRY_TOL, SO.TRACE_TOL, ms["factor_ms"], ms["quad_ms"]))


@pytest.mark.parametrize("pid,mode", CASES)
def test_entries_and_traces_against_the_dense_inverse(pid, mode, monkeypatch):
    _set_mode(monkeypatch, mode)
    h = _handle(pid, mode)
    s2 = SO.problem(pid)["sigma2"]
    ref = _ref(pid, h, s2)
    f = h["sym"].factorize(s2)
    what = "%s/%s" % (pid, mode)
    _gate(h, f, ref, what)
    _check_inverse(h, f, ref, _invert(h, f), what)


@pytest.mark.parametrize("pid", ["P", "A"])
def test_second_inversion_on_the_same_handle(pid, monkeypatch):
    """Invert, refactorize at another sigma2, invert again: the plan is reused, the Y scratch and the panels hold the first
    inversion's numbers, `k_sinv_zero` has to clear what the atomics add to."""
    _set_mode(monkeypatch, "default")
    h = _handle(pid, "default")
    p = SO.problem(pid)
    f = h["sym"].factorize(p["sigma2"])
    _gate(h, f, _ref(pid, h, p["sigma2"]), pid + "/first")
    _invert(h, f)
    f.refactorize(p["sigma2_b"])
    ref = _ref(pid, h, p["sigma2_b"])
    _gate(h, f, ref, pid + "/second")
    _check_inverse(h, f, ref, _invert(h, f), pid + "/second inversion")


def test_refactorize_after_an_inversion_restores_the_tail_padding(monkeypatch):
    """After an inversion the padded positions of the tail panels hold entries of Z; the next factorization must put exact
    structure back: L as a matrix (stored zeros are zeros), the solves, and the log-det of before."""
    _set_mode(monkeypatch, "default")
    h = _handle("P", "default")
    s2 = SO.problem("P")["sigma2"]
    ref = _ref("P", h, s2)
    f = h["sym"].factorize(s2)
    ld = f.logdet()
    _invert(h, f)
    Z = f.L()
    f.refactorize(s2)
    padded = _gate(h, f, ref, "P/after inversion")
    assert abs(f.logdet() - ld) <= 1e-12 * abs(ld)
    # the check is about something: the tail stores structural zeros, and the inversion had filled them
    rows, cols, zdata, _ = SO._positions(Z, h["layout"])
    tail = cols >= h["layout"][0][h["dense_first"]]
    filled = tail & (ref.Ld[rows, cols] == 0.0) & (zdata != 0.0)
    print("P: %d stored structural zeros, %d of them in the tail and non-zero after the inversion" % (padded, int(filled.sum())))
    assert filled.sum() > 0


def test_traces_over_a_dense_a_weighted_diagonal_and_a_partial_matrix(monkeypatch):
    """K = 3 on problem A's pattern: the dense matrix, `sp.diags` of non-constant values (the diagonal-only path reads
    vals[j]) and a sparse symmetric matrix on a few positions, some of its diagonal entries not stored."""
    _set_mode(monkeypatch, "default")
    A = SO.problem("A")["mats"][0]
    n = A.shape[0]
    rng = np.random.default_rng(7)
    Dg = sp.diags(rng.uniform(0.5, 1.5, n) * n).tocsr()
    idx = rng.choice(n, 60, replace=False)
    i, j = rng.choice(idx, 200), rng.choice(idx, 200)
    keep = i != j
    off = sp.coo_matrix((rng.uniform(-0.2, 0.2, keep.sum()) * n, (i[keep], j[keep])), shape=(n, n))
    S = (off + off.T + sp.coo_matrix((np.full(30, 0.3 * n), (idx[:30], idx[:30])), shape=(n, n))).tocsr()
    S.sum_duplicates()
    S.sort_indices()
    touched = np.unique(S.nonzero()[0])
    assert (S.diagonal()[touched] == 0.0).sum() >= 10 and S.nnz < 500 and abs(S - S.T).max() == 0.0
    h = _handle("A3", "default", mats=[A, Dg, S], opts=dict(ordering="natural"))
    s2 = [1.0, 0.7, 0.4]
    ref = _ref("A3", h, s2)
    f = h["sym"].factorize(s2)
    _gate(h, f, ref, "A3")
    _check_inverse(h, f, ref, _invert(h, f), "A3")


def test_the_problems_reach_the_tail_kernels(monkeypatch):
    """From the plan's own report: without a tail, or without items over several fronts, the cases above would pass on the
    prelude kernels alone."""
    _set_mode(monkeypatch, "default")
    rep = {}
    for pid in "ABCP":
        h = _handle(pid, "default")
        if h["report"] is None:
            _invert(h, h["sym"].factorize(SO.problem(pid)["sigma2"]))
        rep[pid] = h["report"]
        assert rep[pid]["tail_fronts"] == len(SO.PROBLEMS[pid][1]["tail"]) and rep[pid]["items"] > 0, (pid, rep[pid])
    print(rep)
    assert rep["A"]["multi"] == 0 and rep["A"]["pre_tiles"] == 0
    assert rep["B"]["multi"] > 0 and rep["C"]["multi"] > 0
    assert rep["P"]["tail_fronts"] == 4 and rep["P"]["pre_tiles"] > 0
