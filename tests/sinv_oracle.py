"""Dense reference for the selected inverse (host only; nothing here calls the engine).

Given the matrices A_k, sigma2 and a permutation P it forms V = sum_k s_k A_k densely, inverts it with LAPACK in fp64 and
offers Zd = inv(V)[P][:,P], the traces np.sum(inv(V) * A_k) and the dense Cholesky factor of V[P][:,P].  Every problem of
the tests that use it has cond(V) < 1e2, so the reference itself is good to about 1e-14.

`compare_entries` takes what `Factor.L()` returns on an inverted handle, with the panel layout of the analysis
(`export_layout`), and compares EVERY stored position (indptr / indices / data; never `.nonzero()`, which would leave out
an entry that was cleared and never written).  The error is normalised per front panel -- max|Z - Zd| over the panel over
max|Zd| over the same panel; a panel contains its diagonal block, so the scale is never small -- and held to the project's
1e-9.

The four problems of tests/test_gpu_selected_inverse.py live here too, with the facts of the host analysis the GPU cases
rely on (tests/test_selected_inverse_shapes.py asserts them without a GPU).
"""
import numpy as np
import scipy.linalg as la
import scipy.sparse as sp

ENTRY_TOL = 1e-9    # per-panel relative error of an entry of Z
TRACE_TOL = 1e-9    # relative error of tr(V^-1 A_k)
FACTOR_TOL = 1e-10  # L / log-det / solve before an inversion (tests/test_gpu_parity.TOL)


def dense_spd(n, seed=0):
    G = np.random.default_rng(seed).standard_normal((n, n))
    return sp.csr_matrix(G @ G.T + n * np.eye(n))


def _dense_problem(n, **opts):
    return dict(mats=[dense_spd(n)], sigma2=[1.0], sigma2_b=[1.7], opts=dict(ordering="natural", **opts))


def _pedigree_problem():
    from tests.helpers import small_pedigree
    A, _ = small_pedigree(6000, 0.01, 5)
    return dict(mats=[A, sp.identity(A.shape[0], format="csr")], sigma2=[0.35, 0.65], sigma2_b=[0.5, 0.5], opts={})


# id -> (builder, facts of the host analysis: n, nsuper, dense_first, widths of the tail fronts)
PROBLEMS = {
    "A": (lambda: _dense_problem(1101), dict(n=1101, nsuper=9, dense_first=0, tail=[128] * 8 + [77])),
    "B": (lambda: _dense_problem(4500, max_width=32), dict(n=4500, nsuper=141, dense_first=0, tail=[32] * 140 + [20])),
    "C": (lambda: _dense_problem(6500, max_width=96), dict(n=6500, nsuper=68, dense_first=0, tail=[96] * 67 + [68])),
    "P": (_pedigree_problem, dict(n=4780, nsuper=655, dense_first=651, tail=[128, 128, 128, 62])),
}
_BUILT = {}


def problem(pid):
    """The problem's matrices, sigma2 (and a second sigma2 for refactorizations) and Symbolic options; built once."""
    if pid not in _BUILT:
        _BUILT[pid] = PROBLEMS[pid][0]()
    return _BUILT[pid]


class DenseReference(object):
    """inv(V), Zd, the traces and the Cholesky factor of V[P][:,P], all dense fp64 (LAPACK)."""

    def __init__(self, mats, sigma2, perm):
        self.mats = [sp.csr_matrix(m) for m in mats]
        self.sigma2 = np.asarray(sigma2, dtype=np.float64)
        self.perm = np.asarray(perm, dtype=np.int64)
        self.n = n = self.mats[0].shape[0]
        assert sorted(self.perm.tolist()) == list(range(n))
        V = np.zeros((n, n))
        for s, m in zip(self.sigma2, self.mats):
            V += s * m.toarray()
        Vp = V[np.ix_(self.perm, self.perm)]
        self.Ld = la.cholesky(Vp, lower=True)                       # the unique factor for this P
        self.Zd = la.cho_solve((self.Ld, True), np.eye(n))          # = inv(V)[P][:,P]
        self.Zd = 0.5 * (self.Zd + self.Zd.T)
        X = np.random.default_rng(1).standard_normal((n, 3))
        resid = np.abs(self.Zd @ (Vp @ X) - X).max()
        assert resid < 1e-11, resid                                 # the reference checks itself

    def traces(self):
        """tr(V^-1 A_k) = sum(inv(V) * A_k), elementwise on dense arrays."""
        inv = np.argsort(self.perm)
        Vi = self.Zd[np.ix_(inv, inv)]                              # back to the matrices' own labels
        return np.array([np.sum(Vi * m.toarray()) for m in self.mats])

    def logdet(self):
        return 2.0 * np.log(np.diag(self.Ld)).sum()

    def solve(self, b):
        x = la.cho_solve((self.Ld, True), np.asarray(b, dtype=np.float64)[self.perm])
        out = np.empty_like(x)
        out[self.perm] = x
        return out


def export_layout(sn_start, sn_rowptr, nnzL_stored):
    """(first column of every front, number of entries `scilmm_export_L` reports) from the analysis' arrays: the stored
    panels minus the strict upper triangles of their diagonal blocks.  `nnzL_stored` counts the same panels plus one
    alignment slot after every panel with an odd number of entries (panels start 16-byte aligned); the two must agree."""
    start, rowptr = np.asarray(sn_start, dtype=np.int64), np.asarray(sn_rowptr, dtype=np.int64)
    w, m = np.diff(start), np.diff(rowptr)
    assert w.size == m.size and np.all(w > 0) and np.all(m >= w)
    count = int((m * w - w * (w - 1) // 2).sum())
    assert int(nnzL_stored) - int((w * (w - 1) // 2).sum()) - int(((m * w) % 2).sum()) == count, (int(nnzL_stored), count)
    return start, count


def _positions(M, layout):
    """(rows, cols, data, first entry of every panel) of every stored position of the exported CSC, lower triangle only,
    after checking that it is the whole export."""
    M = sp.csc_matrix(M)
    n = M.shape[0]
    sn_start, count = layout
    assert sn_start[0] == 0 and sn_start[-1] == n
    indptr, rows, data = M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data
    assert rows.size == data.size == indptr[-1] == count, (rows.size, int(indptr[-1]), count)
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    assert np.all(rows >= cols) and np.all(rows < n)
    assert np.all(rows[indptr[:-1]] == np.arange(n))                # every column starts with its diagonal entry
    return rows, cols, data, indptr[sn_start[:-1]]


def compare_entries(Z, Zd, layout, tol=ENTRY_TOL, what=""):
    """Every stored position of Z (the CSC of `Factor.L()` on an inverted handle) against the dense Zd; returns the largest
    per-panel relative error, raises AssertionError naming the worst entry when it is not below `tol`."""
    sn_start = layout[0]
    rows, cols, data, panel_first = _positions(Z, layout)
    ref = Zd[rows, cols]
    assert np.all(np.isfinite(data)), "%s: %d non-finite entries" % (what, int((~np.isfinite(data)).sum()))
    diff = np.abs(data - ref)
    scale = np.maximum.reduceat(np.abs(ref), panel_first)           # per front panel (entries of a panel are contiguous)
    front_of = np.searchsorted(sn_start, cols, side="right") - 1
    rel = diff / scale[front_of]
    e = int(np.argmax(rel))
    worst = float(rel[e])
    if not worst < tol:
        rf = int(np.searchsorted(sn_start, rows[e], side="right") - 1)
        raise AssertionError("%s: selected inverse off by %.3e of its panel's scale (limit %.1e) at (column front %d, row front %d, "
                             "row %d, column %d): got %.17g, want %.17g; %d of %d entries over the limit"
                             % (what, worst, tol, int(front_of[e]), rf, int(rows[e]), int(cols[e]), data[e], ref[e],
                                int((rel >= tol).sum()), rel.size))
    return worst


def compare_traces(tr, ref, tol=TRACE_TOL, what=""):
    tr, want = np.asarray(tr), ref.traces()
    err = np.abs(tr - want) / np.abs(want)
    assert np.all(err < tol), "%s: traces %s, want %s (relative error %s, limit %.1e)" % (what, tr, want, err, tol)
    ident = abs(ref.sigma2 @ tr - ref.n) / ref.n                    # tr(V^-1 V) = n
    assert ident < tol, "%s: sigma2 . tr = %.15g, n = %d" % (what, ref.sigma2 @ tr, ref.n)
    return float(max(err.max(), ident))


def check_factor(f, ref, layout, rs=(1, 5, 103), tol=FACTOR_TOL, what=""):
    """The L / log-det / solve checks of tests/test_gpu_parity._check_factor against the dense reference: `f.L()` equals the
    reference factor AS A MATRIX (stored positions that are structurally zero -- relaxation and tail padding -- must hold
    zeros), nothing of the reference lies outside the stored pattern.  Returns the number of stored structural zeros."""
    n = ref.n
    assert abs(f.logdet() - ref.logdet()) <= tol * max(1.0, abs(ref.logdet())), (what, "logdet")
    rng = np.random.default_rng(n)
    for r in rs:
        B = rng.standard_normal((n, r))
        want = ref.solve(B)
        assert np.abs(f(B) - want).max() < tol * np.abs(want).max(), (what, "solve", r)
    rows, cols, data, _ = _positions(f.L(), layout)
    want = ref.Ld[rows, cols]
    scale = np.abs(ref.Ld).max()
    err = np.abs(data - want).max()
    assert err < tol * scale, (what, "L", err / scale)
    # the lower triangle of the reference has nothing outside the stored pattern: the squares add up
    total, stored = np.sum(np.tril(ref.Ld) ** 2), np.sum(want ** 2)
    assert abs(total - stored) <= 1e-12 * total, (what, "pattern", total, stored)
    zeros = want == 0.0
    assert np.abs(data[zeros]).max(initial=0.0) < tol * scale, (what, "padding")
    return int(zeros.sum())
