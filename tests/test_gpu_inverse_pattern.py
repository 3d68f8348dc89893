"""``scilmm_inverse_pattern_dev``: the entries of ``M = alpha diag(s) V^-1 diag(s) + beta T T'`` on V's own pattern, read off an
inverted handle, against ``numpy.linalg.inv`` of the dense V -- on the diagonal and on EVERY pattern slot.

Problems: G1 (pedigree, n = 1472: no multiple of 64, 128 or 256, pattern columns of 2 to 209 slots, K = 2) and two of
tests/sinv_oracle.py: A (dense n = 1101: nine dense-tail fronts, every pattern entry in a tail panel) and P (pedigree n = 4780,
651 prelude fronts under a dense tail: pattern entries in both kinds of panel).  Tolerance: the project's 1e-9 relative
max-norm (tests.helpers.rel_err; sinv_oracle.ENTRY_TOL).  Every comparison prints its measured error."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from scilmm_amd import _lib
from tests import blup_oracle as O
from tests import sinv_oracle as SO
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

TOL = SO.ENTRY_TOL
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _CACHE.clear()


def _problem(pid):
    if pid == "G1":
        A = O.golden_g1()[0]
        return dict(mats=[A, sp.identity(A.shape[0], format="csr")], sigma2=[0.4, 0.6], opts={})
    return SO.problem(pid)


def _case(pid, deterministic=False):
    """One handle per (problem, mode) with the dense inverse and the slots' pairs of individuals; the factor is inverted."""
    key = (pid, deterministic)
    if key not in _CACHE:
        from scilmm_amd.factor import Symbolic
        p = _problem(pid)
        sym = Symbolic(p["mats"], deterministic=deterministic, **p["opts"])
        n, P = sym.n, sym.P()
        colptr, rows = sym.get("pat_colptr"), sym.get("pat_row")
        assert rows.size == sym.info().nnz_pattern == colptr[-1]
        V = sum(s * sp.csr_matrix(m).toarray() for s, m in zip(p["sigma2"], p["mats"]))
        stored = sum(sp.csr_matrix((np.ones(m.nnz), m.indices, m.indptr), shape=m.shape) for m in map(sp.csr_matrix, p["mats"]))
        f = sym.factorize(p["sigma2"])
        f.selected_inverse()
        _CACHE[key] = dict(sym=sym, f=f, n=n, P=P, colptr=colptr, Z=np.linalg.inv(V), sigma2=p["sigma2"],
                           i=P[np.repeat(np.arange(n), np.diff(colptr))], j=P[rows], pattern=stored.toarray() != 0)
    return _CACHE[key]


def _call(h, alpha=1.0, s=None, beta=0.0, T=None, want=("diag", "off"), shift=0):
    """The entry point on device copies of ``s`` and ``T`` -> (diag, off) as NumPy arrays; an output not wanted is passed as
    NULL.  ``shift``: T starts that many doubles into its buffer (8-byte instead of 16-byte alignment)."""
    import torch
    vp = C.c_void_p
    f, n, nnz = h["f"], h["n"], h["i"].size
    ds = None if s is None else torch.from_numpy(np.ascontiguousarray(s)).cuda()
    c, dT = 0, None
    if T is not None:
        c = T.shape[1]
        dT = torch.zeros((shift + max(T.size, 1),), dtype=torch.float64, device="cuda")
        dT[shift:shift + T.size] = torch.from_numpy(np.ascontiguousarray(T).ravel()).cuda()
    dd = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
    do = torch.full((nnz,), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    f.inverse_pattern_dev(vp(dd.data_ptr()) if "diag" in want else None, vp(do.data_ptr()) if "off" in want else None, alpha,
                          None if ds is None else vp(ds.data_ptr()), beta, None if dT is None else vp(dT.data_ptr() + 8 * shift), c)
    h["sym"].sync()
    return dd.cpu().numpy(), do.cpu().numpy()


def _dense(h, alpha, s, beta, T):
    Z, n = h["Z"], h["n"]
    s = np.ones(n) if s is None else s
    M = alpha * (s[:, None] * Z * s[None, :])
    return M if T is None else M + beta * (T @ T.T)


def _compare(what, h, got, M):
    diag, off = got
    e1, e2 = rel_err(diag, np.diag(M)), rel_err(off, M[h["i"], h["j"]])
    print(what, "rel.err diag %.3e slots %.3e (%d slots)" % (e1, e2, off.size))
    assert e1 < TOL and e2 < TOL, what
    first = h["colptr"][:-1]
    assert np.array_equal(off[first], diag[h["P"]]), what + ": a diagonal slot holds the bits of the diagonal output"


@pytest.mark.parametrize("pid", ["G1", "A", "P"])
def test_inverse_on_pattern_against_the_dense_inverse(pid):
    h = _case(pid)
    Z = h["Z"]
    diag, M = h["f"].inverse_on_pattern()
    e = rel_err(diag, np.diag(Z))
    print(pid, "diagonal rel.err", e)
    assert e < TOL
    # the CSR holds V's pattern, both halves, and nothing else; every stored entry is the dense inverse's
    assert M.shape == Z.shape and M.has_sorted_indices
    got = np.zeros_like(Z, dtype=bool)
    rows = np.repeat(np.arange(h["n"]), np.diff(M.indptr))
    got[rows, M.indices] = True
    assert np.array_equal(got, h["pattern"] | np.eye(h["n"], dtype=bool))
    e = rel_err(M.data, Z[rows, M.indices])
    print(pid, "pattern rel.err", e, "entries", M.nnz)
    assert e < TOL
    assert abs(M - M.T).max() == 0.0
    _compare(pid + " raw:", h, _call(h), Z)


@pytest.mark.parametrize("pid", ["G1", "P"])
@pytest.mark.parametrize("c", [0, 1, 5, 32])
def test_random_scaling_and_low_rank_term(pid, c):
    h = _case(pid)
    n = h["n"]
    rng = np.random.default_rng(100 + c)
    s = rng.uniform(0.5, 2.0, n)
    T = rng.standard_normal((n, c)) / np.sqrt(max(c, 1)) * np.sqrt(np.abs(np.diag(h["Z"])).max())
    alpha, beta = -1.3, 0.7
    M = _dense(h, alpha, s, beta, T if c else None)
    both = _call(h, alpha, s, beta, T)
    _compare("%s c = %d:" % (pid, c), h, both, M)
    # either output alone: the same bits, and the other buffer is not written
    d_only = _call(h, alpha, s, beta, T, want=("diag",))
    o_only = _call(h, alpha, s, beta, T, want=("off",))
    assert np.array_equal(d_only[0], both[0]) and np.all(np.isnan(d_only[1]))
    assert np.array_equal(o_only[1], both[1]) and np.all(np.isnan(o_only[0]))
    if c:
        # rows of T read 8 bytes at a time (odd c, or a base that is not 16-byte aligned) or 16: the same bits
        moved = _call(h, alpha, s, beta, T, shift=1)
        assert np.array_equal(moved[0], both[0]) and np.array_equal(moved[1], both[1])
    # s = NULL is s = 1, T = NULL is no low-rank term whatever c says
    _compare("%s c = %d, no s:" % (pid, c), h, _call(h, alpha, None, beta, T), _dense(h, alpha, None, beta, T if c else None))
    import torch
    vp = C.c_void_p
    dd = torch.empty((n,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    h["f"].inverse_pattern_dev(vp(dd.data_ptr()), None, 2.0, None, 5.0, None, c)
    h["sym"].sync()
    e = rel_err(dd.cpu().numpy(), 2.0 * np.diag(h["Z"]))
    print("null T rel.err", e)
    assert e < TOL


def test_state_and_argument_errors():
    import torch
    from scilmm_amd import ScilmmError
    from scilmm_amd.factor import Symbolic
    p = _problem("G1")
    sym = Symbolic(p["mats"])
    f = sym.factorize(p["sigma2"])
    L, vp = _lib.lib(), C.c_void_p
    dd = torch.zeros((sym.n,), dtype=torch.float64, device="cuda")
    do = torch.zeros((int(sym.info().nnz_pattern),), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    args = lambda c=0, d=dd, o=do: (f._h, 1.0, None, 0.0, None, c, None if d is None else vp(d.data_ptr()),
                                    None if o is None else vp(o.data_ptr()))
    assert L.scilmm_inverse_pattern_dev(*args()) == _lib.ERR_STATE            # factorized, not inverted
    with pytest.raises(ScilmmError, match="scilmm_selected_inverse"):
        f.inverse_pattern_dev(vp(dd.data_ptr()), vp(do.data_ptr()))
    with pytest.raises(ScilmmError):
        f.inverse_on_pattern()
    B = np.random.default_rng(0).standard_normal((sym.n, 2))
    before = f(B)                                                              # the refusals left the factor usable
    f.selected_inverse()
    for bad in (args(c=33), args(c=-1), args(d=None, o=None)):
        assert L.scilmm_inverse_pattern_dev(*bad) == _lib.ERR_ARG
    assert L.scilmm_inverse_pattern_dev(*args()) == _lib.OK
    assert L.scilmm_inverse_pattern_dev(*args()) == _lib.OK                    # the handle stays inverted: repeatable
    sym.sync()
    assert dd.cpu().numpy().all()
    f.refactorize(p["sigma2"])
    assert L.scilmm_inverse_pattern_dev(*args()) == _lib.ERR_STATE            # a factor again
    e = rel_err(f(B), before)
    print("solve after inversion + refactorization rel.err", e)
    assert e < 1e-10


@pytest.mark.parametrize("pid", ["G1", "P"])
def test_deterministic_handle_repeats_its_bits(pid):
    h = _case(pid, deterministic=True)
    assert h["sym"].deterministic
    rng = np.random.default_rng(3)
    s, T = rng.uniform(0.5, 2.0, h["n"]), rng.standard_normal((h["n"], 4))
    first = _call(h, -1.0, s, 1.0, T)
    _compare(pid + " deterministic:", h, first, _dense(h, -1.0, s, 1.0, T))
    again = _call(h, -1.0, s, 1.0, T)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    h["f"].refactorize(h["sigma2"])
    h["f"].selected_inverse()                                                  # a second inversion of the same factor
    second = _call(h, -1.0, s, 1.0, T)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    assert h["sym"].timing()["n_float_atomic_launches"] == 0


def test_default_handle_call_adds_no_float_atomic_launch():
    h = _case("P")
    before = h["sym"].timing()["n_float_atomic_launches"]
    T = np.random.default_rng(4).standard_normal((h["n"], 6))
    a, b = _call(h, 1.0, None, 1.0, T), _call(h, 1.0, None, 1.0, T)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])        # the call's own bits depend on its inputs alone
    assert h["sym"].timing()["n_float_atomic_launches"] == before
