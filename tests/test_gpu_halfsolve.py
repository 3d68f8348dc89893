"""The halves of factor(b): Factor.solve_L / solve_Lt / apply_P / apply_Pt against the oracle's factor (the Cholesky factor
of V[P][:, P] is unique, so the half-solves are compared directly), through every path the full solve takes: level sweep,
k_chain in its three window widths, SCILMM_NO_CHAIN, the scalar kernels, the pull form of deterministic mode."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as la
import scipy.sparse as sp
import scipy.sparse.linalg as sla

from tests.helpers import random_spd, rel_err, small_pedigree

pytestmark = pytest.mark.gpu

TOL = 1e-10   # sweeps against the oracle factor: the TOL of test_gpu_parity.py


class _Oracle(object):
    """L of the oracle for (V, P) and L^-1 B, L^-T B for one seeded block; computed once per problem, never modified."""

    def __init__(self, V, perm, r, seed):
        from oracle import oracle as O
        n = V.shape[0]
        self.B = np.random.default_rng(seed).standard_normal((n, r))
        L = O.OracleFactor(V, perm).L()
        if n <= 400:
            Ld = L.toarray()
            self.fwd = la.solve_triangular(Ld, self.B, lower=True)
            self.bwd = la.solve_triangular(Ld.T, self.B, lower=False)
        else:
            self.fwd = sla.spsolve_triangular(L.tocsr(), self.B, lower=True)
            self.bwd = sla.spsolve_triangular(L.T.tocsr(), self.B, lower=False)
        self.fwd, self.bwd = self.fwd.reshape(n, r), self.bwd.reshape(n, r)
        for a in (self.B, self.fwd, self.bwd):
            a.setflags(write=False)


def _check_halves(f, o, rs):
    for r in rs:
        B = o.B[:, :r]
        assert rel_err(f.solve_L(B), o.fwd[:, :r]) < TOL, ("solve_L", f.n, r)
        assert rel_err(f.solve_Lt(B), o.bwd[:, :r]) < TOL, ("solve_Lt", f.n, r)
        # the contract: the four pieces compose to factor(b)
        assert rel_err(f.apply_Pt(f.solve_Lt(f.solve_L(f.apply_P(B)))), f(B)) < TOL, ("composition", f.n, r)
    b = o.B[:, 0]
    x = f.solve_L(b)
    assert x.shape == (f.n,) and rel_err(x, o.fwd[:, 0]) < TOL
    x = f.solve_Lt(b)
    assert x.shape == (f.n,) and rel_err(x, o.bwd[:, 0]) < TOL
    assert f.apply_P(b).shape == (f.n,) and np.array_equal(f.apply_Pt(f.apply_P(b)), b)
    assert np.array_equal(f.apply_P(o.B), o.B[f.P()])


@pytest.mark.parametrize("mfma", ["1", "0"])
@pytest.mark.parametrize("n,density,seed", [(1, 1.0, 0), (2, 1.0, 1), (7, 0.5, 2), (65, 0.9, 5), (130, 0.5, 6), (300, 0.02, 8)])
def test_random_spd_half_solves(n, density, seed, mfma, monkeypatch):
    from scilmm_amd.factor import Symbolic
    monkeypatch.setenv("SCILMM_TUNING", "1")
    monkeypatch.setenv("SCILMM_NO_MFMA", "0" if mfma == "1" else "1")
    A = random_spd(n, density, seed)
    for ordering in ("amd", "natural"):
        f = Symbolic([A], ordering=ordering).factorize([1.0])
        _check_halves(f, _Oracle(A, f.P(), 130, n), (1, 5, 103, 130))   # 130 crosses RPMAX


def test_dense_block_chain_half_solves():
    """The dense 300 x 300 matrix of test_dense_block_chain: the split-supernode chain."""
    from scilmm_amd.factor import Symbolic
    n = 300
    G = np.random.default_rng(0).standard_normal((n, n))
    A = sp.csr_matrix(G @ G.T + n * np.eye(n))
    f = Symbolic([A], ordering="natural").factorize([1.0])
    _check_halves(f, _Oracle(A, f.P(), 103, n), (5, 103))


_PED = {}


def _pedigree():
    """small_pedigree(10000, 0.01, 5) with [0.35, 0.65]: built once; the oracle once per permutation."""
    if not _PED:
        A, _ = small_pedigree(10000, 0.01, 5)
        I = sp.identity(A.shape[0], format="csr")
        _PED.update(A=A, I=I, V=(0.35 * A + 0.65 * I).tocsr(), oracle={})
    return _PED


def _pedigree_oracle(perm):
    p = _pedigree()
    key = perm.tobytes()
    if key not in p["oracle"]:
        p["oracle"][key] = _Oracle(p["V"], perm, 103, 10000)
    return p["oracle"][key]


@pytest.mark.parametrize("env", [{}, {"SCILMM_NO_CHAIN": "1"},
                                 {"SCILMM_CHAIN_WIDE_T": "1", "SCILMM_CHAIN_FULL_T": "100000"},  # 64-column chain windows
                                 {"SCILMM_CHAIN_WIDE_T": "1", "SCILMM_CHAIN_FULL_T": "1"},       # 112-column chain windows
                                 {"SCILMM_NO_MFMA": "1"}])
def test_pedigree_10k_half_solves_under_each_schedule(monkeypatch, env):
    from scilmm_amd.factor import Symbolic
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if env:
        monkeypatch.setenv("SCILMM_TUNING", "1")
    p = _pedigree()
    f = Symbolic([p["A"], p["I"]]).factorize([0.35, 0.65])
    _check_halves(f, _pedigree_oracle(f.P()), (5, 103))


@pytest.mark.parametrize("env", [{}, {"SCILMM_NO_CHAIN": "1"}, {"SCILMM_CHAIN_WIDE_T": "1", "SCILMM_CHAIN_FULL_T": "1"}])
def test_deterministic_composition_is_the_full_solve_bit_for_bit(monkeypatch, env):
    """Same kernels in the same order: on a deterministic handle the composed halves ARE factor(b), and neither half
    launches a float-atomic kernel."""
    from scilmm_amd.factor import Symbolic
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if env:
        monkeypatch.setenv("SCILMM_TUNING", "1")
    p = _pedigree()
    sym = Symbolic([p["A"], p["I"]], deterministic=True)
    f = sym.factorize([0.35, 0.65])
    o = _pedigree_oracle(f.P())
    for r in (1, 5, 103):
        B = o.B[:, :r]
        assert rel_err(f.solve_L(B), o.fwd[:, :r]) < TOL, ("solve_L", r)
        assert rel_err(f.solve_Lt(B), o.bwd[:, :r]) < TOL, ("solve_Lt", r)
        assert np.array_equal(f.apply_Pt(f.solve_Lt(f.solve_L(f.apply_P(B)))), f(B)), ("bits", r)
    assert sym.timing()["n_float_atomic_launches"] == 0


def test_small_deterministic_handles_repeat_bits_too():
    """Level-sweep-only problems (no chain): n = 130 and 300, every width up to RPMAX."""
    from scilmm_amd.factor import Symbolic
    for n, density, seed in ((130, 0.5, 6), (300, 0.02, 8)):
        A = random_spd(n, density, seed)
        sym = Symbolic([A], deterministic=True)
        f = sym.factorize([1.0])
        B = np.random.default_rng(n).standard_normal((n, 128))
        for r in (1, 16, 103, 128):
            assert np.array_equal(f.apply_Pt(f.solve_Lt(f.solve_L(f.apply_P(B[:, :r])))), f(B[:, :r])), (n, r)
        assert sym.timing()["n_float_atomic_launches"] == 0


def test_refusals_leave_the_handle_usable(monkeypatch):
    from scilmm_amd import _lib
    from scilmm_amd.factor import Symbolic
    A = random_spd(300, 0.02, 8)
    I = sp.identity(300, format="csr")
    sym = Symbolic([A, I])
    f = sym.factorize([0.4, 0.6])
    B = np.random.default_rng(1).standard_normal((300, 5))
    ref = f(B)
    # r = 0 through the device entry point: an argument error, before anything is looked at
    one = C.c_void_p(8)
    assert _lib.lib().scilmm_solve_L_dev(f._h, one, 0, one) == _lib.ERR_ARG
    assert _lib.lib().scilmm_solve_Lt_dev(f._h, one, 0, one) == _lib.ERR_ARG
    # a factor consumed by the selected inverse: refused until it is refactorized
    f.inverse_traces()
    for half in (f.solve_L, f.solve_Lt):
        with pytest.raises(_lib.ScilmmError):
            half(B)
    f.refactorize([0.4, 0.6])
    assert rel_err(f.apply_Pt(f.solve_Lt(f.solve_L(f.apply_P(B)))), ref) < TOL
    # fp32 fronts: a half-solve cannot be refined against the exact V
    monkeypatch.setenv("SCILMM_TUNING", "1")
    monkeypatch.setenv("SCILMM_DENSE", "1")   # (the tail of a 10k pedigree is narrower than the automatic threshold)
    p = _pedigree()
    sym32 = Symbolic([p["A"], p["I"]])
    sym32.set_front_precision(32)
    f32 = sym32.factorize([0.35, 0.65])
    o = _pedigree_oracle(f32.P())
    B = o.B[:, :5]
    for half in (f32.solve_L, f32.solve_Lt):
        with pytest.raises(_lib.ScilmmError, match="fp32"):
            half(B)
    assert rel_err(p["V"] @ f32(B), B) < 1e-9    # ... and the refusal left the full, refined solve as it was
    sym32.set_front_precision(64)
    f32.refactorize([0.35, 0.65])
    assert rel_err(f32.solve_L(B), o.fwd[:, :5]) < TOL
