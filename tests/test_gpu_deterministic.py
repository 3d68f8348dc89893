"""Deterministic mode on the GPU (scilmm_set_deterministic): the same inputs give the same BITS for the factorization, the
solves, L*R, SpMM and quadratic forms -- inside one process and between two -- no launch of the mode sums with floating-point
atomics, and the order-fixed kernels (k_fwd_pull, k_spmm_row) meet the oracle at the tolerance of the default ones."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests.helpers import rel_err, small_pedigree, small_pedigree_k3

pytestmark = pytest.mark.gpu

TOL = 1e-10  # tests/test_gpu_parity.py: fp64, same permutation
GOLD = os.path.join(os.path.dirname(__file__), "golden")
P = importlib.import_module("scilmm_amd.SparseCholesky")


def _problem(seed=0):
    A, _ = small_pedigree(10000, 0.01, seed)
    return A, sp.identity(A.shape[0], format="csr")


def _round(sym, f, B):
    return f(B), f.lmul(B), sym.spmm(0, B), sym.quadforms(0, B), f.logdet()


def _same_bits_twice(r, seed=0):
    """X, Z, Y, q of one factor; refactorize elsewhere and back; again: every pair identical.  Returns the handle."""
    from scilmm_amd.factor import Symbolic
    A, I = _problem(seed)
    n = A.shape[0]
    sym = Symbolic([A, I], deterministic=True)
    assert sym.deterministic is True
    B = np.random.default_rng(17).standard_normal((n, r))
    f = sym.factorize([0.4, 0.6])
    first = _round(sym, f, B)
    f.refactorize([0.7, 0.2])
    f.refactorize([0.4, 0.6])
    second = _round(sym, f, B)
    for name, a, b in zip(("solve", "lmul", "spmm", "quadforms", "logdet"), first, second):
        assert np.array_equal(a, b), (name, r)
    return sym


def test_same_bits_in_one_process_and_no_float_atomics():
    sym = _same_bits_twice(103)
    # the counter is what makes the claim checkable: nothing this handle launched summed with floating-point atomics
    assert sym.timing()["n_float_atomic_launches"] == 0


@pytest.mark.parametrize("r", [1, 5, 130])
def test_same_bits_for_other_widths(r):
    assert _same_bits_twice(r).timing()["n_float_atomic_launches"] == 0


@pytest.mark.parametrize("env", [{"SCILMM_CHAIN_WIDE_T": "1", "SCILMM_CHAIN_FULL_T": "100000"},  # 64-column chain windows
                                 {"SCILMM_CHAIN_WIDE_T": "1", "SCILMM_CHAIN_FULL_T": "1"},       # 112-column chain windows
                                 {"SCILMM_NO_MFMA": "1"}])
def test_same_bits_under_each_schedule(monkeypatch, env):
    """Bits may differ BETWEEN schedules; each schedule must repeat itself."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SCILMM_TUNING", "1")
    assert _same_bits_twice(103).timing()["n_float_atomic_launches"] == 0


def test_counter_counts_on_a_default_handle(monkeypatch):
    from scilmm_amd.factor import Symbolic
    monkeypatch.delenv("SCILMM_DETERMINISTIC", raising=False)
    A, I = _problem(0)
    n = A.shape[0]
    sym = Symbolic([A, I])
    assert sym.deterministic is False
    f = sym.factorize([0.4, 0.6])
    B = np.random.default_rng(17).standard_normal((n, 103))
    f(B)
    f.lmul(B)
    assert sym.timing()["n_float_atomic_launches"] > 0  # the default mode still takes the atomic kernels


def _check_against_oracle(mats, sigma2, sym, rs):
    from oracle import oracle as O
    V = sum(s * m for s, m in zip(sigma2, mats)).tocsr()
    n = V.shape[0]
    f = sym.factorize(sigma2)
    o = O.OracleFactor(V, f.P())
    assert abs(f.logdet() - o.logdet()) <= TOL * max(1.0, abs(o.logdet()))
    rng = np.random.default_rng(n)
    for r in rs:
        B = rng.standard_normal((n, r))
        assert rel_err(f(B), o(B)) < TOL, ("solve", r)
        assert rel_err(f.lmul(B), o.lmul(B)) < TOL, ("lmul", r)
        for k, m in enumerate(mats):
            assert rel_err(sym.spmm(k, B), m @ B) < TOL, ("spmm", k, r)
            assert rel_err(sym.quadforms(k, B), O.quadforms(m, B)) < TOL, ("quadforms", k, r)
    return f


def test_parity_of_the_order_fixed_kernels():
    from scilmm_amd.factor import Symbolic
    A, I = _problem(5)
    sym = Symbolic([A, I], deterministic=True)
    _check_against_oracle([A, I], [0.4, 0.6], sym, rs=(1, 5, 103, 130))
    assert sym.timing()["n_float_atomic_launches"] == 0


def test_parity_without_chain_sweep_and_without_mfma(monkeypatch):
    """The level-by-level form of the whole forward sweep (no k_chain) and the scalar form of the pull kernel."""
    from scilmm_amd.factor import Symbolic
    monkeypatch.setenv("SCILMM_TUNING", "1")
    A, I = _problem(5)
    monkeypatch.setenv("SCILMM_NO_CHAIN", "1")
    _check_against_oracle([A, I], [0.4, 0.6], Symbolic([A, I], deterministic=True), rs=(5, 103))
    monkeypatch.delenv("SCILMM_NO_CHAIN")
    monkeypatch.setenv("SCILMM_NO_MFMA", "1")
    _check_against_oracle([A, I], [0.4, 0.6], Symbolic([A, I], deterministic=True), rs=(5, 103))


def test_parity_three_components():
    from scilmm_amd.factor import Symbolic
    A, D, _ = small_pedigree_k3(10000, 0.01, 0)
    I = sp.identity(A.shape[0], format="csr")
    sym = Symbolic([A, D, I], deterministic=True)
    _check_against_oracle([A, D, I], [0.3, 0.2, 0.5], sym, rs=(103,))
    assert sym.timing()["n_float_atomic_launches"] == 0


def test_fp32_fronts_refined_solve_repeats(monkeypatch):
    """fp32-product fronts: the solve is refined against the exact V through scilmm_spmm -- order-fixed in this mode -- so
    the refined solve repeats bit for bit and meets the oracle."""
    from oracle import oracle as O
    from scilmm_amd.factor import Symbolic
    monkeypatch.setenv("SCILMM_TUNING", "1")
    monkeypatch.setenv("SCILMM_DENSE", "1")  # (the dense-tail path, which fp32 fronts need, at this small size)
    A, I = _problem(0)
    n = A.shape[0]
    sym = Symbolic([A, I], deterministic=True)
    sym.set_front_precision(32)
    f = sym.factorize([0.4, 0.6])
    B = np.random.default_rng(3).standard_normal((n, 103))
    X1 = f(B)
    f.refactorize([0.7, 0.2])
    f.refactorize([0.4, 0.6])
    X2 = f(B)
    assert np.array_equal(X1, X2)
    o = O.OracleFactor((0.4 * A + 0.6 * I).tocsr(), f.P())
    assert rel_err(X1, o(B)) < TOL
    assert sym.timing()["n_float_atomic_launches"] == 0


def test_same_bits_in_two_fresh_processes():
    script = os.path.join(os.path.dirname(__file__), "deterministic_eval_script.py")
    outs = []
    for _ in range(2):
        p = subprocess.run([sys.executable, script], timeout=600, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0, p.stderr[-2000:]  # (stop at the first failure: nothing more is started)
        outs.append(p.stdout)
    print(outs[0])
    assert outs[0].count("nll=") == 2 and "atomics=0" in outs[0]
    assert outs[0] == outs[1]


def _record(mod):
    trace = []
    orig = mod.bolt_gradient_estimation

    def rec(x, *a, **k):
        nll, grad = orig(x, *a, **k)
        trace.append((np.array(x), nll, np.array(grad)))
        return nll, grad

    mod.bolt_gradient_estimation = rec
    return trace, orig


def _reml_trace(g, A, tag, fused):
    chol = P.SparseCholesky(perm=g["%s_perm" % tag], fused=fused, deterministic=True)
    trace, orig = _record(P)
    try:
        np.random.seed(1)
        res = P.REML(chol, [A], g["C"], g["y"].copy())
    finally:
        P.bolt_gradient_estimation = orig
    return trace, res


def test_reml_trajectory_repeats_and_follows_the_golden():
    """REML on G1, identity-order permutation, unfused, seed 1, twice in one process: identical traces; every evaluation
    shared with the reference's golden trajectory at nll 1e-9 / grad 1e-5, at least min(nref, 12) of them (the conditions
    tests/test_gpu_reml.py holds the default mode to).  The evaluation count is printed, not asserted: determinism fixes
    this engine's rounding, it does not make it the reference's."""
    g = np.load(os.path.join(GOLD, "G1_reml_2000.npz"))
    A = sp.csr_matrix((g["A_data"], g["A_indices"], g["A_indptr"]), shape=tuple(g["A_shape"]))
    t1, res1 = _reml_trace(g, A, "ident", False)
    t2, res2 = _reml_trace(g, A, "ident", False)
    nref = len(g["ident_nll"])
    print("deterministic REML ident/unfused: %d evaluations (golden %d), sigma2 distance to golden %.3e"
          % (len(t1), nref, rel_err(res1["covariance coefficients"], g["ident_sigma2"])))
    assert len(t1) == len(t2)
    for (x1, n1, g1), (x2, n2, g2) in zip(t1, t2):
        assert np.array_equal(x1, x2) and n1 == n2 and np.array_equal(g1, g2)
    k = 0
    while k < min(len(t1), nref) and rel_err(t1[k][0], g["ident_x"][k]) < 1e-6:
        k += 1
    assert k >= min(nref, 12), k
    for i in range(k):
        x, nll, grad = t1[i]
        assert abs(nll - g["ident_nll"][i]) < 1e-9 * abs(g["ident_nll"][i]), i
        assert rel_err(grad, g["ident_grad"][i]) < 1e-5, i


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag", ["amd", "ident"])
def test_reml_evaluation_counts_reported(tag, fused):
    """The four legs of the golden trajectory in deterministic mode: shared evaluations at the golden's tolerances; the
    evaluation count and the distance of sigma2 to the golden are printed (DESIGN.md records them)."""
    g = np.load(os.path.join(GOLD, "G1_reml_2000.npz"))
    A = sp.csr_matrix((g["A_data"], g["A_indices"], g["A_indptr"]), shape=tuple(g["A_shape"]))
    trace, res = _reml_trace(g, A, tag, fused)
    nref = len(g["%s_nll" % tag])
    print("deterministic REML %s/%s: %d evaluations (golden %d), sigma2 distance to golden %.3e"
          % (tag, "fused" if fused else "unfused", len(trace), nref, rel_err(res["covariance coefficients"], g["%s_sigma2" % tag])))
    k = 0
    while k < min(len(trace), nref) and rel_err(trace[k][0], g["%s_x" % tag][k]) < 1e-6:
        k += 1
    assert k >= min(nref, 12), k
    for i in range(k):
        x, nll, grad = trace[i]
        assert abs(nll - g["%s_nll" % tag][i]) < 1e-9 * abs(g["%s_nll" % tag][i]), i
        assert rel_err(grad, g["%s_grad" % tag][i]) < 1e-5, i
