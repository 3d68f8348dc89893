"""Exact-trace REML on a deterministic engine: `SparseCholesky(exact_trace=True, deterministic=True)` takes the selected
inverse's order-fixed kernels, so an evaluation repeats bit for bit between two fresh processes and a whole fit -- L-BFGS-B
or AI-REML -- repeats bit for bit whatever the np.random seed; the fit agrees with the default handle's to rounding."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

M = importlib.import_module("scilmm_amd.SparseCholesky")  # (the package attribute of that name is the class)
_PROBLEM = {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_problem():
    yield
    _PROBLEM.clear()


def _problem():
    """The three-component problem of test_gpu_reml.test_exact_trace_option_gives_the_analytic_gradient."""
    if not _PROBLEM:
        from scilmm_amd.harness import pedigree as H
        mats, C, y = H.make_problem(2500, 0.01, seed=4, with_dominance=True)
        _PROBLEM.update(mats=mats, C=C, y=y)
    return _PROBLEM["mats"], _PROBLEM["C"], _PROBLEM["y"]


def test_same_bits_in_two_fresh_processes():
    script = os.path.join(os.path.dirname(__file__), "deterministic_exact_trace_script.py")
    outs = []
    for _ in range(2):
        p = subprocess.run([sys.executable, script], timeout=600, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0, p.stderr[-2000:]  # (stop at the first failure: nothing more is started)
        outs.append(p.stdout)
    print(outs[0])
    assert outs[0].count("nll=") == 2 and outs[0].count("atomics=0") == 2
    assert outs[0] == outs[1]


@pytest.mark.parametrize("aireml", [False, True])
def test_fit_repeats_bit_for_bit_and_agrees_with_the_default_handle(aireml):
    """Two deterministic fits under different np.random seeds: identical coefficients (the exact trace draws nothing, the
    engine's sums have a fixed order).  Against the default handle, whose inverse and sweeps sum in arrival order: 1e-8, the
    bound test_gpu_reml.py holds between two default fits that differ only in rounding."""
    mats, C, y = _problem()
    res = []
    for seed in (0, 123):
        np.random.seed(seed)
        chol = M.SparseCholesky(exact_trace=True, deterministic=True)
        res.append(np.array(M.REML(chol, mats, C, y, verbose=False, aireml=aireml)["covariance coefficients"]))
        assert chol._last_sym.deterministic and chol._last_sym.timing()["n_float_atomic_launches"] == 0
    np.random.seed(0)
    dflt = np.array(M.REML(M.SparseCholesky(exact_trace=True), mats, C, y, verbose=False, aireml=aireml)["covariance coefficients"])
    print("aireml=%s: deterministic %s, default %s, rel_err %.3e (limit 1e-8)" % (aireml, res[0], dflt, rel_err(res[0], dflt)))
    assert np.array_equal(res[0], res[1]), (res[0], res[1])
    assert rel_err(res[0], dflt) < 1e-8
