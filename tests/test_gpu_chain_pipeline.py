"""k_chain's software-pipelined pair loop (the default) in its three window widths: against the oracle factor, and bit for
bit against the loop it replaces (SCILMM_CHAIN_PIPE=0).  On a short chain every workgroup is resident and consumes one pair
per hop, so SCILMM_CHAIN_STAGGER=k makes each workgroup wait for its k-th-from-last pair first: the later blocks then run a
long final prefix through the pipelined branch, take the waiting branch for the last k pairs, and cross both transitions."""
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests.test_gpu_halfsolve import TOL, _Oracle, _check_halves, _pedigree, _pedigree_oracle

pytestmark = pytest.mark.gpu

# (112: a block of at most 64 columns, r = 1 or 5 here, takes the 64-column kernel -- one 112-column window has nothing to save
#  there; the pipelined loop exists in the 64-column form, so at 32 and 112 columns the bit comparison holds trivially)
WIDTHS = {32: {"SCILMM_CHAIN_WIDE_T": "100000", "SCILMM_CHAIN_FULL_T": "100000"},
          64: {"SCILMM_CHAIN_WIDE_T": "1", "SCILMM_CHAIN_FULL_T": "100000"},
          112: {"SCILMM_CHAIN_WIDE_T": "1", "SCILMM_CHAIN_FULL_T": "1"}}

_DENSE = {}


def _dense():
    """Dense SPD, n = 1100, natural ordering: nine chain blocks, the last one 76 columns wide.  Built once."""
    if not _DENSE:
        n = 1100
        G = np.random.default_rng(0).standard_normal((n, n))
        _DENSE.update(A=sp.csr_matrix(G @ G.T + n * np.eye(n)), handles={}, oracle={})
    return _DENSE


def _dense_factor(deterministic):
    from scilmm_amd.factor import Symbolic
    d = _dense()
    if deterministic not in d["handles"]:
        sym = Symbolic([d["A"]], ordering="natural", deterministic=deterministic)
        d["handles"][deterministic] = (sym, sym.factorize([1.0]))
    return d["handles"][deterministic]


def _dense_oracle(perm):
    d = _dense()
    key = perm.tobytes()
    if key not in d["oracle"]:
        d["oracle"][key] = _Oracle(d["A"], perm, 130, 1100)
    return d["oracle"][key]


def _pedigree_factor(deterministic):
    from scilmm_amd.factor import Symbolic
    p = _pedigree()
    handles = p.setdefault("pipeline_handles", {})
    if deterministic not in handles:
        sym = Symbolic([p["A"], p["I"]], deterministic=deterministic)
        handles[deterministic] = (sym, sym.factorize([0.35, 0.65]))
    return handles[deterministic]


def _set(monkeypatch, width, stagger, pipe=None):
    monkeypatch.setenv("SCILMM_TUNING", "1")     # (the chain switches are read on every call)
    for k, v in WIDTHS[width].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SCILMM_CHAIN_STAGGER", str(stagger))
    if pipe is None:
        monkeypatch.delenv("SCILMM_CHAIN_PIPE", raising=False)
    else:
        monkeypatch.setenv("SCILMM_CHAIN_PIPE", pipe)


def test_both_problems_have_the_chains_these_tests_are_about(monkeypatch, capfd):
    """The plan's own report (SCILMM_VERBOSE): nine chain blocks for the dense problem; a chain with non-contiguous pairs
    (column maps) for the pedigree.  Without them every test below would pass on the level sweep alone."""
    from scilmm_amd.factor import Symbolic
    monkeypatch.setenv("SCILMM_VERBOSE", "1")
    capfd.readouterr()
    Symbolic([_dense()["A"]], ordering="natural").factorize([1.0])
    m = re.search(r"chain sweep: (\d+) fronts", capfd.readouterr().err)
    assert m and int(m.group(1)) == 9, m
    p = _pedigree()
    Symbolic([p["A"], p["I"]]).factorize([0.35, 0.65])
    m = re.search(r"chain sweep: (\d+) fronts .* inner pairs \((\d+) column maps", capfd.readouterr().err)
    assert m and int(m.group(1)) >= 4 and int(m.group(2)) > 0, m


@pytest.mark.parametrize("stagger", [0, 1, 3])
@pytest.mark.parametrize("width", [32, 64, 112])
def test_dense_chain_with_a_ragged_end(monkeypatch, width, stagger):
    _, f = _dense_factor(False)
    _set(monkeypatch, width, stagger)
    _check_halves(f, _dense_oracle(f.P()), (1, 5, 103, 130))   # 130 crosses RPMAX


@pytest.mark.parametrize("stagger", [0, 3])
@pytest.mark.parametrize("width", [32, 64, 112])
def test_pedigree_chain_with_non_contiguous_pairs(monkeypatch, width, stagger):
    _, f = _pedigree_factor(False)
    _set(monkeypatch, width, stagger)
    _check_halves(f, _pedigree_oracle(f.P()), (5, 103))


@pytest.mark.parametrize("width", [32, 64, 112])
@pytest.mark.parametrize("problem", ["dense", "pedigree"])
def test_pipelined_loop_repeats_the_bits_of_the_loop_it_replaces(monkeypatch, problem, width):
    """Same sums in the same order: on a deterministic handle forward, backward and full solve are bit-identical."""
    if problem == "dense":
        sym, f = _dense_factor(True)
        B = _dense_oracle(f.P()).B[:, :103]
    else:
        sym, f = _pedigree_factor(True)
        B = _pedigree_oracle(f.P()).B

    def run():
        return [(r, f.solve_L(B[:, :r]), f.solve_Lt(B[:, :r]), f(B[:, :r])) for r in (5, 103)]

    _set(monkeypatch, width, 3, pipe="0")
    ref = run()
    _set(monkeypatch, width, 3)
    for (r, fw0, bw0, full0), (_, fw1, bw1, full1) in zip(ref, run()):
        assert np.array_equal(fw0, fw1), ("forward", problem, width, r)
        assert np.array_equal(bw0, bw1), ("backward", problem, width, r)
        assert np.array_equal(full0, full1), ("full solve", problem, width, r)
    assert sym.timing()["n_float_atomic_launches"] == 0
