"""Variant sets wider than one device block (``max_markers``) against the un-whitened oracle of ``tests/test_gpu_sets.py``, and
``scilmm_scan_block_keep_dev`` at the C level.

Tolerances are ``test_gpu_sets._compare``'s: 1e-9 relative for s, K, w, the eigenvalues and the derived statistics, the
p-values bit for bit the module's own functions of the returned statistics and within 1e-6 of the oracle's, K exactly
symmetric.  The sets are those of ``tests/test_sets_wide_api.py``, where the host half is held to the same oracle on the CPU
(2e-15 there).  At the C level: the kept columns within 1e-9 of ``Factor.solve_L``, the padding exact zeros, every other
column of the store untouched; the panel of a block against its own kept copy within 1e-12 of its Gram matrix (another
summation order: agreement to rounding, as between the Gram diagonal and the gg row)."""
import ctypes as C

import numpy as np
import pytest

from tests import test_bed_api as T
from tests.helpers import rel_err
from tests.test_gpu_dosage import _codes
from tests.test_gpu_sets import ALLMISS, KEYS, MONO, _centred, _compare, _oracle, _problem, _sets, _tester
from tests.test_sets_wide_api import wide_sets

pytestmark = pytest.mark.gpu

CASES = [(name, c, block, None) for name in ("spd203", "spd300", "pedigree") for c in (1, 4) for block in (16, 128)]
CASES.append(("spd203", 4, 112, 225))            # two sub-blocks of 112 and a ragged third of one marker


def _same(a, b, keys=KEYS):
    for k in keys:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True), k
    for (s, K, w), (s0, K0, w0) in zip(a["kernel"], b["kernel"]):
        assert np.array_equal(s, s0) and np.array_equal(K, K0) and np.array_equal(w, w0)


@pytest.mark.parametrize("name,c,block,k", CASES)
def test_wide_sets_match_the_unwhitened_formula(name, c, block, k):
    p = _problem(name)
    sets = wide_sets(block) if k is None else [np.random.default_rng(9).permutation(304)[:k]]
    tester = _tester(p, c, block)
    with pytest.raises(ValueError, match="more than one device block of %d" % block):
        tester(p["G"], sets)
    out = tester(p["G"], sets, max_markers=max(s.size for s in sets), return_kernel=True)
    assert sorted(out) == sorted(KEYS + ("kernel",)) and all(out[key].shape == (len(sets),) for key in KEYS)
    _compare(out, _oracle(p, c, sets), p["n"])


def test_set_layout_dropped_markers_across_sub_blocks_and_list_order():
    """Two wide sets around a narrow one.  The first holds the monomorphic marker in its first sub-block and the all-missing one
    in its second, so the markers that are left span the sub-blocks; the second shares five markers with it and ends in a
    ragged third sub-block; a second narrow set packs into the block of the first."""
    p = _problem("spd300")
    a = np.array([MONO] + list(range(10, 30)) + [ALLMISS] + list(range(30, 40)))
    sets = [a, np.array([5, 40, 41, 42]), np.arange(35, 72), np.array([7, 8])]
    assert [s.size for s in sets] == [32, 4, 37, 2] and list(a).index(ALLMISS) // 16 == 1
    tester = _tester(p, 4, 16, deterministic=True)
    out = tester(p["G"], sets, max_markers=48, return_kernel=True)
    _compare(out, _oracle(p, 4, sets), p["n"])
    left = []
    for rows in sets:                                                       # what is left of a set, from the markers alone
        n_obs, _, Gt = _centred(p["G"][rows])
        left.append(int(((n_obs > 0) & Gt.any(axis=1)).sum()))
    assert out["n_used"].tolist() == left and left[0] <= 30 and left[1] == 4
    alone = tester(p["G"], [sets[1], sets[3]], return_kernel=True)         # the narrow sets: the blocks of a call on them alone
    for k in KEYS:
        assert np.array_equal(out[k][[1, 3]], alone[k]), k


def test_skato_on_wide_sets_is_skato_pvalue_of_the_returned_kernel():
    from scilmm_amd.sets import RHO_DEFAULT, SKATO_KEYS, skato_pvalue
    p = _problem("spd203")
    sets = wide_sets(16)
    out = _tester(p, 4, 16)(p["G"], sets, max_markers=64, return_kernel=True, skato=True)
    assert sorted(out) == sorted(KEYS + SKATO_KEYS + ("kernel",)) and out["skato_p_rho"].shape == (len(sets), len(RHO_DEFAULT))
    for i, (s, K, w) in enumerate(out["kernel"]):
        pv, pmin, rho, p_rho = skato_pvalue(w * s, w[:, None] * K * w[None, :], RHO_DEFAULT, "saddlepoint")
        assert 0.0 < pv <= 1.0
        assert out["skato_p"][i] == pv and out["skato_pmin"][i] == pmin and out["skato_rho"][i] == rho, i
        assert np.array_equal(out["skato_p_rho"][i], p_rho), i


def test_narrow_sets_keep_their_bits_under_max_markers():
    p = _problem("spd203")
    tester, sets = _tester(p, 4, 128, deterministic=True), _sets()
    a = tester(p["G"], sets, return_kernel=True)
    b = tester(p["G"], sets, return_kernel=True, max_markers=256)
    assert sorted(a) == sorted(b)
    _same(a, b)


def test_wide_calls_repeat_their_bits_in_every_input_form(tmp_path):
    p = _problem("spd203")
    n = p["n"]
    tester = _tester(p, 4, 16, deterministic=True)
    sets = wide_sets(16) + [np.array([5, 40, 41, 42])]
    a = tester(p["G"], sets, max_markers=64, return_kernel=True)
    b = tester(p["G"], sets, max_markers=64, return_kernel=True)
    _same(a, b)
    _compare(a, _oracle(p, 4, sets), n)
    bed = tester.test_bed(T.write_fileset(tmp_path / "wide", T.pack(p["G"]), n), sets, max_markers=64, return_kernel=True)
    _same(bed, a)
    dos = tester.test_dosages(_codes(p["G"]), sets, max_markers=64, return_kernel=True)
    _same(dos, a)
    assert tester.sym.timing()["n_float_atomic_launches"] == 0


CANARY = -7.25


def _gram_block(tester, G, torch):
    """One int8 Gram block of the rows of G, waited for: (device rows kept alive, r x r Gram matrix)."""
    r, n, q = G.shape[0], G.shape[1], tester.q
    ld = (n + 15) // 16 * 16
    dG = torch.zeros((r, ld), dtype=torch.int8, device="cuda")
    dG[:, :n].copy_(torch.from_numpy(G))
    dS = torch.zeros(((q + 4) * r,), dtype=torch.float64, device="cuda")
    dK = torch.zeros((r * r,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    vp = C.c_void_p
    tester.factor.scan_block_gram_dev(vp(dG.data_ptr()), ld, r, vp(tester.dQ.data_ptr()), q, vp(dS.data_ptr()), vp(dK.data_ptr()))
    tester.sym.sync()
    return dK.cpu().numpy().reshape(r, r)


def test_keep_at_the_c_level_and_the_panel_against_the_kept_copy():
    import torch
    p = _problem("spd203")
    n = p["n"]
    tester = _tester(p, 4, 128, deterministic=True)
    fac, vp = tester.factor, C.c_void_p
    G19 = np.ascontiguousarray(np.vstack([p["G"][:4], p["G"][40:55]]))
    _, _, Gt = _centred(G19)
    X = fac.solve_L(fac.apply_P(np.ascontiguousarray(Gt.T)))               # n x 19, permuted rows
    K = _gram_block(tester, G19, torch)
    store = torch.full((n, 64), CANARY, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    fac.scan_block_keep_dev(19, vp(store.data_ptr()), 64, 16)
    tester.sym.sync()
    got = store.cpu().numpy()
    print("kept columns vs solve_L", rel_err(got[:, 16:35], X))
    assert rel_err(got[:, 16:35], X) < 1e-9
    assert np.all(got[:, 35:48] == 0.0)
    assert np.all(got[:, :16] == CANARY) and np.all(got[:, 48:] == CANARY)
    # the block is still there: its panel against its own kept copy is its Gram matrix, in another summation order
    dO = torch.full((19 * 32,), CANARY, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    fac.scan_panel_dev(19, vp(store.data_ptr() + 8 * 16), 64, 32, vp(dO.data_ptr()), 32)
    fac.scan_block_keep_dev(19, vp(store.data_ptr()), 64, 32)               # a further keep behind the panel, over the padding
    tester.sym.sync()
    O = dO.cpu().numpy().reshape(19, 32)
    print("panel against the kept copy vs the Gram block", rel_err(O[:, :19], K))
    assert rel_err(O[:, :19], K) < 1e-12
    assert np.all(O[:, 19:] == 0.0)
    again = store.cpu().numpy()
    assert np.array_equal(again[:, 32:51], got[:, 16:35]) and np.all(again[:, 51:] == 0.0)
    assert np.array_equal(again[:, :32], got[:, :32])


def test_keep_needs_the_block_and_its_r_and_leaves_the_handle_usable():
    import torch
    from scilmm_amd import ScilmmError
    p = _problem("spd203")
    n = p["n"]
    tester = _tester(p, 4, 128, deterministic=True)
    fac, vp = tester.factor, C.c_void_p
    G19 = np.ascontiguousarray(p["G"][40:59])
    K = _gram_block(tester, G19, torch)
    store = torch.full((n, 32), CANARY, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(ScilmmError, match="the block left behind has 19 columns"):
        fac.scan_block_keep_dev(18, vp(store.data_ptr()), 32, 0)
    fac.scan_block_keep_dev(19, vp(store.data_ptr()), 32, 0)               # the block is still there
    fac.solve_L(np.ones((n, 1)))                                            # ... and is forgotten here
    with pytest.raises(ScilmmError, match="no scan block"):
        fac.scan_block_keep_dev(19, vp(store.data_ptr()), 32, 0)
    assert np.array_equal(_gram_block(tester, G19, torch), K)               # the next block still runs
    fac.scan_block_keep_dev(19, vp(store.data_ptr()), 32, 0)
    tester.sym.sync()
    assert not np.any(store.cpu().numpy() == CANARY)


def test_refusals_before_any_launch():
    from scilmm_amd import LogisticMixedModel, SparseCholesky
    p = _problem("spd300")
    tester = _tester(p, 1, 16)
    wide = [np.arange(4, 37)]
    with pytest.raises(ValueError, match="holds one block"):
        tester(p["G"], wide, max_markers=64, finish="device")
    with pytest.raises(ValueError, match="set 0 has 33 markers, more than max_markers = 32"):
        tester(p["G"], wide, max_markers=32)
    for bad in (15, 4097, 32.0):
        with pytest.raises(ValueError, match="max_markers"):
            tester(p["G"], [np.arange(4, 8)], max_markers=bad)
    tester(p["G"], [np.arange(4, 8)], max_markers=64, finish="device")      # narrow sets alone: the device finish as it was
    yb = (p["y"] > np.median(p["y"])).astype(np.float64)
    binary = LogisticMixedModel(SparseCholesky(), [p["A"]], p["C"][:, :1], yb).null_at([0.3], [0.0], np.zeros(p["n"])).sets(block=16)
    for sets in (wide, [np.arange(4, 8)]):                                  # any value but None, whatever the sets
        with pytest.raises(ValueError, match="max_markers is not supported for binary traits"):
            binary(p["G"], sets, max_markers=64)
