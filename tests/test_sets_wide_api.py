"""Variant sets wider than one device block, without a device: ``check_sets`` with ``max_markers``, the order of the work
(``plan_sets``), the argument checks of ``scilmm_scan_block_keep_dev``, and ``assemble_wide`` fed by a dense CPU whitening in
the place of the device -- ``cholesky(V)`` and ``solve_triangular``, the forward solution split into sub-blocks, the cross
blocks as ``X_b' X_a`` laid out as ``scan_panel_dev`` returns them against the padded store -- against the un-whitened oracle of
``tests/test_gpu_sets.py``.

Tolerance: the suite's 1e-9 for s, K, the eigenvalues and the derived statistics (``test_gpu_sets._compare``).  As measured on
the CPU for these inputs on ``spd203`` and ``spd300``: the worst relative error of s, K and lambda is 2e-15, ``n_used`` falls
short of k by 0 to 4 dropped markers, ``skat_p`` lies between 5e-3 and 0.999 and within 2e-13 relative of the oracle's.  At
n = 203, k = 257 the kernel is rank-deficient -- 202 eigenvalues kept at c = 1 and 199 at c = 4 -- and the cut is clean: the
smallest kept eigenvalue is 2e-3 of the largest, the largest dropped one 2e-16 of it."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as la
import scipy.stats as stats

from scilmm_amd import _lib
from tests.helpers import rel_err
from tests.test_gpu_sets import S2, _centred, _compare, _oracle, _problem

M = 304
WIDE = {16: (17, 32, 33, 50), 128: (129, 257)}


def wide_sets(block):
    """``permutation(304)[:k]`` drawn in turn from one generator per block: k = 17, 32, 33, 50 at block 16 -- one marker more than a
    block, two whole sub-blocks, one more than that, a ragged fourth -- and k = 129, 257 at block 128."""
    rng = np.random.default_rng(9)
    return [rng.permutation(M)[:k] for k in WIDE[block]]


def test_check_sets_with_max_markers():
    from scilmm_amd.sets import check_sets
    out = check_sets([np.arange(300), [3]], 400, 128, 300)
    assert [s.size for s in out] == [300, 1] and all(s.dtype == np.int64 for s in out)
    with pytest.raises(ValueError, match="set 1 has 301 markers, more than max_markers = 300"):
        check_sets([[3], np.arange(301)], 400, 128, 300)
    assert check_sets([], 10, 8, 64) == []
    # the bounds of max_markers itself: block .. 4096, an integer
    assert len(check_sets([np.arange(8)], 10, 8, 8)) == 1 and len(check_sets([np.arange(4096)], 5000, 128, 4096)) == 1
    for bad in (7, 4097, 0, -1, 64.0, "64", True):
        with pytest.raises(ValueError, match="max_markers"):
            check_sets([[0]], 10, 8, bad)
    # the old three-argument calls and their messages
    with pytest.raises(ValueError, match="more than one device block of 8: sets wider than a block are not supported"):
        check_sets([[0, 1], list(range(9))], 10, 8)
    with pytest.raises(ValueError, match="more than one device block of 8"):
        check_sets([list(range(9))], 10, 8, None)
    with pytest.raises(ValueError, match="twice"):
        check_sets([[1, 2, 1]], 10, 8, 64)
    with pytest.raises(ValueError, match="outside"):
        check_sets([[10]], 10, 8, 64)
    # the panel's column limit: block = 100 is kept 112 columns wide, 36 kept sub-blocks are 4032 columns, 37 are 4144
    assert len(check_sets([np.arange(3700)], 5000, 100, 4096)) == 1
    with pytest.raises(ValueError, match="4144 columns.*4096 columns of a panel call"):
        check_sets([[0], np.arange(3701)], 5000, 100, 4096)
    assert len(check_sets([np.arange(4096)], 5000, 128, 4096)) == 1          # 31 kept sub-blocks of 128: 3968 columns


def test_plan_sets_keeps_the_narrow_blocks_and_the_list_order():
    from scilmm_amd.sets import pack_sets, plan_sets
    sizes = [3, 200, 4, 5, 130, 2, 8]
    assert plan_sets(sizes, 8) == [[0, 2], [1], [3, 5], [4], [6]]
    narrow = [i for i, k in enumerate(sizes) if k <= 8]
    assert [[narrow[j] for j in b] for b in pack_sets([sizes[i] for i in narrow], 8)] == [[0, 2], [3, 5], [6]]
    assert plan_sets([1, 2, 16, 17], 17) == pack_sets([1, 2, 16, 17], 17)     # nothing wide: the packing as it was
    assert plan_sets([], 8) == [] and plan_sets([9], 8) == [[0]]


def test_exports():
    from scilmm_amd import sets
    from scilmm_amd.factor import Factor
    assert callable(Factor.scan_block_keep_dev) and callable(sets.assemble_wide)
    assert "scilmm_scan_block_keep_dev" in _lib.SYMBOLS and hasattr(_lib.lib(), "scilmm_scan_block_keep_dev")


def test_keep_entry_point_rejects_bad_arguments_before_any_device_state():
    """Dummy non-null pointers, a null handle and a factor whose symbolic handle is null: the code comes from the argument
    checks alone."""
    f = _lib.lib().scilmm_scan_block_keep_dev
    vp = C.c_void_p
    one, a16 = vp(8), vp(32)                        # non-null dummies: any address, and a 16-byte aligned one
    hollow = C.create_string_buffer(256)            # a scilmm_factor with sym == NULL
    fac = C.cast(hollow, vp)
    table = [
        (None, 1, a16, 16, 0), (fac, 1, a16, 16, 0),                            # no handle
        (one, 1, None, 16, 0),                                                  # null d_dst
        (one, 0, a16, 128, 0), (one, 129, a16, 256, 0), (one, -1, a16, 128, 0),  # r outside 1..128
        (one, 1, a16, 64, -16), (one, 1, a16, 64, 8), (one, 1, a16, 64, 17),    # col0 < 0, col0 % 16 != 0
        (one, 1, a16, 24, 0), (one, 1, a16, 1, 0), (one, 1, a16, 0, 0), (one, 1, a16, -16, 0),   # ld_dst % 16 != 0, ld_dst < rp
        (one, 1, a16, 16, 16), (one, 17, a16, 16, 0), (one, 19, a16, 32, 16), (one, 128, a16, 4096, 3984),   # ld_dst < col0 + rp
        (one, 1, one, 16, 0), (one, 19, vp(40), 64, 16),                        # d_dst not 16-byte aligned
    ]
    got = [f(*args) for args in table]
    assert got == [_lib.ERR_ARG] * len(table)


def test_refusals_run_on_an_object_that_was_never_constructed():
    """Every check of a wide call comes before any launch: none of them may touch the device side, which is not there."""
    from scilmm_amd.glmm import BinarySetTest
    from scilmm_amd.sets import VariantSetTest
    n, m = 21, 40
    G = np.random.default_rng(0).integers(0, 3, (m, n)).astype(np.int8)
    t = object.__new__(VariantSetTest)
    t.n, t.block = n, 4
    wide = [[0, 1], list(range(9))]
    with pytest.raises(ValueError, match="more than one device block of 4"):
        t(G, wide)
    with pytest.raises(ValueError, match="set 1 has 9 markers, more than max_markers = 8"):
        t(G, wide, max_markers=8)
    with pytest.raises(ValueError, match="device finish holds one block"):
        t(G, wide, max_markers=16, finish="device")
    for bad in (3, 4097, 8.0):
        with pytest.raises(ValueError, match="max_markers"):
            t(G, [[0, 1]], max_markers=bad)
    with pytest.raises(ValueError, match="twice"):
        t.test_dosages(np.zeros((m, n), dtype=np.float32), [[2, 2]], max_markers=16)
    b = object.__new__(BinarySetTest)
    b.n, b.block = n, 4
    for sets in (wide, [[0, 1]]):                       # any value but None, whatever the sets
        with pytest.raises(ValueError, match="max_markers is not supported for binary traits"):
            b(G, sets, max_markers=16)


def test_assemble_wide_places_the_blocks_and_checks_its_shapes():
    from scilmm_amd.sets import assemble_wide
    S = [np.zeros((6, 4)), np.zeros((6, 4)), np.zeros((6, 3))]
    G = [np.zeros((4, 4)), np.zeros((4, 4)), np.zeros((3, 3))]
    X = [np.zeros((4, 16)), np.zeros((3, 32))]
    s, g = assemble_wide(S, G, X, 16)
    assert s.shape == (6, 11) and g.shape == (11, 11)
    # block 4 kept 16 columns wide: the padding columns 4 .. 15 of every kept sub-block reach nothing
    rng = np.random.default_rng(1)
    Z = rng.standard_normal((30, 11))
    full = Z.T @ Z
    pad = lambda a: np.hstack([np.hstack([a[:, 4 * j:4 * j + 4], np.full((a.shape[0], 12), np.nan)]) for j in range(a.shape[1] // 4)])
    G = [full[:4, :4], full[4:8, 4:8], full[8:, 8:]]
    X = [pad(full[4:8, :4]), pad(full[8:, :8])]
    s, g = assemble_wide([np.arange(24.0).reshape(6, 4), np.zeros((6, 4)), np.ones((6, 3))], G, X, 16)
    assert np.array_equal(g, full) and np.array_equal(s[:, :4], np.arange(24.0).reshape(6, 4)) and np.all(s[:, 8:] == 1.0)
    for bad in ((S, G, X[:1], 16), (S, G[:2], X, 16), (S[::-1], G[::-1], X, 16), (S, G, X, 2)):
        with pytest.raises(ValueError):
            assemble_wide(*bad)


def cpu_blocks(p, c, rows, block):
    """What the device returns for one wide set, from a dense whitening: per sub-block the (c + 5) x r_b statistics and the Gram
    block, per sub-block behind the first its cross block against the kept ones, each padded to bp columns."""
    n = p["n"]
    if "Lc" not in p:
        p["Lc"] = la.cholesky((S2[0] * p["A"] + S2[1] * p["I"]).toarray(), lower=True)
    Q = la.solve_triangular(p["Lc"], np.hstack([p["C"][:, :c], p["y"][:, None]]), lower=True)
    n_obs, mean, Gt = _centred(p["G"][rows])
    X = la.solve_triangular(p["Lc"], np.ascontiguousarray(Gt.T), lower=True)               # n x k
    S = np.vstack([n_obs, mean, (Gt ** 2).sum(axis=1), (X * X).sum(axis=0), Q.T @ X])
    bp = (block + 15) // 16 * 16
    B = -(-rows.size // block)
    store = np.full((n, max(B - 1, 1) * bp), np.nan)
    Ss, Gs, Xs = [], [], []
    for b in range(B):
        Xb = X[:, b * block:(b + 1) * block]
        Ss.append(S[:, b * block:(b + 1) * block])
        Gs.append(Xb.T @ Xb)
        if b:
            Xs.append(Xb.T @ store[:, :b * bp])
        if b < B - 1:
            store[:, b * bp:(b + 1) * bp] = 0.0
            store[:, b * bp:b * bp + block] = Xb
    return Ss, Gs, Xs, bp, Q


@pytest.mark.parametrize("block", [16, 128])
@pytest.mark.parametrize("c", [1, 4])
@pytest.mark.parametrize("name", ["spd203", "spd300", "pedigree"])
def test_assemble_wide_against_the_unwhitened_oracle(name, c, block):
    from scilmm_amd import sets as mod
    p = _problem(name)
    n, sets = p["n"], wide_sets(block)
    ref = _oracle(p, c, sets)
    t = object.__new__(mod.VariantSetTest)            # the host algebra alone: R, u and the F distribution are all it reads
    out = {k: np.full(len(sets), np.nan) for k in mod.KEYS}
    out["n_used"] = np.zeros(len(sets), dtype=np.int64)
    out["kernel"] = []
    for i, rows in enumerate(sets):
        Ss, Gs, Xs, bp, Q = cpu_blocks(p, c, rows, block)
        G0 = Q.T @ Q
        t.R = la.cholesky(G0[:c, :c], lower=False)
        t.u = la.solve_triangular(t.R, G0[:c, c], trans='T', lower=False)
        t._f = stats.f(1, n - 1)
        S, G = mod.assemble_wide(Ss, Gs, Xs, bp)
        assert S.shape == (c + 5, rows.size) and G.shape == (rows.size, rows.size) and np.array_equal(G, G.T)
        out["kernel"].append(t._one_set(out, i, S, G, "beta", mod.mixture_sf_saddlepoint))
        s, K, w = out["kernel"][i]
        s0, K0, _ = ref["kernel"][i]
        lam = la.eigvalsh(w[:, None] * K * w[None, :])
        kept = lam > 1e-10 * lam.max()
        print(name, c, rows.size, "n_used", out["n_used"][i], "s", rel_err(s, s0), "K", rel_err(K, K0), "lam", rel_err(lam, ref["lam"][i]),
              "kept", int(kept.sum()), "smallest kept", lam[kept].min() / lam.max(),
              "largest dropped", (np.abs(lam[~kept]).max() / lam.max()) if (~kept).any() else 0.0, "skat_p", out["skat_p"][i],
              "vs oracle", abs(out["skat_p"][i] - ref["skat_p"][i]) / ref["skat_p"][i])
    _compare(out, ref, n)
