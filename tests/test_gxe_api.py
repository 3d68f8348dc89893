"""The marker x environment scan's surface without a device: the host algebra (``gxe.interaction_stats``) fed with a dense CPU
whitening packed in the layout of ``scilmm_scan_block_gxe_dev`` against the un-whitened GLS oracle (tests/gxe_oracle.py), the
checks of ``env``, the exports and the argument checks of the three C entry points.

Tolerance 1e-9 relative (tests.helpers.rel_err: max-norm over the markers), the suite's for derived statistics; the two
formulas agree to 3e-15 in that norm on these inputs (random_spd(300, 0.05, 3), 40 markers, 2 % missing, m = 1, 2, 3).  The
LEVEL marker's unit-diagonal M has a reciprocal condition number of 4e-16, every other marker's is at least 0.11: the 1e-10
threshold separates them."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as la
import scipy.sparse as sp

from scilmm_amd import _lib
from tests import gxe_oracle as O
from tests.helpers import random_spd

S2 = [0.4, 0.6]
M = 40


@pytest.fixture(scope="module")
def problem():
    A = random_spd(300, 0.05, 3)
    n = A.shape[0]
    V = (S2[0] * A + S2[1] * sp.identity(n)).toarray()
    rng = np.random.default_rng(11)
    E = O.environment(n, 3, 5)
    extra = rng.standard_normal((n, 2))
    y = 0.5 + extra @ np.array([-0.2, 0.1]) + E @ np.array([0.3, -0.1, 0.2]) + rng.standard_normal(n)
    return dict(n=n, L=np.linalg.cholesky(V), Vi=np.linalg.inv(V), E=E, extra=extra, y=y, G=O.markers(n, M, 7, E[:, 0]))


def _whitened_stats(p, Cv, E):
    """(S, R, u): the statistics of the gxe entry points for every marker of the problem from a dense whitening
    w(b) = L^-1 b, and the scan's R and u."""
    from scilmm_amd.gxe import stat_rows
    w = lambda B: la.solve_triangular(p["L"], B, lower=True)
    c, d = Cv.shape[1], 1 + E.shape[1]
    q = c + 1
    Q = w(np.hstack([Cv, p["y"][:, None]]))
    Gm = Q.T @ Q
    R = la.cholesky(Gm[:c, :c], lower=False)
    u = la.solve_triangular(R, Gm[:c, c], trans='T', lower=False)
    n_obs, mean, Gt = O.centred(p["G"])
    S = np.zeros((stat_rows(q, d), M))
    S[0], S[1], S[2] = n_obs, np.where(n_obs > 0, mean, 0.0), (Gt * Gt).sum(axis=1)
    X = [w(Gt.T)] + [w((Gt * E[:, a]).T) for a in range(d - 1)]          # d blocks of n x M
    k = 3 + (q + 1) * d
    for a in range(d):
        S[3 + a] = (X[a] * X[a]).sum(axis=0)
        for j in range(q):
            S[3 + (j + 1) * d + a] = Q[:, j] @ X[a]
        for b in range(a + 1, d):
            S[k] = (X[a] * X[b]).sum(axis=0)
            k += 1
    assert k == S.shape[0]
    return S, R, u


@pytest.mark.parametrize("extra", [False, True])
@pytest.mark.parametrize("m", [1, 2, 3])
def test_host_algebra_matches_unwhitened_gls(problem, m, extra):
    from scilmm_amd.gxe import interaction_stats
    p = problem
    n, E = p["n"], p["E"][:, :m]
    Cv = np.hstack([np.ones((n, 1))] + ([p["extra"]] if extra else []) + [E])
    S, R, u = _whitened_stats(p, Cv, E)
    out = interaction_stats(S, 1 + m, R, u, n)
    assert sorted(out) == sorted(O.KEYS + ("p_int", "p_joint", "n_obs", "mean"))
    O.compare(out, O.oracle(p["Vi"], Cv, p["y"], E, p["G"]), n)


def test_host_algebra_of_no_markers_and_of_a_wrong_layout(problem):
    from scilmm_amd.gxe import interaction_stats, stat_rows
    R, u = np.eye(2), np.zeros(2)
    out = interaction_stats(np.empty((stat_rows(3, 3), 0)), 3, R, u, 300)
    assert out["beta"].shape == (0, 3) and out["cov"].shape == (0, 3, 3) and out["p_int"].shape == (0,)
    with pytest.raises(ValueError):
        interaction_stats(np.zeros((stat_rows(3, 3) + 1, 4)), 3, R, u, 300)


def test_env_checks_need_no_device(problem):
    from scilmm_amd.gxe import check_env
    p = problem
    n, E = p["n"], p["E"]
    Cv = np.hstack([np.ones((n, 1)), E])
    assert check_env(E, n, Cv, 128).shape == (n, 3)
    assert check_env(E[:, 0], n, Cv, 128).shape == (n, 1)                # a vector is n x 1
    assert check_env(E[:, :1], n, Cv, 2).flags.c_contiguous              # block == d is enough
    with pytest.raises(ValueError):
        check_env(E[:-1], n, Cv, 128)                                     # wrong length
    with pytest.raises(ValueError):
        check_env(np.hstack([E, E[:, :1]]), n, Cv, 128)                   # m = 4
    with pytest.raises(ValueError):
        check_env(np.empty((n, 0)), n, Cv, 128)                           # m = 0
    bad = E.copy()
    bad[7, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        check_env(bad, n, Cv, 128)
    with pytest.raises(ValueError, match="block"):
        check_env(E, n, Cv, 3)                                            # block < d = 4
    outside = E.copy()
    outside[:, 2] = np.random.default_rng(1).standard_normal(n)
    with pytest.raises(ValueError, match="column 2"):
        check_env(outside, n, Cv, 128)                                    # its main effect is not in the null model
    assert check_env(outside, n, Cv, 128, require_main_effects=False).shape == (n, 3)
    with pytest.raises(ValueError, match="column 0"):
        check_env(E, n, Cv[:, :1], 128)                                   # intercept only


def test_exports_and_no_cpu_form():
    import scilmm_amd
    from scilmm_amd import AssociationScan, ScilmmError, gxe
    from scilmm_amd.factor import Factor
    assert scilmm_amd.InteractionScan is gxe.InteractionScan and callable(AssociationScan.interaction)
    L = _lib.lib()
    for name in ("scilmm_scan_block_gxe_dev", "scilmm_scan_block_bed_gxe_dev", "scilmm_scan_block_dosage_gxe_dev", "scilmm_gxe_timing"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    for name in ("scan_block_gxe_dev", "scan_block_bed_gxe_dev", "scan_block_dosage_gxe_dev"):
        assert callable(getattr(Factor, name)), name
    assert gxe.stat_rows(5, 1) == 5 + 4                                   # d = 1 would be the plain scan's rows
    with pytest.raises(ScilmmError, match="no CPU form"):
        gxe.InteractionScan(object(), np.zeros(4))                        # no device-engine handle behind it
    with pytest.raises(ScilmmError, match="no CPU form"):
        AssociationScan(lambda V: None, [sp.identity(4, format="csr")], [1.0], np.ones((4, 1)), np.zeros(4))


def test_entry_points_check_their_arguments_first():
    """Dummy non-null pointers: the argument checks come before any dereference."""
    L = _lib.lib()
    one = C.c_void_p(8)
    int8 = lambda r, E, m, fac=one, g=one, Q=one, q=2, S=one: L.scilmm_scan_block_gxe_dev(fac, g, 64, r, E, m, Q, q, S)
    bed = lambda r, E, m: L.scilmm_scan_block_bed_gxe_dev(one, one, 16, 64, None, 0, r, E, m, one, 2, one)
    dos = lambda r, E, m: L.scilmm_scan_block_dosage_gxe_dev(one, one, _lib.DOSAGE_U16, 64, 64, None, r, E, m, one, 2, one)
    for fn in (int8, bed, dos):
        for r, m in ((4, 0), (4, 4), (4, -1), (0, 1), (-1, 1), (65, 1), (43, 2), (33, 3)):
            assert fn(r, one, m) == _lib.ERR_ARG, (r, m)
        assert fn(4, None, 2) == _lib.ERR_ARG                            # a null d_E
    assert int8(4, one, 2, fac=None) == _lib.ERR_ARG                     # what the plain twin rejects
    assert int8(4, one, 2, g=None) == _lib.ERR_ARG
    assert int8(4, one, 2, Q=None) == _lib.ERR_ARG
    assert int8(4, one, 2, S=None) == _lib.ERR_ARG
    assert int8(4, one, 2, q=0) == _lib.ERR_ARG and int8(4, one, 2, q=33) == _lib.ERR_ARG
    assert L.scilmm_scan_block_bed_gxe_dev(one, one, 16, 64, None, 2, 4, one, 2, one, 2, one) == _lib.ERR_ARG   # unknown flag bit
    assert L.scilmm_scan_block_dosage_gxe_dev(one, one, 7, 64, 64, None, 4, one, 2, one, 2, one) == _lib.ERR_ARG  # unknown dtype
    assert L.scilmm_gxe_timing(None, (C.c_double * 2)()) == _lib.ERR_ARG
