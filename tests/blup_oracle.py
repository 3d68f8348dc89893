"""Dense NumPy oracles for the BLUP tests: two independent definitions of the predicted random effects and their
prediction error variances.  Neither shares anything with the whitened formula of scilmm_amd.blup.

``henderson``: Henderson's mixed-model equations for y = C beta + u + e, u ~ N(0, s2g A), e ~ N(0, s2e I):
    [[C'C, C'], [C, I + (s2e / s2g) A^-1]] [beta; u] = [C'y; y],   PEV = s2e * (inverse of the coefficient matrix)_uu.
``dense_pv``: the projection form, any number of components:
    P_V = V^-1 - V^-1 C (C' V^-1 C)^-1 C' V^-1,   u = G P_V y,   PEV = diag(G) - diag(G P_V G)   for the covariance G.
"""
import os

import numpy as np
import scipy.sparse as sp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_g1():
    """(A, C, y, REML estimate of sigma2) of the G1 pedigree, n = 1472."""
    g = np.load(os.path.join(GOLD, "G1_reml_2000.npz"))
    A = sp.csr_matrix((g["A_data"], g["A_indices"], g["A_indptr"]), shape=tuple(g["A_shape"]))
    A.sort_indices()
    return A, g["C"], g["y"], g["amd_sigma2"]


def golden_dominance(shape):
    g2 = np.load(os.path.join(GOLD, "G2_lmm_dominance.npz"))
    D = sp.csr_matrix((g2["D_data"], g2["D_indices"], g2["D_indptr"]), shape=shape)
    D.sort_indices()
    return D


def _dense(M):
    return M.toarray() if sp.issparse(M) else np.asarray(M, dtype=np.float64)


def henderson(A, C, y, s2g, s2e):
    """(beta, u, pev) from the mixed-model equations; A must be nonsingular."""
    A, C = _dense(A), np.asarray(C, dtype=np.float64)
    n, c = C.shape
    M = np.empty((c + n, c + n))
    M[:c, :c] = C.T @ C
    M[:c, c:] = C.T
    M[c:, :c] = C
    M[c:, c:] = np.eye(n) + (s2e / s2g) * np.linalg.inv(A)
    Mi = np.linalg.inv(M)
    sol = Mi @ np.concatenate([C.T @ y, y])
    return sol[:c], sol[c:], s2e * np.diag(Mi)[c:].copy()


class DensePV(object):
    """P_V of V = sum_k sigma2[k] mats[k], built once; ``columns`` / ``rows`` evaluate the projection form."""

    def __init__(self, mats, sigma2, C, y):
        self.mats = [_dense(M) for M in mats]
        self.s2 = np.asarray(sigma2, dtype=np.float64)
        V = sum(s * M for s, M in zip(self.s2, self.mats))
        Vi = np.linalg.inv(V)
        ViC = Vi @ C
        CtViC = C.T @ ViC
        self.beta = np.linalg.solve(CtViC, ViC.T @ y)
        self.P = Vi - ViC @ np.linalg.solve(CtViC, ViC.T)
        self.Py = self.P @ y

    def covariance(self, k):
        if k == "total":
            return sum(s * M for s, M in zip(self.s2[:-1], self.mats[:-1]))
        return self.s2[k] * self.mats[k]

    def columns(self, k):
        """(u, pev) of every individual for component k (an index, or "total")."""
        G = self.covariance(k)
        return G @ self.Py, np.diag(G) - np.einsum("ij,ij->j", G, self.P @ G)

    def rows(self, rows, self_rel, scale):
        """(u, pev) of outside individuals with covariance rows ``scale * rows`` to the cohort and variance
        ``scale * self_rel``."""
        g = scale * _dense(rows)
        return g @ self.Py, scale * np.asarray(self_rel) - np.einsum("ij,ij->i", g, g @ self.P)
