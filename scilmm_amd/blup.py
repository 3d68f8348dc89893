"""BLUP breeding values with exact prediction error variances and reliabilities on the resident factor.

With the marker scan's ``w(b) = L^-1 P b``, ``Q = [w(C) | w(y)]``, ``R'R = w(C)'w(C)`` and ``u = R^-T w(C)'w(y)``
(``scilmm_amd.assoc``), a column ``g`` of a relationship matrix ``G`` gives::

    z = R^-T w(C)' w(g)      a = |w(g)|^2 - |z|^2 = g' P_V g      b = w(g)'w(y) - z'u = g' P_V y
    P_V = V^-1 - V^-1 C (C' V^-1 C)^-1 C' V^-1

so for ``G = A_k`` the predicted random effect of individual i is ``sigma2_k b``, its prediction error variance
``sigma2_k A_k,ii - sigma2_k^2 a`` and its reliability ``1 - PEV / (sigma2_k A_k,ii)``; ``G = sum_k sigma2_k A_k`` over the
genetic components gives the total genetic value, and a sparse row of relationships to the cohort the prediction of
somebody outside it.  An individual costs one column of a forward sweep; the n x r block is built on the device from the
resident values (``scilmm_rel_block_dev``) or from the caller's rows (``scilmm_rows_block_dev``), and ``q + 2`` numbers per
individual come back.  The reference stops at the variance components and the covariates' coefficients
(scilmm/Estimation/LMM.py:129-133).

    blup = BLUP(cholesky_func, mats, sigma2, covariates, y)
    blup.beta                         # GLS fixed effects
    blup.effects(0)                   # all n predicted values of component 0: one backward half-solve, one SpMM
    blup.reliability(0, individuals)  # dict of u, pev, reliability, self_rel
    blup.predict(rows, self_rel, 0)   # the same for relatives without a phenotype
    blup.reliability_all("total")     # everybody at once from ONE selected inverse, and with it
    blup.prediction_error_covariance()   # PEV / PEC of every pair of relatives, CSR on V's pattern
    blup.leave_one_out()              # leave-one-out residuals, variances, studentised residuals: no refit

There is no CPU form: without a GPU or the built library the constructor raises ``ScilmmError``.
"""
import ctypes as C

import numpy as np
import scipy.linalg as la
import scipy.sparse as sp

from .assoc import WhitenedModel


def check_individuals(individuals, n):
    """The requested individuals as the device path takes them: a 1-D int32 array of distinct indices into the matrices' rows.
    TypeError for a non-integer array, ValueError for another shape, an index outside 0 .. n-1 or a repeated one."""
    ids = np.asarray(individuals)
    if ids.dtype.kind not in "iu":
        raise TypeError("individuals must be integers (row indices of the matrices), got %s" % ids.dtype)
    if ids.ndim != 1:
        raise ValueError("individuals must be 1-D, got %d-D" % ids.ndim)
    if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= n):
        raise ValueError("individuals must lie in 0 .. %d" % (n - 1))
    if np.unique(ids).size != ids.size:
        raise ValueError("an individual is requested twice")
    return np.ascontiguousarray(ids, dtype=np.int32)


def check_rows(rows, self_rel, n):
    """``rows`` (m x n SciPy sparse, relationships of m outside individuals to the cohort) as canonical CSR -- float64, int32
    indices sorted and summed, int64 indptr -- and ``self_rel`` (their own diagonal entries) as a length-m float64 array.
    TypeError for a dense ``rows``, ValueError for a shape that does not fit.  The caller's matrix is not modified."""
    if not sp.issparse(rows):
        raise TypeError("rows must be a SciPy sparse matrix, got %s" % type(rows).__name__)
    if rows.ndim != 2 or rows.shape[1] != n:
        raise ValueError("rows have shape %s, the model has %d individuals" % (rows.shape, n))
    self_rel = np.asarray(self_rel, dtype=np.float64)
    if self_rel.shape != (rows.shape[0],):
        raise ValueError("self_rel must have one entry per row of rows")
    R = sp.csr_matrix(rows, dtype=np.float64, copy=True)
    R.sum_duplicates()
    R.sort_indices()
    return (R.indptr.astype(np.int64), R.indices.astype(np.int32), np.ascontiguousarray(R.data, dtype=np.float64)), self_rel


def check_all_component(k, K):
    """The component argument of ``BLUP.reliability_all``: ``"total"`` always, the index 0 when there is one relationship
    matrix (K == 2: component 0 IS the total genetic value).  ValueError otherwise -- for an index with K >= 3 naming
    ``reliability()``, whose column path is the exact one for a single component among several."""
    if isinstance(k, str):
        if k != "total":
            raise ValueError("k must be \"total\" (or 0 when there is one relationship matrix)")
        return k
    if not (isinstance(k, (int, np.integer)) and not isinstance(k, (bool, np.bool_)) and 0 <= k < K - 1):
        raise ValueError("k must be \"total\" (or 0 when there is one relationship matrix), got %r" % (k,))
    if K != 2:
        raise ValueError("reliability_all(%d) with %d relationship matrices: diag(A_k V^-1 A_k) couples pairs of relatives that "
                         "need not lie on the factor's pattern, so one component among several is not exact from the selected "
                         "inverse; use reliability(%d) (one sweep column per individual), or k=\"total\"" % (k, K - 1, k))
    return int(k)


class BLUP(WhitenedModel):
    """Predicted random effects, prediction error variances and reliabilities under V = sum_k sigma2[k] mats[k].

    Arguments and lifetime as for ``AssociationScan``: ``mats`` hold every matrix of V, the identity (last) included; the
    resident factor of ``(mats, sigma2)`` is obtained or re-used, and the object refuses to run once that factor holds other
    values.  ``block``: individuals per device block, 1..128.  A component is chosen by its index ``k``, or ``"total"`` for
    ``sum_k sigma2[k] mats[k]`` over every matrix but the last."""

    def __init__(self, cholesky_func, mats, sigma2, covariates, y, block=None):
        super(BLUP, self).__init__(cholesky_func, mats, sigma2, covariates, y, block)
        if self._s2.shape != (self.sym.K,):
            raise ValueError("sigma2 must have one entry per matrix")
        self.beta = la.solve_triangular(self.R, self.u, lower=False)      # GLS fixed effects (C' V^-1 C)^-1 C' V^-1 y
        self._dv = None                                                    # V^-1 (y - C beta), original order (effects)
        self._y = np.asarray(y, dtype=np.float64).ravel()
        self._inv = None                                                   # the whole-cohort pass (_inverse_pass)

    def _component(self, k):
        """(weights of the matrices in G, factor that takes g' P_V y to the predicted value)."""
        K = self.sym.K
        if isinstance(k, str):
            if k != "total":
                raise ValueError("k must be a matrix index or \"total\"")
            w = self._s2.copy()
            w[K - 1] = 0.0
            return w, 1.0
        if not (isinstance(k, (int, np.integer)) and 0 <= k < K):
            raise ValueError("k must be a matrix index in 0..%d or \"total\"" % (K - 1))
        w = np.zeros(K)
        w[k] = 1.0
        return w, float(self._s2[k])

    def _finish(self, S, scale, self_rel):
        """The (q + 2) x m statistics of the block entry points -> the result dict; ``scale * G`` is the covariance."""
        c = self.c
        z = la.solve_triangular(self.R, S[2:2 + c], trans='T', lower=False) if S.shape[1] else np.empty((c, 0))
        a = S[1] - np.sum(z * z, axis=0)              # g' P_V g
        b = S[2 + c] - self.u.dot(z)                  # g' P_V y
        var = scale * self_rel
        pev = var - (scale * scale) * a
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = 1.0 - pev / var
        return {"u": scale * b, "pev": pev, "reliability": rel, "self_rel": np.array(self_rel, dtype=np.float64)}

    def _blocks(self, m, enqueue):
        """(q + 2) x m statistics: ``enqueue(k0, rb, stats_ptr)`` queues the block of columns k0 .. k0 + rb - 1."""
        out = np.empty((self.q + 2, m))
        if m:
            dS = self._stats_buffer(self.q + 2, m)
            self.torch.cuda.synchronize()
            self._run_blocks(dS, out, enqueue)
        return out

    def reliability(self, k=0, individuals=None):
        """Predicted value, prediction error variance and reliability of ``individuals`` (int array in the matrices' row order,
        distinct; default: everybody) for component ``k``: a dict of arrays ``u``, ``pev``, ``reliability`` and ``self_rel``
        (the diagonal entries of the component's matrix, as resident on the device), in the order of ``individuals``."""
        self._check_factor()
        w, scale = self._component(k)
        ids = np.arange(self.n, dtype=np.int32) if individuals is None else check_individuals(individuals, self.n)
        dQ = C.c_void_p(self.dQ.data_ptr())
        S = self._blocks(ids.size, lambda k0, rb, dst: self.factor.rel_block_dev(w, ids[k0:k0 + rb], dQ, self.q, dst))
        return self._finish(S, scale, S[0])

    def predict(self, rows, self_rel, k=0):
        """The same for m individuals outside the cohort: ``rows`` is the m x n SciPy sparse matrix of their relationships to
        the cohort in component ``k``'s matrix (for ``"total"``: in ``sum_k sigma2[k] mats[k]``), ``self_rel`` their own
        diagonal entries.  A relative without a phenotype has no row in V; its value is predicted through its relatives."""
        self._check_factor()
        _, scale = self._component(k)
        (indptr, indices, data), self_rel = check_rows(rows, self_rel, self.n)
        torch, vp = self.torch, C.c_void_p
        if data.size == 0:                                      # (all rows empty: the entry point still wants non-null arrays)
            indices, data = np.zeros(1, np.int32), np.zeros(1)
        d_ptr, d_idx, d_val = (torch.from_numpy(x).cuda() for x in (indptr, indices, data))
        dQ = vp(self.dQ.data_ptr())
        S = self._blocks(self_rel.size, lambda k0, rb, dst: self.factor.rows_block_dev(
            vp(d_ptr.data_ptr() + 8 * k0), vp(d_idx.data_ptr()), vp(d_val.data_ptr()), rb, dQ, self.q, dst))
        return self._finish(S, scale, self_rel)

    def effects(self, k=0):
        """All n predicted values of component ``k`` without blocks: ``sigma2_k A_k v`` with ``v = V^-1 (y - C beta) =
        P' L^-T (w(y) - w(C) beta)`` from ONE backward half-solve of one column, then one SpMM per matrix of the component."""
        self._check_factor()
        w, scale = self._component(k)
        torch, vp, c, n = self.torch, C.c_void_p, self.c, self.n
        if self._dv is None:
            res = (self.dQ[:, c] - self.dQ[:, :c] @ torch.from_numpy(self.beta).cuda()).contiguous()
            dx = torch.empty_like(res)
            torch.cuda.synchronize()
            self.factor.solve_Lt_dev(vp(res.data_ptr()), 1, vp(dx.data_ptr()))
            self.sym.sync()
            dv = torch.empty_like(dx)
            dv[torch.from_numpy(self.factor.P()).cuda()] = dx        # row p of the factor belongs to individual P[p]
            self._dv = dv
        dY = torch.empty((n,), dtype=torch.float64, device="cuda")
        out = np.zeros(n)
        for j in np.flatnonzero(w):
            torch.cuda.synchronize()
            self.sym.spmm_dev(int(j), vp(self._dv.data_ptr()), 1, vp(dY.data_ptr()))
            self.sym.sync()
            out += (scale * w[j]) * dY.cpu().numpy()
        return out

    # ---- everybody at once, from the selected inverse.  With G the total genetic covariance,
    #      E = sigma2[K-1] mats[K-1] diagonal (e_i its entries), V = G + E, Z = V^-1, H = Z C R^-1 and T = C R^-1 - E H = G H:
    #          G - G P_V G = E - E Z E + T T'        (G = V - E, so G Z G = V - 2 E + E Z E)
    #          P_V         = Z - H H'                u = G P_V y = y - C beta - E r,   r = P_V y
    #      so the diagonal of Z, and its entries on V's pattern for pairs of relatives, are all that is needed of the inverse.

    def _last_is_diagonal(self):
        ix = self.sym._indices[self.sym.K - 1]
        return ix.size == self.n and np.array_equal(ix, np.arange(self.n))

    def _diagonals(self):
        """(e, [diag(mats[k]) for k < K - 1]) in the matrices' row order, from the values resident on the device."""
        sym, P = self.sym, self.factor.P()
        first = sym.get("pat_colptr")[:-1]                         # (the diagonal slot comes first in its column)
        out = []
        for k in range(sym.K):
            v, d = sym.values_slots(k), np.empty(self.n)
            d[P] = v if v.size == self.n else v[first]             # (a diagonal-only matrix keeps one value per column)
            out.append(d)
        return self._s2[sym.K - 1] * out[-1], out[:-1]

    def _inverse_pass(self):
        """The pass the three whole-cohort methods share, run once and kept: ``V^-1 [C | y]`` from one device solve, ``H``,
        ``T`` and ``r`` from it (n x c arrays: torch), then the selected inverse, ``scilmm_inverse_pattern_dev`` twice --
        ``-E Z E + T T'`` on the pattern and its diagonal, ``Z - H H'`` on the diagonal -- and a refactorization at the
        object's own sigma2, so that the resident factor, a scan on it and this object go on as before.  Costs one inversion
        plus one factorization; on a deterministic handle the restored factor has the bits it had."""
        if self._inv is not None:
            return self._inv
        from .SparseCholesky import _solve_on_device
        torch, vp, c, n, sym, fac = self.torch, C.c_void_p, self.c, self.n, self.sym, self.factor
        e, gdiag = self._diagonals()
        dB = torch.from_numpy(np.ascontiguousarray(np.hstack([self.covariates, self._y[:, None]]))).cuda()
        dS = _solve_on_device(torch, sym, fac, dB)                 # Z [C | y], original order
        dRinv = torch.from_numpy(la.solve_triangular(self.R, np.eye(c), lower=False)).cuda()
        de = torch.from_numpy(e).cuda()
        dH = (dS[:, :c] @ dRinv).contiguous()                      # Z C R^-1
        dT = (dB[:, :c] @ dRinv - de[:, None] * dH).contiguous()   # C R^-1 - E H = G H
        dr = dS[:, c] - dH @ torch.from_numpy(self.u).cuda()       # P_V y   (H'y = R^-T C' Z y = u)
        nnz = int(sym.info().nnz_pattern)
        dpev, dpvd = (torch.empty((n,), dtype=torch.float64, device="cuda") for _ in range(2))
        doff = torch.empty((max(nnz, 1),), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        fac.selected_inverse()
        try:
            fac.inverse_pattern_dev(vp(dpev.data_ptr()), vp(doff.data_ptr()), -1.0, vp(de.data_ptr()), 1.0, vp(dT.data_ptr()), c)
            fac.inverse_pattern_dev(vp(dpvd.data_ptr()), None, 1.0, None, -1.0, vp(dH.data_ptr()), c)
            sym.sync()
        finally:
            fac.refactorize(self._s2)                              # (whatever happened: the factor is the caller's again)
        r = dr.cpu().numpy()
        self._inv = dict(e=e, gdiag=gdiag, r=r, pvd=dpvd.cpu().numpy(), pev=e + dpev.cpu().numpy(),
                         u=self._y - self.covariates @ self.beta - e * r, doff=doff[:nnz])
        return self._inv

    def _whole_cohort(self):
        if not self._last_is_diagonal():
            raise ValueError("the last matrix (the residual covariance) must be diagonal -- the identity or record weights -- for "
                             "the whole-cohort forms; reliability() has no such condition")
        self._check_factor()
        return self._inverse_pass()

    def reliability_all(self, k="total"):
        """``reliability`` for ALL n individuals from one selected inverse instead of one sweep column each: the same dict
        (``u``, ``pev``, ``reliability``, ``self_rel``) in the matrices' row order, for the total genetic value (``"total"``; with
        one relationship matrix also ``k = 0``, which is the total).  Exact: ``PEV_i = e_i - e_i^2 (V^-1)_ii + |T_i.|^2``.  A
        single component among several (K >= 3 and an index) is not exact from a selected inverse: ValueError, use
        ``reliability``.  The last matrix must be diagonal.  The first of ``reliability_all`` / ``prediction_error_covariance``
        / ``leave_one_out`` costs one inversion plus one factorization (the factor is consumed and restored at this object's
        sigma2; bit for bit on a deterministic handle); the others then cost nothing."""
        k = check_all_component(k, self.sym.K)
        inv = self._whole_cohort()
        if k == "total":
            scale, self_rel = 1.0, sum(s * d for s, d in zip(self._s2[:-1], inv["gdiag"]))
        else:
            scale, self_rel = float(self._s2[k]), inv["gdiag"][k].copy()
        var = scale * self_rel
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = 1.0 - inv["pev"] / var
        return {"u": inv["u"].copy(), "pev": inv["pev"].copy(), "reliability": rel, "self_rel": self_rel}

    def prediction_error_covariance(self):
        """The prediction error covariance of the total genetic values on V's pattern, as a symmetric SciPy CSR in the
        matrices' row order: PEV on the diagonal, ``PEC_ij = -e_i e_j (V^-1)_ij + T_i. . T_j.`` for every pair of relatives.
        The error variance of the difference of two relatives is ``PEV_i + PEV_j - 2 PEC_ij``.  Cost: see ``reliability_all``."""
        inv = self._whole_cohort()
        return self.factor.pattern_csr(inv["doff"].cpu().numpy(), inv["pev"])

    def leave_one_out(self):
        """Leave-one-out cross-validation of every record with the fixed effects re-estimated, without a refit: with
        ``r = P_V y`` a dict of ``residual`` (``r_i / (P_V)_ii``: the record minus its prediction from all the others),
        ``variance`` (``1 / (P_V)_ii``), ``studentized`` (``r_i / sqrt((P_V)_ii)``), ``prediction`` (``y - residual``) and
        ``leverage`` (``(P_V)_ii = (V^-1)_ii - |H_i.|^2``).  Cost: see ``reliability_all``."""
        inv = self._whole_cohort()
        r, p = inv["r"], inv["pvd"]
        res = r / p
        return {"residual": res, "variance": 1.0 / p, "studentized": r / np.sqrt(p), "prediction": self._y - res,
                "leverage": p.copy()}
