"""Binary traits: a logistic mixed model for the null and a score scan with saddlepoint p-values (SAIGE / GMMAT / fastGWA-GLMM
on a sparse relationship matrix, with the exact ``g' P g`` per marker).

    null = LogisticMixedModel(cholesky_func, mats, covariates, y).fit()     # y: 0 / 1; mats: the relationship matrices only
    scan = null.scan(cutoff=2.0)                                            # a BinaryScan (an AssociationScan) on null.mats_full
    out = scan(genotypes)            # also scan.scan_bed(...), scan.scan_dosages(...): the scan's arguments

NULL MODEL.  ``logit P(y_i = 1) = C_i alpha + b_i``, ``b ~ N(0, sum_k tau_k A_k)``, fitted by penalised quasi-likelihood as GMMAT's
``glmmkin`` runs it for a binomial family with the dispersion fixed at 1.  With ``mu = expit(eta)``, ``w = mu (1 - mu)`` and the
working vector ``y~ = eta + (y - mu) / w`` the working model is Gaussian with ``V = W^-1 + sum_k tau_k A_k``: ``mats + [diag(1 / w)]``
at coefficients ``[tau..., 1]`` is an ordinary evaluation of the engine (only the diagonal's values change between iterations),
and an iteration is ONE average-information step on tau -- ``score_k = y~'P A_k P y~ - tr(P A_k)`` from
``bolt_gradient_estimation(take_exp=False)``, ``AI_kl = y~'P A_k P A_l P y~`` from ``_ai_information`` -- halved until no
component is negative, then ``alpha`` and ``b`` at the new tau from one solve and K - 1 device SpMMs.  A component that is below
``tol`` before and after a step is set to 0 and stays there (glmmkin's rule): ``boundary``.

SCAN.  With ``y~`` in the place of ``y`` the scan block's ``b = g~'P y~`` and ``a = g~'P g~`` are the score and its exact
variance.  Behind every block ``scilmm_scan_spa*_dev`` turns them into a saddlepoint p-value where ``|b| / sqrt(a) > cutoff``:
the variance ratio ``a / a_w`` rescales the score to ``s = b sqrt(a_w / a)`` of the independent-Bernoulli statistic
``sum g^_i (y_i - mu_i)``, whose cumulant generating function is inverted on the device.

There is no CPU form of the device side; the argument checks and ``binary_stats`` are pure NumPy.  Out of scope: other families,
Firth correction, G x E tests for binary traits, distributed handles.  Variant-set tests at a fitted null: ``null.sets()``, a
``BinarySetTest`` (the method: DESIGN.md section 20; its host algebra: ``scilmm_amd.binary_sets``); with sets wider than one device
block, ``null.sets(max_markers=k)``, a ``BinaryWideSetTest``.
"""
import numpy as np
import scipy.linalg as la
import scipy.sparse as sp
import scipy.special as sc
import scipy.stats as stats

from . import _lib, assoc, binary_sets
from . import sets as setmod
from .markers import Int8Rows, as_run, vp

SPA_ROWS = 7                # log_p | a_w | s | zeta_hi | zeta_lo | iters | flag (csrc/spa.hip.h)
CMAX = 31                   # covariates at most (csrc/spa.hip.h SPA_CMAX)


def check_binary(covariates, y):
    """``(covariates, y)`` as float64 arrays: y 0 / 1 with both classes present, covariates n x c with 1 <= c <= 31 and one row per
    entry of y.  ValueError otherwise; nothing of a device is touched."""
    y = np.asarray(y)
    if y.dtype.kind not in "fiub" or y.ndim != 1:
        raise ValueError("y must be a vector of 0 / 1 values")
    y = y.astype(np.float64)
    if not np.all((y == 0) | (y == 1)):
        raise ValueError("y must be 0 / 1 (a missing phenotype is not supported: drop the individual)")
    if y.size == 0 or y.min() == y.max():
        raise ValueError("y holds one class only: nothing to fit")
    covariates = np.asarray(covariates, dtype=np.float64)
    if covariates.ndim != 2 or covariates.shape[0] != y.size:
        raise ValueError("covariates must be n x c with one row per entry of y")
    if not 1 <= covariates.shape[1] <= CMAX:
        raise ValueError("1 .. %d covariates (the intercept is the caller's), got %d" % (CMAX, covariates.shape[1]))
    if not np.all(np.isfinite(covariates)):
        raise ValueError("covariates must be finite")
    return np.ascontiguousarray(covariates), y


def check_cutoff(cutoff):
    cutoff = float(cutoff)
    if not cutoff >= 0.0:
        raise ValueError("cutoff must be >= 0, got %r" % (cutoff,))
    return cutoff


def check_null_covariates(null, covariates):
    """``covariates`` as the contiguous n x c float64 matrix of a fitted null (1 <= c <= 31, one row per fitted probability)."""
    covariates = np.ascontiguousarray(covariates, dtype=np.float64)
    if covariates.ndim != 2 or covariates.shape[0] != np.size(null.mu) or not 1 <= covariates.shape[1] <= CMAX:
        raise ValueError("covariates must be the n x c matrix (1 <= c <= %d) the null model was fitted with" % CMAX)
    return covariates


def upload_null(model, null, covariates):
    """What the saddlepoint kernels read of a fitted null, once per model: ``mu``, ``C``, ``(C'WC)^-1``, ``R`` and ``u`` on the device."""
    torch, model.null = model.torch, null
    w = np.asarray(null.weights, dtype=np.float64)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    model.dmu, model.dC = up(null.mu), up(covariates)
    model.dMinv = up(la.inv((covariates.T * w).dot(covariates)))
    model.dR, model.du = up(model.R), up(model.u)
    torch.cuda.synchronize()


def logistic_irls(C, y, tol=1e-12, max_iter=100):
    """The covariate-only logistic regression the PQL starts from (host)."""
    alpha = np.zeros(C.shape[1])
    for _ in range(max_iter):
        eta = C.dot(alpha)
        mu = sc.expit(eta)
        w = mu * (1.0 - mu)
        new = la.solve((C.T * w).dot(C), C.T.dot(w * eta + y - mu), assume_a="pos")
        done = np.abs(new - alpha).max() <= tol * max(1.0, np.abs(new).max())
        alpha = new
        if done:
            break
    return alpha


def binary_stats(S, SPA, R, u):
    """The host algebra of the binary scan.  ``S``: the (q + 4) x m statistics of the plain blocks; ``SPA``: the SPA_ROWS x m rows
    of the saddlepoint calls; ``R``, ``u``: the whitened model's.  Returns the dict ``BinaryScan.__call__`` documents.  Pure NumPy."""
    S, SPA = np.asarray(S, dtype=np.float64), np.asarray(SPA, dtype=np.float64)
    m, c = S.shape[1], R.shape[0]
    n_obs, mean, css, gg = S[0], S[1].copy(), S[2], S[3]
    z = la.solve_triangular(R, S[4:4 + c], trans='T', lower=False) if m else np.empty((c, 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        a = gg - np.sum(z * z, axis=0)
        b = S[4 + c] - u.dot(z)
        a = np.where((n_obs == 0) | (css == 0), np.nan, a)
        beta, se, chi2 = b / a, 1.0 / np.sqrt(a), b * b / a
        flag = np.where(np.isnan(SPA[6]), 0, SPA[6]).astype(np.int64)
        p_norm = stats.chi2.sf(chi2, 1)
        log_p = np.where(flag == 1, SPA[0], stats.chi2.logsf(chi2, 1))
        p = np.where(flag == 1, np.exp(SPA[0]), p_norm)
        ratio = np.where(flag == 0, np.nan, a / SPA[1])
    mean[n_obs == 0] = np.nan
    return {"beta": beta, "se": se, "chi2": chi2, "p_norm": p_norm, "p": p, "log_p": log_p, "spa_flag": flag,
            "n_obs": n_obs.astype(np.int64), "mean": mean, "variance_ratio": ratio}


class NullModel(object):
    """What ``LogisticMixedModel.fit`` returns: ``tau``, ``alpha``, ``b``, ``eta``, ``mu``, ``weights``, ``working_y``, ``n_iter``,
    ``converged``, ``boundary`` (a component ended at 0), and ``mats_full`` / ``sigma2_full`` (``mats + [diag(1 / weights)]`` at
    ``[tau..., 1]``), ready for ``AssociationScan`` / ``BLUP`` with ``working_y`` as the phenotype."""

    def __init__(self, model, **kw):
        self._model = model
        self.__dict__.update(kw)

    def scan(self, block=None, cutoff=2.0):
        """The score scan with saddlepoint p-values at this null: a ``BinaryScan``."""
        return BinaryScan(self._model.cholesky_func, self, self._model.covariates, block=block, cutoff=cutoff)

    def sets(self, block=None, cutoff=2.0, max_markers=None):
        """Burden, SKAT and SKAT-O of marker sets at this null, with saddlepoint-adjusted variances: a ``BinarySetTest``.  With
        ``max_markers`` (an integer in ``block`` .. 4096) a ``BinaryWideSetTest``, whose sets hold up to that many markers."""
        if max_markers is None:
            return BinarySetTest(self._model.cholesky_func, self, self._model.covariates, block=block, cutoff=cutoff)
        return BinaryWideSetTest(self._model.cholesky_func, self, self._model.covariates, block=block, cutoff=cutoff,
                                 max_markers=max_markers)


class LogisticMixedModel(object):
    """``LogisticMixedModel(cholesky_func, mats, covariates, y).fit(tau0=None, tol=1e-8, max_iter=100)``.  ``cholesky_func``: a
    ``SparseCholesky`` (its ``exact_trace`` decides how ``tr(P A_k)`` is taken: exact and deterministic, or the Monte-Carlo
    estimate); ``mats``: the K - 1 >= 1 relationship matrices; ``covariates``: n x c, 1 <= c <= 31, the intercept is the caller's;
    ``y``: n values 0 / 1.  ValueError for bad arguments before any device work."""

    def __init__(self, cholesky_func, mats, covariates, y):
        mats = list(mats)
        if len(mats) < 1:
            raise ValueError("at least one relationship matrix")
        self.covariates, self.y = check_binary(covariates, y)
        n = self.y.size
        for m in mats:
            if getattr(m, "shape", None) != (n, n):
                raise ValueError("every matrix must be n x n with n = %d (one row per entry of y)" % n)
        self.mats = [m if sp.isspmatrix_csr(m) else sp.csr_matrix(m) for m in mats]
        self.cholesky_func = cholesky_func

    def _check_fit(self, tau0, tol, max_iter):
        K1 = len(self.mats)
        tau = np.full(K1, 0.5) if tau0 is None else np.array(tau0, dtype=np.float64).ravel()
        if tau.shape != (K1,) or not np.all(np.isfinite(tau)) or np.any(tau < 0):
            raise ValueError("tau0 must hold one non-negative number per relationship matrix")
        if not (np.isfinite(tol) and tol > 0):
            raise ValueError("tol must be positive")
        if not (isinstance(max_iter, (int, np.integer)) and max_iter >= 1):
            raise ValueError("max_iter must be a positive integer")
        return tau

    def _full(self, w):
        return self.mats + [sp.diags(1.0 / w, format="csr")]

    def fit(self, tau0=None, tol=1e-8, max_iter=100, sim_num=100):
        from .SparseCholesky import (SparseCholesky, _DeviceProjector, _ai_information, _device_buffers, _final_factor,
                                     _spmm_on_device, bolt_gradient_estimation)
        tau = self._check_fit(tau0, tol, max_iter)
        chol, C, y = self.cholesky_func, self.covariates, self.y
        if not isinstance(chol, SparseCholesky):
            raise _lib.ScilmmError("LogisticMixedModel needs the device engine (a scilmm_amd.SparseCholesky): there is no CPU form")
        _lib.lib()
        torch = _device_buffers()
        if torch is None:
            raise _lib.ScilmmError("LogisticMixedModel needs a GPU that torch can reach (device buffers): there is no CPU form")
        K1, n = len(self.mats), y.size
        exact = bool(getattr(chol, "exact_trace", False))
        alpha, b = logistic_irls(C, y), np.zeros(n)
        converged, it = False, 0
        for it in range(1, max_iter + 1):
            eta = C.dot(alpha) + b
            mu = sc.expit(eta)
            w = mu * (1.0 - mu)
            yt = eta + (y - mu) / w
            full = self._full(w)
            s2 = np.append(tau, 1.0)
            # score / 2 = -(REML gradient) and AI / 2 at [tau..., 1]: one evaluation; with exact traces the information is taken
            # inside it, before the selected inverse consumes the factor (the hook of _ai_reml)
            if exact:
                chol._before_traces = lambda fac: _ai_information(fac, full, C, yt)
                try:
                    _, grad = bolt_gradient_estimation(s2, chol, full, C, yt, True, sim_num, False, take_exp=False)
                finally:
                    chol._before_traces = None
                info = chol._hook_result
            else:
                _, grad = bolt_gradient_estimation(s2, chol, full, C, yt, True, sim_num, False, take_exp=False)
                info = _ai_information(chol._factor_state[id(chol.engine_for(full))], full, C, yt)
            free = np.flatnonzero(tau > 0)                 # a component at 0 stays there
            new = tau.copy()
            if free.size:
                step, t = la.solve(info[np.ix_(free, free)], -grad[free]), 1.0
                for _ in range(64):
                    if np.all(tau[free] + t * step >= 0):
                        break
                    t *= 0.5
                else:
                    t = 0.0
                new[free] = tau[free] + t * step
            new[(new < tol) & (tau < tol)] = 0.0
            # alpha and b at the new tau: V^-1 [C | y~] in one sweep, then sum_k tau_k A_k P y~ by device SpMMs
            fac = _final_factor(chol, full, np.append(new, 1.0))
            sym = fac.sym
            pr = _DeviceProjector(torch, sym, fac, C, yt)
            alpha_new = la.cho_solve(pr.L_CT_Vinv_C, (pr.dC.T @ pr.Viy).cpu().numpy())
            Py = pr.project_solved(pr.Viy[:, None])
            db = torch.zeros_like(Py)
            for k in range(K1):
                if new[k] != 0.0:
                    db.add_(_spmm_on_device(torch, sym, k, Py), alpha=float(new[k]))
            b = db[:, 0].cpu().numpy()
            crit = max(np.max(np.abs(alpha_new - alpha) / (np.abs(alpha_new) + np.abs(alpha) + tol)),
                       np.max(np.abs(new - tau) / (new + tau + tol)))
            alpha, tau = alpha_new, new
            if crit < tol:
                converged = True
                break
        return self.null_at(tau, alpha, b, n_iter=it, converged=converged)

    def null_at(self, tau, alpha, b, n_iter=0, converged=False):
        """The ``NullModel`` of given ``tau`` (K - 1), ``alpha`` (c) and ``b`` (n) -- a fit kept from an earlier run, say: ``eta``,
        ``mu``, the weights, the working vector and ``mats_full`` / ``sigma2_full`` follow from them.  Host only."""
        C, y = self.covariates, self.y
        tau, alpha, b = (np.array(v, dtype=np.float64).ravel() for v in (tau, alpha, b))
        if tau.shape != (len(self.mats),) or alpha.shape != (C.shape[1],) or b.shape != y.shape or np.any(tau < 0):
            raise ValueError("tau, alpha and b must have one entry per relationship matrix, covariate and individual (tau >= 0)")
        eta = C.dot(alpha) + b
        mu = sc.expit(eta)
        w = mu * (1.0 - mu)
        return NullModel(self, tau=tau, alpha=alpha, b=b, eta=eta, mu=mu, weights=w, working_y=eta + (y - mu) / w, n_iter=n_iter,
                         converged=converged, boundary=bool(np.any(tau == 0)), mats_full=self._full(w),
                         sigma2_full=np.append(tau, 1.0))


class _Spa(object):
    """The per-block follow-up of a binary scan in the scan's block loop (``AssociationScan._stats``): a ``scan_spa*_dev`` behind
    every block of a chunk, and the chunk's SPA_ROWS rows per marker copied out when the chunk has been waited for."""

    def __init__(self, scan, src, m):
        self.scan, self.src, self.torch = scan, src, scan.torch
        self.out = np.empty((SPA_ROWS, m))

    def stage(self, rows_max):
        self.dS = self.scan._dS                      # the statistics buffer _stats has just allocated
        self.dP = self.scan._stats_buffer(SPA_ROWS, rows_max, keep=False)

    def block(self, k0, rb):
        s = self.scan
        blk, b = s.block, k0 // s.block
        pS = vp(self.dS.data_ptr() + 8 * b * (s.q + 4) * blk)
        pP = vp(self.dP.data_ptr() + 8 * b * SPA_ROWS * blk)
        self.src.spa(k0, rb, (pS, vp(s.dR.data_ptr()), vp(s.du.data_ptr()), vp(s.dmu.data_ptr()), vp(s.dC.data_ptr()), s.c,
                              vp(s.dMinv.data_ptr()), s.cutoff, pP))

    def chunk(self, j0, mc, dS, nrows, blk):
        hP = self.dP.cpu().numpy()
        for b, k0 in enumerate(range(0, mc, blk)):
            rb = min(blk, mc - k0)
            self.out[:, j0 + k0:j0 + k0 + rb] = hP[b, :SPA_ROWS * rb].reshape(SPA_ROWS, rb)


class BinaryScan(assoc.AssociationScan):
    """The marker scan of a fitted ``NullModel``: an ``AssociationScan`` of ``working_y`` under ``mats_full`` / ``sigma2_full`` whose
    every block is followed by its saddlepoint call.  ``mu``, ``C``, ``(C'WC)^-1``, ``R`` and ``u`` are uploaded once; nothing is
    waited for between a block and its follow-up, and only SPA_ROWS numbers per marker come back beside the scan's q + 4."""

    def __init__(self, cholesky_func, null, covariates, block=None, cutoff=2.0):
        self.cutoff = check_cutoff(cutoff)
        covariates = check_null_covariates(null, covariates)
        super(BinaryScan, self).__init__(cholesky_func, null.mats_full, null.sigma2_full, covariates, null.working_y, block)
        self._dS = None
        upload_null(self, null, covariates)

    def _stats_buffer(self, nrows, m, blk=None, keep=True):
        buf = super(BinaryScan, self)._stats_buffer(nrows, m, blk)
        if keep:
            self._dS = buf
        return buf

    def _binary(self, src, rows, chunk_bytes):
        self._check_factor()
        m = rows.stop - rows.start if isinstance(rows, slice) else rows.size
        follow = _Spa(self, src, m)
        S = self._stats(src, rows, chunk_bytes, follow=follow)
        self.last_spa = follow.out                   # the device's SPA_ROWS x m rows as they came back (a_w, s, the roots, iters)
        return binary_stats(S, follow.out, self.R, self.u)

    def __call__(self, genotypes):
        """``genotypes`` as for ``AssociationScan.__call__``.  Returns a dict of length-m arrays: ``beta = b / a`` (log-odds scale),
        ``se = a^-1/2``, ``chi2 = b^2 / a``, ``p_norm`` (chi2 with 1 df), ``p`` (the saddlepoint value where ``spa_flag == 1``,
        else ``p_norm``), ``log_p``, ``spa_flag`` (0: not attempted, 1: saddlepoint, 2: attempted and failed), ``n_obs``,
        ``mean`` and ``variance_ratio = a / a_w`` (NaN where no saddlepoint was attempted)."""
        g = assoc.check_genotypes(genotypes, self.n)
        return self._binary(Int8Rows(self, g), slice(0, g.shape[0]), assoc._CHUNK_BYTES)

    def scan_bed(self, bed, sample_index=None, markers=None, count="A1", chunk_bytes=None):
        """``__call__`` on the markers of a PLINK 1 fileset; the arguments of ``AssociationScan.scan_bed``."""
        from .bed import marker_indices
        src = self._bed_source(bed, sample_index, count)
        rows = marker_indices(markers, src.m)
        return self._binary(src, as_run(rows), int(assoc._CHUNK_BYTES if chunk_bytes is None else chunk_bytes))

    def scan_dosages(self, dosages, sample_index=None, chunk_bytes=None):
        """``__call__`` on imputed dosages; the arguments of ``AssociationScan.scan_dosages``."""
        src = self._dosage_source(dosages, sample_index)
        chunk_bytes = int(assoc._CHUNK_BYTES if chunk_bytes is None else chunk_bytes)
        if chunk_bytes < 1:
            raise ValueError("chunk_bytes must be positive")
        return self._binary(src, slice(0, src.m), chunk_bytes)


class BinarySetTest(setmod.VariantSetTest):
    """Burden, SKAT and SKAT-O of marker sets at a fitted ``NullModel``, with the variance of every marker and of the burden
    re-calibrated by the saddlepoint approximation before the tests are taken (SAIGE-GENE / SMMAT, with the exact
    ``K = G~' P G~`` of the Gram block): a ``VariantSetTest`` of ``working_y`` under ``mats_full`` /
    ``sigma2_full`` whose every block is followed, on the stream and without a wait in between, by the saddlepoint call of its
    markers (``scan_spa*``), the sets' variance scales and burden saddlepoint (``sets_spa*``) and -- with ``finish="device"`` -- the
    scaled finish.  ``__call__``, ``test_bed`` and ``test_dosages`` take the arguments of ``VariantSetTest``'s and return its keys
    with ``burden_p = chi2_1.sf(burden_chi2)``, plus ``burden_chi2_norm = b_B^2 / a_B`` (the unadjusted burden), ``burden_spa_log_p``
    and ``burden_spa_flag`` (the burden's own saddlepoint call; 0: not attempted), ``burden_scale = phi`` (the burden floor) and
    ``n_adjusted`` (kept markers whose variance scale is not 1).  ``return_kernel=True`` (host finish) hands out
    ``(s, K~, w, vscale)`` per set, ``K~ = diag(vscale) K diag(vscale)``.  ``last_bspa`` keeps the device's 13 numbers per set."""

    def __init__(self, cholesky_func, null, covariates, block=None, cutoff=2.0):
        self.cutoff = check_cutoff(cutoff)
        covariates = check_null_covariates(null, covariates)
        super(BinarySetTest, self).__init__(cholesky_func, null.mats_full, null.sigma2_full, covariates, null.working_y, block)
        upload_null(self, null, covariates)

    def _block_binary(self, src, mode, method, rho, device):
        """(rows, offsets, weights) -> (the sets' 13 saddlepoint numbers, the columns' variance scales, the finish): the Gram entry
        point, the markers' saddlepoint call, the sets' and -- ``device`` -- the scaled finish queued one behind the other, one wait;
        the finish is the sets' rows of the device, or the block's statistics and Gram matrix for the host's."""
        torch, q, blk, c = self.torch, self.q, self.block, self.c
        src.stage(blk)
        new = lambda k: torch.empty((k,), dtype=torch.float64, device="cuda")
        dS, dK, dP, dB, dV, dW = new((q + 4) * blk), new(blk * blk), new(SPA_ROWS * blk), new(blk * binary_sets.BSPA_ROWLEN), new(blk), new(blk)
        ld = setmod.FINISH_HEAD + rho.size
        dO = new(blk * ld)
        meth = setmod.METHODS.index(method)
        pS, pK, pP, pB, pV, pO = (vp(d.data_ptr()) for d in (dS, dK, dP, dB, dV, dO))
        pR, pu = vp(self.dR.data_ptr()), vp(self.du.data_ptr())
        null = (pR, pu, vp(self.dmu.data_ptr()), vp(self.dC.data_ptr()), c, vp(self.dMinv.data_ptr()), self.cutoff, pP)

        def run(rows, start, w):
            rb, ns = rows.size, start.size - 1
            src.load(rows)
            if w is not None:
                dW[:rb].copy_(torch.from_numpy(w))
            pW = vp(dW.data_ptr()) if w is not None else None
            src.enqueue(0, rb, pS, pK)
            src.spa(0, rb, (pS,) + null)
            src.sets_spa(0, rb, (pS, pK) + null + (ns, start, mode, pW, pB, pV))
            if device:
                self.factor.sets_finish_scaled_dev(rb, q, pS, pK, pR, pu, c, ns, start, mode, pW, meth, rho, pO, ld, None, pV)
            self.sym.sync()
            B = dB[:ns * binary_sets.BSPA_ROWLEN].cpu().numpy().reshape(ns, binary_sets.BSPA_ROWLEN)
            if device:
                return B, None, dO[:ns * ld].cpu().numpy().reshape(ns, ld)
            return B, dV[:rb].cpu().numpy(), (dS[:(q + 4) * rb].cpu().numpy().reshape(q + 4, rb), dK[:rb * rb].cpu().numpy().reshape(rb, rb))
        return run

    def _run(self, src, sets, weights, method, return_kernel, skato=False, rho=None, finish="host", max_markers=None):
        """The checks of ``VariantSetTest._run`` (before any launch), then block by block the four calls of ``_block_binary`` and
        step 5 of the method: on the device's rows, or in NumPy on ``(t, A~)`` (``binary_sets.scaled_tests``).  ``max_markers``
        must be None: the set saddlepoint collapses the genotypes of ONE block."""
        if max_markers is not None:
            raise ValueError("max_markers is not supported for binary traits: the set saddlepoint collapses the genotypes of one "
                             "block, so a set holds at most %d markers" % self.block)
        sets = setmod.check_sets(sets, src.m, self.block)
        weights = setmod.check_weights(weights, sets)
        setmod.check_method(method)
        if finish not in setmod.FINISHES:
            raise ValueError("finish must be one of %s, got %r" % (", ".join(setmod.FINISHES), finish))
        if finish == "device" and return_kernel:
            raise ValueError('return_kernel=True needs finish="host": the device finish does not bring K back')
        rho = setmod.check_rho(rho) if skato else None
        self._check_factor()
        ns, device = len(sets), finish == "device"
        out = self._out(ns, skato, rho)
        given, mode = self._weight_mode(weights)
        block = self._block_binary(src, mode, method, rho if skato else np.empty(0), device) if sets else None
        kernel = [None] * ns
        for members in setmod.pack_sets([s.size for s in sets], self.block):
            self._narrow(out, kernel, members, sets, weights, given, block, device, method, rho, skato)
        return self._done(out, kernel, return_kernel)

    def _out(self, ns, skato, rho):
        """The result of a call before any set has run: NaN, the counts 0; ``last_bspa`` likewise."""
        out = {k: np.full(ns, np.nan) for k in setmod.KEYS + binary_sets.BINARY_KEYS}
        for k in ("n_used", "burden_spa_flag", "n_adjusted"):
            out[k] = np.zeros(ns, dtype=np.int64)
        if skato:
            out.update({k: np.full(ns, np.nan) for k in setmod.SKATO_KEYS[:3]})
            out["skato_p_rho"] = np.full((ns, rho.size), np.nan)
        self.last_bspa = np.full((ns, binary_sets.BSPA_ROWLEN), np.nan)
        return out

    @staticmethod
    def _weight_mode(weights):
        given = not (weights is None or isinstance(weights, str))
        return given, setmod.WEIGHT_GIVEN if given else setmod.WEIGHT_ONES if weights is None else setmod.WEIGHT_BETA

    @staticmethod
    def _device_rows(out, members, fin, skato):
        """The rows of a device finish into the result."""
        out["n_used"][members] = fin[:, 0].astype(np.int64)
        for col, k in ((1, "burden_beta"), (2, "burden_se"), (3, "burden_chi2"), (4, "skat_q"), (5, "skat_p")):
            out[k][members] = fin[:, col]
        if skato:
            for col, k in ((6, "skato_p"), (7, "skato_pmin"), (8, "skato_rho")):
                out[k][members] = fin[:, col]
            out["skato_p_rho"][members] = fin[:, setmod.FINISH_HEAD:]

    def _host_set(self, out, kernel, i, S, G, wi, V, method, rho):
        """Step 5 of set ``i`` on the host: its columns of the statistics, its X'X and its columns' scales."""
        s, K, wk, keep = setmod.set_kernel(S, G, self.R, self.u, wi)
        vs = V[keep]
        out["n_used"][i] = int(keep.sum())
        if keep.any():
            t = binary_sets.scaled_tests(s, K, wk, vs, method, rho)
            for k in ("burden_beta", "burden_se", "burden_chi2", "skat_q", "skat_p"):
                out[k][i] = t[k]
            if t["skato"] is not None:
                out["skato_p"][i], out["skato_pmin"][i], out["skato_rho"][i], out["skato_p_rho"][i] = t["skato"]
        kernel[i] = (s, vs[:, None] * K * vs[None, :], wk, vs)

    def _narrow(self, out, kernel, members, sets, weights, given, block, device, method, rho, skato):
        """One block of sets of at most ``block`` markers through ``_block_binary``'s ``block`` and into the result."""
        start = np.concatenate([[0], np.cumsum([sets[i].size for i in members])]).astype(np.int32)
        w = np.ascontiguousarray(np.concatenate([weights[i] for i in members])) if given else None
        B, V, fin = block(np.concatenate([sets[i] for i in members]), start, w)
        self.last_bspa[members] = B
        if device:
            return self._device_rows(out, members, fin, skato)
        S, G = fin
        for i, a, b in zip(members, start[:-1], start[1:]):
            self._host_set(out, kernel, i, S[:, a:b], G[a:b, a:b], weights if not given else weights[i], V[a:b], method, rho)

    def _done(self, out, kernel, return_kernel):
        """What follows from the sets' 13 numbers, for every set of the call at once."""
        P = self.last_bspa
        used = out["n_used"] > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            out["burden_chi2_norm"] = P[:, 8] * P[:, 8] / P[:, 7]
        out["burden_p"][used] = stats.chi2.sf(out["burden_chi2"][used], 1)
        out["burden_spa_log_p"], out["burden_scale"] = P[:, 0].copy(), P[:, 11].copy()
        out["burden_spa_flag"], out["n_adjusted"] = P[:, 6].astype(np.int64), P[:, 12].astype(np.int64)
        if return_kernel:
            out["kernel"] = kernel
        return out


class BinaryWideSetTest(BinarySetTest):
    """``BinarySetTest`` for sets of up to ``max_markers`` <= 4096 markers (``NullModel.sets(max_markers=...)``; DESIGN.md section
    23).  ``__call__``, ``test_bed`` and ``test_dosages`` take the arguments of ``BinarySetTest``'s; a per-call ``max_markers``
    overrides the constructor's, and ``finish`` is ``"host"``, ``"device"`` or ``"wide"`` with the meaning it has on
    ``VariantSetTest`` (``"device"`` with a set wider than ``block`` is the same ``ValueError``).  The sets of at most ``block``
    markers are packed as if the wider ones were not in the list (``sets.plan_sets``) and run as ``BinarySetTest`` runs them: the
    blocks and the bits of a call on them alone.  A wider set runs on its own, in its position, as ``ceil(k / block)`` sub-blocks
    with one wait each: the rows are loaded, then the Gram entry point into the set's slices, the markers' saddlepoint call into
    its slice, the collapse (``scilmm_sets_collapse*_dev``: the burden's collapsed genotype grows by the sub-block's kept
    markers), the panel against the kept sub-blocks and the keep.  ``scilmm_sets_spa_wide_dev`` is queued behind the last one;
    with ``finish="wide"`` ``scilmm_sets_finish_wide_scaled_dev`` follows and the set's 13 numbers and one row come back, with
    ``finish="host"`` the pieces, the 13 numbers and the scales come back and the host runs ``sets.assemble_wide``,
    ``sets.set_kernel`` and ``binary_sets.scaled_tests``.  The result has the keys of ``BinarySetTest``, ``last_bspa`` included;
    ``return_kernel=True`` (host finish) hands out ``(s, K~, w, vscale)`` per set."""

    def __init__(self, cholesky_func, null, covariates, block=None, cutoff=2.0, max_markers=None):
        super(BinaryWideSetTest, self).__init__(cholesky_func, null, covariates, block=block, cutoff=cutoff)
        self.max_markers = setmod.check_max_markers(max_markers, self.block)

    def _block_binary_wide(self, src, bmax, staged, mode, method, rho, device):
        """(rows, weights) -> (the set's 13 saddlepoint numbers, its markers' variance scales, the finish) of one set of more than
        ``block`` rows and up to ``bmax`` sub-blocks: the sub-blocks as in ``VariantSetTest._block_wide_device``, each followed by
        its saddlepoint call and its collapse; then the set saddlepoint and -- ``device`` -- the scaled wide finish.  The finish is
        the row of the device, or the assembled statistics and X'X for the host's."""
        torch, q, blk, c, n = self.torch, self.q, self.block, self.c, self.n
        bp = (blk + 15) // 16 * 16
        ld = (bmax - 1) * bp
        if not staged:
            src.stage(blk)
        new = lambda k: torch.empty((k,), dtype=torch.float64, device="cuda")
        dS, dK, dX, dP = new(bmax * (q + 4) * blk), new(bmax * blk * blk), new(bmax * blk * ld), new(bmax * SPA_ROWS * blk)
        store, dg, dW, dB, dV = new(n * ld), new(n), new(bmax * blk), new(binary_sets.BSPA_ROWLEN), new(bmax * blk)
        lo = setmod.FINISH_HEAD + rho.size
        dO = new(lo)
        meth = setmod.METHODS.index(method)
        pR, pu = vp(self.dR.data_ptr()), vp(self.du.data_ptr())
        null = (pR, pu, vp(self.dmu.data_ptr()), vp(self.dC.data_ptr()), c, vp(self.dMinv.data_ptr()), self.cutoff)
        at = lambda d, off: vp(d.data_ptr() + 8 * off)

        def run(rows, w):
            k = rows.size
            B = -(-k // blk)
            if w is not None:
                dW[:k].copy_(torch.from_numpy(w))
            for b in range(B):
                sub = rows[b * blk:(b + 1) * blk]
                rb, t = sub.size, b * bp
                pS = at(dS, b * (q + 4) * blk)
                src.load(sub)
                src.enqueue(0, rb, pS, at(dK, b * blk * blk))
                src.spa(0, rb, (pS,) + null + (at(dP, b * SPA_ROWS * blk),))
                src.collapse(0, rb, (pS, mode, at(dW, b * blk) if w is not None else None, b == 0, vp(dg.data_ptr())))
                if b > 0:
                    self.factor.scan_panel_dev(rb, vp(store.data_ptr()), ld, t, at(dX, b * blk * ld), ld)
                if b < B - 1:
                    self.factor.scan_block_keep_dev(rb, vp(store.data_ptr()), ld, t)
                self.sym.sync()
            pW = vp(dW.data_ptr()) if w is not None else None
            wide = (k, blk, q, vp(dS.data_ptr()), vp(dK.data_ptr()), vp(dX.data_ptr()), ld)
            self.factor.sets_spa_wide_dev(*(wide + null + (vp(dP.data_ptr()), mode, pW, vp(dg.data_ptr()), vp(dB.data_ptr()),
                                                          vp(dV.data_ptr()))))
            if device:
                self.factor.sets_finish_wide_scaled_dev(*(wide + (pR, pu, c, mode, pW, meth, rho, vp(dO.data_ptr()), None,
                                                                  vp(dV.data_ptr()))))
            self.sym.sync()
            row = dB.cpu().numpy().reshape(1, binary_sets.BSPA_ROWLEN)
            if device:
                return row, None, dO.cpu().numpy().reshape(1, lo)
            hS, hK, hX = dS.cpu().numpy(), dK.cpu().numpy(), dX.cpu().numpy()
            rbs = [min(blk, k - b * blk) for b in range(B)]
            Ss = [hS[b * (q + 4) * blk:][:(q + 4) * rb].reshape(q + 4, rb) for b, rb in enumerate(rbs)]
            Gs = [hK[b * blk * blk:][:rb * rb].reshape(rb, rb) for b, rb in enumerate(rbs)]
            Xs = [hX[b * blk * ld:][:rb * ld].reshape(rb, ld)[:, :b * bp] for b, rb in enumerate(rbs) if b > 0]
            return row, dV[:k].cpu().numpy(), setmod.assemble_wide(Ss, Gs, Xs, bp)
        return run

    def _run(self, src, sets, weights, method, return_kernel, skato=False, rho=None, finish="host", max_markers=None):
        """The checks of ``VariantSetTest._run`` (before any launch); then the work of ``sets.plan_sets`` in its order: a block of
        narrow sets through ``BinarySetTest``'s calls, a wide set through ``_block_binary_wide``."""
        max_markers = self.max_markers if max_markers is None else max_markers
        sets = setmod.check_sets(sets, src.m, self.block, max_markers)
        weights = setmod.check_weights(weights, sets)
        setmod.check_method(method)
        if finish not in setmod.FINISH_VALUES:
            raise ValueError("finish must be one of %s, got %r" % (", ".join(setmod.FINISH_VALUES), finish))
        if finish != "host" and return_kernel:
            raise ValueError('return_kernel=True needs finish="host": the device finish does not bring K back')
        sizes = [s.size for s in sets]
        widest = max(sizes + [0])
        if finish == "device" and widest > self.block:
            raise ValueError('a set of %d markers needs finish="host" or finish="wide": the device finish holds one block of at most '
                             '%d markers in LDS' % (widest, self.block))
        rho = setmod.check_rho(rho) if skato else None
        self._check_factor()
        ns, device = len(sets), finish != "host"
        out = self._out(ns, skato, rho)
        given, mode = self._weight_mode(weights)
        grid = rho if skato else np.empty(0)
        narrow = any(k <= self.block for k in sizes)
        block = self._block_binary(src, mode, method, grid, device) if narrow else None
        wide = self._block_binary_wide(src, -(-widest // self.block), narrow, mode, method, grid, device) if widest > self.block else None
        kernel = [None] * ns
        for members in setmod.plan_sets(sizes, self.block):
            i = members[0]
            if sizes[i] <= self.block:
                self._narrow(out, kernel, members, sets, weights, given, block, device, method, rho, skato)
                continue
            B, V, fin = wide(sets[i], np.ascontiguousarray(weights[i]) if given else None)
            self.last_bspa[members] = B
            if device:
                self._device_rows(out, members, fin, skato)
            else:
                self._host_set(out, kernel, i, fin[0], fin[1], weights if not given else weights[i], V, method, rho)
        return self._done(out, kernel, return_kernel)
