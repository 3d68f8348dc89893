"""Phenotype panels in the marker scan: many traits against one marker block, and null max-chi2 thresholds.

The whitened markers ``X = w(G~)`` of a scan block do not depend on the phenotype, and the block is almost all forward sweep.
With the traits whitened once and projected off the whitened covariates, ``Y~ = (I - Q_c Q_c') w(Y)``, ``Q_c = w(C) R^-1``, the
numerator of every (marker, trait) pair is one entry of ``B = X'Y~`` -- one more GEMM-shaped pass over the block on the fp64
matrix pipe (``scilmm_scan_panel_dev``) -- and the denominator ``a_j = |x_j|^2 - |R^-T w(C)'x_j|^2`` is the scan's own::

    panel = scan.traits(Y, scale="fixed")        # Y: n x T float64, finite, 1 <= T <= 4096, rows in the order of mats
    out = panel(genotypes)                        # also panel.scan_bed(...), panel.scan_dosages(...): the scan's arguments
    null = scan.null_panel(n_rep=1000, seed=0)   # a panel of simulated null phenotypes
    mx = null(genotypes, reduce="max")            # {"max_chi2": (n_rep,), "argmax": (n_rep,) int64, "n_tested": int}
    thr = panel_thresholds(mx["max_chi2"], n=scan.n, alpha=0.05)   # {"chi2", "p", "m_eff"}

Two uses.  MANY TRAITS under a shared V (the EMMAX / P3D approximation: the variance RATIOS of the scan for every trait;
``scale="profile"`` profiles the overall scale per trait, ``scale="fixed"`` takes V as given).  A GENOME-WIDE THRESHOLD that is
valid for related individuals: a parametric bootstrap of the per-replicate maximum chi2 ("max-T") under ``N(C beta, V)`` --
permuting phenotypes is wrong under a kinship covariance, Bonferroni ignores LD.  In whitened space a null phenotype is
``w(y*) = w(C) beta + z``, ``z ~ N(0, I)``, so the replicates are drawn where they are used and need no solve at all.

Out of scope: per-trait missing phenotypes (``check_traits`` refuses a NaN: drop the individuals or run the traits one by one),
another V per trait, panels on ``InteractionScan`` (a marker panel is built from an ``AssociationScan`` only; the variant-set
tests of a ``VariantSetTest`` against a panel are ``tester.set_traits(Y)``, ``scilmm_amd.set_panel``), distributed handles and fp32 fronts (the C entry point refuses both).  There is no CPU form of the device side; the host
algebra (``panel_stats``, ``panel_thresholds``) and the argument checks are pure NumPy.
"""
import numpy as np
import scipy.linalg as la
import scipy.stats as stats

from . import _lib, assoc
from .markers import Int8Rows, as_run, vp

TMAX = 4096                 # columns of a panel at most (csrc/panel.hip.h PANEL_TMAX)
SCALES = ("fixed", "profile")
REDUCES = (None, "max")
# B = X'Y~ of one chunk stays on the device until the chunk is done: a chunk holds at most this many bytes of it (whole
# blocks, at least one), next to the assoc._CHUNK_BYTES of marker rows it is sized by otherwise
_PANEL_BYTES = 64 << 20


def check_scale(scale):
    if scale not in SCALES:
        raise ValueError("scale must be 'fixed' or 'profile', got %r" % (scale,))
    return scale


def check_reduce(reduce):
    if reduce not in REDUCES:
        raise ValueError("reduce must be None or 'max', got %r" % (reduce,))
    return reduce


def check_traits(Y, n):
    """The trait matrix as the device path takes it: n x T float64, C-contiguous (a vector is refused: say ``y[:, None]``),
    1 <= T <= 4096, finite.  TypeError for something that is no real array, ValueError for another shape, for T out of range
    and for a NaN or an infinity (per-trait missing phenotypes are out of scope); nothing of a device is touched."""
    if isinstance(Y, (str, bytes)) or not hasattr(Y, "__len__"):
        raise TypeError("Y must be an n x T array of phenotypes, got %s" % type(Y).__name__)
    Y = np.asarray(Y)
    if Y.dtype.kind not in "fiub":
        raise TypeError("Y must be real numbers, got dtype %s" % Y.dtype)
    if Y.ndim != 2 or Y.shape[0] != n:
        raise ValueError("Y must be n x T with one row per individual (n = %d); got shape %s" % (n, Y.shape))
    if not 1 <= Y.shape[1] <= TMAX:
        raise ValueError("a panel has 1..%d traits, got %d" % (TMAX, Y.shape[1]))
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    if not np.all(np.isfinite(Y)):
        raise ValueError("Y must be finite: per-trait missing phenotypes are not supported (drop the individuals, or scan "
                         "the traits with missing values one by one)")
    return Y


def check_n_rep(n_rep):
    if isinstance(n_rep, bool) or not isinstance(n_rep, (int, np.integer)):
        raise TypeError("n_rep must be an integer, got %s" % type(n_rep).__name__)
    if not 1 <= n_rep <= TMAX:
        raise ValueError("n_rep must be in 1..%d (run several panels with different seeds for more), got %d" % (TMAX, n_rep))
    return int(n_rep)


def check_seed(seed):
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise TypeError("seed must be an integer, got %s" % type(seed).__name__)
    return int(seed)


def panel_stats(S, B, R, n, scale="fixed", s_t=None):
    """The host algebra of a panel.  ``S``: the (q + 4) x m statistics of the scan's plain block (rows n_obs | mean | centred
    sum of squares | |x|^2 | the c rows of w(C)'x | ..., q = c + 1); ``B``: m x T, ``B[j, t] = x_j . y~_t`` for traits projected
    off the whitened covariates; ``R``: c x c upper triangular, R'R = w(C)'w(C); ``n`` individuals.  ``a_j = |x_j|^2 - |z_j|^2``,
    ``z_j = R^-T w(C)'x_j``, exactly as ``AssociationScan._finish`` computes it; ``beta = B / a``.  ``scale="fixed"``: V as given,
    ``se = a^-1/2``, ``chi2 = B^2 / a``.  ``scale="profile"``: the per-trait scale ``s_t`` (T numbers, ``|y~_t|^2 / (n - c)``)
    multiplies se^2 and divides chi2, and is returned as ``"scale"``.  ``p = F(1, n - 1).sf(chi2)``.  A marker without an observed
    value or without variation is NaN across its row.  Pure NumPy: no device."""
    check_scale(scale)
    S, B = np.asarray(S, dtype=np.float64), np.asarray(B, dtype=np.float64)
    c = R.shape[0]
    if S.ndim != 2 or S.shape[0] < 4 + c or B.ndim != 2 or B.shape[0] != S.shape[1]:
        raise ValueError("statistics of shape %s and products of shape %s do not belong together (c = %d)" % (S.shape, B.shape, c))
    m, T = B.shape
    n_obs, mean, css, gg = S[0], S[1].copy(), S[2], S[3]
    z = la.solve_triangular(R, S[4:4 + c], trans='T', lower=False) if m else np.empty((c, 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        a = gg - np.sum(z * z, axis=0)
        a = np.where((n_obs == 0) | (css == 0), np.nan, a)[:, None]
        beta, chi2 = B / a, B * B / a
        se2 = np.broadcast_to(1.0 / a, (m, T))
        out = {}
        if scale == "profile":
            s_t = np.asarray(s_t, dtype=np.float64)
            if s_t.shape != (T,):
                raise ValueError("scale='profile' needs one scale per trait")
            se2, chi2 = se2 * s_t, chi2 / s_t
            out["scale"] = s_t.copy()
        se = np.sqrt(se2)
    mean[n_obs == 0] = np.nan
    out.update({"beta": beta, "se": se, "chi2": chi2, "p": stats.f(1, n - 1).sf(chi2), "n_obs": n_obs.astype(np.int64), "mean": mean})
    return out


def panel_thresholds(max_chi2, n, alpha=0.05):
    """The genome-wide threshold from the per-replicate maxima of a null panel: ``chi2`` = the 1 - alpha quantile of
    ``max_chi2`` by the rule "higher" (an order statistic, conservative), ``p = F(1, n - 1).sf(chi2)`` (the scan's convention),
    ``m_eff = alpha / p`` (the number of independent tests a Bonferroni correction would have to assume).  Pure NumPy."""
    v = np.asarray(max_chi2, dtype=np.float64).ravel()
    if v.size < 1 or not np.all(np.isfinite(v)):
        raise ValueError("max_chi2 must be a non-empty vector of finite numbers")
    if not 0.0 < alpha < 1.0:
        raise ValueError("alpha must lie strictly between 0 and 1")
    chi2 = float(np.quantile(v, 1.0 - alpha, method="higher"))
    p = float(stats.f(1, n - 1).sf(chi2))
    return {"chi2": chi2, "p": p, "m_eff": alpha / p}


class _Products(object):
    """The per-block follow-up of a panel in the scan's block loop (``AssociationScan._stats``): ``B`` of a chunk on the
    device, a ``scan_panel_dev`` behind every block, and what becomes of a finished chunk -- copied out (full) or reduced to the
    running maxima on the device (``reduce="max"``)."""

    def __init__(self, panel, m, reduce):
        self.panel, self.reduce, self.torch = panel, reduce, panel.scan.torch
        T = panel.T
        if reduce is None:
            self.B = np.empty((m, T))
        else:
            self.best = self.torch.full((T,), -np.inf, dtype=self.torch.float64, device="cuda")
            self.arg = self.torch.full((T,), -1, dtype=self.torch.int64, device="cuda")
            self.n_tested = 0

    def stage(self, rows_max):
        self.dB = self.torch.empty((rows_max, self.panel.T), dtype=self.torch.float64, device="cuda")

    def block(self, k0, rb):
        p = self.panel
        p.scan.factor.scan_panel_dev(rb, vp(p.dY.data_ptr()), p.ld, p.T, vp(self.dB.data_ptr() + 8 * k0 * p.T), p.T)

    def chunk(self, j0, mc, dS, nrows, blk):
        """The chunk of markers j0 .. j0 + mc - 1 is done (the stream has been waited for)."""
        if self.reduce is None:
            self.B[j0:j0 + mc] = self.dB[:mc].cpu().numpy()
            return
        torch, scan = self.torch, self.panel.scan
        c, full = scan.c, mc // blk
        # the statistics of the chunk, rows x markers: the full blocks, then the partial last block in its own packing
        parts = []
        if full:
            parts.append(dS[:full].reshape(full, nrows, blk).permute(1, 0, 2).reshape(nrows, full * blk))
        if mc > full * blk:
            parts.append(dS[full, :nrows * (mc - full * blk)].reshape(nrows, mc - full * blk))
        S = torch.cat(parts, dim=1)
        z = torch.linalg.solve_triangular(self.panel.dRt, S[4:4 + c], upper=False)      # R^-T w(C)'x: c x mc
        a = S[3] - (z * z).sum(dim=0)
        ok = (S[0] != 0) & (S[2] != 0)
        B = self.dB[:mc]
        chi2 = B * B / a[:, None]
        chi2[~ok] = -np.inf                                   # a degenerate marker is excluded
        cmax, carg = chi2.max(dim=0)
        better = cmax > self.best
        self.best = torch.where(better, cmax, self.best)
        self.arg = torch.where(better, carg + j0, self.arg)
        self.n_tested += int(ok.sum().item())


class TraitPanel(object):
    """``scan.traits(Y)`` / ``scan.null_panel(...)``: T phenotype columns, whitened, projected off the whitened covariates and
    resident in HBM (n x ld float64, ld = T rounded up to 16), on the factor, ``dQ``, ``R`` and ``block`` of ``scan`` (an
    ``AssociationScan``); it refuses to run when the scan does (``_check_factor``).  ``scale``: "fixed" or "profile"."""

    def __init__(self, scan, dW, scale):
        """``dW``: n x T device tensor of WHITENED traits in the permuted order of ``scan.dQ`` (consumed)."""
        if not isinstance(scan, assoc.AssociationScan):
            raise _lib.ScilmmError("a phenotype panel needs an AssociationScan on the device engine (panels on an InteractionScan "
                                   "or a VariantSetTest are not supported); there is no CPU form")
        check_scale(scale)
        scan._check_factor()
        torch = scan.torch
        self.scan, self.n, self.scale = scan, scan.n, scale
        self.T = T = int(dW.shape[1])
        self.ld = (T + 15) // 16 * 16
        c = scan.c
        dR = torch.from_numpy(np.ascontiguousarray(scan.R)).cuda()
        self.dRt = dR.T.contiguous()                                            # lower triangular R'
        Qc = torch.linalg.solve_triangular(dR, scan.dQ[:, :c], upper=True, left=False).contiguous()   # w(C) R^-1: orthonormal columns
        QcT = Qc.T.contiguous()
        # y~ = w - Q_c (Q_c'w), |y~|^2: trait by trait on contiguous vectors, so that every launch has the same shape whatever T
        # is and wherever the trait sits -- a trait's bits do not depend on its panel (one GEMM over the panel would be free to
        # choose its summation order by T)
        dWt = dW.T.contiguous()
        del dW
        s_t = torch.empty((T,), dtype=torch.float64, device="cuda")
        for k in range(T):
            w = dWt[k]
            w.sub_(torch.mv(Qc, torch.mv(QcT, w)))
            s_t[k] = torch.dot(w, w)
        self.dY = torch.zeros((self.n, self.ld), dtype=torch.float64, device="cuda")
        self.dY[:, :T] = dWt.T
        self.s_t = s_t.cpu().numpy() / (self.n - c)                             # |y~_t|^2 / (n - c)
        torch.cuda.synchronize()

    @classmethod
    def from_traits(cls, scan, Y, scale="fixed"):
        check_scale(scale)
        Y = check_traits(Y, scan.n)
        scan._check_factor()
        torch, fac = scan.torch, scan.factor
        perm = torch.from_numpy(fac.P()).cuda()
        dB = torch.from_numpy(Y).cuda()[perm].contiguous()
        dW = torch.empty_like(dB)
        torch.cuda.synchronize()
        fac.solve_L_dev(vp(dB.data_ptr()), Y.shape[1], vp(dW.data_ptr()))       # (loops over 128-column blocks)
        scan.sym.sync()
        return cls(scan, dW, scale)

    @classmethod
    def null(cls, scan, n_rep=1000, seed=0):
        n_rep, seed = check_n_rep(n_rep), check_seed(seed)
        torch = scan.torch
        gen = torch.Generator(device="cuda").manual_seed(seed)
        return cls(scan, torch.randn((scan.n, n_rep), generator=gen, dtype=torch.float64, device="cuda"), "fixed")

    def _run(self, src, rows, chunk_bytes, reduce):
        check_reduce(reduce)
        scan = self.scan
        scan._check_factor()
        m = rows.stop - rows.start if isinstance(rows, slice) else rows.size
        follow = _Products(self, m, reduce)
        S = scan._stats(src, rows, chunk_bytes, follow=follow, rows_max=max(1, _PANEL_BYTES // (8 * self.T)))
        if reduce is None:
            return panel_stats(S, follow.B, scan.R, self.n, self.scale, self.s_t)
        mx, arg = follow.best.cpu().numpy(), follow.arg.cpu().numpy()
        if follow.n_tested == 0:
            mx = np.full(self.T, np.nan)
        elif self.scale == "profile":
            mx = mx / self.s_t
        return {"max_chi2": mx, "argmax": arg, "n_tested": follow.n_tested}

    def __call__(self, genotypes, reduce=None):
        """``genotypes`` as for ``AssociationScan.__call__`` (m x n int8).  Returns a dict: ``beta``, ``se``, ``chi2``, ``p`` of
        shape (m, T), ``n_obs`` and ``mean`` of length m, with ``scale="profile"`` also ``scale`` (T); a marker without an
        observed value or without variation is NaN across its row.  For ``Y = y[:, None]`` and ``scale="fixed"`` this is the
        scan's result to rounding.  THE (m, T) ARRAYS ARE LARGE -- 4 x 8 m T bytes on the host: callers slice the markers (or
        the traits) so that they fit, or ask for ``reduce="max"``: then nothing of size m x T leaves the device, chi2 is
        formed per chunk on the device and only ``max_chi2`` (T: the maximum over the non-degenerate markers; NaN when there is
        none), ``argmax`` (T int64: the marker's index, -1 when there is none) and ``n_tested`` come back."""
        g = assoc.check_genotypes(genotypes, self.n)
        check_reduce(reduce)
        return self._run(Int8Rows(self.scan, g), slice(0, g.shape[0]), assoc._CHUNK_BYTES, reduce)

    def scan_bed(self, bed, sample_index=None, markers=None, count="A1", chunk_bytes=None, reduce=None):
        """``__call__`` on the markers of a PLINK 1 fileset; the arguments of ``AssociationScan.scan_bed``.  ``argmax`` counts
        along ``markers``.  Bit for bit what ``__call__`` returns for the unpacked, gathered markers in deterministic mode."""
        from .bed import marker_indices
        check_reduce(reduce)
        src = self.scan._bed_source(bed, sample_index, count)
        rows = marker_indices(markers, src.m)
        return self._run(src, as_run(rows), int(assoc._CHUNK_BYTES if chunk_bytes is None else chunk_bytes), reduce)

    def scan_dosages(self, dosages, sample_index=None, chunk_bytes=None, reduce=None):
        """``__call__`` on imputed dosages; the arguments of ``AssociationScan.scan_dosages``."""
        check_reduce(reduce)
        src = self.scan._dosage_source(dosages, sample_index)
        chunk_bytes = int(assoc._CHUNK_BYTES if chunk_bytes is None else chunk_bytes)
        if chunk_bytes < 1:
            raise ValueError("chunk_bytes must be positive")
        return self._run(src, slice(0, src.m), chunk_bytes, reduce)
