"""Variant-set tests over phenotype panels: burden, SKAT and SKAT-O of marker sets against T quantitative traits under one V.

The whitened markers ``X = w(G~)`` of a Gram block do not depend on the phenotype, and neither does anything the variant-set
finish does with ``K = X'X - Z'Z``: the projection, ``A = diag(w) K diag(w)``, its eigendecomposition, the spectra of every
``A R_rho`` and of the remainder term, the Liu moments.  Only the score ``s_t = X'y~_t`` changes with the trait -- one column of the
``B = X'Y~`` that ``scilmm_scan_panel_dev`` forms behind any block for traits projected off the whitened covariates (so there is
no ``u``: ``s = B[:, t]`` as it stands)::

    panel = tester.set_traits(Y, scale="fixed")          # tester: a VariantSetTest; Y: n x T float64, finite, 1 <= T <= 4096
    out = panel(genotypes, sets, weights="beta", method="saddlepoint", skato=False, rho=None, finish="device")
    out = panel.test_bed("cohort", sets, sample_index=idx)          # also panel.test_dosages(ds, sets, sample_index=idx)

One forward sweep, one Gram pass, one ``X'Y~`` and one finish per block of sets, whatever T is.  ``finish="device"`` queues
``scilmm_sets_finish_panel_dev`` behind them: a set's spectra once (``k_sets_spectra``), then a tail per (set, trait)
(``k_sets_panel_tail``); 4 doubles per set and 8 per (set, trait) come back.  ``finish="host"`` is the reference path: the
statistics, the Gram matrix and ``B`` come back, one ``eigvalsh`` of ``A`` and one ``skato_spectra`` per set, then the host tails
of ``scilmm_amd.sets`` per trait.  The two agree as ``VariantSetTest``'s finishes do (1e-6 relative on p-values).

``scale`` is ``TraitPanel``'s: "fixed" takes V as given; "profile" profiles the overall scale per trait, ``s_t = |y~_t|^2 / (n - c)``
divides ``burden_chi2`` and ``skat_q`` (and with it goes into every p-value) and multiplies ``burden_se^2``.

Out of scope: binary traits (V depends on the trait), sets wider than one block (``max_markers``), ``return_kernel``, null panels
and any ``reduce=``, per-trait missing phenotypes, distributed handles and fp32 fronts.  There is no CPU form of the device side;
the host algebra (``host_set``) and the argument checks are pure NumPy / SciPy.
"""
import ctypes as C

import numpy as np
import scipy.linalg as la

from . import _lib
from . import sets as S
from .assoc import check_genotypes
from .markers import Int8Rows
from .panel import TraitPanel, check_scale

KEYS = S.KEYS                        # n_used is (n_sets,), the others (n_sets, T)
SKATO_KEYS = S.SKATO_KEYS[:3]        # (n_sets, T) each; there is no per-rho array
HEAD, ROW = 4, 8                     # doubles of a set's head row and of a (set, trait) row of scilmm_sets_finish_panel_dev
REFUSED = ("return_kernel", "max_markers")
vp = C.c_void_p


def check_finish(finish):
    if finish not in S.FINISHES:
        raise ValueError("finish must be one of %s, got %r" % (", ".join(S.FINISHES), finish))
    return finish


def check_keywords(extra):
    """The keywords of ``VariantSetTest`` a set panel does not take (``return_kernel``, ``max_markers``) and unknown ones: ValueError
    for the first, TypeError for the second, before anything else is looked at."""
    for k in extra:
        if k in REFUSED:
            raise ValueError("%s is not supported by a set panel (K stays on the device; a set holds at most one block)" % k)
    if extra:
        raise TypeError("unexpected keyword argument %r" % sorted(extra)[0])


def check_scales(s_t):
    """The per-trait scales of ``scale="profile"``: finite and positive (a trait in the span of the covariates has none)."""
    s_t = np.asarray(s_t, dtype=np.float64)
    if s_t.ndim != 1 or not np.all(np.isfinite(s_t) & (s_t > 0)):
        raise ValueError("scale='profile' needs a finite positive scale per trait: a trait that the covariates explain exactly has none")
    return s_t


def new_out(ns, T, skato, s_t=None):
    """The dict a set panel returns, empty: ``n_used`` zeros (n_sets), NaN (n_sets, T) for the other keys, ``scale`` a copy of ``s_t``."""
    out = {k: np.full((ns, T), np.nan) for k in KEYS[1:]}
    out["n_used"] = np.zeros(ns, dtype=np.int64)
    if skato:
        out.update({k: np.full((ns, T), np.nan) for k in SKATO_KEYS})
    if s_t is not None:
        out["scale"] = np.array(s_t, dtype=np.float64)
    return out


def host_set(out, i, St, G, B, R, weights, sf, f, rho=None, method="saddlepoint", s_t=None):
    """The host algebra of set ``i`` against every trait, into row ``i`` of ``out``: ``St`` its columns of a block's statistics
    ((c + 5) x m), ``G`` its sub-block of X'X, ``B`` its rows of X'Y~ (m x T), ``R`` the model's; ``sf`` the mixtures' tail, ``f``
    the burden's null law (``.sf``), ``rho`` the SKAT-O grid or None, ``s_t`` the T scales or None (all 1).  For a trait at scale
    1 this is ``VariantSetTest._one_set`` on the set with ``B[:, t]`` for its score row and ``u = 0``, expression by expression;
    what does not depend on the trait -- ``K``, ``A``, its eigenvalues, ``skato_spectra`` -- is computed once.  Pure NumPy / SciPy."""
    c = R.shape[0]
    _, K, w, keep = S.set_kernel(St, G, R, np.zeros(c), weights)
    out["n_used"][i] = k = int(keep.sum())
    if not k:
        return
    wKw = float(w.dot(K.dot(w)))
    A = w[:, None] * K * w[None, :]
    lam = la.eigvalsh(A)
    live = bool(lam.size and lam.max() > 0)
    lamf = lam[lam > S.LAMBDA_FLOOR * lam.max()] if live else None
    spectra = S.skato_spectra(A, rho) if live and rho is not None else None
    for t in range(B.shape[1]):
        sc = 1.0 if s_t is None else float(s_t[t])
        s0 = B[keep, t]
        s = s0 / np.sqrt(sc)
        ws0, ws = float(w.dot(s0)), float(w.dot(s))
        with np.errstate(divide="ignore", invalid="ignore"):
            out["burden_beta"][i, t] = ws0 / wKw
            out["burden_se"][i, t] = np.sqrt(sc) / np.sqrt(wKw)
            out["burden_chi2"][i, t] = chi2 = ws * ws / wKw
        out["burden_p"][i, t] = f.sf(chi2)
        out["skat_q"][i, t] = qs = float(np.sum(w * w * s * s))
        if live:
            out["skat_p"][i, t] = sf(qs, lamf)
            if rho is not None:
                out["skato_p"][i, t], out["skato_pmin"][i, t], out["skato_rho"][i, t], _ = S.skato_pvalue(w * s, A, rho, method, spectra)


def device_rows(out, members, head, rows, s_t=None):
    """The rows of ``scilmm_sets_finish_panel_dev`` of one block (``head``: n x 4, ``rows``: n x T x 8) into the rows ``members`` of
    ``out``; ``burden_p`` is left to the caller.  ``burden_beta = 1'(w o s) / w'Kw`` and ``burden_se = sqrt(s_t / w'Kw)``."""
    out["n_used"][members] = head[:, 0].astype(np.int64)
    wKw = head[:, 1][:, None]
    sc = 1.0 if s_t is None else np.asarray(s_t)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        out["burden_beta"][members] = rows[:, :, 0] / wKw
        out["burden_se"][members] = np.sqrt(sc) / np.sqrt(wKw) * np.ones_like(rows[:, :, 0])
    for col, k in ((1, "burden_chi2"), (2, "skat_q"), (3, "skat_p")):
        out[k][members] = rows[:, :, col]
    if "skato_p" in out:
        for col, k in ((4, "skato_p"), (5, "skato_pmin"), (6, "skato_rho")):
            out[k][members] = rows[:, :, col]


class SetTraitPanel(object):
    """``tester.set_traits(Y, scale)``: the T phenotype columns of a ``TraitPanel`` on the tester's factor and whitening, and the
    variant-set tests of the tester against every one of them.  It refuses to run when the tester does (``_check_factor``)."""

    def __init__(self, tester, Y, scale="fixed"):
        if type(tester) is not S.VariantSetTest:
            raise _lib.ScilmmError("a set panel needs a VariantSetTest (binary traits are out of scope: V depends on the trait), got %s"
                                   % type(tester).__name__)
        check_scale(scale)
        self.tester, self.scale = tester, scale
        self.panel = TraitPanel.from_traits(tester, Y, scale)          # (check_traits first: nothing of a device before it)
        self.T = self.panel.T
        self.s_t = check_scales(self.panel.s_t) if scale == "profile" else None

    def __call__(self, genotypes, sets, weights="beta", method="saddlepoint", skato=False, rho=None, finish="device", **extra):
        """``genotypes``, ``sets``, ``weights``, ``method``, ``skato``, ``rho``: as for ``VariantSetTest.__call__``; ``finish``:
        "device" or "host".  Returns a dict: ``n_used`` (n_sets, int64); ``burden_beta``, ``burden_se``, ``burden_chi2``,
        ``burden_p``, ``skat_q``, ``skat_p`` of shape (n_sets, T); with ``skato`` also ``skato_p``, ``skato_pmin``, ``skato_rho``
        (n_sets, T); with ``scale="profile"`` also ``scale`` (T).  A set with nothing left is NaN across its row.  For
        ``Y = y[:, None]`` and ``scale="fixed"`` this is ``tester(genotypes, sets, ...)`` to rounding.  ``return_kernel``,
        ``max_markers`` and a set wider than ``block`` raise before any launch."""
        check_keywords(extra)
        return self._run(Int8Rows(self.tester, check_genotypes(genotypes, self.tester.n)), sets, weights, method, skato, rho, finish)

    def test_bed(self, bed, sets, sample_index=None, count="A1", chunk_bytes=None, weights="beta", method="saddlepoint", skato=False,
                 rho=None, finish="device", **extra):
        """``__call__`` on the markers of a PLINK 1 fileset: the arguments of ``VariantSetTest.test_bed``.  The bits of ``__call__``
        on the unpacked markers in deterministic mode."""
        check_keywords(extra)
        src = self.tester._bed_source(bed, sample_index, count)
        if chunk_bytes is not None and int(chunk_bytes) < 1:
            raise ValueError("chunk_bytes must be positive")
        return self._run(src, sets, weights, method, skato, rho, finish)

    def test_dosages(self, dosages, sets, sample_index=None, weights="beta", method="saddlepoint", skato=False, rho=None,
                     finish="device", **extra):
        """``__call__`` on imputed dosages: the arguments of ``VariantSetTest.test_dosages``.  For uint16 codes of hard calls, the
        bits of ``__call__`` on the int8 markers in deterministic mode."""
        check_keywords(extra)
        return self._run(self.tester._dosage_source(dosages, sample_index), sets, weights, method, skato, rho, finish)

    def _buffers(self, src):
        t = self.tester
        torch, q, blk = t.torch, t.q, t.block
        src.stage(blk)
        dS = torch.empty(((q + 4) * blk,), dtype=torch.float64, device="cuda")
        dK = torch.empty((blk * blk,), dtype=torch.float64, device="cuda")
        dB = torch.empty((blk * self.T,), dtype=torch.float64, device="cuda")
        return dS, dK, dB

    def _block_host(self, src):
        """rows -> (statistics, Gram matrix, X'Y~) of one block, on the host: the form's Gram entry point and ``scan_panel_dev``
        behind it, one wait, three copies."""
        t, p, T = self.tester, self.panel, self.T
        dS, dK, dB = self._buffers(src)

        def run(rows):
            rb, q = rows.size, t.q
            src.load(rows)
            src.enqueue(0, rb, vp(dS.data_ptr()), vp(dK.data_ptr()))
            t.factor.scan_panel_dev(rb, vp(p.dY.data_ptr()), p.ld, T, vp(dB.data_ptr()), T)
            t.sym.sync()
            return (dS[:(q + 4) * rb].cpu().numpy().reshape(q + 4, rb), dK[:rb * rb].cpu().numpy().reshape(rb, rb),
                    dB[:rb * T].cpu().numpy().reshape(rb, T))
        return run

    def _block_device(self, src, mode, method, rho):
        """(rows, offsets, weights) -> (head rows, (set, trait) rows) of one block, on the host: the form's Gram entry point,
        ``scan_panel_dev`` and ``sets_finish_panel_dev`` queued one behind the other, one wait, two copies."""
        t, p, T = self.tester, self.panel, self.T
        torch, blk = t.torch, t.block
        dS, dK, dB = self._buffers(src)
        dR = torch.from_numpy(np.ascontiguousarray(t.R)).cuda()
        dW = torch.empty((blk,), dtype=torch.float64, device="cuda")
        dH = torch.empty((blk * HEAD,), dtype=torch.float64, device="cuda")
        dO = torch.empty((blk * T * ROW,), dtype=torch.float64, device="cuda")
        dscale = torch.from_numpy(np.ascontiguousarray(self.s_t)).cuda() if self.s_t is not None else None
        meth = S.METHODS.index(method)

        def run(rows, start, w):
            rb, ns = rows.size, start.size - 1
            src.load(rows)
            if w is not None:
                dW[:rb].copy_(torch.from_numpy(w))
            src.enqueue(0, rb, vp(dS.data_ptr()), vp(dK.data_ptr()))
            t.factor.scan_panel_dev(rb, vp(p.dY.data_ptr()), p.ld, T, vp(dB.data_ptr()), T)
            t.factor.sets_finish_panel_dev(rb, t.q, vp(dS.data_ptr()), vp(dK.data_ptr()), vp(dR.data_ptr()), t.c, ns, start, mode,
                                           vp(dW.data_ptr()) if w is not None else None, meth, rho, vp(dB.data_ptr()), T, T,
                                           vp(dscale.data_ptr()) if dscale is not None else None, vp(dH.data_ptr()), vp(dO.data_ptr()))
            t.sym.sync()
            return dH[:ns * HEAD].cpu().numpy().reshape(ns, HEAD), dO[:ns * T * ROW].cpu().numpy().reshape(ns, T, ROW)
        return run

    def _run(self, src, sets, weights, method, skato, rho, finish):
        """The checks (before any launch), then block by block as ``VariantSetTest._run`` packs them."""
        t, T = self.tester, self.T
        sets = S.check_sets(sets, src.m, t.block)
        weights, sf = S.check_weights(weights, sets), S.check_method(method)
        check_finish(finish)
        rho = S.check_rho(rho) if skato else None
        t._check_factor()
        ns = len(sets)
        out = new_out(ns, T, skato, self.s_t)
        packed = S.pack_sets([s.size for s in sets], t.block)
        given = not (weights is None or isinstance(weights, str))
        if finish == "device":
            mode = S.WEIGHT_GIVEN if given else S.WEIGHT_ONES if weights is None else S.WEIGHT_BETA
            block = self._block_device(src, mode, method, rho if skato else np.empty(0)) if packed else None
            for members in packed:
                start = np.concatenate([[0], np.cumsum([sets[i].size for i in members])]).astype(np.int32)
                w = np.ascontiguousarray(np.concatenate([weights[i] for i in members])) if given else None
                head, rows = block(np.concatenate([sets[i] for i in members]), start, w)
                device_rows(out, members, head, rows, self.s_t)
            used = out["n_used"] > 0
            out["burden_p"][used] = t._f.sf(out["burden_chi2"][used])        # (one vectorised call over the sets and the traits)
            return out
        block = self._block_host(src) if packed else None
        for members in packed:
            St, G, B = block(np.concatenate([sets[i] for i in members]))
            a = 0
            for i in members:
                b = a + sets[i].size
                w = weights[i] if given else weights
                host_set(out, i, St[:, a:b], G[a:b, a:b], B[a:b], t.R, w, sf, t._f, rho, method, self.s_t)
                a = b
        return out
