"""Variant-set tests under functional annotation masks crossed with MAF cutoffs, with ACAT-V per cell and ACAT-O per set.

An exome analysis does not test a gene once: SAIGE-GENE+, STAAR and REGENIE test it under several annotation masks (LoF; LoF +
missense; ...) crossed with several cutoffs of the minor allele frequency, and merge the results by a Cauchy combination
(ACAT-O; Liu et al. 2019).  Every (mask, cutoff) cell of a set is a principal submatrix of the set's ``K = G~' P G~`` and a
sub-vector of its score, so the whole grid costs ONE sweep and ONE Gram pass per block of sets::

    masked = tester.masks(annotations, max_maf=(0.01, 0.001, 0.0001), acat_mac=10)     # tester: a VariantSetTest
    out = masked(genotypes, sets, weights="beta", method="saddlepoint", skato=False, rho=None, finish="device",
                 combine=("burden", "skat", "acatv"))
    out = masked.test_bed("cohort", sets, sample_index=idx)          # also masked.test_dosages(ds, sets, sample_index=idx)

Cell (a, f) of a set holds the markers that ``VariantSetTest`` keeps (an observed value, variation) AND that are in annotation a
AND whose ``maf <= max_maf[f]``, ``maf = min(0.5 mean, 1 - 0.5 mean)`` from the block's ``mean`` row (``maf_of``: the expression of
the device's weight mode 0, so membership cannot differ between host and device).  ``finish="device"`` queues
``scilmm_sets_finish_masks_dev`` behind the block's Gram call: one workgroup per cell runs the finish of ``VariantSetTest`` on
the cell's index list (the same routines, the same bits as a call on the cell's markers alone would get from the same Gram
entries) and ACAT-V; ``12 + n_rho`` doubles per cell come back.  ``finish="host"`` is the NumPy / SciPy reference: per cell it
subsets the set's columns of the statistics and of the Gram matrix and runs ``VariantSetTest._one_set`` and ``acatv``.

ACAT-V (``acatv``): a marker with minor allele count ``2 n_obs maf > acat_mac`` gives ``p_j = erfc(sqrt(s_j^2 / 2 K_jj))`` with the
weight ``w_j^2 maf_j (1 - maf_j)``; the rarer ones are pooled into one burden term.  ``acat`` is the Cauchy combination itself.

Out of scope: ``finish="wide"`` and ``max_markers``, binary traits, ``set_traits`` combined with masks,
``return_kernel`` with the device finish.  There is no CPU form of the device side; the host algebra and the argument checks are
pure NumPy / SciPy.
"""
import ctypes as C

import numpy as np
import scipy.special as special

from . import sets as S
from .assoc import check_genotypes
from .markers import Int8Rows

ANN_MAX, CUT_MAX = 32, 8             # annotations and MAF cutoffs at most (scilmm_sets_finish_masks_dev)
ACAT_TINY, ACAT_HUGE = 1e-15, 1e15   # below: 1 / (p pi) for the tangent; above: 1 / (T pi) for the p-value
TAIL = 2                             # doubles of a cell's row behind the row of scilmm_sets_finish_dev: acatv_p | n_pooled
CELL_KEYS = S.KEYS + ("acatv_p", "n_pooled")                 # (n_sets, A, F) each
COMBINE = {"burden": "burden_p", "skat": "skat_p", "acatv": "acatv_p", "skato": "skato_p"}
COMBINE_DEFAULT = ("burden", "skat", "acatv")
REFUSED = {"max_markers": "a cell is finished in LDS: a set holds at most one block",
           "set_traits": "phenotype panels combined with masks are not supported"}
vp = C.c_void_p


def cauchy_term(p):
    """``tan((0.5 - p) pi)`` elementwise, with ``p`` capped at ``1 - 1e-15`` and ``1 / (p pi)`` where ``p < 1e-15`` (infinite at
    0).  Below 0.5 it is evaluated as ``1 / tan(p pi)``: the same function without the cancellation in ``0.5 - p``, which would
    cost a small p its leading digits and the branch at 1e-15 its continuity.  The device's ``fin_cauchy_term`` is this."""
    p = np.minimum(np.asarray(p, dtype=np.float64), 1.0 - ACAT_TINY)
    with np.errstate(divide="ignore", invalid="ignore"):
        low = 1.0 / np.tan(np.where(p < 0.5, p, 0.25) * np.pi)
        return np.where(p < ACAT_TINY, 1.0 / (p * np.pi), np.where(p < 0.5, low, np.tan((0.5 - p) * np.pi)))


def cauchy_sf(T):
    """``0.5 - atan(T) / pi`` elementwise, ``1 / (T pi)`` where ``T > 1e15``; above 1 it is evaluated as ``atan(1 / T) / pi``, the
    same function without the cancellation.  The device's ``fin_cauchy_sf`` is this."""
    T = np.asarray(T, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        big = np.arctan(1.0 / np.where(T > 1.0, T, 2.0)) / np.pi
        return np.where(T > ACAT_HUGE, 1.0 / (T * np.pi), np.where(T > 1.0, big, 0.5 - np.arctan(T) / np.pi))


def acat(p, weights=None, axis=-1):
    """The Cauchy combination (ACAT; Liu et al. 2019) of the p-values ``p`` along ``axis``:
    ``T = sum w tan((0.5 - p) pi) / sum w``, ``p_acat = 0.5 - atan(T) / pi``, with the small-p and large-T branches of
    ``cauchy_term`` and ``cauchy_sf``.  ``weights``: None (equal) or non-negative finite numbers that broadcast against ``p``.
    NaN p-values and terms of weight 0 are skipped; where nothing is left the result is NaN; a term with ``p = 0`` gives 0.
    Callers combine across their own strata with it (``acato_p`` of ``MaskedSetTest`` is ``acat`` over a set's cells)."""
    p = np.asarray(p, dtype=np.float64)
    if np.any((p < 0.0) | (p > 1.0)):                          # (a NaN fails both comparisons)
        raise ValueError("every p-value must lie in [0, 1] or be NaN")
    w = np.ones_like(p) if weights is None else np.broadcast_to(np.asarray(weights, dtype=np.float64), p.shape)
    if not np.all(np.isfinite(w) & (w >= 0.0)):
        raise ValueError("weights must be finite and non-negative")
    live = ~np.isnan(p) & (w > 0.0)
    terms = np.where(live, w, 0.0) * cauchy_term(np.where(live, p, 0.5))
    den = np.sum(np.where(live, w, 0.0), axis=axis)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = cauchy_sf(np.sum(terms, axis=axis) / den)
    return np.where(den > 0.0, out, np.nan)[()]


def maf_of(mean):
    """The minor allele frequency from a block's ``mean`` row: the expression of ``scilmm_sets_finish_dev``'s weight mode 0 and of
    ``fin_maf`` on the device, operation by operation."""
    mean = np.asarray(mean, dtype=np.float64)
    return np.minimum(0.5 * mean, 1.0 - 0.5 * mean)


def acatv(s, K, w, maf, n_obs, acat_mac):
    """ACAT-V of one cell in STAAR's form, ``(p, n_pooled)``: ``s``, ``K``, ``w`` the score, its covariance and the weights of the
    cell's k kept markers (``set_kernel``), ``maf`` and ``n_obs`` theirs.  With ``mac_j = 2 n_obs_j maf_j`` and
    ``omega_j = w_j^2 maf_j (1 - maf_j)``: a marker with ``mac_j > acat_mac`` and ``K_jj > 0`` is a term
    ``p_j = erfc(sqrt(0.5 s_j^2 / K_jj))`` of weight ``omega_j``; the markers with ``mac_j <= acat_mac`` (``n_pooled`` of them) are
    one term ``erfc(sqrt(0.5 (sum w_j s_j)^2 / sum_ij w_i K_ij w_j))`` over the pool, left out where the quadratic form is not
    positive, of weight the mean of the pool's ``omega_j``.  Terms of weight 0 are left out; without a term p is NaN."""
    s, w, maf, n_obs = (np.asarray(v, dtype=np.float64).ravel() for v in (s, w, maf, n_obs))
    K = np.asarray(K, dtype=np.float64).reshape(s.size, s.size)
    mac = 2.0 * n_obs * maf
    om = w * w * maf * (1.0 - maf)
    pool, d = mac <= acat_mac, np.diag(K)
    own = ~pool & (d > 0.0) & (om > 0.0)
    p, wt = list(special.erfc(np.sqrt(0.5 * s[own] ** 2 / d[own]))), list(om[own])
    if pool.any():
        wp = w[pool]
        q, omp = float(wp.dot(K[np.ix_(pool, pool)]).dot(wp)), float(om[pool].sum()) / int(pool.sum())
        if q > 0.0 and omp > 0.0:
            p.append(float(special.erfc(np.sqrt(0.5 * float(wp.dot(s[pool])) ** 2 / q))))
            wt.append(omp)
    return (float(acat(np.array(p), np.array(wt))) if p else np.nan), int(pool.sum())


def check_max_maf(max_maf):
    """The MAF cutoffs as a float64 array, in the order given: 1 .. 8 values in (0, 0.5]."""
    cut = np.atleast_1d(np.asarray(max_maf, dtype=np.float64)).ravel()
    if not 1 <= cut.size <= CUT_MAX:
        raise ValueError("max_maf must hold 1 .. %d cutoffs, got %d" % (CUT_MAX, cut.size))
    if not np.all((cut > 0.0) & (cut <= 0.5)):                # (a NaN fails both comparisons)
        raise ValueError("every max_maf cutoff must lie in (0, 0.5]")
    return cut


def check_acat_mac(acat_mac):
    if isinstance(acat_mac, bool) or not isinstance(acat_mac, (int, float, np.integer, np.floating)):
        raise ValueError("acat_mac must be a number, got %r" % (acat_mac,))
    if not (acat_mac >= 0 and np.isfinite(acat_mac)):
        raise ValueError("acat_mac must be finite and >= 0, got %r" % (acat_mac,))
    return float(acat_mac)


def check_combine(combine, skato):
    """``combine`` as a tuple of distinct names out of burden, skat, acatv, skato (the last with ``skato=True`` only)."""
    names = (combine,) if isinstance(combine, str) else tuple(combine)
    if not names or len(set(names)) != len(names) or any(k not in COMBINE for k in names):
        raise ValueError("combine must name one or more of %s, each once, got %r" % (", ".join(COMBINE), combine))
    if "skato" in names and not skato:
        raise ValueError('combine=("skato", ...) needs skato=True')
    return names


def check_finish(finish, return_kernel):
    if finish == "wide":
        raise ValueError('finish="wide" is not supported under masks: a cell is finished in LDS, a set holds at most one block')
    if finish not in S.FINISHES:
        raise ValueError("finish must be one of %s, got %r" % (", ".join(S.FINISHES), finish))
    if return_kernel and finish != "host":
        raise ValueError('return_kernel=True needs finish="host": the device finish does not bring K back')
    return finish


def check_keywords(extra):
    """``max_markers`` and ``set_traits``: ValueError; an unknown keyword: TypeError; before anything else is looked at."""
    for k in extra:
        if k in REFUSED:
            raise ValueError("%s is not supported under masks (%s)" % (k, REFUSED[k]))
    if extra:
        raise TypeError("unexpected keyword argument %r" % sorted(extra)[0])


def _bool_matrix(a, what):
    a = np.asarray(a)
    if a.ndim != 2 or a.dtype != np.bool_:
        raise ValueError("%s must be a 2-D boolean array, markers x annotations" % what)
    if not 1 <= a.shape[1] <= ANN_MAX:
        raise ValueError("%s has %d annotations: 1 .. %d are supported" % (what, a.shape[1], ANN_MAX))
    return a


def check_annotations(annotations):
    """``annotations`` checked as far as it can be without the sets: ``("global", m x A booleans)`` for a 2-D array, or
    ``("per_set", [k_i x A booleans, ...])`` for a sequence; 1 <= A <= 32, the same A throughout."""
    if isinstance(annotations, np.ndarray) and annotations.dtype != object:
        return "global", _bool_matrix(annotations, "annotations")
    if annotations is None or isinstance(annotations, (str, bytes)) or not hasattr(annotations, "__len__"):
        raise ValueError("annotations must be an m x A boolean array or a sequence of k_i x A boolean arrays aligned with sets")
    per = [_bool_matrix(a, "the annotations of set %d" % i) for i, a in enumerate(annotations)]
    if not per or any(a.shape[1] != per[0].shape[1] for a in per):
        raise ValueError("the per-set annotations must be non-empty and agree in their number of annotations")
    return "per_set", per


def pack_words(B):
    """k x A booleans -> k uint32 words, bit a of word j = ``B[j, a]`` (what ``scilmm_sets_finish_masks_dev`` takes)."""
    B = np.asarray(B, dtype=np.bool_)
    bits = B.astype(np.uint32) << np.arange(B.shape[1], dtype=np.uint32)[None, :]
    return np.bitwise_or.reduce(bits, axis=1, initial=np.uint32(0)).astype(np.uint32)


def set_words(form, ann, sets, m):
    """The annotation words of every set, a list of uint32 arrays aligned with ``sets`` (checked index arrays into ``m`` markers)."""
    if form == "global":
        if ann.shape[0] != m:
            raise ValueError("annotations has %d rows for %d markers" % (ann.shape[0], m))
        words = pack_words(ann)
        return [words[s] for s in sets]
    if len(ann) != len(sets):
        raise ValueError("%d annotation arrays for %d sets" % (len(ann), len(sets)))
    for i, (a, s) in enumerate(zip(ann, sets)):
        if a.shape[0] != s.size:
            raise ValueError("the annotations of set %d have %d rows for %d markers" % (i, a.shape[0], s.size))
    return [pack_words(a) for a in ann]


def cell_members(St, words, a, cut):
    """The columns of a set that cell (a, ``cut``) holds, as booleans: ``St`` the set's columns of a block's statistics (rows
    n_obs, mean, css first), ``words`` its annotation words.  Kept AND bit a AND ``maf_of(mean) <= cut`` (a marker AT the cutoff
    is in)."""
    n_obs, mean, css = St[0], St[1], St[2]
    keep = ~((n_obs == 0) | (css == 0))
    return keep & ((np.asarray(words, dtype=np.uint32) >> np.uint32(a)) & np.uint32(1)).astype(bool) & (maf_of(mean) <= cut)


def new_out(ns, A, F, rho=None):
    """The dict a masked tester returns, empty: counts zero, NaN elsewhere."""
    out = {k: np.full((ns, A, F), np.nan) for k in CELL_KEYS}
    out["n_used"] = np.zeros((ns, A, F), dtype=np.int64)
    out["n_pooled"] = np.zeros((ns, A, F), dtype=np.int64)
    if rho is not None:
        out.update({k: np.full((ns, A, F), np.nan) for k in S.SKATO_KEYS[:3]})
        out["skato_p_rho"] = np.full((ns, A, F, rho.size), np.nan)
    out["acato_p"] = np.full(ns, np.nan)
    out["cells_used"] = np.zeros(ns, dtype=np.int64)
    return out


def combine_cells(out, names):
    """``acato_p`` and ``cells_used`` of ``out`` from its cells: the equal-weight Cauchy combination of the p-values ``names`` over
    every non-empty cell of a set, one vectorised ``acat`` over the sets."""
    ns = out["n_used"].shape[0]
    live = out["n_used"] > 0
    P = np.stack([np.where(live, out[COMBINE[k]], np.nan) for k in names], axis=1).reshape(ns, -1)
    out["acato_p"][:] = acat(P, axis=1) if ns else np.empty(0)
    out["cells_used"][:] = live.reshape(ns, -1).sum(axis=1)


class MaskedSetTest(object):
    """``tester.masks(annotations, max_maf, acat_mac)``: the variant-set tests of a ``VariantSetTest`` under A annotation masks
    crossed with F MAF cutoffs, on the tester's factor and whitening.  It refuses to run when the tester does
    (``_check_factor``)."""

    def __init__(self, tester, annotations, max_maf=(0.01, 0.001, 0.0001), acat_mac=10):
        if type(tester) is not S.VariantSetTest:
            raise ValueError("masks need a VariantSetTest (binary traits and phenotype panels -- set_traits -- are not supported "
                             "under masks), got %s" % type(tester).__name__)
        self.tester = tester
        self.form, self.ann = check_annotations(annotations)
        self.A = (self.ann if self.form == "global" else self.ann[0]).shape[1]
        self.cut = check_max_maf(max_maf)
        self.F = self.cut.size
        self.acat_mac = check_acat_mac(acat_mac)

    def set_traits(self, *args, **kwargs):
        raise ValueError("set_traits combined with masks is not supported")

    def __call__(self, genotypes, sets, weights="beta", method="saddlepoint", skato=False, rho=None, finish="device",
                 combine=COMBINE_DEFAULT, return_kernel=False, **extra):
        """``genotypes``, ``sets``, ``weights``, ``method``, ``skato``, ``rho``: as for ``VariantSetTest.__call__`` (a set holds at
        most ``block`` markers; the sets are packed by ``pack_sets`` exactly as there); ``finish``: "device" or "host".  Returns
        a dict: ``n_used``, ``burden_beta``, ``burden_se``, ``burden_chi2``, ``burden_p``, ``skat_q``, ``skat_p``, ``acatv_p``,
        ``n_pooled`` of shape (n_sets, A, F) (the counts int64); with ``skato`` also ``skato_p``, ``skato_pmin``, ``skato_rho``
        (n_sets, A, F) and ``skato_p_rho`` (n_sets, A, F, n_rho); and ``acato_p``, ``cells_used`` of shape (n_sets,).  An empty
        cell has ``n_used = n_pooled = 0`` and NaN elsewhere.

        ``acato_p`` is the equal-weight Cauchy combination (``acat``) of the p-values named in ``combine`` ("burden", "skat",
        "acatv", and "skato" with ``skato=True``) over the set's ``cells_used`` non-empty cells; NaN p-values are skipped.  Two
        cells that hold the same markers -- a cutoff that removes nothing, nested annotations that add nothing -- are counted as
        often as they occur, as SAIGE-GENE+ counts them: the combination stays valid under any dependence, and deduplication
        would make a set's p-value depend on which of its masks happen to coincide.

        ``finish="host"`` is the NumPy / SciPy reference and may return ``kernel`` (``return_kernel=True``): per set a list of
        ``(s, K, w)`` per cell in the order ``a * F + f``, None for an empty cell.  ``finish="wide"``, ``max_markers``,
        ``set_traits`` and ``return_kernel`` with the device finish raise ValueError before any launch."""
        check_keywords(extra)
        return self._run(Int8Rows(self.tester, check_genotypes(genotypes, self.tester.n)), sets, weights, method, skato, rho, finish,
                         combine, return_kernel)

    def test_bed(self, bed, sets, sample_index=None, count="A1", chunk_bytes=None, weights="beta", method="saddlepoint", skato=False,
                 rho=None, finish="device", combine=COMBINE_DEFAULT, return_kernel=False, **extra):
        """``__call__`` on the markers of a PLINK 1 fileset: the arguments of ``VariantSetTest.test_bed``.  The bits of ``__call__``
        on the unpacked markers in deterministic mode."""
        check_keywords(extra)
        src = self.tester._bed_source(bed, sample_index, count)
        if chunk_bytes is not None and int(chunk_bytes) < 1:
            raise ValueError("chunk_bytes must be positive")
        return self._run(src, sets, weights, method, skato, rho, finish, combine, return_kernel)

    def test_dosages(self, dosages, sets, sample_index=None, weights="beta", method="saddlepoint", skato=False, rho=None,
                     finish="device", combine=COMBINE_DEFAULT, return_kernel=False, **extra):
        """``__call__`` on imputed dosages: the arguments of ``VariantSetTest.test_dosages``.  For uint16 codes of hard calls, the
        bits of ``__call__`` on the int8 markers in deterministic mode."""
        check_keywords(extra)
        return self._run(self.tester._dosage_source(dosages, sample_index), sets, weights, method, skato, rho, finish, combine,
                         return_kernel)

    def _block_device(self, src, mode, method, rho):
        """(rows, offsets, weights, annotation words) -> the block's rows of ``scilmm_sets_finish_masks_dev`` (n_sets x A x F x
        (12 + n_rho)), on the host: the form's Gram entry point, the upload of the words and the finish one behind the other,
        one wait, one device-to-host copy."""
        t, A, F = self.tester, self.A, self.F
        torch, q, blk = t.torch, t.q, t.block
        src.stage(blk)
        dS = torch.empty(((q + 4) * blk,), dtype=torch.float64, device="cuda")
        dK = torch.empty((blk * blk,), dtype=torch.float64, device="cuda")
        dR = torch.from_numpy(np.ascontiguousarray(t.R)).cuda()
        du = torch.from_numpy(np.ascontiguousarray(t.u)).cuda()
        dW = torch.empty((blk,), dtype=torch.float64, device="cuda")
        dA = torch.empty((blk,), dtype=torch.int32, device="cuda")              # (the uint32 words, bit for bit)
        ld = S.FINISH_HEAD + rho.size + TAIL
        dO = torch.empty((blk * A * F * ld,), dtype=torch.float64, device="cuda")
        meth = S.METHODS.index(method)

        def run(rows, start, w, words):
            rb, ns = rows.size, start.size - 1
            src.load(rows)
            if w is not None:
                dW[:rb].copy_(torch.from_numpy(w))
            src.enqueue(0, rb, vp(dS.data_ptr()), vp(dK.data_ptr()))
            dA[:rb].copy_(torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)))
            t.factor.sets_finish_masks_dev(rb, q, vp(dS.data_ptr()), vp(dK.data_ptr()), vp(dR.data_ptr()), vp(du.data_ptr()), t.c, ns,
                                           start, mode, vp(dW.data_ptr()) if w is not None else None, meth, rho, vp(dA.data_ptr()), A,
                                           self.cut, self.acat_mac, vp(dO.data_ptr()), ld)
            t.sym.sync()
            return dO[:ns * A * F * ld].cpu().numpy().reshape(ns, A, F, ld)
        return run

    def _host_set(self, out, i, St, G, words, weights, sf, rho, method):
        """The host algebra of set ``i``, cell by cell: the cell's columns of the set's statistics and of its sub-block of X'X
        through ``VariantSetTest._one_set``, then ``acatv``; returns the list of the cells' (s, K, w)."""
        t, kernel = self.tester, []
        for a in range(self.A):
            for f in range(self.F):
                cols = np.flatnonzero(cell_members(St, words, a, self.cut[f]))
                if not cols.size:
                    kernel.append(None)
                    continue
                one = {k: np.full(1, np.nan) for k in S.KEYS + S.SKATO_KEYS[:3]}
                one["n_used"] = np.zeros(1, dtype=np.int64)
                one["skato_p_rho"] = np.full((1, 0 if rho is None else rho.size), np.nan)
                w = weights if weights is None or isinstance(weights, str) else weights[cols]
                s, K, wk = t._one_set(one, 0, St[:, cols], G[np.ix_(cols, cols)], w, sf, rho, method)
                for k in S.KEYS + (S.SKATO_KEYS if rho is not None else ()):
                    out[k][i, a, f] = one[k][0]
                out["acatv_p"][i, a, f], out["n_pooled"][i, a, f] = acatv(s, K, wk, maf_of(St[1, cols]), St[0, cols], self.acat_mac)
                kernel.append((s, K, wk))
        return kernel

    def _run(self, src, sets, weights, method, skato, rho, finish, combine, return_kernel):
        """The checks (before any launch), then block by block as ``VariantSetTest._run`` packs them."""
        t, A, F = self.tester, self.A, self.F
        sets = S.check_sets(sets, src.m, t.block)
        weights, sf = S.check_weights(weights, sets), S.check_method(method)
        check_finish(finish, return_kernel)
        names = check_combine(combine, skato)
        rho = S.check_rho(rho) if skato else None
        words = set_words(self.form, self.ann, sets, src.m)
        t._check_factor()
        ns = len(sets)
        out = new_out(ns, A, F, rho)
        packed = S.pack_sets([s.size for s in sets], t.block)
        given = not (weights is None or isinstance(weights, str))
        if finish == "device":
            mode = S.WEIGHT_GIVEN if given else S.WEIGHT_ONES if weights is None else S.WEIGHT_BETA
            block = self._block_device(src, mode, method, rho if skato else np.empty(0)) if packed else None
            for members in packed:
                start = np.concatenate([[0], np.cumsum([sets[i].size for i in members])]).astype(np.int32)
                w = np.ascontiguousarray(np.concatenate([weights[i] for i in members])) if given else None
                O = block(np.concatenate([sets[i] for i in members]), start, w, np.concatenate([words[i] for i in members]))
                out["n_used"][members] = O[..., 0].astype(np.int64)
                for col, k in ((1, "burden_beta"), (2, "burden_se"), (3, "burden_chi2"), (4, "skat_q"), (5, "skat_p")):
                    out[k][members] = O[..., col]
                n_rho = rho.size if skato else 0
                if skato:
                    for col, k in ((6, "skato_p"), (7, "skato_pmin"), (8, "skato_rho")):
                        out[k][members] = O[..., col]
                    out["skato_p_rho"][members] = O[..., S.FINISH_HEAD:S.FINISH_HEAD + n_rho]
                out["acatv_p"][members] = O[..., S.FINISH_HEAD + n_rho]
                out["n_pooled"][members] = O[..., S.FINISH_HEAD + n_rho + 1].astype(np.int64)
            used = out["n_used"] > 0
            out["burden_p"][used] = t._f.sf(out["burden_chi2"][used])        # (one vectorised call over the cells)
            combine_cells(out, names)
            return out
        block = t._block(src) if packed else None
        kernel = [None] * ns
        for members in packed:
            St, G = block(np.concatenate([sets[i] for i in members]))
            a = 0
            for i in members:
                b = a + sets[i].size
                w = weights[i] if given else weights
                kernel[i] = self._host_set(out, i, St[:, a:b], G[a:b, a:b], words[i], w, sf, rho, method)
                a = b
        combine_cells(out, names)
        if return_kernel:
            out["kernel"] = kernel
        return out
