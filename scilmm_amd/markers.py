"""Marker sources: what the marker scan (``scilmm_amd.assoc``) and the variant-set tests (``scilmm_amd.sets``) know about an
input form.  A source has ``m`` (its markers), ``row_bytes`` (host bytes of one marker row: what a chunk is sized by) and

    stage(rows_max)            allocate the staging and device buffers for up to ``rows_max`` rows (once per scan)
    load(rows)                 bring marker rows -- a slice or an index array -- to device rows 0 .. k-1 and wait for them
    enqueue(k0, rb, pS, pK)    queue block (k0, rb) of the loaded rows: statistics to ``pS``; with ``pK`` the Gram matrix as well
                               (the ``_gram_dev`` twin of the form's entry point); with ``env=(pE, m)`` the marker x environment
                               block of ``m`` environment columns at ``pE`` (the ``_gxe_dev`` twin)
    spa(k0, rb, tail)          queue the saddlepoint p-values of block (k0, rb) behind its plain block (the ``scilmm_scan_spa*_dev``
                               twin; ``tail``: what follows ``r`` in its arguments -- ``scilmm_amd.glmm``)
    sets_spa(k0, rb, tail)     queue the sets' variance scales and burden saddlepoint rows of block (k0, rb) behind its Gram block
                               and its ``spa`` (the ``scilmm_sets_spa*_dev`` twin -- ``scilmm_amd.binary_sets``)
    collapse(k0, rb, tail)     queue the collapsed genotype of a wide set behind the Gram block of sub-block (k0, rb) (the
                               ``scilmm_sets_collapse*_dev`` twin; ``tail``: statistics, weight mode, weights, first, the row)

Everything else -- chunks, blocks, the synchronisation, the host algebra -- is the callers' and does not depend on the form.
"""
import ctypes as C
import time

import numpy as np

vp = C.c_void_p


def as_run(rows):
    """The index array ``rows`` as a slice where the markers are consecutive: a run is taken as one slab, without a gather."""
    return slice(int(rows[0]), int(rows[0]) + rows.size) if rows.size > 1 and bool(np.all(np.diff(rows) == 1)) else rows


class MarkerSource(object):
    """What the forms share.  The constructor keeps the checked input and reads nothing of the model but ``n`` (the argument
    checks run before the model's device side is looked at); ``stage`` puts the sample map ``idx`` (None = identity) on the
    device, and a block is queued with the model's factor and whitened ``Q``."""

    def __init__(self, model, m, row_bytes, idx=None):
        self.model, self.n, self.m, self.row_bytes, self.idx = model, model.n, m, row_bytes, idx
        self.dI = None

    def stage(self, rows_max):
        self.torch = self.model.torch
        if self.idx is not None:
            self.dI = self.torch.from_numpy(self.idx).cuda()

    def _map(self):
        return None if self.dI is None else vp(self.dI.data_ptr())

    def _call(self, plain, gram, gxe, head, rb, pS, pK, env):
        """Queue one block through the form's entry point (``plain``), with ``pK`` its Gram twin, or with ``env`` its gxe twin:
        ``head`` are the form's own leading arguments, the rest is the same for every form."""
        tail = (vp(self.model.dQ.data_ptr()), self.model.q, pS)
        if env is not None:
            gxe(*(head + (rb,) + tuple(env) + tail))
        elif pK is None:
            plain(*(head + (rb,) + tail))
        else:
            gram(*(head + (rb,) + tail + (pK,)))


class Int8Rows(MarkerSource):
    """m x n int8 allele counts (``check_genotypes``): a direct copy from the array into device rows that start on 16-byte
    boundaries, so every read is an aligned one."""

    def __init__(self, model, g):
        self.g, self.ld = g, (model.n + 15) // 16 * 16
        super(Int8Rows, self).__init__(model, g.shape[0], self.ld)

    def stage(self, rows_max):
        super(Int8Rows, self).stage(rows_max)
        self.dG = self.torch.empty((rows_max, self.ld), dtype=self.torch.int8, device="cuda")

    def load(self, rows):
        g = np.ascontiguousarray(self.g[rows])
        self.dG[:g.shape[0], :self.n].copy_(self.torch.from_numpy(g))
        self.torch.cuda.synchronize()

    def enqueue(self, k0, rb, pS, pK=None, env=None):
        f = self.model.factor
        self._call(f.scan_block_dev, f.scan_block_gram_dev, f.scan_block_gxe_dev, self._head(k0), rb, pS, pK, env)

    def _head(self, k0):
        return (vp(self.dG.data_ptr() + k0 * self.ld), self.ld)

    def spa(self, k0, rb, tail):
        self.model.factor.scan_spa_dev(*(self._head(k0) + (rb,) + tuple(tail)))

    def sets_spa(self, k0, rb, tail):
        self.model.factor.sets_spa_dev(*(self._head(k0) + (rb,) + tuple(tail)))

    def collapse(self, k0, rb, tail):
        self.model.factor.sets_collapse_dev(*(self._head(k0) + (rb,) + tuple(tail)))


class BedRows(MarkerSource):
    """The packed rows of a ``BedFile``, decoded on the device: mapped file -> pinned buffer (the one host pass over the bytes)
    -> device in one copy; the rows keep the file's pitch.  ``t_read`` / ``t_copy``: seconds spent in the two, ``t0``: when the
    buffers stood."""

    def __init__(self, model, bed, idx, flag):
        self.bed, self.flag = bed, flag
        super(BedRows, self).__init__(model, bed.n_markers, bed.row_bytes, idx)
        self.t_read = self.t_copy = 0.0
        self.t0 = time.perf_counter()

    def stage(self, rows_max):
        super(BedRows, self).stage(rows_max)
        cap = (rows_max * self.row_bytes + 15) // 16 * 16
        self.hB = self.torch.empty((cap,), dtype=self.torch.uint8).pin_memory()
        self.dB = self.torch.empty((cap,), dtype=self.torch.uint8, device="cuda")
        self.t0 = time.perf_counter()

    def load(self, rows):
        nb = self.row_bytes
        t1 = time.perf_counter()
        packed = self.bed.packed[rows]
        k = packed.shape[0]
        np.copyto(self.hB.numpy()[:k * nb].reshape(k, nb), packed)
        t2 = time.perf_counter()
        self.dB[:k * nb].copy_(self.hB[:k * nb], non_blocking=True)
        self.torch.cuda.synchronize()
        self.t_read, self.t_copy = self.t_read + t2 - t1, self.t_copy + time.perf_counter() - t2

    def enqueue(self, k0, rb, pS, pK=None, env=None):
        f = self.model.factor
        self._call(f.scan_block_bed_dev, f.scan_block_bed_gram_dev, f.scan_block_bed_gxe_dev, self._head(k0), rb, pS, pK, env)

    def _head(self, k0):
        nb = self.row_bytes
        return (vp(self.dB.data_ptr() + k0 * nb), nb, self.bed.n_samples, self._map(), self.flag)

    def spa(self, k0, rb, tail):
        self.model.factor.scan_spa_bed_dev(*(self._head(k0) + (rb,) + tuple(tail)))

    def sets_spa(self, k0, rb, tail):
        self.model.factor.sets_spa_bed_dev(*(self._head(k0) + (rb,) + tuple(tail)))

    def collapse(self, k0, rb, tail):
        self.model.factor.sets_collapse_bed_dev(*(self._head(k0) + (rb,) + tuple(tail)))


class DosageRows(MarkerSource):
    """m x N dosages (``check_dosages``; ``dtype``: the element type of the C entry point): host array -> pinned buffer (the one
    host pass over the bytes) -> device rows that start on 16-byte boundaries, so every read is an aligned one and the order of
    a float marker's sums does not depend on where its row lies."""

    def __init__(self, model, d, dtype, idx):
        self.d, self.dtype = d, dtype
        super(DosageRows, self).__init__(model, d.shape[0], d.shape[1] * d.dtype.itemsize, idx)
        self.ldb = (self.row_bytes + 15) // 16 * 16

    def stage(self, rows_max):
        super(DosageRows, self).stage(rows_max)
        self.hB = self.torch.empty((rows_max, self.row_bytes), dtype=self.torch.uint8).pin_memory()
        self.dB = self.torch.empty((rows_max, self.ldb), dtype=self.torch.uint8, device="cuda")

    def load(self, rows):
        d = self.d[rows]
        k = d.shape[0]
        np.copyto(self.hB.numpy()[:k], d.view(np.uint8).reshape(k, self.row_bytes))
        self.dB[:k, :self.row_bytes].copy_(self.hB[:k], non_blocking=True)
        self.torch.cuda.synchronize()

    def enqueue(self, k0, rb, pS, pK=None, env=None):
        f = self.model.factor
        self._call(f.scan_block_dosage_dev, f.scan_block_dosage_gram_dev, f.scan_block_dosage_gxe_dev, self._head(k0), rb, pS, pK, env)

    def _head(self, k0):
        return (vp(self.dB.data_ptr() + k0 * self.ldb), self.dtype, self.ldb // self.d.dtype.itemsize, self.d.shape[1], self._map())

    def spa(self, k0, rb, tail):
        self.model.factor.scan_spa_dosage_dev(*(self._head(k0) + (rb,) + tuple(tail)))

    def sets_spa(self, k0, rb, tail):
        self.model.factor.sets_spa_dosage_dev(*(self._head(k0) + (rb,) + tuple(tail)))

    def collapse(self, k0, rb, tail):
        self.model.factor.sets_collapse_dosage_dev(*(self._head(k0) + (rb,) + tuple(tail)))
