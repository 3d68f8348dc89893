"""PLINK 1 binary genotypes (``.bed`` / ``.bim`` / ``.fam``) on the host: the file's layout, its sample and marker tables, and
the host unpack.  Nothing here needs a GPU or the built library.

The ``.bed`` file is three magic bytes ``6c 1b 01`` (the third = variant-major) and then, marker by marker, ``ceil(N / 4)``
bytes: sample ``s`` of the ``.fam`` order is bits ``2 (s & 3) .. 2 (s & 3) + 1`` of byte ``s >> 2``, low bits first.  Codes:
``00`` two copies of allele A1, ``01`` missing, ``10`` one copy, ``11`` none; the bits past the last sample are padding.

    bed = BedFile("cohort")                       # cohort.bed, cohort.bim, cohort.fam
    idx = bed.sample_index(cohort_iids)           # the file's sample of every individual of the model, -1 = not in the file
    out = scan.scan_bed(bed, sample_index=idx)    # decoded on the device (scilmm_amd.assoc.AssociationScan)
    G = bed.read(sample_index=idx)                # the host unpack: the slow path into scan(G)
"""
import os

import numpy as np

MAGIC = b"\x6c\x1b\x01"
# allele A1 counts of the four codes, -1 = missing; and with A2 counted instead
_A1 = np.array([2, -1, 1, 0], dtype=np.int8)
_A2 = np.array([0, -1, 1, 2], dtype=np.int8)


def count_flag(count):
    """0 for ``count="A1"``, 1 for ``"A2"`` (bit 0 of the flags of ``scilmm_scan_block_bed_dev``)."""
    if count not in ("A1", "A2"):
        raise ValueError('count must be "A1" or "A2", got %r' % (count,))
    return int(count == "A2")


def marker_indices(markers, m):
    """``markers`` (None, a slice or a 1-D integer array) as an int64 index array into ``0 .. m-1``."""
    if markers is None:
        return np.arange(m, dtype=np.int64)
    if isinstance(markers, slice):
        return np.arange(m, dtype=np.int64)[markers]
    idx = np.asarray(markers)
    if idx.ndim != 1 or (idx.size and idx.dtype.kind not in "iu"):
        raise ValueError("markers must be None, a slice or a 1-D integer array")
    idx = idx.astype(np.int64)
    if idx.size and (idx.min() < -m or idx.max() >= m):
        raise ValueError("a marker index outside the file's %d markers" % m)
    return np.where(idx < 0, idx + m, idx)


def check_sample_index(sample_index, n_samples, n=None, source="file"):
    """``sample_index`` as a contiguous int32 array: 1-D (of length ``n`` where given), values in ``-1 .. n_samples - 1``;
    ``source`` names what holds the samples in the message."""
    idx = np.asarray(sample_index)
    if idx.ndim != 1 or (idx.size and idx.dtype.kind not in "iu"):
        raise ValueError("sample_index must be a 1-D integer array")
    if n is not None and idx.size != n:
        raise ValueError("sample_index has %d entries, the model has %d individuals" % (idx.size, n))
    if idx.size and (idx.min() < -1 or idx.max() >= n_samples):
        raise ValueError("sample_index holds a value outside -1 .. %d (the %s has %d samples)"
                         % (n_samples - 1, source, n_samples))
    return np.ascontiguousarray(idx, dtype=np.int32)


def _table(path, what):
    """The six whitespace-separated columns of a ``.fam`` or ``.bim`` file, as lists of strings."""
    cols = [[] for _ in range(6)]
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            t = line.split()
            if not t:
                continue
            if len(t) < 6:
                raise ValueError("%s: line %d has %d columns, a %s file has six" % (path, ln, len(t), what))
            for c in range(6):
                cols[c].append(t[c])
    return cols


class BedFile(object):
    """A PLINK 1 binary fileset.  ``path``: ``prefix``, ``prefix.bed``, or any path whose siblings are ``.bim`` / ``.fam``.

    ``n_samples`` (N), ``n_markers`` (m); ``fid``, ``iid``: the first two columns of the ``.fam``; ``bim``: a dict of arrays
    ``chrom``, ``snp``, ``cm``, ``pos``, ``a1``, ``a2``; ``packed``: the genotypes as they lie in the file, a read-only
    ``np.memmap`` of shape ``m x ceil(N / 4)``, uint8.  ValueError, naming the file and the reason: wrong magic bytes, the
    sample-major mode, a size other than ``3 + m * ceil(N / 4)``, a repeated IID."""

    def __init__(self, path):
        path = os.fspath(path)
        root, ext = os.path.splitext(path)
        prefix = root if ext in (".bed", ".bim", ".fam") else path
        self.path = bed = prefix + ".bed"
        fam = _table(prefix + ".fam", ".fam")
        bim = _table(prefix + ".bim", ".bim")
        self.fid, self.iid = np.array(fam[0], dtype=object), np.array(fam[1], dtype=object)
        self.n_samples, self.n_markers = N, m = len(fam[1]), len(bim[1])
        if N < 1:
            raise ValueError("%s: no samples" % (prefix + ".fam"))
        self._index = {}
        for s, name in enumerate(fam[1]):
            if name in self._index:
                raise ValueError("%s: the IID %r is there twice (samples %d and %d)" % (prefix + ".fam", name, self._index[name], s))
            self._index[name] = s
        self.bim = {"chrom": np.array(bim[0], dtype=object), "snp": np.array(bim[1], dtype=object),
                    "cm": np.array(bim[2], dtype=np.float64), "pos": np.array(bim[3], dtype=np.int64),
                    "a1": np.array(bim[4], dtype=object), "a2": np.array(bim[5], dtype=object)}
        self.row_bytes = nb = (N + 3) // 4
        with open(bed, "rb") as f:
            magic = f.read(3)
        size = os.path.getsize(bed)
        if magic[:2] != MAGIC[:2]:
            raise ValueError("%s: not a PLINK 1 .bed file (magic bytes %s, expected 6c 1b)" % (bed, magic[:2].hex(" ") or "none"))
        if magic[2:] == b"\x00":
            raise ValueError("%s: sample-major mode (third byte 00) is not supported; rewrite the file variant-major" % bed)
        if magic[2:] != MAGIC[2:]:
            raise ValueError("%s: unknown mode byte %s (expected 01, variant-major)" % (bed, magic[2:].hex() or "none"))
        if size != 3 + m * nb:
            raise ValueError("%s: %s file: %d bytes, but %d markers x %d samples need 3 + %d x %d = %d"
                             % (bed, "truncated" if size < 3 + m * nb else "oversized", size, m, N, m, nb, 3 + m * nb))
        if m:
            self.packed = np.memmap(bed, dtype=np.uint8, mode="r", offset=3, shape=(m, nb))
        else:
            self.packed = np.empty((0, nb), dtype=np.uint8)

    def sample_index(self, iids):
        """The file's sample of every given IID: an int32 array, -1 where the file lacks it."""
        return np.array([self._index.get(str(i), -1) for i in iids], dtype=np.int32).reshape(-1)

    def check_sample_index(self, sample_index, n=None):
        """``sample_index`` as a contiguous int32 array: 1-D (of length ``n`` where given), values in ``-1 .. N-1``."""
        return check_sample_index(sample_index, self.n_samples, n)

    def read(self, markers=None, sample_index=None, count="A1"):
        """The host unpack: allele counts as an int8 ``len(markers) x N`` array (``x len(sample_index)`` with a map), -1 =
        missing.  ``markers``: None, a slice or an integer array; ``sample_index[i]`` = the file's sample of column i, -1 =
        not in the file (missing everywhere); ``count``: the counted allele, "A1" or "A2"."""
        table = _A2 if count_flag(count) else _A1
        rows = marker_indices(markers, self.n_markers)
        idx = None if sample_index is None else self.check_sample_index(sample_index)
        N = self.n_samples
        out = np.empty((rows.size, N if idx is None else idx.size), dtype=np.int8)
        shifts = np.arange(0, 8, 2, dtype=np.uint8)
        step = max(1, (8 << 20) // max(1, 4 * self.row_bytes))
        for k0 in range(0, rows.size, step):
            p = np.asarray(self.packed[rows[k0:k0 + step]])
            g = table[(p[:, :, None] >> shifts) & 3].reshape(p.shape[0], -1)[:, :N]
            if idx is None:
                out[k0:k0 + step] = g
            else:
                out[k0:k0 + step] = np.where(idx >= 0, g[:, np.maximum(idx, 0)], np.int8(-1))
        return out
