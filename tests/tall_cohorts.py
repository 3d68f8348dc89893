"""The cohorts of tests/test_gpu_blocks_tall.py, the constants of the block kernels read from their sources, and the run
rule of the three fold kernels in Python (host only; nothing here calls the device).

A cohort is a set of families: A is block diagonal with blocks (1 - rho) I + rho 11', so with V = s0 A + s1 I the inverse
and the Cholesky factor are block-wise and no dense n x n matrix is ever formed -- the un-whitened GLS oracle of
tests/test_gpu_assoc.py runs at 65 577 individuals with `block_inverse` in place of np.linalg.inv.

    T8K    8199 = 4 * 2048 + 7    families of 1..8     every fold (k_scan_fold, k_gram_fold, k_panel_fold) gets a full run of
                                                       two or more slices, a shorter run and an empty one; k_scan_moments
                                                       takes three trips
    T65K   65 577 = 65 536 + 41   families of 1..8     k_scan_keep and k_csr_spmm stride over their capped grids; the moments
                                                       kernels of every input form take several trips
    B64    16 448 = 257 * 64      257 families of 64   534 560 slots in the lower triangle: the row part of k_rel_gather strides

`tests/test_tall_cohorts.py` asserts these facts from `kernel_constants()` and `fold_runs` without a GPU: a later change of
a slice, a fold width or a grid cap fails there by name instead of quietly moving the GPU cases off the edges.
"""
import os
import re

import numpy as np
import scipy.sparse as sp

from tests.test_gpu_assoc import _markers

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scilmm_amd", "csrc")
S2 = [0.4, 0.6]
M = 130                       # markers: a partial last block at every block width
COHORTS = {
    "T8K": dict(n=8199, sizes=tuple(range(1, 9))),
    "T65K": dict(n=65577, sizes=tuple(range(1, 9))),
    "B64": dict(n=16448, sizes=(64,)),
}
_BUILT = {}


def family_sizes(n, sizes):
    """The block sizes: `sizes` cycled, the last block truncated so that they add up to n."""
    out, left, k = [], n, 0
    while left > 0:
        s = min(sizes[k % len(sizes)], left)
        out.append(s)
        left -= s
        k += 1
    return np.array(out, dtype=np.int64)


def families(n, sizes, rho=0.5):
    """(A, blocks): A block diagonal (sorted CSR) with blocks (1 - rho) I + rho 11' of the sizes in `sizes`, cycled and
    truncated to n, and the list of the dense blocks."""
    bs = family_sizes(n, sizes)
    start = np.concatenate([[0], np.cumsum(bs)[:-1]])
    row_size = np.repeat(bs, bs)                              # per individual: the size and the first individual of its family
    row_start = np.repeat(start, bs)
    indptr = np.concatenate([[0], np.cumsum(row_size)])
    rows = np.repeat(np.arange(n), row_size)
    indices = np.repeat(row_start, row_size) + (np.arange(indptr[-1]) - np.repeat(indptr[:-1], row_size))
    data = np.where(indices == rows, 1.0, rho)
    A = sp.csr_matrix((data, indices.astype(np.int32), indptr.astype(np.int32)), shape=(n, n))
    A.has_sorted_indices = True
    made = {int(s): (1.0 - rho) * np.eye(s) + rho * np.ones((s, s)) for s in np.unique(bs)}
    return A, [made[int(s)] for s in bs]


def block_inverse(blocks, s0, s1):
    """inv(s0 A + s1 I) for the block-diagonal A of `blocks`, as a sparse matrix."""
    return sp.block_diag([np.linalg.inv(s0 * b + s1 * np.eye(len(b))) for b in blocks], format="csr")


def block_whitener(blocks, s0, s1):
    """inv(L) with L L' = s0 A + s1 I (L block diagonal, lower triangular), as a sparse matrix."""
    return sp.block_diag([np.linalg.inv(np.linalg.cholesky(s0 * b + s1 * np.eye(len(b)))) for b in blocks], format="csr")


def cohort(cid):
    """The cohort's matrices (A, I), blocks, covariates (n x 4, an intercept first), y and the sparse inverses per sigma2
    (filled by `inverse`); built once."""
    if cid not in _BUILT:
        n = COHORTS[cid]["n"]
        A, blocks = families(n, COHORTS[cid]["sizes"])
        rng = np.random.default_rng(11)
        Cv = np.hstack([np.ones((n, 1)), rng.standard_normal((n, 3))])
        y = Cv @ np.array([0.5, -0.2, 0.1, 0.3]) + rng.standard_normal(n)
        _BUILT[cid] = dict(id=cid, A=A, I=sp.identity(n, format="csr"), blocks=blocks, n=n, C=Cv, y=y, vi={}, cache={})
    return _BUILT[cid]


def inverse(p, s2=S2):
    """The block-wise inv(V) of the cohort at `s2`, kept where tests.test_gpu_assoc._oracle looks for its dense inverse."""
    key = tuple(s2)
    if key not in p["vi"]:
        p["vi"][key] = block_inverse(p["blocks"], s2[0], s2[1])
    return p["vi"][key]


def markers(p, m=M, seed=7):
    """tests.test_gpu_assoc._markers at the cohort's n (binomial, 2 % missing, the four overwritten edge markers); built once
    per (m, seed)."""
    key = ("G", m, seed)
    if key not in p["cache"]:
        p["cache"][key] = _markers(p["n"], m, seed)
    return p["cache"][key]


def release():
    _BUILT.clear()


def fold_runs(nslice, nruns):
    """(s0, s1) of each run as k_scan_fold, k_gram_fold and k_panel_fold compute them: run u sums the slices s0 <= sl < s1."""
    per = (nslice + nruns - 1) // nruns
    return [(u * per, min(nslice, u * per + per)) for u in range(nruns)]


def run_lengths(nslice, nruns):
    return [max(0, s1 - s0) for s0, s1 in fold_runs(nslice, nruns)]


def exact_moments(G):
    """Per int8 marker (negative = missing) the three integer sums of its observed values: (count, sum, sum of squares) as
    Python integers.  The centred sum of squares is exactly sq - sum^2 / cnt."""
    out = []
    for g in G:
        obs = g[g >= 0].astype(np.int64)
        out.append((int(obs.size), int(obs.sum()), int((obs * obs).sum())))
    return out


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _int(text, pattern, name):
    m = re.search(pattern, text)
    if m is None:
        raise AssertionError("%s: not found in the kernel sources (pattern %r)" % (name, pattern))
    return int(m.group(1))


def kernel_constants():
    """The constants the tall cases depend on, read from the text of csrc/: a change there is seen by
    tests/test_tall_cohorts.py."""
    scan, gram, panel, blup, spmm = (_text(f) for f in ("scan.hip.h", "gram.hip.h", "panel.hip.h", "blup.hip.h", "csr_spmm.hip"))
    bed, dos, make = _text("bed.hip.h"), _text("dosage.hip.h"), _text("Makefile")
    k = {name: _int(text, r"constexpr int %s = (\d+);" % name, name)
         for name, text in (("SCAN_SLICE", scan), ("SCAN_FOLD", scan), ("GRAM_FOLD", gram), ("PANEL_FOLD", panel),
                            ("KEEP_ROWS", gram), ("KEEP_GRID", gram), ("REL_GRID", blup), ("DOS_FLIGHT", dos), ("DOS_PIECES", dos))}
    k["GRAM_SLICE"] = _int(gram, r"#define SCILMM_GRAM_SLICE (\d+)", "SCILMM_GRAM_SLICE")
    k["PANEL_SLICE"] = _int(panel, r"#define SCILMM_PANEL_SLICE (\d+)", "SCILMM_PANEL_SLICE")
    k["MAKE_GRAM_SLICE"] = _int(make, r"(?m)^GRAM_SLICE \?= (\d+)", "GRAM_SLICE of the Makefile")     # what the library is built with
    k["MAKE_PANEL_SLICE"] = _int(make, r"(?m)^PANEL_SLICE \?= (\d+)", "PANEL_SLICE of the Makefile")
    m = re.search(r"std::min<int64_t>\(\(\(int64_t\)n \+ 3\) / 4, (\d+) \* (\d+)\)", spmm)
    if m is None:
        raise AssertionError("the grid cap of scilmm_csr_spmm_dev: not found in csr_spmm.hip")
    k["SPMM_GRID"] = int(m.group(1)) * int(m.group(2))        # workgroups of four waves, a wave per row
    k["BED_FLIGHT"] = _int(bed, r"i \+= (\d+) \* 256\)", "individuals in flight of k_bed_moments")
    return k
