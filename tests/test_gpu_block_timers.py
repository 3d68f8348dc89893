"""What the per-family timing getters hand back between syncs (scilmm_sync reads a call family's events once, when a call of
the family is pending): the figures of a family stay, bit for bit, until a later call of the same family
has been read; the gxe intervals are zero after a block that was no gxe block and parts of the block's first and third interval
after one that was; the collapse's interval is element 0 of scilmm_sets_spa_wide_timing and moves alone.

The suite's small pedigree with one covariate (c = 1, q = 2) on a handle of its own, so that no earlier call has left a figure
behind; blocks of r = 16 and 128 columns (the gxe block: r / 2 markers with one environment column), shapes the set, gxe and
collapse tests run as well."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import test_gpu_sets as GS

pytestmark = pytest.mark.gpu

vp = C.c_void_p


def _positive(ms):
    return all(v > 0.0 and math.isfinite(v) for v in ms)


@pytest.mark.parametrize("r", [16, 128])
def test_timings_stay_until_the_family_is_read_again(r):
    import torch
    from scilmm_amd import SparseCholesky, VariantSetTest
    p = GS._problem("pedigree")
    t = VariantSetTest(SparseCholesky(), [p["A"], p["I"]], GS.S2, p["C"][:, :1], p["y"], block=128)
    fac, sym, n, q = t.factor, t.sym, p["n"], t.q
    assert q == 2
    ld = (n + 15) // 16 * 16
    dG = torch.zeros((r, ld), dtype=torch.int8, device="cuda")
    dG[:, :n].copy_(torch.from_numpy(np.ascontiguousarray(p["G"][4:4 + r])))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    dS = torch.zeros(((q + 4) * r,), dtype=torch.float64, device="cuda")
    dK = torch.zeros((r * r,), dtype=torch.float64, device="cuda")
    dR, du = dev(t.R), dev(t.u)
    dO = torch.zeros((10,), dtype=torch.float64, device="cuda")
    dE = dev(np.random.default_rng(5).standard_normal((n, 1)))
    dX = torch.zeros((3 + (q + 1) * 2 + 1) * (r // 2), dtype=torch.float64, device="cuda")
    dg = torch.zeros((n,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    G, Q, S = vp(dG.data_ptr()), vp(t.dQ.data_ptr()), vp(dS.data_ptr())
    assert sym.gxe_timing() == (0.0, 0.0) and sym.sets_finish_timing() == 0.0 and sym.sets_spa_wide_timing() == (0.0, 0.0, 0.0)

    # a Gram block and the finish of one set that spans it
    fac.scan_block_gram_dev(G, ld, r, Q, q, S, vp(dK.data_ptr()))
    fac.sets_finish_dev(r, q, S, vp(dK.data_ptr()), vp(dR.data_ptr()), vp(du.data_ptr()), t.c, 1, np.array([0, r], dtype=np.int32), 1, None, 0,
                        np.empty(0), vp(dO.data_ptr()), 10, None)
    sym.sync()
    scan, fin = sym.scan_timing(), sym.sets_finish_timing()
    print("r", r, "scan", scan, "finish", fin)
    assert len(scan) == 3 and _positive(scan) and isinstance(fin, float) and _positive((fin,))
    assert sym.gxe_timing() == (0.0, 0.0)
    # nothing queued: a sync changes no figure
    sym.sync()
    assert sym.scan_timing() == scan and sym.sets_finish_timing() == fin

    # a plain block: the finish keeps its figure
    fac.scan_block_dev(G, ld, r, Q, q, S)
    sym.sync()
    assert _positive(sym.scan_timing()) and sym.gxe_timing() == (0.0, 0.0) and sym.sets_finish_timing() == fin

    # a gxe block of r / 2 markers, one environment column: its two kernels are parts of the first and the third interval
    fac.scan_block_gxe_dev(G, ld, r // 2, vp(dE.data_ptr()), 1, Q, q, vp(dX.data_ptr()))
    sym.sync()
    scan, gxe = sym.scan_timing(), sym.gxe_timing()
    print("r", r, "gxe block", scan, "gxe", gxe)
    assert _positive(scan) and len(gxe) == 2 and _positive(gxe)
    assert gxe[0] <= scan[0] and gxe[1] <= scan[2] and sym.sets_finish_timing() == fin
    sym.sync()
    assert sym.scan_timing() == scan and sym.gxe_timing() == gxe
    # ... and zero again after a block that is none
    fac.scan_block_gram_dev(G, ld, r, Q, q, S, vp(dK.data_ptr()))
    sym.sync()
    assert sym.gxe_timing() == (0.0, 0.0) and sym.sets_finish_timing() == fin

    # the collapse behind that block: element 0 of the wide set saddlepoint's figures, and nothing else moves
    scan = sym.scan_timing()
    fac.sets_collapse_dev(G, ld, r, S, 1, None, True, vp(dg.data_ptr()))
    sym.sync()
    wide = sym.sets_spa_wide_timing()
    print("r", r, "collapse", wide)
    assert len(wide) == 3 and _positive(wide[:1]) and wide[1:] == (0.0, 0.0) and wide == fac.sets_spa_wide_timing()
    assert sym.scan_timing() == scan and sym.sets_finish_timing() == fin and sym.gxe_timing() == (0.0, 0.0)
    sym.sync()
    assert sym.sets_spa_wide_timing() == wide
