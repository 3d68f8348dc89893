"""HIP-event times of one marker x environment block (scilmm_scan_block_gxe_dev: fill + k_scan_expand | forward sweep |
statistics + k_scan_cross) at its full width d r = 128 (m = 1, 3) or 126 (m = 2), against a plain 128-marker block
(scilmm_scan_block_dev) on the same handle and the same whitened Q, at a seeded bench cohort: three warm-up rounds of every
shape, then alternating rounds; medians and IQR.  expand_ms and cross_ms are the two kernels the gxe block adds
(scilmm_gxe_timing), parts of its first and third interval.  A cross-check: |w(g~)|^2 of the gxe block against the plain
block's for the same markers.
  usage: gxe_timing.py 100k|300k [--blocks 20] [--out profiles/gxe_100k.json]"""
import argparse, ctypes, json, os, sys
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
ap = argparse.ArgumentParser()
ap.add_argument("workload"); ap.add_argument("--blocks", type=int, default=20); ap.add_argument("--out", default=None)
args = ap.parse_args()
import torch
from scilmm_amd import AssociationScan, SparseCholesky
from scilmm_amd.gxe import stat_rows
vp = ctypes.c_void_p
S2 = [0.5, 0.5]
A, Cv, y = bench.build_problem(args.workload, 0)
n = A.shape[0]
I = sp.identity(n, format="csr")
rng = np.random.default_rng(0)
E = rng.standard_normal((n, 3))
E[:, 0] = rng.integers(0, 2, n)                       # a binary environment (sex, treatment), two quantitative ones
scan = AssociationScan(SparseCholesky(), [A, I], S2, np.hstack([Cv, E]), y, block=128)
sym, fac, q = scan.sym, scan.factor, scan.q
gxe = {m: scan.interaction(E[:, :m]) for m in (1, 2, 3)}
G = rng.binomial(2, rng.uniform(0.05, 0.5, 128)[:, None], size=(128, n)).astype(np.int8)
G[rng.random(G.shape) < 0.02] = -1
ld = (n + 15) // 16 * 16
dG = torch.zeros((128, ld), dtype=torch.int8, device="cuda"); dG[:, :n].copy_(torch.from_numpy(G))
dS = {m: torch.zeros((stat_rows(q, 1 + m) * 128,), dtype=torch.float64, device="cuda") for m in (0, 1, 2, 3)}
torch.cuda.synchronize()
Q = vp(scan.dQ.data_ptr())


def block(m):
    """One block of shape m (0 = the plain 128-marker block): (prep, sweep, statistics, expand, cross) in ms."""
    if m == 0:
        fac.scan_block_dev(vp(dG.data_ptr()), ld, 128, Q, q, vp(dS[0].data_ptr()))
    else:
        fac.scan_block_gxe_dev(vp(dG.data_ptr()), ld, gxe[m].block, vp(gxe[m].dE.data_ptr()), m, Q, q, vp(dS[m].data_ptr()))
    sym.sync()
    return sym.scan_timing() + sym.gxe_timing()


def summary(v):
    v = np.asarray(v, dtype=float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "iqr": float(np.percentile(v, 75) - np.percentile(v, 25))}


t = {m: [] for m in (0, 1, 2, 3)}
for it in range(3 + args.blocks):                     # three rounds of warm-up of every shape, then the timed rounds
    for m in t:
        ms = block(m)
        if it >= 3: t[m].append(ms)
rec = {"workload": args.workload, "n": int(n), "nnzL": int(sym.info().nnzL), "blocks": args.blocks, "sigma2": S2, "q": int(q),
       "timer": "HIP events on the engine's stream, one block per synchronise; three warm-up rounds of every shape, then "
                "alternating rounds", "gxe": {}}
for m in t:
    a = np.asarray(t[m]); tot = a[:, :3].sum(axis=1)
    r = 128 if m == 0 else gxe[m].block
    e = {"markers": r, "columns": (1 + m) * r, "prep_ms": summary(a[:, 0]), "sweep_ms": summary(a[:, 1]), "stats_ms": summary(a[:, 2]),
         "total_ms": summary(tot), "markers_per_s": float(r / (np.median(tot) * 1e-3))}
    if m == 0:
        rec["plain"] = e
        continue
    e["expand_ms"], e["cross_ms"] = summary(a[:, 3]), summary(a[:, 4])
    e["block_ratio_to_plain"] = float(np.median(tot) / rec["plain"]["total_ms"]["median"])
    e["markers_per_s_ratio_to_plain"] = float(e["markers_per_s"] / rec["plain"]["markers_per_s"])
    plain_extra = rec["plain"]["prep_ms"]["median"] + rec["plain"]["stats_ms"]["median"]
    e["expand_plus_cross_over_plain_prep_plus_stats"] = float((np.median(a[:, 3]) + np.median(a[:, 4])) / plain_extra)
    # term 0 of the gxe block is the plain block's column: |w(g~)|^2 agrees to rounding (other block width, other order)
    gg = dS[m][:stat_rows(q, 1 + m) * r].cpu().numpy().reshape(-1, r)[3]
    ref = dS[0].cpu().numpy().reshape(q + 4, 128)[3, :r]
    e["check_rel_diff_gg"] = float(np.abs(gg - ref).max() / np.abs(ref).max())
    rec["gxe"][str(m)] = e
print(json.dumps(rec))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
