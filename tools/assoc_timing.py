"""HIP-event times of one marker-scan block (scilmm_scan_block_dev: moments + dequantise | forward sweep | statistics) against
the full solve of the same width (scilmm_solve_dev) on the same handle, at a seeded bench cohort; widths 112 (one full chain
window) and 128 (RPMAX), alternating, after a warm-up of every shape, and a cross-check of |w(g~)|^2 against g~' V^-1 g~
from the full solve.
  usage: assoc_timing.py 100k|300k [--blocks 20] [--out FILE] [--solve-only] [--parent FILE]
--solve-only times the full solve alone through entry points every earlier revision has (run it on the parent commit);
--parent merges the JSON such a run wrote as "parent_solve_ms"."""
import argparse, ctypes, json, os, sys
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
ap = argparse.ArgumentParser()
ap.add_argument("workload"); ap.add_argument("--blocks", type=int, default=20); ap.add_argument("--out", default=None)
ap.add_argument("--solve-only", action="store_true"); ap.add_argument("--parent", default=None)
args = ap.parse_args()
import torch
from scilmm_amd.factor import Symbolic
vp = ctypes.c_void_p
WIDTHS, S2 = (112, 128), [0.5, 0.5]
A, Cv, y = bench.build_problem(args.workload, 0)
n = A.shape[0]
I = sp.identity(n, format="csr")
if args.solve_only:
    sym = Symbolic([A, I]); fac = sym.factorize(S2); scan = None
else:
    from scilmm_amd import AssociationScan, SparseCholesky
    scan = AssociationScan(SparseCholesky(), [A, I], S2, Cv, y, block=128)
    sym, fac = scan.sym, scan.factor
rng = np.random.default_rng(0)
G = rng.binomial(2, rng.uniform(0.05, 0.5, 128)[:, None], size=(128, n)).astype(np.int8)
G[rng.random(G.shape) < 0.02] = -1
ld = (n + 15) // 16 * 16
dG = torch.zeros((128, ld), dtype=torch.int8, device="cuda"); dG[:, :n].copy_(torch.from_numpy(G))
obs = dG[:, :n] >= 0
Gt = torch.where(obs, dG[:, :n].double() - (torch.where(obs, dG[:, :n], 0).sum(1).double() / obs.sum(1).double())[:, None], 0.0).T.contiguous()   # n x 128
dB = {r: Gt[:, :r].contiguous() for r in WIDTHS}
dX = {r: torch.empty_like(dB[r]) for r in WIDTHS}
torch.cuda.synchronize()


def solve(r):
    fac.solve_dev(vp(dB[r].data_ptr()), r, vp(dX[r].data_ptr())); sym.sync()
    t = sym.timing()
    return t["solve_fwd_ms"] + t["solve_bwd_ms"]


def block(r):
    fac.scan_block_dev(vp(dG.data_ptr()), ld, r, vp(scan.dQ.data_ptr()), scan.q, vp(dS.data_ptr())); sym.sync()
    return sym.scan_timing()


def summary(v):
    v = np.asarray(v, dtype=float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "iqr": float(np.percentile(v, 75) - np.percentile(v, 25))}


rec = {"workload": args.workload, "n": int(n), "nnzL": int(sym.info().nnzL), "blocks": args.blocks, "sigma2": S2,
       "timer": "HIP events on the engine's stream, one block or solve per synchronise"}
t_solve = {r: [] for r in WIDTHS}
t_scan = {r: [] for r in WIDTHS}
if scan is not None:
    dS = torch.zeros(((scan.q + 4) * 128,), dtype=torch.float64, device="cuda")
for it in range(3 + args.blocks):                     # three rounds of warm-up of every shape, then the timed rounds
    for r in WIDTHS:
        if scan is not None:
            ms = block(r)
            if it >= 3: t_scan[r].append(ms)
        ms = solve(r)
        if it >= 3: t_solve[r].append(ms)
rec["solve_ms"] = {str(r): summary(t_solve[r]) for r in WIDTHS}
if scan is not None:
    rec["scan"] = {}
    for r in WIDTHS:
        a = np.asarray(t_scan[r])
        tot = a.sum(axis=1)
        rec["scan"][str(r)] = {"prep_ms": summary(a[:, 0]), "sweep_ms": summary(a[:, 1]), "stats_ms": summary(a[:, 2]),
                               "total_ms": summary(tot), "markers_per_s": float(r / (np.median(tot) * 1e-3)),
                               "fraction_of_full_solve": float(np.median(tot) / np.median(t_solve[r]))}
    # |w(g~)|^2 of a 128-wide block against g~' V^-1 g~ from the full solve of the same markers
    block(128)
    gg = dS.cpu().numpy().reshape(scan.q + 4, 128)[3]
    solve(128)
    quad = (dB[128] * dX[128]).sum(0).cpu().numpy()
    rec["check_rel_err_gVinvg"] = float(np.abs(gg - quad).max() / np.abs(quad).max())
    rec["default_block"] = max(WIDTHS, key=lambda r: rec["scan"][str(r)]["markers_per_s"])
rec["parent_solve_ms"] = json.load(open(args.parent))["solve_ms"] if args.parent else "not measured"
print(json.dumps(rec))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
