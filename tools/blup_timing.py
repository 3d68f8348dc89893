"""HIP-event times of one 128-wide BLUP block (scilmm_rel_block_dev: block building | forward sweep | statistics) against the
marker-scan block of the same width (scilmm_scan_block_dev) in the same run, alternating, after a warm-up of both; then
wall-clock times (synchronised) of BLUP.effects(0) and of the whole-cohort BLUP.reliability(), and a cross-check of the two
forms of the predicted values.  At a seeded bench cohort.
  usage: blup_timing.py 100k|300k [--blocks 20] [--repeats 5] [--out FILE]"""
import argparse, ctypes, json, os, sys, time
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
ap = argparse.ArgumentParser()
ap.add_argument("workload"); ap.add_argument("--blocks", type=int, default=20); ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
import torch
from scilmm_amd import AssociationScan, BLUP, SparseCholesky
vp = ctypes.c_void_p
R, S2 = 128, [0.5, 0.5]
A, Cv, y = bench.build_problem(args.workload, 0)
n = A.shape[0]
I = sp.identity(n, format="csr")
chol = SparseCholesky()
blup = BLUP(chol, [A, I], S2, Cv, y, block=R)
scan = AssociationScan(chol, [A, I], S2, Cv, y, block=R)     # the same resident factor, the same Q
sym, fac, q = blup.sym, blup.factor, blup.q
assert scan.factor is fac
rng = np.random.default_rng(0)
G = rng.binomial(2, rng.uniform(0.05, 0.5, R)[:, None], size=(R, n)).astype(np.int8)
G[rng.random(G.shape) < 0.02] = -1
ld = (n + 15) // 16 * 16
dG = torch.zeros((R, ld), dtype=torch.int8, device="cuda"); dG[:, :n].copy_(torch.from_numpy(G))
dS = torch.zeros(((q + 4) * R,), dtype=torch.float64, device="cuda")
w = np.array([1.0, 0.0])
id_sets = [rng.choice(n, R, replace=False).astype(np.int32) for _ in range(3 + args.blocks)]
torch.cuda.synchronize()


def rel_block(ids):
    fac.rel_block_dev(w, ids, vp(blup.dQ.data_ptr()), q, vp(dS.data_ptr())); sym.sync()
    return sym.scan_timing()


def scan_block():
    fac.scan_block_dev(vp(dG.data_ptr()), ld, R, vp(scan.dQ.data_ptr()), q, vp(dS.data_ptr())); sym.sync()
    return sym.scan_timing()


def summary(v):
    v = np.asarray(v, dtype=float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "iqr": float(np.percentile(v, 75) - np.percentile(v, 25))}


def parts(t):
    a = np.asarray(t)
    return {"build_ms": summary(a[:, 0]), "sweep_ms": summary(a[:, 1]), "stats_ms": summary(a[:, 2]), "total_ms": summary(a.sum(axis=1))}


def wall(fn, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize(); t0 = time.perf_counter(); res = fn(); torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return out, res


rec = {"workload": args.workload, "n": int(n), "nnzL": int(sym.info().nnzL), "nnz_pattern": int(sp.tril(A).nnz), "width": R,
       "blocks": args.blocks, "sigma2": S2,
       "timer": "blocks: HIP events on the engine's stream, one block per synchronise; effects / reliability: host wall clock "
                "around the synchronised call"}
t_rel, t_scan = [], []
for it in range(3 + args.blocks):                     # three rounds of warm-up of both shapes, then the timed rounds
    ms = rel_block(id_sets[it])
    if it >= 3: t_rel.append(ms)
    ms = scan_block()
    if it >= 3: t_scan.append(ms)
rec["rel_block"], rec["scan_block"] = parts(t_rel), parts(t_scan)
rec["build_over_sweep"] = rec["rel_block"]["build_ms"]["median"] / rec["rel_block"]["sweep_ms"]["median"]
blup.effects(0); blup._dv = None                      # warm-up (the SpMM's first launch)
t_eff, eff = wall(lambda: (setattr(blup, "_dv", None), blup.effects(0))[1], args.repeats)
rec["effects0_ms"] = summary(t_eff)
t_all, rel = wall(lambda: blup.reliability(0), max(1, min(args.repeats, 3)))
rec["reliability_all_ms"] = summary(t_all)
rec["reliability_all_blocks"] = (n + R - 1) // R
rec["check_rel_err_effects_vs_blocks"] = float(np.abs(eff - rel["u"]).max() / np.abs(eff).max())
rec["pev_range"] = [float(rel["pev"].min()), float(rel["pev"].max())]
rec["reliability_range"] = [float(rel["reliability"].min()), float(rel["reliability"].max())]
print(json.dumps(rec))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
