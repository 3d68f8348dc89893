"""HIP-event time of the saddlepoint call (scilmm_scan_spa_dev: k_scan_spa, read through scilmm_spa_timing) behind a plain
128-marker block (scilmm_scan_block_dev: fill | forward sweep | statistics, read through scilmm_scan_timing) on the same handle,
at a seeded bench cohort with a 0 / 1 phenotype of prevalence 0.05 (the top 5 % of the bench phenotype) and null markers: with
cutoff = 0 (every marker takes both roots) and with cutoff = 2 (the markers beyond two standard deviations only), three warm-up
rounds of both, then alternating rounds; medians and IQR.  The null point is not fitted (a timing needs no converged fit): tau =
0.5, the covariate-only logistic fit, b = 0.  Per call the file also records how many markers were saddlepointed, the Newton
passes they took, and the bytes and exponentials that makes by count (16 B and one exp per individual per pass).
  usage: spa_timing.py 100k|300k [--blocks 20] [--out profiles/spa_100k.json]"""
import argparse, ctypes, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
ap = argparse.ArgumentParser()
ap.add_argument("workload"); ap.add_argument("--blocks", type=int, default=20); ap.add_argument("--out", default=None)
args = ap.parse_args()
import torch
from scilmm_amd import LogisticMixedModel, SparseCholesky
from scilmm_amd.glmm import SPA_ROWS, logistic_irls
vp = ctypes.c_void_p
R = 128
A, Cv, y = bench.build_problem(args.workload, 0)
n = A.shape[0]
yb = (y > np.quantile(y, 0.95)).astype(np.float64)
rng = np.random.default_rng(0)
model = LogisticMixedModel(SparseCholesky(), [A], Cv, yb)
scan = model.null_at([0.5], logistic_irls(model.covariates, yb), np.zeros(n)).scan(block=R, cutoff=0.0)
sym, fac, q = scan.sym, scan.factor, scan.q
G = rng.binomial(2, rng.uniform(0.05, 0.5, R)[:, None], size=(R, n)).astype(np.int8)
G[rng.random(G.shape) < 0.02] = -1
ld = (n + 15) // 16 * 16
dG = torch.zeros((R, ld), dtype=torch.int8, device="cuda"); dG[:, :n].copy_(torch.from_numpy(G))
dS = torch.zeros(((q + 4) * R,), dtype=torch.float64, device="cuda")
dP = torch.zeros((SPA_ROWS * R,), dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
tail = tuple(vp(t.data_ptr()) for t in (scan.dR, scan.du, scan.dmu, scan.dC))


def block(cutoff):
    """One plain block, with cutoff >= 0 followed by its saddlepoint call: (prep, sweep, statistics, k_scan_spa) in ms."""
    fac.scan_block_dev(vp(dG.data_ptr()), ld, R, vp(scan.dQ.data_ptr()), q, vp(dS.data_ptr()))
    if cutoff >= 0:
        fac.scan_spa_dev(vp(dG.data_ptr()), ld, R, vp(dS.data_ptr()), *tail, scan.c, vp(scan.dMinv.data_ptr()), float(cutoff), vp(dP.data_ptr()))
    sym.sync()
    return sym.scan_timing() + ((sym.spa_timing(),) if cutoff >= 0 else (0.0,))


def summary(v):
    v = np.asarray(v, dtype=float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "iqr": float(np.percentile(v, 75) - np.percentile(v, 25))}


shapes = [-1.0, 0.0, 2.0]
t, rows = {k: [] for k in shapes}, {}
for it in range(3 + args.blocks):                     # three rounds of warm-up of every shape, then the timed rounds
    for k in shapes:
        ms = block(k)
        if it >= 3: t[k].append(ms)
        if k >= 0: rows[k] = dP.cpu().numpy().reshape(SPA_ROWS, R).copy()
rec = {"workload": args.workload, "n": int(n), "nnzL": int(sym.info().nnzL), "blocks": args.blocks, "q": int(q), "c": int(scan.c), "r": R,
       "prevalence": float(yb.mean()),
       "timer": "HIP events on the engine's stream, one block (and its saddlepoint call) per synchronise; three warm-up rounds of "
                "every shape, then alternating rounds", "spa": {}}
a = np.asarray(t[-1.0]); tot0 = a[:, :3].sum(axis=1)
rec["plain"] = {"prep_ms": summary(a[:, 0]), "sweep_ms": summary(a[:, 1]), "stats_ms": summary(a[:, 2]), "total_ms": summary(tot0)}
for k in shapes[1:]:
    a = np.asarray(t[k]); P = rows[k]
    att = P[6] > 0
    passes = float(np.nansum(np.where(att, 2 * P[5] + 2, 0.0)))        # an upper count: both roots at the larger iteration count, + K at each
    med = np.median(a[:, 3])
    rec["spa"]["cutoff_%g" % k] = {
        "cutoff": k, "spa_ms": summary(a[:, 3]), "block_without_spa_ms": summary(a[:, :3].sum(axis=1)),
        "spa_over_plain_block": float(med / np.median(tot0)), "markers_attempted": int(att.sum()), "flag1": int((P[6] == 1).sum()),
        "flag2": int((P[6] == 2).sum()), "iters_max": float(np.nanmax(P[5])) if att.any() else 0.0, "passes_upper_count": passes,
        "bytes_by_count": 16.0 * n * passes, "exp_by_count": float(n) * passes,
        "gbytes_per_s_by_count": float(16.0 * n * passes / (med * 1e-3) / 1e9) if att.any() else 0.0,
        "gexp_per_s_by_count": float(n * passes / (med * 1e-3) / 1e9) if att.any() else 0.0}
print(json.dumps(rec))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
