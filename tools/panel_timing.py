"""HIP-event times of the phenotype panel's two kernels (scilmm_scan_panel_dev: k_scan_panel | k_panel_fold, read through
scilmm_panel_timing) behind a plain 128-marker block (scilmm_scan_block_dev: fill | forward sweep | statistics, read through
scilmm_scan_timing) on the same handle, at a seeded bench cohort, for panels of T = 128 and 1024 columns: three warm-up rounds
of every shape, then alternating rounds; medians and IQR.  The fraction of the fp64 MFMA peak counts 2 n rp T flop.  With a
library built with -DSCILMM_DIAG, --slices 512,1024,2048 times the row slicings side by side in the same rounds
(SCILMM_PANEL_SHAPE, read per call); a production build carries PANEL_SLICE alone and ignores it.  A cross-check: column 0
of every panel is the first whitened covariate, so x_j . y_0 must agree with row 4 of the block's statistics (another kernel,
another order).
  usage: panel_timing.py 100k|300k [--blocks 20] [--traits 128,1024] [--slices 2048] [--out profiles/panel_100k.json]"""
import argparse, ctypes, json, os, sys
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
ap = argparse.ArgumentParser()
ap.add_argument("workload"); ap.add_argument("--blocks", type=int, default=20); ap.add_argument("--out", default=None)
ap.add_argument("--traits", default="128,1024"); ap.add_argument("--slices", default="")
args = ap.parse_args()
import torch
from scilmm_amd import AssociationScan, SparseCholesky
vp = ctypes.c_void_p
S2 = [0.5, 0.5]
PEAK = 78.6e12                                        # fp64 MFMA peak of the MI355X, flop/s
R = 128
traits = [int(t) for t in args.traits.split(",")]
slices = [int(s) for s in args.slices.split(",")] if args.slices else [0]     # 0: the library's own PANEL_SLICE
A, Cv, y = bench.build_problem(args.workload, 0)
n = A.shape[0]
I = sp.identity(n, format="csr")
rng = np.random.default_rng(0)
scan = AssociationScan(SparseCholesky(), [A, I], S2, Cv, y, block=R)
sym, fac, q = scan.sym, scan.factor, scan.q
G = rng.binomial(2, rng.uniform(0.05, 0.5, R)[:, None], size=(R, n)).astype(np.int8)
G[rng.random(G.shape) < 0.02] = -1
ld = (n + 15) // 16 * 16
dG = torch.zeros((R, ld), dtype=torch.int8, device="cuda"); dG[:, :n].copy_(torch.from_numpy(G))
dS = torch.zeros(((q + 4) * R,), dtype=torch.float64, device="cuda")
gen = torch.Generator(device="cuda").manual_seed(0)
dY = {T: torch.randn((n, T), generator=gen, dtype=torch.float64, device="cuda") for T in traits}
for T in traits: dY[T][:, 0] = scan.dQ[:, 0]          # column 0 = the first whitened covariate: the cross-check below
dB = {T: torch.zeros((R, T), dtype=torch.float64, device="cuda") for T in traits}
torch.cuda.synchronize()
Q = vp(scan.dQ.data_ptr())


def block(T, slice_):
    """One plain block, with T > 0 followed by one panel of T columns: (prep, sweep, statistics, k_scan_panel, k_panel_fold) in ms."""
    fac.scan_block_dev(vp(dG.data_ptr()), ld, R, Q, q, vp(dS.data_ptr()))
    if T:
        if slice_: os.environ["SCILMM_PANEL_SHAPE"] = str(slice_)
        fac.scan_panel_dev(R, vp(dY[T].data_ptr()), T, T, vp(dB[T].data_ptr()), T)
    sym.sync()
    return sym.scan_timing() + (sym.panel_timing() if T else (0.0, 0.0))


def summary(v):
    v = np.asarray(v, dtype=float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "iqr": float(np.percentile(v, 75) - np.percentile(v, 25))}


shapes = [(0, 0)] + [(T, s) for T in traits for s in slices]
t = {k: [] for k in shapes}
for it in range(3 + args.blocks):                     # three rounds of warm-up of every shape, then the timed rounds
    for k in shapes:
        ms = block(*k)
        if it >= 3: t[k].append(ms)
rec = {"workload": args.workload, "n": int(n), "nnzL": int(sym.info().nnzL), "blocks": args.blocks, "sigma2": S2, "q": int(q), "r": R,
       "peak_fp64_mfma_tflops": PEAK / 1e12,
       "timer": "HIP events on the engine's stream, one block (and its panel) per synchronise; three warm-up rounds of every shape, "
                "then alternating rounds", "panel": {}}
a = np.asarray(t[(0, 0)]); tot0 = a[:, :3].sum(axis=1)
rec["plain"] = {"prep_ms": summary(a[:, 0]), "sweep_ms": summary(a[:, 1]), "stats_ms": summary(a[:, 2]), "total_ms": summary(tot0)}
for (T, s) in shapes[1:]:
    a = np.asarray(t[(T, s)]); both = a[:, 3] + a[:, 4]; tot = a[:, :3].sum(axis=1) + both
    flop = 2.0 * n * R * T
    e = {"traits": T, "slice": s or "library", "scan_panel_ms": summary(a[:, 3]), "panel_fold_ms": summary(a[:, 4]), "panel_ms": summary(both),
         "block_without_panel_ms": summary(a[:, :3].sum(axis=1)), "total_ms": summary(tot), "flop": flop,
         "tflops": float(flop / (np.median(both) * 1e-3) / 1e12), "fraction_of_peak": float(flop / (np.median(both) * 1e-3) / PEAK),
         "panel_over_plain_block": float(np.median(both) / np.median(tot0)),
         "block_ratio_to_plain": float(np.median(tot) / np.median(tot0))}
    # column 0 of Y is w(C)[:, 0]: x_j . y_0 is row 4 of the block's statistics (another kernel, another order)
    ref = dS.cpu().numpy().reshape(q + 4, R)[4]
    e["check_rel_diff_col0"] = float(np.abs(dB[T][:, 0].cpu().numpy() - ref).max() / np.abs(ref).max())
    rec["panel"]["T%d_S%s" % (T, s or "lib")] = e
print(json.dumps(rec))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
