"""Whole-cohort reliabilities from the selected inverse (BLUP.reliability_all("total")) against the column path of the same
build (BLUP.reliability("total"), everybody: one forward-sweep column per individual), at a seeded bench cohort, in ONE run on
one resident factor; then the parts of the new path one by one, and the agreement of the two.
  usage: pev_timing.py 100k|300k [--reps 3] [--block 128] [--out FILE]
Wall clock (perf_counter) around whole calls, the device waited for: both paths end in a device-to-host copy.  The new path is
run afresh every time (its cache is dropped): solve, inversion, two pattern calls, refactorization, every time."""
import argparse, ctypes, json, os, sys, time
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
ap = argparse.ArgumentParser()
ap.add_argument("workload"); ap.add_argument("--reps", type=int, default=3); ap.add_argument("--block", type=int, default=128)
ap.add_argument("--out", default=None)
args = ap.parse_args()
import torch
from scilmm_amd import BLUP, SparseCholesky
vp = ctypes.c_void_p
S2 = [0.5, 0.5]
A, Cv, y = bench.build_problem(args.workload, 0)
n = A.shape[0]
I = sp.identity(n, format="csr")
blup = BLUP(SparseCholesky(), [A, I], S2, Cv, y, block=args.block)
sym, fac, c = blup.sym, blup.factor, blup.c
nnz = int(sym.info().nnz_pattern)


def summary(v):
    v = np.asarray(v, dtype=float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def wall(f):
    torch.cuda.synchronize(); sym.sync()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize(); sym.sync()
    return time.perf_counter() - t0, out


def fresh_all():
    blup._inv = None
    return blup.reliability_all("total")


t_col, t_all = [], []
for it in range(1 + args.reps):                       # one warm-up round of either path, then alternating rounds
    s, cols = wall(lambda: blup.reliability("total"))
    if it: t_col.append(s)
    s, alls = wall(fresh_all)
    if it: t_all.append(s)
rec = {"workload": args.workload, "n": int(n), "c": int(c), "nnzL": int(sym.info().nnzL), "nnz_pattern": nnz, "sigma2": S2,
       "block": args.block, "reps": args.reps,
       "timer": "perf_counter around the whole call, device waited for before and after; one warm-up round, then alternating "
                "rounds; reliability_all runs its whole pass every time (cache dropped)",
       "reliability_total_everybody_s": summary(t_col), "reliability_all_total_s": summary(t_all),
       "column_blocks": int((n + args.block - 1) // args.block)}
rec["column_path_over_selected_inverse"] = float(np.median(t_col) / np.median(t_all))
rec["max_rel_diff"] = {k: float(np.abs(alls[k] - cols[k]).max() / np.abs(cols[k]).max()) for k in ("u", "pev", "reliability", "self_rel")}

# the parts of the pass, one by one
parts = {}
parts["diagonals_download_s"] = wall(blup._diagonals)[0]
dB = torch.from_numpy(np.ascontiguousarray(np.hstack([Cv, y[:, None]]))).cuda()
dX = torch.empty_like(dB)
parts["solve_%d_columns_s" % (c + 1)] = wall(lambda: fac.solve_dev(vp(dB.data_ptr()), c + 1, vp(dX.data_ptr())))[0]
parts["selected_inverse_s"] = wall(fac.selected_inverse)[0]
parts["selected_inverse_device_ms"] = float(sym.timing()["quad_ms"])
de = torch.full((n,), S2[1], dtype=torch.float64, device="cuda")
dT = dX[:, :c].contiguous()
dd = torch.empty((n,), dtype=torch.float64, device="cuda")
do = torch.empty((nnz,), dtype=torch.float64, device="cuda")
CALLS = 20


def pattern(diag, off):
    def run():
        for _ in range(CALLS):
            fac.inverse_pattern_dev(vp(dd.data_ptr()) if diag else None, vp(do.data_ptr()) if off else None, -1.0, vp(de.data_ptr()),
                                    1.0, vp(dT.data_ptr()), c)
    run()                                             # warm-up
    return wall(run)[0] / CALLS


t_d, t_o = pattern(True, False), pattern(False, True)
# bytes the kernels' comments count: per individual 36 + 8 c, per slot 52 + 16 c (the column ends: 8 per column once more)
parts["k_invpat_diag_ms"] = 1e3 * t_d
parts["k_invpat_slots_ms"] = 1e3 * t_o
parts["k_invpat_slots_nominal_GBs"] = float((nnz * (52 + 16 * c) + 8 * n) / t_o / 1e9)
parts["pattern_timer"] = "wall clock over %d calls queued back to back, one wait" % CALLS
parts["refactorize_s"] = wall(lambda: fac.refactorize(S2))[0]
rec["parts"] = parts
print(json.dumps(rec))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
