"""HIP-event times of one marker-scan block (scilmm_scan_block_dev: moments + dequantise | forward sweep | statistics) against
the full solve of the same width (scilmm_solve_dev) on the same handle, at a seeded bench cohort; widths 112 (one full chain
window) and 128 (RPMAX), alternating, after a warm-up of every shape, and a cross-check of |w(g~)|^2 against g~' V^-1 g~
from the full solve.
  usage: assoc_timing.py 100k|300k [--blocks 20] [--out FILE] [--solve-only] [--parent FILE]
         assoc_timing.py 100k|300k --bed [--blocks 20] [--markers 2048] [--out FILE]
--bed times the block from packed PLINK rows (scilmm_scan_block_bed_dev) against the int8 block of the same markers,
alternating in one run, with the identity map and with a shuffled map that lacks 5 % of the cohort; then, from a fileset
written to a temporary directory, scan_bed(path) against scan(BedFile(path).read(...)) with the host unpack included.
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
ap.add_argument("--bed", action="store_true"); ap.add_argument("--markers", type=int, default=2048)
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


def pack(G):
    """m x N int8 A1 counts (-1 = missing) as .bed rows, padding bits zero."""
    m, N = G.shape
    codes = np.zeros((m, (N + 3) // 4 * 4), dtype=np.uint8)
    codes[:, :N] = np.array([3, 2, 0, 1], dtype=np.uint8)[G]           # 0 -> 11, 1 -> 10, 2 -> 00, -1 -> 01
    c = codes.reshape(m, -1, 4)
    return np.ascontiguousarray(c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6))


def bed_mode():
    import tempfile, time
    from scilmm_amd.bed import BedFile
    r, q = 128, scan.q
    rec = {"workload": args.workload, "n": int(n), "nnzL": int(sym.info().nnzL), "blocks": args.blocks, "sigma2": S2, "r": r,
           "timer": "HIP events on the engine's stream, one block per synchronise; three warm-up rounds of every shape, then "
                    "alternating rounds; wall clock (perf_counter) for the end-to-end runs"}
    # the shuffled map: the file holds the n individuals in another order, 5 % of the cohort are not in it
    idx = rng.permutation(n).astype(np.int32)
    idx[rng.choice(n, size=n // 20, replace=False)] = -1
    Gmap = np.ascontiguousarray(np.where(idx >= 0, G[:, np.maximum(idx, 0)], -1).astype(np.int8))    # cohort order
    P = pack(G)
    nb = P.shape[1]
    dP = torch.from_numpy(P).cuda()
    dGm = torch.zeros((128, ld), dtype=torch.int8, device="cuda"); dGm[:, :n].copy_(torch.from_numpy(Gmap))
    dI = torch.from_numpy(idx).cuda()
    dS = {k: torch.zeros(((q + 4) * r,), dtype=torch.float64, device="cuda") for k in ("int8", "bed", "int8_map", "bed_map")}
    torch.cuda.synchronize()
    Q = vp(scan.dQ.data_ptr())
    shapes = {
        "int8": lambda: fac.scan_block_dev(vp(dG.data_ptr()), ld, r, Q, q, vp(dS["int8"].data_ptr())),
        "bed": lambda: fac.scan_block_bed_dev(vp(dP.data_ptr()), nb, n, None, 0, r, Q, q, vp(dS["bed"].data_ptr())),
        "int8_map": lambda: fac.scan_block_dev(vp(dGm.data_ptr()), ld, r, Q, q, vp(dS["int8_map"].data_ptr())),
        "bed_map": lambda: fac.scan_block_bed_dev(vp(dP.data_ptr()), nb, n, vp(dI.data_ptr()), 0, r, Q, q, vp(dS["bed_map"].data_ptr())),
    }
    t = {k: [] for k in shapes}
    for it in range(3 + args.blocks):
        for k, f in shapes.items():
            f(); sym.sync()
            if it >= 3: t[k].append(sym.scan_timing())
    rec["block"] = {}
    for k in shapes:
        a = np.asarray(t[k]); tot = a.sum(axis=1)
        rec["block"][k] = {"prep_ms": summary(a[:, 0]), "sweep_ms": summary(a[:, 1]), "stats_ms": summary(a[:, 2]),
                           "total_ms": summary(tot), "markers_per_s": float(r / (np.median(tot) * 1e-3))}
    for a, b in (("bed", "int8"), ("bed_map", "int8_map")):
        ratio = rec["block"][a]["total_ms"]["median"] / rec["block"][b]["total_ms"]["median"]
        rec["block"][a + "_over_" + b] = {"median_total_ratio": float(ratio), "within_1.05": bool(ratio <= 1.05)}
        # rows 0..2 (integer sums) are the same bits in either mode; the rest passes through the default mode's atomic sweep
        Sa, Sb = dS[a].cpu().numpy().reshape(q + 4, r), dS[b].cpu().numpy().reshape(q + 4, r)
        rec["block"][a + "_moments_equal_" + b] = bool(np.array_equal(Sa[:3], Sb[:3]))
        rec["block"][a + "_max_rel_diff_" + b] = float(np.abs(Sa[3:] - Sb[3:]).max() / np.abs(Sb[3:]).max())
    # end to end from a fileset on disk: `markers` markers, the 128 above repeated
    m = args.markers
    rows = np.arange(m) % 128
    rec["end_to_end"] = {"markers": m}
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "cohort")
        with open(prefix + ".fam", "w") as f:
            f.writelines("0 i%d 0 0 0 -9\n" % s for s in range(n))
        with open(prefix + ".bim", "w") as f:
            f.writelines("1 rs%d 0 %d A G\n" % (j, j + 1) for j in range(m))
        with open(prefix + ".bed", "wb") as f:
            f.write(b"\x6c\x1b\x01"); f.write(P[rows].tobytes())
        for name, ix in (("identity", None), ("map", idx)):
            tb, th, share = [], [], []
            for it in range(4):                                       # one warm-up, three timed
                t0 = time.perf_counter()
                a = scan.scan_bed(prefix, sample_index=ix)
                t1 = time.perf_counter()
                b = scan(BedFile(prefix).read(sample_index=ix))
                t2 = time.perf_counter()
                if it:
                    tb.append(t1 - t0); th.append(t2 - t1); share.append(scan.bed_seconds[1] / (t1 - t0))
            same = np.array_equal(a["n_obs"], b["n_obs"]) and np.array_equal(a["mean"], b["mean"], equal_nan=True)
            diff = float(np.nanmax(np.abs(a["chi2"] - b["chi2"])) / np.nanmax(np.abs(b["chi2"])))
            rec["end_to_end"][name] = {
                "scan_bed_s": summary(tb), "host_unpack_scan_s": summary(th),
                "scan_bed_markers_per_s": float(m / np.median(tb)), "host_unpack_markers_per_s": float(m / np.median(th)),
                "speedup": float(np.median(th) / np.median(tb)), "scan_bed_not_slower": bool(np.median(tb) <= np.median(th)),
                "h2d_share_of_scan_bed_wall": float(np.median(share)), "n_obs_and_mean_equal": bool(same),
                "max_rel_diff_chi2": diff}
    return rec


rec = {"workload": args.workload, "n": int(n), "nnzL": int(sym.info().nnzL), "blocks": args.blocks, "sigma2": S2,
       "timer": "HIP events on the engine's stream, one block or solve per synchronise"}
if args.bed:
    rec = bed_mode()
    WIDTHS, scan = (), None
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
if not args.bed:
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
if not args.bed:
    rec["parent_solve_ms"] = json.load(open(args.parent))["solve_ms"] if args.parent else "not measured"
print(json.dumps(rec))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
