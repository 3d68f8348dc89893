"""HIP-event and wall times of the variant-set finish under annotation masks and MAF cutoffs (scilmm_sets_finish_masks_dev:
k_sets_finish_masks, read through scilmm_sets_finish_masks_timing) behind a Gram block, at a seeded bench cohort: the first
packed block of tools/sets_timing.py --finish (512 rare markers in consecutive sets of 2 .. 17, packed into 128-wide blocks: a
dozen sets), A = 3 nested annotations (30 %, 60 %, all of the markers) crossed with F = 3 cutoffs, SKAT-O on the default grid.
In the same rounds the yardstick: the same block through scilmm_sets_finish_dev (one scalar finish), which this work leaves as
it was.  Three warm-up rounds of both shapes, then alternating rounds; medians and IQR.  Wall times, the median of three calls
after one: masked(G, sets, skato=True) per set, and the same cells as NINE tester(G, cell sets, skato=True, finish="device")
calls, one per (annotation, cutoff) with the cells' members computed on the host -- what a user had to do without masks: nine
Gram blocks and nine sweeps.  A cross-check: the cells of the masked call against those nine calls (1e-9 on the statistics,
1e-6 on the p-values; a Gram entry may depend on the column's place, so not bit for bit).
  usage: sets_masks_timing.py 100k [--blocks 20] [--max-maf 0.05,0.025,0.01] [--out profiles/sets_masks_100k.json]"""
import argparse, ctypes, json, os, sys, time
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
ap = argparse.ArgumentParser()
ap.add_argument("workload"); ap.add_argument("--blocks", type=int, default=20); ap.add_argument("--out", default=None)
ap.add_argument("--max-maf", default="0.05,0.025,0.01"); ap.add_argument("--acat-mac", type=float, default=10.0)
args = ap.parse_args()
import torch
from scilmm_amd import SparseCholesky, VariantSetTest
from scilmm_amd.set_masks import TAIL, maf_of, pack_words
from scilmm_amd.sets import FINISH_HEAD, RHO_DEFAULT, pack_sets
vp = ctypes.c_void_p
R, S2, M = 128, [0.5, 0.5], 512
cuts = np.array([float(c) for c in args.max_maf.split(",")])
A, Cv, y = bench.build_problem(args.workload, 0)
n = A.shape[0]
tester = VariantSetTest(SparseCholesky(), [A, sp.identity(n, format="csr")], S2, Cv, y, block=R)
sym, fac, q = tester.sym, tester.factor, tester.q
# the markers and the sets of tools/sets_timing.py --finish: the same draws in the same order
rng = np.random.default_rng(0)
G = rng.binomial(2, rng.uniform(0.005, 0.05, R)[:, None], size=(R, n)).astype(np.int8)
G[rng.random(G.shape) < 0.02] = -1
Gm = rng.binomial(2, rng.uniform(0.005, 0.05, M)[:, None], size=(M, n)).astype(np.int8)
Gm[rng.random(Gm.shape) < 0.02] = -1
sets, at = [], 0
while at < M:
    k = min(int(rng.integers(2, 18)), M - at)
    sets.append(np.arange(at, at + k))
    at += k
members = pack_sets([s.size for s in sets], R)[0]
block_sets = [sets[i] for i in members]
rows = np.concatenate(block_sets)
sizes = [s.size for s in block_sets]
rb, ns = rows.size, len(sizes)
start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
local = [np.arange(a_, b_) for a_, b_ in zip(start[:-1], start[1:])]          # the sets as rows of Gm[rows]
Gb = np.ascontiguousarray(Gm[rows])
# three nested annotations, seeded: 30 %, 60 %, all of the block's markers
u = np.random.default_rng(2).random(rb)
ann = np.stack([u < 0.3, u < 0.6, np.ones(rb, dtype=bool)], axis=1)
NA, NF = ann.shape[1], cuts.size
words = pack_words(ann)
rho = np.asarray(RHO_DEFAULT)
ld = (n + 15) // 16 * 16
dG = torch.zeros((R, ld), dtype=torch.int8, device="cuda"); dG[:rb, :n].copy_(torch.from_numpy(Gb))
dS = torch.zeros(((q + 4) * R,), dtype=torch.float64, device="cuda")
dK = torch.zeros((R * R,), dtype=torch.float64, device="cuda")
dR = torch.from_numpy(np.ascontiguousarray(tester.R)).cuda()
du = torch.from_numpy(np.ascontiguousarray(tester.u)).cuda()
dA = torch.from_numpy(words.view(np.int32)).cuda()
ld1, ldm = FINISH_HEAD + rho.size, FINISH_HEAD + rho.size + TAIL
dO1 = torch.zeros((R * ld1,), dtype=torch.float64, device="cuda")
dOm = torch.zeros((R * NA * NF * ldm,), dtype=torch.float64, device="cuda")
torch.cuda.synchronize()


def gram():
    fac.scan_block_gram_dev(vp(dG.data_ptr()), ld, rb, vp(tester.dQ.data_ptr()), q, vp(dS.data_ptr()), vp(dK.data_ptr()))


def scalar_block():
    """The Gram block and scilmm_sets_finish_dev behind it: (prep, sweep, statistics + Gram, k_sets_finish) in ms."""
    gram()
    fac.sets_finish_dev(rb, q, vp(dS.data_ptr()), vp(dK.data_ptr()), vp(dR.data_ptr()), vp(du.data_ptr()), q - 1, ns, start, 0, None, 0, rho,
                        vp(dO1.data_ptr()), ld1, None)
    sym.sync()
    return sym.scan_timing() + (sym.sets_finish_timing(),)


def masks_block():
    """The Gram block and scilmm_sets_finish_masks_dev behind it: (prep, sweep, statistics + Gram, k_sets_finish_masks) in ms."""
    gram()
    fac.sets_finish_masks_dev(rb, q, vp(dS.data_ptr()), vp(dK.data_ptr()), vp(dR.data_ptr()), vp(du.data_ptr()), q - 1, ns, start, 0, None, 0,
                              rho, vp(dA.data_ptr()), NA, cuts, args.acat_mac, vp(dOm.data_ptr()), ldm)
    sym.sync()
    return sym.scan_timing() + (sym.sets_finish_masks_timing(),)


def summary(v):
    v = np.asarray(v, dtype=float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "iqr": float(np.percentile(v, 75) - np.percentile(v, 25))}


t1, tm = [], []
for it in range(3 + args.blocks):                     # three rounds of warm-up of both shapes, then the timed rounds
    ms = scalar_block()
    if it >= 3: t1.append(ms)
    ms = masks_block()
    if it >= 3: tm.append(ms)
a1, am = np.asarray(t1), np.asarray(tm)
fin1, finm, sweep = float(np.median(a1[:, 3])), float(np.median(am[:, 3])), float(np.median(a1[:, 1]))
rec = {"workload": args.workload, "n": int(n), "nnzL": int(sym.info().nnzL), "blocks": args.blocks, "sigma2": S2, "r": R, "markers": int(rb),
       "n_sets": ns, "set_sizes": [int(s) for s in sizes], "n_rho": int(rho.size), "n_ann": NA, "max_maf": [float(c) for c in cuts],
       "acat_mac": args.acat_mac, "workgroups": ns * NA * NF,
       "timer": "HIP events on the engine's stream, one block with its finish per synchronise; three warm-up rounds of both shapes, "
                "then alternating rounds",
       "scalar": {"gram_block_ms": summary(a1[:, :3].sum(axis=1)), "sweep_ms": summary(a1[:, 1]), "sets_finish_ms": summary(a1[:, 3]),
                  "total_ms": summary(a1.sum(axis=1))},
       "masks": {"gram_block_ms": summary(am[:, :3].sum(axis=1)), "sets_finish_masks_ms": summary(am[:, 3]), "total_ms": summary(am.sum(axis=1)),
                 "masks_finish_over_one_scalar_finish": finm / fin1, "masks_finish_over_nine_scalar_finishes": finm / (NA * NF * fin1),
                 "masks_block_over_nine_scalar_blocks": float(np.median(am.sum(axis=1)) / (NA * NF * np.median(a1.sum(axis=1)))),
                 "sweeps_avoided_ms": (NA * NF - 1) * sweep}}
# the cells' members, from the host side: what VariantSetTest keeps, the annotation, maf <= cutoff
obs = Gb >= 0
n_obs = obs.sum(axis=1)
with np.errstate(invalid="ignore", divide="ignore"):
    mean = np.where(obs, Gb, 0).sum(axis=1) / n_obs
    maf = maf_of(mean)
kept = (n_obs > 0) & np.array([np.unique(g[g >= 0]).size > 1 for g in Gb])
cells = {(a, f): [s[kept[s] & ann[s, a] & (maf[s] <= cuts[f])] for s in local] for a in range(NA) for f in range(NF)}
rec["cell_sizes"] = {"%d,%d" % k: [int(c.size) for c in v] for k, v in cells.items()}
masked = tester.masks(ann, max_maf=cuts, acat_mac=args.acat_mac)
ts = []
for it in range(4):
    t0 = time.perf_counter(); out = masked(Gb, local, skato=True)
    ts.append(time.perf_counter() - t0)
wall = {"masked_ms_per_set": 1e3 * float(np.median(ts[1:])) / ns, "masked_ms": 1e3 * float(np.median(ts[1:]))}
ts, nine = [], None
for it in range(4):
    t0 = time.perf_counter()
    nine = {k: (tester(Gb, [c for c in v if c.size], skato=True, finish="device") if any(c.size for c in v) else None)
            for k, v in cells.items()}
    ts.append(time.perf_counter() - t0)
wall["nine_calls_ms_per_set"] = 1e3 * float(np.median(ts[1:])) / ns
wall["nine_calls_ms"] = 1e3 * float(np.median(ts[1:]))
ts = []
for it in range(4):
    t0 = time.perf_counter(); tester(Gb, local, skato=True, finish="device")
    ts.append(time.perf_counter() - t0)
wall["one_scalar_call_ms"] = 1e3 * float(np.median(ts[1:]))
rec["wall"] = wall
stat, pv, same = 0.0, 0.0, True
for (a, f), v in cells.items():
    live = [i for i, c in enumerate(v) if c.size]
    same = same and np.array_equal(out["n_used"][:, a, f], [c.size for c in v])
    if not live:
        continue
    ref = nine[(a, f)]
    for k in ("burden_beta", "burden_se", "burden_chi2", "skat_q"):
        stat = max(stat, float(np.nanmax(np.abs(out[k][live, a, f] - ref[k]) / np.abs(ref[k]))))
    for k in ("burden_p", "skat_p", "skato_p", "skato_pmin"):
        pv = max(pv, float(np.nanmax(np.abs(out[k][live, a, f] - ref[k]) / np.abs(ref[k]))))
    same = same and np.array_equal(out["skato_rho"][live, a, f], ref["skato_rho"])
rec["check_cells_rel_diff"] = {"statistics": stat, "p_values": pv, "same_n_used_and_rho": bool(same)}
rec["acato_p"] = [float(v) for v in out["acato_p"]]
print(json.dumps(rec))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
