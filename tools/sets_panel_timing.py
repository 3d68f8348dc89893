"""HIP-event times of the variant-set finish over a phenotype panel (scilmm_sets_finish_panel_dev: k_sets_spectra |
k_sets_panel_tail, read through scilmm_sets_finish_panel_timing) behind a Gram block and its scilmm_scan_panel_dev, at a seeded
bench cohort: the first packed block of tools/sets_timing.py --finish (512 rare markers in consecutive sets of 2 .. 17, packed
into 128-wide blocks: a dozen sets), SKAT-O on the default grid, for panels of T = 1, 64 and 1024 traits.  In the same rounds the
yardstick: the same block through scilmm_sets_finish_dev (one trait), which this work leaves as it was.  Three warm-up rounds of
every shape, then alternating rounds; medians and IQR.  --groups times the trait-group sizes of the tail kernel side by side
(SCILMM_SETS_PANEL_GROUP, read per call; 0 = the engine's own choice); the numbers do not depend on it, and the tool checks that
they do not.  Wall times: panel(G, sets, skato=True) per (set, trait) and tester(G, sets, skato=True, finish="device") per set, the
median of three calls after one.  A cross-check: column 0 of every panel is the tester's own phenotype, so its rows must agree
with the scalar finish (1e-9 on the statistics, 1e-6 on the p-values).
  usage: sets_panel_timing.py 100k [--blocks 20] [--traits 1,64,1024] [--groups 0,1,2,4,8,16,32] [--out profiles/sets_panel_100k.json]"""
import argparse, ctypes, json, os, sys, time
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
ap = argparse.ArgumentParser()
ap.add_argument("workload"); ap.add_argument("--blocks", type=int, default=20); ap.add_argument("--out", default=None)
ap.add_argument("--traits", default="1,64,1024"); ap.add_argument("--groups", default="0")
args = ap.parse_args()
import torch
from scilmm_amd import SparseCholesky, VariantSetTest
from scilmm_amd.sets import FINISH_HEAD, RHO_DEFAULT, pack_sets
vp = ctypes.c_void_p
R, S2, M = 128, [0.5, 0.5], 512
GROUP = "SCILMM_SETS_PANEL_GROUP"
traits = [int(t) for t in args.traits.split(",")]
groups = [int(g) for g in args.groups.split(",")]
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
rho = np.asarray(RHO_DEFAULT)
ld = (n + 15) // 16 * 16
dG = torch.zeros((R, ld), dtype=torch.int8, device="cuda"); dG[:rb, :n].copy_(torch.from_numpy(np.ascontiguousarray(Gm[rows])))
dS = torch.zeros(((q + 4) * R,), dtype=torch.float64, device="cuda")
dK = torch.zeros((R * R,), dtype=torch.float64, device="cuda")
dR = torch.from_numpy(np.ascontiguousarray(tester.R)).cuda()
du = torch.from_numpy(np.ascontiguousarray(tester.u)).cuda()
ld_out = FINISH_HEAD + rho.size
dO1 = torch.zeros((R * ld_out,), dtype=torch.float64, device="cuda")
gen = np.random.default_rng(1)
panels, dB, dH, dO = {}, {}, {}, {}
for T in traits:
    Y = Cv @ gen.standard_normal((Cv.shape[1], T)) + gen.standard_normal((n, T))
    Y[:, 0] = y                                       # column 0 = the tester's own phenotype: the cross-check below
    panels[T] = tester.set_traits(Y)
    dB[T] = torch.zeros((R * T,), dtype=torch.float64, device="cuda")
    dH[T] = torch.zeros((R * 4,), dtype=torch.float64, device="cuda")
    dO[T] = torch.zeros((R * T * 8,), dtype=torch.float64, device="cuda")
torch.cuda.synchronize()


def gram():
    fac.scan_block_gram_dev(vp(dG.data_ptr()), ld, rb, vp(tester.dQ.data_ptr()), q, vp(dS.data_ptr()), vp(dK.data_ptr()))


def scalar_block():
    """The Gram block and scilmm_sets_finish_dev behind it: (prep, sweep, statistics + Gram, k_sets_finish) in ms."""
    gram()
    fac.sets_finish_dev(rb, q, vp(dS.data_ptr()), vp(dK.data_ptr()), vp(dR.data_ptr()), vp(du.data_ptr()), q - 1, ns, start, 0, None, 0, rho,
                        vp(dO1.data_ptr()), ld_out, None)
    sym.sync()
    return sym.scan_timing() + (sym.sets_finish_timing(),)


def panel_block(T, group):
    """The Gram block, X'Y~ and the panel finish behind it: (prep, sweep, statistics + Gram, k_scan_panel, k_panel_fold,
    k_sets_spectra, k_sets_panel_tail) in ms."""
    p = panels[T].panel
    if group:
        os.environ[GROUP] = str(group)
    else:
        os.environ.pop(GROUP, None)
    gram()
    fac.scan_panel_dev(rb, vp(p.dY.data_ptr()), p.ld, T, vp(dB[T].data_ptr()), T)
    fac.sets_finish_panel_dev(rb, q, vp(dS.data_ptr()), vp(dK.data_ptr()), vp(dR.data_ptr()), q - 1, ns, start, 0, None, 0, rho,
                              vp(dB[T].data_ptr()), T, T, None, vp(dH[T].data_ptr()), vp(dO[T].data_ptr()))
    sym.sync()
    os.environ.pop(GROUP, None)
    return sym.scan_timing() + sym.panel_timing() + sym.sets_finish_panel_timing()


def summary(v):
    v = np.asarray(v, dtype=float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "iqr": float(np.percentile(v, 75) - np.percentile(v, 25))}


def finish_bits(T, group):
    """The panel finish alone, on what the last block and its X'Y~ left behind (the handle is not in deterministic mode: a block
    repeats its statistics to rounding only, so the bits of two finishes are compared on the SAME inputs): (head, rows)."""
    if group:
        os.environ[GROUP] = str(group)
    fac.sets_finish_panel_dev(rb, q, vp(dS.data_ptr()), vp(dK.data_ptr()), vp(dR.data_ptr()), q - 1, ns, start, 0, None, 0, rho,
                              vp(dB[T].data_ptr()), T, T, None, vp(dH[T].data_ptr()), vp(dO[T].data_ptr()))
    sym.sync()
    os.environ.pop(GROUP, None)
    return dH[T].cpu().numpy()[:ns * 4].copy(), dO[T].cpu().numpy()[:ns * T * 8].copy()


shapes = [(T, g) for T in traits for g in groups]
t, t1, bits = {k: [] for k in shapes}, [], {}
for it in range(3 + args.blocks):                     # three rounds of warm-up of every shape, then the timed rounds
    ms = scalar_block()
    if it >= 3: t1.append(ms)
    for k in shapes:
        ms = panel_block(*k)
        if it >= 3: t[k].append(ms)
scalar_block()                                        # dS, dK and dO1 of ONE block for everything below
for T in traits:
    p = panels[T].panel
    fac.scan_panel_dev(rb, vp(p.dY.data_ptr()), p.ld, T, vp(dB[T].data_ptr()), T)
    sym.sync()
    for g in groups:
        bits[(T, g)] = finish_bits(T, g)
a1 = np.asarray(t1)
rec = {"workload": args.workload, "n": int(n), "nnzL": int(sym.info().nnzL), "blocks": args.blocks, "sigma2": S2, "r": R, "markers": int(rb),
       "n_sets": ns, "set_sizes": [int(s) for s in sizes], "n_rho": int(rho.size),
       "timer": "HIP events on the engine's stream, one block (with its panel and its finish) per synchronise; three warm-up rounds of "
                "every shape, then alternating rounds",
       "scalar": {"gram_block_ms": summary(a1[:, :3].sum(axis=1)), "sets_finish_ms": summary(a1[:, 3]), "total_ms": summary(a1.sum(axis=1))},
       "panel": {}}
fin1 = float(np.median(a1[:, 3]))
scal = dO1.cpu().numpy()[:ns * ld_out].reshape(ns, ld_out)
for (T, g) in shapes:
    a = np.asarray(t[(T, g)])
    fin = a[:, 5] + a[:, 6]
    e = {"traits": T, "group": g or "engine", "gram_block_ms": summary(a[:, :3].sum(axis=1)), "scan_panel_ms": summary(a[:, 3] + a[:, 4]),
         "spectra_ms": summary(a[:, 5]), "tails_ms": summary(a[:, 6]), "panel_finish_ms": summary(fin), "total_ms": summary(a.sum(axis=1)),
         "tail_us_per_set_trait": float(1e3 * np.median(a[:, 6]) / (ns * T)),
         "panel_finish_over_T_scalar_finishes": float(np.median(fin) / (T * fin1)),
         "block_over_T_scalar_blocks": float(np.median(a.sum(axis=1)) / (T * np.median(a1.sum(axis=1))))}
    H, O_ = bits[(T, g)]
    H0, O0 = bits[(T, groups[0])]
    e["same_bits_as_first_group"] = bool(np.array_equal(H, H0, equal_nan=True) and np.array_equal(O_, O0, equal_nan=True))
    Hh, Oo = H.reshape(ns, 4), O_.reshape(ns, T, 8)[:, 0]
    stat = np.abs(np.c_[Oo[:, 0] / Hh[:, 1], Oo[:, 1], Oo[:, 2]] - scal[:, [1, 3, 4]]) / np.abs(scal[:, [1, 3, 4]])
    pv = np.abs(Oo[:, 3:6] - scal[:, 5:8]) / np.abs(scal[:, 5:8])
    e["check_col0_rel_diff"] = {"statistics": float(stat.max()), "p_values": float(pv.max()), "same_rho": bool(np.array_equal(Oo[:, 6], scal[:, 8]))}
    rec["panel"]["T%d_G%s" % (T, g or "engine")] = e
wall = {}
ts = []
for it in range(4):
    t0 = time.perf_counter(); tester(Gm[rows], [np.arange(a_, b_) for a_, b_ in zip(start[:-1], start[1:])], skato=True, finish="device")
    ts.append(time.perf_counter() - t0)
wall["scalar_device_ms_per_set"] = 1e3 * float(np.median(ts[1:])) / ns
for T in traits:
    ts = []
    for it in range(4):
        t0 = time.perf_counter(); panels[T](Gm[rows], [np.arange(a_, b_) for a_, b_ in zip(start[:-1], start[1:])], skato=True)
        ts.append(time.perf_counter() - t0)
    wall["panel_T%d_ms_per_set_trait" % T] = 1e3 * float(np.median(ts[1:])) / (ns * T)
rec["wall"] = wall
print(json.dumps(rec))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
