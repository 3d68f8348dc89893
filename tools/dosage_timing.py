"""HIP-event times (moments + dequantise | forward sweep | statistics) of one 128-wide marker-scan block from imputed dosages
(scilmm_scan_block_dosage_dev) in both element types, against the int8 block (scilmm_scan_block_dev) of the same markers
rounded to hard calls, at a seeded bench cohort: all shapes in the same run, alternating, after a warm-up of every shape.
Identity map and a shuffled map that lacks 5 % of the cohort (its int8 block takes the markers gathered on the host).
  usage: dosage_timing.py 100k|300k [--blocks 20] [--out profiles/dosage_100k.json]
No time here is a pass / fail condition; the figures of interest are prep_ms of each dosage form over prep_ms of the int8 block
of the same run, and each whole block over the int8 block."""
import argparse, ctypes, json, math, os, sys
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
ap = argparse.ArgumentParser()
ap.add_argument("workload"); ap.add_argument("--blocks", type=int, default=20); ap.add_argument("--out", default=None)
args = ap.parse_args()
import torch
from scilmm_amd import AssociationScan, SparseCholesky, _lib
from scilmm_amd.dosage import decode, encode
vp = ctypes.c_void_p
S2, r = [0.5, 0.5], 128
A, Cv, y = bench.build_problem(args.workload, 0)
n = A.shape[0]
scan = AssociationScan(SparseCholesky(), [A, sp.identity(n, format="csr")], S2, Cv, y, block=r)
sym, fac, q = scan.sym, scan.factor, scan.q
rng = np.random.default_rng(0)
# dosages around binomial calls, 2 % missing; the int8 block takes them rounded
D = np.clip(rng.binomial(2, rng.uniform(0.05, 0.5, r)[:, None], size=(r, n)) + 0.5 * (rng.beta(2.0, 2.0, size=(r, n)) - 0.5), 0.0, 2.0)
D[rng.random(D.shape) < 0.02] = np.nan
idx = rng.permutation(n).astype(np.int32)
idx[rng.choice(n, size=n // 20, replace=False)] = -1


def rounded(D):
    return np.where(np.isnan(D), -1, np.rint(D)).astype(np.int8)


def device_rows(a):
    """Rows on the device at a pitch that is a multiple of 16 bytes, as the Python interface lays them out: (tensor, ld)."""
    per = 16 // a.dtype.itemsize
    ld = (a.shape[1] + per - 1) // per * per
    host = np.zeros((a.shape[0], ld), dtype=a.dtype)
    host[:, :a.shape[1]] = a
    return torch.from_numpy(host.view(np.uint8)).cuda(), ld


Dmap = np.where(idx >= 0, D[:, np.maximum(idx, 0)], np.nan)                      # cohort order, for the int8 block of the map
bufs = {"int8": device_rows(rounded(D)), "u16": device_rows(encode(D)), "f32": device_rows(D.astype(np.float32)),
        "int8_map": device_rows(rounded(Dmap))}
dI = torch.from_numpy(idx).cuda()
names = ("int8", "u16", "f32", "int8_map", "u16_map", "f32_map")
dS = {k: torch.zeros(((q + 4) * r,), dtype=torch.float64, device="cuda") for k in names}
torch.cuda.synchronize()
Q = vp(scan.dQ.data_ptr())


def dosage(form, kind, mapped):
    buf, ld = bufs[form]
    out = vp(dS[form + ("_map" if mapped else "")].data_ptr())
    return lambda: fac.scan_block_dosage_dev(vp(buf.data_ptr()), kind, ld, n, vp(dI.data_ptr()) if mapped else None, r, Q, q, out)


def int8(form):
    buf, ld = bufs[form]
    return lambda: fac.scan_block_dev(vp(buf.data_ptr()), ld, r, Q, q, vp(dS[form].data_ptr()))


shapes = {"int8": int8("int8"), "u16": dosage("u16", _lib.DOSAGE_U16, False), "f32": dosage("f32", _lib.DOSAGE_F32, False),
          "int8_map": int8("int8_map"), "u16_map": dosage("u16", _lib.DOSAGE_U16, True), "f32_map": dosage("f32", _lib.DOSAGE_F32, True)}


def summary(v):
    v = np.asarray(v, dtype=float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "iqr": float(np.percentile(v, 75) - np.percentile(v, 25))}


t = {k: [] for k in shapes}
for it in range(3 + args.blocks):                     # three rounds of warm-up of every shape, then the timed rounds
    for k, f in shapes.items():
        f(); sym.sync()
        if it >= 3: t[k].append(sym.scan_timing())
rec = {"workload": args.workload, "n": int(n), "nnzL": int(sym.info().nnzL), "blocks": args.blocks, "sigma2": S2, "r": r,
       "timer": "HIP events on the engine's stream, one block per synchronise; three warm-up rounds of every shape, then "
                "alternating rounds", "block": {}}
for k in shapes:
    a = np.asarray(t[k]); tot = a.sum(axis=1)
    rec["block"][k] = {"prep_ms": summary(a[:, 0]), "sweep_ms": summary(a[:, 1]), "stats_ms": summary(a[:, 2]),
                       "total_ms": summary(tot), "markers_per_s": float(r / (np.median(tot) * 1e-3))}
for k in ("u16", "f32", "u16_map", "f32_map"):
    b = "int8_map" if k.endswith("_map") else "int8"
    rec["block"][k + "_over_" + b] = {
        "median_prep_ratio": float(rec["block"][k]["prep_ms"]["median"] / rec["block"][b]["prep_ms"]["median"]),
        "median_total_ratio": float(rec["block"][k]["total_ms"]["median"] / rec["block"][b]["total_ms"]["median"])}
# a check beside the times: n_obs of every form equals the host count, the uint16 mean is the exact quotient
S = {k: dS[k].cpu().numpy().reshape(q + 4, r) for k in names}
rec["n_obs_equal_host"] = bool(all(np.array_equal(S[k][0], np.isfinite(Dmap if k.endswith("_map") else D).sum(axis=1)) for k in names))
host_mean = [math.fsum(row[np.isfinite(row)]) / np.isfinite(row).sum() for row in decode(encode(D))]   # exactly rounded sums
rec["u16_mean_equals_host"] = bool(np.array_equal(S["u16"][1], host_mean))
print(json.dumps(rec))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
