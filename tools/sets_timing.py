"""HIP-event times of one 128-wide variant-set block (scilmm_scan_block_gram_dev: moments + dequantise | forward sweep |
statistics + Gram) against the plain marker-scan block of the same markers (scilmm_scan_block_dev) in the same run, at a seeded
bench cohort: three warm-up rounds of every shape, then alternating rounds; medians and IQRs.  The Gram kernel and its fold
run inside the statistics interval, so their time is the paired difference of that interval between the two blocks.
  usage: sets_timing.py 100k|300k [--blocks 20] [--out FILE] [--shapes 256:1,512:1,1024:1,2048:1,512:0]
--shapes times other slicings of k_scan_gram (<rows per slice>:<1 = LDS image, 0 = fragments from global memory>) side by
side in the same run; it needs a library built with `make DIAG=1` (SCILMM_HIP_LIB), which reads SCILMM_GRAM_SHAPE per call.
Reported per shape: Gram + fold time, its ratio to k_scan_stats + k_scan_fold on the same X, the bandwidth n * rp * 8 bytes /
time implies (against the 6.3 TB/s a streaming read achieves on this part), the block's total as a fraction of the plain
block's, and the agreement of X'X with the gg row and between shapes.
  usage: sets_timing.py 100k --finish [--out profiles/sets_finish_100k.json]
--finish times the finish of a block instead (scilmm_sets_finish_dev): 512 markers in consecutive sets of 2 .. 17 markers, packed
into 128-wide blocks, and a block that is one 128-marker set.  Per block: k_sets_finish by HIP events, with and without SKAT-O
(three warm-up rounds, 20 rounds, median and IQR), next to the block's forward sweep; and the wall time per set of the whole
call with finish="device" and finish="host", with and without skato, on the same packed sets (the median of three calls).
  usage: sets_timing.py 100k --binary [--out profiles/sets_spa_100k.json]
--binary times one block of a dozen sets (3 .. 18 rare markers, 128 together) as the binary-trait tests queue it
(scilmm_amd.glmm.BinarySetTest, finish="device"): the Gram block, k_scan_spa of its markers, k_sets_spa and the scaled
k_sets_finish with SKAT-O, each by its own HIP events, at a null point of a simulated 5 % phenotype, at the default cutoff 2 and
at cutoff 0 (every marker and every burden saddlepointed: the most the block can cost); next to it, in the same run and on the
same sets, the quantitative Gram block + k_sets_finish, and the ratio of the two totals.
  usage: sets_timing.py 100k --wide 256,1024 [--out profiles/sets_wide_100k.json]
--wide times one set of k rare markers per width as VariantSetTest(..., max_markers=k) queues it, sub-block by sub-block: the Gram
blocks (sweeps with statistics and Gram, scilmm_scan_timing) and the panels (scilmm_panel_timing) by their HIP events, the
keeps as the wall time of 20 keeps queued behind one block over 20 (k_scan_keep has no events of its own); the same markers as
ceil(k / 128) separate 128-marker sets without max_markers (the Gram blocks alone), in alternating rounds of the same run; the
ratio of the two device times; the panel of the last block against its own kept copy next to its Gram matrix; the host finish
of the assembled set with and without SKAT-O, and the wall time of the whole call.  One warm-up round, then --blocks rounds (use
--blocks 5).
  usage: sets_timing.py 100k --wide-finish 256,1024 [--host-reps 3] [--out profiles/sets_wide_finish_100k.json]
--wide-finish times the finish of one set of k rare markers per width (scilmm_sets_finish_wide_dev): the
sub-blocks are queued once as VariantSetTest(..., max_markers=k, finish="wide") queues them and leave their pieces on the device;
then, per round, the finish with SKAT-O and without, its four phases by HIP events (prep + form | reduction | eigenvalues |
tails); the host finish of the same set in the same run (--host-reps timings each; 0 leaves it out), the deviation of the device's
row from the host's, and the wall time of the whole call with finish="wide" and finish="host".  One warm-up round, then --blocks
rounds.
  usage: sets_timing.py 100k --binary-wide 256,1024 [--blocks 5] [--out profiles/sets_binary_wide_100k.json]
--binary-wide times one set of k rare markers per width as the binary-trait tests queue it (scilmm_amd.glmm.BinaryWideSetTest,
finish="wide", SKAT-O, cutoff 2), at a null point of a simulated 5 % phenotype: per sub-block the Gram block,
k_scan_spa of its markers, k_sets_collapse and the panel by their HIP events (the keeps as for --wide), then
scilmm_sets_spa_wide_dev by phase and the scaled wide finish by phase; the same markers as ceil(k / 128) separate 128-marker binary
sets (Gram block, k_scan_spa, k_sets_spa, the scaled k_sets_finish), in alternating rounds of the same run; the ratio of the two
device times, the share of the panels and keeps, and every collapse against the k_scan_spa of its own sub-block.  One warm-up
round, then --blocks rounds."""
import argparse, ctypes, json, os, sys
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
ap = argparse.ArgumentParser()
ap.add_argument("workload"); ap.add_argument("--blocks", type=int, default=20); ap.add_argument("--out", default=None)
ap.add_argument("--shapes", default=None)
ap.add_argument("--finish", action="store_true")
ap.add_argument("--binary", action="store_true")
ap.add_argument("--wide", default=None)
ap.add_argument("--wide-finish", dest="wide_finish", default=None)
ap.add_argument("--binary-wide", dest="binary_wide", default=None)
ap.add_argument("--host-reps", dest="host_reps", type=int, default=3)
args = ap.parse_args()
import torch
from scilmm_amd import SparseCholesky, VariantSetTest
vp = ctypes.c_void_p
R, S2, HBM = 128, [0.5, 0.5], 6.3e12
A, Cv, y = bench.build_problem(args.workload, 0)
n = A.shape[0]
tester = VariantSetTest(SparseCholesky(), [A, sp.identity(n, format="csr")], S2, Cv, y, block=R)
sym, fac, q = tester.sym, tester.factor, tester.q
rng = np.random.default_rng(0)
G = rng.binomial(2, rng.uniform(0.005, 0.05, R)[:, None], size=(R, n)).astype(np.int8)       # rare variants, 2 % missing
G[rng.random(G.shape) < 0.02] = -1
ld = (n + 15) // 16 * 16
dG = torch.zeros((R, ld), dtype=torch.int8, device="cuda"); dG[:, :n].copy_(torch.from_numpy(G))
dS = torch.zeros(((q + 4) * R,), dtype=torch.float64, device="cuda")
dK = torch.zeros((R * R,), dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
shapes = ["default"] + ([s for s in args.shapes.split(",") if s] if args.shapes else [])


def summary(v):
    v = np.asarray(v, dtype=float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "iqr": float(np.percentile(v, 75) - np.percentile(v, 25))}


def finish_leg():
    import time
    from scilmm_amd.sets import FINISH_HEAD, RHO_DEFAULT, pack_sets
    M = 512
    Gm = rng.binomial(2, rng.uniform(0.005, 0.05, M)[:, None], size=(M, n)).astype(np.int8)
    Gm[rng.random(Gm.shape) < 0.02] = -1
    sets, at = [], 0
    while at < M:
        k = min(int(rng.integers(2, 18)), M - at)
        sets.append(np.arange(at, at + k))
        at += k
    packed = pack_sets([s.size for s in sets], R)
    rho = np.asarray(RHO_DEFAULT)
    dR = torch.from_numpy(np.ascontiguousarray(tester.R)).cuda()
    du = torch.from_numpy(np.ascontiguousarray(tester.u)).cuda()
    dO = torch.zeros((R * (FINISH_HEAD + rho.size),), dtype=torch.float64, device="cuda")
    rec = {"workload": args.workload, "n": int(n), "r": R, "markers": M, "n_sets": len(sets), "set_sizes": [int(s.size) for s in sets],
           "blocks": [], "timer": "HIP events around k_sets_finish, one call per synchronise; three warm-up rounds, then %d rounds" % args.blocks}
    shapes_ = [("packed block %d" % b, np.concatenate([sets[i] for i in mem]), [sets[i].size for i in mem]) for b, mem in enumerate(packed)]
    shapes_.append(("one set of 128", np.arange(R), [R]))
    for name, rows, sizes in shapes_:
        rb = rows.size
        dG[:rb, :n].copy_(torch.from_numpy(np.ascontiguousarray(Gm[rows])))
        torch.cuda.synchronize()
        start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        fac.scan_block_gram_dev(vp(dG.data_ptr()), ld, rb, vp(tester.dQ.data_ptr()), q, vp(dS.data_ptr()), vp(dK.data_ptr())); sym.sync()
        block_ms = sym.scan_timing()
        t = {"skato": [], "burden_skat": []}
        for it in range(3 + args.blocks):
            for key, grid in (("skato", rho), ("burden_skat", rho[:0])):
                fac.sets_finish_dev(rb, q, vp(dS.data_ptr()), vp(dK.data_ptr()), vp(dR.data_ptr()), vp(du.data_ptr()), q - 1, len(sizes), start,
                                    0, None, 0, grid, vp(dO.data_ptr()), FINISH_HEAD + rho.size, None)
                sym.sync()
                if it >= 3: t[key].append(sym.sets_finish_timing())
        rec["blocks"].append({"block": name, "markers": int(rb), "sets": len(sizes), "largest_set": int(max(sizes)),
                              "gram_block_ms": {"prep": block_ms[0], "sweep": block_ms[1], "stats_gram": block_ms[2]},
                              "finish_skato_ms": summary(t["skato"]), "finish_burden_skat_ms": summary(t["burden_skat"])})
    wall = {}
    for fin in ("device", "host"):
        for sk in (False, True):
            ts = []
            for it in range(4):
                t0 = time.perf_counter()
                tester(Gm, sets, skato=sk, finish=fin)
                ts.append(time.perf_counter() - t0)
            wall["%s%s" % (fin, "+skato" if sk else "")] = {"ms_per_set_median_of_3": 1e3 * float(np.median(ts[1:])) / len(sets),
                                                               "ms_per_call": [1e3 * v for v in ts[1:]]}
    rec["wall"] = wall
    return rec


def binary_leg():
    from scilmm_amd import LogisticMixedModel
    from scilmm_amd.binary_sets import BSPA_ROWLEN
    from scilmm_amd.glmm import SPA_ROWS, logistic_irls
    from scilmm_amd.sets import FINISH_HEAD, RHO_DEFAULT
    sizes = [3, 5, 8, 8, 10, 10, 11, 12, 13, 14, 16, 18]
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    assert start[-1] == R
    rho, ld_out = np.asarray(RHO_DEFAULT), FINISH_HEAD + len(RHO_DEFAULT)
    new = lambda k: torch.zeros((k,), dtype=torch.float64, device="cuda")
    dP, dB, dV, dO = new(SPA_ROWS * R), new(BSPA_ROWLEN * R), new(R), new(R * ld_out)
    pG, pS, pK, pP, pB, pV, pO = (vp(d.data_ptr()) for d in (dG, dS, dK, dP, dB, dV, dO))
    rec = {"workload": args.workload, "n": int(n), "r": R, "set_sizes": sizes, "n_rho": int(rho.size), "prevalence": 0.05,
           "timer": "HIP events around each kernel, the block's calls queued behind each other, one synchronise per round; three "
                    "warm-up rounds, then %d rounds" % args.blocks}
    # the quantitative block on the same sets: Gram + finish
    dR, du = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (tester.R, tester.u))
    t = []
    for it in range(3 + args.blocks):
        fac.scan_block_gram_dev(pG, ld, R, vp(tester.dQ.data_ptr()), q, pS, pK)
        fac.sets_finish_dev(R, q, pS, pK, vp(dR.data_ptr()), vp(du.data_ptr()), q - 1, len(sizes), start, 0, None, 0, rho, pO, ld_out, None)
        sym.sync()
        if it >= 3: t.append(list(sym.scan_timing()) + [sym.sets_finish_timing()])
    a = np.asarray(t)
    quant = float(np.median(a.sum(axis=1)))
    rec["quantitative"] = {"gram_block_ms": summary(a[:, :3].sum(axis=1)), "finish_ms": summary(a[:, 3]), "total_ms": summary(a.sum(axis=1))}
    # the binary block: a null point at the covariate-only fit, a random effect drawn on top
    yb = (rng.random(n) < 0.05).astype(np.float64)
    model = LogisticMixedModel(SparseCholesky(), [A], Cv, yb)
    null = model.null_at([0.5], logistic_irls(model.covariates, yb), 0.3 * rng.standard_normal(n))
    rec["binary"] = {}
    for cutoff in (2.0, 0.0):
        bt = null.sets(block=R, cutoff=cutoff)
        bf, bs, c = bt.factor, bt.sym, bt.c
        tail = (vp(bt.dR.data_ptr()), vp(bt.du.data_ptr()), vp(bt.dmu.data_ptr()), vp(bt.dC.data_ptr()), c, vp(bt.dMinv.data_ptr()), cutoff, pP)
        t = []
        for it in range(3 + args.blocks):
            bf.scan_block_gram_dev(pG, ld, R, vp(bt.dQ.data_ptr()), bt.q, pS, pK)
            bf.scan_spa_dev(pG, ld, R, pS, *tail)
            bf.sets_spa_dev(pG, ld, R, pS, pK, *(tail + (len(sizes), start, 0, None, pB, pV)))
            bf.sets_finish_scaled_dev(R, bt.q, pS, pK, vp(bt.dR.data_ptr()), vp(bt.du.data_ptr()), c, len(sizes), start, 0, None, 0, rho, pO,
                                      ld_out, None, pV)
            bs.sync()
            if it >= 3: t.append(list(bs.scan_timing()) + [bs.spa_timing(), bs.sets_spa_timing(), bs.sets_finish_timing()])
        b = np.asarray(t)
        P = dP.cpu().numpy().reshape(SPA_ROWS, R)
        Bs = dB.cpu().numpy()[:BSPA_ROWLEN * len(sizes)].reshape(len(sizes), BSPA_ROWLEN)
        tot = summary(b.sum(axis=1))
        rec["binary"]["cutoff_%g" % cutoff] = {
            "gram_block_ms": summary(b[:, :3].sum(axis=1)), "scan_spa_ms": summary(b[:, 3]), "sets_spa_ms": summary(b[:, 4]),
            "scaled_finish_ms": summary(b[:, 5]), "total_ms": tot, "total_over_quantitative": tot["median"] / quant,
            "markers_saddlepointed": int(np.sum(P[6] > 0)), "burdens_saddlepointed": int(np.sum(Bs[:, 6] > 0)),
            "sets_with_an_adjusted_marker": int(np.sum(Bs[:, 12] > 0)), "sets_at_the_burden_floor": int(np.sum(Bs[:, 11] > 1.0))}
        del bt
    return rec


def wide_leg(widths):
    import time
    from scilmm_amd import sets as mod
    bp = R
    rec = {"workload": args.workload, "n": int(n), "block": R, "widths": {},
           "timer": "HIP events of the Gram blocks and the panels, one sub-block per synchronise; keeps: wall time of 20 queued keeps / 20; "
                    "one warm-up round, then %d alternating rounds of the wide set and of its sub-blocks as separate sets" % args.blocks}
    for k in widths:
        B = -(-k // R)
        ldw = (B - 1) * bp
        Gm = rng.binomial(2, rng.uniform(0.005, 0.05, k)[:, None], size=(k, n)).astype(np.int8)
        Gm[rng.random(Gm.shape) < 0.02] = -1
        store = torch.empty((n * ldw,), dtype=torch.float64, device="cuda")
        dX = torch.empty((R * ldw,), dtype=torch.float64, device="cuda")
        pS, pK, pQ = vp(dS.data_ptr()), vp(dK.data_ptr()), vp(tester.dQ.data_ptr())

        def load(b):
            sub = np.ascontiguousarray(Gm[b * R:(b + 1) * R])
            dG[:sub.shape[0], :n].copy_(torch.from_numpy(sub))
            torch.cuda.synchronize()
            return sub.shape[0]

        t_wide, t_base, Ss, Gs, Xs = [], [], [], [], []
        for it in range(1 + args.blocks):
            gram_ms = panel_ms = 0.0
            for b in range(B):                                   # the wide set, as VariantSetTest._block_wide queues it
                rb = load(b)
                fac.scan_block_gram_dev(vp(dG.data_ptr()), ld, rb, pQ, q, pS, pK)
                if b > 0: fac.scan_panel_dev(rb, vp(store.data_ptr()), ldw, b * bp, vp(dX.data_ptr()), b * bp)
                if b < B - 1: fac.scan_block_keep_dev(rb, vp(store.data_ptr()), ldw, b * bp)
                sym.sync()
                gram_ms += float(sum(sym.scan_timing()))
                if b > 0: panel_ms += float(sum(sym.panel_timing()))
                if it == 0:
                    Ss.append(dS[:(q + 4) * rb].cpu().numpy().reshape(q + 4, rb)); Gs.append(dK[:rb * rb].cpu().numpy().reshape(rb, rb))
                    if b > 0: Xs.append(dX[:rb * b * bp].cpu().numpy().reshape(rb, b * bp))
            base_ms = 0.0
            for b in range(B):                                   # the same markers as separate sets: the Gram blocks alone
                rb = load(b)
                fac.scan_block_gram_dev(vp(dG.data_ptr()), ld, rb, pQ, q, pS, pK); sym.sync()
                base_ms += float(sum(sym.scan_timing()))
            if it >= 1:
                t_wide.append((gram_ms, panel_ms)); t_base.append(base_ms)
        keeps = []
        for it in range(4):                                      # the last block is still in X: 20 keeps of it behind each other
            sym.sync(); t0 = time.perf_counter()
            for _ in range(20): fac.scan_block_keep_dev(rb, vp(store.data_ptr()), ldw, 0)
            sym.sync(); keeps.append(1e3 * (time.perf_counter() - t0) / 20)
        keep_ms = float(np.median(keeps[1:])) * (B - 1)
        tp = (rb + 15) // 16 * 16                                # the block against its own kept copy: its Gram matrix again
        fac.scan_panel_dev(rb, vp(store.data_ptr()), ldw, tp, vp(dX.data_ptr()), tp); sym.sync()
        own = dX[:rb * tp].cpu().numpy().reshape(rb, tp)[:, :rb]
        Kb = dK[:rb * rb].cpu().numpy().reshape(rb, rb)
        own_err = float(np.abs(own - Kb).max() / np.abs(Kb).max())
        a = np.asarray(t_wide)
        wide_ms = float(np.median(a.sum(axis=1))) + keep_ms
        S, K = mod.assemble_wide(Ss, Gs, Xs, bp)
        host = {}
        for key, grid in (("burden_skat", None), ("skato", mod.check_rho(None))):
            out = {kk: np.full(1, np.nan) for kk in mod.KEYS + mod.SKATO_KEYS[:3]}
            out["n_used"] = np.zeros(1, dtype=np.int64); out["skato_p_rho"] = np.full((1, len(mod.RHO_DEFAULT)), np.nan)
            t0 = time.perf_counter()
            tester._one_set(out, 0, S, K, "beta", mod.mixture_sf_saddlepoint, grid, "saddlepoint")
            host[key + "_ms"] = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        tester(Gm, [np.arange(k)], max_markers=k)
        call_ms = 1e3 * (time.perf_counter() - t0)
        rec["widths"][str(k)] = {
            "sub_blocks": B, "store_bytes": int(n) * ldw * 8,
            "wide_device_ms": {"sweeps_with_gram": summary(a[:, 0]), "panels": summary(a[:, 1]), "keeps": keep_ms,
                               "keep_ms_each_of_20_queued": summary(keeps[1:]), "total": wide_ms},
            "separate_sets_device_ms": summary(t_base), "wide_over_separate": wide_ms / float(np.median(t_base)),
            "host_finish_ms": host, "host_share_burden_skat": host["burden_skat_ms"] / (host["burden_skat_ms"] + wide_ms),
            "host_share_skato": host["skato_ms"] / (host["skato_ms"] + wide_ms), "whole_call_wall_ms": call_ms,
            "symmetric_bits": bool(np.array_equal(K, K.T)), "panel_of_kept_copy_vs_gram_rel_err": own_err}
        del store, dX
    return rec


def wide_finish_leg(widths):
    import time
    from scilmm_amd import sets as mod
    bp = R
    rho = mod.check_rho(None)
    rec = {"workload": args.workload, "n": int(n), "block": R, "widths": {},
           "timer": "HIP events of scilmm_sets_finish_wide_dev, one call per synchronise; one warm-up round, then %d rounds; the host "
                    "finish: perf_counter around VariantSetTest._one_set, %d times" % (args.blocks, args.host_reps)}
    dR, du = torch.from_numpy(np.ascontiguousarray(tester.R)).cuda(), torch.from_numpy(np.ascontiguousarray(tester.u)).cuda()
    for k in widths:
        B = -(-k // R)
        ldw = max(B - 1, 1) * bp
        Gm = rng.binomial(2, rng.uniform(0.005, 0.05, k)[:, None], size=(k, n)).astype(np.int8)
        Gm[rng.random(Gm.shape) < 0.02] = -1
        store = torch.empty((n * ldw,), dtype=torch.float64, device="cuda")
        dSa = torch.empty((B * (q + 4) * R,), dtype=torch.float64, device="cuda")
        dKa = torch.empty((B * R * R,), dtype=torch.float64, device="cuda")
        dXa = torch.empty((B * R * ldw,), dtype=torch.float64, device="cuda")
        dO = torch.empty((mod.FINISH_HEAD + rho.size,), dtype=torch.float64, device="cuda")
        pQ = vp(tester.dQ.data_ptr())
        sweeps_ms, Ss, Gs, Xs = 0.0, [], [], []
        for b in range(B):                                       # the sub-blocks, as VariantSetTest._block_wide_device queues them
            sub = np.ascontiguousarray(Gm[b * R:(b + 1) * R])
            rb = sub.shape[0]
            dG[:rb, :n].copy_(torch.from_numpy(sub)); torch.cuda.synchronize()
            fac.scan_block_gram_dev(vp(dG.data_ptr()), ld, rb, pQ, q, vp(dSa.data_ptr() + 8 * b * (q + 4) * R), vp(dKa.data_ptr() + 8 * b * R * R))
            if b > 0: fac.scan_panel_dev(rb, vp(store.data_ptr()), ldw, b * bp, vp(dXa.data_ptr() + 8 * b * R * ldw), ldw)
            if b < B - 1: fac.scan_block_keep_dev(rb, vp(store.data_ptr()), ldw, b * bp)
            sym.sync()
            sweeps_ms += float(sum(sym.scan_timing())) + (float(sum(sym.panel_timing())) if b > 0 else 0.0)
            Ss.append(dSa[b * (q + 4) * R:b * (q + 4) * R + (q + 4) * rb].cpu().numpy().reshape(q + 4, rb))
            Gs.append(dKa[b * R * R:b * R * R + rb * rb].cpu().numpy().reshape(rb, rb))
            if b > 0: Xs.append(dXa[b * R * ldw:(b * R + rb) * ldw].cpu().numpy().reshape(rb, ldw)[:, :b * bp])
        phases = {"skato": [], "burden_skat": []}
        rows = {}
        for it in range(1 + args.blocks):
            for key, grid in (("skato", rho), ("burden_skat", np.empty(0))):
                fac.sets_finish_wide_dev(k, R, q, vp(dSa.data_ptr()), vp(dKa.data_ptr()), vp(dXa.data_ptr()) if B > 1 else None, ldw if B > 1 else 0,
                                         vp(dR.data_ptr()), vp(du.data_ptr()), q - 1, 0, None, 0, grid, vp(dO.data_ptr()), None)
                sym.sync()
                if it >= 1: phases[key].append(sym.sets_finish_wide_timing())
                rows[key] = dO.cpu().numpy().copy()
        dev = {}
        for key, v in phases.items():
            a = np.asarray(v)
            dev[key] = {"prep_form_ms": summary(a[:, 0]), "reduction_ms": summary(a[:, 1]), "eigenvalues_ms": summary(a[:, 2]),
                        "tails_ms": summary(a[:, 3]), "total_ms": summary(a.sum(axis=1))}
        host, dev_vs_host = {}, None
        if args.host_reps > 0:
            S, K = mod.assemble_wide(Ss, Gs, Xs, bp)
            for key, grid in (("burden_skat", None), ("skato", rho)):
                t = []
                for _ in range(args.host_reps):
                    out = {kk: np.full(1, np.nan) for kk in mod.KEYS + mod.SKATO_KEYS[:3]}
                    out["n_used"] = np.zeros(1, dtype=np.int64); out["skato_p_rho"] = np.full((1, rho.size), np.nan)
                    t0 = time.perf_counter()
                    tester._one_set(out, 0, S, K, "beta", mod.mixture_sf_saddlepoint, grid, "saddlepoint")
                    t.append(1e3 * (time.perf_counter() - t0))
                host[key + "_ms"] = summary(t)
            h = np.r_[out["skat_p"][0], out["skato_p"][0], out["skato_pmin"][0], out["skato_p_rho"][0]]
            d = np.r_[rows["skato"][5:8], rows["skato"][mod.FINISH_HEAD:]]
            dev_vs_host = {"worst_rel_dev_of_a_p_value": float(np.max(np.abs(d - h) / np.abs(h))), "skat_q_rel_dev": float(abs(rows["skato"][4] - out["skat_q"][0]) / out["skat_q"][0]),
                           "same_rho": bool(rows["skato"][8] == out["skato_rho"][0]), "n_used": int(rows["skato"][0]), "flags": int(rows["skato"][9]),
                           "skato_p": float(rows["skato"][6])}
        calls = {}
        for fin, reps in (("wide", 3), ("host", min(3, args.host_reps))):
            t = []
            for _ in range(reps):
                t0 = time.perf_counter()
                tester(Gm, [np.arange(k)], max_markers=k, skato=True, finish=fin)
                t.append(1e3 * (time.perf_counter() - t0))
            if t: calls[fin] = summary(t)
        rec["widths"][str(k)] = {"sub_blocks": B, "sweeps_and_panels_device_ms": sweeps_ms, "wide_finish_device_ms": dev, "host_finish_ms": host,
                                 "device_row_vs_host_row": dev_vs_host, "whole_call_wall_ms_skato": calls}
        del store, dSa, dKa, dXa
    return rec


def binary_wide_leg(widths):
    import time
    from scilmm_amd import LogisticMixedModel
    from scilmm_amd.binary_sets import BSPA_ROWLEN
    from scilmm_amd.glmm import SPA_ROWS, logistic_irls
    from scilmm_amd.sets import FINISH_HEAD, RHO_DEFAULT
    bp, cutoff = R, 2.0
    rho, ld_out = np.asarray(RHO_DEFAULT), FINISH_HEAD + len(RHO_DEFAULT)
    yb = (rng.random(n) < 0.05).astype(np.float64)
    model = LogisticMixedModel(SparseCholesky(), [A], Cv, yb)
    null = model.null_at([0.5], logistic_irls(model.covariates, yb), 0.3 * rng.standard_normal(n))
    bt = null.sets(block=R, cutoff=cutoff, max_markers=max(widths))
    bf, bs, c, bq = bt.factor, bt.sym, bt.c, bt.q
    nullp = (vp(bt.dR.data_ptr()), vp(bt.du.data_ptr()), vp(bt.dmu.data_ptr()), vp(bt.dC.data_ptr()), c, vp(bt.dMinv.data_ptr()), cutoff)
    pQ = vp(bt.dQ.data_ptr())
    new = lambda m: torch.zeros((m,), dtype=torch.float64, device="cuda")
    rec = {"workload": args.workload, "n": int(n), "block": R, "cutoff": cutoff, "prevalence": 0.05, "n_rho": int(rho.size), "widths": {},
           "timer": "HIP events of every call, one sub-block per synchronise; keeps: wall time of 20 queued keeps / 20; one warm-up "
                    "round, then %d alternating rounds of the wide set and of its sub-blocks as separate narrow binary sets" % args.blocks}
    for k in widths:
        B = -(-k // R)
        ldw = (B - 1) * bp
        Gm = rng.binomial(2, rng.uniform(0.005, 0.05, k)[:, None], size=(k, n)).astype(np.int8)
        Gm[rng.random(Gm.shape) < 0.02] = -1
        store, dSa, dKa, dXa, dPa = new(n * ldw), new(B * (bq + 4) * R), new(B * R * R), new(B * R * ldw), new(B * SPA_ROWS * R)
        dg, dBw, dVw, dOw = new(n), new(BSPA_ROWLEN), new(B * R), new(ld_out)
        dBn, dVn, dOn, dPn = new(BSPA_ROWLEN), new(R), new(ld_out), new(SPA_ROWS * R)
        at = lambda d, off: vp(d.data_ptr() + 8 * off)
        wide = (k, R, bq, vp(dSa.data_ptr()), vp(dKa.data_ptr()), vp(dXa.data_ptr()), ldw)

        def load(b):
            sub = np.ascontiguousarray(Gm[b * R:(b + 1) * R])
            dG[:sub.shape[0], :n].copy_(torch.from_numpy(sub))
            torch.cuda.synchronize()
            return sub.shape[0]

        t_wide, t_base, per_block = [], [], []
        for it in range(1 + args.blocks):
            w = dict(gram=0.0, spa=0.0, collapse=0.0, panel=0.0)
            blocks = []
            for b in range(B):                                   # the wide set, as BinaryWideSetTest queues it
                rb = load(b)
                pS = at(dSa, b * (bq + 4) * R)
                bf.scan_block_gram_dev(vp(dG.data_ptr()), ld, rb, pQ, bq, pS, at(dKa, b * R * R))
                bf.scan_spa_dev(vp(dG.data_ptr()), ld, rb, pS, *(nullp + (at(dPa, b * SPA_ROWS * R),)))
                bf.sets_collapse_dev(vp(dG.data_ptr()), ld, rb, pS, 0, None, b == 0, vp(dg.data_ptr()))
                if b > 0: bf.scan_panel_dev(rb, vp(store.data_ptr()), ldw, b * bp, at(dXa, b * R * ldw), ldw)
                if b < B - 1: bf.scan_block_keep_dev(rb, vp(store.data_ptr()), ldw, b * bp)
                bs.sync()
                spa_ms, coll_ms = bs.spa_timing(), bs.sets_spa_wide_timing()[0]
                w["gram"] += float(sum(bs.scan_timing())); w["spa"] += spa_ms; w["collapse"] += coll_ms
                if b > 0: w["panel"] += float(sum(bs.panel_timing()))
                blocks.append((coll_ms, spa_ms))
            bf.sets_spa_wide_dev(*(wide + nullp + (vp(dPa.data_ptr()), 0, None, vp(dg.data_ptr()), vp(dBw.data_ptr()), vp(dVw.data_ptr()))))
            bf.sets_finish_wide_scaled_dev(*(wide + (nullp[0], nullp[1], c, 0, None, 0, rho, vp(dOw.data_ptr()), None, vp(dVw.data_ptr()))))
            bs.sync()
            sw, fw = bs.sets_spa_wide_timing(), bs.sets_finish_wide_timing()
            base = dict(gram=0.0, spa=0.0, sets_spa=0.0, finish=0.0)
            for b in range(B):                                   # the same markers as separate narrow sets: BinarySetTest's calls
                rb = load(b)
                start = np.array([0, rb], dtype=np.int32)
                pS, pK, pP = vp(dS.data_ptr()), vp(dK.data_ptr()), vp(dPn.data_ptr())
                bf.scan_block_gram_dev(vp(dG.data_ptr()), ld, rb, pQ, bq, pS, pK)
                bf.scan_spa_dev(vp(dG.data_ptr()), ld, rb, pS, *(nullp + (pP,)))
                bf.sets_spa_dev(vp(dG.data_ptr()), ld, rb, pS, pK, *(nullp + (pP, 1, start, 0, None, vp(dBn.data_ptr()), vp(dVn.data_ptr()))))
                bf.sets_finish_scaled_dev(rb, bq, pS, pK, nullp[0], nullp[1], c, 1, start, 0, None, 0, rho, vp(dOn.data_ptr()), ld_out, None,
                                          vp(dVn.data_ptr()))
                bs.sync()
                base["gram"] += float(sum(bs.scan_timing())); base["spa"] += bs.spa_timing()
                base["sets_spa"] += bs.sets_spa_timing(); base["finish"] += bs.sets_finish_timing()
            if it >= 1:
                t_wide.append([w["gram"], w["spa"], w["collapse"], w["panel"], sw[1], sw[2], float(sum(fw))] + list(fw))
                t_base.append([base["gram"], base["spa"], base["sets_spa"], base["finish"]])
                per_block.append(blocks)
        keeps = []
        for it in range(4):                                      # the last block is still in X: 20 keeps of it behind each other
            bs.sync(); t0 = time.perf_counter()
            for _ in range(20): bf.scan_block_keep_dev(rb, vp(store.data_ptr()), ldw, 0)
            bs.sync(); keeps.append(1e3 * (time.perf_counter() - t0) / 20)
        keep_ms = float(np.median(keeps[1:])) * (B - 1)
        # the set saddlepoint once more at cutoff 0: the burden is attempted whatever its score (the row is put back every round,
        # the call overwrites it with g^_B)
        Bw2 = dBw.cpu().numpy().copy()
        g0, forced = dg.clone(), []
        for it in range(1 + args.blocks):
            dg.copy_(g0)
            bf.sets_spa_wide_dev(*(wide + nullp[:6] + (0.0, vp(dPa.data_ptr()), 0, None, vp(dg.data_ptr()), vp(dBw.data_ptr()), vp(dVw.data_ptr()))))
            bs.sync()
            if it >= 1: forced.append(bs.sets_spa_wide_timing()[1:])
        forced, Bf = np.asarray(forced), dBw.cpu().numpy().copy()
        dBw.copy_(torch.from_numpy(Bw2))
        a, bb, pb = np.asarray(t_wide), np.asarray(t_base), np.asarray(per_block)
        wide_ms = float(np.median(a[:, :7].sum(axis=1))) + keep_ms
        base_ms = float(np.median(bb.sum(axis=1)))
        Bw, hP = dBw.cpu().numpy(), dPa.cpu().numpy()
        t0 = time.perf_counter()
        out = bt(Gm, [np.arange(k)], skato=True, finish="wide")
        call_ms = 1e3 * (time.perf_counter() - t0)
        names = ("sweeps_with_gram", "marker_spa", "collapses", "panels", "sets_spa_wide_markers_pairs", "sets_spa_wide_burden", "scaled_finish")
        rec["widths"][str(k)] = {
            "sub_blocks": B, "store_bytes": int(n) * ldw * 8,
            "wide_device_ms": dict({nm: summary(a[:, i]) for i, nm in enumerate(names)}, keeps=keep_ms, total=wide_ms,
                                   scaled_finish_phases={nm: summary(a[:, 7 + i]) for i, nm in enumerate(("prep_form", "reduction", "eigenvalues", "tails"))}),
            "separate_sets_device_ms": dict({nm: summary(bb[:, i]) for i, nm in enumerate(("sweeps_with_gram", "marker_spa", "sets_spa", "scaled_finish"))},
                                            total=base_ms),
            "wide_over_separate": wide_ms / base_ms,
            "panels_and_keeps_share_of_wide": (float(np.median(a[:, 3])) + keep_ms) / wide_ms,
            "collapse_over_scan_spa_per_sub_block": [float(np.median(pb[:, b, 0]) / np.median(pb[:, b, 1])) for b in range(B)],
            "collapse_ms_per_sub_block": [float(np.median(pb[:, b, 0])) for b in range(B)],
            # (sub-block 1: r bytes of genotypes per individual, the row read and written)
            "collapse_implied_bytes_per_s": float(n) * (min(R, k - R) + 16) / (1e-3 * float(np.median(pb[:, 1, 0]))),
            "markers_saddlepointed": int(sum(np.sum(hP[b * SPA_ROWS * R:][:SPA_ROWS * min(R, k - b * R)].reshape(SPA_ROWS, -1)[6] > 0) for b in range(B))),
            "sets_spa_wide_at_cutoff_0_ms": {"markers_pairs": summary(forced[:, 0]), "burden": summary(forced[:, 1]), "burden_flag": int(Bf[6]),
                                             "iters": float(Bf[5]), "phi": float(Bf[11])},
            "burden_flag": int(Bw[6]), "n_adjusted": int(Bw[12]), "phi": float(Bw[11]), "n_used": int(out["n_used"][0]),
            "skato_p": float(out["skato_p"][0]), "whole_call_wall_ms_skato": call_ms}
        del store, dSa, dKa, dXa, dPa
    return rec


if args.finish or args.binary or args.wide or args.wide_finish or args.binary_wide:
    if args.binary_wide:
        rec = binary_wide_leg([int(v) for v in args.binary_wide.split(",")])
        print(json.dumps(rec))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(rec, open(args.out, "w"), indent=1)
        sys.exit(0)
    if args.wide_finish:
        rec = wide_finish_leg([int(v) for v in args.wide_finish.split(",")])
        print(json.dumps(rec))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(rec, open(args.out, "w"), indent=1)
        sys.exit(0)
    rec = wide_leg([int(v) for v in args.wide.split(",")]) if args.wide else binary_leg() if args.binary else finish_leg()
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rec, open(args.out, "w"), indent=1)
    sys.exit(0)


def scan():
    fac.scan_block_dev(vp(dG.data_ptr()), ld, R, vp(tester.dQ.data_ptr()), q, vp(dS.data_ptr())); sym.sync()
    return sym.scan_timing()


def gram(shape):
    if shape == "default":
        os.environ.pop("SCILMM_GRAM_SHAPE", None)
    else:
        os.environ["SCILMM_GRAM_SHAPE"] = shape
    fac.scan_block_gram_dev(vp(dG.data_ptr()), ld, R, vp(tester.dQ.data_ptr()), q, vp(dS.data_ptr()), vp(dK.data_ptr())); sym.sync()
    return sym.scan_timing()


t_scan, t_gram = [], {s: [] for s in shapes}
for it in range(3 + args.blocks):                     # three rounds of warm-up of every shape, then the timed rounds
    ms = scan()
    if it >= 3: t_scan.append(ms)
    for s in shapes:
        ms = gram(s)
        if it >= 3: t_gram[s].append(ms)
a = np.asarray(t_scan)
rec = {"workload": args.workload, "n": int(n), "nnzL": int(sym.info().nnzL), "blocks": args.blocks, "sigma2": S2, "r": R,
       "library": os.path.basename(os.environ.get("SCILMM_HIP_LIB", "libscilmm_hip.so")),
       "timer": "HIP events on the engine's stream, one block per synchronise; three warm-up rounds of every shape, then "
                "alternating rounds",
       "x_bytes": int(n) * R * 8, "hbm_streaming_read_bytes_per_s": HBM,
       "scan_block": {"prep_ms": summary(a[:, 0]), "sweep_ms": summary(a[:, 1]), "stats_ms": summary(a[:, 2]),
                      "total_ms": summary(a.sum(axis=1))},
       "gram_block": {}}
K = {}
for s in shapes:
    b = np.asarray(t_gram[s])
    extra = b[:, 2] - a[:, 2]                          # paired: the round's Gram block against the round's plain block
    g = float(np.median(extra))
    tot_s, tot_g = summary(a.sum(axis=1)), summary(b.sum(axis=1))
    over = tot_g["median"] - tot_s["median"]
    rec["gram_block"][s] = {
        "prep_ms": summary(b[:, 0]), "sweep_ms": summary(b[:, 1]), "stats_ms": summary(b[:, 2]), "total_ms": tot_g,
        "gram_plus_fold_ms": summary(extra), "ratio_to_scan_stats": g / float(np.median(a[:, 2])),
        "implied_bytes_per_s": int(n) * R * 8 / (g * 1e-3), "fraction_of_hbm_streaming_read": int(n) * R * 8 / (g * 1e-3) / HBM,
        "total_over_scan_block": tot_g["median"] / tot_s["median"],
        "excess_within_iqr_plus_gram": bool(over <= max(tot_s["iqr"], tot_g["iqr"]) + g)}
    gram(s)
    K[s] = dK.cpu().numpy().reshape(R, R).copy()
    gg = dS.cpu().numpy().reshape(q + 4, R)[3]
    rec["gram_block"][s]["diag_rel_err_vs_gg"] = float(np.abs(np.diag(K[s]) - gg).max() / np.abs(gg).max())
    rec["gram_block"][s]["symmetric_bits"] = bool(np.array_equal(K[s], K[s].T))
    rec["gram_block"][s]["max_rel_diff_vs_default"] = float(np.abs(K[s] - K["default"]).max() / np.abs(K["default"]).max())
os.environ.pop("SCILMM_GRAM_SHAPE", None)
print(json.dumps(rec))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
