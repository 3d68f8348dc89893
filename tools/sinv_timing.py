"""Time the selected inverse (scilmm_selected_inverse + scilmm_inverse_traces) on a BASELINE workload.
usage: python tools/sinv_timing.py 100k|300k|1m [out.json] [--deterministic | --both] [--reps N] [--problem-cache A.npz]

  (no flag)        a default handle: the atomic kernels
  --deterministic  a handle in deterministic mode: the order-fixed kernels (k_sinv_tail<true> / k_sinv_cc_ordered + folds)
  --both           one handle of each in one process, inverted alternately after one warm-up inversion each: the record
                   holds both series, their medians and the ratio; the order-fixed plan's report (slot bytes) is kept too
"""
import argparse
import contextlib
import json
import os
import re
import sys
import tempfile
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, ".")
import bench
from scilmm_amd.factor import Symbolic

ORDERED = re.compile(r"selected inverse, order-fixed: tail row tiles (\d+) direct, (\d+) folded from (\d+) slots \((\d+) bytes\); "
                     r"cc segments of up to (\d+) tiles: (\d+) direct, (\d+) folded \((\d+) bytes\)")


@contextlib.contextmanager
def _stderr_text(out):
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as fh:
        os.dup2(fh.fileno(), 2)
        try:
            yield
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            fh.seek(0)
            out.append(fh.read().decode(errors="replace"))


def _one(sym, fac, s2, n, flops):
    t0 = time.time()
    tr = fac.inverse_traces()
    wall = time.time() - t0
    dev = sym.timing()["quad_ms"] / 1e3
    fac.refactorize(s2)
    return {"wall_s": wall, "device_s": dev, "tflops": 2.0 * flops / dev / 1e12, "traces": tr.tolist(),
            "trace_identity_residual": float(abs(s2 @ tr - n) / n)}


def main():
    ap = argparse.ArgumentParser(description="time the selected inverse on a BASELINE workload")
    ap.add_argument("workload", nargs="?", default="100k")
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--both", action="store_true")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--problem-cache", default=None, help="keep the cohort's matrix in this .npz between runs of the tool")
    a = ap.parse_args()
    name, out, reps = a.workload, a.out, a.reps
    modes = [False, True] if a.both else [True] if a.deterministic else [False]
    if a.problem_cache and os.path.exists(a.problem_cache):
        A = sp.load_npz(a.problem_cache)
    else:
        A, C, y = bench.build_problem(name, 0)
        if a.problem_cache:
            sp.save_npz(a.problem_cache, A, compressed=False)
    n = A.shape[0]
    s2 = np.array([0.4, 0.6])
    rec = {"workload": name, "n": n}
    handles = []
    for det in modes:
        sym = Symbolic([A, sp.identity(n, format="csr")], deterministic=det)
        info = sym.info()
        fac = sym.factorize(s2)
        rec.update(nnzL=int(info.nnzL), factor_flops=info.flops)
        key = "deterministic" if det else "default"
        rec[key] = {"factor_s": sym.timing()["factor_ms"] / 1e3, "runs": []}
        # the warm-up inversion builds the plan; its report says what the order-fixed form stores where
        text = []
        os.environ["SCILMM_VERBOSE"] = "1"
        with _stderr_text(text):
            rec[key]["warmup"] = _one(sym, fac, s2, n, info.flops)
        del os.environ["SCILMM_VERBOSE"]
        m = ORDERED.search(text[0])
        if m:
            rec[key]["plan"] = dict(zip(("tail_tiles_direct", "tail_tiles_folded", "tail_slots", "tail_slot_bytes", "cc_tiles_per_segment",
                                         "cc_segments_direct", "cc_segments_folded", "cc_slot_bytes"), map(int, m.groups())))
        handles.append((key, sym, fac, info.flops))
    for rep in range(reps):
        for key, sym, fac, flops in handles:  # alternated
            rec[key]["runs"].append(_one(sym, fac, s2, n, flops))
    for key, sym, fac, flops in handles:
        dev = sorted(r["device_s"] for r in rec[key]["runs"])
        rec[key]["device_s_median"] = dev[len(dev) // 2]
        rec[key]["device_s_min_max"] = [dev[0], dev[-1]]
        rec[key]["n_float_atomic_launches"] = int(sym.timing()["n_float_atomic_launches"])
    if len(handles) == 2:
        rec["deterministic_over_default"] = rec["deterministic"]["device_s_median"] / rec["default"]["device_s_median"]
    print(json.dumps(rec))
    if out:
        json.dump(rec, open(out, "w"), indent=1)


if __name__ == "__main__":
    main()
