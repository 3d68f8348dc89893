"""Every output double of the variant-set finish kernels (k_sets_finish, the k_wide_* chain, k_sets_spa) on a fixed seeded list of
cases, as 16-hex-digit bit patterns in a JSON file: run at two commits on the same machine, the two files are identical, NaNs
included, where the kernels compute the same thing bit for bit.  Only entry points are used, and the made-up blocks of the GPU
tests (tests/test_gpu_skato.py, tests/test_gpu_sets_wide_finish.py), so the tool runs unchanged at an older commit.
  usage: sets_bits.py OUT.json
The cases (no set wider than 300 markers):
  scilmm_sets_finish_dev, scilmm_sets_finish_scaled_dev : a block of sets of 1, 2, 3, 17 and 64 markers, a set with nothing left,
      one with a dropped marker and a rank-one set (256 threads); a block with a 65-marker set (512 threads); one 128-marker set;
  scilmm_sets_finish_wide_dev : 0, 1, 2, 3, 65 and 300 kept markers and a rank-one set, in sub-blocks of 16 and of 128;
  with no grid, one grid value and the default grid (rho = 1 in it), both tails, the three weight modes, c = 1 and 4, one change
  at a time from a base case; d_lam is given in the base case of the first narrow block and of the 65-marker wide set and null
  elsewhere (the eigenvalues feed every p-value), which keeps the file small;
  BinarySetTest(finish="device") on a cohort of 100: the result, the rows of k_sets_spa and the variance scales."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tests import test_gpu_binary_sets as GB
from tests import test_gpu_sets as GS
from tests import test_gpu_sets_wide_finish as WF
from tests import test_gpu_skato as GK

vp = C.c_void_p
RHO = GK.RHO
GRIDS = {"grid8": RHO, "grid1": np.array([0.3]), "grid0": np.empty(0)}
OUT = {}


def record(name, *arrays):
    assert name not in OUT, name
    flat = np.concatenate([np.ascontiguousarray(a, dtype=np.float64).ravel() for a in arrays])
    OUT[name] = " ".join("%016x" % v for v in flat.view(np.uint64))


def model(c):
    rng = np.random.default_rng(7 + c)
    return np.triu(0.2 * rng.standard_normal((c, c))) + np.diag(rng.uniform(1.0, 2.0, c)), 0.5 * rng.standard_normal(c)


def member(rng, k, dropped=(), rank=None, signal=0.0):
    """A made-up set of k kept markers (GK._made_up_sets' form): a positive semidefinite K, a score drawn from it."""
    K = GK._psd(rng, k, rank) if k else np.zeros((0, 0))
    ev, U = np.linalg.eigh(K) if k else (np.zeros(0), np.zeros((0, 0)))
    s = (U * np.sqrt(np.maximum(ev, 0.0))) @ rng.standard_normal(k) + signal * np.sqrt(np.diag(K))
    return ("m%d" % k, K, s, False, tuple(dropped))


def rank_one(rng, k):
    b = rng.standard_normal(k)
    return ("rank_one%d" % k, np.outer(b, b), 2.1 * b, True, ())


def narrow(fac, sym, S, G, R, u, start, mode, weights, method, rho, lam, vscale):
    """One call of scilmm_sets_finish_dev, or of scilmm_sets_finish_scaled_dev where vscale is given: the rows, then d_lam."""
    q, r, ns, ld = S.shape[0] - 4, S.shape[1], start.size - 1, GK.HEAD + len(rho)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    dS, dG, dR, du = dev(S), dev(G), dev(R), dev(u)
    dW = dev(weights) if weights is not None else None
    dO, dL = torch.zeros((ns * ld,), dtype=torch.float64, device="cuda"), torch.zeros((r,), dtype=torch.float64, device="cuda")
    args = (r, q, vp(dS.data_ptr()), vp(dG.data_ptr()), vp(dR.data_ptr()), vp(du.data_ptr()), q - 1, ns, start, mode,
            vp(dW.data_ptr()) if dW is not None else None, method, rho, vp(dO.data_ptr()), ld, vp(dL.data_ptr()) if lam else None)
    torch.cuda.synchronize()
    if vscale is None:
        fac.sets_finish_dev(*args)
    else:
        dV = dev(vscale)
        fac.sets_finish_scaled_dev(*(args + (vp(dV.data_ptr()),)))
    sym.sync()
    return dO.cpu().numpy(), dL.cpu().numpy()


def variants():
    """(label, weight mode, tail method, grid) of a case: the base, then one change at a time."""
    yield "base", 1, 0, "grid8"
    yield "liu", 1, 1, "grid8"
    yield "beta", 0, 0, "grid8"
    yield "given", 2, 0, "grid8"
    yield "grid1", 1, 0, "grid1"
    yield "grid0", 1, 0, "grid0"


def narrow_cases(fac, sym):
    for c in (4, 1):
        R, u = model(c)
        rng = np.random.default_rng(100 + c)
        blocks = {
            "small": [member(rng, 1), member(rng, 2, signal=1.0), member(rng, 3), member(rng, 17, signal=0.5), member(rng, 64),
                      member(rng, 0, dropped=(0, 1)), member(rng, 5, dropped=(2,)), rank_one(rng, 9)],
            "odd65": [member(rng, 3), member(rng, 65, signal=0.3), member(rng, 17)],
            "one128": [member(rng, 128)]}
        for name, members in blocks.items():
            S, G, start = GK._made_up_block(members, rng, R, u)
            w = rng.uniform(0.5, 2.0, S.shape[1])
            vs = rng.uniform(0.5, 2.0, S.shape[1])
            vs[::3] = 1.0
            for label, mode, method, grid in variants():
                if label != "base" and (name != "small" or (c == 1 and label != "liu")):
                    continue
                lam = label == "base" and name == "small"
                for scaled in (False, True) if label in ("base", "grid0") else (False,):
                    rows, L = narrow(fac, sym, S, G, R, u, start, mode, w if mode == 2 else None, method, GRIDS[grid], lam, vs if scaled else None)
                    record("narrow/c%d/%s/%s/%s" % (c, name, label, "scaled" if scaled else "plain"), rows, L if lam else L[:0])


def wide_cases(fac, sym):
    for c in (4, 1):
        R, u = model(c)
        rng = np.random.default_rng(200 + c)
        sets = {"m0": member(rng, 0, dropped=tuple(range(20))), "m1": member(rng, 1, dropped=(0, 2)), "m2": member(rng, 2, signal=1.0),
                "m3": member(rng, 3), "m65": member(rng, 65, dropped=(0, 40), signal=0.3), "m300": member(rng, 300), "rank_one": rank_one(rng, 33)}
        for name, m in sets.items():
            S, G, _ = GK._made_up_block([m], rng, R, u)
            w = rng.uniform(0.5, 2.0, S.shape[1])
            for label, mode, method, grid in variants():
                if (label != "base" and (name != "m65" or c == 1)) or (c == 1 and name not in ("m3", "m65")):
                    continue
                lam = label == "base" and name == "m65"
                for block in (16, 128):
                    row, L = WF._wide(fac, sym, torch, S, G, R, u, block, mode=mode, weights=w if mode == 2 else None, method=method,
                                      rho=GRIDS[grid], lam=lam)
                    record("wide/c%d/%s/%s/block%d" % (c, name, label, block), row, L if lam else L[:0])


def binary_case():
    p = GB._problem("sub100")
    tester = GB._tester(p, 4, cutoff=0.5, deterministic=True)
    dev = tester(p["G"], p["sets"], skato=True, finish="device")
    record("binary/bspa", tester.last_bspa)
    for k in sorted(dev):
        record("binary/" + k, dev[k])
    host = tester(p["G"], p["sets"], skato=True, finish="host", return_kernel=True)      # (the scales are the device's in both)
    record("binary/vscale", *[kern[3] for kern in host["kernel"] if kern is not None])


p = GS._problem("spd203")
tester = GS._tester(p, 4, 128, deterministic=True)
narrow_cases(tester.factor, tester.sym)
wide_cases(tester.factor, tester.sym)
binary_case()
with open(sys.argv[1], "w") as f:                               # a case per line: the doubles' bit patterns, separated by spaces
    f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(OUT[k])) for k in sorted(OUT)) + "\n}\n")
print("sets_bits: %d cases, %d doubles -> %s" % (len(OUT), sum(len(v.split()) for v in OUT.values()), sys.argv[1]))
